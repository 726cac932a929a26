"""The four hand-tiled point models (csrc/svdpp.hip, delf.hip, caser.hip, sasrec.hip) at the edges of their own loops
(tests/point_edge_cases.py: widths that do not divide the workgroup, lengths on a chunk seam, second trips of the strided loops,
the widest rows on either side, one window past a sweep, an exact tie of the window maximum, saturated keys, the LDS bound from
the inside).  Per case: a. one forward + backward through the model's own _pass, checked by the model's own _check against its
float64 restatement (loss 2e-5 relative to max(1, |loss|), y 1e-4, saved arrays and every gradient rtol 2e-4 / atol 2e-6), row 0
of the table's gradient exactly zero; b. the same pass on a fresh model gives the same bits (the kernels promise fixed-order
sums: an idle thread leaking into a reduction would show here first); c. two train() steps against the restatement's RefModel
(the second step's loss is what checks the first step's backward pass and update), then eval() on the whole batch.
tests/test_point_edge_cases_cpu.py judges the same inputs on the restatements alone."""
import numpy as np
import pytest
import torch

import point_edge_cases as pe
import test_gpu_caser as on_caser
import test_gpu_delf as on_delf
import test_gpu_sasrec as on_sasrec
import test_gpu_svdpp as on_svdpp
from test_gpu_model import close

pytestmark = pytest.mark.gpu

ON_GPU = {"svdpp": on_svdpp, "delf": on_delf, "caser": on_caser, "sasrec": on_sasrec}
_ORACLE = {}


def _oracle(name):
    """the restatement's float64 pass over a case (reg_lambda 0): computed once, never written to"""
    if name not in _ORACLE:
        k = pe.case(name)
        _ORACLE[name] = k.ref.loss_and_grads(k.c, k.P, k.batch, 0.0)
    return _ORACLE[name]


def _same_bits(g1, g2, name):
    assert set(g1) == set(g2)
    for f in g1:
        if f == "grads":
            for v in g1[f]:
                assert np.array_equal(g1[f][v], g2[f][v]), (name, v)
        else:
            assert np.array_equal(np.asarray(g1[f]), np.asarray(g2[f])), (name, f)


def _train_steps(mod, k, name):
    """two TF-Adam steps against the restatement's (train() returns the loss of the forward pass BEFORE its update), then the
    predictions on the whole batch (a forward pass is continuous at the kinks)"""
    bt = k.ref.batch_tuple
    m, ref = mod._model(k.c, k.P), k.ref.RefModel(k.c, k.P)
    for step in range(2):
        lg = m.train(None, bt(k.batch), 1e-3, 1e-4, keep_prob=1.0)
        lo = ref.train(None, bt(k.batch), 1e-3, 1e-4, keep_prob=1.0)
        print("%s: Adam step %d: loss %.7f, restatement %.7f" % (name, step, lg, lo))
        assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo)), (name, step, lg, lo)
    pg, lab, _ = m.eval(None, bt(k.batch_all), 1e-4)
    po, lab_o, _ = ref.eval(None, bt(k.batch_all), 1e-4)
    torch.cuda.synchronize()
    assert lab == lab_o
    err = float(np.abs(np.asarray(pg) - np.asarray(po)).max())
    print("%s: eval after two steps, max |dy| %.2e" % (name, err))
    assert err < 1e-4, (name, err)


@pytest.mark.parametrize("name", list(pe.CASES))
def test_edge_case_against_restatement_twice_and_trained(name):
    k = pe.case(name)
    mod, c, P, b = ON_GPU[k.row.model], k.c, k.P, k.batch
    D, T, Fu, Fi, B = k.row.shape
    out, go = _oracle(name)
    print("%s: kept %d of %d" % (name, k.kept.size, B))
    # a. against the restatement in float64
    got = mod._pass(c, P, b)
    errs = {v: close(got["grads"][v], go[v], rtol=2e-4, atol=2e-6)[1] for v in go}
    worst = max(errs, key=errs.get)
    print("%s: worst gradient error %.2e (%s)" % (name, errs[worst], worst))
    if k.row.model == "svdpp":
        mod._check(got, out, go, name, Fu + Fi)
    else:
        mod._check(got, out, go, name)
    assert np.abs(go["emb_mtx"]).max() > 0 and not got["grads"]["emb_mtx"][0].any()
    assert np.isfinite(got["loss"]) and all(np.isfinite(v).all() for v in got["grads"].values())
    if k.row.model == "delf":
        # masked positions weigh exactly 0; a length <= 0 is exactly uniform (tests/test_gpu_delf.py)
        for a, ln in ((got["att_user"], b["user_seq_length"]), (got["att_item"], b["item_seq_length"])):
            for i in range(len(ln)):
                if ln[i] <= 0:
                    assert np.array_equal(a[i], np.full(T, np.float32(1.0) / np.float32(T))), (name, i)
                else:
                    assert not a[i, min(int(ln[i]), T):].any(), (name, i)
    if name == "delf_t257":
        assert b["user_seq_length"][2] == 0          # (the uniform row above was there)
    if name == "caser_zero_history":
        # the exact tie: every window sum of the sample is bh, bit for bit, and the first position keeps the maximum
        z = pe.ZERO_HISTORY_SAMPLE
        assert np.unique(got["hwin"][z]).size == 1 and got["arg"][z] == 0 == out["arg"][z]
    if k.row.model == "caser":
        assert np.array_equal(got["arg"], out["arg"])
    # b. a fresh model, the same bits
    _same_bits(got, mod._pass(c, P, b), name)
    # c. optimizer steps
    _train_steps(mod, k, name)
    torch.cuda.synchronize()
