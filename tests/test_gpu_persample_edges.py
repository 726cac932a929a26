"""The per-sample whole-model kernels (csrc/persample.h, ps_fwd.hip, ps_bwd.hip) at the edges of what ps_plan_shape admits
(tests/persample_cases.py: every <KMAX, MT> instance, I up to 192 -- the third column tile of backward phase 8, the last k chunks
of the forward projections and of fc1 --, gather groups of 1 to 64 lanes, full and one-row row tiles, Tidx != A, PS_MAX_B and the
LDS bound from both sides, lengths above T and all zero): the form each shape takes,
the forms against each other with the bounds of tests/test_gpu_persample.py, and the per-sample form against the float64 oracle.
tests/test_persample_cases_cpu.py judges the same inputs on the oracle alone."""
import numpy as np
import pytest
import torch

from oracle import score_oracle as so
from helpers import batch_tuple
from test_gpu_model import make_model, close, LOGIT_TOL
from test_gpu_persample import _run
import persample_cases as pc

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle(name):
    """loss, predictions and every gradient of a case in float64 (reg_lambda 0), computed once"""
    if name not in _ORACLE:
        c = pc.case(name)
        oo, go = so.loss_and_grads(c.cfg, c.P, c.batch, 0.0, dtype=torch.float64)
        _ORACLE[name] = (float(oo["loss"].detach()), oo["y_pred"].detach().numpy(), go)
    return _ORACLE[name]


def _active(c):
    a = pc.computed_slices(c.row)
    return 0 if a >= c.cfg.T else a


def _same_bits(x, y):
    return torch.equal(x[0], y[0]) and x[1] == y[1] and torch.equal(x[2], y[2]) and torch.equal(x[3], y[3])


def _forms_agree(m, c, name):
    """flags 0 / 1024 / 2048 (per-sample, per-sample forward only, per-sample backward only) against 512 (layer by layer): the
    assertions and bounds of test_gpu_persample.py::_forms_and_oracle"""
    b = c.batch
    ref = _run(m, b, 512)
    for flags in (0, 1024, 2048):
        got = _run(m, b, flags)
        dy, dl = float((got[0] - ref[0]).abs().max()), abs(got[1] - ref[1])
        errs = {}
        for e in m.entries:
            errs[e[0]] = close(m._view(got[2], e).cpu().numpy(), m._view(ref[2], e).cpu().numpy(), rtol=3e-5, atol=3e-8)
        errs["emb_mtx"] = close(got[3].cpu().numpy(), ref[3].cpu().numpy(), rtol=3e-5, atol=3e-8)
        print("%s flags %d vs 512: |dy| %.2e, |dloss| %.2e, worst gradient %.2e" % (name, flags, dy, dl, max(v[1] for v in errs.values())))
        assert dy < 2e-6, flags
        assert dl < 2e-6 * max(1.0, abs(ref[1])), flags
        for k, (ok, err) in errs.items():
            assert ok, (flags, k, err)


def _against_oracle(m, c, name, flags):
    """loss, predictions, every gradient of one form against the float64 oracle; returns the gradients"""
    want_loss, want_y, go = _oracle(name)
    b, Bk = c.batch, c.batch["label"].shape[0]
    m.debug_flags = flags
    lay, ws = m.forward_backward(batch_tuple(b), 0.0, 1.0)
    torch.cuda.synchronize()
    loss, y = float(ws[lay.loss].item()), ws[lay.y_pred:lay.y_pred + Bk].cpu().numpy()
    g = m.get_grads()
    m.debug_flags = 0
    dl, dy = abs(loss - want_loss), float(np.abs(y - want_y).max())
    print("%s flags %d vs float64: |dloss| %.2e, |dy| %.2e" % (name, flags, dl, dy))
    res = {}
    for k in go:
        res[k] = close(g[k].reshape(np.asarray(go[k]).shape), go[k], rtol=2e-4, atol=2e-6)
        print("    %-44s %.2e" % (k, res[k][1]))
    assert dl < 2e-5 * max(1.0, abs(want_loss)), (loss, want_loss)
    assert dy < LOGIT_TOL
    for k, (ok, err) in res.items():
        assert np.isfinite(g[k]).all(), k
        assert ok, (flags, k, err)
    assert np.all(g["emb_mtx"][0] == 0)
    return g


def _adam_steps(m, c):
    """two TF-Adam steps against the oracle's (train() returns the loss of the forward pass BEFORE its update: the second step's
    loss is what checks the first step's backward pass and update), then the predictions on the whole batch (a forward pass is
    continuous at the kinks) -- as test_gpu_persample.py::_forms_and_oracle; nothing is left in flight behind the test"""
    cfg = c.cfg
    om = so.OracleModel(cfg.N, cfg.D, cfg.H, cfg.T, cfg.K, cfg.Fu, cfg.Fi, cfg.model_type, params={k: v.copy() for k, v in c.P.items()})
    for step in range(2):
        lg = m.train(None, batch_tuple(c.batch), 1e-3, 1e-4, keep_prob=1.0)
        lo = om.train(None, batch_tuple(c.batch), 1e-3, 1e-4, keep_prob=1.0)
        print("    Adam step %d: loss %.7f, oracle %.7f" % (step, lg, lo))
        assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo)), (step, lg, lo)
    pg, _, _ = m.eval(None, batch_tuple(c.batch_all), 1e-4)
    po, _, _ = om.eval(None, batch_tuple(c.batch_all), 1e-4)
    torch.cuda.synchronize()
    assert np.abs(np.asarray(pg) - np.asarray(po)).max() < LOGIT_TOL


@pytest.mark.parametrize("name", pc.PERSAMPLE)
def test_edge_case_takes_the_kernels_and_matches_both_references(name):
    c = pc.case(name)
    b, Bk = c.batch, c.batch["label"].shape[0]
    m = make_model(c.cfg, c.P)
    # a. the form
    assert m.device_batch(batch_tuple(b)).active_slices == _active(c)
    assert m.persample_form(Bk, _active(c)) is True
    # b. the forms against each other
    _forms_agree(m, c, name)
    # c. against the oracle in float64: the layer-by-layer pass (pinned independently: what a wider bound would be derived from)
    # and the per-sample form, then optimizer steps
    _against_oracle(m, c, name, 512)
    g = _against_oracle(m, c, name, 0)
    if name == "all_lengths_zero":
        # d. nothing reaches the recurrences (dynamic_rnn: zero outputs, and the softmax over an all-masked row passes no gradient
        # on): exact zeros where the oracle's are -- with the ONE slice a batch of zero lengths computes, and with all T computed
        # (the softmax is then uniform over T: att_score = 1 / T times zero states, through the oracle comparison)
        go = _oracle(name)[2]
        m_all = make_model(c.cfg, c.P)
        m_all.skip_masked_slices = False
        assert m_all.device_batch(batch_tuple(b)).active_slices == 0 and m_all.persample_form(Bk, 0) is True
        g_all = _against_oracle(m_all, c, name, 0)
        rec = [k for k in go if "gru_cell" in k]
        assert len(rec) == 8
        for k in rec:
            assert np.all(go[k] == 0)
            assert np.all(g[k] == 0) and np.all(g_all[k] == 0), k
    if name == "lengths_over_T":
        # e. min(length, A) in the kernels: the lengths clipped to T on the host give the same bits
        clipped = dict(b, length=np.minimum(b["length"], c.cfg.T).astype(np.int32))
        assert int((clipped["length"] != b["length"]).sum()) >= 3
        assert _same_bits(_run(m, b, 0), _run(m, clipped, 0))
    if name in ("gs64_k7_a48", "smallest"):
        # f. the slab sums of the co-attention's dW and the row scatter are fixed-order: two runs, the same bits
        r0, r1 = _run(m, b, 0), _run(m, b, 0)
        assert torch.equal(r0[2], r1[2]) and torch.equal(r0[3], r1[3])
    if name != "b512":      # (there the pass comparison is the point)
        _adam_steps(m, c)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", pc.LAYERED)
def test_one_past_the_bound_takes_the_layered_pass(name):
    """PS_MAX_B + 1 samples, and the first K whose backward LDS layout is over ps_plan_shape's 150 KiB at A = 48, I = 192 (128 bytes
    over): not the kernels' -- the runs with and without debug_flags bit 9 are the same pass, bit for bit"""
    c = pc.case(name)
    b, Bk = c.batch, c.batch["label"].shape[0]
    m = make_model(c.cfg, c.P)
    assert m.device_batch(batch_tuple(b)).active_slices == _active(c)
    assert m.persample_form(Bk, _active(c)) is False
    a0, a1 = _run(m, b, 0), _run(m, b, 512)
    assert _same_bits(a0, a1)
    assert np.isfinite(a0[1]) and bool(torch.isfinite(a0[2]).all()) and bool(torch.isfinite(a0[3]).all())
