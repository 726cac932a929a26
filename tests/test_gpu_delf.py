"""The DELF point baseline (point_model.py:200-249) on the GPU against its float64 restatement (tests/delf_ref.py): the pass,
both attention-weight arrays, both attention outputs, every gradient and the training trajectory; the two length tensors
(longer than T, zero, and short enough that only the leading slices are computed); and the step's other forms -- single stream,
time-tiled optimizer, captured graph, the three feed forms, the restated dual-sequence loader, checkpoints, bad ids,
device-side evaluation -- against the plain eager step.

Tolerances are those of tests/test_gpu_caser.py: loss 2e-5 relative, y 1e-4, arrays and gradients rtol 2e-4 / atol 2e-6."""
import pickle

import numpy as np
import pytest
import torch

import delf_cases as dc
import delf_ref as dr
from delf_ref import batch_tuple
from test_gpu_gru4rec import _same_state
from test_gpu_model import close

pytestmark = pytest.mark.gpu

TMALL = dc.TMALL
_batches = dc.batches


def _model(c, P, flags=0, **kw):
    from score_amd.model import DELF
    m = DELF(*c.args, **kw)
    m.set_params(P)
    m.debug_flags = flags
    return m


def _pass(c, P, b, flags=0, reg=0.0, model=None, skip=True):
    """one forward + backward -> loss, y_pred, attention weights and outputs of both sides, every gradient"""
    from score_amd import _lib
    m = model if model is not None else _model(c, P, flags)
    m.skip_masked_slices = skip
    B = len(b["label"])
    db = m.device_batch(batch_tuple(b))
    TA = db.active_slices or c.T
    lay, ws = m.forward_backward(db, reg, 1.0)
    att, rep = _lib.workspace_field(m.cfg, B, "delf_att"), _lib.workspace_field(m.cfg, B, "delf_rep")
    full = lambda a: np.concatenate([a, np.zeros((B, c.T - TA), a.dtype)], 1)        # (slices not computed: weight 0)
    return dict(loss=float(ws[lay.loss].item()), y=ws[lay.y_pred:lay.y_pred + B].cpu().numpy().copy(),
                att_user=full(ws[att[0]:att[0] + B * TA].view(B, TA).cpu().numpy().copy()),
                att_item=full(ws[att[1]:att[1] + B * TA].view(B, TA).cpu().numpy().copy()),
                ru=ws[rep[0]:rep[0] + B * c.Ci].view(B, c.Ci).cpu().numpy().copy(),
                ri=ws[rep[1]:rep[1] + B * c.Cu].view(B, c.Cu).cpu().numpy().copy(), grads=m.get_grads(), active=db.active_slices)


def _check(got, out, want_g, what):
    want_loss, want_y = float(out["loss"].detach()), out["y_pred"].detach().numpy()
    print(what, "loss", got["loss"], want_loss, "max |dy|", float(np.abs(got["y"] - want_y).max()))
    assert abs(got["loss"] - want_loss) < 2e-5 * max(1.0, abs(want_loss)), (what, got["loss"], want_loss)
    assert np.abs(got["y"] - want_y).max() < 1e-4, what
    for k in ("att_user", "att_item", "ru", "ri"):
        ok, err = close(got[k], out[k].detach().numpy(), rtol=2e-4, atol=2e-6)
        print(what, k, err)
        assert ok, (what, k, err)
    assert set(got["grads"]) == set(want_g)
    for k in want_g:
        assert got["grads"][k].shape == want_g[k].shape, (what, k, got["grads"][k].shape)
        ok, err = close(got["grads"][k], want_g[k], rtol=2e-4, atol=2e-6)
        print(what, k, err)
        assert ok, (what, k, err)


@pytest.mark.parametrize("D,T,Fu,Fi,B", list(dc.SHAPES))
def test_forward_backward_against_restatement(D, T, Fu, Fi, B):
    c, P, b, kept = dc.case(D, T, Fu, Fi, B)
    print("kept", kept.size, "of", B)
    out, go = dr.loss_and_grads(c, P, b, 0.0)
    got = _pass(c, P, b)
    _check(got, out, go, "delf")
    assert np.abs(go["emb_mtx"]).max() > 0 and not got["grads"]["emb_mtx"][0].any()
    # masked positions weigh exactly 0; a length <= 0 is exactly uniform
    for a, ln in ((got["att_user"], b["user_seq_length"]), (got["att_item"], b["item_seq_length"])):
        for i in range(len(ln)):
            if ln[i] <= 0:
                assert np.array_equal(a[i], np.full(T, np.float32(1.0) / np.float32(T)))
            else:
                assert not a[i, min(int(ln[i]), T):].any()
    if (D, T, Fu, Fi, B) == (16, 7, 3, 4, 33):
        # every length <= 5: only the leading slices were computed; all T computed gives the same loss and gradients
        assert got["active"] == int(max(b["user_seq_length"].max(), b["item_seq_length"].max())) < T
        allT = _pass(c, P, b, skip=False)
        assert allT["active"] == 0
        _check(allT, out, go, "delf, all slices")
        assert abs(allT["loss"] - got["loss"]) < 2e-5 * max(1.0, abs(got["loss"]))
        for k in go:
            ok, err = close(allT["grads"][k], got["grads"][k], rtol=2e-4, atol=2e-6)
            assert ok, (k, err)
    else:
        assert got["active"] == 0


def test_a_zero_length_makes_the_batch_compute_every_slice():
    c = dr.Cfg(500, 8, 32, 9, 2, 1)
    P = dr.init_params(c, 3, bias_scale=0.1)
    b = _batches(c, 6, 1, 4, max_length=(4, 4))[0]
    m = _model(c, P)
    assert m.device_batch(batch_tuple(b)).active_slices == 4
    for arrays in (batch_tuple(dict(b, item_seq_length=np.array([1, 2, 0, 3, 4, 1], dtype=np.int32))),):
        for feed in (arrays, tuple(torch.as_tensor(a).cuda() for a in arrays)):
            assert m.device_batch(feed).active_slices == 0
    b0 = dict(b, user_seq_length=np.array([0, 2, 3, 1, 4, 2], dtype=np.int32))
    out, go = dr.loss_and_grads(c, P, b0, 0.0)
    _check(_pass(c, P, b0), out, go, "zero length")


def test_two_fresh_models_give_the_same_bits():
    """every sum over the batch or over T is taken in a fixed order (csrc/delf.hip, the queued products): no result depends on
    how the workgroups ran"""
    c, P, b, _ = dc.case(16, 7, 3, 4, 33)
    big = _batches(dr.Cfg(3000, *TMALL), 200, 1, 5)[0]
    for cc, bb in ((c, b), (dr.Cfg(3000, *TMALL), big)):
        PP = dr.init_params(cc, 3)
        g1, g2 = _pass(cc, PP, bb), _pass(cc, PP, bb)
        assert g1["loss"] == g2["loss"] and np.array_equal(g1["y"], g2["y"])
        for k in ("att_user", "att_item", "ru", "ri"):
            assert np.array_equal(g1[k], g2[k]), k
        for k in g1["grads"]:
            assert np.array_equal(g1["grads"][k], g2["grads"][k]), k


def test_ten_train_steps_against_restatement_and_adam():
    c = dr.Cfg(20011, *TMALL)
    P = dr.init_params(c, 4)
    m, ref = _model(c, P), dr.RefModel(c, P)
    bs = _batches(c, 200, 5, 8)
    for step in range(10):
        b = batch_tuple(bs[step % len(bs)])
        lg = m.train(None, b, 1e-3, 1e-4, keep_prob=1.0)
        lo = ref.train(None, b, 1e-3, 1e-4, keep_prob=1.0)
        print(step, lg, lo)
        assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo)), (step, lg, lo)
    pg, lab, _ = m.eval(None, batch_tuple(bs[0]), 1e-4)
    po, lab_o, _ = ref.eval(None, batch_tuple(bs[0]), 1e-4)
    assert lab == lab_o
    assert np.abs(np.asarray(pg) - np.asarray(po)).max() < 1e-4


def test_keep_prob_has_no_effect():
    c = dr.Cfg(3001, *TMALL)
    P = dr.init_params(c, 4)
    a, b = _model(c, P), _model(c, P)
    for bt in _batches(c, 100, 2, 3):
        assert a.train(None, batch_tuple(bt), 1e-3, 1e-4, keep_prob=0.8) == b.train(None, batch_tuple(bt), 1e-3, 1e-4, keep_prob=1.0)
    assert _same_state(a, b)


def test_single_stream_gives_the_same_bits():
    """debug_flags bit 12: no second stream anywhere."""
    c = dr.Cfg(5003, *TMALL)
    P = dr.init_params(c, 6)
    a, b = _model(c, P), _model(c, P, 4096)
    for bt in _batches(c, 200, 3, 7):
        assert a.train(None, batch_tuple(bt), 1e-3, 1e-4) == b.train(None, batch_tuple(bt), 1e-3, 1e-4)
    assert _same_state(a, b)


def test_time_tiled_optimizer_equals_the_sweep():
    c = dr.Cfg(6007, *TMALL)
    P = dr.init_params(c, 7)
    tiled, swept = _model(c, P), _model(c, P)
    for m, win in ((tiled, 24), (swept, 0)):
        m.adam_tiled_min_bytes = 0
        m.adam_window = win
    bs = _batches(c, 200, 6, 9)
    for step in range(30):
        bt = batch_tuple(bs[step % len(bs)])
        assert tiled.train(None, bt, 1e-3, 1e-4, keep_prob=1.0) == swept.train(None, bt, 1e-3, 1e-4, keep_prob=1.0), step
    assert np.array_equal(tiled.get_params()["emb_mtx"], swept.get_params()["emb_mtx"])
    assert torch.equal(tiled.w, swept.w)


def test_captured_step_is_bit_identical_to_eager():
    c = dr.Cfg(4001, *TMALL)
    P = dr.init_params(c, 4)
    eager, graphed = _model(c, P, seed=77), _model(c, P, seed=77)
    graphed.enable_graph(True)
    rng = np.random.default_rng(1)
    kw = dict(max_length=(3 * c.T, 3 * c.T))
    bs = [dr.random_batch(rng, c, 200, **kw) for _ in range(5)]
    other = dr.random_batch(rng, c, 100, **kw)
    seq = [bs[0], bs[1], bs[2], other, bs[3], other, bs[4], other, bs[0]]
    for i, b in enumerate(seq):
        le = eager.train(None, batch_tuple(b), 1e-3, 1e-4)
        lg = graphed.train(None, batch_tuple(b), 1e-3, 1e-4)
        assert le == lg, (i, le, lg)
    assert len([v for v in graphed._graphs.values() if isinstance(v, tuple)]) == 2
    assert _same_state(eager, graphed)
    pe, _, _ = eager.eval(None, batch_tuple(bs[1]), 1e-4)
    pg, _, _ = graphed.eval(None, batch_tuple(bs[1]), 1e-4)
    assert pe == pg


def test_lists_arrays_and_device_tensors_feed_the_same_batch():
    c = dr.Cfg(3001, 16, 32, 52, 3, 4)
    P = dr.init_params(c, 5)
    ms = [_model(c, P) for _ in range(3)]
    for b in _batches(c, 64, 3, 12, max_length=(150, 150)):
        arrays = batch_tuple(b)
        lists = tuple(a.tolist() for a in arrays)                  # what the reference's loader yields
        device = tuple(torch.as_tensor(a).cuda() for a in arrays)
        losses = [m.train(None, f, 1e-3, 1e-4, keep_prob=1.0) for m, f in zip(ms, (arrays, lists, device))]
        assert losses[0] == losses[1] == losses[2]
    assert _same_state(ms[0], ms[1]) and _same_state(ms[0], ms[2])
    db = ms[0].device_batch(batch_tuple(b))
    assert len(db.tensors) == 9 and np.array_equal(db.tensors[8].cpu().numpy(), b["item_seq_length"])
    assert np.array_equal(db.tensors[2].cpu().numpy().reshape(b["item_seq"].shape), b["item_seq"])
    # shape errors name the field of the 7-tuple
    for field, pos in (("item_seq_length", 3), ("item_seq", 2), ("user_seq_length", 1)):
        with pytest.raises(ValueError) as ei:
            ms[0].device_batch(batch_tuple(dict(b, **{field: b[field][:-1]})))
        assert "batch_data[%d] (%s)" % (pos, field) in str(ei.value)
    with pytest.raises(ValueError):
        ms[0].device_batch(batch_tuple(b)[:5])


def _write_dual_files(d, rng, lines, T, Fu, Fi):
    """synthetic target / user-history / item-history / feature-dictionary files; -> (paths, feature_size)"""
    U, I = 40, 90
    users, items = np.arange(1, U + 1), np.arange(U + 1, U + I + 1)
    nfeat = 25
    N = U + I + 1 + nfeat
    with open(str(d / "target.txt"), "w") as ft, open(str(d / "hist.txt"), "w") as fh, open(str(d / "ihist.txt"), "w") as fi:
        for _ in range(lines):
            ft.write("%d,%s\n" % (rng.choice(users), ",".join(str(x) for x in rng.choice(items, 2, replace=False))))
            fh.write(",".join(str(x) for x in rng.choice(items, int(rng.integers(1, 3 * T)))) + "\n")
            fi.write("\t".join(",".join(str(x) for x in rng.choice(users, int(rng.integers(1, 3 * T)))) for _ in range(2)) + "\n")
    uf = {str(u): [int(x) for x in rng.integers(U + I + 1, N, Fu - 1)] for u in users}
    itf = {str(i): [int(x) for x in rng.integers(U + I + 1, N, Fi - 1)] for i in items}
    for name, dct in (("uf.pkl", uf), ("if.pkl", itf)):
        with open(str(d / name), "wb") as f:
            pickle.dump(dct, f)
    return (str(d / "target.txt"), str(d / "hist.txt"), str(d / "ihist.txt"), str(d / "uf.pkl"), str(d / "if.pkl")), N


def test_forty_steps_through_the_dual_loader_and_feed(tmp_path):
    from score_amd.pointdata import DataLoaderDualSeq
    T, Fu, Fi, B = 12, 2, 3, 32
    (tf, hf, ihf, uf, itf), N = _write_dual_files(tmp_path, np.random.default_rng(31), 16 * 5 + 3, T, Fu, Fi)
    c = dr.Cfg(N, 16, 32, T, Fu, Fi)
    P = dr.init_params(c, 3)
    m, ref = _model(c, P), dr.RefModel(c, P)
    batches = list(DataLoaderDualSeq(B, T, tf, hf, ihf, 1, uf, itf))
    assert len(batches) == 5 and batches[0][0].shape == (B, T, Fi) and batches[0][2].shape == (B, T, Fu)
    assert int(max(b[1].max() for b in batches)) > T and int(max(b[3].max() for b in batches)) > T
    assert int(min(b[1].min() for b in batches)) < T and int(min(b[3].min() for b in batches)) < T
    step = 0
    for db, host in zip(m.feed(batches * 8), batches * 8):
        lg = m.train(None, db, 1e-3, 1e-4, keep_prob=1.0)
        lo = ref.train(None, host, 1e-3, 1e-4, keep_prob=1.0)
        assert abs(lg - lo) < 1e-3 * max(abs(lo), 1e-6), (step, lg, lo)
        step += 1
    assert step == 40
    print("last losses", lg, lo)


def test_save_restore_roundtrip(tmp_path):
    c = dr.Cfg(3001, *TMALL)
    P = dr.init_params(c, 8)
    m = _model(c, P)
    bs = _batches(c, 50, 3, 2)
    for b in bs[:2]:
        m.train(None, batch_tuple(b), 1e-3, 1e-4)
    m.save(None, str(tmp_path / "delf"))
    z = np.load(str(tmp_path / "delf") + ".npz")
    spec = {s[0]: s[1] for s in dr.param_spec(c)}
    spec["emb_mtx"] = (c.N, c.D)
    names = set(spec)
    assert set(z.files) == names | {n + s for n in names for s in ("/Adam", "/Adam_1")} | {"beta1_power", "beta2_power", "global_step"}
    for n in names:
        for s in ("", "/Adam", "/Adam_1"):
            assert z[n + s].shape == spec[n], (n + s, z[n + s].shape)
    m2 = _model(c, dr.init_params(c, 99))
    m2.restore(None, str(tmp_path / "delf"))
    assert _same_state(m, m2)
    assert m.eval(None, batch_tuple(bs[2]), 1e-4) == m2.eval(None, batch_tuple(bs[2]), 1e-4)
    assert set(m2.get_params()) == names
    assert m.train(None, batch_tuple(bs[2]), 1e-3, 1e-4) == m2.train(None, batch_tuple(bs[2]), 1e-3, 1e-4)


@pytest.mark.parametrize("field,where,named", [("item_seq", (1, 2, 0), "batch_data[2] (item_seq)"),
                                               ("user_seq", (1, 2, 0), "batch_data[0] (user_seq)"),
                                               ("target_item", (0, 1), "batch_data[5] (target_item)"),
                                               ("target_user", (3, 0), "batch_data[4] (target_user)")])
def test_bad_id_raises_and_the_model_trains_on(field, where, named):
    c = dr.Cfg(2003, 16, 32, 50, 3, 4)
    P = dr.init_params(c, 2)
    m, clean = _model(c, P), _model(c, P)
    good = _batches(c, 8, 1, 3)[0]
    bad = {k: v.copy() for k, v in good.items()}
    bad[field][where] = c.N + 7
    with pytest.raises(ValueError) as ei:
        m.train(None, batch_tuple(bad), 1e-3, 1e-4)
    assert named in str(ei.value), str(ei.value)
    assert _same_state(m, clean) and m.step == clean.step == 0          # no variable, slot or beta power was changed
    assert m.beta1_power == clean.beta1_power and m.beta2_power == clean.beta2_power
    assert m.train(None, batch_tuple(good), 1e-3, 1e-4) == clean.train(None, batch_tuple(good), 1e-3, 1e-4)
    assert _same_state(m, clean)


def test_evaluate_device_equals_host_evaluate():
    from score_amd import harness as h
    c = dr.Cfg(4001, *TMALL)
    m = _model(c, dr.init_params(c, 3, bias_scale=0.1))
    neg, lines = 99, 4
    batches = []
    for i in range(2):
        b = _batches(c, lines * (neg + 1), 1, 40 + i)[0]
        b["label"] = (np.arange(lines * (neg + 1)) % (neg + 1) == 0).astype(np.int32)     # one positive per line
        batches.append(batch_tuple(b))
    host = h.evaluate(m, [tuple(a.tolist() for a in b) for b in batches], 1e-4, neg_sample_num=neg)
    dev = h.evaluate_device(m, batches, 1e-4, neg_sample_num=neg)
    assert np.allclose(host, dev, rtol=1e-5, atol=2e-6)
    assert m.target_item_field == 5 and np.array_equal(m.device_batch(batches[0]).tensors[5].cpu().numpy(), batches[0][5])
