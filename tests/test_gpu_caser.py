"""The Caser point baseline (point_model.py:140-164) on the GPU against its float64 restatement (tests/caser_ref.py): the pass,
its saved window sums / chosen positions / vertical sums, every gradient and the training trajectory; the padded head input's
pad rows; the length tensor that the model does not read; and the step's other forms -- single stream, time-tiled optimizer,
captured graph, the three feed forms, checkpoints, bad ids, device-side evaluation -- against the plain eager step."""
import numpy as np
import pytest
import torch

import caser_ref as cr
from caser_ref import batch_tuple
from test_gpu_gru4rec import _same_state, _write_point_files
from test_gpu_model import close

pytestmark = pytest.mark.gpu

TMALL = (16, 32, 50, 3, 4)          # D, H, T, Fu, Fi of the reference's point-model run (train_time_point_models.py:15-35)

# (D, T, Fu, Fi, B) -> the seed of its batch.  C = Fi * D: 4 (below a wave; one window, one sample) | two windows | Tmall | CCMR
# (C = 80: no power of two) | Taobao | eight windows, ragged batch | C = 320 (above the 256-thread workgroup: two column blocks)
# | 71 windows (nine sweeps of eight).  The seeds of the shapes with more than one window are the first ones whose batch chooses
# more than one position (tests/test_caser_cpu.py proves that, and the kink filter's cap, on the restatement alone).
SHAPES = {(4, 50, 1, 1, 1): 0, (4, 51, 2, 1, 3): 0, (16, 50, 3, 4, 200): 0, (16, 50, 1, 5, 100): 0, (16, 50, 1, 2, 100): 0,
          (16, 57, 3, 4, 33): 0, (64, 50, 3, 5, 17): 0, (8, 120, 2, 2, 40): 0}
DROPOUT_CASE = (21, 22)             # batch seed, mask seed of the explicit-mask test


def case(D, T, Fu, Fi, B, seed=None):
    """cfg, parameters (TF's initial values, the biases and bn1 moved off their zeros / ones), the batch behind the kink filter"""
    c = cr.Cfg(3000, D, 32, T, Fu, Fi)
    P = cr.init_params(c, 3)
    rng = np.random.default_rng(100 + (SHAPES[(D, T, Fu, Fi, B)] if seed is None else seed))
    for n in P:
        if "bias" in n or n.startswith("bn1"):
            P[n] = (P[n] + 0.1 * rng.standard_normal(P[n].shape)).astype(np.float32)
    b = cr.random_batch(rng, c, B)
    b["label"] = (np.arange(B) % 2).astype(np.int32)
    b, _, kept = cr.away_from_kinks(c, P, b)
    return c, P, b, kept


def dropout_case():
    c = cr.Cfg(3000, *TMALL)
    P = cr.init_params(c, 3)
    B = 200
    b = _batches(c, B, 1, DROPOUT_CASE[0])[0]
    rng = np.random.default_rng(DROPOUT_CASE[1])
    masks = [(rng.random((B, 200)) < 0.8).astype(np.uint8), (rng.random((B, 80)) < 0.8).astype(np.uint8)]
    b, masks, kept = cr.away_from_kinks(c, P, b, keep_prob=0.8, dropout_masks=masks)
    return c, P, b, masks, kept


def _model(c, P, flags=0, **kw):
    from score_amd.model import Caser
    m = Caser(*c.args, **kw)
    m.set_params(P)
    m.debug_flags = flags
    return m


def _batches(c, B, n, seed, **kw):
    rng = np.random.default_rng(seed)
    return [cr.random_batch(rng, c, B, **kw) for _ in range(n)]


def _pass(c, P, b, flags=0, reg=0.0, keep_prob=1.0, masks=None, model=None):
    """one forward + backward -> loss, y_pred, the saved window sums / positions / vertical sums, every gradient"""
    from score_amd import _lib
    m = model if model is not None else _model(c, P, flags)
    B = len(b["label"])
    lay, ws = m.forward_backward(batch_tuple(b), reg, keep_prob, dropout_masks=masks)
    f = lambda name: _lib.workspace_field(m.cfg, B, name)[0]
    hw, ar, v = f("caser_hwin"), f("caser_arg"), f("caser_v")
    return dict(loss=float(ws[lay.loss].item()), y=ws[lay.y_pred:lay.y_pred + B].cpu().numpy().copy(),
                hwin=ws[hw:hw + B * c.NW].view(B, c.NW).cpu().numpy().copy(),
                arg=ws[ar:ar + B].view(torch.int32).cpu().numpy().copy(),
                v=ws[v:v + B * c.C].view(B, c.C).cpu().numpy().copy(), grads=m.get_grads())


def _check(got, out, want_g, what):
    want_loss, want_y = float(out["loss"].detach()), out["y_pred"].detach().numpy()
    print(what, "loss", got["loss"], want_loss, "max |dy|", float(np.abs(got["y"] - want_y).max()))
    assert abs(got["loss"] - want_loss) < 2e-5 * max(1.0, abs(want_loss)), (what, got["loss"], want_loss)
    assert np.abs(got["y"] - want_y).max() < 1e-4, what
    for k in ("hwin", "v"):
        ok, err = close(got[k], out[k].detach().numpy(), rtol=2e-4, atol=2e-6)
        print(what, k, err)
        assert ok, (what, k, err)
    assert np.array_equal(got["arg"], out["arg"]), (what, got["arg"], out["arg"])
    assert set(got["grads"]) == set(want_g)
    for k in want_g:
        assert got["grads"][k].shape == want_g[k].shape, (what, k, got["grads"][k].shape)
        ok, err = close(got["grads"][k], want_g[k], rtol=2e-4, atol=2e-6)
        print(what, k, err)
        assert ok, (what, k, err)


@pytest.mark.parametrize("D,T,Fu,Fi,B", list(SHAPES))
def test_forward_backward_against_restatement(D, T, Fu, Fi, B):
    c, P, b, kept = case(D, T, Fu, Fi, B)
    print("kept", kept.size, "of", B)
    out, go = cr.loss_and_grads(c, P, b, 0.0)
    if c.NW > 1:
        assert np.unique(out["arg"]).size > 1           # (a property of the inputs: more than one window is chosen)
    got = _pass(c, P, b)
    _check(got, out, go, "caser")
    assert np.abs(go["emb_mtx"]).max() > 0 and not got["grads"]["emb_mtx"][0].any()


def test_pad_rows_stay_zero_and_the_boundary_has_tf_shapes():
    c = cr.Cfg(5003, *TMALL)
    P = cr.init_params(c, 6)
    m = _model(c, P)
    fresh = _model(c, P, seed=5)            # its own initialisation, before set_params: pad rows zero there too
    from score_amd.model import Caser
    own = Caser(*c.args, seed=5)
    pads = lambda mm, flat: [mm._view(flat, e)[1:4] for e in mm.entries if e[0] in mm.head_pad_vars]
    assert len(pads(own, own.w)) == 3 and all(not bool(p.any().item()) for p in pads(own, own.w))
    assert float(own._view(own.w, [e for e in own.entries if e[0] == "bn1/gamma"][0])[0].item()) == 1.0
    for bt in _batches(c, 200, 5, 7) * 2:
        m.train(None, batch_tuple(bt), 1e-3, 1e-4, keep_prob=0.8)
    assert m.step == 10
    for flat in (m.w, m.w_m, m.w_v):
        for p in pads(m, flat):
            assert p.numel() > 0 and torch.count_nonzero(p).item() == 0 and not bool(torch.signbit(p).any().item())
    spec = {n: s for n, s, _, _ in cr.param_spec(c)}
    spec["emb_mtx"] = (c.N, c.D)
    for d in (m.get_params(), m.get_grads(), fresh.get_params()):
        assert {k: v.shape for k, v in d.items()} == spec
    # the rows TF has did move
    assert np.abs(m.get_params()["fc1/kernel"] - P["fc1/kernel"]).max() > 0
    assert np.abs(m.get_params()["bn1/gamma"] - P["bn1/gamma"]).min() > 0


def test_user_seq_length_is_ignored():
    c = cr.Cfg(4000, 16, 32, 57, 3, 4)
    P = cr.init_params(c, 11)
    B = 48
    rng = np.random.default_rng(17)
    b = cr.random_batch(rng, c, B)
    ln = b["user_seq_length"]
    assert ln.min() < c.T
    runs = []
    for lengths in (np.ones(B), np.full(B, c.T), rng.integers(1, 3 * c.T + 1, B)):
        for skip in (True, False):
            m = _model(c, P)
            m.skip_masked_slices = skip
            bt = dict(b, user_seq_length=lengths.astype(np.int32))
            assert m.device_batch(batch_tuple(bt)).active_slices == 0
            lay, ws = m.forward_backward(batch_tuple(bt), 1e-4, 1.0)
            runs.append((float(ws[lay.loss].item()), ws[lay.y_pred:lay.y_pred + B].cpu().numpy().copy(), m.get_grads()))
    for loss, y, g in runs[1:]:
        assert loss == runs[0][0] and np.array_equal(y, runs[0][1])
        assert all(np.array_equal(g[k], runs[0][2][k]) for k in g)
    # rows named only by positions beyond a sample's length DO get gradient (they take part in both filters)
    bd = {k: v.copy() for k, v in b.items()}
    used = np.unique(np.concatenate([b[k].ravel() for k in ("user_seq", "target_user", "target_item")]))
    fresh = iter(np.setdiff1d(np.arange(1, c.N), used))
    only_padded = []
    for i in range(B):
        if ln[i] < c.T and len(only_padded) < 20:
            r = int(next(fresh))
            bd["user_seq"][i, ln[i]:, :] = r
            only_padded.append(r)
    assert len(only_padded) > 5
    got = _pass(c, P, bd)
    assert (np.abs(got["grads"]["emb_mtx"][np.array(only_padded)]).max(1) > 0).all()
    out, go = cr.loss_and_grads(c, P, bd, 0.0)
    ok, err = close(got["grads"]["emb_mtx"], go["emb_mtx"], rtol=2e-4, atol=2e-6)
    assert ok, err


def test_ten_train_steps_against_restatement_and_adam():
    c = cr.Cfg(20011, *TMALL)
    P = cr.init_params(c, 4)
    m, ref = _model(c, P), cr.RefModel(c, P)
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


def test_one_step_with_explicit_dropout_masks():
    c, P, b, masks, kept = dropout_case()
    print("kept", kept.size, "of", 200)
    # (reg_lambda 0: get_grads() is the data term's gradient; the L2 term's is added by the optimizer step, test above)
    out, go = cr.loss_and_grads(c, P, b, 0.0, 0.8, masks)
    got = _pass(c, P, b, reg=0.0, keep_prob=0.8, masks=masks)
    _check(got, out, go, "dropout 0.8")
    # ... and as a training step with the L2 term: its loss, and the loss of the step after it (which sees the update)
    m, ref = _model(c, P), cr.RefModel(c, P)
    for kp, dm in ((0.8, masks), (1.0, None)):
        lg = m.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=kp, dropout_masks=dm)
        lo = ref.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=kp, dropout_masks=dm)
        print("train", kp, lg, lo)
        assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo)), (kp, lg, lo)


def test_forty_steps_through_the_point_loader_and_feed(tmp_path):
    from score_amd.pointdata import DataLoaderUserSeq
    T, Fu, Fi, B = 50, 2, 3, 32
    (tf, hf, uf, itf), N = _write_point_files(tmp_path, np.random.default_rng(31), 16 * 5 + 3, T, Fu, Fi)
    c = cr.Cfg(N, 16, 32, T, Fu, Fi)
    P = cr.init_params(c, 3)
    m, ref = _model(c, P), cr.RefModel(c, P)
    batches = list(DataLoaderUserSeq(B, T, tf, hf, 1, uf, itf))
    assert len(batches) == 5 and batches[0][0].shape == (B, T, Fi) and int(max(b[1].max() for b in batches)) > T
    assert int(min(b[1].min() for b in batches)) < T
    step = 0
    for db, host in zip(m.feed(batches * 8), batches * 8):
        assert db.active_slices == 0
        lg = m.train(None, db, 1e-3, 1e-4, keep_prob=1.0)
        lo = ref.train(None, host, 1e-3, 1e-4, keep_prob=1.0)
        assert abs(lg - lo) < 1e-3 * max(abs(lo), 1e-6), (step, lg, lo)
        step += 1
    assert step == 40
    print("last losses", lg, lo)


def test_single_stream_gives_the_same_bits():
    """debug_flags bit 12: no second stream anywhere."""
    c = cr.Cfg(5003, *TMALL)
    P = cr.init_params(c, 6)
    a, b = _model(c, P), _model(c, P, 4096)
    for bt in _batches(c, 200, 3, 7):
        assert a.train(None, batch_tuple(bt), 1e-3, 1e-4) == b.train(None, batch_tuple(bt), 1e-3, 1e-4)
    assert _same_state(a, b)


def test_time_tiled_optimizer_equals_the_sweep():
    c = cr.Cfg(6007, *TMALL)
    P = cr.init_params(c, 7)
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
    c = cr.Cfg(4001, *TMALL)
    P = cr.init_params(c, 4)
    eager, graphed = _model(c, P, seed=77), _model(c, P, seed=77)
    graphed.enable_graph(True)
    rng = np.random.default_rng(1)
    bs = [cr.random_batch(rng, c, 200) for _ in range(5)]
    other = cr.random_batch(rng, c, 100)
    seq = [bs[0], bs[1], bs[2], other, bs[3], other, bs[4], other, bs[0]]
    for i, b in enumerate(seq):
        le = eager.train(None, batch_tuple(b), 1e-3, 1e-4)         # train()'s default keep_prob = 0.8
        lg = graphed.train(None, batch_tuple(b), 1e-3, 1e-4)
        assert le == lg, (i, le, lg)
    assert len([v for v in graphed._graphs.values() if isinstance(v, tuple)]) == 2
    assert _same_state(eager, graphed)
    pe, _, _ = eager.eval(None, batch_tuple(bs[1]), 1e-4)
    pg, _, _ = graphed.eval(None, batch_tuple(bs[1]), 1e-4)
    assert pe == pg


def test_lists_arrays_and_device_tensors_feed_the_same_batch():
    c = cr.Cfg(3001, 16, 32, 52, 3, 4)
    P = cr.init_params(c, 5)
    ms = [_model(c, P) for _ in range(3)]
    for b in _batches(c, 64, 3, 12, max_length=150):
        arrays = batch_tuple(b)
        lists = tuple(a.tolist() for a in arrays)                  # what the reference's loader yields
        device = tuple(torch.as_tensor(a).cuda() for a in arrays)
        losses = [m.train(None, f, 1e-3, 1e-4, keep_prob=1.0) for m, f in zip(ms, (arrays, lists, device))]
        assert losses[0] == losses[1] == losses[2]
    assert _same_state(ms[0], ms[1]) and _same_state(ms[0], ms[2])
    # the length tensor is not read, but it is part of the tuple and its shape is checked
    with pytest.raises(ValueError) as ei:
        ms[0].device_batch(batch_tuple(dict(b, user_seq_length=b["user_seq_length"][:-1])))
    assert "batch_data[1] (user_seq_length)" in str(ei.value)


def test_two_fresh_models_give_the_same_bits():
    """every sum over the batch is taken in a fixed order (csrc/caser.hip): no gradient depends on how the workgroups ran"""
    c, P, b, _ = case(16, 57, 3, 4, 33)
    big = _batches(cr.Cfg(3000, *TMALL), 200, 1, 5)[0]
    for cc, bb in ((c, b), (cr.Cfg(3000, *TMALL), big)):
        PP = cr.init_params(cc, 3)
        g1, g2 = _pass(cc, PP, bb), _pass(cc, PP, bb)
        assert g1["loss"] == g2["loss"] and np.array_equal(g1["y"], g2["y"])
        for k in g1["grads"]:
            assert np.array_equal(g1["grads"][k], g2["grads"][k]), k


def test_save_restore_roundtrip(tmp_path):
    c = cr.Cfg(3001, *TMALL)
    P = cr.init_params(c, 8)
    m = _model(c, P)
    bs = _batches(c, 50, 3, 2)
    for b in bs[:2]:
        m.train(None, batch_tuple(b), 1e-3, 1e-4)
    m.save(None, str(tmp_path / "caser"))
    z = np.load(str(tmp_path / "caser") + ".npz")
    spec = {s[0]: s[1] for s in cr.param_spec(c)}
    spec["emb_mtx"] = (c.N, c.D)
    names = set(spec)
    assert set(z.files) == names | {n + s for n in names for s in ("/Adam", "/Adam_1")} | {"beta1_power", "beta2_power", "global_step"}
    for n in names:
        for s in ("", "/Adam", "/Adam_1"):
            assert z[n + s].shape == spec[n], (n + s, z[n + s].shape)
    m2 = _model(c, cr.init_params(c, 99))
    m2.restore(None, str(tmp_path / "caser"))
    assert _same_state(m, m2)
    assert m.eval(None, batch_tuple(bs[2]), 1e-4) == m2.eval(None, batch_tuple(bs[2]), 1e-4)
    assert set(m2.get_params()) == names
    assert m.train(None, batch_tuple(bs[2]), 1e-3, 1e-4) == m2.train(None, batch_tuple(bs[2]), 1e-3, 1e-4)


@pytest.mark.parametrize("field,where,named", [("user_seq", (1, 2, 0), "batch_data[0] (user_seq)"),
                                               ("target_item", (0, 1), "batch_data[3] (target_item)"),
                                               ("target_user", (3, 0), "batch_data[2] (target_user)")])
def test_bad_id_raises_and_the_model_trains_on(field, where, named):
    c = cr.Cfg(2003, 16, 32, 50, 3, 4)
    P = cr.init_params(c, 2)
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
    c = cr.Cfg(4001, *TMALL)
    m = _model(c, cr.init_params(c, 3))
    neg, lines = 99, 4
    batches = []
    for i in range(2):
        b = _batches(c, lines * (neg + 1), 1, 40 + i)[0]
        b["label"] = (np.arange(lines * (neg + 1)) % (neg + 1) == 0).astype(np.int32)     # one positive per line
        batches.append(batch_tuple(b))
    host = h.evaluate(m, [tuple(a.tolist() for a in b) for b in batches], 1e-4, neg_sample_num=neg)
    dev = h.evaluate_device(m, batches, 1e-4, neg_sample_num=neg)
    assert np.allclose(host, dev, rtol=1e-5, atol=2e-6)
    assert m.target_item_field == 3 and np.array_equal(m.device_batch(batches[0]).tensors[5].cpu().numpy(), batches[0][3])


def test_sharded_training_refuses_the_point_model():
    from score_amd.dist import ShardedSCORE
    with pytest.raises(ValueError, match="Caser"):
        ShardedSCORE(1000, 16, 32, 50, 1, 3, 4, comm=object(), model_type="Caser")
