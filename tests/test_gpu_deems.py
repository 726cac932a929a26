"""The DEEMS point baseline (point_model.py:281-311) on the GPU against its float64 restatement (tests/deems_ref.py): the pass in
its four forms (debug_flags bit 6: the towers layer by layer; bit 13: one recurrence per launch), both final states, both
towers' predictions, every gradient and the training trajectory; the two length tensors; dropout from masks and from a seed; the
consistency term, reported and not trained on; the dormant DELF variables; and the step's other forms -- single stream,
time-tiled optimizer, captured graph, the three feed forms, checkpoints, bad ids, device-side evaluation -- against the plain
eager step.

Tolerances are the project's for point models (tests/test_gpu_delf.py, tests/test_gpu_gru4rec.py): loss 2e-5 relative to
max(1, |loss|), y 1e-4, arrays and gradients rtol 2e-4 / atol 2e-6."""
import functools

import numpy as np
import pytest
import torch

import deems_cases as ec
import deems_ref as er
from deems_ref import batch_tuple
from test_gpu_gru4rec import _same_state
from test_gpu_model import close

pytestmark = pytest.mark.gpu

TMALL = ec.TMALL
_batches = ec.batches
LAYERED, PER_SIDE = 64, 8192                 # debug_flags bit 6, bit 13
FORMS = (0, LAYERED, PER_SIDE, LAYERED | PER_SIDE)


def _model(c, P, flags=0, **kw):
    from score_amd.model import DEEMS
    m = DEEMS(*c.args, **kw)
    m.set_params(P)
    m.debug_flags = flags
    return m


def _field(m, ws, B, name, n):
    from score_amd import _lib
    a, b = _lib.workspace_field(m.cfg, B, name)
    return [ws[o:o + B * n].view(B, n).cpu().numpy().copy() if n > 1 else ws[o:o + B].cpu().numpy().copy() for o in (a, b)]


def _pass(c, P, b, flags=0, reg=0.0, keep_prob=1.0, masks=None, model=None, skip=True):
    """one forward + backward -> loss, y_pred, y_u, y_i, h_u, h_i, the towers' fc1 outputs, every gradient"""
    m = model if model is not None else _model(c, P, flags)
    m.skip_masked_slices = skip
    B = len(b["label"])
    db = m.device_batch(batch_tuple(b))
    lay, ws = m.forward_backward(db, reg, keep_prob, dropout_masks=masks)
    (yu, yi), (hu, hi), (f1u, f1i) = _field(m, ws, B, "deems_y", 1), _field(m, ws, B, "gru_final", c.H), _field(m, ws, B, "deems_f1", 200)
    return dict(loss=float(ws[lay.loss].item()), y_pred=ws[lay.y_pred:lay.y_pred + B].cpu().numpy().copy(), y_u=yu, y_i=yi, h_u=hu,
                h_i=hi, f1_u=f1u, f1_i=f1i, grads=m.get_grads(), active=db.active_slices)


def _check(got, out, want_g, what):
    want_loss = float(out["loss"].detach())
    print(what, "loss", got["loss"], want_loss)
    assert abs(got["loss"] - want_loss) < 2e-5 * max(1.0, abs(want_loss)), (what, got["loss"], want_loss)
    for k in ("y_pred", "y_u", "y_i"):
        err = float(np.abs(got[k] - out[k].detach().numpy()).max())
        print(what, k, err)
        assert err < 1e-4, (what, k, err)
    for k in ("h_u", "h_i"):
        ok, err = close(got[k], out[k].detach().numpy(), rtol=2e-4, atol=2e-6)
        print(what, k, err)
        assert ok, (what, k, err)
    assert set(got["grads"]) == set(want_g) and len(want_g) == 47
    for k in want_g:
        assert got["grads"][k].shape == want_g[k].shape, (what, k, got["grads"][k].shape)
        ok, err = close(got["grads"][k], want_g[k], rtol=2e-4, atol=2e-6)
        print(what, k, err)
        assert ok, (what, k, err)


def _same_bits(g1, g2):
    assert g1["loss"] == g2["loss"]
    for k in ("y_pred", "y_u", "y_i", "h_u", "h_i", "f1_u", "f1_i"):
        assert np.array_equal(g1[k], g2[k]), k
    for k in g1["grads"]:
        assert np.array_equal(g1["grads"][k], g2["grads"][k]), k


@functools.lru_cache(maxsize=None)
def _case(shape):
    """a case of deems_cases.SHAPES and the restatement's pass over it: computed once, shared, never written to"""
    c, P, b, kept = ec.case(*shape)
    out, go = er.loss_and_grads(c, P, b, 0.0)
    return c, P, b, kept, out, go


@pytest.mark.parametrize("D,H,T,Fu,Fi,B", list(ec.SHAPES))
def test_forward_backward_against_restatement(D, H, T, Fu, Fi, B):
    c, P, b, kept, out, go = _case((D, H, T, Fu, Fi, B))
    print("kept", kept.size, "of", B)
    got = {f: _pass(c, P, b, f) for f in FORMS}
    for f in FORMS:
        _check(got[f], out, go, "deems, flags %d" % f)
        assert not got[f]["grads"]["emb_mtx"][0].any()
    assert np.abs(go["emb_mtx"]).max() > 0
    # one grouped launch or one launch per side: the same kernels on the same rows
    _same_bits(got[0], got[PER_SIDE])
    _same_bits(got[LAYERED], got[LAYERED | PER_SIDE])
    # a length <= 0: that recurrence never runs
    for h, ln in ((got[0]["h_u"], b["user_seq_length"]), (got[0]["h_i"], b["item_seq_length"])):
        for i in np.nonzero(ln <= 0)[0]:
            assert not h[i].any()
    if B == 3:
        assert (b["user_seq_length"] <= 0).any() and (b["item_seq_length"] <= 0).any()
        assert (b["user_seq_length"] > T).any() and (b["item_seq_length"] > T).any()
    if (T, B) == (7, 33):
        # every length <= 5: only the leading slices were computed; all T computed gives the same loss and gradients
        assert got[0]["active"] == int(max(b["user_seq_length"].max(), b["item_seq_length"].max())) < T
        allT = _pass(c, P, b, skip=False)
        assert allT["active"] == 0
        _check(allT, out, go, "deems, all slices")
        assert abs(allT["loss"] - got[0]["loss"]) < 2e-5 * max(1.0, abs(got[0]["loss"]))
        for k in go:
            ok, err = close(allT["grads"][k], got[0]["grads"][k], rtol=2e-4, atol=2e-6)
            assert ok, (k, err)
    else:
        assert got[0]["active"] == 0


def test_a_zero_length_does_not_make_the_batch_compute_every_slice():
    c = er.Cfg(500, 8, 32, 9, 2, 1)
    P = ec.params(c)
    b = _batches(c, 6, 1, 4, max_length=(4, 4))[0]
    b0 = dict(b, user_seq_length=np.array([0, 2, 3, 1, 4, 2], dtype=np.int32), item_seq_length=np.array([1, 2, 0, 3, 4, 1], dtype=np.int32))
    m = _model(c, P)
    arrays = batch_tuple(b0)
    for feed in (arrays, tuple(a.tolist() for a in arrays), tuple(torch.as_tensor(a).cuda() for a in arrays)):
        assert m.device_batch(feed).active_slices == 4
    out, go = er.loss_and_grads(c, P, b0, 0.0)
    got = _pass(c, P, b0)
    assert got["active"] == 4
    _check(got, out, go, "zero length")
    assert not got["h_u"][0].any() and not got["h_i"][2].any()


def test_each_side_runs_under_its_own_lengths():
    c = er.Cfg(3000, 16, 32, 9, 3, 4)
    P = ec.params(c)
    b = _batches(c, 33, 1, 6, max_length=(12, 12))[0]
    assert not np.array_equal(b["user_seq_length"], b["item_seq_length"])
    swapped = dict(b, user_seq_length=b["item_seq_length"], item_seq_length=b["user_seq_length"])
    g, gs = _pass(c, P, b), _pass(c, P, swapped)
    assert g["loss"] != gs["loss"] and not np.array_equal(g["h_u"], gs["h_u"]) and not np.array_equal(g["h_i"], gs["h_i"])
    with torch.no_grad():
        want, want_s = er.forward(c, er.to_torch(P), b), er.forward(c, er.to_torch(P), swapped)
    for got, w in ((g, want), (gs, want_s)):
        for k in ("h_u", "h_i"):
            ok, err = close(got[k], w[k].numpy(), rtol=2e-4, atol=2e-6)
            assert ok, (k, err)
    # equal lengths on both sides: the grouped launch gives the bits of the per-side launches
    same = dict(b, item_seq_length=b["user_seq_length"])
    _same_bits(_pass(c, P, same), _pass(c, P, same, PER_SIDE))


def test_one_step_with_explicit_dropout_masks():
    c, P, b, masks, kept = ec.dropout_case(0.8)
    out, go = er.loss_and_grads(c, P, b, 0.0, 0.8, masks)
    got = {f: _pass(c, P, b, f, keep_prob=0.8, masks=masks) for f in FORMS}
    for f in FORMS:
        _check(got[f], out, go, "deems, masks, flags %d" % f)
        for k, tw in (("f1_u", 0), ("f1_i", 1)):
            assert not got[f][k][masks[0][tw] == 0].any()          # what the mask drops is dropped, tower by tower
    _same_bits(got[0], got[PER_SIDE])
    m = _model(c, P)
    with pytest.raises(ValueError):
        m.forward_backward(batch_tuple(b), 0.0, 0.8, dropout_masks=[masks[0][0], masks[1][0]])       # (one tower's masks)


def test_dropout_from_a_seed():
    c = er.Cfg(3000, 16, 32, 9, 3, 4)
    P = ec.params(c)
    b = _batches(c, 33, 1, 8)[0]
    for f in (0, LAYERED):
        g1, g2 = _pass(c, P, b, f, keep_prob=0.8, model=_model(c, P, f, seed=5)), _pass(c, P, b, f, keep_prob=0.8, model=_model(c, P, f, seed=5))
        _same_bits(g1, g2)                                         # two fresh models, one seed
        # the towers draw from streams of their own: what one keeps of f1 is not what the other keeps
        base = _pass(c, P, b, f)
        ku, ki = g1["f1_u"] != 0, g1["f1_i"] != 0
        both = (base["f1_u"] > 0) & (base["f1_i"] > 0)             # units alive in both towers without dropout
        assert both.sum() > 200 and (ku[both] != ki[both]).mean() > 0.1
        for kept_, full in ((ku, base["f1_u"] > 0), (ki, base["f1_i"] > 0)):
            assert not (kept_ & ~full).any() and 0.7 < kept_[full].mean() < 0.9
        other = _pass(c, P, b, f, keep_prob=0.8, model=_model(c, P, f, seed=6))
        assert not np.array_equal(other["f1_u"], g1["f1_u"])
    # the fused head and the layer-by-layer form drop the same units
    a, l = _pass(c, P, b, 0, keep_prob=0.8, model=_model(c, P, 0, seed=5)), _pass(c, P, b, LAYERED, keep_prob=0.8, model=_model(c, P, LAYERED, seed=5))
    assert np.array_equal(a["f1_u"] != 0, l["f1_u"] != 0) and np.array_equal(a["f1_i"] != 0, l["f1_i"] != 0)


def test_keep_prob_one_reads_no_mask():
    c, P, b, masks, _ = ec.dropout_case(0.8)
    for f in (0, LAYERED):
        _same_bits(_pass(c, P, b, f, keep_prob=1.0, masks=masks), _pass(c, P, b, f))


def test_the_consistency_term_is_reported_and_not_trained_on():
    c, P, b, kept, out, go = _case((16, 32, 50, 3, 4, 200))
    cons, loss = float(out["consistency"].detach()), float(out["loss"].detach())
    assert cons > 0.01 * loss
    got = _pass(c, P, b)
    assert abs(got["loss"] - loss) < 2e-5 * max(1.0, abs(loss))
    assert abs(got["loss"] - float(out["train_loss"].detach())) > 0.5 * cons
    _check(got, out, go, "consistency")                           # (the gradients of train_loss: without the term)
    _, g_rep = er.loss_and_grads(c, P, b, 0.0, of="loss")
    k = "dense_13/kernel"
    assert not close(got["grads"][k], g_rep[k], rtol=2e-4, atol=2e-6)[0]


@pytest.mark.parametrize("reg", [1e-2, 0.0])
def test_the_dormant_delf_variables(reg):
    c = er.Cfg(3001, 16, 32, 9, 3, 4)
    P = ec.params(c)
    m, ref = _model(c, P), er.RefModel(c, P)
    bs = _batches(c, 33, 5, 11)
    for b in bs:
        m.train(None, batch_tuple(b), 1e-3, reg, keep_prob=1.0)
        ref.train(None, batch_tuple(b), 1e-3, reg, keep_prob=1.0)
    got = m.get_params()
    for i in range(11):
        nm = "dense" if i == 0 else "dense_%d" % i
        assert np.array_equal(got[nm + "/bias"], P[nm + "/bias"]), nm
        if reg == 0.0:
            assert np.array_equal(got[nm + "/kernel"], P[nm + "/kernel"]), nm
        else:
            assert not np.array_equal(got[nm + "/kernel"], P[nm + "/kernel"]), nm
            ok, err = close(got[nm + "/kernel"], ref.params[nm + "/kernel"], rtol=2e-4, atol=2e-6)
            assert ok, (nm, err)


def test_ten_train_steps_against_restatement_and_adam():
    c = er.Cfg(20011, *TMALL)
    P = er.init_params(c, 4)
    m, ref = _model(c, P), er.RefModel(c, P)
    bs = _batches(c, 200, 5, 8)
    for step in range(10):
        b = batch_tuple(bs[step % len(bs)])
        lg = m.train(None, b, 1e-3, 1e-4, keep_prob=1.0)
        lo = ref.train(None, b, 1e-3, 1e-4, keep_prob=1.0)
        print(step, lg, lo)
        assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo)), (step, lg, lo)
    pg, lab, lg = m.eval(None, batch_tuple(bs[0]), 1e-4)
    po, lab_o, lo = ref.eval(None, batch_tuple(bs[0]), 1e-4)
    assert lab == lab_o
    assert np.abs(np.asarray(pg) - np.asarray(po)).max() < 1e-4
    assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo))


def test_two_fresh_models_give_the_same_bits():
    """every sum over the batch is taken in a fixed order (csrc/deems.hip, the queued products): no result depends on how the
    workgroups ran"""
    c, P, b, _, _, _ = _case((16, 32, 7, 3, 4, 33))
    big = _batches(er.Cfg(3000, *TMALL), 200, 1, 5)[0]
    for cc, bb in ((c, b), (er.Cfg(3000, *TMALL), big)):
        PP = er.init_params(cc, 3)
        _same_bits(_pass(cc, PP, bb), _pass(cc, PP, bb))


def test_single_stream_gives_the_same_bits():
    """debug_flags bit 12: no second stream anywhere."""
    c = er.Cfg(5003, *TMALL)
    P = er.init_params(c, 6)
    a, b = _model(c, P, seed=3), _model(c, P, 4096, seed=3)
    for bt in _batches(c, 200, 3, 7):
        assert a.train(None, batch_tuple(bt), 1e-3, 1e-4) == b.train(None, batch_tuple(bt), 1e-3, 1e-4)
    assert _same_state(a, b)


def test_time_tiled_optimizer_equals_the_sweep():
    c = er.Cfg(6007, *TMALL)
    P = er.init_params(c, 7)
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
    c = er.Cfg(4001, *TMALL)
    P = er.init_params(c, 4)
    eager, graphed = _model(c, P, seed=77), _model(c, P, seed=77)
    graphed.enable_graph(True)
    rng = np.random.default_rng(1)
    kw = dict(max_length=(3 * c.T, 3 * c.T))
    bs = [er.random_batch(rng, c, 200, **kw) for _ in range(5)]
    other = er.random_batch(rng, c, 100, **kw)
    seq = [bs[0], bs[1], bs[2], other, bs[3], other, bs[4], other, bs[0]]
    for i, b in enumerate(seq):
        le = eager.train(None, batch_tuple(b), 1e-3, 1e-4)            # (keep_prob 0.8: the step's seed comes from device memory)
        lg = graphed.train(None, batch_tuple(b), 1e-3, 1e-4)
        assert le == lg, (i, le, lg)
    assert len([v for v in graphed._graphs.values() if isinstance(v, tuple)]) == 2
    assert _same_state(eager, graphed)
    pe, _, _ = eager.eval(None, batch_tuple(bs[1]), 1e-4)
    pg, _, _ = graphed.eval(None, batch_tuple(bs[1]), 1e-4)
    assert pe == pg


def test_lists_arrays_and_device_tensors_feed_the_same_batch():
    c = er.Cfg(3001, 16, 32, 52, 3, 4)
    P = er.init_params(c, 5)
    ms = [_model(c, P) for _ in range(4)]
    bs = _batches(c, 64, 3, 12, max_length=(150, 150))
    fed = ms[3].feed([batch_tuple(b) for b in bs])
    for b, db in zip(bs, fed):
        arrays = batch_tuple(b)
        lists = tuple(a.tolist() for a in arrays)                  # what the reference's loader yields
        device = tuple(torch.as_tensor(a).cuda() for a in arrays)
        losses = [m.train(None, f, 1e-3, 1e-4, keep_prob=1.0) for m, f in zip(ms, (arrays, lists, device, db))]
        assert losses[0] == losses[1] == losses[2] == losses[3]
    assert all(_same_state(ms[0], m) for m in ms[1:])
    db = ms[0].device_batch(batch_tuple(b))
    assert len(db.tensors) == 9 and np.array_equal(db.tensors[8].cpu().numpy(), b["item_seq_length"])
    assert np.array_equal(db.tensors[2].cpu().numpy().reshape(b["item_seq"].shape), b["item_seq"])
    for field, pos in (("item_seq_length", 3), ("item_seq", 2), ("user_seq_length", 1)):
        with pytest.raises(ValueError) as ei:
            ms[0].device_batch(batch_tuple(dict(b, **{field: b[field][:-1]})))
        assert "batch_data[%d] (%s)" % (pos, field) in str(ei.value)
    with pytest.raises(ValueError):
        ms[0].device_batch(batch_tuple(b)[:5])


def test_save_restore_roundtrip(tmp_path):
    c = er.Cfg(3001, *TMALL)
    P = er.init_params(c, 8)
    m = _model(c, P)
    bs = _batches(c, 50, 3, 2)
    for b in bs[:2]:
        m.train(None, batch_tuple(b), 1e-3, 1e-4)
    m.save(None, str(tmp_path / "deems"))
    z = np.load(str(tmp_path / "deems") + ".npz")
    spec = {s[0]: s[1] for s in er.param_spec(c)}
    spec["emb_mtx"] = (c.N, c.D)
    names = set(spec)
    assert len(names) == 47
    assert set(z.files) == names | {n + s for n in names for s in ("/Adam", "/Adam_1")} | {"beta1_power", "beta2_power", "global_step"}
    for n in names:
        for s in ("", "/Adam", "/Adam_1"):
            assert z[n + s].shape == tuple(spec[n]), (n + s, z[n + s].shape)
    m2 = _model(c, er.init_params(c, 99))
    m2.restore(None, str(tmp_path / "deems"))
    assert _same_state(m, m2)
    assert m.eval(None, batch_tuple(bs[2]), 1e-4) == m2.eval(None, batch_tuple(bs[2]), 1e-4)
    assert set(m2.get_params()) == names
    assert m.train(None, batch_tuple(bs[2]), 1e-3, 1e-4, keep_prob=1.0) == m2.train(None, batch_tuple(bs[2]), 1e-3, 1e-4, keep_prob=1.0)


@pytest.mark.parametrize("field,where,named", [("item_seq", (1, 2, 0), "batch_data[2] (item_seq)"),
                                               ("user_seq", (1, 2, 0), "batch_data[0] (user_seq)"),
                                               ("target_item", (0, 1), "batch_data[5] (target_item)"),
                                               ("target_user", (3, 0), "batch_data[4] (target_user)")])
def test_bad_id_raises_and_the_model_trains_on(field, where, named):
    c = er.Cfg(2003, 16, 32, 50, 3, 4)
    P = er.init_params(c, 2)
    m, clean = _model(c, P, seed=9), _model(c, P, seed=9)
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
    c = er.Cfg(4001, *TMALL)
    m = _model(c, ec.params(c))
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
