"""The SASRec point baseline (point_model.py:313-469) on the GPU against its float64 restatement (tests/sasrec_ref.py): the loss,
the prediction, Y, final, the attention weights, all 14 gradients and the table gradient over the shapes of sasrec_cases.SHAPES;
id 0 at whole positions and in single fields (key masks, and with beta = 0 query masks); a history that is all id 0; keep_prob
0.8 with all three explicit masks; evaluation; ten training steps; training from a seed; and the step's other forms -- two fresh
models, single stream, captured graph at keep_prob 1 and 0.8, time-tiled optimizer, the three feed forms, checkpoints, bad ids,
device-side evaluation -- against the plain eager step.

Tolerances are the project's for point models (tests/test_gpu_deems.py): loss 2e-5 relative to max(1, |loss|), y 1e-4, arrays and
gradients rtol 2e-4 / atol 2e-6."""
import functools

import numpy as np
import pytest
import torch

import sasrec_cases as sc
import sasrec_ref as sr
from sasrec_ref import batch_tuple
from test_gpu_gru4rec import _same_state
from test_gpu_model import close

pytestmark = pytest.mark.gpu

TMALL = sc.TMALL
_batches = sc.batches


def _model(c, P, flags=0, **kw):
    from score_amd.model import SASRec
    m = SASRec(*c.args, **kw)
    m.set_params(P)
    m.debug_flags = flags
    return m


def _field(m, ws, B, name, shape):
    from score_amd import _lib
    o, _ = _lib.workspace_field(m.cfg, B, name)
    return ws[o:o + int(np.prod(shape))].view(*shape).cpu().numpy().copy()


def _pass(c, P, b, flags=0, reg=0.0, keep_prob=1.0, masks=None, model=None):
    """one forward + backward -> loss, y_pred, Y, final, the attention weights, every gradient"""
    m = model if model is not None else _model(c, P, flags)
    B, T, C = len(b["label"]), c.T, c.Ci
    db = m.device_batch(batch_tuple(b))
    lay, ws = m.forward_backward(db, reg, keep_prob, dropout_masks=masks)
    return dict(loss=float(ws[lay.loss].item()), y_pred=ws[lay.y_pred:lay.y_pred + B].cpu().numpy().copy(),
                Y=_field(m, ws, B, "sasrec_y", (B, T, C)), final=_field(m, ws, B, "sasrec_final", (B, C)),
                att=_field(m, ws, B, "sasrec_att", (B, 2, T, T)), grads=m.get_grads(), active=db.active_slices)


def _check(got, out, want_g, what):
    want_loss = float(out["loss"].detach())
    print(what, "loss", got["loss"], want_loss)
    assert abs(got["loss"] - want_loss) < 2e-5 * max(1.0, abs(want_loss)), (what, got["loss"], want_loss)
    err = float(np.abs(got["y_pred"] - out["y_pred"].detach().numpy()).max())
    print(what, "y_pred", err)
    assert err < 1e-4, (what, err)
    for k in ("Y", "final", "att"):
        ok, err = close(got[k], out[k].detach().numpy(), rtol=2e-4, atol=2e-6)
        print(what, k, err)
        assert ok, (what, k, err)
    assert set(got["grads"]) == set(want_g) and len(want_g) == 15
    for k in want_g:
        assert got["grads"][k].shape == want_g[k].shape, (what, k, got["grads"][k].shape)
        ok, err = close(got["grads"][k], want_g[k], rtol=2e-4, atol=2e-6)
        print(what, k, err)
        assert ok, (what, k, err)
    assert not got["grads"]["emb_mtx"][0].any()


def _same_bits(g1, g2):
    assert g1["loss"] == g2["loss"]
    for k in ("y_pred", "Y", "final", "att"):
        assert np.array_equal(g1[k], g2[k]), k
    for k in g1["grads"]:
        assert np.array_equal(g1["grads"][k], g2["grads"][k]), k


@functools.lru_cache(maxsize=None)
def _case(shape):
    """a case of sasrec_cases.SHAPES and the restatement's pass over it: computed once, shared, never written to"""
    c, P, b, kept = sc.case(*shape)
    out, go = sr.loss_and_grads(c, P, b, 0.0)
    return c, P, b, kept, out, go


@pytest.mark.parametrize("D,T,Fu,Fi,B", list(sc.SHAPES))
def test_forward_backward_against_restatement(D, T, Fu, Fi, B):
    c, P, b, kept, out, go = _case((D, T, Fu, Fi, B))
    print("kept", kept.size, "of", B)
    got = _pass(c, P, b)
    _check(got, out, go, "sasrec")
    assert got["active"] == 0          # all T positions, whatever the lengths
    for name, _, _, _ in sr.param_spec(c):
        # (the keys' bias shifts every score of a row alike, and the softmax does not see it: its gradient is a rounding residue)
        assert name == "multihead_attention/dense_1/bias" or np.abs(go[name]).max() > 0, name
    assert np.abs(go["multihead_attention/dense_1/bias"]).max() < 1e-12
    if B == 3:
        assert b["user_seq_length"].tolist() == [1, 4, 9]


@pytest.mark.parametrize("beta_zero", [False, True])
def test_id_zero_at_whole_positions_and_in_single_fields(beta_zero):
    c, P, b, kept = sc.masked_case(beta_zero)
    out, go = sr.loss_and_grads(c, P, b, 0.0)
    got = _pass(c, P, b)
    _check(got, out, go, "masked, beta zero" if beta_zero else "masked")
    zero = (b["user_seq"] == 0).all(2)
    assert zero.sum() > 10
    assert not got["att"][np.broadcast_to(zero[:, None, None, :], got["att"].shape)].any()           # masked keys: exact zeros
    if beta_zero:
        assert not got["att"][np.broadcast_to(zero[:, None, :, None], got["att"].shape)].any()       # ... and masked queries


def test_a_history_of_id_zero_gets_uniform_weights():
    c, P, b = sc.all_masked_case()
    out, go = sr.loss_and_grads(c, P, b, 0.0)
    got = _pass(c, P, b)
    _check(got, out, go, "all masked")
    assert np.array_equal(got["att"][1], np.full((2, c.T, c.T), np.float32(1.0) / np.float32(c.T)))
    assert np.isfinite(got["loss"]) and all(np.isfinite(v).all() for v in got["grads"].values())


def test_one_step_with_explicit_dropout_masks():
    c, P, b, masks, kept = sc.dropout_case()
    print("kept", kept.size, "of", 33)
    out, go = sr.loss_and_grads(c, P, b, 0.0, 0.8, masks)
    got = _pass(c, P, b, keep_prob=0.8, masks=masks)
    _check(got, out, go, "dropout 0.8")
    assert (got["att"] == 0).sum() > 0.1 * got["att"].size
    # ... and as a training step with the L2 term: its loss, and the loss of the step after it (which sees the update)
    m, ref = _model(c, P), sr.RefModel(c, P)
    for kp, dm in ((0.8, masks), (1.0, None)):
        lg = m.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=kp, dropout_masks=dm)
        lo = ref.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=kp, dropout_masks=dm)
        print("train", kp, lg, lo)
        assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo)), (kp, lg, lo)
    with pytest.raises(ValueError, match="dropout masks"):
        m.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=0.8, dropout_masks=masks[:2])


def test_eval_equals_the_restatement():
    c, P, b, kept, out, go = _case((16, 9, 3, 4, 33))
    m = _model(c, P)
    y, lab, loss = m.eval(None, batch_tuple(b), 1e-3)
    with torch.no_grad():
        want = sr.forward(c, sr.to_torch(P), b, 1e-3)
    assert lab == b["label"].tolist() and m.step == 0
    assert np.abs(np.asarray(y) - want["y_pred"].numpy()).max() < 1e-4
    assert abs(loss - float(want["loss"])) < 2e-5 * max(1.0, abs(float(want["loss"])))


def test_ten_train_steps_against_restatement_and_adam():
    c, P, bs = sc.trajectory_case()
    m, ref = _model(c, P), sr.RefModel(c, P)
    for step in range(10):
        b = batch_tuple(bs[step % len(bs)])
        lg = m.train(None, b, 1e-3, 1e-2, keep_prob=1.0)
        lo = ref.train(None, b, 1e-3, 1e-2, keep_prob=1.0)
        print(step, lg, lo)
        assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo)), (step, lg, lo)
    print("min |sum Qin|", ref.min_qsum)
    assert ref.min_qsum > 1e-3          # the query mask was decided by a wide margin on the whole trajectory
    got = m.get_params()
    for name, _, _, _ in sr.param_spec(c):
        assert not np.array_equal(got[name], P[name]), name
        if name == "multihead_attention/dense_1/bias":
            # The keys' bias shifts every score of a row alike and the softmax does not see it: its gradient is the rounding
            # residue of an exact 0 (1e-17 in the float64 restatement, 1e-9 in fp32), and Adam divides a gradient by its own
            # magnitude -- either implementation walks this variable by up to (1 - beta1) / sqrt(1 - beta2) = 3.17 lr per step in
            # a direction that rounding picks.  No loss depends on it.  What holds for both: it stays within 10 such steps of P.
            # Measured on this trajectory: the float64 restatement does not move it at all (|g| = 3e-17 is far below Adam's
            # epsilon), its float32 run walks it 3.4e-4 from P (|g| = 1.6e-8), so "4 x the restatement's own fp32 error" would
            # pin a random walk to another random walk; the bound below is Adam's, not a measured one.
            for v in (got[name], ref.params[name]):
                print(name, "walked", float(np.abs(v - P[name]).max()))
                assert np.abs(v - P[name]).max() <= 10 * 3.17 * 1e-3, name
            continue
        ok, err = close(got[name], ref.params[name], rtol=2e-4, atol=2e-6)
        print(name, err)
        assert ok, (name, err)
    touched = np.unique(np.concatenate([np.concatenate([b[k].reshape(-1) for k in ("user_seq", "target_user", "target_item")]) for b in bs]))
    touched = touched[touched > 0]
    ok, err = close(got["emb_mtx"][touched], ref.params["emb_mtx"][touched], rtol=2e-4, atol=2e-6)
    print("emb_mtx", err)
    assert ok, err
    pg, lab, lg = m.eval(None, batch_tuple(bs[0]), 1e-2)
    po, lab_o, lo = ref.eval(None, batch_tuple(bs[0]), 1e-2)
    assert lab == lab_o
    assert np.abs(np.asarray(pg) - np.asarray(po)).max() < 1e-4
    assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo))


def test_training_from_a_seed():
    """keep_prob 0.8 without masks: the same seed gives the same bits, another seed another loss, eval afterwards is deterministic"""
    c = sr.Cfg(3001, *TMALL)
    P = sc.params(c)
    bs = _batches(c, 24, 3, 31)
    a, b, other = _model(c, P, seed=5), _model(c, P, seed=5), _model(c, P, seed=6)
    la = [a.train(None, batch_tuple(x), 1e-3, 1e-4, keep_prob=0.8) for x in bs]
    lb = [b.train(None, batch_tuple(x), 1e-3, 1e-4, keep_prob=0.8) for x in bs]
    lo = [other.train(None, batch_tuple(x), 1e-3, 1e-4, keep_prob=0.8) for x in bs]
    assert la == lb and _same_state(a, b)
    assert la[0] != lo[0] and all(np.isfinite(la)) and all(np.isfinite(lo))
    # dropout was on: the first step's loss differs from the loss without it
    plain = _model(c, P, seed=5).train(None, batch_tuple(bs[0]), 1e-3, 1e-4, keep_prob=1.0)
    assert plain != la[0]
    e1, e2 = a.eval(None, batch_tuple(bs[0]), 1e-4), a.eval(None, batch_tuple(bs[0]), 1e-4)
    assert e1 == e2 == b.eval(None, batch_tuple(bs[0]), 1e-4)


def test_two_fresh_models_give_the_same_bits():
    """every sum is taken in a fixed order (csrc/sasrec.hip, the queued products and column sums): no result depends on how the
    workgroups ran.  The second shape, B = 200 at T = 50, only exercises the full-size launch: no restatement is involved"""
    c, P, b, _, _, _ = _case((16, 9, 3, 4, 37))
    big_c = sr.Cfg(3000, *TMALL)
    for cc, PP, bb in ((c, P, b), (big_c, sc.params(big_c), _batches(big_c, 200, 1, 5)[0])):
        g = _pass(cc, PP, bb)
        _same_bits(g, _pass(cc, PP, bb))
        _same_bits(g, _pass(cc, PP, bb, 4096))
        assert np.isfinite(g["loss"])


def test_single_stream_gives_the_same_bits():
    """debug_flags bit 12: no second stream anywhere."""
    c = sr.Cfg(5003, *TMALL)
    P = sc.params(c)
    a, b = _model(c, P, seed=3), _model(c, P, 4096, seed=3)
    for bt in _batches(c, 24, 3, 7):
        assert a.train(None, batch_tuple(bt), 1e-3, 1e-4) == b.train(None, batch_tuple(bt), 1e-3, 1e-4)
    assert _same_state(a, b)


def test_time_tiled_optimizer_equals_the_sweep():
    c = sr.Cfg(6007, *TMALL)
    P = sc.params(c)
    tiled, swept = _model(c, P), _model(c, P)
    for m, win in ((tiled, 24), (swept, 0)):
        m.adam_tiled_min_bytes = 0
        m.adam_window = win
    bs = _batches(c, 16, 6, 9)
    for step in range(30):
        bt = batch_tuple(bs[step % len(bs)])
        assert tiled.train(None, bt, 1e-3, 1e-4, keep_prob=1.0) == swept.train(None, bt, 1e-3, 1e-4, keep_prob=1.0), step
    assert np.array_equal(tiled.get_params()["emb_mtx"], swept.get_params()["emb_mtx"])
    assert torch.equal(tiled.w, swept.w)


@pytest.mark.parametrize("keep_prob", [1.0, 0.8])
def test_captured_step_is_bit_identical_to_eager(keep_prob):
    c = sr.Cfg(4001, *TMALL)
    P = sc.params(c)
    eager, graphed = _model(c, P, seed=77), _model(c, P, seed=77)
    graphed.enable_graph(True)
    rng = np.random.default_rng(1)
    bs = [sr.random_batch(rng, c, 24, max_length=3 * c.T) for _ in range(5)]
    other = sr.random_batch(rng, c, 10, max_length=3 * c.T)
    seq = [bs[0], bs[1], bs[2], other, bs[3], other, bs[4], other, bs[0]]
    for i, b in enumerate(seq):
        le = eager.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=keep_prob)
        lg = graphed.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=keep_prob)
        assert le == lg, (i, le, lg)
    assert len([v for v in graphed._graphs.values() if isinstance(v, tuple)]) == 2
    assert _same_state(eager, graphed)
    pe, _, _ = eager.eval(None, batch_tuple(bs[1]), 1e-4)
    pg, _, _ = graphed.eval(None, batch_tuple(bs[1]), 1e-4)
    assert pe == pg


def test_lists_arrays_and_device_tensors_feed_the_same_batch():
    c = sr.Cfg(3001, 16, 32, 20, 3, 4)
    P = sc.params(c)
    ms = [_model(c, P) for _ in range(3)]
    for b in _batches(c, 16, 3, 12, max_length=60):
        arrays = batch_tuple(b)
        lists = tuple(a.tolist() for a in arrays)                  # what the reference's loader yields
        device = tuple(torch.as_tensor(a).cuda() for a in arrays)
        losses = [m.train(None, f, 1e-3, 1e-4, keep_prob=1.0) for m, f in zip(ms, (arrays, lists, device))]
        assert losses[0] == losses[1] == losses[2]
    assert _same_state(ms[0], ms[1]) and _same_state(ms[0], ms[2])
    assert len(ms[0].device_batch(batch_tuple(b)).tensors) == 8


def test_save_restore_roundtrip(tmp_path):
    c = sr.Cfg(3001, *TMALL)
    P = sc.params(c)
    m = _model(c, P)
    bs = _batches(c, 12, 3, 2)
    for b in bs[:2]:
        m.train(None, batch_tuple(b), 1e-3, 1e-4)
    m.save(None, str(tmp_path / "sasrec"))
    z = np.load(str(tmp_path / "sasrec") + ".npz")
    spec = {s[0]: s[1] for s in sr.param_spec(c)}
    spec["emb_mtx"] = (c.N, c.D)
    names = set(spec)
    assert len(names) == 15
    assert set(z.files) == names | {n + s for n in names for s in ("/Adam", "/Adam_1")} | {"beta1_power", "beta2_power", "global_step"}
    for n in names:
        for s in ("", "/Adam", "/Adam_1"):
            assert z[n + s].shape == tuple(spec[n]), (n + s, z[n + s].shape)
    assert z["ln/Variable_1"].shape == (c.Ci,) and z["multihead_attention/dense_2/kernel/Adam"].shape == (c.Ci, c.Ci)
    m2 = _model(c, sr.init_params(c, 99))
    m2.restore(None, str(tmp_path / "sasrec"))
    assert _same_state(m, m2)
    assert m.eval(None, batch_tuple(bs[2]), 1e-4) == m2.eval(None, batch_tuple(bs[2]), 1e-4)
    assert set(m2.get_params()) == names
    assert m.train(None, batch_tuple(bs[2]), 1e-3, 1e-4, keep_prob=1.0) == m2.train(None, batch_tuple(bs[2]), 1e-3, 1e-4, keep_prob=1.0)


def test_fresh_model_has_tfs_initial_values():
    from score_amd.model import SASRec
    c = sr.Cfg(500, 16, 32, 9, 3, 4)
    a, b = SASRec(*c.args, seed=5), SASRec(*c.args, seed=5)
    p = a.get_params()
    assert not p["ln/Variable"].any() and (p["ln/Variable_1"] == 1).all()
    for name, shape, init, _ in sr.param_spec(c):
        assert p[name].shape == tuple(shape), name
        if init == "glorot":
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            assert np.abs(p[name]).max() <= lim and p[name].std() > 0.4 * lim, name
        elif name.endswith("bias"):
            assert not p[name].any(), name
    assert torch.equal(a.w, b.w)


def test_bad_id_in_user_seq_raises_and_the_model_trains_on():
    c = sr.Cfg(2003, 16, 32, 6, 3, 4)
    P = sc.params(c)
    m, clean = _model(c, P), _model(c, P)
    good = _batches(c, 8, 1, 3)[0]
    bad = {k: v.copy() for k, v in good.items()}
    bad["user_seq"][1, 2, 0] = c.N + 7
    with pytest.raises(ValueError) as ei:
        m.train(None, batch_tuple(bad), 1e-3, 1e-4)
    assert "batch_data[0] (user_seq)" in str(ei.value), str(ei.value)
    assert _same_state(m, clean) and m.step == clean.step == 0          # no variable, slot or beta power was changed
    assert m.beta1_power == clean.beta1_power and m.beta2_power == clean.beta2_power
    assert m.train(None, batch_tuple(good), 1e-3, 1e-4) == clean.train(None, batch_tuple(good), 1e-3, 1e-4)
    assert _same_state(m, clean)


def test_evaluate_device_equals_host_evaluate():
    from score_amd import harness as h
    c = sr.Cfg(4001, *TMALL)
    m = _model(c, sc.params(c))
    neg, lines = 9, 4
    batches = []
    for i in range(2):
        b = _batches(c, lines * (neg + 1), 1, 40 + i)[0]
        b["label"] = (np.arange(lines * (neg + 1)) % (neg + 1) == 0).astype(np.int32)     # one positive per line
        batches.append(batch_tuple(b))
    host = h.evaluate(m, [tuple(a.tolist() for a in b) for b in batches], 1e-4, neg_sample_num=neg)
    dev = h.evaluate_device(m, batches, 1e-4, neg_sample_num=neg)
    assert np.allclose(host, dev, rtol=1e-5, atol=2e-6)
    assert m.target_item_field == 3 and np.array_equal(m.device_batch(batches[0]).tensors[5].cpu().numpy(), batches[0][3])
