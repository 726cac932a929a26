"""The SVD++ point baseline (point_model.py:167-198) on the GPU against its float64 restatement (tests/svdpp_ref.py): the
prediction, the loss, every scalar weight's gradient and the dense table gradient over the shapes of svdpp_cases.SHAPES; id 0 at
live positions; exact ties of the matrix 1-norm's maximum; a degenerate (zero-length) sample; the training trajectory with the
pad floats of the scalars' cells; and the step's other forms -- two fresh models, single stream, captured graph, time-tiled
optimizer, the three feed forms, checkpoints, bad ids, device-side evaluation -- against the plain eager step.

Tolerances are the project's for point models (tests/test_gpu_deems.py): loss 2e-5 relative to max(1, |loss|), y 1e-4, arrays and
gradients rtol 2e-4 / atol 2e-6."""
import functools

import numpy as np
import pytest
import torch

import svdpp_cases as sc
import svdpp_ref as sr
from svdpp_ref import batch_tuple
from test_gpu_gru4rec import _same_state
from test_gpu_model import close

pytestmark = pytest.mark.gpu

TMALL = sc.TMALL
_batches = sc.batches


def _model(c, P, flags=0, **kw):
    from score_amd.model import SVDpp
    m = SVDpp(*c.args, **kw)
    m.set_params(P)
    m.debug_flags = flags
    return m


def _pass(c, P, b, flags=0, reg=0.0, model=None, skip=True):
    """one forward + backward -> loss, y_pred, what the forward kernel saved, every gradient"""
    from score_amd import _lib
    m = model if model is not None else _model(c, P, flags)
    m.skip_masked_slices = skip
    B, D = len(b["label"]), c.D
    db = m.device_batch(batch_tuple(b))
    lay, ws = m.forward_backward(db, reg, 1.0)
    o, _ = _lib.workspace_field(m.cfg, B, "svdpp_act")
    act = ws[o:o + B * (4 * D + 4)].view(B, 4 * D + 4).cpu().numpy().copy()
    return dict(loss=float(ws[lay.loss].item()), y_pred=ws[lay.y_pred:lay.y_pred + B].cpu().numpy().copy(), p_u=act[:, :D],
                p_i=act[:, D:2 * D], nb=act[:, 2 * D:3 * D], share=act[:, 3 * D:4 * D], n=act[:, 4 * D], ties=act[:, 4 * D + 1],
                grads=m.get_grads(), active=db.active_slices)


def _check(got, out, want_g, what, n_vars):
    want_loss = float(out["loss"].detach())
    print(what, "loss", got["loss"], want_loss)
    assert abs(got["loss"] - want_loss) < 2e-5 * max(1.0, abs(want_loss)), (what, got["loss"], want_loss)
    err = float(np.abs(got["y_pred"] - out["y_pred"].detach().numpy()).max())
    print(what, "y_pred", err)
    assert err < 1e-4, (what, err)
    for k in ("p_u", "p_i", "nb", "n"):
        ok, err = close(got[k], out[k].detach().numpy(), rtol=2e-4, atol=2e-6)
        print(what, k, err)
        assert ok, (what, k, err)
    assert np.array_equal(got["ties"], out["ties"].numpy().astype(np.float32)), what
    assert set(got["grads"]) == set(want_g) and len(want_g) == n_vars + 1
    for k in want_g:
        assert got["grads"][k].shape == want_g[k].shape, (what, k, got["grads"][k].shape)
        ok, err = close(got["grads"][k], want_g[k], rtol=2e-4, atol=2e-6)
        print(what, k, err)
        assert ok, (what, k, err)
    assert not got["grads"]["emb_mtx"][0].any()


def _same_bits(g1, g2):
    assert g1["loss"] == g2["loss"]
    for k in ("y_pred", "p_u", "p_i", "nb", "share", "n", "ties"):
        assert np.array_equal(g1[k], g2[k]), k
    for k in g1["grads"]:
        assert np.array_equal(g1["grads"][k], g2["grads"][k]), k


@functools.lru_cache(maxsize=None)
def _case(shape):
    """a case of svdpp_cases.SHAPES and the restatement's pass over it: computed once, shared, never written to"""
    c, P, b, kept = sc.case(*shape)
    out, go = sr.loss_and_grads(c, P, b, 0.0)
    return c, P, b, kept, out, go


@pytest.mark.parametrize("D,T,Fu,Fi,B", list(sc.SHAPES))
def test_forward_backward_against_restatement(D, T, Fu, Fi, B):
    c, P, b, kept, out, go = _case((D, T, Fu, Fi, B))
    print("kept", kept.size, "of", B)
    got = _pass(c, P, b)
    _check(got, out, go, "svdpp", Fu + Fi)
    assert np.abs(go["emb_mtx"]).max() > 0
    for name, _, _, _ in sr.param_spec(c):
        assert got["grads"][name].shape == () and abs(float(go[name])) > 0, name
    if B == 3:
        assert b["user_seq_length"].tolist() == [1, 3, 7]
    if (T, B) == (7, 33):
        # every length <= 5: only the leading slices were computed; all T computed gives the same loss and gradients
        assert got["active"] == int(b["user_seq_length"].max()) < T
        allT = _pass(c, P, b, skip=False)
        assert allT["active"] == 0
        _check(allT, out, go, "svdpp, all slices", Fu + Fi)
        assert abs(allT["loss"] - got["loss"]) < 2e-5 * max(1.0, abs(got["loss"]))
        for k in go:
            ok, err = close(allT["grads"][k], got["grads"][k], rtol=2e-4, atol=2e-6)
            assert ok, (k, err)
    else:
        assert got["active"] == 0


def test_id_zero_at_live_positions():
    c, P, b, kept = sc.masked_case()
    out, go = sr.loss_and_grads(c, P, b, 0.0)
    got = _pass(c, P, b)
    _check(got, out, go, "masked rows", c.Fu + c.Fi)
    seq, ln = b["user_seq"], b["user_seq_length"]
    live = np.arange(c.T)[None, :] < ln[:, None]
    assert ((seq == 0).all(2) & live).sum() > 10          # whole live rows of the dummy id: s_t = 0 exactly, sign(0) = 0
    assert not got["grads"]["emb_mtx"][0].any()


def test_exact_ties_share_the_gradient_equally():
    c, P, b, kept = sc.tie_case()
    out, go = sr.loss_and_grads(c, P, b, 0.0)
    assert (out["ties"].numpy() == 2).all()
    got = _pass(c, P, b)
    assert (got["ties"] == 2).all(), got["ties"]           # (not vacuous: both maximal columns of every sample were found equal)
    assert np.array_equal(got["share"][:, :2], np.full((len(kept), 2), 0.5, dtype=np.float32)) and not got["share"][:, 2:].any()
    _check(got, out, go, "ties", c.Fu + c.Fi)
    # the two tied columns of a table row see the same gradient through the norm: equal bits
    g = got["grads"]["emb_mtx"]
    rows = np.unique(b["user_seq"])
    assert np.array_equal(g[rows, 0], g[rows, 1]) and np.abs(g[rows, 0]).max() > 0


def test_a_zero_length_sample_is_nan_in_eval():
    c, P, b = sc.degenerate_case()
    m = _model(c, P)
    y, lab, loss = m.eval(None, batch_tuple(b), 1e-3)
    with torch.no_grad():
        want = sr.forward(c, sr.to_torch(P), b, 1e-3)["y_pred"].numpy()
    y = np.asarray(y)
    assert np.isnan(y[2]) and np.isnan(want[2])
    others = [0, 1, 3, 4]
    assert np.isfinite(y[others]).all() and np.abs(y[others] - want[others]).max() < 1e-4
    assert np.isnan(loss)
    assert lab == b["label"].tolist() and m.step == 0


def test_ten_train_steps_against_restatement_and_adam():
    c = sr.Cfg(20011, *TMALL)
    P = sr.init_params(c, 4)
    m, ref = _model(c, P), sr.RefModel(c, P)
    bs = _batches(c, 200, 5, 8)
    for step in range(10):
        b = batch_tuple(bs[step % len(bs)])
        lg = m.train(None, b, 1e-3, 1e-2, keep_prob=1.0)
        lo = ref.train(None, b, 1e-3, 1e-2, keep_prob=1.0)
        print(step, lg, lo)
        assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo)), (step, lg, lo)
    got = m.get_params()
    for name, _, _, _ in sr.param_spec(c):
        assert got[name].shape == () and got[name] != P[name], name
        ok, err = close(got[name], ref.params[name], rtol=2e-4, atol=2e-6)
        print(name, float(got[name]), float(ref.params[name]), err)
        assert ok, (name, err)
    touched = np.unique(np.concatenate([np.concatenate([b[k].reshape(-1) for k in ("user_seq", "target_user", "target_item")]) for b in bs]))
    touched = touched[touched > 0]
    assert not np.array_equal(got["emb_mtx"][touched], P["emb_mtx"][touched])
    ok, err = close(got["emb_mtx"][touched], ref.params["emb_mtx"][touched], rtol=2e-4, atol=2e-6)
    print("emb_mtx", err)
    assert ok, err
    # every scalar's cell: the value, then three pad floats that are exactly 0 in the variable and in both Adam slots
    for flat in (m.w, m.w_m, m.w_v):
        cells = flat.cpu().numpy().reshape(c.Fu + c.Fi, 4)
        assert cells[:, 0].all() and not cells[:, 1:].any()
    pg, lab, lg = m.eval(None, batch_tuple(bs[0]), 1e-2)
    po, lab_o, lo = ref.eval(None, batch_tuple(bs[0]), 1e-2)
    assert lab == lab_o
    assert np.abs(np.asarray(pg) - np.asarray(po)).max() < 1e-4
    assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo))


def test_fresh_model_draws_truncated_normal_weights_and_zero_pads():
    from score_amd.model import SVDpp
    c = sr.Cfg(500, 16, 32, 9, 8, 8)
    a, b, other = SVDpp(*c.args, seed=5), SVDpp(*c.args, seed=5), SVDpp(*c.args, seed=6)
    cells = a.w.cpu().numpy().reshape(16, 4)
    assert cells[:, 0].all() and (np.abs(cells[:, 0]) <= 2.0).all() and len(set(cells[:, 0].tolist())) == 16 and not cells[:, 1:].any()
    assert torch.equal(a.w, b.w) and not torch.equal(a.w, other.w)


def test_two_fresh_models_give_the_same_bits():
    """every sum over the rows, the columns and the batch is taken in a fixed order (csrc/svdpp.hip, the queued column sums): no
    result depends on how the workgroups ran"""
    c, P, b, _, _, _ = _case((16, 7, 3, 4, 33))
    big = _batches(sr.Cfg(3000, *TMALL), 200, 1, 5)[0]
    for cc, bb in ((c, b), (sr.Cfg(3000, *TMALL), big)):
        PP = sr.init_params(cc, 3)
        _same_bits(_pass(cc, PP, bb), _pass(cc, PP, bb))
        _same_bits(_pass(cc, PP, bb), _pass(cc, PP, bb, 4096))


def test_single_stream_gives_the_same_bits():
    """debug_flags bit 12: no second stream anywhere."""
    c = sr.Cfg(5003, *TMALL)
    P = sr.init_params(c, 6)
    a, b = _model(c, P, seed=3), _model(c, P, 4096, seed=3)
    for bt in _batches(c, 200, 3, 7):
        assert a.train(None, batch_tuple(bt), 1e-3, 1e-4) == b.train(None, batch_tuple(bt), 1e-3, 1e-4)
    assert _same_state(a, b)


def test_time_tiled_optimizer_equals_the_sweep():
    c = sr.Cfg(6007, *TMALL)
    P = sr.init_params(c, 7)
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
    c = sr.Cfg(4001, *TMALL)
    P = sr.init_params(c, 4)
    eager, graphed = _model(c, P, seed=77), _model(c, P, seed=77)
    graphed.enable_graph(True)
    rng = np.random.default_rng(1)
    bs = [sr.random_batch(rng, c, 200, max_length=3 * c.T) for _ in range(5)]
    other = sr.random_batch(rng, c, 100, max_length=3 * c.T)
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
    c = sr.Cfg(3001, 16, 32, 20, 3, 4)
    P = sr.init_params(c, 5)
    ms = [_model(c, P) for _ in range(3)]
    for b in _batches(c, 64, 3, 12, max_length=60):
        arrays = batch_tuple(b)
        lists = tuple(a.tolist() for a in arrays)                  # what the reference's loader yields
        device = tuple(torch.as_tensor(a).cuda() for a in arrays)
        losses = [m.train(None, f, 1e-3, 1e-4, keep_prob=1.0) for m, f in zip(ms, (arrays, lists, device))]
        assert losses[0] == losses[1] == losses[2]
    assert _same_state(ms[0], ms[1]) and _same_state(ms[0], ms[2])
    assert len(ms[0].device_batch(batch_tuple(b)).tensors) == 8


def test_save_restore_roundtrip(tmp_path):
    c = sr.Cfg(3001, *TMALL)
    P = sr.init_params(c, 8)
    m = _model(c, P)
    bs = _batches(c, 50, 3, 2)
    for b in bs[:2]:
        m.train(None, batch_tuple(b), 1e-3, 1e-4)
    m.save(None, str(tmp_path / "svdpp"))
    z = np.load(str(tmp_path / "svdpp") + ".npz")
    spec = {s[0]: s[1] for s in sr.param_spec(c)}
    spec["emb_mtx"] = (c.N, c.D)
    names = set(spec)
    assert len(names) == c.Fu + c.Fi + 1
    assert set(z.files) == names | {n + s for n in names for s in ("/Adam", "/Adam_1")} | {"beta1_power", "beta2_power", "global_step"}
    for n in names:
        for s in ("", "/Adam", "/Adam_1"):
            assert z[n + s].shape == tuple(spec[n]), (n + s, z[n + s].shape)
    assert z["user_feat_w_0"].shape == () and z["item_feat_w_3/Adam_1"].shape == ()
    m2 = _model(c, sr.init_params(c, 99))
    m2.restore(None, str(tmp_path / "svdpp"))
    assert _same_state(m, m2)
    assert m.eval(None, batch_tuple(bs[2]), 1e-4) == m2.eval(None, batch_tuple(bs[2]), 1e-4)
    assert set(m2.get_params()) == names and all(m2.get_params()[n].shape == () for n in names - {"emb_mtx"})
    assert m.train(None, batch_tuple(bs[2]), 1e-3, 1e-4, keep_prob=1.0) == m2.train(None, batch_tuple(bs[2]), 1e-3, 1e-4, keep_prob=1.0)


def test_bad_id_in_user_seq_raises_and_the_model_trains_on():
    c = sr.Cfg(2003, 16, 32, 6, 3, 4)
    P = sr.init_params(c, 2)
    m, clean = _model(c, P), _model(c, P)
    good = _batches(c, 8, 1, 3)[0]
    good["user_seq_length"][:] = c.T
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
