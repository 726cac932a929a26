"""The GRU4Rec point baseline (point_model.py:123-138) on the GPU against its float64 restatement (tests/gru4rec_ref.py):
the pass, its gradients and its training trajectory, in both forms of the two stacked recurrences -- the stacked kernel
(csrc/gru_stack.hip) and the composed form (debug_flags bit 13: one layer per launch, the projection GEMM between them) --
and the step's other forms -- single stream, time-tiled optimizer, captured graph, the three feed forms, checkpoints, bad
ids, device-side evaluation -- against the plain eager step."""
import pickle

import numpy as np
import pytest
import torch

import baseline_cases as bc
import gru4rec_ref as gr
from gru4rec_ref import batch_tuple
from test_gpu_model import close

pytestmark = pytest.mark.gpu

TMALL = (16, 32, 50, 3, 4)          # D, H, T, Fu, Fi of the reference's point-model run (train_time_point_models.py:15-35)
COMPOSED = 8192                     # debug_flags bit 13

# (D, H, T, Fu, Fi, B): the reference's three datasets' widths; H = 16 and H = 64 with a ragged last workgroup (a workgroup owns
# 16 samples; B = 37 is there because the kink filter below takes one of the 33); and two hidden sizes the stacked kernel does
# not cover (the composed form either way)
SHAPES = [(16, 32, 50, 3, 4, 200), (16, 32, 50, 1, 5, 100), (16, 32, 50, 1, 2, 100), (16, 16, 9, 3, 4, 33), (16, 16, 9, 3, 4, 37),
          (16, 64, 20, 3, 4, 64), (8, 48, 7, 2, 2, 40), (64, 128, 12, 3, 4, 96)]


def _model(c, P, flags=0, **kw):
    from score_amd.model import GRU4Rec
    m = GRU4Rec(*c.args, **kw)
    m.set_params(P)
    m.debug_flags = flags
    return m


def _batches(c, B, n, seed, **kw):
    rng = np.random.default_rng(seed)
    return [gr.random_batch(rng, c, B, **kw) for _ in range(n)]


def _same_state(a, b):
    return (torch.equal(a.w, b.w) and torch.equal(a.table, b.table) and torch.equal(a.w_m, b.w_m)
            and torch.equal(a.w_v, b.w_v) and torch.equal(a.table_m, b.table_m) and torch.equal(a.table_v, b.table_v))


def _pass(c, P, b, flags, reg=0.0, keep_prob=1.0, masks=None):
    """one forward + backward -> loss, y_pred, both layers' outputs over the computed slices, every gradient"""
    from score_amd import _lib
    m = _model(c, P, flags)
    B, TA = len(b["label"]), min(int(b["user_seq_length"].max()), c.T)
    lay, ws = m.forward_backward(batch_tuple(b), reg, keep_prob, dropout_masks=masks)
    o = _lib.workspace_field(m.cfg, B, "gru_out")
    outs = [ws[x:x + B * TA * c.H].view(B, TA, c.H).cpu().numpy().copy() for x in o]
    return dict(loss=float(ws[lay.loss].item()), y=ws[lay.y_pred:lay.y_pred + B].cpu().numpy().copy(), o1=outs[0], o2=outs[1],
                grads=m.get_grads())


def _check(got, want_loss, want_y, want_o1, want_o2, want_g, what):
    print(what, "loss", got["loss"], want_loss, "max |dy|", float(np.abs(got["y"] - want_y).max()))
    assert abs(got["loss"] - want_loss) < 2e-5 * max(1.0, abs(want_loss)), (what, got["loss"], want_loss)
    assert np.abs(got["y"] - want_y).max() < 1e-4, what
    TA = got["o1"].shape[1]
    for k, w in (("o1", want_o1), ("o2", want_o2)):
        ok, err = close(got[k], w[:, :TA], rtol=2e-4, atol=2e-6)
        print(what, k, err)
        assert ok, (what, k, err)
    assert set(got["grads"]) == set(want_g)
    for k in want_g:
        ok, err = close(got["grads"][k].reshape(want_g[k].shape), want_g[k], rtol=2e-4, atol=2e-6)
        print(what, k, err)
        assert ok, (what, k, err)


@pytest.mark.parametrize("D,H,T,Fu,Fi,B", SHAPES)
def test_forward_backward_against_restatement(D, H, T, Fu, Fi, B):
    c = gr.Cfg(3000, D, H, T, Fu, Fi)
    P = gr.init_params(c, 3)
    b = _batches(c, B, 1, D + H + T)[0]
    b["label"] = (np.arange(B) % 2).astype(np.int32)
    b, _, kept = gr.away_from_relu_kinks(c, P, b, max_dropped=max(2, B // 50))
    print("kept", kept.size, "of", B)
    out, go = gr.loss_and_grads(c, P, b, 0.0)
    want = (float(out["loss"].detach()), out["y_pred"].detach().numpy(), out["o1"].detach().numpy(), out["o2"].detach().numpy(), go)
    stacked = _pass(c, P, b, 0)
    composed = _pass(c, P, b, COMPOSED)
    _check(stacked, *want, "default")
    _check(composed, *want, "bit 13")
    # ... and the two forms against each other (they sum in different orders: not bit for bit)
    _check(stacked, composed["loss"], composed["y"], composed["o1"], composed["o2"], composed["grads"], "default vs bit 13")


def _want(c, P, b):
    out, go = gr.loss_and_grads(c, P, b, 0.0)
    return out, (float(out["loss"].detach()), out["y_pred"].detach().numpy(), out["o1"].detach().numpy(), out["o2"].detach().numpy(), go)


def _both_forms(c, P, b, want):
    """both forms of the recurrences against the restatement and against each other (_check: loss, y, o1, o2, every gradient)"""
    stacked = _pass(c, P, b, 0)
    composed = _pass(c, P, b, COMPOSED)
    _check(stacked, *want, "default")
    _check(composed, *want, "bit 13")
    _check(stacked, composed["loss"], composed["y"], composed["o1"], composed["o2"], composed["grads"], "default vs bit 13")
    for got in (stacked, composed):
        assert all(np.isfinite(v).all() for v in got["grads"].values()) and np.isfinite(got["loss"])
    return stacked, composed


@pytest.mark.parametrize("D,H,T,Fu,Fi,B,ML,seed", bc.G4R_SHORT)
def test_short_batches_against_restatement(D, H, T, Fu, Fi, B, ML, seed):
    """active_slices < T: the gather, the hoisted projection, both recurrences, the workspace and every backward product are
    laid out on TA = max(length) slices.  Also the stacked form's workgroup edges (16 samples each): B = 1, 15, 16, 17, 31.
    (tests/test_gru4rec_cpu.py proves the inputs: longest sample below T, batch size after the kink filter.)"""
    c, P, b, kept, _ = bc.g4r_case(D, H, T, Fu, Fi, B, ML, seed)
    Bk = len(b["label"])
    print("kept", Bk, "of", B, "longest", int(b["user_seq_length"].max()))
    m = _model(c, P)
    assert m.device_batch(batch_tuple(b)).active_slices == int(b["user_seq_length"].max()) < c.T
    out, want = _want(c, P, b)
    stacked, _ = _both_forms(c, P, b, want)
    assert stacked["o1"].shape[1] == int(b["user_seq_length"].max())
    # the same batch with every slice computed: the skip changes the sums' shapes, not the result
    m_all = _model(c, P)
    m_all.skip_masked_slices = False
    assert m_all.device_batch(batch_tuple(b)).active_slices == 0
    lay, ws = m_all.forward_backward(batch_tuple(b), 0.0, 1.0)
    la, ya = float(ws[lay.loss].item()), ws[lay.y_pred:lay.y_pred + Bk].cpu().numpy()
    assert abs(stacked["loss"] - la) < 2e-6 * max(1.0, abs(la)), (stacked["loss"], la)
    assert np.abs(stacked["y"] - ya).max() < 2e-6 * max(1.0, float(np.abs(ya).max()))
    # eval() on the short batch
    for flags in (0, COMPOSED):
        pg, lab, _ = _model(c, P, flags).eval(None, batch_tuple(b), 1e-4)
        po, lab_o, _ = gr.RefModel(c, P).eval(None, batch_tuple(b), 1e-4)
        assert lab == lab_o and np.abs(np.asarray(pg) - np.asarray(po)).max() < 1e-4


def test_samples_of_length_zero_against_restatement():
    """dynamic_rnn with sequence_length 0: zero outputs and a zero final state.  Three samples of the batch (the first, one in
    the middle, the last), the rest ragged; the table rows only they name get no gradient."""
    c, P, b, kept, B = bc.g4r_case(*bc.G4R_ZERO_LEN, zero_len=True)
    zero = np.nonzero(b["user_seq_length"] == 0)[0]
    assert zero.size == 3 and zero[0] == 0 and zero[-1] == len(b["label"]) - 1
    out, want = _want(c, P, b)
    for got in _both_forms(c, P, b, want):
        assert not got["o1"][zero].any() and not got["o2"][zero].any()
        assert not got["grads"]["emb_mtx"][c.N - bc.FRESH:].any() and not got["grads"]["emb_mtx"][0].any()


@pytest.mark.parametrize("shape,scale", bc.G4R_SATURATED)
def test_saturated_recurrences_against_restatement(shape, scale):
    """The table scaled until layer 1's states reach |h| > 0.999 (the fast sigmoid / tanh forms of gru_stack.hip and gru.hip at
    the ends of their range), fc3 scaled down so that every prediction stays in [1e-3, 1 - 1e-3]: beyond that the reference's
    own float32 log(1 - y + 1e-7) loses its precision and float64 stops being a fair yardstick (test_gru4rec_cpu.py asserts
    both conditions on the restatement).  The bounds are the unsaturated ones."""
    c, P, b, kept, B = bc.g4r_case(*shape, scale=scale)
    out, want = _want(c, P, b)
    assert float(out["o1"].detach().abs().max()) > 0.999
    _both_forms(c, P, b, want)


_TRAJ = {}


def _reference_trajectory():
    """the restatement's side of the trajectory tests, once for both forms"""
    if not _TRAJ:
        c = gr.Cfg(20011, *TMALL)
        P = gr.init_params(c, 4)
        bs = bc.g4r_trajectory(c)
        ref = gr.RefModel(c, P)
        losses = [ref.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=1.0) for b in bs]
        _TRAJ.update(c=c, P=P, bs=bs, losses=losses, params=ref.params, evals=[ref.eval(None, batch_tuple(b), 1e-4)[0] for b in (bs[0], bs[1])])
    return _TRAJ


@pytest.mark.parametrize("flags", [0, COMPOSED])
def test_trajectory_whose_shape_changes_every_step(flags):
    """Twelve train() steps on ONE model object whose B and active slices change from step to step, every "smaller after
    larger" transition among them: the workspace is reused under a different layout each time (and parts of it are relied on
    to hold zeros), and so are the per-shape caches.  Default configuration: two streams, time-tiled optimizer where it applies."""
    t = _reference_trajectory()
    c, bs = t["c"], t["bs"]
    m = _model(c, t["P"], flags)
    seen = []
    for step, (b, lo) in enumerate(zip(bs, t["losses"])):
        seen.append((len(b["label"]), m.device_batch(batch_tuple(b)).active_slices))
        lg = m.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=1.0)
        print(step, seen[-1], lg, lo)
        assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo)), (step, seen[-1], lg, lo)
    assert seen == [(B, 0 if ml is None else ml) for B, ml in bc.G4R_TRAJECTORY]
    for b, po in zip((bs[0], bs[1]), t["evals"]):
        pg, _, _ = m.eval(None, batch_tuple(b), 1e-4)
        assert np.abs(np.asarray(pg) - np.asarray(po)).max() < 1e-4
    got, steps = m.get_params(), len(bs)
    assert set(got) == set(t["params"])
    # the bound of test_gpu_gcmc.py::test_virtual_ranks_match_single_device, on the same two bodies: the dense variables, the table
    dense = sorted(k for k in got if k != "emb_mtx")
    for what, keys in (("dense", dense), ("emb_mtx", ["emb_mtx"])):
        d = np.concatenate([np.abs(got[k].reshape(-1) - t["params"][k].reshape(-1)) for k in keys])
        print(what, float((d <= 3e-6).mean()), float(d.max()))
        assert (d <= 3e-6).mean() > 0.999 and d.max() <= 2.2 * steps * 1e-3, what


def test_form_taken_per_hidden_size():
    """H in {16, 32, 64} have the stacked kernel; bit 13 and every other H run the composed form, whose per-layer kernels leave
    layer 2's hoisted projection in its workspace region (the stacked kernel never writes it)."""
    from score_amd import _lib
    for H, flags, stacked in ((32, 0, True), (32, COMPOSED, False), (48, 0, False), (64, 0, True), (16, 0, True)):
        c = gr.Cfg(500, 8, H, 6, 2, 2)
        m = _model(c, gr.init_params(c, 1), flags)
        b = _batches(c, 20, 1, 3)[0]
        b["user_seq_length"][0] = c.T
        B = 20
        ws = m._workspace(B)[1]
        _, x2 = _lib.workspace_field(m.cfg, B, "xproj")
        ws[x2:x2 + B * c.T * 3 * H].fill_(float("nan"))
        m.forward_backward(batch_tuple(b), 0.0, 1.0)
        torch.cuda.synchronize()
        written = not bool(torch.isnan(ws[x2:x2 + B * c.T * 3 * H]).any().item())
        assert written == (not stacked), (H, flags)


@pytest.mark.parametrize("flags", [0, COMPOSED])
def test_lengths_above_T_and_ids_past_the_length(flags):
    c = gr.Cfg(4000, 16, 32, 50, 3, 4)
    P = gr.init_params(c, 11)
    B = 48
    rng = np.random.default_rng(17)
    b = gr.random_batch(rng, c, B)
    b["user_seq"] = rng.integers(1, c.N - 600, (B, c.T, c.Fi)).astype(np.int32)
    b["target_user"] = rng.integers(1, c.N - 600, (B, c.Fu)).astype(np.int32)
    b["target_item"] = rng.integers(1, c.N - 600, (B, c.Fi)).astype(np.int32)
    ln = rng.integers(1, c.T + 1, B)
    ln[:6] = [1, c.T, c.T + 1, 120, 300, 2]
    b["user_seq_length"] = ln.astype(np.int32)
    m = _model(c, P, flags)
    lay, ws = m.forward_backward(batch_tuple(b), 1e-4, 1.0)
    loss, y, g = float(ws[lay.loss].item()), ws[lay.y_pred:lay.y_pred + B].cpu().numpy().copy(), m.get_grads()
    # a length above T behaves as T, bit for bit
    bc = dict(b, user_seq_length=np.minimum(ln, c.T).astype(np.int32))
    m2 = _model(c, P, flags)
    lay, ws = m2.forward_backward(batch_tuple(bc), 1e-4, 1.0)
    assert float(ws[lay.loss].item()) == loss and np.array_equal(ws[lay.y_pred:lay.y_pred + B].cpu().numpy(), y)
    g2 = m2.get_grads()
    assert all(np.array_equal(g[k], g2[k]) for k in g)
    # ids past a sample's length, changed to ids nothing else names: the same loss and predictions bit for bit, and no gradient
    # on the rows only they name
    bd = {k: v.copy() for k, v in b.items()}
    fresh = iter(range(c.N - 600, c.N))
    only_dead = []
    for i in range(B):
        for t in range(min(int(ln[i]), c.T), c.T):
            if len(only_dead) < 590:
                r = next(fresh)
                bd["user_seq"][i, t, :] = r
                only_dead.append(r)
    assert len(only_dead) > 100
    m3 = _model(c, P, flags)
    lay, ws = m3.forward_backward(batch_tuple(bd), 1e-4, 1.0)
    assert float(ws[lay.loss].item()) == loss and np.array_equal(ws[lay.y_pred:lay.y_pred + B].cpu().numpy(), y)
    g3 = m3.get_grads()
    assert not g3["emb_mtx"][np.array(only_dead)].any() and not g3["emb_mtx"][0].any()
    assert all(np.array_equal(g[k], g3[k]) for k in g if k != "emb_mtx")
    # ... and against the restatement, lengths above T included
    out, go = gr.loss_and_grads(c, P, b, 1e-4)
    assert abs(loss - float(out["loss"].detach())) < 2e-5 * max(1.0, abs(float(out["loss"].detach())))
    assert np.abs(y - out["y_pred"].detach().numpy()).max() < 1e-4


@pytest.mark.parametrize("flags", [0, COMPOSED])
def test_ten_train_steps_against_restatement_and_adam(flags):
    c = gr.Cfg(20011, *TMALL)
    P = gr.init_params(c, 4)
    m, ref = _model(c, P, flags), gr.RefModel(c, P)
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


@pytest.mark.parametrize("flags", [0, COMPOSED])
def test_one_step_with_explicit_dropout_masks(flags):
    c = gr.Cfg(3000, *TMALL)
    P = gr.init_params(c, 3)
    B = 200
    b = _batches(c, B, 1, 21)[0]
    rng = np.random.default_rng(22)
    masks = [(rng.random((B, 200)) < 0.8).astype(np.uint8), (rng.random((B, 80)) < 0.8).astype(np.uint8)]
    b, masks, kept = gr.away_from_relu_kinks(c, P, b, keep_prob=0.8, dropout_masks=masks, max_dropped=max(2, B // 50))
    print("kept", kept.size, "of", B)
    # (reg_lambda 0: get_grads() is the data term's gradient; the L2 term's is added by the optimizer step, test above)
    out, go = gr.loss_and_grads(c, P, b, 0.0, 0.8, masks)
    got = _pass(c, P, b, flags, reg=0.0, keep_prob=0.8, masks=masks)
    _check(got, float(out["loss"].detach()), out["y_pred"].detach().numpy(), out["o1"].detach().numpy(), out["o2"].detach().numpy(),
           go, "dropout 0.8")
    # ... and as a training step with the L2 term: its loss, and the loss of the step after it (which sees the update)
    m, ref = _model(c, P, flags), gr.RefModel(c, P)
    for kp, dm in ((0.8, masks), (1.0, None)):
        lg = m.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=kp, dropout_masks=dm)
        lo = ref.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=kp, dropout_masks=dm)
        print("train", kp, lg, lo)
        assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo)), (kp, lg, lo)


def _write_point_files(d, rng, lines, T, Fu, Fi):
    """synthetic target / history / feature-dictionary files; -> (paths, feature_size)"""
    U, I = 40, 90
    users, items = np.arange(1, U + 1), np.arange(U + 1, U + I + 1)
    nfeat = 25
    N = U + I + 1 + nfeat
    with open(str(d / "target.txt"), "w") as ft, open(str(d / "hist.txt"), "w") as fh:
        for _ in range(lines):
            ft.write("%d,%s\n" % (rng.choice(users), ",".join(str(x) for x in rng.choice(items, 2, replace=False))))
            fh.write(",".join(str(x) for x in rng.choice(items, int(rng.integers(1, 3 * T)))) + "\n")
    uf = {str(u): [int(x) for x in rng.integers(U + I + 1, N, Fu - 1)] for u in users}
    itf = {str(i): [int(x) for x in rng.integers(U + I + 1, N, Fi - 1)] for i in items}
    for name, dct in (("uf.pkl", uf), ("if.pkl", itf)):
        with open(str(d / name), "wb") as f:
            pickle.dump(dct, f)
    return (str(d / "target.txt"), str(d / "hist.txt"), str(d / "uf.pkl"), str(d / "if.pkl")), N


def test_forty_steps_through_the_point_loader_and_feed(tmp_path):
    from score_amd.pointdata import DataLoaderUserSeq
    T, Fu, Fi, B = 12, 2, 3, 32
    (tf, hf, uf, itf), N = _write_point_files(tmp_path, np.random.default_rng(31), 16 * 5 + 3, T, Fu, Fi)
    c = gr.Cfg(N, 16, 32, T, Fu, Fi)
    P = gr.init_params(c, 3)
    m, ref = _model(c, P), gr.RefModel(c, P)
    batches = list(DataLoaderUserSeq(B, T, tf, hf, 1, uf, itf))
    assert len(batches) == 5 and batches[0][0].shape == (B, T, Fi) and int(max(b[1].max() for b in batches)) > T
    step = 0
    for db, host in zip(m.feed(batches * 8), batches * 8):
        lg = m.train(None, db, 1e-3, 1e-4, keep_prob=1.0)
        lo = ref.train(None, host, 1e-3, 1e-4, keep_prob=1.0)
        assert abs(lg - lo) < 1e-3 * max(abs(lo), 1e-6), (step, lg, lo)
        step += 1
    assert step == 40
    print("last losses", lg, lo)


def test_single_stream_gives_the_same_bits():
    """debug_flags bit 12: no second stream anywhere."""
    c = gr.Cfg(5003, *TMALL)
    P = gr.init_params(c, 6)
    a, b = _model(c, P), _model(c, P, 4096)
    for bt in _batches(c, 200, 3, 7):
        assert a.train(None, batch_tuple(bt), 1e-3, 1e-4) == b.train(None, batch_tuple(bt), 1e-3, 1e-4)
    assert _same_state(a, b)


def test_time_tiled_optimizer_equals_the_sweep():
    c = gr.Cfg(6007, *TMALL)
    P = gr.init_params(c, 7)
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
    c = gr.Cfg(4001, *TMALL)
    P = gr.init_params(c, 4)
    eager, graphed = _model(c, P, seed=77), _model(c, P, seed=77)
    graphed.enable_graph(True)
    rng = np.random.default_rng(1)
    bs = [gr.random_batch(rng, c, 200) for _ in range(5)]
    other = gr.random_batch(rng, c, 100)
    for b in bs + [other]:
        b["user_seq_length"][0] = c.T                              # (every batch computes all T slices: one graph per batch size)
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
    c = gr.Cfg(3001, 16, 32, 20, 3, 4)
    P = gr.init_params(c, 5)
    ms = [_model(c, P) for _ in range(3)]
    for b in _batches(c, 64, 3, 12, max_length=60):
        arrays = batch_tuple(b)
        lists = tuple(a.tolist() for a in arrays)                  # what the reference's loader yields
        device = tuple(torch.as_tensor(a).cuda() for a in arrays)
        losses = [m.train(None, f, 1e-3, 1e-4, keep_prob=1.0) for m, f in zip(ms, (arrays, lists, device))]
        assert losses[0] == losses[1] == losses[2]
    assert _same_state(ms[0], ms[1]) and _same_state(ms[0], ms[2])


def test_wrong_tuple_or_shape_raises_naming_the_point_field():
    c = gr.Cfg(500, 16, 32, 10, 3, 4)
    m = _model(c, gr.init_params(c, 1))
    b = _batches(c, 8, 1, 2)[0]
    with pytest.raises(ValueError, match="5-tuple"):
        m.train(None, batch_tuple(b) + (b["label"],), 1e-3, 1e-4)
    with pytest.raises(ValueError, match="5-tuple"):
        m.eval(None, batch_tuple(b)[:4], 1e-4)
    for field, wrong in (("user_seq", b["user_seq"][:, :-1]), ("user_seq_length", b["user_seq_length"][:-1]),
                         ("target_user", b["target_user"][:, :-1]), ("target_item", np.concatenate([b["target_item"]] * 2, 1))):
        for conv in (lambda a: a, lambda a: a.tolist(), lambda a: torch.as_tensor(a).cuda()):
            bad = dict(b, **{field: wrong})
            with pytest.raises(ValueError) as ei:
                m.device_batch(tuple(conv(a) for a in batch_tuple(bad)))
            assert "batch_data[%d] (%s)" % (gr.FEED.index(field), field) in str(ei.value), str(ei.value)
    assert m.step == 0


def test_save_restore_roundtrip(tmp_path):
    c = gr.Cfg(3001, *TMALL)
    P = gr.init_params(c, 8)
    m = _model(c, P)
    bs = _batches(c, 50, 3, 2)
    for b in bs[:2]:
        m.train(None, batch_tuple(b), 1e-3, 1e-4)
    m.save(None, str(tmp_path / "gru4rec"))
    z = np.load(str(tmp_path / "gru4rec") + ".npz")
    names = {"emb_mtx"} | {s[0] for s in gr.param_spec(c)}
    assert set(z.files) == names | {n + s for n in names for s in ("/Adam", "/Adam_1")} | {"beta1_power", "beta2_power", "global_step"}
    m2 = _model(c, gr.init_params(c, 99))
    m2.restore(None, str(tmp_path / "gru4rec"))
    assert m.eval(None, batch_tuple(bs[2]), 1e-4) == m2.eval(None, batch_tuple(bs[2]), 1e-4)
    assert set(m2.get_params()) == names
    assert m.train(None, batch_tuple(bs[2]), 1e-3, 1e-4) == m2.train(None, batch_tuple(bs[2]), 1e-3, 1e-4)


@pytest.mark.parametrize("field,where,named", [("user_seq", (1, 2, 0), "batch_data[0] (user_seq)"),
                                               ("target_item", (0, 1), "batch_data[3] (target_item)"),
                                               ("target_user", (3, 0), "batch_data[2] (target_user)")])
def test_bad_id_raises_and_the_model_trains_on(field, where, named):
    c = gr.Cfg(2003, 16, 32, 6, 3, 4)
    P = gr.init_params(c, 2)
    m, clean = _model(c, P), _model(c, P)
    good = _batches(c, 8, 1, 3)[0]
    good["user_seq_length"][:] = c.T
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
    c = gr.Cfg(4001, *TMALL)
    m = _model(c, gr.init_params(c, 3))
    neg, lines = 99, 4
    batches = []
    for i in range(2):
        b = _batches(c, lines * (neg + 1), 1, 40 + i)[0]
        b["label"] = (np.arange(lines * (neg + 1)) % (neg + 1) == 0).astype(np.int32)     # one positive per line
        batches.append(batch_tuple(b))
    host = h.evaluate(m, [tuple(a.tolist() for a in b) for b in batches], 1e-4, neg_sample_num=neg)
    dev = h.evaluate_device(m, batches, 1e-4, neg_sample_num=neg)
    assert np.allclose(host, dev, rtol=1e-5, atol=2e-6)
    # the ranking metrics read the target item ids of the model's own field, batch_data[3]: with the ids of batch_data[2] (all
    # from one range too) the two would still agree, so check the column itself
    assert m.target_item_field == 3 and np.array_equal(m.device_batch(batches[0]).tensors[5].cpu().numpy(), batches[0][3])


def test_sharded_training_refuses_the_point_model():
    from score_amd.dist import ShardedSCORE
    with pytest.raises(ValueError, match="GRU4Rec"):
        ShardedSCORE(1000, 16, 32, 50, 1, 3, 4, comm=object(), model_type="GRU4Rec")
