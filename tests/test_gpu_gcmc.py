"""The GCMC slice baseline (slice_model.py:177-203) on the GPU against its float64 restatement (tests/gcmc_ref.py): the
pass, its gradients and its training trajectory, and the step's other forms -- single stream, time-tiled optimizer,
captured graph, row-sharded ranks, checkpoints, bad ids, device-side evaluation -- against the plain eager step."""
import numpy as np
import pytest
import torch

import baseline_cases as bc
import gcmc_ref as gr
from helpers import NAMES, batch_tuple, random_batch
from test_gpu_model import close

pytestmark = pytest.mark.gpu

TMALL = (16, 32, 11, 10, 3, 4)          # D, H, T, K, Fu, Fi of the reference's slice-model run (train_time_slice_models.py)


def _model(c, P, **kw):
    from score_amd.model import GCMC
    m = GCMC(*c.args, **kw)
    m.set_params(P)
    return m


def _batches(c, B, n, seed):
    rng = np.random.default_rng(seed)
    return [random_batch(rng, c, B) for _ in range(n)]


def _same_state(a, b):
    return (torch.equal(a.w, b.w) and torch.equal(a.table, b.table) and torch.equal(a.w_m, b.w_m)
            and torch.equal(a.w_v, b.w_v) and torch.equal(a.table_m, b.table_m) and torch.equal(a.table_v, b.table_v))


@pytest.mark.parametrize("D,H,T,K,Fu,Fi,B", [
    (16, 32, 11, 10, 3, 4, 200),     # the reference's Tmall shape
    (16, 32, 40, 10, 1, 5, 64),      # CCMR
    (8, 48, 5, 6, 2, 2, 40),         # Fu == Fi: both sides' projections in one grouped launch
    (64, 128, 6, 10, 3, 4, 96),      # cfg-3 widths
    (32, 256, 4, 4, 2, 2, 32),       # H = 256: the streaming recurrence
])
def test_forward_backward_against_restatement(D, H, T, K, Fu, Fi, B):
    c = gr.Cfg(3000, D, H, T, K, Fu, Fi)
    P = gr.init_params(c, 3)
    b = _batches(c, B, 1, D + H + T)[0]
    b["label"] = (np.arange(B) % 2).astype(np.int32)
    b, _ = gr.away_from_relu_kinks(c, P, b, max_dropped=max(2, B // 50))
    _parity(c, P, b)


def _parity(c, P, b):
    """one forward + backward against the restatement: loss, predictions, the per-side activations, every gradient"""
    from score_amd import _lib
    Bk, TA = len(b["label"]), max(int(b["length"].max()), 1)
    m = _model(c, P)
    lay, ws = m.forward_backward(batch_tuple(b), 0.0, 1.0)
    out, go = gr.loss_and_grads(c, P, b, 0.0)
    loss, want = float(ws[lay.loss].item()), float(out["loss"].detach())
    y = ws[lay.y_pred:lay.y_pred + Bk].cpu().numpy()
    print("B", Bk, "TA", TA, "loss", loss, want, "max |dy|", float(np.abs(y - out["y_pred"].detach().numpy()).max()))
    assert abs(loss - want) < 2e-5 * max(1.0, abs(want)), (loss, want)
    assert np.abs(y - out["y_pred"].detach().numpy()).max() < 1e-4
    # the per-side activations A and Z, [B * active slices, Dx], in their workspace regions
    for f, keys in (("gcmc_a", ("a_u", "a_i")), ("gcmc_z", ("z_u", "z_i"))):
        offs = _lib.workspace_field(m.cfg, Bk, f)
        for o, k, Dx in zip(offs, keys, (c.Di, c.Du)):
            got = ws[o:o + Bk * TA * Dx].view(Bk, TA, Dx).cpu().numpy()
            ok, err = close(got, out[k][:, :TA].detach().numpy(), rtol=2e-4, atol=2e-6)
            assert ok, (k, err)
    g = m.get_grads()
    assert set(g) == set(go)
    for k in go:
        assert np.isfinite(g[k]).all(), k
        ok, err = close(g[k].reshape(go[k].shape), go[k], rtol=2e-4, atol=2e-6)
        print(k, err)
        assert ok, (k, err)
    return out, g


@pytest.mark.parametrize("D,H,T,K,Fu,Fi,B,seed", bc.GCMC_EDGES + bc.GCMC_ODD_H)
def test_workgroup_edges_and_odd_hidden_sizes_against_restatement(D, H, T, K, Fu, Fi, B, seed):
    """gcmc_head_*_kernel owns SB = 8 * (256 / H) samples per workgroup: B = 1, SB - 1 and SB + 1 for each covered layout (and
    B = 4 SB + 1 at H = 256); and two hidden sizes off the vector widths -- H = 20 (a multiple of 4, not of 16) and H = 18 (the
    scalar branch of gcmc_head_bwd_kernel; every product of the pass then takes its GEMM's unaligned form).  The kink filter
    takes nothing from these batches (tests/test_gcmc_cpu.py), so the B that runs is the B listed."""
    c, P, b, kept, _ = bc.gcmc_case(D, H, T, K, Fu, Fi, B, seed)
    assert len(b["label"]) == B
    _parity(c, P, b)


def test_samples_of_length_zero_against_restatement():
    """dynamic_rnn with sequence_length 0: a zero final state on both sides, so a = c = 0 and y = 1 / 2 for those samples; no
    gradient reaches the table rows only they name."""
    c, P, b, kept, B = bc.gcmc_case(*bc.GCMC_ZERO_LEN, zero_len=True, exact=False)
    zero = np.nonzero(b["length"] == 0)[0]
    assert zero.size == 3 and zero[0] == 0 and zero[-1] == len(b["label"]) - 1
    out, g = _parity(c, P, b)
    assert not g["emb_mtx"][c.N - bc.FRESH:].any() and not g["emb_mtx"][0].any()
    m = _model(c, P)
    pg, _, _ = m.eval(None, batch_tuple(b), 1e-4)
    assert np.abs(np.asarray(pg)[zero] - 0.5).max() < 1e-6


@pytest.mark.parametrize("shape,scale", bc.GCMC_SATURATED)
def test_saturated_recurrences_against_restatement(shape, scale):
    """The table scaled until both recurrences' final states reach |h| > 0.999 (the fast sigmoid / tanh forms of the register,
    bf16x3 and streaming kernels at the ends of their range), dense_4 / dense_5 scaled down so that every prediction stays in
    [1e-3, 1 - 1e-3] and |a|, |c| < 80 (tests/test_gcmc_cpu.py asserts the conditions on the restatement; beyond them the
    reference's own float32 log(1 - y + 1e-7) is no yardstick).  The bounds are the unsaturated ones."""
    c, P, b, kept, B = bc.gcmc_case(*shape, scale=scale, exact=False)
    out, _ = _parity(c, P, b)
    assert min(float(out["h_u"].detach().abs().max()), float(out["h_i"].detach().abs().max())) > 0.999


def test_trajectory_whose_shape_changes_every_step():
    """Twelve train() steps on ONE model object whose B and active slices change from step to step, every "smaller after
    larger" transition among them: the workspace is reused under a different layout each time, and so are the per-shape
    caches.  Default configuration."""
    c = gr.Cfg(20011, *TMALL)
    P = gr.init_params(c, 4)
    m, ref = _model(c, P), gr.RefModel(c, P)
    bs = bc.gcmc_trajectory(c)
    seen = []
    for step, b in enumerate(bs):
        seen.append((len(b["label"]), m.device_batch(batch_tuple(b)).active_slices))
        lg = m.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=1.0)
        lo = ref.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=1.0)
        print(step, seen[-1], lg, lo)
        assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo)), (step, seen[-1], lg, lo)
    assert seen == [(B, 0 if ml is None else ml) for B, ml in bc.GCMC_TRAJECTORY]
    for b in (bs[0], bs[1]):
        pg, _, _ = m.eval(None, batch_tuple(b), 1e-4)
        po, _, _ = ref.eval(None, batch_tuple(b), 1e-4)
        assert np.abs(np.asarray(pg) - np.asarray(po)).max() < 1e-4
    # the bound of test_virtual_ranks_match_single_device, on the same two bodies: the dense variables, the table
    got, steps = m.get_params(), len(bs)
    assert set(got) == set(ref.params)
    dense = sorted(k for k in got if k != "emb_mtx")
    for what, keys in (("dense", dense), ("emb_mtx", ["emb_mtx"])):
        d = np.concatenate([np.abs(got[k].reshape(-1) - ref.params[k].reshape(-1)) for k in keys])
        print(what, float((d <= 3e-6).mean()), float(d.max()))
        assert (d <= 3e-6).mean() > 0.999 and d.max() <= 2.2 * steps * 1e-3, what


def test_ten_train_steps_against_restatement_and_adam():
    c = gr.Cfg(20011, *TMALL)
    P = gr.init_params(c, 4)
    m, ref = _model(c, P), gr.RefModel(c, P)
    bs = _batches(c, 200, 5, 8)
    for step in range(10):
        b = batch_tuple(bs[step % len(bs)])
        lg = m.train(None, b, 1e-3, 1e-4, keep_prob=1.0)
        lo = ref.train(None, b, 1e-3, 1e-4, keep_prob=1.0)
        assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo)), (step, lg, lo)
    pg, lab, _ = m.eval(None, batch_tuple(bs[0]), 1e-4)
    po, lab_o, _ = ref.eval(None, batch_tuple(bs[0]), 1e-4)
    assert lab == lab_o
    assert np.abs(np.asarray(pg) - np.asarray(po)).max() < 1e-4


from test_gpu_cfg1 import pipeline, _loader      # noqa: E402,F401  (module fixture: the bundled Tmall sample)


def test_forty_steps_on_the_tmall_sample_through_the_device_loader(pipeline):
    cf, g, r, targets = pipeline
    T = cf["time_slice_num"] - cf["start_time"] - 1
    c = gr.Cfg(r["feature_size"], cf["eb_dim"], cf["hidden_size"], T, cf["obj_per_time_slice"], cf["user_fnum"], cf["item_fnum"])
    P = gr.init_params(c, 3)
    m, ref = _model(c, P), gr.RefModel(c, P)
    train = list(_loader(cf, g, targets, "train", 32))
    assert len(train) >= 2
    for step in range(40):
        db = train[step % len(train)]
        host = tuple(t.cpu().numpy() for t in db.tensors)
        lg = m.train(None, tuple(db.tensors), 1e-3, 1e-4, keep_prob=1.0)
        lo = ref.train(None, host, 1e-3, 1e-4, keep_prob=1.0)
        assert abs(lg - lo) < 1e-3 * max(abs(lo), 1e-6), (step, lg, lo)


def test_keep_prob_has_no_effect():
    c = gr.Cfg(4001, *TMALL)
    P = gr.init_params(c, 5)
    a, b = _model(c, P), _model(c, P)
    for bt in _batches(c, 200, 3, 1):
        assert a.train(None, batch_tuple(bt), 1e-3, 1e-4, keep_prob=0.8) == b.train(None, batch_tuple(bt), 1e-3, 1e-4, keep_prob=1.0)
    assert _same_state(a, b)


def test_skipped_masked_slices_agree_with_the_full_pass():
    c = gr.Cfg(4000, 16, 32, 8, 6, 3, 4)
    P = gr.init_params(c, 4)
    m, m_all = _model(c, P), _model(c, P)
    m_all.skip_masked_slices = False
    b = _batches(c, 64, 1, 23)[0]
    b["length"] = np.random.default_rng(2).integers(1, 6, 64).astype(np.int32)      # longest sample: 5 of T = 8
    assert m.device_batch(batch_tuple(b)).active_slices == int(b["length"].max()) < c.T
    for _ in range(3):
        lg = m.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=1.0)
        la = m_all.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=1.0)
        assert abs(lg - la) < 2e-6 * max(1.0, abs(la)), (lg, la)
    pg, _, _ = m.eval(None, batch_tuple(b), 1e-4)
    pa, _, _ = m_all.eval(None, batch_tuple(b), 1e-4)
    assert np.abs(np.asarray(pg) - np.asarray(pa)).max() < 2e-6


@pytest.mark.parametrize("B,T", [(200, 11), (1024, 8)])
def test_single_stream_gives_the_same_bits(B, T):
    """debug_flags bit 12: no second stream anywhere.  (1024 x 8 rows: the dense gradient's finishers and the loss reduction
    go to the side stream in the default form)"""
    c = gr.Cfg(5003, 16, 32, T, 10, 3, 4)
    P = gr.init_params(c, 6)
    a, b = _model(c, P), _model(c, P)
    b.debug_flags = 4096
    for bt in _batches(c, B, 3, 7):
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
    bs = [random_batch(rng, c, 200) for _ in range(5)]
    for b in bs:
        b["length"] = np.full(200, 9, dtype=np.int32)
    other = random_batch(rng, c, 100)
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


def test_save_restore_roundtrip(tmp_path):
    c = gr.Cfg(3001, *TMALL)
    P = gr.init_params(c, 8)
    m = _model(c, P)
    bs = _batches(c, 50, 3, 2)
    for b in bs[:2]:
        m.train(None, batch_tuple(b), 1e-3, 1e-4)
    m.save(None, str(tmp_path / "gcmc"))
    m2 = _model(c, gr.init_params(c, 99))
    m2.restore(None, str(tmp_path / "gcmc"))
    assert m.eval(None, batch_tuple(bs[2]), 1e-4) == m2.eval(None, batch_tuple(bs[2]), 1e-4)
    assert set(m2.get_params()) == {"emb_mtx"} | {s[0] for s in gr.param_spec(c)}
    assert m.train(None, batch_tuple(bs[2]), 1e-3, 1e-4) == m2.train(None, batch_tuple(bs[2]), 1e-3, 1e-4)


def test_virtual_ranks_match_single_device():
    from score_amd.dist import ShardedSCORE
    from test_gpu_dist import run_ranks
    world, B, steps = 2, 12, 4
    c = gr.Cfg(5001, 16, 32, 5, 10, 3, 4)
    params = gr.init_params(c, 5)
    batches = [[random_batch(np.random.default_rng(100 * r + s), c, B) for s in range(steps)] for r in range(world)]

    def fn(rank, comm):
        m = ShardedSCORE(*c.args, comm=comm, model_type="GCMC")
        m.backend.m.set_params(params)
        bts = [batch_tuple(b) for b in batches[rank]]
        losses = [m.train(None, bt, 1e-3, 1e-3, keep_prob=1.0, next_batch=bts[i + 1] if i + 1 < len(bts) else None)
                  for i, bt in enumerate(bts)]
        pred, _, _ = m.eval(None, batch_tuple(batches[rank][0]), 1e-3)
        torch.cuda.synchronize()
        return losses, m.backend.m.table.cpu().numpy(), m.backend.m.w.cpu().numpy(), pred

    res = run_ranks(world, fn)
    ref = _model(c, params)
    for s in range(steps):
        cat = tuple(np.concatenate([batches[r][s][n] for r in range(world)]) for n in NAMES)
        lref = ref.train(None, cat, 1e-3, 1e-3, keep_prob=1.0)
        for r in range(world):
            assert abs(res[r][0][s] - lref) < 2e-5 * max(1.0, abs(lref)), (s, r, res[r][0][s], lref)
    assert np.array_equal(res[0][2], res[1][2])
    wref = ref.w.cpu().numpy()
    assert (np.abs(res[0][2] - wref) <= 3e-6).mean() > 0.999 and np.abs(res[0][2] - wref).max() <= 2.2 * steps * 1e-3
    full = np.zeros((c.N, c.D), dtype=np.float32)
    for r in range(world):
        n_r = len(range(r, c.N, world))
        full[r::world] = res[r][1][:n_r]
    d = np.abs(full - ref.table.cpu().numpy())
    assert (d <= 3e-6).mean() > 0.999 and d.max() <= 2.2 * steps * 1e-3
    for r in range(world):
        pr, _, _ = ref.eval(None, batch_tuple(batches[r][0]), 1e-3)
        assert np.abs(np.asarray(res[r][3]) - np.asarray(pr)).max() < 1e-4


@pytest.mark.parametrize("field,where", [("user_1hop", (1, 2, 3, 0)), ("target_item", (0, 1))])
def test_bad_id_raises_and_the_model_trains_on(field, where):
    c = gr.Cfg(2003, 16, 32, 6, 5, 3, 4)
    P = gr.init_params(c, 2)
    m, clean = _model(c, P), _model(c, P)
    good = _batches(c, 8, 1, 3)[0]
    bad = {k: v.copy() for k, v in good.items()}
    bad[field][where] = c.N + 7
    with pytest.raises(ValueError) as ei:
        m.train(None, batch_tuple(bad), 1e-3, 1e-4)
    assert "(%s)" % field in str(ei.value)
    assert _same_state(m, clean) and m.step == clean.step == 0          # no variable was updated
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
