"""The per-sample whole-model kernels (csrc/persample.h: one workgroup per sample runs the whole forward / backward pass
of score.py:188-224, the form SCORE / SCORE_USER / SCORE_ITEM take at the reference's own shapes, train_score.py:15-16,
285-372) against the oracle and against the layer-by-layer pass they replace (score_state_t.debug_flags bit 9 forces
that one; bits 10 / 11 mix the forms: fused forward + layered backward and the reverse).  The shapes here are the workloads';
tests/test_gpu_persample_edges.py (cases: tests/persample_cases.py) runs the same comparisons at the edges of what ps_plan_shape
admits."""
import numpy as np
import pytest
import torch

from oracle import score_oracle as so
from helpers import away_from_relu_kinks, batch_tuple, random_batch
from test_gpu_model import make_model, close, LOGIT_TOL

pytestmark = pytest.mark.gpu

# (N, D, H, T, K, Fu, Fi, B, max length): the reference's three data-set shapes (Tmall 3/4 features, Taobao 1/2, CCMR 1/5 with its
# 40 slices), cfg-2's K = 5, an eb_dim whose feature widths are not multiples of 16, a batch above 256 and a tiny one
SHAPES = [(3000, 16, 32, 11, 10, 3, 4, 200, 9), (3000, 16, 32, 8, 10, 1, 2, 100, 6), (3000, 16, 32, 40, 10, 1, 5, 24, 38),
          (2000, 16, 32, 10, 5, 3, 4, 256, 8), (1500, 12, 32, 5, 3, 2, 3, 33, 5), (1500, 8, 32, 20, 7, 3, 4, 300, 17),
          (800, 4, 32, 3, 2, 3, 4, 3, 3)]


# Arbitrary batch seeds (until round 5 this test ran on hand-picked seeds whose oracle forward pass kept every
# relu pre-activation -- co-attention, dense_3 / dense_4, fc1 / fc2: 10^5 units and more per batch -- at least 1e-5 away from the
# kink).  A relu network's gradient is discontinuous there: two correct fp32 passes whose pre-activation of ONE unit differs in
# the last bit differ by that unit's whole gradient (seen at seed 17 of one shape: one fc1 unit of one sample, 3 % of the largest
# table-row gradient).  helpers.away_from_relu_kinks drops the SAMPLES that own such a unit (every unit belongs to one sample,
# nothing crosses the batch) and the rest of the batch is compared -- on any seed.
ARBITRARY_SEEDS = (17, 101, 2024, 7, 555)


def _batch(cfg, B, maxlen, seed):
    rng = np.random.default_rng(seed)
    b = random_batch(rng, cfg, B)
    b["length"] = rng.integers(1, maxlen + 1, B).astype(np.int32)
    b["length"][0] = maxlen
    b["label"] = (np.arange(B) % 2).astype(np.int32)
    return b


def _run(m, b, flags, lam=1e-4, keep=1.0, masks=None):
    m.debug_flags = flags
    lay, ws = m.forward_backward(batch_tuple(b), lam, keep, masks)
    torch.cuda.synchronize()
    B = b["label"].shape[0]
    out = (ws[lay.y_pred:lay.y_pred + B].clone(), float(ws[lay.loss].item()), m.w_g.clone(), m.dense_table_grad().clone())
    m.debug_flags = 0
    return out


# What the oracle's forward pass alone (on the CPU, no GPU involved) drops from these tests' inputs at thr = 1e-5; the cap handed to
# away_from_relu_kinks is that count plus 2, not the helper's default quarter of the batch.  (shape index, model type) -> samples
# dropped, for test_forms_agree_and_match_the_oracle (every case not listed: 0) ...
DROPPED_FORMS = {(0, "SCORE"): 1, (1, "SCORE_USER"): 1, (1, "SCORE_ITEM"): 1, (3, "SCORE"): 1, (4, "SCORE_USER"): 1, (5, "SCORE"): 5}
# ... and (seed, shape index) -> samples dropped, for test_forms_match_the_oracle_on_arbitrary_seeds (not listed: 0)
DROPPED_ARBITRARY = {(17, 0): 1, (101, 0): 2, (2024, 0): 1, (555, 0): 2, (555, 4): 1}


def _forms_and_oracle(shape, mt, seed, adam_steps=2, counted=0):
    N, D, H, T, K, Fu, Fi, B, maxlen = shape
    cfg = so.Cfg(N, D, H, T, K, Fu, Fi, mt)
    P = so.init_params(cfg, 5)
    b_all = _batch(cfg, B, maxlen, seed)
    b, _, keep = away_from_relu_kinks(cfg, P, b_all, max_dropped=counted + 2)
    m = make_model(cfg, P)
    ref = _run(m, b, 512)
    for flags in (0, 1024, 2048):
        got = _run(m, b, flags)
        assert float((got[0] - ref[0]).abs().max()) < 2e-6, flags
        assert abs(got[1] - ref[1]) < 2e-6 * max(1.0, abs(ref[1])), flags
        for e in m.entries:
            ok, err = close(m._view(got[2], e).cpu().numpy(), m._view(ref[2], e).cpu().numpy(), rtol=3e-5, atol=3e-8)
            assert ok, (flags, e[0], err)
        ok, err = close(got[3].cpu().numpy(), ref[3].cpu().numpy(), rtol=3e-5, atol=3e-8)
        assert ok, (flags, "emb_mtx", err)
    # ... and the fused form against the oracle: gradients, then TF-Adam steps and the predictions
    m.forward_backward(batch_tuple(b), 0.0, 1.0)
    g = m.get_grads()
    oo, go = so.loss_and_grads(cfg, P, b, 0.0)
    assert oo["relu_margin"] >= 1e-5, oo["relu_margin"]        # (what away_from_relu_kinks left)
    for k in go:
        ok, err = close(g[k].reshape(np.asarray(go[k]).shape), go[k], rtol=2e-4, atol=2e-6)
        assert ok, (k, err, seed, len(keep))
    assert np.all(g["emb_mtx"][0] == 0)
    if not adam_steps:
        return
    om = so.OracleModel(cfg.N, cfg.D, cfg.H, cfg.T, cfg.K, cfg.Fu, cfg.Fi, mt, params={k: v.copy() for k, v in P.items()})
    for _ in range(adam_steps):
        lg = m.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=1.0)
        lo = om.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=1.0)
        assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo))
    # (the predictions on the WHOLE batch: a forward pass is continuous at the kinks)
    pg, _, _ = m.eval(None, batch_tuple(b_all), 1e-4)
    po, _, _ = om.eval(None, batch_tuple(b_all), 1e-4)
    assert np.abs(np.asarray(pg) - np.asarray(po)).max() < LOGIT_TOL


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mt", ["SCORE", "SCORE_USER", "SCORE_ITEM"])
def test_forms_agree_and_match_the_oracle(shape, mt):
    if mt != "SCORE" and shape[7] > 100:
        pytest.skip("the ablations' head wiring is covered at the smaller batches")
    _forms_and_oracle(shape, mt, 1000 + 37 * SHAPES.index(shape) + len(mt), counted=DROPPED_FORMS.get((SHAPES.index(shape), mt), 0))


@pytest.mark.parametrize("seed", ARBITRARY_SEEDS)
def test_forms_match_the_oracle_on_arbitrary_seeds(seed):
    """the reference's Tmall shape (B = 200: ~2 * 10^5 relu units per batch) and the odd-width shape, five seeds nobody chose"""
    _forms_and_oracle(SHAPES[0], "SCORE", seed, adam_steps=0, counted=DROPPED_ARBITRARY.get((seed, 0), 0))
    _forms_and_oracle(SHAPES[4], "SCORE", seed, adam_steps=1, counted=DROPPED_ARBITRARY.get((seed, 4), 0))


def test_the_switch_switches_and_dropout_is_the_same_mask():
    """the two forms are different code (some bit differs somewhere), and they draw the SAME dropout mask from a seed
    (element numbering of the fused head / the GEMM epilogue): predictions and gradients agree with keep_prob 0.8"""
    cfg = so.Cfg(3000, 16, 32, 6, 5, 3, 4, "SCORE")
    b = _batch(cfg, 80, 6, 3)
    m = make_model(cfg, so.init_params(cfg, 3))
    a0, a1 = _run(m, b, 0), _run(m, b, 512)
    assert not (torch.equal(a0[0], a1[0]) and torch.equal(a0[2], a1[2]) and torch.equal(a0[3], a1[3]))
    d0, d1 = _run(m, b, 0, keep=0.8), _run(m, b, 512, keep=0.8)
    assert float((d0[0] - d1[0]).abs().max()) < 2e-6 and float((d0[0] - a0[0]).abs().max()) > 1e-4
    for e in m.entries:
        ok, err = close(m._view(d0[2], e).cpu().numpy(), m._view(d1[2], e).cpu().numpy(), rtol=3e-5, atol=3e-8)
        assert ok, (e[0], err)
    rng = np.random.default_rng(1)
    masks = [(rng.random((80, 200)) < 0.8).astype(np.uint8), (rng.random((80, 80)) < 0.8).astype(np.uint8)]
    e0, e1 = _run(m, b, 0, keep=0.8, masks=masks), _run(m, b, 512, keep=0.8, masks=masks)
    assert float((e0[0] - e1[0]).abs().max()) < 2e-6
    ok, err = close(e0[3].cpu().numpy(), e1[3].cpu().numpy(), rtol=3e-5, atol=3e-8)
    assert ok, err


def test_shapes_outside_the_kernels_take_the_layered_pass():
    """H != 32, K > 10, more than 48 computed slices, B > 512, RIA / RCA / RRN: same results with and without bit 9, bit for bit
    (nothing switched), and correct against the oracle elsewhere in this suite"""
    for (N, D, H, T, K, Fu, Fi, B, mt) in [(1500, 8, 16, 4, 3, 3, 4, 20, "SCORE"), (1500, 8, 32, 4, 12, 3, 4, 20, "SCORE"),
                                           (1500, 8, 32, 50, 2, 1, 2, 8, "SCORE"), (1500, 8, 32, 3, 2, 3, 4, 600, "SCORE"),
                                           (1500, 8, 32, 4, 3, 3, 4, 20, "RIA"), (1500, 8, 32, 4, 3, 3, 4, 20, "RCA")]:
        cfg = so.Cfg(N, D, H, T, K, Fu, Fi, mt)
        b = _batch(cfg, B, T, 9)
        m = make_model(cfg, so.init_params(cfg, 2))
        a0, a1 = _run(m, b, 0), _run(m, b, 512)
        assert torch.equal(a0[0], a1[0]) and torch.equal(a0[2], a1[2]) and torch.equal(a0[3], a1[3]), (H, K, T, B, mt)


def test_bad_ids_are_reported_by_the_fused_gather():
    cfg = so.Cfg(3000, 16, 32, 6, 5, 3, 4, "SCORE")
    b = _batch(cfg, 40, 6, 4)
    m = make_model(cfg, so.init_params(cfg, 3))
    for i, name in enumerate(("user_1hop", "user_2hop", "item_1hop", "item_2hop", "target_user", "target_item")):
        bb = {k: v.copy() for k, v in b.items()}
        bb[name].reshape(-1)[0] = cfg.N + 5
        with pytest.raises(ValueError) as ei:
            m.train(None, batch_tuple(bb), 1e-3, 1e-4, keep_prob=1.0)
        assert "batch_data[%d]" % i in str(ei.value)
    l = m.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=1.0)
    assert np.isfinite(l)


@pytest.mark.parametrize("two", [False, True, "auto"])
def test_one_call_step_equals_the_call_by_call_step(two):
    """score_train_step (csrc/step.hip): the steady-state step as ONE library call -- the same entry points, arguments, streams and
    events as forward_backward + apply_adam make one by one.  Two models, one with fast_step off: the same losses (train()'s
    read-back and train_async's device scalar), predictions and optimizer state bit for bit, with right hints, a wrong hint, no
    hint, an evaluation and a table read in between, a batch of another size, and an lr change -- and the fast path did run."""
    from test_gpu_adam_tiled import make, batches, same_state
    cfg = so.Cfg(3000, 16, 32, 5, 3, 2, 3, "SCORE")
    a, b = make(cfg, 5), make(cfg, 5)
    b.fast_step = False
    # (two = True: the next batch's plan alternates between two buffers and is sorted beside the step, score_state_t.plan_workspace;
    #  "auto": by the number of occurrences per batch -- these small batches get two)
    a.plan_two_workspaces = two
    bs = batches(cfg, 6, 8, seed=33, hot_rows=150) + batches(cfg, 2, 5, seed=34, hot_rows=150)
    da, db_ = [a.device_batch(x) for x in bs], [b.device_batch(x) for x in bs]
    order = [0, 1, 2, 3, 4, 5, 0, 2, 4, 1, 3, 5, 5, 0, 1, 6, 7, 2, 3, 4, 0, 1, 2, 3, 4, 5, 0, 1]
    calls = {"n": 0}
    real = a.lib.score_train_step

    def counting(*args):
        calls["n"] += 1
        return real(*args)

    class Lib(object):
        def __getattr__(self, name):
            return counting if name == "score_train_step" else getattr(a_lib, name)
    a_lib, a.lib = a.lib, Lib()
    for i, bi in enumerate(order):
        lr = 1e-2 if i < 17 else 3e-3
        nxt = order[i + 1] if i + 1 < len(order) else 0
        hint = None if i % 9 == 8 else (nxt + 1) % 6 if i % 7 == 3 else nxt
        ha, hb = (None, None) if hint is None else (da[hint], db_[hint])
        if i % 3 == 2:
            la, lb = a.train(None, da[bi], lr, 1e-4, keep_prob=0.8, next_batch=ha), b.train(None, db_[bi], lr, 1e-4, keep_prob=0.8, next_batch=hb)
        else:
            la = float(a.train_async(da[bi], lr, 1e-4, keep_prob=0.8, next_batch=ha))
            lb = float(b.train_async(db_[bi], lr, 1e-4, keep_prob=0.8, next_batch=hb))
        assert la == lb, (i, la, lb)
        if i == 10:
            assert a.eval(None, da[4], 1e-4)[0] == b.eval(None, db_[4], 1e-4)[0]
        if i == 20:
            assert same_state(a, b), i
    assert same_state(a, b)
    assert calls["n"] >= 12, calls            # (most steps: every one whose batch was the one announced a step earlier)
    if two == "auto":
        assert a._two_buffers(da[0]) is True and a._plan_stream is not None
        a.TWO_BUFFERS_BELOW = 10
        assert a._two_buffers(da[0]) is False
    if two is True:
        assert a._plan_stream is not None
    a.lib = a_lib


@pytest.mark.parametrize("two", [True, False])
def test_six_hundred_one_call_steps_stay_bit_identical(two):
    """a soak for the orderings the one-call step relies on -- the touched-row update beside the look-ahead and the window slice
    (publish protocol), the next plan sorted beside the step into the other buffer, the loss from pinned host memory --: 600 steps
    against the call-by-call twin at a shape with ~40 K live rows, hot rows shared by consecutive batches, a short window (rows lag,
    the slice is busy), state compared every 100 steps"""
    from test_gpu_adam_tiled import make, batches, same_state
    cfg = so.Cfg(40000, 16, 32, 6, 5, 2, 3, "SCORE")
    a, b = make(cfg, 4), make(cfg, 4)
    b.fast_step = False
    a.plan_two_workspaces = two
    bs = batches(cfg, 24, 48, seed=77, hot_rows=3000)
    da, db_ = [a.device_batch(x) for x in bs], [b.device_batch(x) for x in bs]
    rng = np.random.default_rng(5)
    order = rng.integers(0, len(bs), 601).tolist()
    for i in range(600):
        bi, nx = order[i], order[i + 1]
        if i % 50 == 49:
            la = a.train(None, da[bi], 3e-3, 1e-4, keep_prob=0.8, next_batch=da[nx])
            lb = b.train(None, db_[bi], 3e-3, 1e-4, keep_prob=0.8, next_batch=db_[nx])
        else:
            la = a.train_async(da[bi], 3e-3, 1e-4, keep_prob=0.8, next_batch=da[nx])
            lb = b.train_async(db_[bi], 3e-3, 1e-4, keep_prob=0.8, next_batch=db_[nx])
            if i % 10 == 9:
                la, lb = float(la), float(lb)
            else:
                la = lb = 0.0
        assert la == lb, (i, la, lb)
        if i % 100 == 99:
            assert same_state(a, b), i
    assert same_state(a, b)
    assert a._step_args is not None and b._step_args is None and a._tiled_on()       # (the one-call step did run, on the time-tiled optimizer)
    assert (a._plan_stream is not None) == bool(two)
