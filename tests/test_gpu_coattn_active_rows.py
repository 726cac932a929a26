"""The co-attention backward (csrc/embed.hip coattn_bwd_kernel_t) loads, for the w1 / w2 gradients, only the seq1 / seq2
rows of the neighbours whose relu'd score is > 0; the load of an inactive one goes to the all-zero row 0.  Checked here
through the whole model at the smallest shapes of every geometry the kernel has (several units per wave, one unit per
wave, two slots per lane; K below and at the instance's KMAX), in three activity regimes set through the co-attention
biases, against

* the same build with debug_flags bit 15 (every row loaded, the form before): bit for bit, pull-form scatter;
* the oracle's autograd, with the tolerances of test_gpu_ops.py test_coattn_fwd_bwd, pull-form and atomic scatter;
* the rows the atomic scatter must reach: an inactive neighbour's row still gets p_k g1 (seq1) or g2 / K (seq2).

H = 16 keeps these batches off the per-sample whole-model kernels (H = 32 only), which have a backward of their own.
K = 3 runs in the KMAX = 4 instance (score_coattn_bwd_multi sends K <= 4 there); K = 7 is the K < KMAX case of the
KMAX = 10 instance."""
import functools

import numpy as np
import pytest
import torch

from oracle import score_oracle as so
from helpers import away_from_relu_kinks, random_batch

pytestmark = pytest.mark.gpu

ALL_ROWS = 32768      # score_state_t.debug_flags bit 15
H, N = 16, 1500

# name -> (D, Fu, Fi, K, B, T).  Units per block of the backward: 4 waves x (64 / GS); B * T is never a multiple of it.
SHAPES = {
    "gs8_k3": (8, 3, 3, 3, 37, 5),        # GS = 8: eight units per wave, activity differs inside a wave; 6 of 8 lanes own a slot
    "gs8_k7": (8, 3, 3, 7, 37, 5),        # K < KMAX = 10
    "gs8_k10": (8, 3, 3, 10, 61, 5),      # more than one block per call
    "gs8_k20": (8, 3, 3, 20, 21, 4),
    "gs64_k7": (64, 3, 4, 7, 9, 5),       # GS = 64, the cfg-3 geometry (48 and 64 slots)
    "gs64_k10": (64, 3, 4, 10, 9, 5),
    "gs64_k20": (64, 3, 4, 20, 5, 3),
    "spl2_k10": (128, 3, 4, 10, 7, 3),    # 96 and 128 slots: two per lane
    "spl2_k20": (128, 3, 4, 20, 5, 3),
}
REGIMES = ("active", "inactive", "mixed")
# w_t.tgt + w_1.seq1_k + w_2.seq2_k has a standard deviation of about sqrt(2) under init_params (three dot products of
# variance <= 2 / 3 each): 20 is fourteen of them, and test_regime_is_what_it_says asserts that no score crosses
BIAS = {"active": 20.0, "inactive": -20.0}
MIXED_SEED = 5


def make_model(cfg, params):
    from score_amd.model import MODELS
    m = MODELS[cfg.model_type](cfg.N, cfg.D, cfg.H, cfg.T, cfg.K, cfg.Fu, cfg.Fi)
    m.set_params(params)
    return m


def batch_tuple(b):
    from helpers import NAMES
    return tuple(b[n] for n in NAMES)


@functools.lru_cache(maxsize=None)
def case(shape, regime):
    """(cfg, params, batch, oracle grads, active fraction): computed once per (shape, regime), read-only afterwards."""
    D, Fu, Fi, K, B, T = SHAPES[shape]
    cfg = so.Cfg(N, D, H, T, K, Fu, Fi, "SCORE")
    P = so.init_params(cfg, MIXED_SEED)
    if regime != "mixed":
        P["dense/bias"][:] = BIAS[regime]
        P["dense_1/bias"][:] = BIAS[regime]
    rng = np.random.default_rng(B * 131 + K)
    b = random_batch(rng, cfg, B)            # ragged length; a fifth of the slices all-zero ids
    b["length"][0] = T                       # (every slice is computed)
    for name in ("user_1hop", "user_2hop", "item_1hop", "item_2hop"):      # ids equal to 0 inside live slices
        hit = rng.random(b[name].shape) < 0.1
        b[name][hit] = 0
    b, _, keep = away_from_relu_kinks(cfg, P, b)
    if keep[0] != 0:
        pytest.fail("the sample that keeps every slice computed sits on a relu kink: another batch seed")
    per_block = 4 * (64 // min(64, 1 << int(np.ceil(np.log2(Fu * D // 4)))))
    if (len(keep) * T) % per_block == 0:     # the last block stays ragged
        b = {k: np.ascontiguousarray(v[:-1]) for k, v in b.items()}
    out, go = so.loss_and_grads(cfg, P, b, 0.0)
    info = out["atten_info"].detach().numpy()      # [B, T, 4K]: K r of call 0, ..., K r of call 1, ...
    live = (np.arange(T)[None, :] < b["length"][:, None])
    r = np.concatenate([info[..., :K][live], info[..., 2 * K:3 * K][live]])
    for v in list(P.values()) + list(b.values()) + list(go.values()):
        v.setflags(write=False)
    return cfg, P, b, go, float((r > 0).mean())


def run(cfg, P, b, scatter_mode, flags=0):
    m = make_model(cfg, {k: v.copy() for k, v in P.items()})      # (the shared reference stays read-only)
    m.scatter_mode = scatter_mode
    m.debug_flags = flags
    db = m.device_batch(batch_tuple(b))
    assert not m.persample_form(db.B, db.active_slices)      # the layer-by-layer pass: coattn_bwd_kernel_t
    m.forward_backward(db, 0.0, 1.0)
    torch.cuda.synchronize()
    return m


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_regime_is_what_it_says(shape, regime):
    frac = case(shape, regime)[4]
    print("%s %s: active fraction %.3f" % (shape, regime, frac))
    if regime == "active":
        assert frac == 1.0
    elif regime == "inactive":
        assert frac == 0.0
    else:
        assert 0.2 < frac < 0.8


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bitwise_equal_to_all_rows(shape, regime):
    cfg, P, b, _, _ = case(shape, regime)
    m = run(cfg, P, b, 0)
    ma = run(cfg, P, b, 0, ALL_ROWS)
    assert torch.equal(m.w_g, ma.w_g)
    assert torch.equal(m.dense_table_grad(), ma.dense_table_grad())
    assert bool(m.dense_table_grad().any())


@pytest.mark.parametrize("scatter_mode", [0, 1])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_oracle_autograd(shape, regime, scatter_mode):
    cfg, P, b, go, _ = case(shape, regime)
    m = run(cfg, P, b, scatter_mode)
    g = m.get_grads()
    Dx = (cfg.Di, cfg.Du)
    for name in sorted(go):
        got, want = np.asarray(g[name]).reshape(go[name].shape), go[name]
        err = float(np.abs(got - want).max())
        print("%s %s mode %d %s: max |d| %.3e, max |want| %.3e" % (shape, regime, scatter_mode, name, err, np.abs(want).max()))
        assert np.allclose(got, want, rtol=2e-4, atol=2e-5), (name, err)       # (test_coattn_fwd_bwd's)
    assert not g["emb_mtx"][0].any()
    if regime == "inactive":      # dz = 0 everywhere: no score gradient at all, exactly
        for i, name in enumerate(("dense", "dense_1")):
            assert not g[name + "/kernel"].any() and not g[name + "/bias"].any()
            assert not go[name + "/kernel"].any()
    else:                         # ... and a real one otherwise, in the w1 and in the w2 block
        for i, name in enumerate(("dense", "dense_1")):
            k = g[name + "/kernel"].reshape(-1)
            assert k[Dx[i]:2 * Dx[i]].any() and k[2 * Dx[i]:].any()


@pytest.mark.parametrize("regime", ["inactive", "mixed"])
@pytest.mark.parametrize("shape", ["gs8_k10", "gs64_k7", "spl2_k20"])
def test_atomic_scatter_reaches_rows_of_inactive_neighbours(shape, regime):
    # the pattern check of test_scatter_modes_agree_and_pull_is_deterministic, and the oracle's pattern: with no active
    # neighbour at all (`inactive`) EVERY neighbour row's gradient is p_k g1 or g2 / K alone
    cfg, P, b, go, frac = case(shape, regime)
    g0 = run(cfg, P, b, 0).dense_table_grad()
    g1 = run(cfg, P, b, 1).dense_table_grad()
    assert float((g0 - g1).abs().max()) <= 2e-5 * float(g0.abs().max())
    nz0, nz1 = (g0 != 0).any(dim=1).cpu().numpy(), (g1 != 0).any(dim=1).cpu().numpy()
    assert np.array_equal(nz0, nz1)
    assert np.array_equal(nz1, (go["emb_mtx"] != 0).any(axis=1))
    live = np.arange(cfg.T)[None, :] < b["length"][:, None]
    rows = np.unique(np.concatenate([b[n][live].ravel() for n in ("user_1hop", "user_2hop", "item_1hop", "item_2hop")]))
    rows = rows[rows != 0]
    assert rows.size > 100 and nz1[rows].all()
