"""The co-attention backward (csrc/embed.hip coattn_bwd_kernel_t, K <= 10) holds a unit's ids and saved scalars one
element per lane of the unit's group and hands them out by shuffles; with debug_flags bit 16 it requests them one unit
ahead: behind the pass-1 rows of the unit before, from a prologue for a wave's first unit, from a clamped unit behind
its last.  Checked here through the whole model at the smallest shapes at which that loop can go wrong.  The backward
launches at most 512 workgroups of four waves per call, so a wave gets a second unit only above 2048 * (64 / GS) units
per call (GS = lanes per unit):

* one iteration (no next unit at all), two with a nearly empty second one (the clamped request and the dropped tail in
  almost every wave), three;
* GS = 8, eight units per wave, where the next unit differs per group inside a wave: K = 3 (two registers per list) and
  K = 7 (four);
* K = 20 with F = 4 at GS = 64 (80 ids per tensor: the form every lane reads its own ids in, which K > 10 keeps);
  two slots per lane (D = 128);
* fewer computed slices than the index tensors hold (their time stride is not the computed units');
* ids outside the table, clamped to row 0 on the lane that loads them.

Every case: gradients against the oracle's autograd with the tolerances of test_gpu_ops.py test_coattn_fwd_bwd, pull-form
and atomic scatter, with and without bit 16; w_g and the table's gradient bit for bit between debug_flags 0, 65536
(bit 16) and 32768 (bit 15: every row loaded).  H = 16 keeps the batches off the per-sample whole-model kernels, which
have a backward of their own."""
import functools

import numpy as np
import pytest
import torch

from oracle import score_oracle as so
from helpers import NAMES, away_from_relu_kinks, random_batch

META_AHEAD = 65536    # score_state_t.debug_flags bit 16
ALL_ROWS = 32768      # bit 15
H, N = 16, 1500
HOPS = ("user_1hop", "user_2hop", "item_1hop", "item_2hop")

# name -> (D, Fu, Fi, K, B, T, slices computed, (fewest, most) units per call the case is about, seed)
CASES = {
    "one_iter_k7": (64, 3, 4, 7, 9, 5, 5, (1, 2048), 2),           # GS = 64 (48 and 64 slots), ragged last block
    "one_iter_k10": (64, 3, 4, 10, 9, 5, 5, (1, 2048), 1),
    "two_iter_tail": (64, 3, 4, 10, 105, 20, 20, (2049, 2100), 1),    # a handful of live units in the second iteration
    "three_iter": (64, 3, 4, 10, 230, 20, 20, (4097, 6144), 1),
    "gs8_k3": (8, 3, 3, 3, 850, 20, 20, (16385, 32768), 1),         # KMAX = 4 instance
    "gs8_k7": (8, 3, 3, 7, 850, 20, 20, (16385, 32768), 1),         # KMAX = 10 instance, K < KMAX
    "two_id_regs": (64, 3, 4, 20, 9, 5, 5, (1, 2048), 1),           # 80 ids of the F = 4 call (K > 10)
    "spl2_k10": (128, 3, 4, 10, 7, 3, 3, (1, 2048), 1),             # 96 and 128 slots: two per lane
    "short_slices": (64, 3, 4, 10, 430, 7, 5, (2049, 2150), 1),     # every length <= T - 2: index stride 7, 5 computed
    "bad_ids": (64, 3, 4, 10, 105, 20, 20, (2049, 2100), 1),        # a few ids >= N and < 0
}
BAD_IN = ("user_1hop", "item_2hop")      # feed positions 0 and 3
BAD_BITS = (1 << 0) | (1 << 3)


@functools.lru_cache(maxsize=None)
def batch_of(name):
    """(cfg, params, batch as the oracle sees it, batch as the model is fed): read-only.  The two differ in `bad_ids`
    only, where the oracle reads row 0 in place of an id outside the table."""
    D, Fu, Fi, K, B, T, slices, (lo, hi), seed = CASES[name]
    cfg = so.Cfg(N, D, H, T, K, Fu, Fi, "SCORE")
    P = so.init_params(cfg, 5)
    rng = np.random.default_rng(seed)
    b = random_batch(rng, cfg, B)            # ragged length; a fifth of the slices all-zero ids
    if slices < T:
        b["length"] = rng.integers(1, slices + 1, (B,)).astype(np.int32)
    b["length"][0] = slices
    for n in HOPS:                           # ids equal to 0 inside live slices
        b[n][rng.random(b[n].shape) < 0.1] = 0
    bad = {}
    if name == "bad_ids":
        live = np.arange(T)[None, :] < b["length"][:, None]
        for n in BAD_IN:
            bad[n] = (rng.random(b[n].shape) < 0.002) & live[:, :, None, None]
            b[n][bad[n]] = 0
    b, _, keep = away_from_relu_kinks(cfg, P, b)      # (asserts that three quarters of the batch stay)
    if keep[0] != 0:
        pytest.fail("%s: the sample that keeps every slice computed sits on a relu kink: another batch seed" % name)
    fed = {k: v.copy() for k, v in b.items()}
    for i, n in enumerate(bad):
        hit = np.nonzero(bad[n][keep].reshape(-1))[0]
        if hit.size < 4:
            pytest.fail("%s: fewer than four ids outside the table in %s: another batch seed" % (name, n))
        flat = fed[n].reshape(-1)
        flat[hit] = np.resize(np.array([N, N + 5, 10 ** 6, -3], dtype=np.int32), hit.size)
    units = len(keep) * slices
    if not lo <= units <= hi:
        pytest.fail("%s: %d units per call after the kink filter, the case needs %d .. %d" % (name, units, lo, hi))
    for v in list(P.values()) + list(b.values()) + list(fed.values()):
        v.setflags(write=False)
    return cfg, P, b, fed


@functools.lru_cache(maxsize=None)
def oracle_grads(name):
    cfg, P, b, _ = batch_of(name)
    _, go = so.loss_and_grads(cfg, P, b, 0.0)
    for v in go.values():
        v.setflags(write=False)
    return go


@pytest.mark.parametrize("name", list(CASES))
def test_case_has_its_unit_count(name):
    """the oracle alone: the kink filter leaves the case the unit count it is about (batch_of fails otherwise)"""
    cfg, _, b, fed = batch_of(name)
    slices = CASES[name][6]
    assert int(b["length"].max()) == slices and int(b["length"][0]) == slices
    print("%s: %d samples, %d units per call" % (name, len(b["label"]), len(b["label"]) * slices))
    if name == "bad_ids":
        assert all(((fed[n] < 0) | (fed[n] >= N)).sum() >= 4 for n in BAD_IN)
        assert all(np.array_equal(fed[n], b[n]) for n in NAMES if n not in BAD_IN)


def run(name, scatter_mode, flags=0):
    from score_amd.model import MODELS
    cfg, P, _, fed = batch_of(name)
    m = MODELS[cfg.model_type](cfg.N, cfg.D, cfg.H, cfg.T, cfg.K, cfg.Fu, cfg.Fi)
    m.set_params({k: v.copy() for k, v in P.items()})      # (the shared reference stays read-only)
    m.scatter_mode = scatter_mode
    m.debug_flags = flags
    db = m.device_batch(tuple(fed[n] for n in NAMES))
    assert (db.active_slices or cfg.T) == CASES[name][6]      # (0: all T)
    assert not m.persample_form(db.B, db.active_slices)      # the layer-by-layer pass: coattn_bwd_kernel_t
    m.forward_backward(db, 0.0, 1.0)
    torch.cuda.synchronize()
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_bitwise_equal_to_unit_ahead_and_to_all_rows(name):
    m = run(name, 0)
    status = int(m._id_status[0].item())
    assert status == (BAD_BITS if name == "bad_ids" else 0)
    assert bool(m.w_g.any()) and bool(m.dense_table_grad().any())
    for flags in (META_AHEAD, ALL_ROWS):
        mf = run(name, 0, flags)
        assert torch.equal(m.w_g, mf.w_g), flags
        assert torch.equal(m.dense_table_grad(), mf.dense_table_grad()), flags
        assert int(mf._id_status[0].item()) == status


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, META_AHEAD])
@pytest.mark.parametrize("scatter_mode", [0, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_against_oracle_autograd(name, scatter_mode, flags):
    cfg = batch_of(name)[0]
    go = oracle_grads(name)
    g = run(name, scatter_mode, flags).get_grads()
    Dx = (cfg.Di, cfg.Du)
    for n in sorted(go):
        got, want = np.asarray(g[n]).reshape(go[n].shape), go[n]
        err = float(np.abs(got - want).max())
        print("%s mode %d flags %d %s: max |d| %.3e, max |want| %.3e" % (name, scatter_mode, flags, n, err, np.abs(want).max()))
        assert np.allclose(got, want, rtol=2e-4, atol=2e-5), (n, err)       # (test_coattn_fwd_bwd's)
    assert not g["emb_mtx"][0].any()          # row 0 gets no gradient: ids equal to 0, and the clamped ones
    assert g["emb_mtx"].any()
    for i, n in enumerate(("dense", "dense_1")):      # a real score gradient, in the w1 and in the w2 block
        k = g[n + "/kernel"].reshape(-1)
        assert k[Dx[i]:2 * Dx[i]].any() and k[2 * Dx[i]:].any()
