"""The row scatter's two kernels give the same bits: pull_kernel_lanes (one occurrence per lane, the default where
score_pull_form allows it) against pull_kernel (debug_flags bit 18), through forward_backward on the same batch.

Shapes are the smallest that reach each seam of the new kernel: every window size of score_pull_window (occurrence
counts just below and above 2^18, 2^19, 2^20), lists that are no multiple of the trip (16) nor of the window, the three
group widths (D = 16, 32, 64: 4, 8, 16 lanes) with D = 128 staying on pull_kernel, runs of one occurrence, a run of
thousands of windows, runs that end exactly on a window edge, windows of dummy-row uses only, both contribution forms
(SCORE: co-attention coefficients; RCA: constant ones) and the three destinations (row id with and without row marks,
unique position of the sharded plan)."""
import numpy as np
import pytest
import torch

from oracle import score_oracle as so
from helpers import batch_tuple, random_batch

pytestmark = pytest.mark.gpu

OLD_FORM = 262144      # score_state_t.debug_flags bit 18
FU, FI = 3, 4


def n_occurrences(B, T, K):
    return B * (2 * T * K * (FU + FI) + FU + FI) + 1       # + the dummy row's sentinel


def models(cfg, seed=3):
    from score_amd.model import MODELS
    P = so.init_params(cfg, seed)
    out = []
    for flags in (0, OLD_FORM):
        m = MODELS[cfg.model_type](cfg.N, cfg.D, cfg.H, cfg.T, cfg.K, cfg.Fu, cfg.Fi)
        m.set_params(P)
        m.debug_flags = flags
        out.append(m)
    return out


def grads(m, b, scatter_mode=0):
    m.scatter_mode = scatter_mode
    m.forward_backward(batch_tuple(b), 1e-4, 1.0)
    torch.cuda.synchronize()
    return m.dense_table_grad().clone(), m.w_g.clone(), m.table_flags.clone()


def check_same_bits(cfg, b, lanes=True):
    from score_amd import _lib
    lib = _lib.load()
    m, mo = models(cfg)
    g, w, f = grads(m, b)
    assert lib.score_pull_last_form() == (1 if lanes else 0)        # the default took the kernel this test is about
    g2, w2, f2 = grads(m, b)
    assert torch.equal(g, g2) and torch.equal(w, w2) and torch.equal(f, f2)      # bit-stable run to run
    go, wo, fo = grads(mo, b)
    assert lib.score_pull_last_form() == 0
    assert torch.equal(g, go) and torch.equal(w, wo) and torch.equal(f, fo)
    assert bool(g.any()) and float(g[0].abs().max()) == 0.0         # (something was scattered; the dummy row got nothing)
    return g


# B * 2527 + 1 occurrences at T = 18, K = 10: 103 / 104 straddle 2^18 (windows of 8 / 16), 207 / 208 2^19 (16 / 32),
# 414 / 415 2^20 (32 / 64); none is a multiple of 16.  B = 3, T = 2, K = 2: 190 occurrences, 23 windows and 6 left over.
@pytest.mark.parametrize("B,T,K", [(103, 18, 10), (104, 18, 10), (207, 18, 10), (208, 18, 10), (414, 18, 10),
                                   (415, 18, 10), (3, 2, 2)])
def test_every_window_size(B, T, K):
    n = n_occurrences(B, T, K)
    assert n % 16 and n % 64
    cfg = so.Cfg(3001, 16, 16, T, K, FU, FI, "SCORE")
    b = random_batch(np.random.default_rng(B), cfg, B)
    check_same_bits(cfg, b)


@pytest.mark.parametrize("D,B,T,K,lanes", [(32, 37, 5, 4, True), (64, 37, 5, 4, True), (64, 415, 18, 10, True),
                                           (32, 208, 18, 10, True), (128, 19, 3, 4, False)])
def test_group_widths(D, B, T, K, lanes):
    # 8 and 16 lanes a group, short trips (window 8 under 16 lanes) and full ones (window 64); D = 128 (32 lanes: not
    # inside one DPP row) must stay on pull_kernel
    cfg = so.Cfg(2003, D, 16, T, K, FU, FI, "SCORE")
    b = random_batch(np.random.default_rng(D + B), cfg, B)
    check_same_bits(cfg, b, lanes)


@pytest.mark.parametrize("model_type", ["RCA", "RRN"])
def test_constant_coefficients(model_type):
    # MODE 1: no cA / cB / Wv
    cfg = so.Cfg(1009, 16, 16, 6, 5, FU, FI, model_type)
    b = random_batch(np.random.default_rng(8), cfg, 45)
    check_same_bits(cfg, b)
    cfg = so.Cfg(1009, 64, 16, 18, 10, FU, FI, model_type)
    b = random_batch(np.random.default_rng(9), cfg, 415)
    check_same_bits(cfg, b)


def _all_slots(b):
    return [b[k] for k in ("user_1hop", "user_2hop", "item_1hop", "item_2hop", "target_user", "target_item")]


def test_all_ids_distinct():
    # every run is one occurrence: a head on every lane of every trip
    B, T, K = 8, 3, 4
    n = n_occurrences(B, T, K) - 1
    cfg = so.Cfg(n + 10, 16, 16, T, K, FU, FI, "SCORE")
    rng = np.random.default_rng(1)
    b = random_batch(rng, cfg, B)
    ids = rng.permutation(np.arange(1, n + 1)).astype(np.int32)
    at = 0
    for a in _all_slots(b):
        a[...] = ids[at:at + a.size].reshape(a.shape)
        at += a.size
    b["length"][:] = T
    g = check_same_bits(cfg, b)
    assert int((g != 0).any(dim=1).sum()) > n // 2


@pytest.mark.parametrize("D", [16, 64])
def test_one_constant_column(D):
    # one feature of user_1hop is the same id in the whole batch: 74,700 uses, over a thousand windows of 64 in one run
    # (far beyond LONG_CHAIN), and the same of a target column
    B, T, K = 415, 18, 10
    cfg = so.Cfg(3001, D, 16, T, K, FU, FI, "SCORE")
    b = random_batch(np.random.default_rng(5), cfg, B, zero_frac=0.0)
    b["user_1hop"][..., 0] = 7
    b["target_user"][:, 1] = 11
    g = check_same_bits(cfg, b)
    assert bool(g[7].any()) and bool(g[11].any())


def test_runs_end_on_window_edges():
    # 568 sorted keys, windows of 8: eight of the dummy row (seven uses and the sentinel), then 50 rows with eight uses
    # each and 10 rows with sixteen -- every run starts and ends exactly on a window edge
    B, T, K = 9, 2, 2
    n = n_occurrences(B, T, K)
    assert n == 568
    cfg = so.Cfg(101, 16, 16, T, K, FU, FI, "SCORE")
    rng = np.random.default_rng(2)
    b = random_batch(rng, cfg, B, zero_frac=0.0)
    b["length"][:] = T
    pool = np.concatenate([np.repeat(np.arange(1, 51), 8), np.repeat(np.arange(51, 61), 16)]).astype(np.int32)
    assert pool.size == n - 8
    pool = rng.permutation(pool)
    slots = _all_slots(b)
    flat = np.concatenate([np.zeros(7, np.int32), pool])       # the seven dummy-row uses land in user_1hop
    at = 0
    for a in slots:
        a[...] = flat[at:at + a.size].reshape(a.shape)
        at += a.size
    assert sum(int((a == 0).sum()) for a in slots) == 7
    check_same_bits(cfg, b)


def test_dummy_row_windows():
    # ragged lengths from 0 and 1 up, the slices past a sample's length all dummy-row ids: most of the sorted list is
    # key 0, whole windows of it return early, the window where it ends drops its partial sum
    B, T, K = 60, 6, 5
    cfg = so.Cfg(1501, 16, 16, T, K, FU, FI, "SCORE")
    rng = np.random.default_rng(4)
    b = random_batch(rng, cfg, B)
    b["length"] = (np.arange(B) % (T + 1)).astype(np.int32)       # 0, 1, ..., T, 0, 1, ...
    for k in ("user_1hop", "user_2hop", "item_1hop", "item_2hop"):
        for s in range(B):
            b[k][s, b["length"][s]:] = 0
    check_same_bits(cfg, b)


def test_unique_position_destinations():
    # scatter_mode 2 (the sharded plan on one rank): a run's destination is its unique position, read per occurrence;
    # the mini-table gradients of the two kernels are the same bits
    from score_amd import _lib
    from score_amd.dist import ShardedSCORE

    class OneRank(object):
        rank, world = 0, 1

        def exchange_counts(self, send_counts, device, extra=None):
            return list(send_counts) if extra is None else (list(send_counts), [extra])

        def all_to_all(self, out, inp, out_splits, in_splits):
            out.copy_(inp)

        def all_reduce_sum(self, t):
            pass

    lib = _lib.load()
    cfg_args = (3001, 64, 16, 5, 4, FU, FI)
    cfg = so.Cfg(*cfg_args, model_type="SCORE")
    P = so.init_params(cfg, 6)
    b = random_batch(np.random.default_rng(6), cfg, 37)
    got = []
    for flags in (0, 0, OLD_FORM):
        m = ShardedSCORE(*cfg_args, comm=OneRank(), model_type="SCORE")
        m.backend.m.set_params(P)
        m.backend.m.debug_flags = flags
        kept = []
        inner = m.backend.backward

        def backward(*a, **kw):
            r = inner(*a, **kw)
            kept.append(r[0] if isinstance(r, tuple) else r)
            return r
        m.backend.backward = backward
        m.forward_backward(batch_tuple(b), 1e-4, 1.0)
        torch.cuda.synchronize()
        assert lib.score_pull_last_form() == (0 if flags else 1)
        got.append((kept[0].clone(), m.backend.m.w_g.clone()))
    assert bool(got[0][0].any())
    for g, w in got[1:]:
        assert torch.equal(got[0][0], g) and torch.equal(got[0][1], w)
