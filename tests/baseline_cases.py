"""The inputs of the GRU4Rec and GCMC edge tests, built in ONE place: the GPU tests (test_gpu_gru4rec.py, test_gpu_gcmc.py) run
them, and the CPU tests (test_gru4rec_cpu.py, test_gcmc_cpu.py) rebuild exactly the same inputs and assert on the float64
restatement alone the properties that make them worth running -- a longest sample below T, a batch on the intended side of a
workgroup's share, recurrences driven to saturation under a head that is not, samples of length 0, and how many samples the
relu-kink filter takes.  Seeds were chosen on the CPU from the restatement (never from a GPU run); the CPU tests keep them honest."""
import numpy as np

import gcmc_ref as gc
import gru4rec_ref as g4
from helpers import random_batch as slice_batch

N = 3000
FRESH = 64          # the last FRESH table rows are named by the zero-length samples' sets only


def cap(B):
    """How many samples of a batch of B the kink filter may take in a baseline test.  Up to 17 samples nothing may go: those
    batches are there for their size (a workgroup of the stacked recurrence owns 16 samples)."""
    return 0 if B <= 17 else max(2, B // 50)


# ---------------------------------------------------------------------------------------------- GRU4Rec
G4R_STACK_ROWS = 16                    # samples per workgroup of gru_stack.hip
# (D, H, T, Fu, Fi, B, ML, seed): lengths drawn from [1, ML], ML < T: the pass is laid out on TA = max(length) < T slices.
# The stacked kernel's three widths and one composed-only width (H = 48); ML = 1: layer 2 one step behind a one-step layer 1;
# B = 1, 15, 16, 17 with the stacked form: below, at and just over one workgroup.
G4R_SHORT = [(16, 32, 50, 3, 4, 200, 17, 0), (16, 16, 9, 3, 4, 17, 4, 0), (16, 64, 20, 3, 4, 31, 1, 0), (8, 48, 7, 2, 2, 15, 3, 0),
             (16, 32, 50, 3, 4, 1, 5, 0), (16, 64, 20, 3, 4, 15, 6, 0), (16, 32, 50, 3, 4, 16, 9, 0), (16, 16, 9, 3, 4, 1, 2, 0)]
G4R_ZERO_LEN = (16, 32, 20, 3, 4, 35, 20, 0)       # ML == T here: ragged over [1, T], three samples of length 0
# (shape, what scales): the table x `emb` drives both recurrences to |h| -> 1; fc3 x `fc3` keeps the predictions off 0 and 1
G4R_SATURATED = [((16, 32, 12, 3, 4, 40, 12, 0), dict(emb=8.0, fc3=0.5)), ((16, 64, 6, 3, 4, 24, 4, 0), dict(emb=8.0, fc3=0.5))]
# (B, longest sample or None for T) of a trajectory on ONE model object: every "smaller after larger" transition, in B and in TA
G4R_TRAJECTORY = [(200, None), (64, 3), (200, None), (17, None), (200, 5), (1, 1), (200, None), (96, 2), (33, None), (15, 4),
                  (200, 17), (64, None)]


def zero_positions(B):
    return [0, B // 2, B - 1]


def g4r_case(D, H, T, Fu, Fi, B, ML, seed, zero_len=False, scale=None):
    """-> (cfg, params, batch after the kink filter, indices kept, batch size before)"""
    c = g4.Cfg(N, D, H, T, Fu, Fi)
    P = g4.init_params(c, 3)
    if scale:
        P["emb_mtx"] = (P["emb_mtx"] * np.float32(scale["emb"])).astype(np.float32)
        P["fc3/kernel"] = (P["fc3/kernel"] * np.float32(scale["fc3"])).astype(np.float32)
    rng = np.random.default_rng(1000 * seed + D + H + T + B)
    b = g4.random_batch(rng, g4.Cfg(N - FRESH, D, H, T, Fu, Fi), B, max_length=ML)       # (ids below the fresh rows)
    b["label"] = (np.arange(B) % 2).astype(np.int32)
    if zero_len:
        for n, i in enumerate(zero_positions(B)):
            b["user_seq_length"][i] = 0
            b["user_seq"][i] = N - FRESH + (np.arange(T * Fi).reshape(T, Fi) + n * 20) % FRESH
    bk, _, kept = g4.away_from_relu_kinks(c, P, b, max_dropped=cap(B))
    return c, P, bk, kept, B


def g4r_trajectory(c, seed=8):
    """the batches of G4R_TRAJECTORY for cfg c: the longest sample of each has exactly the listed length"""
    rng = np.random.default_rng(seed)
    out = []
    for B, ml in G4R_TRAJECTORY:
        b = g4.random_batch(rng, c, B, max_length=ml or c.T)
        b["user_seq_length"][rng.integers(0, B)] = ml or c.T
        out.append(b)
    return out


# ---------------------------------------------------------------------------------------------- GCMC
def gcmc_sb(H):
    """samples per workgroup of gcmc_head_*_kernel: 8 per group of H lanes, 256 / H groups"""
    return 8 * (256 // H)


# (D, H, T, K, Fu, Fi, B, seed): B around a workgroup's share SB (64 / 40 / 16 / 8 at H = 32 / 48 / 128 / 256), and two hidden
# sizes off the vector widths (H = 20: a multiple of 4, not of 16; H = 18: the scalar branch of gcmc_head_bwd_kernel)
GCMC_EDGES = ([(8, 32, 4, 4, 2, 3, B, 0) for B in (1, 63, 65)] + [(8, 48, 4, 4, 2, 3, B, 0) for B in (39, 41)]
              + [(8, 128, 4, 4, 2, 3, B, 0) for B in (15, 17)] + [(8, 256, 4, 4, 2, 3, B, 0) for B in (7, 9, 33)])
GCMC_ODD_H = [(8, 20, 4, 4, 2, 3, 30, 0), (8, 18, 4, 4, 2, 3, 30, 0)]
GCMC_ZERO_LEN = (16, 32, 6, 5, 3, 4, 35, 0)
# the table x `emb` saturates both recurrences; dense_4 / dense_5 x `head` keeps |a - c| small enough for y in [1e-3, 1 - 1e-3]
# (H = 32: the register recurrence at the reference's Tmall shape; H = 128: the bf16x3 one; H = 256: the streaming one)
GCMC_SATURATED = [((16, 32, 11, 10, 3, 4, 200, 0), dict(emb=4.0, head=0.2)), ((8, 128, 4, 4, 2, 3, 24, 0), dict(emb=16.0, head=0.2)),
                  ((16, 256, 4, 4, 2, 2, 20, 0), dict(emb=16.0, head=0.2))]
GCMC_TRAJECTORY = [(200, None), (64, 3), (200, None), (17, None), (200, 5), (1, 1), (200, None), (96, 2), (33, None), (15, 4),
                   (200, 7), (64, None)]


def gcmc_case(D, H, T, K, Fu, Fi, B, seed, zero_len=False, scale=None, exact=True):
    """-> (cfg, params, batch after the kink filter, indices kept, batch size before).  exact: nothing may be dropped (the
    batch is there for its size)."""
    c = gc.Cfg(N, D, H, T, K, Fu, Fi)
    P = gc.init_params(c, 3)
    if scale:
        P["emb_mtx"] = (P["emb_mtx"] * np.float32(scale["emb"])).astype(np.float32)
        for n in ("dense_4/kernel", "dense_5/kernel"):
            P[n] = (P[n] * np.float32(scale["head"])).astype(np.float32)
    rng = np.random.default_rng(1000 * seed + D + H + T + B)
    b = slice_batch(rng, gc.Cfg(N - FRESH, D, H, T, K, Fu, Fi), B)
    b["label"] = (np.arange(B) % 2).astype(np.int32)
    if zero_len:
        for n, i in enumerate(zero_positions(B)):
            b["length"][i] = 0
            b["user_1hop"][i] = N - FRESH + (np.arange(T * K * Fi).reshape(T, K, Fi) + n * 20) % FRESH
            b["item_1hop"][i] = N - FRESH + (np.arange(T * K * Fu).reshape(T, K, Fu) + n * 20 + 7) % FRESH
    bk, kept = gc.away_from_relu_kinks(c, P, b, max_dropped=0 if exact else cap(B))
    return c, P, bk, kept, B


def gcmc_trajectory(c, seed=8):
    rng = np.random.default_rng(seed)
    out = []
    for B, ml in GCMC_TRAJECTORY:
        b = slice_batch(rng, c, B)
        b["length"] = rng.integers(1, (ml or c.T) + 1, B).astype(np.int32)
        b["length"][rng.integers(0, B)] = ml or c.T
        out.append(b)
    return out
