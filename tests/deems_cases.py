"""The inputs of the DEEMS GPU tests (tests/test_gpu_deems.py), built in one place so that tests/test_deems_cpu.py can judge the
same inputs on the float64 restatement alone: the kink filter (deems_ref.away_from_kinks) may take at most cap(B) samples of a
case, and the seeds below are fixed so that it does."""
import numpy as np

import deems_ref as er

TMALL = (16, 32, 50, 3, 4)          # D, H, T, Fu, Fi of the reference's point-model run (train_time_point_models.py:15-35)

# (D, H, T, Fu, Fi, B) -> (batch seed, per-side minimum lengths, per-side maximum lengths or None = up to 3 T, forced lengths).
# One position, one sample | zero and over-long lengths, different per side | head widths 28 and 20: neither K loop of the head
# fills a 16-step chunk | a ragged last 16-row tile, twice | every length <= 5 (active_slices is taken) | the grouped launch at
# H = 64 | H = 48: no register kernel, one call per side | the Tmall point shape | CCMR's widths (Ci = 80)
SHAPES = {(4, 16, 1, 1, 1, 1): (0, (1, 1), (3, 3), None),
          (4, 16, 3, 2, 1, 3): (0, (1, 1), (3, 3), ((0, 2, 7), (7, 0, 2))),
          (4, 16, 5, 3, 1, 5): (0, (1, 1), None, None),
          (16, 16, 9, 3, 4, 33): (0, (1, 1), None, None),
          (16, 16, 9, 3, 4, 37): (0, (1, 1), None, None),
          (16, 32, 7, 3, 4, 33): (0, (1, 1), (5, 5), None),
          (16, 64, 9, 1, 2, 17): (0, (1, 1), None, None),
          (16, 48, 9, 3, 4, 20): (0, (1, 1), None, None),
          (16, 32, 50, 3, 4, 200): (0, (1, 1), None, None),
          (16, 32, 50, 1, 5, 100): (0, (1, 1), None, None)}
DROPOUT_SHAPE = (16, 32, 9, 3, 4, 33)       # the explicit-mask case (keep_prob 0.8)
DROPOUT_SEED = 0


def params(c, seed=3):
    """TF's initial values, every bias and beta moved by 0.1 N(0, 1)"""
    return er.init_params(c, seed, bias_scale=0.1)


def case(D, H, T, Fu, Fi, B):
    """cfg, parameters, the batch behind the kink filter, kept"""
    seed, lo, hi, forced = SHAPES[(D, H, T, Fu, Fi, B)]
    c = er.Cfg(3000, D, H, T, Fu, Fi)
    P = params(c)
    rng = np.random.default_rng(100 + seed)
    b = er.random_batch(rng, c, B, min_length=lo, max_length=hi or (3 * T, 3 * T))
    if forced is not None:
        b["user_seq_length"] = np.array(forced[0], dtype=np.int32)
        b["item_seq_length"] = np.array(forced[1], dtype=np.int32)
    b["label"] = (np.arange(B) % 2).astype(np.int32)
    b, _, kept = er.away_from_kinks(c, P, b)
    return c, P, b, kept


def dropout_case(keep_prob=0.8):
    """cfg, parameters, batch, masks [2, B', 200] / [2, B', 80] behind the kink filter, kept"""
    D, H, T, Fu, Fi, B = DROPOUT_SHAPE
    c = er.Cfg(3000, D, H, T, Fu, Fi)
    P = params(c)
    rng = np.random.default_rng(200 + DROPOUT_SEED)
    b = er.random_batch(rng, c, B, max_length=(3 * T, 3 * T))
    masks = [(rng.random((2, B, n)) < keep_prob).astype(np.uint8) for n in (200, 80)]
    b, masks, kept = er.away_from_kinks(c, P, b, keep_prob, masks)
    return c, P, b, masks, kept


def batches(c, B, n, seed, **kw):
    rng = np.random.default_rng(seed)
    kw.setdefault("max_length", (3 * c.T, 3 * c.T))
    return [er.random_batch(rng, c, B, **kw) for _ in range(n)]
