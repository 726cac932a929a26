"""The inputs of the DELF GPU tests (tests/test_gpu_delf.py), built in one place so that tests/test_delf_cpu.py can judge the
same inputs on the float64 restatement alone."""
import numpy as np

import delf_ref as dr

TMALL = (16, 32, 50, 3, 4)          # D, H, T, Fu, Fi of the reference's point-model run (train_time_point_models.py:15-35)

# (D, T, Fu, Fi, B) -> (batch seed, per-side minimum lengths, per-side maximum lengths or None = up to 3 T, forced lengths).
# One position, one sample, C below a wave | Cu != Ci with lengths {0, 2, 7} | Tmall | CCMR (Ci = 80: no power of two) | Taobao |
# every length <= 5 on both sides (active_slices is taken) | Ci = 128, the width limit | long T
SHAPES = {(4, 1, 1, 1, 1): (0, (1, 1), (3, 3), None),
          (4, 3, 2, 1, 3): (0, (1, 1), (3, 3), ((0, 2, 7), (7, 0, 2))),
          (16, 50, 3, 4, 200): (0, (1, 1), None, None),
          (16, 50, 1, 5, 100): (0, (1, 1), None, None),
          (16, 50, 1, 2, 100): (0, (1, 1), None, None),
          (16, 7, 3, 4, 33): (0, (1, 1), (5, 5), None),
          (32, 50, 1, 4, 17): (0, (1, 1), None, None),
          (8, 120, 2, 2, 40): (0, (1, 1), None, None)}


def case(D, T, Fu, Fi, B):
    """cfg, parameters (TF's initial values, the biases moved by 0.1 N(0, 1)), the batch behind the kink filter, kept"""
    seed, lo, hi, forced = SHAPES[(D, T, Fu, Fi, B)]
    c = dr.Cfg(3000, D, 32, T, Fu, Fi)
    P = dr.init_params(c, 3)
    rng = np.random.default_rng(100 + seed)
    for n in P:
        if "bias" in n:
            P[n] = (P[n] + 0.1 * rng.standard_normal(P[n].shape)).astype(np.float32)
    b = dr.random_batch(rng, c, B, min_length=lo, max_length=hi or (3 * T, 3 * T))
    if forced is not None:
        b["user_seq_length"] = np.array(forced[0], dtype=np.int32)
        b["item_seq_length"] = np.array(forced[1], dtype=np.int32)
    b["label"] = (np.arange(B) % 2).astype(np.int32)
    b, kept = dr.away_from_kinks(c, P, b)
    return c, P, b, kept


def batches(c, B, n, seed, **kw):
    rng = np.random.default_rng(seed)
    kw.setdefault("max_length", (3 * c.T, 3 * c.T))
    return [dr.random_batch(rng, c, B, **kw) for _ in range(n)]
