"""The inputs of the SASRec GPU tests (tests/test_gpu_sasrec.py), built in one place so that tests/test_sasrec_cpu.py can judge the
same inputs on the float64 restatement alone: the edge filter (sasrec_ref.away_from_edges) may take at most a quarter of a
batch -- the project's default cap, although a sample owns (2 T - 3) * 280 relu units here --, and the seeds below are fixed so
that it does.

Every case runs at gamma = 1 + 0.1 n, beta = 0.5 + 0.1 n, biases 0.1 n (sasrec_ref.init_params(perturbed=True)): every
sum_c Qin is of order C / 2, padded rows included, so the query mask is decided by a wide margin.  At TF's own initial values
(gamma = 1, beta = 0) that sum is a rounding residue and the mask an accident of the summation order: not compared."""
import numpy as np

import sasrec_ref as sr

TMALL = (16, 32, 50, 3, 4)          # D, H, T, Fu, Fi of the reference's point-model run (train_time_point_models.py:15-35)
H = 32                              # hidden_size: accepted and ignored

# (D, T, Fu, Fi, B) -> (batch seed, forced lengths).
# The smallest legal T, head width 2, one sample | lengths (1, 4, 9): one live row, exactly T, longer than T | ragged batch tails,
# twice | C = 128, the width limit | Taobao's widths | CCMR's widths (C = 80, head width 40) at T = 50 | Tmall's widths and T
SHAPES = {(4, 3, 1, 1, 1): (0, None),
          (4, 4, 2, 1, 3): (0, (1, 4, 9)),
          (16, 9, 3, 4, 33): (0, None),
          (16, 9, 3, 4, 37): (0, None),
          (32, 5, 1, 4, 5): (0, None),
          (16, 12, 1, 2, 17): (0, None),
          (16, 50, 1, 5, 6): (0, None),
          (16, 50, 3, 4, 8): (0, None)}


def cfg(D, T, Fu, Fi, N=3000):
    return sr.Cfg(N, D, H, T, Fu, Fi)


def params(c, seed=3):
    return sr.init_params(c, seed, perturbed=True)


def batches(c, B, n, seed, max_length=None):
    rng = np.random.default_rng(seed)
    return [sr.random_batch(rng, c, B, max_length=max_length or 3 * c.T) for _ in range(n)]


def case(D, T, Fu, Fi, B):
    """cfg, parameters, the batch behind the edge filter, kept"""
    seed, forced = SHAPES[(D, T, Fu, Fi, B)]
    c = cfg(D, T, Fu, Fi)
    P = params(c)
    rng = np.random.default_rng(100 + seed)
    b = sr.random_batch(rng, c, B, max_length=3 * T)
    if forced is not None:
        b["user_seq_length"] = np.array(forced, dtype=np.int32)
    b["label"] = (np.arange(B) % 2).astype(np.int32)
    b, _, kept = sr.away_from_edges(c, P, b)
    return c, P, b, kept


def masked_case(beta_zero=False):
    """a batch whose history holds id 0 at whole positions (every field 0: the key mask fires, and with beta = 0 exactly the
    row's Qin is 0 exactly, so the query mask is 0 there in every precision) and in single fields; row 0 gets no gradient.
    -> cfg, parameters, batch behind the filter, kept"""
    c = cfg(16, 9, 3, 4)
    P = params(c)
    if beta_zero:
        P["ln/Variable"] = np.zeros_like(P["ln/Variable"])
    rng = np.random.default_rng(300)
    b = sr.random_batch(rng, c, 33, max_length=3 * c.T)
    seq = b["user_seq"]
    seq[rng.random(seq.shape[:2]) < 0.25] = 0             # whole positions
    seq[rng.random(seq.shape) < 0.15] = 0                 # single fields
    b["label"] = (np.arange(33) % 2).astype(np.int32)
    b, _, kept = sr.away_from_edges(c, P, b)
    return c, P, b, kept


def all_masked_case():
    """one sample (index 1 of 3) whose history is all id 0: every key masked, uniform weights 1 / T"""
    c = cfg(16, 9, 3, 4)
    P = params(c)
    b = batches(c, 3, 1, 500)[0]
    b["user_seq"][1] = 0
    b["label"] = np.array([0, 1, 1], dtype=np.int32)
    b, _, kept = sr.away_from_edges(c, P, b, max_dropped=0)
    return c, P, b


def dropout_case(keep_prob=0.8):
    """keep_prob 0.8 with all three explicit masks at (16, 9, 3, 4, 33) -> cfg, parameters, batch, masks, kept"""
    c = cfg(16, 9, 3, 4)
    P = params(c)
    rng = np.random.default_rng(700)
    b = sr.random_batch(rng, c, 33, max_length=3 * c.T)
    b["label"] = (np.arange(33) % 2).astype(np.int32)
    masks = sr.random_masks(rng, c, 33, keep_prob)
    b, masks, kept = sr.away_from_edges(c, P, b, keep_prob, masks)
    return c, P, b, masks, kept


def trajectory_case():
    """ten training steps at the Tmall widths, B = 24 -> cfg, parameters, five batches"""
    c = sr.Cfg(20011, *TMALL)
    return c, sr.init_params(c, 4, perturbed=True), batches(c, 24, 5, 8)
