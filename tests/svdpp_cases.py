"""The inputs of the SVD++ GPU tests (tests/test_gpu_svdpp.py), built in one place so that tests/test_svdpp_cpu.py can judge the
same inputs on the float64 restatement alone: the kink filter (svdpp_ref.away_from_kinks) may take at most cap(B) samples of a
case -- none when B <= 3 --, and the seeds below are fixed so that it does."""
import numpy as np

import svdpp_ref as sr

TMALL = (16, 32, 50, 3, 4)          # D, H, T, Fu, Fi of the reference's point-model run (train_time_point_models.py:15-35)
H = 32                              # hidden_size: accepted and ignored

# (D, T, Fu, Fi, B) -> (batch seed, maximum length or None = up to 3 T, forced lengths).
# One position, one sample | a single live row, exactly T, longer than T | ragged batch tails, twice | every length <= 5
# (active_slices is taken) | the widest rows and the eb_dim limit (two row groups per workgroup) | the Tmall point shape | CCMR's
# widths (Ci = 80)
SHAPES = {(4, 1, 1, 1, 1): (0, None, None),
          (4, 3, 2, 1, 3): (0, None, (1, 3, 7)),
          (16, 9, 3, 4, 33): (0, None, None),
          (16, 9, 3, 4, 37): (0, None, None),
          (16, 7, 3, 4, 33): (0, 5, None),
          (64, 9, 1, 2, 17): (0, None, None),
          (128, 5, 1, 1, 5): (0, None, None),
          (16, 50, 3, 4, 200): (0, None, None),
          (16, 50, 1, 5, 100): (0, None, None)}


def cfg(D, T, Fu, Fi, N=3000):
    return sr.Cfg(N, D, H, T, Fu, Fi)


def params(c, seed=3):
    return sr.init_params(c, seed)


def case(D, T, Fu, Fi, B):
    """cfg, parameters, the batch behind the kink filter, kept"""
    seed, hi, forced = SHAPES[(D, T, Fu, Fi, B)]
    c = cfg(D, T, Fu, Fi)
    P = params(c)
    rng = np.random.default_rng(100 + seed)
    b = sr.random_batch(rng, c, B, max_length=hi or 3 * T)
    if forced is not None:
        b["user_seq_length"] = np.array(forced, dtype=np.int32)
    b["label"] = (np.arange(B) % 2).astype(np.int32)
    b, kept = sr.away_from_kinks(c, P, b)
    return c, P, b, kept


def batches(c, B, n, seed, max_length=None):
    rng = np.random.default_rng(seed)
    return [sr.random_batch(rng, c, B, max_length=max_length or 3 * c.T) for _ in range(n)]


def masked_case():
    """a batch whose history holds id 0 at some LIVE positions: whole rows (every field 0: s_t = 0 exactly, sign(0) = 0) and
    single fields; row 0 gets no gradient.  -> cfg, parameters, batch behind the filter, kept"""
    c = cfg(16, 9, 3, 4)
    P = params(c)
    rng = np.random.default_rng(300)
    b = sr.random_batch(rng, c, 33, max_length=3 * c.T)
    b["user_seq_length"] = np.maximum(b["user_seq_length"], 4)
    seq = b["user_seq"]
    seq[rng.random(seq.shape[:2]) < 0.25] = 0             # whole positions
    seq[rng.random(seq.shape) < 0.15] = 0                 # single fields
    seq[:, 3] = np.maximum(seq[:, 3], 1)                  # (one live row per sample stays whole: n > 0)
    b["label"] = (np.arange(33) % 2).astype(np.int32)
    b, kept = sr.away_from_kinks(c, P, b)
    return c, P, b, kept


def tie_case():
    """a table whose columns 0 and 1 are identical and scaled x4: the two maximal column sums of every sample are equal bit for bit
    (the same operations on the same values), and reduce_max's gradient is split equally between them.  Lengths >= 5, so that
    the scaled columns are the maximal ones.  -> cfg, parameters, batch behind the filter, kept"""
    c = cfg(16, 9, 3, 4)
    P = params(c, seed=5)
    emb = P["emb_mtx"].copy()
    emb[:, 0] *= 4.0
    emb[:, 1] = emb[:, 0]
    P["emb_mtx"] = emb
    rng = np.random.default_rng(401)           # (a seed for which columns 0 and 1 are the maximal ones of every sample: test_svdpp_cpu.py)
    b = sr.random_batch(rng, c, 33, max_length=3 * c.T)
    b["user_seq_length"] = np.maximum(b["user_seq_length"], 5)
    b["label"] = (np.arange(33) % 2).astype(np.int32)
    b, kept = sr.away_from_kinks(c, P, b)
    return c, P, b, kept


def degenerate_case():
    """one zero-length sample (index 2) in a batch of 5: n = 0, q = 0 / 0"""
    c = cfg(16, 9, 3, 4)
    P = params(c)
    b = batches(c, 5, 1, 500)[0]
    b["user_seq_length"] = np.array([3, 9, 0, 20, 1], dtype=np.int32)
    return c, P, b
