"""The inputs of tests/test_gpu_point_edges.py, built in one place so that tests/test_point_edge_cases_cpu.py can judge the same
inputs on the float64 restatements alone: the four hand-tiled point models (csrc/svdpp.hip, delf.hip, caser.hip, sasrec.hip) at
the edges of their own loops -- widths that do not divide the 256-thread workgroup, lengths on a chunk seam, the second trip of
a strided loop, the widest rows on either side, one window past a sweep of eight, an exact tie of the window maximum, saturated
keys, and the LDS bound of the attention kernels from the inside.

Every case follows the recipe of its model's own cases: N = 3000, hidden_size 32 (ignored by all four), the batch drawn from
default_rng(100 + seed), labels alternating, and the batch passed through the model's own kink / edge filter with a cap that the
CPU test holds against the model's own.  Parameters: SVD++ init_params(c, 3); DELF init_params(c, 3, bias_scale=0.1); Caser TF's
initial values with the biases and bn1 moved by 0.1 N(0, 1) from the batch's generator (tests/test_gpu_caser.py::case); SASRec
init_params(c, 3, perturbed=True).  The seeds are fixed here, on the CPU, from the restatements; never from a GPU run."""
import collections
import functools

import numpy as np
import torch

import caser_ref as cr
import delf_ref as dr
import sasrec_ref as sa
import svdpp_ref as sv

N, H = 3000, 32

# name -> model, (D, T, Fu, Fi, B), batch seed, how many samples the filter may take (the CPU test: no more than the model's own
# cap), and what is forced on the batch.  What each row is about:
#   svdpp_d12            G = 256 / 12 = 21 row groups, 4 idle threads (g == G); T = 30 spans two trips of the row loop; sample 0 is
#                        forced to length 1 (twenty groups without a row), sample 1 to 3 T (clipped to T)
#   svdpp_d24, _d48      G = 10 / 5, 16 idle threads
#   svdpp_d96            G = 2: one whole idle wave, and the upper half of svdpp_wave_dsum (lane + 64 < D) filled to 32 lanes
#   svdpp_fmax           Fu = Fi = 8 = SVDPP_FMAX: the last slot of wi[] / acc[] and of s_w[]; T == G = 16
#   svdpp_t17            T == G + 1: the row loop's second trip is taken by group 0 alone
#   delf_seam            C = 16 on both sides: chunks of RC = 64 rows; live lengths 63, 64 (the backward pass skips the product of
#                        the last chunk and still writes its dX / dpre), 65 (one row in the second chunk), 1 and 130 (clipped)
#   delf_t257            C = 4: RC = 256; the strided softmax / ds loops take a second trip; lengths 256, 257, 300, 1 and a zero
#                        length (uniform weights 1 / 257)
#   delf_two_wave        Cu = Ci = 80: the row group of two waves (sums through s_red) on both sides
#   delf_cu128           Cu = 128, the limit, on side 1; Ci = 96
#   delf_c12, _c24       a multiple of 4 that is none of 8 / 16: idle lanes inside a group_sum width
#   delf_saturated       the table x 8 and the four first fusion kernels x 1/8: most keys beyond |key| = 0.999 (1 - key^2 loses
#                        its digits in fp32), the attention one-hot, the predictions still off 0 and 1
#   caser_nw9            NW = T - 49 = 9: a second sweep that holds ONE window (nj = 1) over rows 8 .. 57
#   caser_nw16_b9        two full sweeps; B = 9: caser_params_kernel's share 0 holds two samples, the others one
#   caser_nw17           a third sweep with one window
#   caser_c256           C = 256 exactly: CW = 256, one row group
#   caser_c260           a second column block with 4 live lanes of 256
#   caser_zero_history   sample 1 of 3 has a history of id 0: every window sum is bh exactly, the first position keeps the maximum
#   sasrec_t130          2 T = 260 softmax rows per sample: the second trip of `for (r = tid; r < 2 T; r += 256)`
#   sasrec_t137          the last T whose buffers fit the LDS bound at C = 4 (40 826 of 40 960 floats)
#   sasrec_t8, _t16, _t17  sas_proj's 8-row register blocks: one exact, two exact, one row over
#   sasrec_c12, _c100    head widths 6 and 50
Row = collections.namedtuple("Row", "model shape seed drop forced")


def _row(model, shape, seed=0, drop=0, forced=None):
    return Row(model, shape, seed, drop, forced)


CASES = collections.OrderedDict([
    ("svdpp_d12", _row("svdpp", (12, 30, 2, 3, 9), forced={0: 1, 1: 90})),
    ("svdpp_d24", _row("svdpp", (24, 12, 1, 2, 9))),
    ("svdpp_d48", _row("svdpp", (48, 7, 1, 1, 5))),
    # (seed 0: the only sample whose prediction is not saturated has G live rows -- the others' logits are beyond +-17, where
    # log_loss's epsilon leaves no gradient --, so a slip in the rows past the first trip would weigh 1e-3 of the gradient)
    ("svdpp_d96", _row("svdpp", (96, 5, 1, 1, 5), seed=6)),
    ("svdpp_fmax", _row("svdpp", (16, 16, 8, 8, 9))),
    ("svdpp_t17", _row("svdpp", (16, 17, 1, 8, 9))),
    ("delf_seam", _row("delf", (16, 65, 1, 1, 5), forced=((64, 65, 1, 63, 130), (65, 64, 130, 1, 63)))),
    ("delf_t257", _row("delf", (4, 257, 1, 1, 3), forced=((257, 256, 0), (1, 300, 257)))),
    ("delf_two_wave", _row("delf", (16, 9, 5, 5, 9))),
    ("delf_cu128", _row("delf", (32, 5, 4, 3, 5))),
    ("delf_c12", _row("delf", (4, 9, 3, 3, 9))),
    ("delf_c24", _row("delf", (8, 10, 3, 3, 9))),
    ("delf_saturated", _row("delf", (16, 12, 3, 4, 40), drop=2, forced="saturated")),
    ("caser_nw9", _row("caser", (16, 58, 3, 4, 17))),
    ("caser_nw16_b9", _row("caser", (16, 65, 3, 4, 9))),
    ("caser_nw17", _row("caser", (16, 66, 3, 4, 9))),
    ("caser_c256", _row("caser", (64, 50, 1, 4, 9))),
    ("caser_c260", _row("caser", (52, 50, 1, 5, 7))),
    ("caser_zero_history", _row("caser", (16, 58, 3, 4, 3), forced="zero_history")),
    ("sasrec_t130", _row("sasrec", (4, 130, 1, 1, 2))),
    ("sasrec_t137", _row("sasrec", (4, 137, 1, 1, 1))),
    ("sasrec_t8", _row("sasrec", (8, 8, 1, 2, 5))),
    ("sasrec_t16", _row("sasrec", (8, 16, 1, 2, 5))),
    ("sasrec_t17", _row("sasrec", (8, 17, 1, 2, 5), seed=1)),      # (seed 0: one of the five samples sits on a relu kink)
    ("sasrec_c12", _row("sasrec", (4, 16, 1, 3, 5))),
    ("sasrec_c100", _row("sasrec", (20, 6, 1, 5, 5))),
])
# Bounds against the float64 restatements are the project's for point models (loss 2e-5 relative to max(1, |loss|), y 1e-4, arrays
# and gradients rtol 2e-4 / atol 2e-6).  Measured on an MI355X, every row holds them with room: the largest gradient error
# (relative to the array's largest entry) is delf_saturated's, 1.9e-5 on dense_1/bias, then caser_zero_history's 1.6e-5 on
# dense/bias; every other row is below 1e-5 and most below 1e-6.  delf_saturated needed no bound of its own: the lost digits of
# 1 - key^2 sit under pre-activation gradients that are themselves small.
REF = {"svdpp": sv, "delf": dr, "caser": cr, "sasrec": sa}
SATURATED_EMB, SATURATED_FUSION = 8.0, 0.125
ZERO_HISTORY_SAMPLE = 1

Case = collections.namedtuple("Case", "row ref c P batch kept batch_all")


def cap(model, B):
    """how many samples of a batch of B the model's own filter may take: svdpp_ref.cap, delf_ref.cap, caser_ref.cap, and for
    SASRec the project's default of helpers.check_dropped (a quarter of the batch, one sample at least kept)"""
    if model == "sasrec":
        return B - max(1, (3 * B) // 4)
    return REF[model].cap(B)


def sas_lds_floats(T, C):
    """sas_lds_floats of csrc/sasrec.hip, restated: four [T, C + 1] matrices, both heads' [T, T] scores, four [T] vectors"""
    return 4 * T * (C + 1) + 2 * T * T + 4 * T


SAS_LDS_LIMIT_FLOATS = 160 * 1024 // 4


def raw_batch(name):
    """cfg, parameters, the batch before the filter"""
    r = CASES[name]
    D, T, Fu, Fi, B = r.shape
    ref = REF[r.model]
    c = ref.Cfg(N, D, H, T, Fu, Fi)
    rng = np.random.default_rng(100 + r.seed)
    if r.model == "svdpp":
        P = sv.init_params(c, 3)
        b = sv.random_batch(rng, c, B, max_length=3 * T)
        for i, ln in (r.forced or {}).items():
            b["user_seq_length"][i] = ln
    elif r.model == "delf":
        P = dr.init_params(c, 3, bias_scale=0.1)
        if r.forced == "saturated":
            P["emb_mtx"] = (P["emb_mtx"] * np.float32(SATURATED_EMB)).astype(np.float32)
            for k in (2, 4, 6, 8):
                P["dense_%d/kernel" % k] = (P["dense_%d/kernel" % k] * np.float32(SATURATED_FUSION)).astype(np.float32)
        b = dr.random_batch(rng, c, B, min_length=(1, 1), max_length=(3 * T, 3 * T))
        if isinstance(r.forced, tuple):
            b["user_seq_length"] = np.array(r.forced[0], dtype=np.int32)
            b["item_seq_length"] = np.array(r.forced[1], dtype=np.int32)
    elif r.model == "caser":
        P = cr.init_params(c, 3)
        for n in P:
            if "bias" in n or n.startswith("bn1"):
                P[n] = (P[n] + 0.1 * rng.standard_normal(P[n].shape)).astype(np.float32)
        b = cr.random_batch(rng, c, B)
        if r.forced == "zero_history":
            b["user_seq"][ZERO_HISTORY_SAMPLE] = 0
    else:
        P = sa.init_params(c, 3, perturbed=True)
        b = sa.random_batch(rng, c, B, max_length=3 * T)
    b["label"] = (np.arange(B) % 2).astype(np.int32)
    return c, P, b


def _zero_history_filter(c, P, b):
    """caser_ref.away_from_kinks would take the zero-history sample by design (its window sums are all equal: margin 0).  Here
    that sample passes the relu filter alone, the others both filters, and nothing may go."""
    with torch.no_grad():
        out = cr.forward(c, cr.to_torch(P), b)
    ok = out["relu_margin_per_sample"] > cr.RELU_THR
    others = np.arange(ok.size) != ZERO_HISTORY_SAMPLE
    ok &= (out["window_margin_per_sample"] > cr.WINDOW_THR) | ~others
    assert ok.all(), "a sample of the zero-history batch sits on a kink: another batch seed"
    return b, np.arange(ok.size)


@functools.lru_cache(maxsize=None)
def case(name):
    """the row, its restatement module, cfg, parameters, the batch behind the filter, kept, the whole batch.  Built once per
    process; nobody writes into it."""
    r = CASES[name]
    c, P, b_all = raw_batch(name)
    if r.forced == "zero_history":
        b, kept = _zero_history_filter(c, P, b_all)
    elif r.model == "svdpp":
        b, kept = sv.away_from_kinks(c, P, b_all, max_dropped=r.drop)
    elif r.model == "delf":
        b, kept = dr.away_from_kinks(c, P, b_all, max_dropped=r.drop)
    elif r.model == "caser":
        b, _, kept = cr.away_from_kinks(c, P, b_all, max_dropped=r.drop)
    else:
        b, _, kept = sa.away_from_edges(c, P, b_all, max_dropped=r.drop)
    return Case(r, REF[r.model], c, P, b, kept, b_all)


def delf_keys(c, P, b, side=0):
    """the attention keys tanh(X W + b) of one side in float64, [B, T, C], and the mask of the live positions [B, T]"""
    emb = P["emb_mtx"].astype(np.float64)
    emb[0] = 0
    seq, ln, W, bias = ((b["user_seq"], b["user_seq_length"], P["dense/kernel"], P["dense/bias"]) if side == 0 else
                        (b["item_seq"], b["item_seq_length"], P["dense_1/kernel"], P["dense_1/bias"]))
    X = emb[seq].reshape(seq.shape[0], c.T, -1)
    live = np.arange(c.T)[None, :] < ln[:, None]
    return np.tanh(X @ W.astype(np.float64) + bias.astype(np.float64)), live
