"""The inputs of tests/test_gpu_score_head_edges.py, built in one place so that tests/test_score_head_cases_cpu.py can judge the same
inputs on the oracle alone: the four fused kernels of the launch-stream pass (csrc/head_fused.hip, head_tiles.h: head_fwd_fused_kernel
in one and in two launches, head_bwd_fused_kernel, attn_fwd_fused_kernel<KQ>, attn_inp_bwd_fused_kernel) at their loop edges -- the
chunks of hf_tiles, the head forward's split, the shares of the head backward's grid, the samples per workgroup, row tiles, widths
and LDS bound of the attention, lengths past T, explicit dropout masks, and saturated parameters.  The file also mirrors the four
launch rules in Python, so that every row states the forms it expects in the terms of score_head_last_forms (include/score_hip.h)
and a row meant for a fused kernel that falls back to the layered pass fails instead of testing the wrong code.
Every case runs with debug_flags = 512 (H = 32, B <= 512 stays off the per-sample kernels).  The seeds are fixed here, on the CPU, so
that the kink filter (helpers.away_from_relu_kinks, thr = 1e-5) drops no more than the row says."""
import collections
import functools

import numpy as np

from oracle import score_oracle as so
from helpers import away_from_relu_kinks, random_batch

N = 1500
PARAM_SEED = 5
FLAGS = 512                       # debug_flags of every case
FLAGS_LAYERED = 512 | 64 | 128    # ... of the pass they are compared with: head and attention layer by layer / as separate launches
FC1, FC2, AT1, AT2 = 200, 80, 80, 40
LDS_BOUND = 150 * 1024

# ---------------------------------------------------------------------------------------------------------------------------
# The launch rules of csrc/head_fused.hip and of engine.hip's bwd_attention, restated.  T is the number of slices the pass
# computes (every case has a sample of length >= T, so it is the configuration's).


def dims(r):
    """Dh, NI, Dk, off_u, off_i of a row (engine.hip: make_dims)"""
    nstate = 2 if r.mt in ("SCORE", "RCA") else 1
    NI = 0 if r.mt == "RCA" else 4 * r.K
    off_u = -1 if r.mt == "SCORE_ITEM" else 0
    off_i = -1 if r.mt == "SCORE_USER" else (0 if r.mt == "SCORE_ITEM" else r.H)
    return nstate * r.H + (r.Fu + r.Fi) * r.D, NI, 2 * r.H + NI, off_u, off_i


def _ceil16(x):
    return (x + 15) & ~15


def head_fwd_form(B, Dh):
    """0 layer by layer, 1 one launch, 2 two launches (score_launch_head_fwd_fused)"""
    lds = 16 * (_ceil16(Dh) + 4 + _ceil16(FC1) + 4 + _ceil16(FC2) + 4) * 4
    if B <= 0 or lds > LDS_BOUND:
        return 0
    mt, nt1 = (B + 15) // 16, (FC1 + 15) // 16
    return 2 if nt1 >= 4 and mt >= 32 else 1


def head_bwd_ny(B, Dh):
    """shares of d bn1's column tiles per row tile (score_launch_head_bwd_fused)"""
    mt, ntile = (B + 15) // 16, (Dh + 15) // 16
    return (4 if mt <= 64 else 2) if (mt <= 128 and ntile >= 32) else 1


def _samples_per_workgroup(B):
    return 4 if B >= 1024 else 2 if B >= 512 else 1


def attn_fwd_lds(S, T, K2):
    LD = _ceil16(K2) + 4
    return (2 * 16 * LD + S * T * (AT1 + 1) + AT1 * AT2 + S * T * (AT2 + 1) + S * T) * 4


def attn_fwd_form(B, T, H, NI):
    """(S, KQ) of attn_fwd_fused_kernel, (0, 0) with separate launches (score_launch_attn_fwd_fused)"""
    if B <= 0 or T <= 0 or (H & 3) or (NI & 3) or B * T >= 1 << 30:
        return 0, 0
    K2 = 2 * (2 * H + NI)
    S = _samples_per_workgroup(B)
    while S >= 1 and attn_fwd_lds(S, T, K2) > LDS_BOUND:
        S >>= 1
    kq = _ceil16(K2) // 4
    if S < 1 or kq not in (36, 44, 52, 84, 148):
        return 0, 0
    return S, kq


def attn_bwd_lds(S, T, K2, pool):
    RT = _ceil16(S * T)
    n = RT * (AT1 + 4) + 16 * (K2 + 4) + S * (K2 // 2)
    if pool:
        n += S * T + S * T * (AT2 + 1) + AT1 * (AT2 + 1)
    return n * 4


def ab_plan(B, T, H, NI, ldh, off_u, off_i, pool):
    """S of attn_inp_bwd_fused_kernel or 0 (ab_plan: no loop that reduces S)"""
    K2 = 2 * (2 * H + NI)
    if (B <= 0 or T <= 0 or (H & 3) or (NI & 3) or K2 > 640 or B * T >= 1 << 30 or (ldh & 3) or (off_u >= 0 and off_u & 3)
            or (off_i >= 0 and off_i & 3)):
        return 0
    S = _samples_per_workgroup(B)
    return S if attn_bwd_lds(S, T, K2, pool) <= LDS_BOUND else 0


def attn_bwd_form(B, T, H, NI, ldh, off_u, off_i):
    """(S, pooling inside) of attn_inp_bwd_fused_kernel, (0, 0) with separate launches (engine.hip: bwd_attention)"""
    if B * T < 8192:
        S = ab_plan(B, T, H, NI, ldh, off_u, off_i, True)
        if S:
            return S, 1
    return ab_plan(B, T, H, NI, ldh, off_u, off_i, False), 0


Forms = collections.namedtuple("Forms", "hf ny af_S af_KQ ab_S ab_pool")
LAYERED = Forms(0, 0, 0, 0, 0, 0)


def pack(f):
    """a Forms as score_head_last_forms reports it behind a forward and a backward pass"""
    return f.hf | f.ny << 2 | f.af_S << 5 | f.af_KQ << 8 | f.ab_S << 16 | f.ab_pool << 19 | 1 << 20 | 1 << 21


def unpack(w):
    return Forms(w & 3, w >> 2 & 7, w >> 5 & 7, w >> 8 & 255, w >> 16 & 7, w >> 19 & 1)


def mirror(r):
    """the forms the launch rules give a row"""
    Dh, NI, _, off_u, off_i = dims(r)
    return Forms(head_fwd_form(r.B, Dh), head_bwd_ny(r.B, Dh), *(attn_fwd_form(r.B, r.T, r.H, NI) +
                                                                  attn_bwd_form(r.B, r.T, r.H, NI, Dh, off_u, off_i)))


# ---------------------------------------------------------------------------------------------------------------------------
# name -> D, Fu, Fi, H, K, T, B, model type, batch seed, samples the kink filter drops (counted on the CPU:
# test_score_head_cases_cpu.py; cap = that + 2), the forms expected, and
#   gen      samples generated where the batch BEHIND the filter has to have exactly B (the first B kept are the batch)
#   lengths  "ragged" 1 .. T with sample 0 at T | "ends_zero" the same with sample 0 and every sample from B - 1 on at 0, sample 1 at T |
#            "over" 0, 1, T, T + 1, 3 T on samples 1 .. 5, sample 0 at T, ragged 1 .. 3 T behind them
#   keep     keep_prob; below 1 the case runs with explicit dropout masks [B, 200], [B, 80] (drawn here)
#   params   a parameter case: what is done to init_params' values (PARAMS below); these rows skip the kink filter -- dead_relus
#            puts EVERY dense_4 / fc2 unit on its kink (zero input, zero bias) -- and are compared at operator level, from the
#            kernels' own fp32 inputs, never through gradients of a saturated sigmoid
# What each row is about (Dh = nstate H + (Fu + Fi) D the head's input width; Dk = 2 H + 4 K, 2 H for RCA; K2 = 2 Dk;
# KQ = ceil16(K2) / 4; hf_tiles deals ceil16(Dh) / 4 k-steps to each lane quarter in chunks of HF_CH = 16, two chunks a trip):
#   dh40               12 k-steps a quarter: less than one chunk.  Attention KQ = 20 is no instance -> separate launches
#   dh64               exactly one chunk; one full row tile plus one row (B = 17)
#   dh68               Kp0 = 80: the last quarter holds 8 live of its 20 k-steps (clamped rows of W1, masked products)
#   dh128              exactly two chunks: the third fetch is clamped as a whole
#   dh140              36 k-steps a quarter: the second trip has 4 steps
#   dh30_user          SCORE_USER at H = 18: Dh & 3 == 2 takes the scalar bn1 path; K = 30 of Kp0 = 32, the clamp inside the last
#                      quarter.  (H & 3 != 0: the attention runs as separate launches both ways)
#   b496 / b497        31 row tiles: one launch | 32: two launches, the last tile with one row
#   dh496/512/528      head backward at B = 5: 31 column tiles, ny = 1 | 32, ny = 4, one tile per wave | 33 dealt 9, 9, 9, 6:
#                      wave 0 of a share takes two tiles (the double-buffered fetch)
#   b1025/2048_ny2     Dh = 512 at mt = 65 and 128: ny = 2; b1025 is also the attention at S = 4 with ns = 1 in the last workgroup
#   b2049_ny1          mt = 129: ny = 1
#   t1 t16 t17 t33     rows per workgroup 1, exactly one tile, one row into the second, one into the third
#   s2_t8              S = 2: two samples fill exactly one tile; B odd: the last workgroup has ns = 1; lengths 0 at both ends
#   s2_t9              S = 2, T = 9: the second sample straddles two tiles (the lo / hi ranges of the d q sums)
#   s4_ns3             S = 4, the last workgroup with ns = 3
#   pool_in / pool_out B T = 8190 / 8197: the pooling backward inside the fused kernel | a launch of its own
#   kq*                every KQ instance with K padding (K = 9: K2 no multiple of 16), KQ = 44 without, KQ = 52 at H = 48
#   rca_h36            RCA: NI = 0, H no multiple of 16
#   user_/item_kq36    SCORE_USER / SCORE_ITEM (off_i / off_u = -1) on a fused width
#   fwd_sep_bwd_fused  KQ = 60 is no instance, K2 = 240 <= 640: the forward as separate launches, the backward fused
#   both_sep           K2 = 672 > 640: separate both ways
#   lds_s1_in / _out   T = 247 / 248 at S = 1: the forward's LDS bound from the inside | one past it (separate launches; the
#                      backward's own plan still fits, with the pooling inside)
#   lds_s4_in          B = 1024, T = 61: S = 4 just fits
#   lds_s4_to_s2       T = 62: the forward drops to S = 2, the backward keeps S = 4 (without the pooling: B T >= 8192)
#   t129               T > 128: the second trip of the backward's dscore loop
#   lengths_over       lengths 0, 1, T, T + 1, 3 T: the kernels clamp
#   masks_b21 / _b500  explicit masks, keep_prob 0.8, B % 16 != 0 (the rows of the last tile past B read the mask's last row:
#                      csrc/cell.h relu_dropout); B = 500 takes the two-launch head, the last tile with four rows
#   softmax_onehot     dense_5/kernel x 200     softmax_uniform  dense_5/kernel = 0
#   sigmoid_01         fc3/kernel x 300, labels alternating: y_pred exactly 0.0 and exactly 1.0
#   dead_relus         fc1/bias and dense_3/bias at -1e3: f1 = 0, a1 = 0
Row = collections.namedtuple("Row", "D Fu Fi H K T B mt seed dropped forms gen lengths keep params")


def _row(D, Fu, Fi, H, K, T, B, forms, seed=1, dropped=0, mt="SCORE", gen=None, lengths="ragged", keep=1.0, params=None):
    return Row(D, Fu, Fi, H, K, T, B, mt, seed, dropped, Forms(*forms), gen or B, lengths, keep, params)


def _attn(T, B, forms, **kw):
    return _row(4, 1, 1, 16, 10, T, B, forms, **kw)


CASES = {
    # head forward, hf_tiles
    "dh40": _row(4, 1, 1, 16, 2, 2, 3, (1, 1, 0, 0, 1, 1)),
    "dh64": _row(4, 3, 5, 16, 10, 3, 17, (1, 1, 1, 36, 1, 1), gen=19),
    "dh68": _row(4, 4, 5, 16, 10, 3, 5, (1, 1, 1, 36, 1, 1)),
    "dh128": _row(16, 1, 3, 32, 10, 3, 5, (1, 1, 1, 52, 1, 1)),
    "dh140": _row(4, 1, 2, 64, 10, 3, 5, (1, 1, 1, 84, 1, 1)),
    "dh30_user": _row(4, 1, 2, 18, 3, 3, 5, (1, 1, 0, 0, 0, 0), mt="SCORE_USER"),
    # head forward split
    "b496": _row(4, 1, 1, 16, 10, 2, 496, (1, 1, 1, 36, 1, 1), gen=520, dropped=5),
    "b497": _row(4, 1, 1, 16, 10, 2, 497, (2, 1, 1, 36, 1, 1), gen=520, dropped=5),
    # head backward shares
    "dh496": _row(64, 3, 4, 24, 6, 2, 5, (1, 1, 1, 36, 1, 1)),
    "dh512": _row(64, 3, 4, 32, 2, 2, 5, (1, 4, 1, 36, 1, 1)),
    "dh528": _row(64, 3, 4, 40, 6, 2, 5, (1, 4, 1, 52, 1, 1)),
    "b1025_ny2": _row(64, 3, 4, 32, 2, 1, 1025, (2, 2, 4, 36, 4, 1), gen=1060, dropped=2),
    "b2048_ny2": _row(64, 3, 4, 32, 2, 1, 2048, (2, 2, 4, 36, 4, 1), gen=2110, dropped=6),
    "b2049_ny1": _row(64, 3, 4, 32, 2, 1, 2049, (2, 1, 4, 36, 4, 1), gen=2110, dropped=6),
    # attention tiles
    "t1": _attn(1, 3, (1, 1, 1, 36, 1, 1)),
    "t16": _attn(16, 3, (1, 1, 1, 36, 1, 1)),
    "t17": _attn(17, 3, (1, 1, 1, 36, 1, 1)),
    "t33": _attn(33, 3, (1, 1, 1, 36, 1, 1)),
    "s2_t8": _attn(8, 513, (2, 1, 2, 36, 2, 1), gen=540, lengths="ends_zero", dropped=8),
    "s2_t9": _attn(9, 514, (2, 1, 2, 36, 2, 1), gen=540, dropped=14),
    "s4_ns3": _attn(5, 1027, (2, 1, 4, 36, 4, 1), gen=1060, dropped=14),
    "pool_in": _attn(7, 1170, (2, 1, 4, 36, 4, 1), gen=1210, dropped=13),
    "pool_out": _attn(7, 1171, (2, 1, 4, 36, 4, 0), gen=1210, dropped=13),
    # attention widths
    "kq36_pad": _row(4, 1, 1, 16, 9, 5, 5, (1, 1, 1, 36, 1, 1)),
    "kq44": _row(4, 1, 1, 32, 6, 5, 5, (1, 1, 1, 44, 1, 1)),
    "kq52_pad": _row(4, 1, 1, 32, 9, 5, 5, (1, 1, 1, 52, 1, 1)),
    "kq52_h48": _row(4, 1, 1, 48, 2, 5, 5, (1, 1, 1, 52, 1, 1)),
    "kq84_pad": _row(4, 1, 1, 64, 9, 5, 5, (1, 1, 1, 84, 1, 1)),
    "kq148_pad": _row(4, 1, 1, 128, 9, 5, 5, (1, 1, 1, 148, 1, 1), seed=2),
    "rca_h36": _row(4, 1, 1, 36, 3, 5, 5, (1, 1, 1, 36, 1, 1), mt="RCA", seed=2),
    "user_kq36": _row(4, 1, 1, 16, 10, 5, 5, (1, 1, 1, 36, 1, 1), mt="SCORE_USER"),
    "item_kq36": _row(4, 1, 1, 16, 10, 5, 5, (1, 1, 1, 36, 1, 1), mt="SCORE_ITEM", seed=2),
    "fwd_sep_bwd_fused": _row(4, 1, 1, 48, 6, 5, 5, (1, 1, 0, 0, 1, 1)),
    "both_sep": _row(4, 1, 1, 128, 20, 2, 3, (1, 1, 0, 0, 0, 0)),
    # attention LDS
    "lds_s1_in": _attn(247, 3, (1, 1, 1, 36, 1, 1), seed=2),
    "lds_s1_out": _attn(248, 3, (1, 1, 0, 0, 1, 1), seed=2),
    "lds_s4_in": _attn(61, 1024, (2, 1, 4, 36, 4, 0), gen=1060, dropped=31),
    "lds_s4_to_s2": _attn(62, 1024, (2, 1, 2, 36, 4, 0), gen=1060, dropped=24),
    "t129": _attn(129, 3, (1, 1, 1, 36, 1, 1)),
    # lengths
    "lengths_over": _row(4, 1, 1, 32, 6, 6, 9, (1, 1, 1, 44, 1, 1), lengths="over", seed=2),
    # explicit masks
    "masks_b21": _attn(3, 21, (1, 1, 1, 36, 1, 1), gen=24, keep=0.8),
    "masks_b500": _attn(3, 500, (2, 1, 1, 36, 1, 1), gen=530, keep=0.8, dropped=2),
    # parameter cases
    "softmax_onehot": _attn(6, 37, (1, 1, 1, 36, 1, 1), params="softmax_onehot"),
    "softmax_uniform": _attn(6, 37, (1, 1, 1, 36, 1, 1), params="softmax_uniform"),
    "sigmoid_01": _attn(6, 37, (1, 1, 1, 36, 1, 1), params="sigmoid_01"),
    "dead_relus": _attn(6, 37, (1, 1, 1, 36, 1, 1), params="dead_relus"),
}
SHAPE_CASES = [n for n, r in CASES.items() if r.params is None]
PARAM_CASES = [n for n, r in CASES.items() if r.params is not None]


def _scale(name, f):
    def fn(P):
        P[name] = (P[name] * np.float32(f)).astype(np.float32)
    return fn


def _fill(names, v):
    def fn(P):
        for n in names:
            P[n] = np.full_like(P[n], v)
    return fn


PARAMS = {
    "softmax_onehot": _scale("dense_5/kernel", 200.0),
    "softmax_uniform": _scale("dense_5/kernel", 0.0),
    "sigmoid_01": _scale("fc3/kernel", 300.0),
    "dead_relus": _fill(("fc1/bias", "dense_3/bias"), -1e3),
}

Case = collections.namedtuple("Case", "cfg P batch kept masks batch_all row")


def raw_batch(name):
    """cfg, parameters, the batch before the kink filter, its dropout masks or None"""
    r = CASES[name]
    cfg = so.Cfg(N, r.D, r.H, r.T, r.K, r.Fu, r.Fi, r.mt)
    P = so.init_params(cfg, PARAM_SEED)
    if r.params:
        PARAMS[r.params](P)
    rng = np.random.default_rng(r.seed)
    b = random_batch(rng, cfg, r.gen)
    L = rng.integers(1, r.T + 1, r.gen).astype(np.int32)
    L[0] = r.T
    if r.lengths == "ends_zero":
        L[1] = r.T
        L[0] = 0
        L[r.B - 1:] = 0                 # (the last of the first B kept is one of these)
    elif r.lengths == "over":
        L = rng.integers(1, 3 * r.T + 1, r.gen).astype(np.int32)
        L[:6] = (r.T, 0, 1, r.T, r.T + 1, 3 * r.T)
    b["length"] = L
    b["label"] = (np.arange(r.gen) % 2).astype(np.int32)
    masks = None
    if r.keep < 1.0:
        masks = [(rng.random((r.gen, n)) < r.keep).astype(np.uint8) for n in (FC1, FC2)]
    return cfg, P, b, masks


@functools.lru_cache(maxsize=None)
def case(name):
    """cfg, parameters, the batch behind the kink filter (a parameter case: the whole batch), kept, the masks of the kept samples
    or None (+ the whole batch, the row).  Built once per process; nobody writes into it."""
    r = CASES[name]
    cfg, P, b_all, masks = raw_batch(name)
    if r.params:
        b, kept = b_all, np.arange(r.gen)
    else:
        b, masks, kept = away_from_relu_kinks(cfg, P, b_all, keep_prob=r.keep, dropout_masks=masks, max_dropped=r.dropped + 2)
    assert kept.size >= r.B, "%s: fewer than %d samples behind the kink filter: another batch seed or a larger gen" % (name, r.B)
    if kept.size != r.B:
        assert r.gen != r.B, "%s: the filter drops from a batch that has to keep its size: another batch seed" % name
        kept = kept[:r.B]
        b = {k: np.ascontiguousarray(v[:r.B]) for k, v in b.items()}
        masks = [np.ascontiguousarray(m[:r.B]) for m in masks] if masks is not None else None
    assert int(b["length"].max()) >= r.T, "%s: the sample that keeps every slice computed sits on a relu kink: another seed" % name
    return Case(cfg, P, b, kept, masks, b_all, r)


# Bounds against the float64 oracle are the project's own for these passes (tests/test_gpu_persample.py, test_gpu_model.py):
# loss 2e-5 relative to max(1, |loss|), y_pred and logit 1e-4, arrays and gradients rtol 2e-4 / atol 2e-6 (test_gpu_model.close).
# tests/test_score_head_cases_cpu.py holds the float32 oracle to them on every row, so an fp32 pass can meet them.  An indexing or
# padding slip shows as errors of the size of the values; should a row ever miss by a small factor, the rule is: measure the
# float32 oracle against the float64 oracle on that row and allow four times that (4-step MFMA chains against MKL's blocking).
LOSS_TOL, Y_TOL, RTOL, ATOL = 2e-5, 1e-4, 2e-4, 2e-6

# Measured on an MI355X (tests/test_gpu_score_head_edges.py with -s), the largest error of each row: against the float64 oracle
# `loss` (relative to max(1, |loss|)), `y` (y_pred), `z` (logit) and the worst of att_score, head_inp and the gradients (relative to
# the array's largest value, test_gpu_model.close); `lay` the worst gradient against the layered pass.  Every row holds the bounds
# above with room, no bound was set by the four-times rule.  The two largest figures are dense/bias of lds_s1_out and masks_b500
# (the gradient of the co-attention's bias: a sum of thousands of terms of both signs that cancel to ~1e-5 of their size); the
# float32 ORACLE is further from the float64 oracle there than the kernels are (1.7e-05 and 1.5e-04: test_score_head_cases_cpu.py).
#   row                loss     y        z        worst array                               lay
#   dh40               3.2e-08  1.3e-08  8.4e-08  3.8e-06 dense_1/bias                      3.8e-06
#   dh64               6.5e-08  5.9e-08  2.1e-07  1.6e-06 dense/bias                        1.8e-06
#   dh68               4.0e-08  5.6e-08  1.9e-07  1.2e-06 dense_2/bias                      1.3e-06
#   dh128              4.6e-08  6.4e-08  1.6e-07  8.0e-07 dense_4/bias                      1.3e-06
#   dh140              6.9e-09  4.1e-08  8.4e-08  7.6e-07 gru_item_side gates/bias          1.4e-06
#   dh30_user          2.2e-08  2.5e-08  4.7e-08  5.1e-07 dense_2/kernel                    1.2e-06
#   b496               4.0e-08  8.6e-08  1.6e-07  1.3e-06 att_score                         1.3e-06
#   b497               1.6e-08  8.6e-08  1.6e-07  1.3e-06 att_score                         1.0e-06
#   dh496              8.1e-08  6.8e-08  3.8e-07  8.3e-07 dense/bias                        8.5e-07
#   dh512              6.5e-08  1.3e-07  5.0e-07  2.7e-06 dense_5/kernel                    1.2e-06
#   dh528              4.9e-08  1.5e-07  5.3e-07  1.8e-06 dense_1/bias                      1.6e-06
#   b1025_ny2          7.6e-08  2.8e-07  1.1e-06  9.0e-07 dense/bias                        7.8e-07
#   b2048_ny2          2.2e-08  2.5e-07  1.1e-06  3.1e-06 dense_1/bias                      2.6e-06
#   b2049_ny1          4.3e-08  2.5e-07  1.1e-06  3.5e-06 dense_1/bias                      8.5e-06
#   t1                 6.1e-08  3.3e-08  5.6e-08  5.5e-07 gru_user_side gates/kernel        3.9e-07
#   t16                2.6e-08  2.3e-08  2.5e-08  1.8e-06 dense_1/bias                      1.5e-06
#   t17                6.8e-08  2.9e-08  5.2e-08  1.1e-06 dense_2/bias                      2.3e-06
#   t33                5.2e-08  2.7e-08  7.2e-08  4.2e-06 dense_1/bias                      5.6e-06
#   s2_t8              4.2e-08  6.1e-08  1.5e-07  1.4e-06 att_score                         1.7e-06
#   s2_t9              3.7e-08  7.5e-08  1.6e-07  2.4e-06 dense/bias                        2.0e-06
#   s4_ns3             4.7e-08  7.7e-08  2.0e-07  1.4e-06 dense_2/kernel                    1.7e-06
#   pool_in            5.2e-08  7.5e-08  1.7e-07  1.6e-06 att_score                         1.4e-06
#   pool_out           2.7e-08  7.5e-08  1.7e-07  1.6e-06 att_score                         1.6e-06
#   kq36_pad           4.6e-08  3.5e-08  5.7e-08  3.3e-06 dense/bias                        2.7e-05 (dense/bias, |g| ~ 1e-5: inside atol)
#   kq44               2.6e-08  4.7e-08  3.5e-08  9.3e-07 gru_item_side gates/bias          7.2e-07
#   kq52_pad           4.2e-08  3.9e-08  8.6e-08  3.1e-06 dense_1/bias                      4.3e-06
#   kq52_h48           6.3e-09  4.6e-08  5.3e-08  1.4e-06 dense/bias                        1.3e-06
#   kq84_pad           1.0e-07  3.4e-08  4.2e-08  1.2e-06 gru_item_side gates/bias          1.2e-06
#   kq148_pad          1.0e-08  5.5e-08  4.5e-08  1.0e-06 dense_3/kernel                    9.8e-07
#   rca_h36            2.3e-08  4.2e-08  7.9e-08  2.8e-06 dense_3/kernel                    1.4e-06
#   user_kq36          3.3e-08  6.0e-08  5.8e-08  1.3e-06 dense_4/kernel                    4.2e-06
#   item_kq36          8.8e-08  2.4e-08  2.0e-08  1.9e-06 dense_2/kernel                    4.2e-06
#   fwd_sep_bwd_fused  4.1e-08  2.9e-08  1.7e-08  1.3e-06 dense_2/bias                      1.5e-06
#   both_sep           8.8e-08  2.5e-08  1.2e-08  1.5e-06 dense_4/kernel                    7.3e-07
#   lds_s1_in          5.7e-08  3.5e-08  7.6e-08  5.6e-06 dense_5/kernel                    1.9e-06
#   lds_s1_out         6.1e-08  3.7e-08  9.0e-08  3.2e-05 dense/bias                        1.8e-05
#   lds_s4_in          1.6e-08  7.2e-08  1.7e-07  1.7e-06 dense_5/kernel                    2.4e-06
#   lds_s4_to_s2       5.4e-08  6.9e-08  2.2e-07  1.8e-06 dense/kernel                      2.5e-06
#   t129               1.4e-07  1.2e-08  6.0e-08  1.6e-06 dense/bias                        3.0e-06
#   lengths_over       2.3e-08  2.2e-08  5.1e-08  7.5e-07 dense_4/kernel                    6.7e-07
#   masks_b21          2.1e-08  4.6e-08  9.6e-08  2.2e-06 dense_3/bias                      2.9e-06
#   masks_b500         9.0e-08  7.3e-08  2.6e-07  5.6e-05 dense/bias                        5.7e-05 (dense/bias, |g| ~ 1e-5: inside atol)
# The parameter cases, at operator level: att_score against its float64 restatement from the kernel's a2 -- softmax_onehot 2.4e-22
# (every row one-hot to the last bit), softmax_uniform and dead_relus 9.9e-09 (1 / n in float32 against float64), sigmoid_01
# 1.7e-07; lossb and dlogit relative to their float64 restatement from the kernel's y_pred: at most 1.4e-07 and 1.2e-07.
