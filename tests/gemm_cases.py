"""The rows of tests/test_gpu_gemm_edges.py and their CPU twin (tests/test_gemm_cases_cpu.py): score_gemm's launch decision
(csrc/gemm.hip) restated in Python, a table whose rows each name the form they expect in the terms of score_gemm_last_form
(include/score_hip.h), the rows' inputs from fixed seeds, and the float64 reference with the bound the GPU test holds the kernels
to.  No GPU and no library is needed to import or evaluate anything here.

The bound is the project's own (tests/test_gpu_ops.py::test_gemm_fp32): |C - want| <= 2e-6 (|A| . |B|) + 1e-6 against the float64
product of the fp32 inputs, the epilogue applied in float64."""
from collections import namedtuple

import numpy as np

# ---------------------------------------------------------------------------------------------- the launch rule, restated
SPLITK_MIN_K, SPLITK_MIN_CHUNK, BK_ALIGN = 512, 128, 32      # csrc/gemm.hip: GEMM_SPLITK_MIN_K / _MIN_CHUNK, BK_ALIGN
F32, X3 = 1, 2                                                # the family field of score_gemm_last_form
GF_BIAS, GF_RELU, GF_ACC, GF_DROP, GF_X3, GF_X3F, GF_RELUGRAD = 1, 2, 4, 8, 16, 32, 64
E_BADARG = -1

Form = namedtuple("Form", "family wm wn slabs")              # wn = 0 for bf16x3 (its tile is always 128 columns wide)


def pack(form, trans, grouped=0):
    """a Form as score_gemm_last_form reports it behind a product of layout `trans`"""
    return form.family | form.wm << 2 | form.wn << 4 | trans << 6 | grouped << 8 | form.slabs << 12


def unpack(word):
    return Form(word & 3, word >> 2 & 3, word >> 4 & 3, word >> 12 & 0xFFFF), word >> 6 & 3, word >> 8 & 1


def cdiv(a, b):
    return -(-a // b)


def x3_ok(trans, M, N, K, lda, ldb, a_off, b_off):
    """may the bf16x3 kernel stage these operands?  a_off / b_off: the operands' distance in floats from a 16-byte boundary.
    k-contiguous operands (A unless trans 2, B when trans 1) need K % 4 == 0, the others a column count that is a multiple of 4"""
    al = lda % 4 == 0 and a_off % 4 == 0 and ldb % 4 == 0 and b_off % 4 == 0
    a_kc, b_kc = trans != 2, trans == 1
    return al and (K % 4 == 0 if a_kc else M % 4 == 0) and (K % 4 == 0 if b_kc else N % 4 == 0)


def x3_shape(trans, M, N, K):
    """where flag 16 alone takes the bf16x3 kernel ("where it measured faster")"""
    return (trans == 0 and M >= 4096 and N >= 64) or (trans == 1 and M >= 4096 and N >= 256) or \
           (trans == 2 and M * N >= 32768 and K >= 4096)


def _split(tiles, M, N, K, scratch, min_k, max_split):
    """slabs and chunk length of the reduced dimension: ~1.25 workgroups per CU, chunks multiples of 32, never more slabs than
    the scratch holds"""
    ns = 1
    if tiles < 256 and K >= min_k and scratch is not None:
        ns = min(cdiv(320, tiles), max_split)
        while ns > 1 and ns * M * N > scratch:
            ns -= 1
        ns = max(ns, 1)
    kc = K
    if ns > 1:
        kc = cdiv(cdiv(K, ns), BK_ALIGN) * BK_ALIGN
        ns = cdiv(K, kc)
    return ns, kc


def decide(trans, M, N, K, lda, ldb, flags, scratch, a_off=0, b_off=0):
    """(Form, k_chunk) of score_gemm.  scratch: floats of split-K scratch, None for a null pointer"""
    if flags & (GF_X3 | GF_X3F) and x3_ok(trans, M, N, K, lda, ldb, a_off, b_off) and M >= 64 and N >= 32 and K >= 32 and \
            (x3_shape(trans, M, N, K) or flags & GF_X3F):
        def rounds(wm):      # tiles the busiest CU gets; a 64-row tile costs 57 % of a 128-row one
            return cdiv(cdiv(N, 128) * cdiv(M, 64 * wm), 256) * (1.0 if wm == 2 else 0.57)
        wm = 1 if rounds(1) < rounds(2) else 2
        ns, kc = _split(cdiv(N, 128) * cdiv(M, 64 * wm), M, N, K, scratch, 512, K // 128)
        return Form(X3, wm, 0, ns), kc
    nblocks = lambda wm, wn: cdiv(N, 64 * wn) * cdiv(M, 64 * wm)
    ksplit_cap = K // SPLITK_MIN_CHUNK if K >= SPLITK_MIN_K and scratch is not None else 1
    wn = 2 if N > 64 and nblocks(1, 2) * ksplit_cap >= 384 else 1
    wm = 2 if M > 64 and nblocks(2, wn) * ksplit_cap >= 384 else 1
    ns, kc = _split(nblocks(wm, wn), M, N, K, scratch, SPLITK_MIN_K, K // SPLITK_MIN_CHUNK)
    return Form(F32, wm, wn, ns), kc


def slab_lengths(K, kc):
    return [min(kc, K - k) for k in range(0, K, kc)]


# ---------------------------------------------------------------------------------------------- the table
# route: 0, 16 (bf16x3 allowed where the shape rule says so) or 32 (forced wherever legal); eflags: the epilogue bits;
# mask: "" none, "byte" explicit keep mask, "hash" hashed from `seed`, "y" the layer's fp32 output for flag 64; g: bias row group;
# lda_pad / ldb_pad: floats between rows beyond the operand's own; a_off / b_off: floats into the allocation;
# scratch: "full" (room for every slab the rule could want), None (null pointer), or a number of floats, "short" = 4 M N - 1;
# kslabs: the lengths of the K chunks the row expects (their count is form.slabs); same_bits_as: a row of the same operands whose
# output must be equal bit for bit
Row = namedtuple("Row", "name trans M N K route eflags keep mask g lda_pad ldb_pad a_off b_off scratch form kslabs same_bits_as why")
ROWS = {}
SCRATCH_FULL = 1 << 22
HASH_SEED = 0x5EED0000C0FFEE


def _row(name, trans, M, N, K, form, route=0, eflags=0, keep=1.0, mask="", g=0, lda_pad=0, ldb_pad=0, a_off=0, b_off=0,
         scratch="full", kslabs=None, same_bits_as=None, why=""):
    name = "%s-t%d" % (name, trans)
    assert name not in ROWS, name
    if same_bits_as is not None:
        same_bits_as = "%s-t%d" % (same_bits_as, trans)
    ROWS[name] = Row(name, trans, M, N, K, route, eflags, keep, mask, g, lda_pad, ldb_pad, a_off, b_off, scratch, Form(*form),
                     kslabs if kslabs is not None else [K] * 1, same_bits_as, why)


EPILOGUES = [          # (tag, eflags, keep, mask, g as a function of M)
    ("plain", 0, 1.0, "", None), ("bias", 1, 1.0, "", None), ("bias_relu", 1 | 2, 1.0, "", None), ("acc", 4, 1.0, "", None),
    ("bias_acc", 1 | 4, 1.0, "", None), ("drop_bytes", 1 | 2 | 8, 0.8, "byte", None), ("drop_hash", 1 | 8, 0.8, "hash", None),
    ("relugrad", 64, 1.0, "y", None), ("relugrad_keep", 64, 0.8, "y", None),
    ("bias_g3", 1 | 2, 1.0, "", lambda M: 3), ("bias_gbig", 1 | 2, 1.0, "", lambda M: M + 5)]

for t in (0, 1, 2):
    # -- f32 tile forms at their seams, K = 16, no scratch.  With N = 65 the rule's seams in M are: (1,1) up to 24448 (two column
    # blocks of 191 row pairs = 382 < 384), (2,1) from 24449 to 24512 (2 x 192 = 384, while one 128-column block of 383 rows of 64
    # is still short), (1,2) from 24513 (384 blocks of 64 x 128) to 49024, (2,2) from 49025.
    _row("seam_24448x65", t, 24448, 65, 16, (F32, 1, 1, 1), scratch=None, why="last M of the (1,1) form at N = 65")
    _row("seam_24449x65", t, 24449, 65, 16, (F32, 2, 1, 1), scratch=None, why="first M of (2,1) at N = 65")
    _row("seam_24512x65", t, 24512, 65, 16, (F32, 2, 1, 1), scratch=None, why="last M before (1,2): 2 x 192 blocks of 128 x 64")
    _row("seam_24513x65", t, 24513, 65, 16, (F32, 1, 2, 1), scratch=None, why="first M of (1,2)")
    _row("seam_49024x65", t, 49024, 65, 16, (F32, 1, 2, 1), scratch=None, why="last M of (1,2)")
    _row("seam_49025x65", t, 49025, 65, 16, (F32, 2, 2, 1), scratch=None, why="first M of (2,2): the largest row of the table")
    _row("seam_49025x64", t, 49025, 64, 16, (F32, 2, 1, 1), scratch=None, why="N = 64 never widens")
    _row("seam_49025x5", t, 49025, 5, 16, (F32, 2, 1, 1), scratch=None, why="a sliver of columns")
    # -- f32 forms reached through ksplit_cap
    _row("cap_6081x65", t, 6081, 65, 512, (F32, 1, 2, 4), kslabs=[128] * 4, why="(1,2) only because four slabs multiply the grid")
    _row("cap_6081x65_short", t, 6081, 65, 512, (F32, 1, 2, 3), scratch="short", kslabs=[192, 192, 128],
         why="scratch one float short of four slabs: the --nsplit loop, chunks re-rounded to 32")
    _row("cap_12288x64", t, 12288, 64, 512, (F32, 2, 1, 4), kslabs=[128] * 4, why="(2,1) behind split-K")
    # -- the K loop of the two-register-set pipeline
    for K in (1, 15, 16, 17, 31, 32, 33, 48, 49):
        _row("kloop_%d" % K, t, 70, 40, K, (F32, 1, 1, 1), eflags=1, why="K-loop edge of the staged pipeline")
    # -- bf16x3's two tile heights, forced: 257 tiles of 64 rows are two rounds (1.14), 129 of 128 rows one
    _row("x3_tall", t, 16388, 36, 32, (X3, 2, 0, 1), route=32, why="wm = 2 by the rounds rule")
    _row("x3_forced", t, 72, 40, 48, (X3, 1, 0, 1), route=32, why="the control of the refusal rows: legal, so taken")
    # -- every x3_ok refusal under flag 32 lands on the f32 kernel (or, where the rule does not look at that operand, does not)
    _row("refuse_a_base", t, 72, 40, 48, (F32, 1, 1, 1), route=32, a_off=1, lda_pad=0, why="A one float off a 16-byte boundary")
    _row("refuse_b_base", t, 72, 40, 48, (F32, 1, 1, 1), route=32, b_off=1, why="B one float off a 16-byte boundary")
    _row("refuse_lda", t, 72, 40, 48, (F32, 1, 1, 1), route=32, lda_pad=1, why="lda % 4 = 1")
    _row("refuse_ldb", t, 72, 40, 48, (F32, 1, 1, 1), route=32, ldb_pad=2, why="ldb % 4 = 2")
    # -- leading dimensions and views, f32: the scalar path of load_quad must give the bits of the vector path
    # (ld % 4 == 0 on both sides, so that the aligned copies take the 16-byte loads with the `c + 3 < clim` guard live -- M = 70
    # and K = 590 end inside a quad -- and the views the guarded scalars)
    pa, pb = (2 if t == 2 else 4), (4 if t == 1 else 8)
    _row("ld_base", t, 70, 40, 48, (F32, 1, 1, 1), eflags=1, why="lda = K (M for layout 2), ldb = N (K): the copy the others are compared with")
    _row("ld_wide", t, 70, 40, 48, (F32, 1, 1, 1), eflags=1, lda_pad=pa, ldb_pad=pb, same_bits_as="ld_base",
         why="lda = K + 4 (M + 2), ldb wider, both % 4 == 0")
    for off in (1, 2, 3):
        _row("ld_view%d" % off, t, 70, 40, 48, (F32, 1, 1, 1), eflags=1, lda_pad=pa, ldb_pad=pb, a_off=off, b_off=off,
             same_bits_as="ld_base", why="A and B %d floats into their allocations, ld %% 4 == 0: guarded scalar loads" % off)
    pa, pb = (4 if t == 2 else 2), (2 if t == 1 else 4)
    _row("ld_split_base", t, 200, 72, 590, (F32, 1, 1, 4), eflags=1, lda_pad=pa, ldb_pad=pb, kslabs=[160, 160, 160, 110],
         why="aligned copy behind split-K: chunks of 160, the last ends two floats into a quad")
    _row("ld_split_view", t, 200, 72, 590, (F32, 1, 1, 4), eflags=1, a_off=3, b_off=1, lda_pad=pa, ldb_pad=pb,
         kslabs=[160, 160, 160, 110], same_bits_as="ld_split_base", why="the same operands as views: scalar loads behind split-K")
    # -- epilogues: directly in the kernel at (70, 40, 48), in splitk_reduce_kernel at (200, 72, 512); f32 and forced bf16x3.
    # Layout 2 stages A in 4 x 4 blocks of its M columns, so M = 70 is refused there (refuse_m below): its forced rows have 76
    for tag, ef, keep, mask, gf in EPILOGUES:
        for fam in ("f32", "x3"):
            Ms = 76 if (fam == "x3" and t == 2) else 70
            _row("ep_%s_%s_direct" % (tag, fam), t, Ms, 40, 48, (F32, 1, 1, 1) if fam == "f32" else (X3, 1, 0, 1),
                 route=0 if fam == "f32" else 32, eflags=ef, keep=keep, mask=mask, g=gf(Ms) if gf else 0, why="epilogue in the kernel")
            _row("ep_%s_%s_split" % (tag, fam), t, 200, 72, 512, (F32, 1, 1, 4) if fam == "f32" else (X3, 1, 0, 4),
                 route=0 if fam == "f32" else 32, eflags=ef, keep=keep, mask=mask, g=gf(200) if gf else 0, kslabs=[128] * 4,
                 why="epilogue in splitk_reduce_kernel")
    # -- one (M, N, seed) in all four places the hashed mask is computed (ep_drop_hash_*_split are the other two)
    _row("hash_f32_direct", t, 200, 72, 48, (F32, 1, 1, 1), eflags=1 | 8, keep=0.8, mask="hash", why="hashed mask, f32 kernel")
    _row("hash_x3_direct", t, 200, 72, 48, (X3, 1, 0, 1), route=32, eflags=1 | 8, keep=0.8, mask="hash", why="hashed mask, bf16x3 kernel")

# what the rule looks at depends on the layout: K % 4 for k-contiguous operands, M % 4 / N % 4 for the strided ones
_row("refuse_k", 0, 72, 40, 50, (F32, 1, 1, 1), route=32, why="A[M,K] is k-contiguous: K % 4 = 2 refuses")
_row("refuse_k", 1, 72, 40, 50, (F32, 1, 1, 1), route=32, why="both operands k-contiguous")
_row("refuse_k", 2, 72, 40, 50, (X3, 1, 0, 1), route=32, why="neither operand is k-contiguous: K % 4 is not looked at, the K tail runs in bf16x3")
_row("refuse_m", 0, 70, 40, 48, (X3, 1, 0, 1), route=32, why="M % 4 is not looked at for A[M,K]")
_row("refuse_m", 1, 70, 40, 48, (X3, 1, 0, 1), route=32, why="M % 4 is not looked at for A[M,K]")
_row("refuse_m", 2, 70, 40, 48, (F32, 1, 1, 1), route=32, why="A[K,M] is staged in 4 x 4 blocks: M % 4 = 2 refuses")
_row("refuse_n", 0, 72, 42, 48, (F32, 1, 1, 1), route=32, why="B[K,N]: N % 4 = 2 refuses")
_row("refuse_n", 1, 72, 42, 48, (X3, 1, 0, 1), route=32, why="B[N,K] is k-contiguous: N % 4 is not looked at")
_row("refuse_n", 2, 72, 42, 48, (F32, 1, 1, 1), route=32, why="B[K,N]: N % 4 = 2 refuses")
# -- flag 16 at the thresholds of its shape rule
_row("x3rule_4096x64", 0, 4096, 64, 32, (X3, 1, 0, 1), route=16, why="trans 0: M >= 4096 and N >= 64")
_row("x3rule_4095x64", 0, 4095, 64, 32, (F32, 1, 1, 1), route=16, why="one row short")
_row("x3rule_4096x60", 0, 4096, 60, 32, (F32, 1, 1, 1), route=16, why="N < 64")
_row("x3rule_4096x256", 1, 4096, 256, 32, (X3, 1, 0, 1), route=16, why="trans 1: M >= 4096 and N >= 256")
_row("x3rule_4096x252", 1, 4096, 252, 32, (F32, 1, 1, 1), route=16, why="N < 256")
_row("x3rule_k4096", 2, 256, 128, 4096, (X3, 1, 0, 32), route=16, kslabs=[128] * 32, why="trans 2: M N >= 32768 and K >= 4096, split-K")
_row("x3rule_k4092", 2, 256, 128, 4092, (F32, 1, 1, 26), route=16, kslabs=[160] * 25 + [92], why="K < 4096: f32, 26 slabs")

BADARG_ROWS = [("relugrad_with_drop", 64 | 8, "y"), ("relugrad_null_mask", 64, "")]      # (name, flags, mask) at (70, 40, 48)

# every kernel instance the launcher can take: (family, trans, wm, wn)
ALL_INSTANCES = {(F32, t, wm, wn) for t in (0, 1, 2) for wm in (1, 2) for wn in (1, 2)} | {(X3, t, wm, 0) for t in (0, 1, 2) for wm in (1, 2)}


def scratch_floats(r):
    if r.scratch is None:
        return None
    if r.scratch == "short":
        return 4 * r.M * r.N - 1
    return SCRATCH_FULL


def kernel_flags(r):
    return r.route | r.eflags | r.g << 16


def ld(r):
    """(lda, ldb) of the stored operands"""
    return (r.M if r.trans == 2 else r.K) + r.lda_pad, (r.K if r.trans == 1 else r.N) + r.ldb_pad


def mirror(r):
    lda, ldb = ld(r)
    return decide(r.trans, r.M, r.N, r.K, lda, ldb, kernel_flags(r), scratch_floats(r), r.a_off, r.b_off)


# ---------------------------------------------------------------------------------------------- inputs
def hash_uniform(seed, idx):
    """csrc/common.h hash_uniform: splitmix64's finaliser of (seed, idx), the top 24 bits as a float32 in [0, 1)"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (idx.astype(np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def hashed_keep(seed, M, N, keep):
    e = np.arange(M * N, dtype=np.uint64).reshape(M, N)
    return hash_uniform(seed, e) < np.float32(keep)


Inputs = namedtuple("Inputs", "a b A B bias c0 mask y keepmask")


def _operand_seed(r):
    """rows that must agree bit for bit share their operands: the seed leaves out what only places them in memory"""
    return [r.trans, r.M, r.N, r.K, r.eflags, r.g, int(r.keep * 100)]


def _stored(x, pad, off):
    """x [rows, cols] float32 as a view `off` floats into an allocation with `pad` more floats per row; everything a kernel must not
    read is NaN"""
    rows, cols = x.shape
    buf = np.full(off + rows * (cols + pad) + 4, np.nan, dtype=np.float32)
    view = buf[off:off + rows * (cols + pad)].reshape(rows, cols + pad)
    view[:, :cols] = x
    return buf, view


def inputs(r):
    """a [M, K], b [K, N]: the product's logical operands; A / B: (allocation, stored view) in the row's layout; bias [rows, N];
    c0 [M, N + 3]: C before the call (read by flag 4; its last three columns are the canary); mask: bytes or None; y: float32 or
    None; keepmask: which elements the epilogue keeps (dropout / flag 64), None if all"""
    rng = np.random.default_rng(_operand_seed(r))
    a = rng.standard_normal((r.M, r.K)).astype(np.float32)
    b = rng.standard_normal((r.K, r.N)).astype(np.float32)
    nb = cdiv(r.M, r.g) if r.g else 1
    bias = rng.standard_normal((nb, r.N)).astype(np.float32)
    c0 = rng.standard_normal((r.M, r.N + 3)).astype(np.float32)
    mask = y = keepmask = None
    if r.mask == "byte":
        keepmask = rng.random((r.M, r.N)) < r.keep
        mask = keepmask.astype(np.uint8) * np.uint8(1 + 4 * (r.M % 2))      # any non-zero byte keeps
    elif r.mask == "hash":
        keepmask = hashed_keep(HASH_SEED, r.M, r.N, r.keep)
    elif r.mask == "y":
        y = rng.standard_normal((r.M, r.N)).astype(np.float32)
        y[rng.random((r.M, r.N)) < 0.3] = 0.0                                # a relu output: exact zeros among positives ...
        y[0, 0] = -0.0
        keepmask = y > 0
    A = _stored(a.T.copy() if r.trans == 2 else a, r.lda_pad, r.a_off)
    B = _stored(b.T.copy() if r.trans == 1 else b, r.ldb_pad, r.b_off)
    return Inputs(a, b, A, B, bias, c0, mask, y, keepmask)


# ---------------------------------------------------------------------------------------------- the reference and the bound
def bias_rows(r, bias, shift=0):
    """the bias row of each output row: one row, or one per group of g rows (shift: the perturbation (r + 1) / g)"""
    if not r.g:
        return np.broadcast_to(bias[0], (r.M, r.N))
    return bias[np.minimum((np.arange(r.M) + shift) // r.g, bias.shape[0] - 1)]


def epilogue64(r, prod, inp, bias_shift=0, keepmask=None):
    """what the kernels do to the product before they store it, in float64; returns (want, pre): pre = the relu's argument"""
    v = prod.astype(np.float64)
    if r.eflags & GF_BIAS:
        v = v + bias_rows(r, inp.bias, bias_shift).astype(np.float64)
    pre = v
    if r.eflags & GF_RELU:
        v = np.maximum(v, 0.0)
    km = inp.keepmask if keepmask is None else keepmask
    if r.eflags & (GF_DROP | GF_RELUGRAD):
        v = np.where(km, v / np.float64(np.float32(r.keep)), 0.0)
    if r.eflags & GF_ACC:
        v = v + inp.c0[:, :r.N].astype(np.float64)
    return v, pre


def reference(r, inp):
    """(want [M, N] float64, tol [M, N], skip [M, N] bool): skip marks the elements whose relu argument, or whose flag-64 Y, lies
    within the bound of zero (either side of the kink is then a correct answer of an fp32 product)"""
    prod = inp.a.astype(np.float64) @ inp.b.astype(np.float64)
    tol = 2e-6 * (np.abs(inp.a).astype(np.float64) @ np.abs(inp.b).astype(np.float64)) + 1e-6
    want, pre = epilogue64(r, prod, inp)
    skip = np.zeros((r.M, r.N), dtype=bool)
    if r.eflags & GF_RELU:
        skip |= np.abs(pre) <= tol
    if r.eflags & GF_RELUGRAD:
        skip |= (np.abs(inp.y.astype(np.float64)) <= tol) & (inp.y != 0)       # (an exact zero is not near the kink: it IS off)
    return want, tol, skip


SKIP_CAP = 0.01


def judge(got, want, tol, skip):
    """worst |got - want| / tol over the elements that are not skipped (<= 1 passes); NaN counts as infinitely wrong"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want) / tol
    err = np.where(np.isnan(err), np.inf, err)
    return float(np.where(skip, 0.0, err).max())
