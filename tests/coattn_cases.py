"""The fused gather + co-attention kernels (csrc/embed.hip) at every instance, geometry and K seam: the launch rules restated
in Python in the terms of score_coattn_last_forms (include/score_hip.h), a table whose rows each name the forms they promise,
the inputs of every row, float64 references of the forward and of the backward, a float32 restatement that measures what the
bounds leave, and the judge.  tests/test_coattn_cases_cpu.py checks all of it without a GPU; tests/test_gpu_coattn_edges.py
runs the rows.

The mirror restates coattn_geom, coattn_ksh, coattn_meta_regs, coattn_fwd_units_regs, COATTN_DISPATCH's KMAX choice,
coattn_bwd_ahead's NM choice and coattn_check's refusals, and nothing else (the chunk length CH of the forward word comes from
score_coattn_fwd_chunk, the library's own host-side query).

Bounds (the project's, tests/test_gpu_ops.py::test_coattn_fwd_bwd): forward 1e-5 of the largest reference magnitude per
output; backward rtol 2e-4, atol 2e-5; info[:, :K] == K * rsave bit for bit; mode 1 equals the int64 sums bit for bit.

Where a row stands apart from what one might expect:
  * B = T = 1 launches hold one unit, so with K = 1 they cannot mix active and inactive scores: the active / inactive
    condition (a quarter each) is asserted on a row's large launch.
  * With GS = 64 a wave holds one unit (upw = 1) and every count is a multiple of upw: there the large count is no multiple
    of 4 (a ragged last workgroup); with upw > 1 it is no multiple of upw either (a ragged last wave).
  * W is drawn at 1 / sqrt(2 Dx), so that scores are of order 1 at every width: at Dx = 1024 a score of order 10 leaves the
    float32 restatement more than a quarter of the forward bound.  No bound is widened.
  * Six rows draw their gradients four times smaller (GRAD_SCALE), so that the float32 restatement keeps to a quarter of
    the backward bound.
  * Model rows: ATOMIC = false is the model's pull-form pass alone, whose plan path takes Fu, Fi <= 8.  Four of the 40
    backward instances are reached by no legal shape (BWD_UNREACHED in the CPU twin, with the reason): ATOMIC = false at
    SPL = 2 with (KMAX, NM) = (4, 0), (10, 0), (4, 2), (10, 4).  Eight model rows beyond the issue's eight reach the other
    ATOMIC = false instances.

Measured on the MI355X (worst ratio of an error to its bound over all rows; the GPU module prints every row's with -s); no
row failed, faulted or differed between two runs:
  forward   out1 0.034 (d256_f2_k32), out2 0.023 (d64_f13_k20), info and rsave 0.180 (d8_f40_k2)
  backward  dW 0.512 (d256_f3_k20; 0.213 in the float32 restatement: a weight gradient that cancels to ~0.01 out of terms of
            order 10), every other row's dW at most 0.22; table gradient 0.020 (d4_f1_k5); dzsum 0.058 (d64_f9_k10)
  model     0.017 (spl1_in_spl4, both scatter modes)
  mode 1    exact, as it must be
"""
import collections
import functools

import numpy as np

E_BADARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
N_ROWS = 300                       # rows of every row's table; row 0 is the zero row
CANARY = np.float32(-7777.25)
FWD_BOUND, RTOL, ATOL = 1e-5, 2e-4, 2e-5
MARGIN = 1e-4                      # every pre-relu score of a built row is at least this far from the kink (float64)

# ------------------------------------------------------------------------------------------------ the mirror
Fwd = collections.namedtuple("Fwd", "units kmax reg ch")            # reg: SPL (one-unit kernel) or NM (units kernel)
Bwd = collections.namedtuple("Bwd", "kmax spl nm atomic mode")


def pack_fwd(f):
    return f.units | f.kmax << 1 | f.reg << 8 | f.ch << 12


def pack_bwd(b):
    return b.kmax << 1 | b.spl << 8 | b.nm << 12 | b.atomic << 16 | b.mode << 20


def unpack_fwd(w):
    return Fwd(w & 1, w >> 1 & 63, w >> 8 & 7, w >> 12 & 0xFFFF)


def unpack_bwd(w):
    return Bwd(w >> 1 & 63, w >> 8 & 7, w >> 12 & 7, w >> 16 & 1, w >> 20 & 3)


def geom(D, F):
    """coattn_geom: (GS, SPL, nslots)"""
    nslots = F * (D // 4)
    gs = 1
    while gs < nslots and gs < 64:
        gs <<= 1
    return gs, (nslots + gs - 1) // gs, nslots


def ksh(GS, F):
    """coattn_ksh: log2 of the neighbours per id register; -1: a feature set does not fit a group"""
    if F > GS:
        return -1
    sh = 0
    while (2 << sh) * F <= GS:
        sh += 1
    return sh


def meta_regs(GS, F, K):
    """coattn_meta_regs"""
    s = ksh(GS, F)
    if s < 0:
        return 0
    return max((K + (1 << s) - 1) >> s, (3 * K + GS - 1) // GS)


def fwd_units_regs(D, K, mode, Fs):
    """coattn_fwd_units_regs (with coattn_fwd_id_regs)"""
    if mode != 0 or K > 10:
        return 0
    need = 1
    for F in Fs:
        GS, SPL, _ = geom(D, F)
        s = ksh(GS, F)
        n = 0 if s < 0 else (K + (1 << s) - 1) >> s
        if SPL != 1 or n == 0 or n > (2 if K <= 4 else 1):
            return 0
        need = max(need, n)
    return need


def dispatch_kmax(spl, K):
    """the KMAX COATTN_DISPATCH takes"""
    if spl <= 2:
        return 4 if K <= 4 else 10 if K <= 10 else 20 if K <= 20 else 32
    return 10 if K <= 10 else 20


def launch_spl(D, Fs):
    spl = max(geom(D, F)[1] for F in Fs)
    return 4 if spl == 3 else spl


def fwd_form(D, Fs, K, mode, ch=1):
    """the forward's form for the calls Fs of one grid; ch: what score_coattn_fwd_chunk answers (used by the units kernel only)"""
    nm = fwd_units_regs(D, K, mode, Fs)
    if nm > 0:
        return Fwd(1, 4, nm, ch) if K <= 4 else Fwd(1, 10, 1, ch)
    spl = launch_spl(D, Fs)
    return Fwd(0, dispatch_kmax(spl, K), spl, 0)


def bwd_form(D, Fs, K, mode, atomic=1):
    """the backward's form: coattn_bwd_ahead's instance where the lists of every call fit one, COATTN_DISPATCH's otherwise"""
    spl = launch_spl(D, Fs)
    need = 1 if mode == 0 and spl <= 2 else 0
    for F in Fs:
        if need == 0:
            break
        n = meta_regs(geom(D, F)[0], F, K)
        need = 0 if n == 0 else max(n, need)
    nm = 0
    if 1 <= need <= 4 and K <= 10 and not (K <= 4 and need > 2):
        nm = 4 if need == 3 else need
    return Bwd(4 if K <= 4 else 10, spl, nm, atomic, mode) if nm else Bwd(dispatch_kmax(spl, K), spl, 0, atomic, mode)


def check(table_ok, n_rows, D, F, K, B, T):
    """coattn_check"""
    if not table_ok or n_rows <= 0 or B <= 0 or T <= 0:
        return E_BADARG
    if D <= 0 or D & 3 or D > 256 or F <= 0 or K <= 0 or K > 32:
        return E_SHAPE
    if F * (D // 4) > 256:
        return E_SHAPE
    if F * (D // 4) > 128 and K > 20:
        return E_SHAPE
    return 0


def fwd_name(f):
    return ("units<%d,%d>" if f.units else "one-unit<%d,%d>") % (f.kmax, f.reg)


# ------------------------------------------------------------------------------------------------ the rows
# (D, F, K) -> backward (SPL, KMAX, NM) and the forward form as the issue that asked for this table states them ("one-unit":
# the kernel alone, the instance is the mirror's).  ROWS below takes its forms from the mirror; the CPU twin holds the two
# against each other.
STATED = {}
for _shapes, _bwd, _fwd in (
        (((4, 1, 1),), (1, 4, 0), "units<4,1>"),                      # GS = 1: 64 units per wave
        (((4, 1, 5),), (1, 10, 0), "one-unit<10,1>"),
        (((4, 2, 3),), (1, 4, 0), "one-unit<4,1>"),                   # GS = 2
        (((4, 3, 2),), (1, 4, 2), "units<4,2>"),
        (((4, 3, 4),), (1, 4, 0), "one-unit"),
        (((8, 3, 3),), (1, 4, 2), "units<4,2>"),
        (((8, 3, 7),), (1, 10, 4), "one-unit"),
        (((8, 3, 10),), (1, 10, 0), "one-unit"),
        (((16, 4, 5), (16, 4, 8)), (1, 10, 2), "one-unit<10,1>"),
        (((16, 4, 10), (16, 3, 10)), (1, 10, 4), "one-unit"),         # (16, 3, 10): need 3 -> NM 4
        (((64, 4, 4),), (1, 4, 1), "units<4,1>"),
        (((64, 4, 5), (64, 4, 10), (64, 3, 10)), (1, 10, 1), "units<10,1>"),
        (((64, 4, 11), (64, 4, 20)), (1, 20, 0), "one-unit<20,1>"),
        (((64, 4, 21), (64, 4, 32), (256, 1, 32)), (1, 32, 0), "one-unit<32,1>"),
        (((4, 64, 3),), (1, 4, 0), "one-unit"),                       # need 3 at K <= 4
        (((4, 65, 2),), (2, 4, 0), "one-unit<4,2>"),                  # F > GS, 65 slots: one live lane in the second slot
        (((4, 65, 10),), (2, 10, 0), "one-unit<10,2>"),
        (((8, 40, 2),), (2, 4, 2), "one-unit"),
        (((8, 40, 4),), (2, 4, 0), "one-unit"),
        (((32, 12, 8), (64, 5, 10)), (2, 10, 2), "one-unit"),         # 96 / 80 slots: a partly live second slot
        (((32, 12, 10),), (2, 10, 4), "one-unit"),
        (((128, 4, 4),), (2, 4, 1), "one-unit<4,2>"),
        (((128, 4, 10), (128, 3, 10)), (2, 10, 1), "one-unit<10,2>"),
        (((128, 4, 11), (128, 4, 20)), (2, 20, 0), "one-unit<20,2>"),
        (((128, 4, 21), (128, 4, 32), (256, 2, 32), (64, 5, 32)), (2, 32, 0), "one-unit<32,2>"),
        (((64, 9, 1), (64, 9, 10), (64, 12, 10), (64, 13, 10), (256, 4, 10)), (4, 10, 0), "one-unit<10,4>"),
        (((64, 9, 11), (64, 9, 20), (64, 13, 20), (256, 3, 20), (256, 4, 20)), (4, 20, 0), "one-unit<20,4>")):
    for _s in _shapes:
        STATED[_s] = (_bwd, _fwd)

Row = collections.namedtuple("Row", "name D F K mode fwd bwd planted")
T_BIG = 3


def big_B(D, F):
    """samples of a row's large launch at T = 3: more than two workgroups of units, a ragged last workgroup and (where a wave
    holds more than one unit) a ragged last wave"""
    upw = 64 // geom(D, F)[0]
    B = 8 * upw // T_BIG + 1
    while not (T_BIG * B > 8 * upw and (T_BIG * B) % (4 * upw) and (upw == 1 or (T_BIG * B) % upw)):
        B += 1
    return B


def _row(D, F, K, mode=0, planted=False):
    name = "%sd%d_f%d_k%d" % ("planted_" if planted else "rca_" if mode else "", D, F, K)
    return Row(name, D, F, K, mode, None if planted else fwd_form(D, (F,), K, mode), bwd_form(D, (F,), K, mode), planted)


PLANTED_SHAPES = ((64, 4, 10), (128, 4, 20), (256, 4, 20), (64, 4, 32), (8, 3, 7))
# one mode 1 row per (SPL, KMAX) pair of the table
MODE1_SHAPES = ((4, 2, 3), (16, 4, 8), (64, 4, 20), (256, 1, 32), (4, 65, 2), (32, 12, 10), (128, 4, 11), (64, 5, 32), (64, 9, 1),
                (256, 3, 20))
ROWS = collections.OrderedDict()
for _s in STATED:
    _r = _row(*_s)
    ROWS[_r.name] = _r
for _s in PLANTED_SHAPES:
    _r = _row(*_s, planted=True)
    ROWS[_r.name] = _r
for _s in MODE1_SHAPES:
    _r = _row(*_s, mode=1)
    ROWS[_r.name] = _r
COUNTS = ("one", "big")            # B = T = 1, and big_B x 3
# Rows whose float32 restatement left more than a quarter of the backward bound at gradients of order 1 (dW entries that
# cancel to ~0.01 out of terms of order 10, at K >= 20 and four features: 0.27 .. 0.76 of the bound): their g1, g2 and ginfo
# are drawn four times smaller.  The bounds stay.
GRAD_SCALE = {"d128_f4_k32": 0.25, "d256_f2_k32": 0.25, "d64_f5_k32": 0.25, "d256_f4_k20": 0.25, "planted_d128_f4_k20": 0.25,
              "planted_d256_f4_k20": 0.25}


def dims(r, count):
    return (1, 1) if count == "one" else (big_B(r.D, r.F), T_BIG)


# refusals: host only, nothing launched.  name -> (D, F, K, ld1 padding, what is null, scratch short, the code)
REFUSALS = collections.OrderedDict((
    ("d6", (6, 2, 3, 4, None, False, E_SHAPE)),
    ("d260", (260, 1, 3, 4, None, False, E_SHAPE)),
    ("slots257", (4, 257, 3, 4, None, False, E_SHAPE)),
    ("k33", (16, 2, 33, 4, None, False, E_SHAPE)),
    ("k21_slots129", (4, 129, 21, 4, None, False, E_SHAPE)),
    ("ld1_odd", (16, 2, 3, 2, None, False, E_SHAPE)),
    ("null_idx", (16, 2, 3, 4, "idx1", False, E_BADARG)),
    ("null_table", (16, 2, 3, 4, "table", False, E_BADARG)),
    ("null_mode0", (16, 2, 3, 4, "mode0", False, E_BADARG)),      # W / rsave: null is legal in mode 1 only
    ("scratch_short", (16, 2, 3, 4, None, True, E_WORKSPACE)),
))

# model rows (two calls in one grid): name -> (D, Fu, Fi, K, B, T, slices computed, model type, seed)
MODEL_ROWS = collections.OrderedDict((
    ("spl1_in_spl2", (128, 1, 4, 10, 5, 4, 4, "SCORE", 1)),        # 32 and 128 slots
    ("spl1_in_spl4", (256, 1, 4, 10, 5, 4, 4, "SCORE", 1)),        # 64 and 256 slots
    ("spl4_k20", (256, 3, 4, 20, 4, 3, 3, "SCORE", 1)),            # 192 (three slots run as four) and 256 slots
    ("spl2_k4", (128, 3, 4, 4, 6, 4, 4, "SCORE", 1)),              # SPL 2, KMAX 4, NM 1
    ("spl2_k32", (128, 3, 4, 32, 4, 3, 3, "SCORE", 1)),
    ("spl1_k32", (64, 3, 4, 32, 5, 4, 4, "SCORE", 1)),
    ("need_of_two_calls", (32, 5, 8, 8, 6, 5, 3, "SCORE", 1)),     # SPL 1 + SPL 1, fewer slices computed than T; NM: below
    ("rca", (64, 3, 4, 10, 6, 4, 4, "RCA", 1)),                    # mode 1
    # the remaining ATOMIC = false instances a model shape reaches (scatter_mode 0 is their only route)
    ("gs2_k2", (8, 1, 1, 2, 9, 4, 4, "SCORE", 1)),                 # GS = 2, need 3 at K <= 4: NM 0, KMAX 4
    ("spl1_k4", (64, 3, 4, 4, 6, 4, 4, "SCORE", 1)),               # KMAX 4, NM 1
    ("gs8_k3", (8, 3, 3, 3, 9, 4, 4, "SCORE", 1)),                 # KMAX 4, NM 2
    ("gs8_k10", (8, 3, 3, 10, 9, 4, 4, "SCORE", 1)),               # five id registers wanted: KMAX 10, NM 0
    ("gs16_k8", (16, 3, 4, 8, 7, 4, 4, "SCORE", 1)),               # KMAX 10, NM 2
    ("gs16_k10", (16, 3, 4, 10, 7, 4, 4, "SCORE", 1)),             # KMAX 10, NM 4
    ("gs16_k12", (16, 3, 4, 12, 7, 4, 4, "SCORE", 1)),             # KMAX 20, SPL 1
    ("spl2_nm2", (64, 3, 5, 10, 5, 4, 4, "SCORE", 1)),             # 48 and 80 slots: SPL 1 (need 1) inside SPL 2 with need 2
    ("spl2_k12", (128, 3, 4, 12, 4, 3, 3, "SCORE", 1)),            # KMAX 20, SPL 2
))


def model_forms(name, scatter_mode, ch=1):
    D, Fu, Fi, K = MODEL_ROWS[name][:4]
    mode = 1 if MODEL_ROWS[name][7] == "RCA" else 0
    return fwd_form(D, (Fi, Fu), K, mode, ch), bwd_form(D, (Fi, Fu), K, mode, 1 if scatter_mode == 1 else 0)


# ------------------------------------------------------------------------------------------------ inputs
Inputs = collections.namedtuple("Inputs", "B T table idx1 idx2 tgt W bias g1 g2 ginfo rsave ld1 ldi")


def _clamp(idx):
    return np.where((idx < 0) | (idx >= N_ROWS), 0, idx)


def _draw_ids(rng, B, T, K, F):
    idx1 = rng.integers(1, N_ROWS, (B, T, K, F)).astype(np.int32)
    idx2 = rng.integers(1, N_ROWS, (B, T, K, F)).astype(np.int32)
    n = B * T
    a, b = idx1.reshape(n, K, F), idx2.reshape(n, K, F)
    a[rng.random(a.shape) < 0.08] = 0                      # id 0 inside live units
    b[rng.random(b.shape) < 0.08] = 0
    if K > 1:
        a[1::3, K - 1] = a[1::3, 0]                        # the same id several times in a unit
        b[2::3, K // 2] = b[2::3, 0]
    b[::2, 0] = a[::2, K - 1]                              # the same id in idx1 and idx2 of one unit: both passes add to one row
    if n > 1:                                              # a few ids outside the table, last: read as row 0, no gradient
        a[n // 2, 0, 0], a[n - 1, K - 1, F - 1] = N_ROWS, -3
        b[n // 3, K - 1, 0], b[n - 2, 0, F - 1] = 10 ** 6, N_ROWS + 5
    elif K * F >= 4:
        a[0, K - 1, F - 1], b[0, 0, F - 1] = N_ROWS, -3
    return idx1, idx2


@functools.lru_cache(maxsize=None)
def inputs(name, count):
    """the inputs of a row at one of its two unit counts: read-only, drawn once"""
    r = ROWS[name]
    B, T = dims(r, count)
    D, F, K = r.D, r.F, r.K
    Dx, n = F * D, B * T
    base = sum(ord(c) for c in name) * 7 + (1 if count == "big" else 0)
    ld1, ldi = Dx + 4, 2 * K + 1
    if r.mode == 1:                                        # small integers: every sum is exact in float32
        rng = np.random.default_rng(base)
        table = rng.integers(-3, 4, (N_ROWS, D)).astype(np.float32)
        table[0] = 0
        idx1, idx2 = _draw_ids(rng, B, T, K, F)
        g1 = rng.integers(-2, 3, (n, Dx)).astype(np.float32)
        g2 = rng.integers(-2, 3, (n, Dx)).astype(np.float32)
        out = Inputs(B, T, table, idx1, idx2, None, None, None, g1, g2, None, None, ld1, ldi)
    else:
        for attempt in range(64):                          # redrawn, deterministically, until no score sits near the kink
            rng = np.random.default_rng(base + 1000 * attempt)
            table = rng.standard_normal((N_ROWS, D)).astype(np.float32)
            table[0] = 0
            idx1, idx2 = _draw_ids(rng, B, T, K, F)
            tgt = rng.standard_normal((B, Dx)).astype(np.float32)
            W = (rng.standard_normal(3 * Dx) / np.sqrt(2.0 * Dx)).astype(np.float32)
            gs = GRAD_SCALE.get(name, 1.0)
            g1 = (rng.standard_normal((n, Dx)) * gs).astype(np.float32)
            g2 = (rng.standard_normal((n, Dx)) * gs).astype(np.float32)
            ginfo = (rng.standard_normal((n, 2 * K)) * 0.25 * gs).astype(np.float32)
            z0 = forward_ref(Inputs(B, T, table, idx1, idx2, tgt, W, np.zeros(1, np.float32), g1, g2, ginfo, None, ld1, ldi), K, F, 0).z
            # the bias puts the kink into the widest gap between neighbouring scores of the middle fifth: about half of all
            # (unit, k) active (one unit, K = 1: an active one)
            zs = np.sort(z0.reshape(-1))
            lo, hi = max(0, int(zs.size * 0.4) - 1), min(zs.size - 1, int(zs.size * 0.6) + 1)
            m = lo + int(np.argmax(np.diff(zs[lo:hi + 1]))) if hi > lo else 0
            bias = np.asarray([-(zs[m] + zs[m + 1]) / 2 if zs.size > 1 else 0.5 - zs[0]], dtype=np.float32)
            inp = Inputs(B, T, table, idx1, idx2, tgt, W, bias, g1, g2, ginfo, None, ld1, ldi)
            ref = forward_ref(inp, K, F, 0)
            if np.abs(ref.z).min() >= MARGIN:
                break
        else:
            raise AssertionError("%s/%s: no draw keeps every score %g away from the kink" % (name, count, MARGIN))
        rsave = ref.r.astype(np.float32)                   # what the backward is fed: the reference's relu decisions
        if r.planted:
            rsave = planted_rsave(rng, n, K)
        out = inp._replace(rsave=rsave)
    for v in out:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def planted_rsave(rng, n, K):
    """saved scores planted per unit, five kinds in turn: every r = 0 (den = K, no dz, every pass-2/3 load goes to row 0);
    every r > 0; all equal and positive; one r = 90 among about 1 (the other exp terms underflow); a random relu'd mix"""
    rs = np.zeros((n, K), dtype=np.float32)
    for u in range(n):
        kind = u % 5
        if kind == 1:
            rs[u] = rng.uniform(0.1, 2.0, K)
        elif kind == 2:
            rs[u] = 0.75
        elif kind == 3:
            rs[u] = rng.uniform(0.9, 1.1, K)
            rs[u, u % K] = 90.0
        elif kind == 4:
            rs[u] = np.maximum(rng.standard_normal(K), 0)
    return rs


# ------------------------------------------------------------------------------------------------ float64 references
FwdRef = collections.namedtuple("FwdRef", "out1 out2 info z r p den s1 s2")
BwdRef = collections.namedtuple("BwdRef", "gtable dW dzsum named dz")


def _seqs(inp, K, F, dtype=np.float64):
    n = inp.B * inp.T
    t = inp.table.astype(dtype)
    s1 = t[_clamp(inp.idx1)].reshape(n, K, -1)            # [n, K, F * D]: feature f of neighbour k at columns [f D, (f + 1) D)
    s2 = t[_clamp(inp.idx2)].reshape(n, K, -1)
    return s1, s2


def forward_ref(inp, K, F, mode):
    """the collapsed co-attention (oracle/score_oracle.py _co_attention_collapsed) from the ids and the table, in float64"""
    s1, s2 = _seqs(inp, K, F)
    if mode == 1:
        return FwdRef(s1.sum(1), s2.sum(1), None, None, None, None, None, s1, s2)
    Dx = s1.shape[2]
    W = inp.W.astype(np.float64)
    wt, w1, w2 = W[:Dx], W[Dx:2 * Dx], W[2 * Dx:]
    c = inp.tgt.astype(np.float64) @ wt + np.float64(inp.bias[0])          # [B]
    z = s1 @ w1 + s2 @ w2 + np.repeat(c, inp.T)[:, None]
    r = np.maximum(z, 0)
    e = np.exp(r - r.max(1, keepdims=True))
    den = e.sum(1, keepdims=True)
    p = e / den
    out1 = (p[:, :, None] * s1).sum(1)
    out2 = s2.sum(1) / K
    info = np.concatenate([K * r, np.repeat(r.sum(1, keepdims=True), K, 1)], 1)
    return FwdRef(out1, out2, info, z, r, p, den, s1, s2)


def backward_ref(inp, K, F, mode, rsave=None):
    """the formulas above atomic_add4 in csrc/embed.hip, in float64, from the ids, the table and the rsave the kernel is given:
         dr_i = K ga_i + sum_j ga_{K+j} + p_i (dp_i - sum_k p_k dp_k),  dp_i = g1 . seq1_i,  p = softmax(rsave)
         dz_i = dr_i [r_i > 0];  dseq1_i = p_i g1 + dz_i w1;  dseq2_i = g2 / K + dz_i w2
         dw1 = sum_i dz_i seq1_i;  dw2 = sum_i dz_i seq2_i;  dzsum = sum_i dz_i
    Row 0, and an id outside the table (read as row 0), get no gradient.  mode 1: dseq1_i = g1, dseq2_i = g2."""
    n, D = inp.B * inp.T, inp.table.shape[1]
    s1, s2 = _seqs(inp, K, F)
    Dx = s1.shape[2]
    g1, g2 = inp.g1.astype(np.float64), inp.g2.astype(np.float64)
    if mode == 1:
        d1 = np.repeat(g1[:, None, :], K, 1)
        d2 = np.repeat(g2[:, None, :], K, 1)
        dW = dzsum = dz = None
    else:
        rs = (inp.rsave if rsave is None else rsave).astype(np.float64)
        W = inp.W.astype(np.float64)
        w1, w2 = W[Dx:2 * Dx], W[2 * Dx:]
        ga = inp.ginfo.astype(np.float64)
        e = np.exp(rs - np.maximum(rs.max(1, keepdims=True), 0))
        p = e / e.sum(1, keepdims=True)
        dp = np.einsum("nkd,nd->nk", s1, g1)
        dr = K * ga[:, :K] + ga[:, K:].sum(1, keepdims=True) + p * (dp - (p * dp).sum(1, keepdims=True))
        dz = dr * (rs > 0)
        d1 = p[:, :, None] * g1[:, None, :] + dz[:, :, None] * w1
        d2 = g2[:, None, :] / K + dz[:, :, None] * w2
        dW = np.zeros(3 * Dx)
        dW[Dx:2 * Dx] = np.einsum("nk,nkd->d", dz, s1)
        dW[2 * Dx:] = np.einsum("nk,nkd->d", dz, s2)
        dzsum = dz.sum(1)
    gtable = np.zeros((N_ROWS, D))
    i1, i2 = _clamp(inp.idx1).reshape(-1), _clamp(inp.idx2).reshape(-1)
    np.add.at(gtable, i1, d1.reshape(-1, D))
    np.add.at(gtable, i2, d2.reshape(-1, D))
    gtable[0] = 0
    named = np.zeros(N_ROWS, dtype=bool)
    named[i1] = True
    named[i2] = True
    named[0] = False
    return BwdRef(gtable, dW, dzsum, named, dz)


def autograd_ref(inp, K, F):
    """float64 torch autograd of the oracle's _co_attention_collapsed on the same inputs (each unit a sample of its own, so the
    gradient of its target row is dzsum[u] w_t): (table gradient with row 0 zeroed, dW, d target per unit)"""
    import torch
    from oracle import score_oracle as so
    n = inp.B * inp.T
    t = torch.tensor(inp.table.astype(np.float64), requires_grad=True)
    W = torch.tensor(inp.W.astype(np.float64).reshape(-1, 1), requires_grad=True)
    b = torch.tensor(inp.bias.astype(np.float64))
    s1 = t[torch.as_tensor(_clamp(inp.idx1)).long()].reshape(n, 1, K, -1)
    s2 = t[torch.as_tensor(_clamp(inp.idx2)).long()].reshape(n, 1, K, -1)
    tg = torch.tensor(np.repeat(inp.tgt.astype(np.float64), inp.T, 0), requires_grad=True)
    o1, o2, info = so._co_attention_collapsed(s1, s2, tg, W, b)
    g = lambda a: torch.tensor(a.astype(np.float64)).reshape(n, 1, -1)
    ((o1 * g(inp.g1)).sum() + (o2 * g(inp.g2)).sum() + (info * g(inp.ginfo)).sum()).backward()
    gt = t.grad.numpy().copy()
    gt[0] = 0
    return gt, W.grad.numpy().reshape(-1), tg.grad.numpy()


# ------------------------------------------------------------------------------------------------ float32 restatement
def _tree(x):
    """sum over the last axis (a power of two long) by halving, as a butterfly over the lanes of a group does"""
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


def _lane_dots(s, w, GS, SPL):
    """per lane: sum over its slots j (in order) of dot4(row slot, weight slot), float32; s [..., Dx], w [Dx] or [..., Dx]"""
    f32 = np.float32
    Dx = s.shape[-1]
    pad = GS * SPL * 4 - Dx
    prod = (s * w).astype(f32)
    prod = np.concatenate([prod, np.zeros(prod.shape[:-1] + (pad,), f32)], -1).reshape(prod.shape[:-1] + (SPL, GS, 4))
    d4 = ((prod[..., 0] + prod[..., 1]) + prod[..., 2]) + prod[..., 3]                # [..., SPL, GS]
    acc = np.zeros(d4.shape[:-2] + (GS,), f32)
    for j in range(SPL):
        acc = acc + d4[..., j, :]
    return acc


def restate_f32(inp, K, F, D):
    """forward and backward in float32 in the kernels' order where a lane fixes it: a lane's slots in order, k in order, a tree
    over the lanes of a group; dW as the kernel sums it (a unit over k, the groups of a workgroup in order, then the workgroups' slabs one after
    another); the table gradient's occurrences in unit order, which is one of the orders the atomics can land in.  Returns (out1, out2, info, r, gtable, dW, dzsum)."""
    f32 = np.float32
    GS, SPL, _ = geom(D, F)
    s1, s2 = _seqs(inp, K, F, f32)
    n, _, Dx = s1.shape
    wt, w1, w2 = inp.W[:Dx], inp.W[Dx:2 * Dx], inp.W[2 * Dx:]
    part = _lane_dots(s1, w1, GS, SPL) + _lane_dots(s2, w2, GS, SPL)                  # [n, K, GS]
    cpart = _lane_dots(np.repeat(inp.tgt, inp.T, 0), wt, GS, SPL)                     # [n, GS]
    c = _tree(cpart) + inp.bias[0]
    r = np.maximum(_tree(part) + c[:, None], f32(0))
    e = np.exp(r - r.max(1, keepdims=True), dtype=f32)
    den = np.zeros(n, f32)
    rsum = np.zeros(n, f32)
    for k in range(K):
        den = den + e[:, k]
        rsum = rsum + r[:, k]
    inv = f32(1) / den
    out1 = np.zeros((n, Dx), f32)
    sum2 = np.zeros((n, Dx), f32)
    for k in range(K):
        out1 = out1 + (e[:, k] * inv)[:, None] * s1[:, k]
        sum2 = sum2 + s2[:, k]
    out2 = sum2 / f32(K)
    info = np.concatenate([f32(K) * r, np.repeat(rsum[:, None], K, 1)], 1)
    # backward, from inp.rsave
    rs = inp.rsave
    g1, g2, ga = inp.g1, inp.g2, inp.ginfo
    eb = np.exp(rs - np.maximum(rs.max(1, keepdims=True), f32(0)), dtype=f32)
    denb = np.zeros(n, f32)
    gsum = np.zeros(n, f32)
    for k in range(K):
        denb = denb + eb[:, k]
        gsum = gsum + ga[:, K + k]
    p = eb * (f32(1) / denb)[:, None]
    dp = _tree(_lane_dots(s1, g1[:, None, :], GS, SPL))
    pdp = np.zeros(n, f32)
    for k in range(K):
        pdp = pdp + p[:, k] * dp[:, k]
    dr = (f32(K) * ga[:, :K] + gsum[:, None]) + p * (dp - pdp[:, None])
    dz = np.where(rs > 0, dr, f32(0)).astype(f32)
    dzsum = np.zeros(n, f32)
    for k in range(K):
        dzsum = dzsum + dz[:, k]
    d1 = (dz[:, :, None] * w1 + p[:, :, None] * g1[:, None, :]).astype(f32)
    d2 = (dz[:, :, None] * w2 + (g2 * (f32(1) / f32(K)))[:, None, :]).astype(f32)
    # dW: a group's own unit over k, the 4 * upw groups of a workgroup one after another, then the workgroups' slabs
    per = 4 * (64 // GS)
    nb = (n + per - 1) // per
    du = np.zeros((nb * per, 2 * Dx), f32)
    for k in range(K):
        du[:n, :Dx] = du[:n, :Dx] + dz[:, k, None] * s1[:, k]
        du[:n, Dx:] = du[:n, Dx:] + dz[:, k, None] * s2[:, k]
    du = du.reshape(nb, per, 2 * Dx)
    slab = np.zeros((nb, 2 * Dx), f32)
    for q in range(per):
        slab = slab + du[:, q]
    dW = np.zeros(3 * Dx, f32)
    for q in range(nb):
        dW[Dx:] = dW[Dx:] + slab[q]
    gtable = np.zeros((N_ROWS, D), f32)
    np.add.at(gtable, _clamp(inp.idx1).reshape(-1), d1.reshape(-1, D))
    np.add.at(gtable, _clamp(inp.idx2).reshape(-1), d2.reshape(-1, D))
    gtable[0] = 0
    return out1, out2, info, r, gtable, dW, dzsum


# ------------------------------------------------------------------------------------------------ the judge
GotFwd = collections.namedtuple("GotFwd", "out1 out2 info rsave")      # as the kernel leaves them: [n + 1, ld] with padding, canary-filled before
GotBwd = collections.namedtuple("GotBwd", "gtable dW dzsum")           # gtable: canary in row 0 and in every row no id names, 0 elsewhere,
                                                                       # before the launch; dW: canary in [0, Dx), 0 behind; dzsum [n + 1]


class Rejected(AssertionError):
    pass


def _need(cond, what):
    if not cond:
        raise Rejected(what)


def _is_canary(a):
    return bool((np.asarray(a, np.float32).view(np.uint32) == CANARY.view(np.uint32)).all())


def _share(got, want):            # the forward's: max |d| as a share of 1e-5 of the largest reference magnitude
    return float(np.abs(got.astype(np.float64) - want).max() / (FWD_BOUND * max(np.abs(want).max(), 1e-30)))


def _share_b(got, want):          # the backward's: max of |d| / (atol + rtol |want|)
    return float((np.abs(got.astype(np.float64) - want) / (ATOL + RTOL * np.abs(want))).max())


def fwd_buffers(inp, K, Dx):
    n = inp.B * inp.T
    c = lambda *s: np.full(s, CANARY, np.float32)
    return GotFwd(c(n + 1, inp.ld1), c(n + 1, inp.ld1), c(n + 1, inp.ldi), c(n + 1, K))


def bwd_buffers(inp, ref, Dx):
    n = inp.B * inp.T
    gt = np.zeros(inp.table.shape, np.float32)
    gt[~ref.named] = CANARY
    dW = np.zeros(3 * Dx, np.float32)
    dW[:Dx] = CANARY
    return GotBwd(gt, dW, np.full(n + 1, CANARY, np.float32))


def judge_fwd(inp, K, Dx, mode, got, ref):
    """raises Rejected, or returns every output's error as a share of its bound (mode 1: exact, {})"""
    n = inp.B * inp.T
    _need(_is_canary(got.out1[:, Dx:]) and _is_canary(got.out2[:, Dx:]) and _is_canary(got.out1[n:]) and _is_canary(got.out2[n:]),
          "padding or the row behind the last unit of out1 / out2 written")
    o1, o2 = got.out1[:n, :Dx], got.out2[:n, :Dx]
    if mode == 1:
        _need(_is_canary(got.info) and _is_canary(got.rsave), "mode 1 wrote info / rsave")
        _need(np.array_equal(o1.astype(np.int64), np.rint(ref.out1).astype(np.int64)) and np.array_equal(o1, np.rint(o1)), "out1 != the int64 sum")
        _need(np.array_equal(o2.astype(np.int64), np.rint(ref.out2).astype(np.int64)) and np.array_equal(o2, np.rint(o2)), "out2 != the int64 sum")
        return {}
    _need(_is_canary(got.info[:, 2 * K:]) and _is_canary(got.info[n:]) and _is_canary(got.rsave[n:]), "padding of info / rsave written")
    rs, info = got.rsave[:n], got.info[:n, :2 * K]
    _need(np.array_equal(rs > 0, ref.r > 0), "relu pattern of rsave")
    _need(np.array_equal(info[:, :K].view(np.uint32), (np.float32(K) * rs).view(np.uint32)), "info[:, :K] != K * rsave bit for bit")
    e = {"out1": _share(o1, ref.out1), "out2": _share(o2, ref.out2), "info": _share(info, ref.info), "rsave": _share(rs, ref.r)}
    _need(max(e.values()) <= 1.0, "forward outside 1e-5 of the largest magnitude: %r" % (e,))
    return e


def judge_bwd(inp, Dx, mode, got, ref):
    """raises Rejected, or returns every output's error as a share of its bound (mode 1: exact, {})"""
    n = inp.B * inp.T
    _need(_is_canary(got.gtable[~ref.named]), "row 0 or a row no id names written in the gradient table")
    gt = got.gtable[ref.named]
    if mode == 1:
        _need(_is_canary(got.dzsum), "mode 1 wrote dzsum")
        _need(np.array_equal(gt.astype(np.int64), np.rint(ref.gtable[ref.named]).astype(np.int64)) and np.array_equal(gt, np.rint(gt)),
              "table gradient != the int64 sums")
        return {}
    _need(_is_canary(got.dW[:Dx]) and _is_canary(got.dzsum[n:]), "dW[0, Dx) or dzsum behind the last unit written")
    e = {"gtable": _share_b(gt, ref.gtable[ref.named]), "dW": _share_b(got.dW[Dx:], ref.dW[Dx:]), "dzsum": _share_b(got.dzsum[:n], ref.dzsum)}
    _need(max(e.values()) <= 1.0, "backward outside rtol 2e-4, atol 2e-5: %r" % (e,))
    return e
