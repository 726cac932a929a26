"""The rows of tests/test_gpu_scatter_edges.py and their CPU twin (tests/test_scatter_cases_cpu.py): the embedding-gradient path
below the model -- the row-sum scatter ("sort once, pull per row": pull_kernel, pull_fixup_kernel behind score_segment_sum_rows),
the owner-side combine (score_rows_accumulate / _multi), score_index_plan's de-duplication products and score_auc_logloss
(all csrc/scatter.hip) -- each with a plain numpy restatement and the judge both tests share.  Pure numpy: no GPU, no library.

1. The scatter.  `structure` restates what the two launches make of a sorted key list: the window size, every run's chain (a run
   that starts in window w and continues through w+1 .. w+L), its class (closed L = 0, short 1 <= L <= LONG_CHAIN, long beyond),
   the workgroup that opens it, a long chain's split over the workgroup's groups (chunk = ceil(L / gpb), full eight-window trips
   and tail per group) and the distance the run-end search has to cover (re - end).  SCATTER_ROWS are built from explicit run
   lists (row id, start offset inside its window, length) so that each seam is hit exactly; every row CLAIMS what it is there to
   reach and both tests assert the claim before any number.  Two fills per row:
     exact     integers in [-4, 4] as float32: every partial sum stays below 2^24, every association gives the same bits, the
               result must be the int64 sum bit for bit -- a dropped, doubled or misdirected window fails for certain;
     rounding  Gaussians scaled by 2^e, e uniform in [-10, 10] per slot: |got - want64| <= gamma(m - 1) * sum|src| per element,
               m the run's length, gamma(k) = k u / (1 - k u), u = 2^-24 -- the bound of a float32 sum in ANY order (additions of
               an exact zero, which the kernels make, add no error).  want64 is a float64 sum: its own error, at most
               (m - 1) 2^-53 sum|src|, is below gamma(m - 1) - ((1 + u)^(m - 1) - 1) >= (m - 1) m u^2 / 2, the bound's slack.
2. score_rows_accumulate(_multi): a float32 numpy loop in source order, bit for bit (the ops promise the association).
3. score_index_plan: owner = id % G, local = id // G, key order (owner, local), unique position 0 is row 0, an id outside [0, N)
   is row 0 and sets its tensor's bit.
4. score_auc_logloss: mid-rank AUC in exact rational arithmetic, log-loss in float64 with the documented clip at 2^-52."""
import math
import zlib
from collections import namedtuple
from fractions import Fraction

import numpy as np

E_BADARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
LONG_CHAIN = 16
U = 2.0 ** -24
WINDOWS = (8, 16, 32, 64)


def _seed(name, salt=0):
    return zlib.crc32(name.encode()) + salt


# ---------------------------------------------------------------------------------------------- 1. the scatter: restatement
def window(n):
    """occurrences per window (score_pull_window)"""
    return 64 if n >= 1 << 20 else 32 if n >= 1 << 19 else 16 if n >= 1 << 18 else 8


def lanes(D):
    """lanes of a group, four floats each: the power of two at or above D / 4"""
    lpr = 1
    while lpr < D // 4:
        lpr <<= 1
    return lpr


def geometry(n, D):
    """(window, lanes per row, groups per workgroup, LONG_CHAIN) of a launch, None where the launcher refuses the width"""
    lpr = lanes(D)
    return None if lpr > 64 else (window(n), lpr, 256 // lpr, LONG_CHAIN)


CLOSED, SHORT, LONG = 0, 1, 2
Structure = namedtuple("Structure", "n window lanes gpb heads ends ids L cls wg gallop longs max_L n_long max_per_wg chunks "
                                    "full_trip partial_end")
LongChain = namedtuple("LongChain", "run w0 L chunk counts trips tails")


def structure(keys, D):
    """what pull_kernel + pull_fixup_kernel make of the ascending key list `keys` at row width D"""
    keys = np.asarray(keys)
    n = len(keys)
    ws, lpr, gpb, _ = geometry(n, D)
    heads = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    ends = np.concatenate([heads[1:], [n]])                     # run i is [heads[i], ends[i])
    w0, wl = heads // ws, (ends - 1) // ws
    L = wl - w0                                                 # windows w0+1 .. w0+L continue the run
    cls = np.where(L == 0, CLOSED, np.where(L <= LONG_CHAIN, SHORT, LONG))
    wg = w0 // gpb                                              # the workgroup whose group opens the chain
    gallop = np.where(L > 0, ends - np.minimum((w0 + 1) * ws, n), 0)      # re - end: keys the run-end search has to pass
    longs = []
    for i in np.flatnonzero(cls == LONG):
        chunk = -(-int(L[i]) // gpb)
        g = np.arange(gpb)
        j0, j1 = 1 + g * chunk, np.minimum(int(L[i]), (g + 1) * chunk)
        counts = np.maximum(j1 - j0 + 1, 0)                     # windows group g sums; 0: an idle group
        longs.append(LongChain(int(i), int(w0[i]), int(L[i]), chunk, counts, counts // 8, counts % 8))
    per_wg = np.bincount(wg[cls == LONG]) if longs else np.zeros(1, int)
    partial_end = bool(n % ws and np.any((L > 0) & (wl == (n - 1) // ws)))
    return Structure(n, ws, lpr, gpb, heads, ends, keys[heads], L, cls, wg, gallop, longs, int(L.max()), len(longs),
                     int(per_wg.max()), tuple(sorted({c.chunk for c in longs})), any(c.trips.any() for c in longs), partial_end)


# ---------------------------------------------------------------------------------------------- 1. the scatter: rows
# claim: window; max_L over all runs; n_long long chains; max_per_wg long chains opened by one workgroup; chunks of the long
# chains (ascending, distinct); full_trip: some group makes a full eight-window trip; partial_end: a chain ends in the list's
# partial last window; gallop: set of (re - end) over the open runs.  None = not claimed by this row.
Claim = namedtuple("Claim", "window max_L n_long max_per_wg chunks full_trip partial_end gallop")
# runs: (row id, start offset inside its window, length), ascending ids; the slots in front of a run that its offset asks for
# are one-slot runs of the ids just above the previous run's; `tail` more one-slot runs close the list.  big: (n,) -- many
# two-slot runs, one long chain of L = 300 (see _big_keys).  n_out: rows of `out` (None: highest id + 1).
ScatterRow = namedtuple("ScatterRow", "name D runs tail n_out big claim why")
SCATTER_ROWS = {}


def _srow(name, D, runs, claim, tail=3, n_out=None, big=None, why=""):
    assert name not in SCATTER_ROWS, name
    SCATTER_ROWS[name] = ScatterRow(name, D, tuple(runs), tail, n_out, big, claim, why)


def _claim(window=8, max_L=0, n_long=0, max_per_wg=None, chunks=None, full_trip=None, partial_end=None, gallop=None):
    if max_per_wg is None:
        max_per_wg = min(n_long, 1) if n_long <= 1 else None
    if chunks is None and n_long == 0:
        chunks = ()
    if full_trip is None and n_long == 0:
        full_trip = False
    return Claim(window, max_L, n_long, max_per_wg, chunks, full_trip, partial_end, gallop)


def _len(off, L, last_slot, ws=8):
    """length of a run that starts at `off` of its window, continues through L more and ends on a window's last slot or on
    slot 3 of its last window"""
    if L == 0:
        return ws - off if last_slot else max(1, (ws - off) // 2)
    return (ws - off) + ws * (L - 1) + (ws if last_slot else 4)


def _gpb(D):
    return 256 // lanes(D)


def _cdiv(a, b):
    return -(-a // b)


# widths: every lane-group size, a closed run, a short chain and a long chain each (D = 12, 20: lane groups that are not full)
for _D in (4, 8, 12, 16, 20, 64, 128, 256):
    _srow("width_d%d" % _D, _D, [(10, 2, 5), (40, 3, _len(3, 2, False)), (80, 0, _len(0, 17, True)), (120, 7, 1)],
          _claim(max_L=17, n_long=1, chunks=(_cdiv(17, _gpb(_D)),), full_trip=_cdiv(17, _gpb(_D)) >= 8),
          why="lane group of %d, %d used" % (lanes(_D), _D // 4))

# chain length on both sides of LONG_CHAIN at window 8: start offsets 0, 3, 7, ending on a window's last slot and mid-window
for _L in (0, 1, 2, 15, 16, 17):
    for _off in (0, 3, 7):
        for _last in ((True,) if _L == 0 else (True, False)):
            _srow("chain_L%d_o%d_%s" % (_L, _off, "last" if _last else "mid"), 16, [(30, _off, _len(_off, _L, _last))],
                  _claim(max_L=_L, n_long=int(_L > 16), chunks=(1,) if _L > 16 else None, full_trip=False),
                  why="L = %d from offset %d" % (_L, _off))

# the run-end search: gallop 1, 2, 4, 8, 16 then bisect; the run passes its opening window's end by g keys
for _g in (1, 2, 3, 4, 7, 8, 9, 15, 16, 17):
    _srow("gallop_%d" % _g, 16, [(20, 5, 3 + _g)], _claim(max_L=_cdiv(_g, 8), gallop={_g}), why="re - end = %d" % _g)
for _g in (1, 3, 4, 11, 16):
    # the search's `lo + step < n` exit: the run is the list's last (re = n), or one key short of it
    _srow("gallop_%d_to_n" % _g, 16, [(20, 5, 3 + _g)], _claim(max_L=_cdiv(_g, 8), gallop={_g}, partial_end=bool((8 + _g) % 8)),
          tail=0, why="run reaches n")
    _srow("gallop_%d_to_n_minus_1" % _g, 16, [(20, 5, 3 + _g)], _claim(max_L=_cdiv(_g, 8), gallop={_g}), tail=1,
          why="run stops one short of n")

# the long-chain split over the workgroup's groups: chunk = ceil(L / gpb) across 8 and 16, idle groups, tails
for _D, _Ls in ((256, (17, 31, 32, 33, 63, 64, 65)), (64, (17, 127, 128, 129)), (16, (65, 511, 512, 513)), (4, (17, 300))):
    for _i, _L in enumerate(_Ls):
        _c = _cdiv(_L, _gpb(_D))
        _srow("split_d%d_L%d" % (_D, _L), _D, [(9, 3, _len(3, _L, bool(_i & 1)))],
              _claim(max_L=_L, n_long=1, chunks=(_c,), full_trip=_c >= 8), why="gpb %d, chunk %d" % (_gpb(_D), _c))

# a long chain whose last window is the list's partial last window (n = 2 + 6 + 8 * 19 + 3 = 163)
_srow("long_into_partial_window", 16, [(50, 2, 6 + 8 * 19 + 3)], _claim(max_L=20, n_long=1, chunks=(1,), full_trip=False,
                                                                       partial_end=True), tail=0)
# several long chains opened by ONE workgroup (s_long).  A long chain covers more than 17 windows and a workgroup owns gpb
# consecutive ones, so this needs gpb >= 35 for two and gpb = 64 (D <= 16) for four: at D = 256 (gpb 4) a workgroup can open one.
_srow("four_long_one_workgroup_d16", 16, [(10 + 10 * _i, 2 if _i == 0 else 6, 8 * 17) for _i in range(4)],
      _claim(max_L=17, n_long=4, max_per_wg=4, chunks=(1,), full_trip=False), why="windows 0, 17, 34, 51 of workgroup 0")
_srow("nine_long_one_workgroup_d4", 4, [(10 + 10 * _i, 2 if _i == 0 else 6, 8 * 24) for _i in range(9)],
      _claim(max_L=24, n_long=9, max_per_wg=9, chunks=(1,), full_trip=False), why="gpb 256: windows 0, 24, ..., 192")
# two long chains in neighbouring workgroups (D = 16: windows 60 and 77)
_srow("long_chains_neighbouring_workgroups", 16, [(_i + 1, 0, 8) for _i in range(60)] + [(100, 4, 8 * 17), (110, 4, 8 * 17)],
      _claim(max_L=17, n_long=2, max_per_wg=1, chunks=(1,), full_trip=False))
# the one place a workgroup of four groups can be made to hold a long chain in EVERY window it owns does not exist; what does:
# every group of a workgroup busy with the same long chain while the next workgroup opens its own (D = 256: chains from
# windows 3 and 24, workgroups 0 and 6)
_srow("long_chains_d256_back_to_back", 256, [(5, 0, 8), (6, 0, 8), (7, 0, 8), (20, 1, 7 + 8 * 20 + 4), (30, 5, 3 + 8 * 33)],
      _claim(max_L=33, n_long=2, max_per_wg=1, chunks=(6, 9), full_trip=True))

# row 0: the owner-side sum has zero_is_dummy = 0 -- local row 0 is a real row on shards > 0
_srow("row0_one_slot", 16, [(0, 0, 1), (9, 3, 14)], _claim(max_L=2))
_srow("row0_short_chain", 16, [(0, 0, 20), (9, 7, 2)], _claim(max_L=2))
_srow("row0_long_chain", 16, [(0, 0, 8 * 18 + 3)], _claim(max_L=18, n_long=1, chunks=(1,), full_trip=False))
_srow("row0_long_chain_d12", 12, [(0, 0, 8 * 70 + 3)], _claim(max_L=70, n_long=1, chunks=(2,), full_trip=False))

# the row-id range: out rows 1, 2, 2^k, 2^k + 1 with the highest row present; rows never named keep value and flag
_srow("n_out_1", 16, [(0, 0, 21)], _claim(max_L=2), tail=0, n_out=1)
_srow("n_out_2", 16, [(0, 0, 5), (1, 5, 20)], _claim(max_L=3), tail=0, n_out=2)
_srow("n_out_1024", 16, [(511, 2, 9), (512, 3, 9), (1023, 4, 9)], _claim(max_L=1), tail=0, n_out=1024)
_srow("n_out_1025", 16, [(1023, 2, 9), (1024, 3, 9)], _claim(max_L=1), tail=0, n_out=1025)
_srow("n_out_1025_highest_unnamed", 20, [(3, 2, 9), (1000, 3, 9)], _claim(max_L=1), tail=0, n_out=1025)

# list length: below, at and above one window
_srow("n_1", 16, [(3, 0, 1)], _claim(), tail=0)
_srow("n_7", 16, [(2, 0, 3), (5, 3, 4)], _claim(), tail=0)
_srow("n_8", 16, [(1, 0, 5), (2, 5, 3)], _claim(), tail=0)
_srow("n_8_one_run", 8, [(4, 0, 8)], _claim(), tail=0)
_srow("n_9", 16, [(1, 0, 5), (2, 5, 4)], _claim(max_L=1, gallop={1}, partial_end=True), tail=0)
_srow("n_9_d4", 4, [(6, 0, 9)], _claim(max_L=1, gallop={1}, partial_end=True), tail=0)


# n on both sides of every window size at D = 4: many two-slot runs (odd offsets: every fourth / eighth / ... straddles a
# window edge) and one long chain of L = 300 (gpb 256: chunk 2, most groups idle)
def _big_long_len(n):
    ws = window(n)
    return (300 + 13 // ws) * ws - 7                                       # starts at slot 13, ends on slot 5 of its last window


def _big_keys(n):
    ll = _big_long_len(n)
    head = np.concatenate([[1], np.repeat(np.arange(2, 8), 2), np.full(ll, 8)])
    rest = n - len(head)
    return np.concatenate([head, np.repeat(np.arange(9, 9 + (rest + 1) // 2), 2)[:rest]]).astype(np.int32)


for _n in ((1 << 18) - 1, 1 << 18, (1 << 19) - 1, 1 << 19, (1 << 20) - 1, (1 << 20) + 5):
    _srow("straddle_n%d" % _n, 4, [], _claim(window=window(_n), max_L=300, n_long=1, chunks=(2,), full_trip=False), big=(_n,),
          why="window %d" % window(_n))


def sorted_keys(r):
    """the ascending key list a row describes"""
    if r.big:
        return _big_keys(r.big[0])
    ws = r.claim.window
    out, pos, prev = [], 0, -1
    for rid, off, length in r.runs:
        f = (off - pos) % ws
        assert prev + f < rid and length >= 1, (r.name, rid)
        out.append(np.arange(prev + 1, prev + 1 + f))
        out.append(np.full(length, rid))
        pos += f + length
        prev = rid
    out.append(np.arange(prev + 1, prev + 1 + r.tail))
    return np.concatenate(out).astype(np.int32)


_INPUTS = {}
ScatterInputs = namedtuple("ScatterInputs", "rows n_out out0 flags0 order keys")


def scatter_inputs(r):
    """the row's `rows` array (its sorted keys in a fixed shuffle: the sort is part of the op), out's rows, the contents of `out`
    and `row_flags` before the call, and the stable sort restated"""
    if r.name not in _INPUTS:
        keys = sorted_keys(r)
        rows = keys[np.random.default_rng(_seed(r.name)).permutation(len(keys))]
        n_out = r.n_out or int(keys.max()) + 1
        out0 = (np.arange(n_out * r.D) % 251 + 1000).astype(np.float32).reshape(n_out, r.D)
        flags0 = (np.arange(n_out) % 3 == 0).astype(np.uint8)
        order = np.argsort(rows, kind="stable")
        if r.big:                                                # (the large rows: one of them held at a time)
            for k in [k for k in _INPUTS if SCATTER_ROWS[k].big]:
                del _INPUTS[k]
        _INPUTS[r.name] = ScatterInputs(rows, n_out, out0, flags0, order, rows[order])
    return _INPUTS[r.name]


def scatter_fill(r, kind):
    n = len(scatter_inputs(r).rows)
    rng = np.random.default_rng(_seed(r.name, 1 if kind == "exact" else 2))
    if kind == "exact":
        return rng.integers(-4, 5, (n, r.D)).astype(np.float32)
    return (rng.standard_normal((n, r.D)) * 2.0 ** rng.integers(-10, 11, (n, 1))).astype(np.float32)


def check_claim(r, st):
    """the row reaches what it names"""
    c = r.claim
    got = Claim(st.window, st.max_L, st.n_long, st.max_per_wg, st.chunks, st.full_trip, st.partial_end,
                set(int(g) for g in st.gallop[st.L > 0]))
    for f in Claim._fields:
        want = getattr(c, f)
        if want is None:
            continue
        have = getattr(got, f)
        assert (want <= have if f == "gallop" else want == have), (r.name, f, want, have)
    assert st.window == window(st.n)


# ---------------------------------------------------------------------------------------------- 1. the scatter: reference and judge
Worst = namedtuple("Worst", "all runs_of_3_up")


def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1.0 - k * U)


def scatter_reference(inp, src, exact):
    """per run of the stably sorted list: (row ids, run lengths, sums [runs, D] -- int64 for the exact fill, float64 else --,
    sums of |src| in float64)"""
    heads = np.flatnonzero(np.concatenate([[True], inp.keys[1:] != inp.keys[:-1]]))
    s = src[inp.order]
    m = np.diff(np.concatenate([heads, [len(inp.keys)]]))
    if exact:
        return inp.keys[heads], m, np.add.reduceat(s.astype(np.int64), heads, axis=0), None
    s = s.astype(np.float64)
    return inp.keys[heads], m, np.add.reduceat(s, heads, axis=0), np.add.reduceat(np.abs(s), heads, axis=0)


def scatter_judge(r, kind, src, got, got_flags):
    """got: `out` after the call; got_flags: row_flags after it, or None where the call had none.  Returns the worst
    error / bound of the rounding fill over all runs and over the runs of three slots and more (a run of two has one addition and
    one order: its bound, u |a + b| against u (|a| + |b|), is met to the last digit by any correct sum); zeros for the exact
    fill.  Raises AssertionError on any miss."""
    inp = scatter_inputs(r)
    ids, m, want, sabs = scatter_reference(inp, src, kind == "exact")
    named = np.zeros(inp.n_out, bool)
    named[ids] = True
    assert got.shape == inp.out0.shape and got.dtype == np.float32
    assert np.array_equal(got[~named].view(np.uint32), inp.out0[~named].view(np.uint32)), (r.name, "a row never named was written")
    if got_flags is not None:
        assert np.array_equal(got_flags, np.where(named, 2, inp.flags0).astype(np.uint8)), (r.name, "row flags")
    g = got[ids]
    if kind == "exact":
        assert np.abs(want).max() < 1 << 24
        bad = g.view(np.uint32) != want.astype(np.float32).view(np.uint32)
        assert not bad.any(), (r.name, "exact fill: rows", ids[bad.any(axis=1)][:8].tolist())
        return Worst(0.0, 0.0)
    assert np.isfinite(g).all(), r.name
    err = np.abs(g.astype(np.float64) - want)
    bound = gamma(m - 1)[:, None] * sabs
    assert (err <= bound).all(), (r.name, "rounding fill", float((err / np.maximum(bound, 1e-300)).max()))
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    return Worst(float(ratio.max()), float(ratio[m >= 3].max()) if (m >= 3).any() else 0.0)


def plain_float32_sums(r, src):
    """`out` as a plain float32 left-to-right sum in slot order leaves it (the reference alone, inside its own bound)"""
    inp = scatter_inputs(r)
    heads = np.flatnonzero(np.concatenate([[True], inp.keys[1:] != inp.keys[:-1]]))
    ends = np.concatenate([heads[1:], [len(inp.keys)]])
    s = src[inp.order]
    out = inp.out0.copy()
    acc = s[heads].copy()
    m = ends - heads
    for k in range(1, 4):                                        # the short runs together
        sel = m > k
        acc[sel] = acc[sel] + s[heads[sel] + k]
    for i in np.flatnonzero(m > 4):                              # a long run on its own: cumsum adds left to right
        acc[i] = np.cumsum(s[heads[i]:ends[i]], axis=0, dtype=np.float32)[-1]
    out[inp.keys[heads]] = acc
    return out


PERTURBATIONS = ("pfirst_left_out", "pfirst_twice", "total_to_next_row", "last_slot_ignored", "row0_dropped", "last_group_left_out")


def simulate(r, src, perturb=None):
    """the two launches on the exact fill, window by window in int64: pull_kernel leaves a partial sum per (run, window),
    pull_fixup_kernel adds a chain's in window order.  perturb: one of PERTURBATIONS, applied to the first chain it fits."""
    inp = scatter_inputs(r)
    st = structure(inp.keys, r.D)
    s = src[inp.order].astype(np.int64)
    if perturb == "last_slot_ignored":
        s[-1] = 0
    out = inp.out0.copy()
    done = perturb is None or perturb == "last_slot_ignored"
    for i in range(len(st.heads)):
        h, e, L, rid = int(st.heads[i]), int(st.ends[i]), int(st.L[i]), int(st.ids[i])
        w0 = h // st.window
        parts = [s[max(h, w * st.window):min(e, (w + 1) * st.window)].sum(axis=0) for w in range(w0, w0 + L + 1)]
        hit = None
        if not done:
            if perturb == "pfirst_left_out" and L >= 2 and parts[1].any():
                hit = parts.pop(1)
            elif perturb == "pfirst_twice" and L >= 2 and parts[1].any():
                hit = parts[1]
                parts.append(hit)
            elif perturb == "last_group_left_out" and st.cls[i] == LONG:
                c = [c for c in st.longs if c.run == i][0]
                g = int(np.flatnonzero(c.counts)[-1])                        # the last group that has windows
                lo = 1 + g * c.chunk
                hit = sum(parts[lo:lo + int(c.counts[g])])
                parts = parts[:lo] + parts[lo + int(c.counts[g]):]
                hit = hit if np.any(hit) else None
            elif perturb == "row0_dropped" and rid == 0:
                done = True
                continue
            elif perturb == "total_to_next_row" and L >= 1 and rid + 1 < inp.n_out:
                hit = True
                rid += 1
            done = hit is not None
        out[rid] = sum(parts).astype(np.float32)
    assert done, (r.name, perturb, "nothing to perturb in this row")
    return out


# ---------------------------------------------------------------------------------------------- 2. score_rows_accumulate(_multi)
AccRow = namedtuple("AccRow", "name D n_out lists why")
ACC_ROWS = {}


def _arow(name, D, n_out, lists, why=""):
    lists = tuple(np.asarray(l, np.int32).reshape(-1) for l in lists)
    for l in lists:
        assert np.all(np.diff(l) > 0) and (not len(l) or (l[0] >= 0 and l[-1] < n_out)), name       # unique, ascending, in range
    ACC_ROWS[name] = AccRow(name, D, n_out, lists, why)


_arow("one_source_d4", 4, 12, [[0, 5, 11]], "n_sources 1: lowest and highest row of out")
_arow("one_source_one_element_d256", 256, 3, [[1]])
_arow("two_sources_one_element_each_d12", 12, 7, [[3], [3]], "lists of one element, the same row")
_arow("two_sources_disjoint_d20", 20, 9, [[0, 1, 2], [6, 7, 8]])
_arow("eight_sources_empty_first_middle_last_d20", 20, 40, [[], [1, 4, 9], [], [4, 9, 30], [0, 4, 39], [], [4], []],
      "row 4 named by every non-empty source")
_arow("eight_sources_all_empty_d4", 4, 5, [[]] * 8, "nothing to do: out and flags untouched")
# row 7 by every source; row 33 only by the last; row 2 by the first and the last; 0 / 63 the lowest / highest of their lists
_arow("eight_sources_named_rows_d12", 12, 64,
      [[2, 7, 20], [0, 7], [7, 63], [5, 6, 7, 8], [7], [1, 7, 62, 63], [0, 3, 7, 40, 41, 42, 63], [2, 7, 33]],
      "ends of acc_find: a hit on a list's first and on its last element, misses below and above")
_arow("eight_sources_d256", 256, 20, [[1, 3, 19], [0, 3], [3, 4, 5], [3], [2, 3, 18, 19], [3, 19], [0, 3, 19], [3, 10]])


def _many(name, D, n_out, n_sources, always, seed):
    rng = np.random.default_rng(seed)
    lists = []
    for p in range(n_sources):
        l = np.flatnonzero(rng.random(n_out) < 0.3)
        lists.append([] if p in (0, 31) else np.union1d(l, always))
    lists[-1] = np.union1d(lists[-1], [n_out - 1])
    _arow(name, D, n_out, lists, "64 sources, two of them empty, row %d in all the others" % always[0])


_many("sixty_four_sources_d4", 4, 300, 64, [17], 11)           # more than one workgroup
_many("sixty_four_sources_d20", 20, 70, 64, [0], 12)
_many("sixty_four_sources_d256", 256, 30, 64, [29], 13)


def acc_inputs(r):
    """src [n, D] for the lists back to back, `out` and the state bytes before the call: rows enter in state 0, 1 (stale contents,
    never read: NaN here) and 2 (added to)"""
    rng = np.random.default_rng(_seed(r.name))
    n = sum(len(l) for l in r.lists)
    src = rng.standard_normal((n, r.D)).astype(np.float32)
    flags0 = (np.arange(r.n_out) % 3).astype(np.uint8)
    out0 = rng.standard_normal((r.n_out, r.D)).astype(np.float32)
    out0[flags0 != 2] = np.nan
    return src, out0, flags0


def acc_reference(r, src, out0, flags0):
    """the float32 loop in source order: the first writer of a row stores, later ones add -- ((g_p0 + g_p1) + g_p2) ..."""
    out, flags, off = out0.copy(), flags0.copy(), 0
    for l in r.lists:
        g = src[off:off + len(l)]
        add = flags[l] == 2
        out[l[add]] = out[l[add]] + g[add]
        out[l[~add]] = g[~add]
        flags[l] = 2
        off += len(l)
    return out, flags


def acc_judge(r, want, want_flags, got, got_flags):
    assert np.array_equal(got_flags, want_flags), (r.name, "state bytes")
    bad = (got.view(np.uint32) != want.view(np.uint32)).any(axis=1)
    assert not bad.any(), (r.name, "rows", np.flatnonzero(bad)[:8].tolist())


# ---------------------------------------------------------------------------------------------- 3. score_index_plan
# ids: "random" in [0, N); "equal"; "distinct" (a permutation); "bad_all": every id outside the table; "mixed": random, with ids
# outside the table in user_2hop and target_user only -- and, where slices are masked, in the masked slices of user_1hop, which
# nobody may look at
PlanRow = namedtuple("PlanRow", "name G N B T K Fu Fi active ids why")
PLAN_ROWS = {}
PLAN_SORT_FLAGS = (0, 32, 256)                                   # debug_flags: by size, the library's sort, csrc/sort.hip
REMAP_SENTINEL = -77
FEED_OF_SEG = (0, 3, 1, 2, 4, 5)                                 # plan order -> position in the feed tuple (the id_status bit)


def _prow(name, G, N, B, T, K, Fu, Fi, active=0, ids="random", why=""):
    PLAN_ROWS[name] = PlanRow(name, G, N, B, T, K, Fu, Fi, active, ids, why)


_prow("g1_n64_b1", 1, 64, 1, 1, 1, 1, 1, why="one shard, dedup alone; B = T = K = 1")
_prow("g1_n1024_b3", 1, 1024, 3, 2, 2, 8, 1, why="N = 2^k: the highest id fills the key bits")
_prow("g1_n3001_masked_mixed", 1, 3001, 128, 3, 2, 1, 1, active=2, ids="mixed", why="256 * 9 + 1 occurrences with the sentinel")
_prow("g2_n1024_b3", 2, 1024, 3, 2, 2, 1, 8)
_prow("g2_n1025_active1", 2, 1025, 3, 3, 2, 8, 1, active=1, why="active_slices 1 of 3; N = 2^k + 1: 513 local rows, shift 10")
_prow("g3_n1025_masked_mixed", 3, 1025, 3, 2, 2, 8, 1, active=1, ids="mixed")
_prow("g3_n64_equal", 3, 64, 3, 2, 2, 8, 8, ids="equal")
_prow("g3_n3001_bad_all_masked", 3, 3001, 3, 3, 2, 1, 8, active=2, ids="bad_all", why="U = 1")
_prow("g8_n7_b1_distinct", 8, 7, 1, 1, 1, 1, 1, ids="distinct", why="N below n_shards: one local row a shard, shift 1")
_prow("g8_n7_b3", 8, 7, 3, 2, 2, 1, 1)
_prow("g8_n1024_bad_all", 8, 1024, 3, 2, 2, 1, 8, ids="bad_all")
_prow("g8_n1024_mixed", 8, 1024, 3, 2, 2, 8, 8, ids="mixed")
_prow("g64_n64_distinct", 64, 64, 3, 2, 2, 1, 1, ids="distinct", why="N = n_shards: every shard owns exactly row 0 of its own")
_prow("g64_n1024_b3", 64, 1024, 3, 2, 2, 8, 8, why="16 local rows: shift 4")
_prow("g64_n3001_b16", 64, 3001, 16, 2, 1, 8, 8, why="256 * 5 + 1 occurrences with the sentinel")
_prow("g64_n3001_equal", 64, 3001, 1, 1, 1, 8, 1, ids="equal")


def plan_shapes(c):
    return ((c.B, c.T, c.K, c.Fi), (c.B, c.T, c.K, c.Fu), (c.B, c.T, c.K, c.Fu), (c.B, c.T, c.K, c.Fi), (c.B, c.Fu), (c.B, c.Fi))


def plan_active(c):
    return c.active if 0 < c.active < c.T else c.T


def plan_occurrences(c):
    """occurrences the plan sorts, the sentinel of row 0 included"""
    return c.B * (2 * plan_active(c) * c.K * (c.Fu + c.Fi) + c.Fu + c.Fi) + 1


def plan_inputs(c):
    """the six id tensors in FEED order: user_1hop, user_2hop, item_1hop, item_2hop, target_user, target_item"""
    rng = np.random.default_rng(_seed(c.name))
    shapes = plan_shapes(c)
    total = sum(int(np.prod(s)) for s in shapes)
    outside = np.array([c.N, c.N + 5, -1, -c.N, 2 ** 31 - 1, -2 ** 31], np.int64)
    if c.ids == "equal":
        flat = np.full(total, c.N - 1)
    elif c.ids == "distinct":
        assert total <= c.N - 1
        flat = rng.permutation(np.arange(1, c.N))[:total]
    elif c.ids == "bad_all":
        flat = outside[rng.integers(0, len(outside), total)]
    else:
        flat = rng.integers(0, c.N, total)
    t, off = [], 0
    for s in shapes:
        k = int(np.prod(s))
        t.append(flat[off:off + k].reshape(s).astype(np.int32))
        off += k
    if c.ids == "mixed":
        for i in (1, 4):
            v = t[i].reshape(-1)
            v[::3] = outside[np.arange(len(v[::3])) % len(outside)].astype(np.int32)
        if plan_active(c) < c.T:
            t[0][:, plan_active(c):] = c.N + 1
    return t


PlanProducts = namedtuple("PlanProducts", "U offsets unique_rows remap id_status")


def plan_reference(c, t):
    """the de-duplication products restated: U, the owner offsets meta[1 .. G + 1], unique_rows, the six remapped tensors in
    PLAN order (user_1hop, item_2hop, user_2hop, item_1hop, target_user, target_item; REMAP_SENTINEL in masked slices) and the
    id_status word"""
    G, TA = c.G, plan_active(c)
    shift = 1
    while shift < 31 and (1 << shift) < -(-c.N // G):
        shift += 1
    status, keys = 0, []
    for seg, feed in enumerate(FEED_OF_SEG):
        ids = t[feed].astype(np.int64)
        if seg < 4:
            ids = ids[:, :TA]
        bad = (ids < 0) | (ids >= c.N)
        if bad.any():
            status |= 1 << feed
        row = np.where(bad, 0, ids)
        keys.append(((row % G) << shift | (row // G)) if G > 1 else row)
    uk = np.unique(np.concatenate([k.reshape(-1) for k in keys] + [[0]]))          # (the sentinel: position 0 is row 0)
    offsets = np.concatenate([np.searchsorted(uk, np.arange(G) << shift), [len(uk)]]) if G > 1 else np.array([0, len(uk)])
    remap = []
    for seg, feed in enumerate(FEED_OF_SEG):
        full = np.full(t[feed].shape, REMAP_SENTINEL, np.int32)
        pos = np.searchsorted(uk, keys[seg]).astype(np.int32)
        if seg < 4:
            full[:, :TA] = pos
        else:
            full[...] = pos
        remap.append(full)
    return PlanProducts(len(uk), offsets.astype(np.int32), (uk & ((1 << shift) - 1)).astype(np.int32), remap, status)


def plan_judge(c, t, got):
    """got: PlanProducts read back from the workspace (remap: the six whole tensors, pre-filled with REMAP_SENTINEL)"""
    want = plan_reference(c, t)
    assert got.U == want.U, (c.name, "U", got.U, want.U)
    assert np.array_equal(got.offsets, want.offsets), (c.name, "owner offsets", got.offsets.tolist(), want.offsets.tolist())
    assert np.array_equal(got.unique_rows, want.unique_rows), (c.name, "unique_rows")
    assert got.id_status == want.id_status, (c.name, "id_status", got.id_status, want.id_status)
    TA = plan_active(c)
    for seg, feed in enumerate(FEED_OF_SEG):
        g = np.asarray(got.remap[seg]).reshape(t[feed].shape)
        if seg < 4:
            assert (g[:, TA:] == REMAP_SENTINEL).all(), (c.name, seg, "a masked slice was remapped")
            g, ids = g[:, :TA], t[feed][:, :TA].astype(np.int64)
        else:
            ids = t[feed].astype(np.int64)
        # the position names the id: its local row times G plus the owner read from the offsets
        assert ((g >= 0) & (g < got.U)).all(), (c.name, seg)
        owner = np.searchsorted(got.offsets[1:], g, side="right")
        named = got.unique_rows[g].astype(np.int64) * c.G + owner
        assert np.array_equal(named, np.where((ids < 0) | (ids >= c.N), 0, ids)), (c.name, seg, "remap")
        assert np.array_equal(g, want.remap[seg][:, :TA] if seg < 4 else want.remap[seg]), (c.name, seg)


# ---------------------------------------------------------------------------------------------- 4. score_auc_logloss
AUC_TOL = 1e-12
AucRow = namedtuple("AucRow", "name n kind why")
AUC_ROWS = {}
for _n in (1, 2, 255, 256, 257, 65536, 65537, 131073):
    AUC_ROWS["n%d" % _n] = AucRow("n%d" % _n, _n, "random", "one class only at n = 1: nan AUC" if _n == 1 else "")
for _name, _n, _kind, _why in (
        ("all_equal", 70001, "all_equal", "AUC exactly 0.5"),
        ("tie_across_the_grid_seam", 131073, "tie_60000_70000", "one tie group over sorted positions 60000 .. 70000 (seam at 65536)"),
        ("saturated", 1031, "saturated", "scores of exactly 0.0 and 1.0 with both labels: the clip at 2^-52"),
        ("labels_any_integer", 4099, "labels", "labels in {-1, 0, 2, 7}: non-zero is positive"),
        ("positives_only", 300, "pos_only", "nan AUC"), ("negatives_only", 300, "neg_only", "nan AUC")):
    AUC_ROWS[_name] = AucRow(_name, _n, _kind, _why)


def auc_inputs(r):
    rng = np.random.default_rng(_seed(r.name))
    n = r.n
    p = (rng.random(n) * 0.98 + 0.01).astype(np.float32)
    y = (rng.random(n) < p).astype(np.int32)
    if n >= 2:
        y[:2] = [0, 1]
    if r.kind == "all_equal":
        p[:] = np.float32(0.3)
    elif r.kind == "tie_60000_70000":
        p = ((np.arange(n) + 1.0) / (n + 2.0)).astype(np.float32)              # distinct, ascending
        p[60000:70001] = p[60000]
        perm = rng.permutation(n)
        p, y = p[perm], (rng.random(n) < 0.4).astype(np.int32)
    elif r.kind == "saturated":
        p[::3] = 0.0
        p[1::3] = 1.0
        y = (np.arange(n) // 3 % 2).astype(np.int32)
    elif r.kind == "labels":
        y = np.array([-1, 0, 2, 7, 0, 0], np.int32)[rng.integers(0, 6, n)]
    elif r.kind == "pos_only":
        y[:] = 3
    elif r.kind == "neg_only":
        y[:] = 0
    return p, y


def auc_reference(p, y):
    """(mid-rank AUC as a Fraction, None with one class only; log-loss in float64 with the clip at 2^-52)"""
    pos = y != 0
    n, n_pos = len(p), int(pos.sum())
    order = np.argsort(p, kind="stable")
    ps, ys = p[order], pos[order]
    heads = np.flatnonzero(np.concatenate([[True], ps[1:] != ps[:-1]]))
    cnt = np.diff(np.concatenate([heads, [n]]))
    pcnt = np.add.reduceat(ys.astype(np.int64), heads)
    # a tie group at sorted positions s .. s + c - 1 has the mid-rank (2 s + c + 1) / 2
    twice = sum(int(a) * (2 * int(s) + int(c) + 1) for a, s, c in zip(pcnt, heads, cnt) if a)
    auc = Fraction(twice - n_pos * (n_pos + 1), 2 * n_pos * (n - n_pos)) if 0 < n_pos < n else None
    eps = 2.0 ** -52
    q = np.clip(p.astype(np.float64), eps, 1.0 - eps)
    ll = -math.fsum(np.where(pos, np.log(q), np.log(1.0 - q)).tolist()) / n
    return auc, ll


def auc_judge(r, want_auc, want_ll, got_auc, got_ll):
    if want_auc is None:
        assert math.isnan(got_auc), (r.name, got_auc)
    else:
        assert abs(got_auc - float(want_auc)) < AUC_TOL, (r.name, "auc", got_auc, float(want_auc))
    assert abs(got_ll - want_ll) < AUC_TOL, (r.name, "log-loss", got_ll, want_ll)
