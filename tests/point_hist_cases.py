"""The inputs of the history-build edge tests (csrc/pointhist.hip: score_point_hist_build), built in ONE place: the GPU test
(test_gpu_point_history.py) runs them, and the CPU test (test_point_history_cpu.py) rebuilds exactly the same inputs and asserts,
on the restatement below alone, the properties that make them worth running.  Seeds were chosen on the CPU from the restatement
(never from a GPU run); the CPU test keeps them honest.

`restate` is an independent yardstick: plain Python written the way the reference's gen_user_item_hist_dict_* builds a history
(gen_target.py:223-275) -- a dict of (other, time) lists per entity filled in log order, each list sorted with Python's STABLE
sorted(key=time) -- with no numpy sort and no call into score_amd.

What the build does with a key, for reading the table (pointhist.hip, sort.hip): bits(n_ent) counts the sink entity n_ent, so it
is n_ent.bit_length(); ONE sort of bits(n_ent) + time_bits bits where that is at most 32, else TWO, by time_bits and then by
bits(n_ent); a sort of b bits takes ceil(b / 12) radix passes; its tiles hold 8,192 pairs, and up to 64 tiles the scatter kernel
scans its own histogram columns, beyond that a column-scan launch does."""
import functools

import numpy as np

TILE = 8192                      # pairs per tile of the sort
FUSED_MAX_TILES = 64             # the last tile count without a column-scan launch
WINDOW = (2, 5)                  # [start_time, pred_time) of every case but empty_window; t_idx is uniform over 0 .. 6
T_IDX_HI = 7

# name -> (n, n_ent, id_lo, time_bits, H, seed, key bits as the table of the issue states them, sorts, passes per sort)
CASES = {
    "one_pass":          (300, 5, 1, 4, 3, 0, 7, 1, (1,)),                   # 7-bit key: one radix pass, result in the alt buffers
    "tile_exact":        (8192, 300, 7, 10, 64, 0, 19, 1, (2,)),             # exactly one full tile; id_lo != 1
    "two_tiles":         (8193, 300, 1, 10, 64, 1, 19, 1, (2,)),             # a second tile of one pair (seed: it ends a tie)
    "ties_across_tiles": (16384, 3, 1, 1, 5000, 0, 3, 1, (1,)),              # runs of equal keys thousands long over the tile seam
    "pack30":            (20000, 400000, 1, 11, 8, 0, 30, 1, (3,)),          # Tmall users' width: 19 + 11
    "pack32_top_bit":    (20000, 2 ** 20 + 3, 1, 11, 8, 0, 32, 1, (3,)),     # Tmall items' width: 21 + 11, top bit set, n_ent > n
    "pack33":            (20000, 2 ** 20 + 3, 1, 12, 8, 0, 33, 2, (1, 2)),   # one bit more: two sorts
    "both_even":         (20000, 10000, 1, 20, 8, 0, 34, 2, (2, 2)),         # two sorts, an even number of passes each
    "ent255_t24":        (5000, 255, 1, 24, 10, 0, 32, 1, (3,)),             # 8 + 24 = 32: one sort
    "ent256_t24":        (5000, 256, 1, 24, 10, 0, 33, 2, (2, 1)),           # a power of two: the sink needs a 9th bit
    "ent256_t23":        (5000, 256, 1, 23, 10, 0, 32, 1, (3,)),             # 9 + 23 = 32: one sort again
    "time31":            (5000, 300, 1000, 31, 1, 0, 40, 2, (3, 1)),         # the widest legal time key; H = 1
    "one_entity":        (700, 1, 5, 6, 1, 0, 7, 1, (1,)),                   # n_ent = 1: entity 0 and the sink only
    "fused_limit":       (524288, 3000, 1, 11, 300, 0, 23, 1, (2,)),         # 64 tiles: the last size on the fused column scan
    "past_fused":        (524289, 3000, 1, 11, 300, 0, 23, 1, (2,)),         # 65 tiles: the first size with the column-scan launch
    "empty_window":      (5000, 300, 1, 10, 64, 0, 19, 1, (2,)),             # window [9, 9): every key is the sink, off all zero
}
NAMES = tuple(CASES)

# The second build of a case, into the same workspace right behind the first (PointLogStore._build_device's use of `temp`), has
# the roles of the two id columns exchanged.  `other` holds random 31-bit words, so as ENTITIES they are sparse: the exchanged
# build looks at the 2^22 + 1 ids from 2^30 on -- n / 512 of the events -- and keeps 2 ids each.  23 entity bits (one sort of
# 3 passes up to time_bits 9, two sorts above, the entity sort of 2 passes); where that is the first build's own pass structure
# (pack33, both_even), 2^24 + 1 ids: 25 bits, an entity sort of 3 passes.  So the workspace is always left by another structure.
SWAP_ID_LO, SWAP_H = 2 ** 30, 2


def bits_of(x):
    """bits that hold the values 0 .. x"""
    return max(1, int(x).bit_length())


def passes(key_bits):
    return (key_bits + 11) // 12


def structure(n_ent, time_bits):
    """(key bits, number of sorts, radix passes of each sort) of a build"""
    eb = bits_of(n_ent)
    if eb + time_bits <= 32:
        return eb + time_bits, 1, (passes(eb + time_bits),)
    return eb + time_bits, 2, (passes(time_bits), passes(eb))


def swap_n_ent(name):
    n_ent, time_bits = CASES[name][1], CASES[name][3]
    wide = 2 ** 22 + 1
    return wide if structure(wide, time_bits)[1:] != structure(n_ent, time_bits)[1:] else 2 ** 24 + 1


def _ranked(rng, lo, hi, hole, k):
    """k entities of lo .. hi - 1, the highest the most frequent (weight rank^-1.5 from the top), `hole` never"""
    ents = np.arange(hi - 1, lo - 1, -1, dtype=np.int64)
    w = (1.0 + np.arange(len(ents))) ** -1.5
    w[ents == hole] = 0.0
    return rng.choice(ents, size=k, p=w / w.sum())


@functools.lru_cache(maxsize=None)
def case(name):
    """the log of a case and its arguments: dict(ent, other, time_key, t_idx [n] int32 (read-only), start, pred, id_lo, n_ent,
    time_bits, H, n).
    Entities: half the events from the lowest 50 of the range, half from the highest 40, skewed inside each group towards its
    highest entity (so that one entity is cut at H even where H is thousands, and the entity in front of the sink is a busy one);
    entity n_ent - 2 never occurs (an empty segment between two full ones).  5 % of the events have ids just below id_lo
    (negative where id_lo = 1), 5 % just above the range.  `other`: random 31-bit words -- equal keys carry different payloads,
    so a stability error is visible.  Times: about a dozen values, always 0 and 2^time_bits - 1, so ties are the rule."""
    n, n_ent, id_lo, time_bits, H, seed = CASES[name][:6]
    rng = np.random.default_rng([seed, NAMES.index(name)])
    hole = n_ent - 2 if n_ent > 1 else -1
    group = rng.random(n) < 0.5
    e = np.where(group, _ranked(rng, 0, min(50, n_ent), hole, n), _ranked(rng, max(0, n_ent - 40), n_ent, hole, n))
    u = rng.random(n)
    near = rng.integers(0, 3, n)
    ent = np.where(u < 0.05, id_lo - 1 - near, np.where(u < 0.10, id_lo + n_ent + near, id_lo + e))
    other = rng.integers(0, 2 ** 31, n)
    top = 2 ** time_bits - 1
    times = np.unique(np.concatenate([[0, top], rng.integers(0, top + 1, 10)]))
    time_key = rng.choice(times, n)
    t_idx = rng.integers(0, T_IDX_HI, n)
    start, pred = (9, 9) if name == "empty_window" else WINDOW
    cols = [np.ascontiguousarray(a, dtype=np.int32) for a in (ent, other, time_key, t_idx)]
    for a in cols:
        a.setflags(write=False)
    return dict(ent=cols[0], other=cols[1], time_key=cols[2], t_idx=cols[3], start=start, pred=pred, id_lo=id_lo, n_ent=n_ent,
                time_bits=time_bits, H=H, n=n, name=name)


def swapped(c):
    """the arguments of the case's second build: the two id columns exchanged"""
    return dict(c, ent=c["other"], other=c["ent"], id_lo=SWAP_ID_LO, n_ent=swap_n_ent(c["name"]), H=SWAP_H)


def histories(ent, other, time_key, t_idx, start, pred, id_lo, n_ent):
    """{entity 0 .. n_ent - 1: [(other, time, position in the log), ...] in history order} over the events of the window"""
    hist = {}
    for pos, (e, o, tk, t) in enumerate(zip(ent.tolist(), other.tolist(), time_key.tolist(), t_idx.tolist())):
        if t < start or t >= pred:
            continue
        e -= id_lo
        if e < 0 or e >= n_ent:
            continue
        if e not in hist:
            hist[e] = [(o, tk, pos)]
        else:
            hist[e].append((o, tk, pos))
    return {e: sorted(l, key=lambda tup: tup[1]) for e, l in hist.items()}


def restate(ent, other, time_key, t_idx, start, pred, id_lo, n_ent, H):
    """-> off int64 [n_ent + 1], seq int32 [off[n_ent]], len int32 [n_ent]"""
    hist = histories(ent, other, time_key, t_idx, start, pred, id_lo, n_ent)
    count = np.zeros(n_ent, dtype=np.int64)
    seq = []
    for e in sorted(hist):
        count[e] = len(hist[e])
        seq += [tup[0] for tup in hist[e]]
    off = np.zeros(n_ent + 1, dtype=np.int64)
    off[1:] = np.cumsum(count)
    return off, np.asarray(seq, dtype=np.int32).reshape(-1), np.minimum(count, H).astype(np.int32)


ARGS = ("ent", "other", "time_key", "t_idx", "start", "pred", "id_lo", "n_ent", "H")


@functools.lru_cache(maxsize=None)
def expected(name, swap=False):
    """restate over the case (or its exchanged second build), computed once per process; the arrays are read-only"""
    c = swapped(case(name)) if swap else case(name)
    out = restate(*[c[k] for k in ARGS])
    for a in out:
        a.setflags(write=False)
    return out
