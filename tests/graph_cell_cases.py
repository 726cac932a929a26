"""The per-cell draw rule of TemporalGraph.from_log(draws="cell") restated in plain Python -- one list per cell, Python's
`sorted` on (key, position), nothing of score_amd, no numpy sort -- and the logs test_graph_cell_draws.py and
test_gpu_graph_build.py share.  Not a test module."""
import os
from collections import defaultdict

import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, tag, c, j):
    h = mix((seed + G * ((tag << 40) + c + 1)) & M64)
    return mix((h + G * (j + 1)) & M64) >> 32


def random_order(seed, tag, c, n, key=key):
    """the random order of n positions of cell c: sorted by (key, position)"""
    return sorted(range(n), key=lambda j: (key(seed, tag, c, j), j))


def restate(uid, iid, t_idx, U, I, S, m1, m2, seed, key=key):
    """-> ({'user' | 'item': (hop1, hop2, deg)}, stats); hop1 / hop2 / deg: dict cell -> list, non-empty cells only.
    stats: what the log exercises (cell lengths, candidate counts, neighbour degrees seen, cuts of permuted lists)."""
    u1, i1 = defaultdict(list), defaultdict(list)
    for u, i, t in zip(np.asarray(uid).tolist(), np.asarray(iid).tolist(), np.asarray(t_idx).tolist()):
        if 1 <= u <= U and U + 1 <= i <= U + I and 0 <= t < S:          # anything else joins no cell
            u1[(u - 1) * S + t].append(i)
            i1[(i - U - 1) * S + t].append(u)
    stats = dict(len1=set(), cand=set(), d=set(), permuted_cut=0, shuffled=0)

    def shuffle(own, tag):
        for c, nb in own.items():
            stats["len1"].add(len(nb))
            if len(nb) > m1:
                nb[:] = [nb[j] for j in random_order(seed, tag, c, len(nb), key)]
                stats["shuffled"] += 1

    def two_hop(own, other, other_base, tag, other_log):
        out, deg = {}, {}
        for c, nb in own.items():
            t = c % S
            acc, dg = [], []
            for x in nb[:m1]:
                oc = (x - other_base) * S + t
                lst = other.get(oc, [])
                d = len(lst)
                stats["d"].add(d)
                if d > 1:
                    acc += lst[:m1]
                    dg += [d] * min(d, m1)
                    if other_log is not None and d > m1 and lst[:m1] != other_log[oc][:m1]:
                        stats["permuted_cut"] += 1
            stats["cand"].add(len(acc))
            if len(acc) > m2:
                order = random_order(seed, tag, c, len(acc), key)[:m2]
                acc, dg = [acc[j] for j in order], [dg[j] for j in order]
            if acc:
                out[c], deg[c] = acc, dg
        return out, deg
    i_log = {c: list(l) for c, l in i1.items()}
    shuffle(i1, 0)
    i2, ideg = two_hop(i1, u1, 1, 1, None)                 # reads user lists still in log order
    shuffle(u1, 2)
    u2, udeg = two_hop(u1, i1, U + 1, 3, i_log)            # reads item lists as the item pass left them
    return {"user": (dict(u1), u2, udeg), "item": (dict(i1), i2, ideg)}, stats


def assert_csr_equals(off, flat, cells, ncell, what):
    """CSR (off [ncell + 1], flat) == the non-empty cells of the restatement, every offset included"""
    off = np.asarray(off)
    assert off.shape == (ncell + 1,) and int(off[0]) == 0, what
    lens = np.diff(off)
    assert int(np.count_nonzero(lens)) == len(cells) and int(lens.min(initial=0)) >= 0, what
    assert int(off[-1]) == sum(len(l) for l in cells.values()) == len(flat), what
    for c, l in cells.items():
        assert np.asarray(flat[off[c]:off[c + 1]]).tolist() == l, (what, c)


def assert_graph_equals_restatement(g, sides, U, I, S):
    for side, n, csr, deg in (("user", U, g.user_csr, g.user_degrees), ("item", I, g.item_csr, g.item_degrees)):
        hop1, hop2, dg = sides[side]
        assert_csr_equals(csr["off1"], csr["nbr1"], hop1, n * S, side + " 1-hop")
        assert_csr_equals(csr["off2"], csr["nbr2"], hop2, n * S, side + " 2-hop")
        assert_csr_equals(csr["off2"], deg, dg, n * S, side + " degrees")


# ---- the shared logs: name -> (uid, iid, t_idx, U, I, S, max_1hop, max_2hop, seed) ------------------------------------------
def _random_log(rng, U, I, S, n, skew=3):
    uid = rng.integers(1, U + 1, n)
    iid = U + 1 + np.minimum((I * rng.random(n) ** skew).astype(np.int64), I - 1)
    return uid, iid, rng.integers(0, S, n)


def g5_case(tag, seed=3):
    z = np.load(os.path.join(GOLDEN, "g5_graph_store.npz"))
    U, I, S, m1, m2 = [int(x) for x in z[tag + "/dims"]]
    log = z[tag + "/log"]
    return log[:, 0], log[:, 1], log[:, 2], U, I, S, m1, m2, seed


def case(name):
    rng = np.random.default_rng(20)
    if name in ("g5_sparse", "g5_dense"):
        return g5_case(name[3:])
    if name == "edges":            # cell lengths max_1hop and max_1hop + 1, candidate counts max_2hop and max_2hop + 1, d = 1 and 2,
        return _random_log(rng, 12, 9, 3, 120, 2) + (12, 9, 3, 3, 5, 7)      # user cuts of item lists the item pass permuted
    if name == "max_1hop_1":
        return _random_log(rng, 10, 8, 2, 200) + (10, 8, 2, 1, 4, 8)
    if name == "max_2hop_1":
        return _random_log(rng, 10, 8, 2, 200) + (10, 8, 2, 4, 1, 9)
    if name == "rank_4096":        # max_1hop 64: up to 4,096 candidates ranked in one cell
        return _random_log(rng, 70, 70, 1, 20000, 1) + (70, 70, 1, 64, 100, 10)
    if name == "tile_seam":        # one cell of 8,192 and one of 8,193 entries: the sort's tile seam inside one shuffle
        U, I, S = 300, 5, 2
        u0, i0, t0 = _random_log(rng, U, I, S, 500)
        i0 = np.where((i0 <= U + 2) & (t0 == 0), U + 3, i0)                      # the two hot cells hold nothing else
        uid = np.concatenate([rng.integers(1, U + 1, 8192), u0, rng.integers(1, U + 1, 8193)])
        iid = np.concatenate([np.full(8192, U + 1), i0, np.full(8193, U + 2)])
        return uid, iid, np.concatenate([np.zeros(8192, np.int64), t0, np.zeros(8193, np.int64)]), U, I, S, 10, 100, 11
    if name == "no_over_long":     # no cell above max_1hop: the shuffle is skipped; max_2hop is still hit
        return _random_log(rng, 30, 30, 2, 600, 1) + (30, 30, 2, 64, 100, 12)
    if name == "flat":             # slice 2 unused, trailing entities without events: flat offsets
        uid, iid, t = _random_log(rng, 14, 11, 3, 300)
        return uid, iid, np.where(t == 2, 3, t), 20, 16, 5, 3, 6, 13
    if name == "sink":             # ids and slices outside their ranges
        U, I, S = 9, 7, 3
        uid, iid, t = _random_log(rng, U, I, S, 300)
        uid[::17], iid[5::19], t[3::23] = 0, U, -1
        uid[7::29], iid[11::31], t[13::37] = U + 1, U + I + 1, S
        return uid, iid, t, U, I, S, 3, 6, 14
    if name.startswith("cells_"):  # item cells on both sides of 4,096 and 2^24: one, two and three radix passes of the sort
        ncell = int(name[6:])
        U, I, S = 7, ncell, 1
        uid = rng.integers(1, U + 1, 20000)
        iid = U + 1 + rng.integers(0, I, 20000)
        iid[:3] = U + I, U + I - 1, U + 1                                        # the last cells are used
        return uid, iid, np.zeros(20000, np.int64), U, I, S, 10, 100, 15
    raise KeyError(name)


SMALL_CASES = ("g5_sparse", "g5_dense", "edges", "max_1hop_1", "max_2hop_1", "rank_4096", "tile_seam", "no_over_long", "flat",
               "sink", "cells_4095", "cells_4096", "cells_4097")
BIG_CASES = ("cells_16777215", "cells_16777216", "cells_16777217")


def rows(U, I):
    return np.arange(1, U + 1, dtype=np.int32)[:, None], np.arange(U + 1, U + I + 1, dtype=np.int32)[:, None]
