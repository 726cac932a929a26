"""Inputs shared by test_target_cell_draws.py (CPU) and test_gpu_target_build.py: named logs for the target-line build.
case(name) -> dict(uid, iid, t_idx, U, I, S, pred, start, neg, seed, pop, factor); the arrays are read-only."""
import functools
import os

import numpy as np

from score_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCAN_TILE, SORT_TILE = _lib.TARGET_SCAN_TILE, _lib.TARGET_SORT_TILE
# event counts at one below, exactly and one above each tile size, and twice a tile plus one (seven distinct counts: twice the
# scan's tile plus one IS the sort's tile plus one)
TILE_COUNTS = sorted({t + d for t in (SCAN_TILE, SORT_TILE) for d in (-1, 0, 1)} | {2 * SCAN_TILE + 1, 2 * SORT_TILE + 1})


def _random_log(rng, n, U, I, S):
    return rng.integers(1, U + 1, n), rng.integers(U + 1, U + I + 1, n), rng.integers(0, S, n)


def _edges():
    """U = 9, I = 6 (items 10 .. 15), S = 6, start 2, pred 4.
    user 1: history and two slice events                                  -> line, positive the first
    user 2: a slice event, no other event                                 -> no line
    user 3: a slice event, earlier events all before start_time           -> no line
    user 4: slice events interleaved with others'; first in log order is the LARGEST id -> that one
    user 5: history only, no slice event                                  -> no line
    user 6: its first slice event carries an item id outside the range (dropped); the next is the positive
    user 7: a slice event; its only history event has a negative slice / a bad item id (dropped) -> no line
    user 8: history at the last counted slice (pred - 1) and at start exactly
    user 9 (the highest id): eligible
    uid 0 and uid 10: outside the range, dropped."""
    ev = [(1, 10, 2), (4, 15, 4), (1, 12, 4), (2, 11, 4), (4, 10, 4), (3, 10, 0), (3, 11, 1), (1, 11, 4), (3, 12, 4),
          (4, 11, 3), (5, 10, 2), (5, 13, 3), (6, 16, 4), (6, 9, 4), (6, 14, 4), (6, 10, 2), (7, 10, -1), (7, 16, 3),
          (7, 12, 4), (8, 13, 3), (8, 14, 2), (8, 15, 4), (9, 10, 3), (9, 11, 4), (0, 10, 4), (10, 10, 4), (0, 10, 3),
          (10, 11, 2), (4, 12, 4), (2, 12, 5), (3, 13, 5)]
    a = np.asarray(ev, dtype=np.int64)
    return a[:, 0], a[:, 1], a[:, 2]


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.Generator(np.random.PCG64(abs(hash_name(name))))
    c = dict(S=6, pred=4, start=1, neg=3, seed=11, pop=None, factor=0)
    if name.startswith("tile_"):                       # tile_<n>: n random events
        n = int(name.split("_")[1])
        c.update(U=300, I=50)
        c["uid"], c["iid"], c["t_idx"] = _random_log(rng, n, 300, 50, 6)
    elif name.startswith("edges"):                     # edges, edges_neg<k>, edges_factor<f>_seed<s>, edges_pop
        c.update(U=9, I=6, start=2)
        c["uid"], c["iid"], c["t_idx"] = _edges()
        for part in name.split("_")[1:]:
            if part.startswith("neg"):
                c["neg"] = int(part[3:])
            elif part.startswith("factor"):
                c["factor"] = int(part[6:])
            elif part.startswith("seed"):
                c["seed"] = int(part[4:])
            elif part == "pop":
                c["pop"] = np.asarray([11, 12, 15], dtype=np.int32)
    elif name == "no_pred_slice":
        c.update(U=40, I=20, pred=5)
        u, i, t = _random_log(rng, 500, 40, 20, 5)
        c["uid"], c["iid"], c["t_idx"] = u, i, t
    elif name.startswith("all_eligible"):              # all_eligible, all_eligible_neg<k>
        rng = np.random.Generator(np.random.PCG64(130))
        c.update(U=130, I=17)
        if "_neg" in name:
            c["neg"] = int(name.split("_neg")[1])
        u = np.concatenate([np.arange(1, 131), rng.permutation(np.arange(1, 131)), rng.integers(1, 131, 200)])
        t = np.concatenate([np.full(130, 3), np.full(130, 4), rng.integers(0, 6, 200)])
        c["uid"], c["iid"], c["t_idx"] = u, rng.integers(131, 148, len(u)), t
    elif name == "one_item":
        c.update(U=70, I=1)
        u, _, t = _random_log(rng, 700, 70, 1, 6)
        c["uid"], c["iid"], c["t_idx"] = u, np.full(700, 71), t
    elif name == "highest_user_only":
        c.update(U=200, I=30)
        u, i, t = _random_log(rng, 900, 199, 30, 4)               # nobody else reaches slice 4
        c["uid"] = np.concatenate([u, [200, 200]])
        c["iid"] = np.concatenate([i + 1, [205, 230]])
        c["t_idx"] = np.concatenate([t, [2, 4]])
    elif name.startswith("factor"):                    # factor<f>: 3000 events, down-sampled
        c.update(U=400, I=64, factor=int(name[6:]))
        c["uid"], c["iid"], c["t_idx"] = _random_log(rng, 3000, 400, 64, 6)
    elif name.startswith("pop_list"):                  # pop_list, pop_list_factor4_neg99
        rng = np.random.Generator(np.random.PCG64(5))
        c.update(U=150, I=90, neg=7, pop=np.sort(rng.choice(np.arange(151, 241), 23, replace=False)).astype(np.int32))
        c["uid"], c["iid"], c["t_idx"] = _random_log(rng, 1500, 150, 90, 6)
        if name.endswith("_factor4_neg99"):
            c.update(factor=4, neg=99)
        elif "_neg" in name:
            c["neg"] = int(name.split("_neg")[1])
    elif name.startswith("users_"):                    # users_<U>, users_<U>_pop: 600 events, most users absent, 40 or so eligible
        U = int(name.split("_")[1])                    # (both ends of the id range among them); the sort's keys are 0 .. U
        some = np.unique(np.concatenate([[1, U], rng.integers(1, U + 1, 38)]))
        u, i, t = _random_log(rng, 600 - 2 * len(some), U, 50, 6)
        order = rng.permutation(600)
        c.update(U=U, I=50)
        c["uid"] = np.concatenate([some, some, u])[order]
        c["iid"] = np.concatenate([rng.integers(U + 1, U + 51, 2 * len(some)), i])[order]
        c["t_idx"] = np.concatenate([np.full(len(some), 2), np.full(len(some), 4), t])[order]
        if name.endswith("_pop"):
            c["pop"] = np.sort(rng.choice(np.arange(U + 1, U + 51), 9, replace=False)).astype(np.int32)
    else:
        raise KeyError(name)
    for k in ("uid", "iid", "t_idx"):
        c[k] = np.ascontiguousarray(c[k], dtype=np.int64)
        c[k].setflags(write=False)
    return c


def hash_name(name):
    return sum((k + 1) * ord(ch) for k, ch in enumerate(name)) * 2654435761 % (2 ** 31)


def sort_passes(max_key):
    """radix passes of score_sort_pairs over keys 0 .. max_key: 12 bits a pass.  An odd count leaves the result in the
    alternate pair of arrays, an even one in the first"""
    return -(-max(1, int(max_key).bit_length()) // 12)


# line widths 1 + neg above 4 that are no multiple of 4 words: most lines start off a 16-byte boundary, so the fill kernel's
# one-word stores in front of and behind its 16-byte stores all run
ODD_WIDTH_CASES = ["all_eligible_neg4", "all_eligible_neg6", "all_eligible_neg100", "pop_list_neg6", "pop_list_neg10"]
# user counts on both sides of the sort's second pass (keys 0 .. U: 12 bits hold 4,095, 13 are two passes)
PASS_CASES = ["users_4095", "users_4096", "users_4096_pop"]
CASES = (["tile_%d" % n for n in TILE_COUNTS] +
         ["edges", "edges_neg0", "edges_neg1", "edges_neg99", "edges_neg4095", "edges_factor1", "edges_factor4_seed3", "edges_pop",
          "pop_list_factor4_neg99", "no_pred_slice", "all_eligible", "one_item", "highest_user_only", "factor0", "factor1",
          "factor4", "pop_list"] + ODD_WIDTH_CASES + PASS_CASES)


def host_lines(c):
    """the host rule on a case: gen_target_lines(draws="cell"), then sample_target_lines(draws="cell") where factor > 1"""
    from score_amd import dataprep as dp
    lines = dp.gen_target_lines(c["uid"], c["iid"], c["t_idx"], c["U"], c["I"], c["pred"], c["neg"], c["start"], c["seed"],
                                draws="cell", pop_items=c["pop"])
    return dp.sample_target_lines(lines, c["factor"], c["seed"], draws="cell") if c["factor"] > 1 else lines


def rows(U, I):
    """feature tables whose column 0 is the id"""
    ur = np.stack([np.arange(1, U + 1), np.arange(1, U + 1) % 5 + U + I + 1], axis=1).astype(np.int32)
    ir = np.stack([np.arange(U + 1, U + I + 1), np.arange(I) % 7 + U + I + 6], axis=1).astype(np.int32)
    return ur, ir


# ---- graphs for the pop list: (U, I, S, events) with item counts at the scan's tile edges ---------------------------------
@functools.lru_cache(maxsize=None)
def pop_graph_log(n_items):
    """a log over n_items items, S = 5, in which the number of non-empty slices per item covers 0 .. S"""
    rng = np.random.Generator(np.random.PCG64(n_items))
    U, S = 37, 5
    want = rng.integers(0, S + 1, n_items)                         # non-empty slices of item i
    want[[0, n_items - 1]] = S                                     # both ends of the id range in the list at pop_standard S
    ev = [(int(rng.integers(1, U + 1)), U + 1 + i, int(t)) for i in range(n_items)
          for t in rng.permutation(S)[:want[i]] for _ in range(int(rng.integers(1, 3)))]
    ev = np.asarray([ev[j] for j in rng.permutation(len(ev))], dtype=np.int64)
    for a in (ev, want):
        a.setflags(write=False)
    return U, n_items, S, ev, want


POP_ITEM_COUNTS = (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1, 50)
