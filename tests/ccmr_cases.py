"""Inputs shared by the CCMR device tests (test_gpu_ccmr_prep.py): target-build cases of target_cases.py with negative events
beside them, and raw rating logs.  case(name) -> target_cases' dict plus neg_uid / neg_iid; the arrays are read-only."""
import datetime
import functools

import numpy as np

import target_cases as tc

SCAN_TILE, SORT_TILE = tc.SCAN_TILE, tc.SORT_TILE
NEG_COUNTS = (0, 1, SCAN_TILE - 1, SCAN_TILE + 1, SORT_TILE - 1, SORT_TILE + 1)
WIDTHS = (1, 5, 6, 99, 100)                       # neg_sample_num: lines of 2, 6, 7, 100 and 101 words


def _events_of_lengths(rng, lens, U, I):
    """negative events in a random order in which user u + 1 has lens[u] of them"""
    u = np.repeat(np.arange(1, len(lens) + 1), lens)
    u = u[rng.permutation(len(u))]
    return u, rng.integers(U + 1, U + I + 1, len(u))


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.Generator(np.random.PCG64(tc.hash_name(name)))
    if name.startswith("nneg_"):                    # nneg_<n>: n negative events over all users (and two outside the id range)
        c = dict(tc.case("all_eligible"), neg=99)   # (99: above every list's length, so each line holds a list AND draws)
        n = int(name.split("_")[1])
        u, i = rng.integers(1, c["U"] + 1, n), rng.integers(c["U"] + 1, c["U"] + c["I"] + 1, n)
        if n > 10:
            u[[3, n - 2]] = [0, c["U"] + 1]
    elif name == "one_owner":                       # one user owns every negative event
        c = dict(tc.case("all_eligible"))
        u, i = np.full(500, 77), rng.integers(c["U"] + 1, c["U"] + c["I"] + 1, 500)
    elif name == "all_long_neg5":                   # every list at least neg long: no draw is made
        c = dict(tc.case("all_eligible_neg4"), neg=5)
        u, i = _events_of_lengths(rng, rng.integers(5, 9, c["U"]), c["U"], c["I"])
    elif name == "lens_neg5":                       # lists of length neg - 1, neg, neg + 1 (and 0)
        c = dict(tc.case("all_eligible_neg4"), neg=5)
        u, i = _events_of_lengths(rng, np.asarray([4, 5, 6, 0])[np.arange(c["U"]) % 4], c["U"], c["I"])
    elif name.startswith("width_neg"):              # width_neg<k>: lists of 0 .. k + 2 entries
        k = int(name[len("width_neg"):])
        c = dict(tc.case("all_eligible_neg4"), neg=k)
        u, i = _events_of_lengths(rng, rng.integers(0, k + 3, c["U"]), c["U"], c["I"])
    elif name == "pop_lists":                       # a pop list together with lists
        c = dict(tc.case("pop_list"))
        u, i = _events_of_lengths(rng, rng.integers(0, 12, c["U"]), c["U"], c["I"])
    elif name == "factor_lists":                    # a down-sampling factor together with lists
        c = dict(tc.case("factor4"))
        u, i = _events_of_lengths(rng, rng.integers(0, 6, c["U"]), c["U"], c["I"])
    elif name.startswith("users_"):                 # users_<U>: target_cases' case of that name and 500 negative events, half of
        c = dict(tc.case(name))                     # them of users of its log; a uid outside the range on each side
        u = np.concatenate([rng.choice(c["uid"], 250), rng.integers(1, c["U"] + 1, 250)])
        u[[7, 491]] = [c["U"] + 1, 0]
        i = rng.integers(c["U"] + 1, c["U"] + c["I"] + 1, 500)
    else:
        raise KeyError(name)
    c["neg_uid"], c["neg_iid"] = np.ascontiguousarray(u, dtype=np.int64), np.ascontiguousarray(i, dtype=np.int64)
    c["neg_uid"].setflags(write=False)
    c["neg_iid"].setflags(write=False)
    return c


LIST_CASES = (["nneg_%d" % n for n in NEG_COUNTS] + ["one_owner", "all_long_neg5", "lens_neg5", "pop_lists", "factor_lists"] +
              ["width_neg%d" % k for k in WIDTHS] + ["users_4095", "users_4096"])
PASS_LOGS = ("items_4095", "items_4096")          # raw logs whose movie lines sort in one and in two passes (keys 0 .. I)

START = datetime.date(2005, 5, 19)
# calendar edges, and both sides of the start: the 89th day before it is still slice 0, the 90th is slice -1
EDGE_DATES = (20040228, 20040229, 20040301, 20050228, 20050301, 20000229, 20001231, 20010101, 19000228, 19000301, 21000228,
              21000301, 20050430, 20050501, 20051231, 20060101, 10101, 99991231, 20050219, 20050218, 20050217, 20050518, 20050519,
              20050520, 20050816, 20050817, 20041120, 20041119)
VOCAB = (9, 14, 4, 6)


def yyyymmdd(day_from_start):
    d = START + datetime.timedelta(days=int(day_from_start))
    return d.year * 10000 + d.month * 100 + d.day


@functools.lru_cache(maxsize=None)
def raw_log(name):
    """-> (log [n, 4], movie_info [m, 5], U, I): 'edges' = one event per EDGE_DATES entry and rating; 'tenk' = about 10 k events
    over 41 slices and some days before the start, about a fifth of them negative; 'items_<I>' = 400 events over the 250 items
    that have a movie line (300 lines: 50 items have two), most of the I items without one"""
    rng = np.random.Generator(np.random.PCG64(tc.hash_name(name)))
    if name == "edges":
        U, I = 7, 5
        dates = np.repeat(np.asarray(EDGE_DATES), 5)
        n = len(dates)
        log = np.stack([rng.integers(0, U, n), rng.integers(0, I, n), np.tile(np.arange(1, 6), len(EDGE_DATES)), dates], axis=1)
    elif name == "tenk":
        U, I, n = 300, 120, 10000
        days = rng.integers(-150, 41 * 90, n)
        days[:3000] = rng.integers(37 * 90, 41 * 90, 3000)          # the three prediction slices are well filled
        rating = np.where(rng.random(n) < 0.2, rng.integers(1, 4, n), rng.integers(4, 6, n))
        log = np.stack([rng.integers(0, U, n), rng.integers(0, I, n), rating, [yyyymmdd(d) for d in days]], axis=1)
        log = log[rng.permutation(n)]
    elif name.startswith("items_"):
        U, I, n = 40, int(name.split("_")[1]), 400
        lined = np.concatenate([[0, I - 1], rng.choice(np.arange(1, I - 1), 248, replace=False)])
        rating = np.where(rng.random(n) < 0.2, rng.integers(1, 4, n), rng.integers(4, 6, n))
        log = np.stack([rng.integers(0, U, n), rng.choice(lined, n), rating, [yyyymmdd(d) for d in rng.integers(0, 41 * 90, n)]], axis=1)
        items = np.concatenate([lined, rng.choice(lined, 50, replace=False)])[rng.permutation(300)]
    else:
        raise KeyError(name)
    if not name.startswith("items_"):
        items = np.concatenate([rng.permutation(I), rng.integers(0, I, I // 3)])  # a third of the items has a second line
    feat = np.stack([np.where(rng.random(len(items)) < 0.2, -1, rng.integers(0, v - 1, len(items))) for v in VOCAB], axis=1)
    movie = np.concatenate([items[:, None], feat], axis=1)
    log, movie = np.ascontiguousarray(log, dtype=np.int64), np.ascontiguousarray(movie, dtype=np.int64)
    log.setflags(write=False)
    movie.setflags(write=False)
    return log, movie, U, I
