"""Cases and numpy restatements for "recommend by user id" (PointLogStore.user_lines / host_user_lines; include/score_hip.h:
score_point_user_lines, score_catalog_history_exclusions), built in ONE place: the CPU tests (test_user_lines_cpu.py) pin the
restatements and the cases' properties, the GPU tests (test_gpu_user_lines.py, test_gpu_history_exclusions.py) run them.

Logs.  `crafted_log` gives every user an exact number of events inside the window (what the kept-length cases need);
`hist_case_log` turns a case of tests/point_hist_cases.py (imported, not copied) into a log a PointLogStore takes: the events
whose entity lies in the case's range, the payload words folded into the item range.

Exclusions.  `restate_exclusions` is the contract in numpy -- per line np.unique of the catalogue positions of the user's whole
segment, without the keep id --, `brute_exclusions` the same by a double loop."""
import functools

import numpy as np

import point_hist_cases as phc

WINDOW = (2, 5)                  # [start_time, pred_time) of every crafted log


def rows_of(U, I, Fu, Fi, n_feat, seed):
    """user_rows [U, Fu] / item_rows [I, Fi]: column 0 the ids 1 .. U / U + 1 .. U + I, the others feature ids in [1, n_feat)"""
    rng = np.random.default_rng(seed)
    ur = rng.integers(1, n_feat, size=(U, Fu)).astype(np.int32)
    ir = rng.integers(1, n_feat, size=(I, Fi)).astype(np.int32)
    ur[:, 0] = np.arange(1, U + 1)
    ir[:, 0] = np.arange(U + 1, U + I + 1)
    return ur, ir


def crafted_log(counts, I, seed):
    """A log in which user u (1-based) has exactly counts[u - 1] events inside WINDOW, plus counts[u - 1] + 1 outside it (both
    sides), in random order with a dozen time keys (ties are the rule).  -> uid, iid, time_key, t_idx int32 [n]"""
    rng = np.random.default_rng(seed)
    U = len(counts)
    uid, ti = [], []
    for u, n in enumerate(counts, 1):
        uid += [u] * (2 * n + 1)
        ti += rng.integers(WINDOW[0], WINDOW[1], n).tolist() + rng.choice([0, 1, 5, 6], n + 1).tolist()
    order = rng.permutation(len(uid))
    uid, ti = np.asarray(uid, dtype=np.int32)[order], np.asarray(ti, dtype=np.int32)[order]
    iid = rng.integers(U + 1, U + I + 1, len(uid)).astype(np.int32)
    tk = rng.integers(0, 12, len(uid)).astype(np.int32)
    return uid, iid, tk, ti


def hist_case_log(name, I):
    """A case of point_hist_cases as a PointLogStore's log: events with the entity in range, users 1 .. n_ent, items
    n_ent + 1 + (payload mod I).  -> uid, iid, time_key, t_idx, U, (start, pred), H"""
    c = phc.case(name)
    e = c["ent"].astype(np.int64) - c["id_lo"]
    ok = (e >= 0) & (e < c["n_ent"])
    U = int(c["n_ent"])
    uid = (e[ok] + 1).astype(np.int32)
    iid = (U + 1 + c["other"][ok].astype(np.int64) % I).astype(np.int32)
    return uid, iid, c["time_key"][ok].copy(), c["t_idx"][ok].copy(), U, (c["start"], c["pred"]), c["H"]


def target_lines(uid, t_idx, window, U, I, per_line, n_lines, seed):
    """n_lines target lines (user, [per_line items]) over users that have an event inside the window, user 1 .. first"""
    rng = np.random.default_rng(seed)
    have = np.unique(uid[(t_idx >= window[0]) & (t_idx < window[1])])
    assert len(have) >= 1
    users = have[np.arange(n_lines) % len(have)]
    return [(int(u), rng.integers(U + 1, U + I + 1, per_line).tolist()) for u in users]


# ---- kept-length cases of the lines kernel ----------------------------------------------------------------------------------
H_LINES = 12                                 # hist_max_len of the lines stores
T_LINES = (8, 7)                             # T * Fi is a multiple of 4 for every Fi at 8; at 7 it is not for Fi = 1, 2
SHAPES_LINES = ((1, 1), (3, 4), (2, 2))      # (Fu, Fi)
# events per user: user 1 and user U have events; user 2 has none; 1, T - 1, T, T + 1 for both T; above hist_max_len
COUNTS_LINES = (3, 0, 1, 6, 7, 8, 9, H_LINES + 5, H_LINES, 2)
I_LINES = 40
NEG_LINES = 2


@functools.lru_cache(maxsize=None)
def lines_world(Fu, Fi):
    """-> dict(log=(uid, iid, time_key, t_idx), rows=(user_rows, item_rows), lines, U, I, args for PointLogStore)"""
    U = len(COUNTS_LINES)
    log = crafted_log(COUNTS_LINES, I_LINES, seed=5)
    rows = rows_of(U, I_LINES, Fu, Fi, 100, seed=6)
    lines = target_lines(log[0], log[3], WINDOW, U, I_LINES, 1 + NEG_LINES, 9, seed=7)
    for a in log + rows:
        a.setflags(write=False)
    return dict(log=log, rows=rows, lines=lines, U=U, I=I_LINES)


def store_of(w, build, neg=NEG_LINES, H=H_LINES, window=WINDOW, **kw):
    from score_amd.pointdata import PointLogStore
    per = 1 + neg
    log, rows = [a.copy() for a in w["log"]], [a.copy() for a in w["rows"]]          # (the world's arrays are read-only)
    return PointLogStore(*log, w["lines"], window[0], window[1], H, neg, len(w["lines"]) * per, rows[0], rows[1], False,
                         build=build, **kw)


def first_samples(batches, per_line):
    """(user_seq, length, target_user) of the first sample of every line of host-loader batches (5-tuples)"""
    seq = np.concatenate([b[0][::per_line] for b in batches])
    ln = np.concatenate([b[1][::per_line] for b in batches])
    tu = np.concatenate([b[2][::per_line] for b in batches])
    return seq, ln, tu


# ---- the exclusion contract ----------------------------------------------------------------------------------------------------
def restate_exclusions(off, seq, user_ids, keep_ids, cat_ids):
    """-> (excl_off int64 [L + 1], excl_idx int32): per line np.unique of the catalogue positions of the user's WHOLE segment
    seq[off[u - 1]:off[u]], without the keep id; an id outside 1 .. U has none"""
    off, seq, cat = np.asarray(off), np.asarray(seq), np.asarray(cat_ids)
    U = len(off) - 1
    lists = []
    for l, u in enumerate(np.asarray(user_ids).tolist()):
        if not 1 <= u <= U:
            lists.append(np.zeros((0,), dtype=np.int32))
            continue
        ids = seq[off[u - 1]:off[u]]
        if keep_ids is not None:
            ids = ids[ids != np.asarray(keep_ids)[l]]
        pos = np.searchsorted(cat, ids)
        hit = (pos < len(cat)) & (cat[np.minimum(pos, len(cat) - 1)] == ids)
        lists.append(np.unique(pos[hit]).astype(np.int32))
    out_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return out_off, (np.concatenate(lists) if lists else np.zeros((0,))).astype(np.int32)


def brute_exclusions(off, seq, user_ids, keep_ids, cat_ids):
    """the same by a double loop over (catalogue index, history entry)"""
    U = len(off) - 1
    out_off, out = [0], []
    for l, u in enumerate(list(user_ids)):
        if 1 <= u <= U:
            seg = [int(x) for x in seq[off[u - 1]:off[u]]]
            for j, c in enumerate(list(cat_ids)):
                if (keep_ids is None or int(c) != int(keep_ids[l])) and any(x == int(c) for x in seg):
                    out.append(j)
        out_off.append(len(out))
    return np.asarray(out_off, dtype=np.int64), np.asarray(out, dtype=np.int32)


EXCL_THREADS = 256               # history entries a workgroup takes a stride (the plan function says so: asserted by the tests)
EXCL_RANGE = 32768               # catalogue indices a workgroup covers (likewise)
EXCL_SMALL_N = (1, 31, 32, 33, 64, 65)
EXCL_SEGMENTS = (0, 1, 255, 256, 257, 300, 40, 600)       # user 1 .. 8; 300: one item throughout; 40: nothing of the catalogue
CAT_BASE = 10                    # catalogue ids are CAT_BASE + 2 j: every odd id, and every id outside the span, is in no catalogue


def excl_seam_ns(R=EXCL_RANGE):
    return (R - 1, R, R + 1, 2 * R + 1)


@functools.lru_cache(maxsize=None)
def excl_world(N, R=EXCL_RANGE):
    """A history CSR of eight users against a catalogue of N ids, made for the seams: -> dict(off, seq, cat_ids, U, keep) with
    user 2: one event, catalogue index 0;   users 3 .. 5: 255 / 256 / 257 events (the stride's seam), a mix of catalogue ids
    (with repeats), odd ids and ids below / above the catalogue's span;   user 5 also holds the first and the last catalogue index
    and every index next to a range seam (R - 1, R, 2 R - 1, 2 R where N has them);   user 6: 300 times one item;   user 7: 40
    events, none of the catalogue;   user 8: 600 events, its keep id 37 times among them, catalogue indices on both sides of every
    range seam.  keep[u - 1]: a keep id per user -- absent from the segment (users 1 .. 5, 7: an id of the catalogue where N
    allows), the repeated item itself (user 6), present many times (user 8)."""
    rng = np.random.default_rng([N, 3])
    cat = (CAT_BASE + 2 * np.arange(N)).astype(np.int32)
    seams = np.asarray([j for j in (0, N - 1, R - 2, R - 1, R, R + 1, 2 * R - 1, 2 * R) if 0 <= j < N], dtype=np.int64)

    def mix(n):
        kind = rng.random(n)
        inside = cat[rng.integers(0, N, n)].astype(np.int64)
        odd = CAT_BASE + 1 + 2 * rng.integers(0, N, n)
        far = np.where(rng.random(n) < 0.5, rng.integers(1, CAT_BASE, n), int(cat[-1]) + 1 + rng.integers(0, 50, n))
        return np.where(kind < 0.5, inside, np.where(kind < 0.8, odd, far))
    segs = [np.zeros((0,), dtype=np.int64), cat[:1].astype(np.int64), mix(255), mix(256), mix(257),
            np.full(300, int(cat[N // 2])), None, mix(600)]
    segs[4][:len(seams)] = cat[seams]
    segs[4] = rng.permutation(segs[4])
    segs[6] = np.where(rng.random(40) < 0.5, CAT_BASE + 1 + 2 * rng.integers(0, N, 40), rng.integers(1, CAT_BASE, 40))
    keep8 = int(cat[min(N - 1, R)] if N > R else cat[N - 1])
    segs[7][:len(seams)] = cat[seams]
    segs[7][len(seams):len(seams) + 37] = keep8
    segs[7] = rng.permutation(segs[7])
    assert [len(s) for s in segs] == list(EXCL_SEGMENTS)
    off = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    seq = np.concatenate(segs).astype(np.int32)
    keep = []
    for u, s in enumerate(segs, 1):
        free = np.setdiff1d(cat, s)
        keep.append(int(free[len(free) // 2]) if len(free) else -7)
    absent8 = keep[7]            # (a catalogue id user 8's segment does not hold; -7, in no catalogue, where it holds them all)
    keep[5], keep[7] = int(cat[N // 2]), keep8
    for a in (off, seq, cat):
        a.setflags(write=False)
    return dict(off=off, seq=seq, cat_ids=cat, U=len(segs), keep=np.asarray(keep, dtype=np.int32), seams=seams, absent8=absent8)


def keep_present_once(w):
    """a catalogue id that stands exactly once in user 8's segment (where there is none -- N = 1 --, the segment's first id)"""
    seg = w["seq"][w["off"][7]:w["off"][8]]
    vals, cnt = np.unique(seg, return_counts=True)
    ones = vals[(cnt == 1) & np.isin(vals, w["cat_ids"])]
    return int(ones[0]) if len(ones) else int(seg[0])


# user-id vectors of the exclusion calls: L = 1, 2 (one more than the lines a workgroup takes), 3, every user with the unknown
# ids 0, U + 1 and -3 between known ones, and one user three times (its keep id absent / present once / present many times is
# the keep vector's business: excl_calls pairs them)
def excl_calls(w):
    U, keep = w["U"], w["keep"]
    k = lambda users: np.asarray([keep[u - 1] if 1 <= u <= U else 0 for u in users], dtype=np.int32)
    every = [1, 2, 3, 0, 4, 5, U + 1, 6, 7, -3, 8]
    once = keep_present_once(w)
    calls = [([5], k([5])), ([8, 5], k([8, 5])), ([3, U + 7, 4], k([3, U + 7, 4])), (every, k(every)), (every, None),
             ([8, 8, 8], np.asarray([w["absent8"], once, keep[7]], dtype=np.int32)), ([6, 6], np.asarray([keep[5], keep[0]], dtype=np.int32))]
    return [(np.asarray(u, dtype=np.int32), kk) for u, kk in calls]
