"""Inputs shared by test_log_remap_cpu.py and test_gpu_log_remap.py, and a plain-Python restatement of the two
feature-engineering scripts (feateng_tmall.py:30-133, feateng_taobao.py:16-88): their own loops over the log with
dictionaries, with "numbered in order of first appearance" where they enumerate list(set(...)).  The arrays are read-only."""
import datetime
import functools
import os

import numpy as np

from score_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCAN_TILE, SORT_TILE = _lib.TARGET_SCAN_TILE, _lib.TARGET_SORT_TILE
# event counts at the sort's tile and the scan's chunk, one below and one above each, the smallest, and three sort tiles plus one
EVENT_COUNTS = (1, 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 3 * SORT_TILE + 1)
# key widths at the sort's pass edges: 12 bits per pass, so one, two and three passes
KEY_BITS = (1, 12, 13, 24, 25, 32)
INT32_MIN = -2 ** 31


def _ro(a):
    a.setflags(write=False)
    return a


# ---- the restatements -------------------------------------------------------------------------------------------------------
def first_appearance_dict(values, remap_id):
    """value -> id, numbered from remap_id in order of first appearance; -> (dict, next remap_id)"""
    d = {}
    for v in values:
        if v not in d:
            d[v] = remap_id
            remap_id += 1
    return d, remap_id


def restate_tmall(log, age, gender):
    """feateng_tmall.preprocess_raw_data on integer rows: seven vocabularies one behind the other from 1, the two feature
    dictionaries assigned row by row (later rows overwrite), t_idx from the date.  -> dict like remap_tmall_log's, the
    dictionaries as row tables ordered by id"""
    rows = [tuple(int(x) for x in r[:6]) + (int(a), int(g)) for r, a, g in zip(np.asarray(log).tolist(), age, gender)]
    remap_id, dicts = 1, []
    for col in (0, 1, 2, 3, 4, 6, 7):                  # uid, iid, cid, sid, bid, aid, gid
        d, remap_id = first_appearance_dict([r[col] for r in rows], remap_id)
        dicts.append(d)
    ud, idd, cd, sd, bd, ad, gd = dicts
    start = datetime.date(2015, 5, 1)
    user_feat, item_feat, uid, iid, t_idx = {}, {}, [], [], []
    for u, i, c, s, b, mmdd, a, g in rows:
        item_feat[idd[i]] = [cd[c], sd[s], bd[b]]
        user_feat[ud[u]] = [ad[a], gd[g]]
        uid.append(ud[u])
        iid.append(idd[i])
        t_idx.append((datetime.date(2015, mmdd // 100, mmdd % 100) - start).days // 15)
    return dict(uid=uid, iid=iid, t_idx=t_idx, n_users=len(ud), n_items=len(idd), feature_size=remap_id,
                user_rows=[[k] + user_feat[k] for k in sorted(user_feat)], item_rows=[[k] + item_feat[k] for k in sorted(item_feat)],
                vocab_sizes=tuple(len(d) for d in dicts))


def restate_taobao(log, start_ts, end_ts, delta):
    """feateng_taobao.preprocess_raw_data on integer rows (is_pv in place of the behaviour string)"""
    kept = [(p, r) for p, r in enumerate(np.asarray(log).tolist())
            if not (r[4] < start_ts or r[4] > end_ts) and r[3] != 0]
    remap_id, dicts = 1, []
    for col in (0, 1, 2):
        d, remap_id = first_appearance_dict([r[col] for _, r in kept], remap_id)
        dicts.append(d)
    ud, idd, cd = dicts
    item_feat, uid, iid, t_idx = {}, [], [], []
    for _, (u, i, c, _, t) in kept:
        item_feat[idd[i]] = [cd[c]]
        uid.append(ud[u])
        iid.append(idd[i])
        t_idx.append((t - start_ts) // delta)
    return dict(uid=uid, iid=iid, t_idx=t_idx, n_users=len(ud), n_items=len(idd), feature_size=remap_id,
                item_rows=[[k] + item_feat[k] for k in sorted(item_feat)], user_rows=[[k] for k in sorted(ud.values())],
                vocab_sizes=tuple(len(d) for d in dicts), kept=[p for p, _ in kept])


def first_appearance_ids(cols):
    """[columns] -> ([id column per column] int32, counts): the vocabularies one behind the other from 1 (the dict rule)"""
    remap_id, ids, counts = 1, [], []
    for c in cols:
        d, nxt = first_appearance_dict(np.asarray(c).tolist(), remap_id)
        ids.append(np.asarray([d[v] for v in np.asarray(c).tolist()], dtype=np.int32))
        counts.append(nxt - remap_id)
        remap_id = nxt
    return ids, counts


def last_rows(ids, counts, entity, feats):
    """the row table of `entity` with feature columns `feats`: row id - base = [id, features of the entity's LAST event]"""
    base = 1 + sum(counts[:entity])
    rows = np.zeros((counts[entity], 1 + len(feats)), dtype=np.int32)
    for p in range(len(ids[0])):                        # (later events overwrite earlier ones)
        rows[ids[entity][p] - base] = [ids[entity][p]] + [ids[f][p] for f in feats]
    return rows


# ---- the bundled sample, the g11 log --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tmall_sample():
    return _ro(np.load(os.path.join(GOLDEN, "tmall_sample_log.npz"))["log"])


@functools.lru_cache(maxsize=None)
def g11():
    z = np.load(os.path.join(GOLDEN, "g11_taobao_remap.npz"))
    return {k: _ro(z[k]) for k in z.files}


def valid_dates_2015():
    """every MMDD of 2015 as an int64 array"""
    d, out = datetime.date(2015, 1, 1), []
    while d.year == 2015:
        out.append(d.month * 100 + d.day)
        d += datetime.timedelta(days=1)
    return np.asarray(out, dtype=np.int64)


INVALID_DATES = (229, 431, 1301, 0)


# ---- synthetic raw columns ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def raw_columns(n, key_bits, n_cols=3, seed=0):
    """n_cols raw int32 columns of n events whose patterns need exactly key_bits bits (some column holds the top bit; at 32
    bits column 0 holds -1 and INT32_MIN); vocabularies of different sizes, so runs of many lengths"""
    rng = np.random.Generator(np.random.PCG64(1000 * key_bits + 17 * n_cols + seed + n))
    cols = []
    for c in range(n_cols):
        vocab = max(1, min(1 << min(key_bits, 20), (3, 40, 700, 2, 9000, 5, 100, 64)[c % 8]))
        pat = rng.integers(0, 1 << key_bits, vocab, dtype=np.uint64).astype(np.uint32)
        if c == 0:
            pat[0] = np.uint32((1 << key_bits) - 1)                 # the widest pattern (at 32 bits: -1)
            if key_bits == 32 and vocab > 1:
                pat[1] = np.uint32(0x80000000)                      # INT32_MIN
        col = pat[rng.integers(0, vocab, n)]
        if c == 0:
            col[0] = pat[0]
            if n > 1 and vocab > 1:
                col[n - 1] = pat[1]
        cols.append(_ro(col.view(np.int32).copy()))
    return tuple(cols)


@functools.lru_cache(maxsize=None)
def taobao_log(n, mode, seed=5):
    """a synthetic Taobao-style log [n, 5] and its window: mode 'mixed', 'none' (no event kept), 'all', 'last' (only the last)"""
    rng = np.random.Generator(np.random.PCG64(seed + n))
    start, delta = 1511568000, 86400
    end = start + 9 * delta
    t = rng.integers(start - delta, end + delta, n)
    pv = (rng.integers(0, 4, n) != 0).astype(np.int64)
    if mode == "none":
        pv[:] = 0
    elif mode == "all":
        t, pv[:] = rng.integers(start, end + 1, n), 1
    elif mode == "last":
        t[:], pv[:] = start - 1, 1
        t[n - 1] = end
    log = np.stack([rng.integers(-50, 50, n), 10 ** 6 + rng.integers(0, 200, n), rng.integers(0, 12, n), pv, t], axis=1)
    return _ro(log.astype(np.int64)), start, end, delta
