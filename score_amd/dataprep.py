"""The three offline steps between a raw Tmall behaviour log and the hot path's inputs, as far as the
cfg-1 plumbing needs them (BASELINE.json configs[0]: bundled sample -> graph store -> loader -> train/eval).
Host-side NumPy/Python, run once per dataset exactly like the reference's scripts; nothing here is on the
step path.

  remap_tmall_log      code/feateng_tmall.py:30-133   one contiguous id space starting at 1: users, items,
                                                       cats, sellers, brands, ages, genders; feature rows
  tmall_slice_index    code/feateng_tmall.py:10-11,53-56   15-day time slices counted from 2015-05-01
  gen_target_lines     code/gen_target.py:99-121       'uid,pos_iid,neg...' lines of one prediction slice

The reference enumerates each id vocabulary through ``list(set(...))`` (feateng_tmall.py:58-64), i.e. in
Python's per-process string-hash order: its remap is not reproducible from run to run.  Here every
vocabulary is numbered in order of first appearance in the log -- a valid instance of the same layout.
``user_info_format1.csv`` (age, gender per user) is missing from the reference mount; callers synthesise
it (age = uid % 9, gender = uid % 3).
"""
import datetime

import numpy as np

TMALL_START = datetime.date(2015, 5, 1)     # feateng_tmall.py:10
TMALL_SLICE_DAYS = 15                       # feateng_tmall.py:11


def tmall_slice_index(mmdd):
    """time_stamp column 'MMDD' (as int) -> 15-day slice index (feateng_tmall.py:53-56)."""
    mmdd = np.asarray(mmdd).astype(np.int64)
    out = np.empty(mmdd.shape, dtype=np.int32)
    cache = {}
    for i, v in enumerate(mmdd.reshape(-1).tolist()):
        t = cache.get(v)
        if t is None:
            t = cache[v] = (datetime.date(2015, v // 100, v % 100) - TMALL_START).days // TMALL_SLICE_DAYS
        out.reshape(-1)[i] = t
    return out


def _first_appearance(col):
    """value -> 0-based rank of its first appearance"""
    uniq, first, inv = np.unique(col, return_index=True, return_inverse=True)
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(uniq))
    return rank[inv.reshape(-1)], len(uniq)


def remap_tmall_log(log, age=None, gender=None):
    """log: int array [n, >=6] with columns user_id, item_id, cat_id, seller_id, brand_id, time_stamp(MMDD)
    (tests/golden/tmall_sample_log.npz).  age / gender: per-row arrays (the joined user profile,
    feateng_tmall.py:13-28); default = the synthesised profile uid % 9 / uid % 3.

    Returns a dict: uid, iid (remapped ids per row), t_idx, n_users, n_items, feature_size (the reference
    prints it as 'feat size', :104), user_rows [U, 3] = [uid, age_id, gender_id] and item_rows [I, 4] =
    [iid, cat_id, seller_id, brand_id] (user_feat_dict / item_feat_dict, :125-133, keyed by row order)."""
    log = np.asarray(log)
    raw_u, raw_i, raw_c, raw_s, raw_b = (log[:, j].astype(np.int64) for j in range(5))
    if age is None:
        age = raw_u % 9
    if gender is None:
        gender = raw_u % 3
    cols = [raw_u, raw_i, raw_c, raw_s, raw_b, np.asarray(age).astype(np.int64), np.asarray(gender).astype(np.int64)]
    base = 1                                         # remap_id starts at 1; 0 is the dummy node (:74)
    ids, sizes = [], []
    for c in cols:                                   # users, items, cats, sellers, brands, ages, genders (:83-103)
        r, n = _first_appearance(c)
        ids.append((r + base).astype(np.int32))
        sizes.append(n)
        base += n
    uid, iid, cid, sid, bid, aid, gid = ids
    U, I = sizes[0], sizes[1]
    user_rows = np.zeros((U, 3), dtype=np.int32)
    item_rows = np.zeros((I, 4), dtype=np.int32)
    # later rows overwrite earlier ones, as the dict assignments of :130-131 do
    user_rows[uid - 1] = np.stack([uid, aid, gid], axis=1)
    item_rows[iid - 1 - U] = np.stack([iid, cid, sid, bid], axis=1)
    return dict(uid=uid, iid=iid, t_idx=tmall_slice_index(log[:, 5]), n_users=U, n_items=I, feature_size=int(base),
                user_rows=user_rows, item_rows=item_rows, vocab_sizes=tuple(sizes))


def gen_target_lines(uid, iid, t_idx, n_users, n_items, pred_time, neg_sample_num, start_time=0, seed=11):
    """TargetGen.gen_target_file (gen_target.py:99-121) on an in-memory log: one line per user that has at
    least one interaction in slice `pred_time` AND a history in [start_time, pred_time) (user_hist_dict,
    :225-236): (uid, [pos_iid, neg...]) with pos_iid the user's FIRST item of the slice in log order and the
    negatives uniform over the item id range (gen_user_neg_items with no pop list, :88-90).  Users are
    visited in id order, as the collection scan does."""
    rng = np.random.Generator(np.random.PCG64(seed))
    uid, iid, t_idx = np.asarray(uid), np.asarray(iid), np.asarray(t_idx)
    has_hist = np.zeros(n_users + 1, dtype=bool)
    has_hist[uid[(t_idx >= start_time) & (t_idx < pred_time)]] = True
    first_pos = {}
    for u, i, t in zip(uid.tolist(), iid.tolist(), t_idx.tolist()):
        if t == pred_time and u not in first_pos:
            first_pos[u] = i
    lines = []
    for u in sorted(first_pos):
        if has_hist[u]:
            negs = rng.integers(n_users + 1, n_users + n_items + 1, neg_sample_num).tolist()
            lines.append((u, [first_pos[u]] + negs))
    return lines


# constants of the Tmall run, code/score/train_score.py:45-54,339-364 and code/graph_storage.py:39-47
TMALL = dict(obj_per_time_slice=10, time_slice_num=12, graph_time_slice_num=14, start_time=0, user_fnum=3, item_fnum=4,
             pred_time_train=9, pred_time_validation=10, pred_time_test=11, eb_dim=16, hidden_size=32,
             eval_batch_size=100, train_neg=1, test_neg=99, max_1hop=10, max_2hop=100)


def tmall_pipeline(log, seed=11, build="host", draws="stream"):
    """Raw Tmall log -> (TemporalGraph, remap dict, {'train' | 'validation' | 'test': target lines}).  Train
    lines carry 1 negative (train_score.py:18), validation / test lines 99 (:19).  build / draws: TemporalGraph.from_log's."""
    from .graph import TemporalGraph
    r = remap_tmall_log(log)
    c = TMALL
    g = TemporalGraph.from_log(r["uid"], r["iid"], r["t_idx"], r["n_users"], r["n_items"], c["graph_time_slice_num"],
                               r["user_rows"], r["item_rows"], max_1hop=c["max_1hop"], max_2hop=c["max_2hop"], seed=seed,
                               build=build, draws=draws)
    targets = {}
    for name, pt, neg in (("train", c["pred_time_train"], c["train_neg"]),
                          ("validation", c["pred_time_validation"], c["test_neg"]),
                          ("test", c["pred_time_test"], c["test_neg"])):
        targets[name] = gen_target_lines(r["uid"], r["iid"], r["t_idx"], r["n_users"], r["n_items"], pt, neg,
                                         c["start_time"], seed + pt)
    return g, r, targets


# ---- the point baselines' history files (gen_target.py:223-275, gen_history_point.py:22-65) ------------------------------------
POINT_HIST_MAX_LEN = 300                    # gen_history_point.py:12-20 (MAX_LEN_CCMR / _Taobao / _Tmall)


def point_history_lines(uid, iid, time_key, t_idx, target_lines, start_time, pred_time, hist_max_len=POINT_HIST_MAX_LEN):
    """The two history files of the point baselines as text lines (without the newline), from an in-memory log:
    TargetGen.gen_user_item_hist_dict_* (gen_target.py:223-275) followed by gen_history_point.py's gen_user_hist_seq_file /
    gen_item_hist_seq_file (:22-65), restated in plain Python -- the yardstick of PointLogStore.

    An event counts if start_time <= t_idx < pred_time (:241-244).  A user's history is the items of its events ordered by
    time_key with Python's stable sorted (:257), so events of one time stay in log order; an item's the same with the roles
    exchanged.  time_key: any non-negative integer that orders events as the reference's time_int does (Tmall: the MMDD
    column).  Line l of the user file is the last hist_max_len ids of the user of target line l (:31-32); a user without
    history makes the reference exit(1) (:36) -- here a ValueError naming the line.  Line l of the item file holds one history
    per item of target line l AS WRITTEN (all of them, not only the first 1 + neg_sample_num, :48), tab separated; an item
    without history has the history '0' (:59).

    -> (user_hist_lines, item_hist_lines)"""
    H = int(hist_max_len)
    if H <= 0:
        raise ValueError("hist_max_len must be positive")
    user_hist, item_hist = {}, {}
    for u, i, k, t in zip(np.asarray(uid).tolist(), np.asarray(iid).tolist(), np.asarray(time_key).tolist(),
                          np.asarray(t_idx).tolist()):
        if t < start_time or t >= pred_time:
            continue
        user_hist.setdefault(u, []).append((i, k))
        item_hist.setdefault(i, []).append((u, k))
    for d in (user_hist, item_hist):
        for key in d:
            d[key] = [str(x[0]) for x in sorted(d[key], key=lambda tup: tup[1])]
    user_lines, item_lines = [], []
    for l, (u, items) in enumerate(target_lines):
        if int(u) not in user_hist:
            raise ValueError("target line %d: user %d has no history in slices [%d, %d)" % (l, int(u), start_time, pred_time))
        user_lines.append(",".join(user_hist[int(u)][-H:]))
        item_lines.append("\t".join(",".join(item_hist[int(i)][-H:]) if int(i) in item_hist else "0" for i in items))
    return user_lines, item_lines


def write_point_files(directory, target_lines, user_hist_lines, item_hist_lines, user_rows, item_rows):
    """The files DataLoaderUserSeq / DataLoaderDualSeq / PointSeqStore read, written into `directory`: target.txt
    ('uid,iid,iid,...' per line), user_hist.txt, item_hist.txt and the two pickled feature dictionaries, keyed by the id as a
    string with the features that follow the id as values (feateng_tmall.py:125-133) -- plus a key '0' with zeros, the row the
    reference's loader looks up for the stand-in history of an item without one.  user_rows [U, Fu] / item_rows [I, Fi] are
    remap_tmall_log's tables (column 0 the id).  -> (target, user_hist, item_hist, user_feat_dict, item_feat_dict) paths"""
    import os
    import pickle
    os.makedirs(directory, exist_ok=True)
    paths = [os.path.join(directory, n) for n in ("target.txt", "user_hist.txt", "item_hist.txt", "user_feat_dict.pkl",
                                                  "item_feat_dict.pkl")]
    texts = (["%d,%s" % (int(u), ",".join(str(int(i)) for i in items)) for u, items in target_lines], user_hist_lines,
             item_hist_lines)
    for p, lines in zip(paths[:3], texts):
        with open(p, "w") as f:
            f.write("".join(l + "\n" for l in lines))
    for p, rows in zip(paths[3:], (user_rows, item_rows)):
        rows = np.asarray(rows)
        dct = {str(int(r[0])): [int(x) for x in r[1:]] for r in rows}
        dct["0"] = [0] * (rows.shape[1] - 1)
        with open(p, "wb") as f:
            pickle.dump(dct, f)
    return tuple(paths)


def tmall_point_stores(log, seed=11, dual=True, batch_size=None, build="device", device=None):
    """Raw Tmall log -> ({'train' | 'validation' | 'test': PointLogStore}, remap dict): the point baselines' data path on the
    log SCoRe trains from (tmall_pipeline's target lines: the same seed gives the same lines).  Train lines carry 1 negative,
    validation / test lines 99; histories are cut at the reference's 300.  batch_size: a dict per split or one number;
    default 200 for train (a multiple of 2) and TMALL's eval_batch_size for the others."""
    from .pointdata import PointLogStore
    r = remap_tmall_log(log)
    c = TMALL
    stores = {}
    for name, pt, neg in (("train", c["pred_time_train"], c["train_neg"]),
                          ("validation", c["pred_time_validation"], c["test_neg"]),
                          ("test", c["pred_time_test"], c["test_neg"])):
        lines = gen_target_lines(r["uid"], r["iid"], r["t_idx"], r["n_users"], r["n_items"], pt, neg, c["start_time"], seed + pt)
        B = batch_size.get(name) if isinstance(batch_size, dict) else batch_size
        if B is None:
            B = 200 if name == "train" else c["eval_batch_size"]
        stores[name] = PointLogStore(r["uid"], r["iid"], np.asarray(log)[:, 5], r["t_idx"], lines, c["start_time"], pt,
                                     POINT_HIST_MAX_LEN, neg, B, r["user_rows"], r["item_rows"], dual, build=build, device=device)
    return stores, r
