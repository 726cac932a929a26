"""The three offline steps between a raw Tmall behaviour log and the hot path's inputs, as far as the
cfg-1 plumbing needs them (BASELINE.json configs[0]: bundled sample -> graph store -> loader -> train/eval).
Host-side NumPy/Python, run once per dataset exactly like the reference's scripts; nothing here is on the
step path.

  remap_tmall_log      code/feateng_tmall.py:30-133   one contiguous id space starting at 1: users, items,
                                                       cats, sellers, brands, ages, genders; feature rows
  tmall_slice_index    code/feateng_tmall.py:10-11,53-56   15-day time slices counted from 2015-05-01
  gen_target_lines     code/gen_target.py:99-121       'uid,pos_iid,neg...' lines of one prediction slice
  gen_pop_items        code/gen_target.py:277-290      the popular-item list negatives may be drawn from
  sample_target_lines  code/sampling.py:31-37          1-in-N down-sampling of validation / test lines
  remap_taobao_log     code/feateng_taobao.py:16-88   the pv events of a time window; users, items, categories
  remap_ccmr_log       code/feateng_ccmr.py:24-171    positive / negative split by rating, 90-day slices, offset ids, movie rows
(targets.TargetStore.from_log(build="device") evaluates the three on the device, csrc/targetgen.hip; remap_tmall_log and
remap_taobao_log(build="device") number the ids, fill the feature rows and cut the slices there, csrc/logremap.hip;
remap_ccmr_log(build="device") in csrc/ccmr.hip.  CCMR's user_neg_dict, feateng_ccmr.py:173-183, is targets.UserNegLists.)

The reference enumerates each id vocabulary through ``list(set(...))`` (feateng_tmall.py:58-64), i.e. in
Python's per-process string-hash order: its remap is not reproducible from run to run.  Here every
vocabulary is numbered in order of first appearance in the log -- a valid instance of the same layout.
``user_info_format1.csv`` (age, gender per user) is missing from the reference mount; callers synthesise
it (age = uid % 9, gender = uid % 3).
"""
import datetime

import numpy as np

from .placement import check_build, device_i32, device_of, is_tensor, to_host

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


def remap_tmall_log(log, age=None, gender=None, build="host", device=None):
    """log: int array [n, >=6] with columns user_id, item_id, cat_id, seller_id, brand_id, time_stamp(MMDD)
    (tests/golden/tmall_sample_log.npz).  age / gender: per-row arrays (the joined user profile,
    feateng_tmall.py:13-28); default = the synthesised profile uid % 9 / uid % 3.

    Returns a dict: uid, iid (remapped ids per row), t_idx, n_users, n_items, feature_size (the reference
    prints it as 'feat size', :104), user_rows [U, 3] = [uid, age_id, gender_id] and item_rows [I, 4] =
    [iid, cat_id, seller_id, brand_id] (user_feat_dict / item_feat_dict, :125-133, keyed by row order).

    build="device" (needs a GPU): the six raw columns are uploaded once and everything is computed there
    (csrc/logremap.hip), the same integers: uid, iid and t_idx are int32 tensors on the device, a further key time_key is the
    raw MMDD column there (what PointLogStore orders histories by), and user_rows / item_rows are numpy arrays, downloaded
    once (TemporalGraph keeps its row tables on the host).  The default profile is computed from the uploaded user column.
    An invalid MMDD raises ValueError, as datetime.date does on the host."""
    check_build(build)
    if build == "device":
        return _remap_tmall_device(log, age, gender, device)
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


def _remap_tmall_device(log, age, gender, device):
    import torch
    from . import logremap as lr
    dev = device_of(device, "remap_tmall_log(build='device')")
    with torch.cuda.device(dev):
        raw, wide = lr.upload_columns(log, 6, dev)                 # [6, n]: the one upload
        n = int(raw.shape[1])
        if n == 0:
            raise ValueError("remap_tmall_log(build='device'): the log is empty")
        prof = [torch.remainder(raw[0], m).to(torch.int32) if a is None else device_i32(np.asarray(a).astype(np.int64), dev)
                for a, m in ((age, 9), (gender, 3))]
        if any(int(p.numel()) != n for p in prof):
            raise ValueError("age / gender must hold one value per log row")
        cols = [raw[j] for j in range(5)] + prof
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
        t_idx = lr.log_slices_tmall(raw[5], status)
        ext = torch.stack([torch.stack([c.amin() for c in cols]).amin().long(), torch.stack([c.amax() for c in cols]).amax().long(),
                           status[0].long(), wide]).cpu().tolist()  # one read-back: the key width (and the two status words)
        if ext[3]:
            raise ValueError(lr.WIDE_MESSAGE)
        if ext[2]:
            raise ValueError("time_stamp must be a date MMDD of 2015: month must be in 1..12, day in the month's range")
        ids, sizes, rows = lr.log_remap(cols, lr.key_bits_of(ext[0], ext[1]), tables=((0, (5, 6)), (1, (2, 3, 4))))
    return dict(uid=ids[0], iid=ids[1], t_idx=t_idx, time_key=raw[5], n_users=sizes[0], n_items=sizes[1],
                feature_size=1 + int(sum(sizes)), user_rows=rows[0], item_rows=rows[1], vocab_sizes=tuple(sizes))


TAOBAO_START_DATE, TAOBAO_END_DATE = "2017-11-25", "2017-12-04"    # feateng_taobao.py:11-12 (midnights, local time there)
TAOBAO_SLICE_SECONDS = 24 * 3600                                   # feateng_taobao.py:13


def remap_taobao_log(log, start_ts, end_ts, delta=TAOBAO_SLICE_SECONDS, build="host", device=None):
    """feateng_taobao.py:16-88 on an in-memory log: int array [n, 5] with columns user, item, category, is_pv (1 where the
    behaviour type is 'pv', else 0) and unix time.  An event is kept iff start_ts <= time <= end_ts (both inclusive: :27 drops
    `< START or > END`) and is_pv != 0 (:29); its slice is (time - start_ts) // delta (:32).  Users, items and categories of the
    KEPT events are numbered one behind the other from 1, each in order of first appearance among the kept events (the
    reference: set order, see the module header).

    start_ts / end_ts: the reference takes time.mktime of TAOBAO_START_DATE and TAOBAO_END_DATE (2017-11-25 and 2017-12-04,
    00:00), which follows the machine's time zone -- so both are parameters here (UTC: 1511568000 and 1512345600).

    Returns a dict: uid, iid, t_idx (per kept event), n_users, n_items, feature_size, item_rows [I, 2] = [iid, cid] with the
    category of the item's LAST kept event (item_feat_dict, :81), user_rows [U, 1] = [uid], vocab_sizes (users, items,
    categories) and kept, the log positions of the kept events.  build="device" (needs a GPU): one upload, then slices,
    compaction and remap on the device (csrc/logremap.hip); uid, iid, t_idx and kept are int32 tensors there, the row tables
    numpy."""
    check_build(build)
    start_ts, end_ts, delta = int(start_ts), int(end_ts), int(delta)
    if delta <= 0 or end_ts < start_ts:
        raise ValueError("remap_taobao_log: delta must be positive and end_ts >= start_ts")
    if build == "device":
        return _remap_taobao_device(log, start_ts, end_ts, delta, device)
    log = np.asarray(log)
    t = log[:, 4].astype(np.int64)
    kept = np.flatnonzero((t >= start_ts) & (t <= end_ts) & (log[:, 3] != 0))
    base = 1
    ids, sizes = [], []
    for j in range(3):                                   # users, items, categories (:48-61)
        r, n = _first_appearance(log[kept, j].astype(np.int64))
        ids.append((r + base).astype(np.int32))
        sizes.append(n)
        base += n
    uid, iid, cid = ids
    U, I = sizes[0], sizes[1]
    item_rows = np.zeros((I, 2), dtype=np.int32)
    item_rows[iid - 1 - U] = np.stack([iid, cid], axis=1)          # later events overwrite earlier ones (:81)
    return dict(uid=uid, iid=iid, t_idx=((t[kept] - start_ts) // delta).astype(np.int32), n_users=U, n_items=I,
                feature_size=int(base), item_rows=item_rows, user_rows=np.arange(1, U + 1, dtype=np.int32).reshape(U, 1),
                vocab_sizes=tuple(sizes), kept=kept)


def _remap_taobao_device(log, start_ts, end_ts, delta, device):
    import torch
    from . import logremap as lr
    dev = device_of(device, "remap_taobao_log(build='device')")
    if not -2 ** 31 <= start_ts <= end_ts < 2 ** 31:
        raise ValueError("the device remap takes int32 times: start_ts / end_ts lie outside")
    with torch.cuda.device(dev):
        raw, wide = lr.upload_columns(log, 5, dev)                 # [5, n]: the one upload
        empty = torch.empty((0,), dtype=torch.int32, device=dev)
        cols, kept = [empty] * 4, empty
        if int(raw.shape[1]):
            t_idx, keep = lr.log_slices_epoch(raw[4], raw[3], start_ts, end_ts, delta)
            cols, kept = lr.log_compact([raw[0], raw[1], raw[2], t_idx], keep)
        if int(kept.numel()) == 0:
            if int(wide):
                raise ValueError(lr.WIDE_MESSAGE)
            z = lambda w: np.zeros((0, w), dtype=np.int32)
            return dict(uid=empty, iid=empty, t_idx=empty, n_users=0, n_items=0, feature_size=1, item_rows=z(2), user_rows=z(1),
                        vocab_sizes=(0, 0, 0), kept=empty)
        ext = torch.stack([torch.stack([c.amin() for c in cols[:3]]).amin().long(),
                           torch.stack([c.amax() for c in cols[:3]]).amax().long(), wide]).cpu().tolist()   # the key width's read-back
        if ext[2]:
            raise ValueError(lr.WIDE_MESSAGE)
        ids, sizes, rows = lr.log_remap(cols[:3], lr.key_bits_of(ext[0], ext[1]), tables=((0, ()), (1, (2,))))
    return dict(uid=ids[0], iid=ids[1], t_idx=cols[3], n_users=sizes[0], n_items=sizes[1], feature_size=1 + int(sum(sizes)),
                item_rows=rows[1], user_rows=rows[0], vocab_sizes=tuple(sizes), kept=kept)


CCMR_START_DATE = 20050519        # feateng_ccmr.py:22: 1116432000 is 2005-05-19 00:00 at UTC+8
CCMR_DELTA_DAYS = 90              # feateng_ccmr.py:19
CCMR_VOCAB = (80171 + 1, 213481 + 1, 62 + 1, 1043 + 1)      # feateng_ccmr.py:13-16: directors, actors, genres, nations, each + "none"


def _ordinal(yyyymmdd):
    v = int(yyyymmdd)
    if v <= 0:
        raise ValueError("date must be a calendar date YYYYMMDD: got %d" % v)
    try:
        return datetime.date(v // 10000, v // 100 % 100, v % 100).toordinal()
    except ValueError:
        raise ValueError("date must be a calendar date YYYYMMDD: got %d" % v)


def ccmr_slice_index(day, start_day, delta_days=CCMR_DELTA_DAYS):
    """day numbers -> slice index, int((day - start_day) / delta_days): truncated TOWARDS ZERO (feateng_ccmr.py:125)"""
    d = np.asarray(day).astype(np.int64) - int(start_day)
    return (np.sign(d) * (np.abs(d) // int(delta_days))).astype(np.int32)


def _ccmr_field_ids(feat, n_users, n_items, vocab):
    """[m, 4] raw first features (-1 = empty) -> their ids (feateng_ccmr.py:150-165)"""
    out = np.empty(feat.shape, dtype=np.int64)
    base = n_users + n_items
    for k in range(4):
        out[:, k] = np.where(feat[:, k] >= 0, base + 1 + feat[:, k], base + vocab[k])
        base += vocab[k]
    return out


CCMR_ERRORS = ("date must be a calendar date YYYYMMDD", "a raw user id lies outside [0, n_users)",
               "a raw item id lies outside [0, n_items)", "movie_info: a raw item id lies outside [0, n_items)",
               "movie_info: a feature lies outside its vocabulary (-1 = empty, else 0 .. vocab - 2)",
               "%d items occur among the positive events and have no movie_info line")


def remap_ccmr_log(log, movie_info, n_users, n_items, vocab=CCMR_VOCAB, start_date=CCMR_START_DATE, delta_days=CCMR_DELTA_DAYS,
                   build="host", device=None):
    """feateng_ccmr.py's pos_neg_split, time2idx, remap_ids on an in-memory rating log.  log: int array [n, 4] with columns raw
    user, raw item, rating, date as the integer YYYYMMDD.  movie_info: int array [m, 5] with columns raw item, first director,
    first actor, first genre, first nation, -1 for an empty field (the reference keeps only the first value of a field).

    An event is positive iff its rating is 4 or 5 (:34), negative otherwise.  uid = raw + 1, iid = raw + 1 + n_users (:137).  A
    present feature f of field k gets 1 + f + n_users + n_items + sum(vocab[:k]), an empty field the LAST id of its vocabulary,
    n_users + n_items + sum(vocab[:k + 1]) (:150-165): vocab counts that "none" entry, as DIRECTOR_NUM = 80171 + 1 does.
    item_rows [n_items, 5] = [iid, did, aid, gid, nid] from the item's FIRST movie_info line (:167 -- the opposite of Tmall's
    "last event wins"); an item without a line that does not occur among the positive events gets the four "none" ids, one
    that does occur raises ValueError with the count (the reference's loader would raise KeyError).  user_rows [n_users, 1].

    t_idx = trunc((days(date) - days(start_date)) / delta_days), truncated TOWARDS ZERO as int() does at :125: a date 1 .. 89 days
    before the start lies in slice 0, one 90 or more days before it in a negative slice (the graph and target builds drop
    those).  This is time2idx, which the reference's __main__ runs; time_filter is not called there.
    start_date: the reference takes time.mktime of the date, which follows the machine's time zone, and compares it with the
    constant 1116432000 = 2005-05-19 00:00 at UTC+8; in that zone, without DST, the difference is whole days -- so the rule is
    stated in days here and the start is a parameter (YYYYMMDD).

    ValueError: an invalid calendar date; a raw id outside [0, n_users) / [0, n_items); a feature outside its vocabulary.

    Returns a dict: uid, iid, t_idx, time_key (the day number, datetime.date.toordinal()) of the positive events in log order;
    neg_uid, neg_iid of the negative events in log order (targets.UserNegLists.from_events); pos, neg: the log positions of the
    two halves; n_users, n_items, feature_size = 1 + n_users + n_items + sum(vocab), user_rows, item_rows, vocab_sizes.
    build="device" (needs a GPU): log and movie_info are uploaded once and everything is computed there (csrc/ccmr.hip, then
    score_log_compact for the two halves), the same integers; the per-event arrays are int32 tensors on the device, the row
    tables numpy, downloaded once together with the status words."""
    check_build(build)
    U, I, vocab = int(n_users), int(n_items), tuple(int(v) for v in vocab)
    delta = int(delta_days)
    if U <= 0 or I <= 0 or len(vocab) != 4 or min(vocab) < 1 or delta <= 0:
        raise ValueError("remap_ccmr_log: n_users, n_items, delta_days must be positive and vocab four sizes of at least 1")
    start_day = _ordinal(start_date)
    size = 1 + U + I + sum(vocab)
    if build == "device":
        return _remap_ccmr_device(log, movie_info, U, I, vocab, start_day, delta, size, device)
    log, mi = np.asarray(log), np.asarray(movie_info)
    if log.ndim != 2 or log.shape[1] < 4 or mi.ndim != 2 or mi.shape[1] < 5:
        raise ValueError("the log must be [n, >= 4] and movie_info [m, >= 5]: got %r and %r" % (log.shape, mi.shape))
    raw_u, raw_i, rating, date = (log[:, j].astype(np.int64) for j in range(4))
    dates, inv = np.unique(date, return_inverse=True)
    day = np.asarray([_ordinal(v) for v in dates.tolist()], dtype=np.int64)[inv.reshape(-1)]
    if ((raw_u < 0) | (raw_u >= U)).any():
        raise ValueError(CCMR_ERRORS[1])
    if ((raw_i < 0) | (raw_i >= I)).any():
        raise ValueError(CCMR_ERRORS[2])
    m_item, feat = mi[:, 0].astype(np.int64), mi[:, 1:5].astype(np.int64)
    if ((m_item < 0) | (m_item >= I)).any():
        raise ValueError(CCMR_ERRORS[3])
    if ((feat < -1) | (feat >= np.asarray(vocab) - 1)).any():
        raise ValueError(CCMR_ERRORS[4])
    is_pos = (rating == 4) | (rating == 5)
    pos, neg = np.flatnonzero(is_pos), np.flatnonzero(~is_pos)
    item_rows = np.empty((I, 5), dtype=np.int64)
    item_rows[:, 0] = np.arange(U + 1, U + I + 1)
    item_rows[:, 1:] = _ccmr_field_ids(np.full((1, 4), -1, dtype=np.int64), U, I, vocab)
    has_line = np.zeros(I, dtype=bool)
    lined, first = np.unique(m_item, return_index=True)            # (the first line of an item: :167)
    item_rows[lined, 1:] = _ccmr_field_ids(feat[first], U, I, vocab)
    has_line[lined] = True
    missing = int((~has_line[np.unique(raw_i[pos])]).sum())
    if missing:
        raise ValueError(CCMR_ERRORS[5] % missing)
    uid, iid = (raw_u + 1).astype(np.int32), (raw_i + 1 + U).astype(np.int32)
    return dict(uid=uid[pos], iid=iid[pos], t_idx=ccmr_slice_index(day[pos], start_day, delta), time_key=day[pos].astype(np.int32),
                neg_uid=uid[neg], neg_iid=iid[neg], pos=pos, neg=neg, n_users=U, n_items=I, feature_size=size,
                user_rows=np.arange(1, U + 1, dtype=np.int32).reshape(U, 1), item_rows=item_rows.astype(np.int32),
                vocab_sizes=(U, I) + vocab)


def _remap_ccmr_device(log, movie_info, U, I, vocab, start_day, delta, size, device):
    import torch
    from . import _lib
    from . import logremap as lr
    dev = device_of(device, "remap_ccmr_log(build='device')")
    if size >= 2 ** 31:
        raise ValueError("the device remap takes int32 ids: feature_size %d lies outside" % size)
    with torch.cuda.device(dev):
        raw, wide = lr.upload_columns(log, 4, dev)                 # [4, n] and [5, m]: the two uploads
        movie, wide_m = lr.upload_columns(movie_info, 5, dev)
        if int(raw.shape[1]) == 0:
            raise ValueError("remap_ccmr_log(build='device'): the log is empty")
        cols, flat = lr.ccmr_prep(raw, movie, U, I, vocab, start_day, delta)
        host = torch.cat([torch.stack([wide, wide_m]).to(torch.int32), flat]).cpu().numpy()     # the one download
        if host[0] or host[1]:
            raise ValueError(lr.WIDE_MESSAGE)
        status = host[2:2 + _lib.CCMR_STATUS_WORDS]
        for k in range(5):
            if status[k]:
                raise ValueError(CCMR_ERRORS[k])
        if status[_lib.CCMR_ST_MISSING]:
            raise ValueError(CCMR_ERRORS[5] % int(status[_lib.CCMR_ST_MISSING]))
        item_rows = host[2 + _lib.CCMR_STATUS_WORDS:].reshape(I, 5).copy()
        (uid, iid, t_idx, day), pos = lr.log_compact(cols[:4], cols[4])
        (neg_uid, neg_iid), neg = lr.log_compact(cols[:2], cols[5])
    return dict(uid=uid, iid=iid, t_idx=t_idx, time_key=day, neg_uid=neg_uid, neg_iid=neg_iid, pos=pos, neg=neg, n_users=U,
                n_items=I, feature_size=size, user_rows=np.arange(1, U + 1, dtype=np.int32).reshape(U, 1), item_rows=item_rows,
                vocab_sizes=(U, I) + vocab)


TAG_TARGET_NEG, TAG_TARGET_POP, TAG_TARGET_SAMPLE = 4, 5, 6      # next to graph.TAG_*: the cell of a draw is the line's user id


def _target_heads(uid, iid, t_idx, n_users, n_items, pred_time, start_time):
    """draws="cell": (users that get a line, ascending; their positives).  Events with a uid or iid outside its range or a
    negative slice are dropped, as TemporalGraph.from_log(draws="cell") drops them."""
    uid, iid, t_idx = (np.asarray(a).astype(np.int64).ravel() for a in (uid, iid, t_idx))
    ok = (uid >= 1) & (uid <= n_users) & (iid >= n_users + 1) & (iid <= n_users + n_items) & (t_idx >= 0)
    uid, iid, t_idx = uid[ok], iid[ok], t_idx[ok]
    has_hist = np.zeros(n_users + 1, dtype=bool)
    has_hist[uid[(t_idx >= start_time) & (t_idx < pred_time)]] = True
    at = np.flatnonzero(t_idx == pred_time)
    users, first = np.unique(uid[at], return_index=True)         # (the first occurrence: the first event in log order)
    keep = has_hist[users]
    return users[keep], iid[at[first[keep]]]


def gen_target_lines(uid, iid, t_idx, n_users, n_items, pred_time, neg_sample_num, start_time=0, seed=11, draws="stream",
                     pop_items=None, neg_lists=None):
    """TargetGen.gen_target_file (gen_target.py:99-121) on an in-memory log: one line per user that has at
    least one interaction in slice `pred_time` AND a history in [start_time, pred_time) (user_hist_dict,
    :225-236): (uid, [pos_iid, neg...]) with pos_iid the user's FIRST item of the slice in log order and the
    negatives uniform over the item id range (gen_user_neg_items with no pop list, :88-90).  Users are
    visited in id order, as the collection scan does.

    pop_items: the popular-item list (gen_pop_items; the Taobao run's mode, gen_target.py:92-96): every negative is an entry
      of it, uniform over its positions.  An empty list with at least one eligible user raises ValueError (the reference's
      random.randint(0, -1) raises there too).  (targets.TargetStore.from_log, which folds the down-sampling in, raises only
      if a line is left after it.)
    draws: "stream" (the default) takes the negatives from ONE sequential PCG64 stream, rng.integers per eligible user -- with
      a pop list rng.integers(0, len(pop)) --; "cell" takes negative j of user u from the counter rule of graph._cell_keys,
      lo + ((key(seed, tag, u, j) * n) >> 32) in 64-bit arithmetic: lo = n_users + 1, n = n_items, tag TAG_TARGET_NEG without a
      pop list, pop_items[(key * len(pop)) >> 32], tag TAG_TARGET_POP with one.  No line depends on another, which is what
      csrc/targetgen.hip evaluates on the device; events with an id outside its range or a negative slice are dropped.
      Eligibility, the positive and the line order are the same under both rules.
    neg_lists: a targets.UserNegLists, CCMR's user_neg_dict (gen_target.py:79-96): negative j of user u (j = 0-based position
      among the line's negatives) is the user's own j-th negatively rated item, in file order, where the list is that long;
      only the rest is drawn.  "cell": the draw the rule above makes at position j, same tag and j -- so empty lists give the
      lines of neg_lists=None word for word, and under one seed a user's padding is the same for every pred_time (what the
      reference does by accident: gen_user_neg_items appends its pads to the list INSIDE the dict, :89-95, and one TargetGen
      writes target_40, _39, _38, :309-311).  "stream" (host only): the neg_sample_num - len missing values of each eligible
      user come from the one PCG64 stream, in line order, and are APPENDED to the user's list in neg_lists -- the object is
      mutated, as the reference's dict is, so a second split sees them.  As there, this holds for a user that HAS an entry: for
      a user without one the reference pads a fresh [] that it never stores (:82-83), so such a user is drawn anew in every
      split.  Eligibility, the positive and the line order do not change."""
    if draws not in ("stream", "cell"):
        raise ValueError("draws is 'stream' or 'cell': got %r" % (draws,))
    pop = None if pop_items is None else np.asarray(pop_items).astype(np.int64).ravel()
    if neg_lists is not None and neg_lists.n_users != int(n_users):
        raise ValueError("neg_lists is over %d users, the log over %d" % (neg_lists.n_users, int(n_users)))
    if draws == "cell":
        from .graph import _cell_keys
        users, pos = _target_heads(uid, iid, t_idx, int(n_users), int(n_items), pred_time, start_time)
        if pop is not None and len(pop) == 0 and len(users):
            raise ValueError("pop_items is empty and %d users are eligible" % len(users))
        neg = int(neg_sample_num)
        key = _cell_keys(seed, TAG_TARGET_NEG if pop is None else TAG_TARGET_POP, np.repeat(users, neg),
                         np.tile(np.arange(neg, dtype=np.int64), len(users))).astype(np.uint64).reshape(len(users), neg)
        if pop is None:
            negs = n_users + 1 + ((key * np.uint64(n_items)) >> np.uint64(32)).astype(np.int64)
        else:
            negs = pop[((key * np.uint64(len(pop))) >> np.uint64(32)).astype(np.int64)] if len(users) else key.astype(np.int64)
        if neg_lists is not None and len(users) and neg:
            off, items = neg_lists.arrays()
            if len(items):
                j = np.arange(neg, dtype=np.int64)[None, :]
                own = j < (off[users] - off[users - 1])[:, None]
                negs = np.where(own, items[np.minimum(off[users - 1][:, None] + j, len(items) - 1)], negs)
        return [(int(u), [int(p)] + row) for u, p, row in zip(users.tolist(), pos.tolist(), negs.tolist())]
    if neg_lists is not None and neg_lists.on_device:
        raise ValueError("draws='stream' exists on the host only: neg_lists lives on the device")
    own_lists, pads = {} if neg_lists is None else neg_lists.lists(), {}
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
            own = own_lists.get(u, [])
            need = neg_sample_num - len(own) if own else neg_sample_num
            if pop is not None and len(pop) == 0:
                raise ValueError("pop_items is empty and user %d is eligible" % u)
            if need <= 0 and own:
                negs = own[:neg_sample_num]
            elif pop is None:
                negs = own + rng.integers(n_users + 1, n_users + n_items + 1, need).tolist()
            else:
                negs = own + pop[rng.integers(0, len(pop), need)].tolist()
            if own and len(negs) > len(own):                    # (a user without an entry: the reference's fresh [] is not kept)
                pads[u] = negs[len(own):]
            lines.append((u, [first_pos[u]] + negs))
    if pads:
        neg_lists._append(pads)
    return lines


def gen_pop_items(graph, pop_standard, max_iid=None):
    """TargetGen.gen_pop_items (gen_target.py:277-290): the item ids, ascending, with at least `pop_standard` non-empty
    slices among the graph's S and iid <= max_iid (default: all).  Reads the item side's off1.  -> int32 array"""
    off1 = np.asarray(graph.item_csr["off1"]).astype(np.int64)
    nonempty = (np.diff(off1) > 0).reshape(graph.I, graph.S).sum(axis=1)
    ids = np.arange(graph.U + 1, graph.U + graph.I + 1, dtype=np.int64)
    keep = nonempty >= int(pop_standard)
    if max_iid is not None:
        keep &= ids <= int(max_iid)
    return ids[keep].astype(np.int32)


def sample_target_lines(lines, sample_factor, seed=11, draws="stream"):
    """sampling.py:31-37, the 1-in-N down-sampling of validation / test lines.  "stream": line l stays iff
    rng.integers(1, sample_factor + 1) == 1, drawn in line order from one PCG64 stream; "cell": iff
    (key(seed, TAG_TARGET_SAMPLE, uid, 0) * sample_factor) >> 32 == 0 -- a line's fate depends on its user alone.
    Factor 1 keeps every line; a factor below 1 raises ValueError."""
    f = int(sample_factor)
    if f < 1:
        raise ValueError("sample_factor must be at least 1: got %r" % (sample_factor,))
    if draws not in ("stream", "cell"):
        raise ValueError("draws is 'stream' or 'cell': got %r" % (draws,))
    lines = list(lines)
    if f == 1 or not lines:
        return lines
    if draws == "cell":
        keep = target_sample_keep([int(l[0]) for l in lines], f, seed)
    else:
        rng = np.random.Generator(np.random.PCG64(seed))
        keep = [int(rng.integers(1, f + 1)) == 1 for _ in lines]
    return [l for l, k in zip(lines, keep) if k]


def target_sample_keep(users, sample_factor, seed):
    """the "cell" sample rule on an array of user ids -> bool array"""
    from .graph import _cell_keys
    users = np.asarray(users, dtype=np.int64)
    key = _cell_keys(seed, TAG_TARGET_SAMPLE, users, np.zeros(len(users), dtype=np.int64)).astype(np.uint64)
    return ((key * np.uint64(int(sample_factor))) >> np.uint64(32)) == 0


# constants of the Tmall run, code/score/train_score.py:45-54,339-364 and code/graph_storage.py:39-47
TMALL = dict(obj_per_time_slice=10, time_slice_num=12, graph_time_slice_num=14, start_time=0, user_fnum=3, item_fnum=4,
             pred_time_train=9, pred_time_validation=10, pred_time_test=11, eb_dim=16, hidden_size=32,
             eval_batch_size=100, train_neg=1, test_neg=99, max_1hop=10, max_2hop=100)


TMALL_SPLITS = (("train", "pred_time_train", "train_neg"), ("validation", "pred_time_validation", "test_neg"),
                ("test", "pred_time_test", "test_neg"))


def _split_factor(sample_factor, name):
    """sample_factor= of the pipelines: one number for validation and test, or a dict per split; never the train split"""
    if isinstance(sample_factor, dict):
        return sample_factor.get(name)
    return None if name == "train" else sample_factor


def _check_targets(targets, draws, sample_factor):
    if targets not in ("host", "device"):
        raise ValueError("targets is 'host' or 'device': got %r" % (targets,))
    if targets == "device" and draws != "cell":
        raise ValueError("targets='device' needs draws='cell': the sequential stream of draws='stream' has no device form")
    if targets == "host" and sample_factor is not None:
        raise ValueError("sample_factor= needs targets='device' (sample_target_lines down-samples host lines)")


def _check_remap(remap, build):
    if remap not in ("host", "device"):
        raise ValueError("remap is 'host' or 'device': got %r" % (remap,))
    if remap == "device" and build != "device":
        raise ValueError("remap='device' needs build='device': its columns are born on the device and stay there")


class _LogFront(object):
    """A remap dict's per-event columns where the pipeline's stages want them, every copy made when first asked for and once:
    host() is numpy (a download where the remap ran on the device; the dict's very arrays where it did not), device() int32
    tensors (an upload where the remap ran on the host, RuntimeError without a GPU; the dict's very tensors where it did
    not).  names: uid, iid, t_idx by default; time_key is the dict's where the remap returns one and column 5 of the raw log
    for Tmall's host remap, which does not -- this is the one place that knows."""
    LOG, LOG4 = ("uid", "iid", "t_idx"), ("uid", "iid", "time_key", "t_idx")

    def __init__(self, r, targets, device=None, raw_log=None):
        self.r, self.targets, self.device_arg, self._raw_log = r, targets, device, raw_log
        self._host, self._dev, self._upload_to, self._neg_lists = {}, {}, None, None

    def _column(self, k):
        if k == "time_key" and k not in self.r:
            return np.asarray(self._raw_log)[:, 5]
        return self.r[k]

    def host(self, names=LOG):
        for k in names:
            if k not in self._host:
                self._host[k] = to_host(self._column(k))
        return tuple(self._host[k] for k in names)

    def device(self, names=LOG):
        for k in names:
            if k not in self._dev:
                a = self._column(k)
                if not is_tensor(a):
                    if self._upload_to is None:
                        self._upload_to = device_of(self.device_arg, "targets='device'", instead="targets='host' does not")
                    a = device_i32(a, self._upload_to)
                self._dev[k] = a
        return tuple(self._dev[k] for k in names)

    def stage(self, build, names=LOG):
        """the columns for a stage that runs where `build` says.  A device stage shares the copy that is on the device anyway
        -- the remap's own, or the upload the device targets make: one upload serves the graph, the lines and the histories --;
        every other stage takes the host arrays, which a device stage uploads itself."""
        shared = build == "device" and (self.targets == "device" or is_tensor(self.r["uid"]))
        return self.device(names) if shared else self.host(names)

    def neg_lists(self):
        """CCMR's user_neg_dict from the remap's negative events, built where the targets are"""
        if self._neg_lists is None:
            from .targets import UserNegLists
            r = self.r
            self._neg_lists = UserNegLists.from_events(r["neg_uid"], r["neg_iid"], r["n_users"], build=self.targets,
                                                       device=self.device_arg)
        return self._neg_lists


def _graph_of(front, c, seed, build, draws):
    from .graph import TemporalGraph
    r = front.r
    return TemporalGraph.from_log(*front.stage(build), r["n_users"], r["n_items"], c["graph_time_slice_num"], r["user_rows"],
                                  r["item_rows"], max_1hop=c["max_1hop"], max_2hop=c["max_2hop"], seed=seed, build=build,
                                  draws=draws)


def _split_lines(front, c, splits, seed_of, draws, sample_factor, neg_lists=False, store=None):
    """{split: its target lines} over `splits` (name, key of the prediction time, key of the negatives' number in the data
    set's constants c) IN THAT ORDER, which matters under draws="stream".  seed_of(pred_time): the split's seed.  Device
    targets are TargetStore objects built from the front's device columns, host targets gen_target_lines of its host columns;
    neg_lists: with the front's negative lists (CCMR).  store(name, pred_time, neg, lines): what the dict holds instead."""
    from .targets import TargetStore
    r, out = front.r, {}
    for name, pt, neg in splits:
        pt, neg = c[pt], c[neg]
        cols = front.device() if front.targets == "device" else front.host()
        own = front.neg_lists() if neg_lists else None
        if front.targets == "device":
            lines = TargetStore.from_log(*cols, r["n_users"], r["n_items"], pt, neg, c["start_time"], seed_of(pt), build="device",
                                         sample_factor=_split_factor(sample_factor, name), neg_lists=own)
        else:
            lines = gen_target_lines(*cols, r["n_users"], r["n_items"], pt, neg, c["start_time"], seed_of(pt), draws=draws,
                                     neg_lists=own)
        out[name] = lines if store is None else store(name, pt, neg, lines)
    return out


def _point_store_of(front, c, batch_size, dual, build):
    """_split_lines' store=: the PointLogStore of a split's lines.  batch_size: a dict per split or one number; default 200
    for train and the data set's eval_batch_size for the others."""
    from .pointdata import PointLogStore
    r = front.r

    def store(name, pt, neg, lines):
        B = batch_size.get(name) if isinstance(batch_size, dict) else batch_size
        if B is None:
            B = 200 if name == "train" else c["eval_batch_size"]
        uid, iid, time_key, t_idx = front.stage(build, front.LOG4)
        return PointLogStore(uid, iid, time_key, t_idx, lines, c["start_time"], pt, POINT_HIST_MAX_LEN, neg, B, r["user_rows"],
                             r["item_rows"], dual, build=build, device=front.device_arg)
    return store


def tmall_pipeline(log, seed=11, build="host", draws="stream", targets="host", sample_factor=None, remap="host"):
    """Raw Tmall log -> (TemporalGraph, remap dict, {'train' | 'validation' | 'test': target lines}).  Train
    lines carry 1 negative (train_score.py:18), validation / test lines 99 (:19).  build / draws: TemporalGraph.from_log's.
    targets: "host" (the default) gen_target_lines with the same draws; "device" (needs a GPU and draws="cell") the log is
    uploaded once and the dict holds targets.TargetStore objects built from it (csrc/targetgen.hip), which the loaders take in
    place of lines; sample_factor (one number, or a dict per split) then down-samples the validation / test lines as
    sampling.py does.  remap: "host" (the default) remap_tmall_log in numpy; "device" (needs build="device") the RAW log is
    uploaded once, remapped there (csrc/logremap.hip), and the graph and the targets are built from those columns -- the dict
    then holds device tensors under uid / iid / t_idx / time_key."""
    _check_targets(targets, draws, sample_factor)
    _check_remap(remap, build)
    front = _LogFront(remap_tmall_log(log, build=remap), targets)
    g = _graph_of(front, TMALL, seed, build, draws)
    return g, front.r, _split_lines(front, TMALL, TMALL_SPLITS, lambda pt: seed + pt, draws, sample_factor)


# constants of the CCMR run: graph_storage.py:16-25 (41 graph slices, caps 10 / 100), gen_target.py:14-23,309-311 (start index 0,
# splits at prediction times 38 / 39 / 40, all three files with NEG_SAMPLE_NUM = 99 negatives), train_score.py:23-32,285-310
CCMR = dict(obj_per_time_slice=10, time_slice_num=41, graph_time_slice_num=41, start_time=0, user_fnum=1, item_fnum=5,
            pred_time_train=38, pred_time_validation=39, pred_time_test=40, eb_dim=16, hidden_size=32, eval_batch_size=100,
            train_neg=99, test_neg=99, max_1hop=10, max_2hop=100, start_date=CCMR_START_DATE, delta_days=CCMR_DELTA_DAYS)


# the reference's order: target_40, _39, _38 on ONE TargetGen (gen_target.py:309-311) -- it matters under draws="stream"
CCMR_SPLITS = (("test", "pred_time_test", "test_neg"), ("validation", "pred_time_validation", "test_neg"),
               ("train", "pred_time_train", "train_neg"))


def ccmr_pipeline(log, movie_info, n_users, n_items, vocab=CCMR_VOCAB, seed=11, build="host", draws="stream", targets="host",
                  sample_factor=None, remap="host"):
    """Raw CCMR rating log (remap_ccmr_log's log and movie_info) -> (TemporalGraph, remap dict, {'train' | 'validation' |
    'test': target lines or TargetStore}), the shape of tmall_pipeline.  The graph is built from the POSITIVE events; a line's
    negatives are the user's own negatively rated items first (the remap dict's neg_uid / neg_iid as a targets.UserNegLists),
    draws only behind them (gen_target_lines' neg_lists).  All three splits carry 99 negatives and use ONE seed -- not
    tmall_pipeline's seed + pt --, so that under draws="cell" a user's padding is the same in every split, which is what the
    reference's one TargetGen does; under draws="stream" the splits are generated in the reference's order, test first, from
    one stream per call with the pads carried along in the lists.  build / draws / targets / sample_factor / remap:
    tmall_pipeline's."""
    _check_targets(targets, draws, sample_factor)
    _check_remap(remap, build)
    front = _LogFront(remap_ccmr_log(log, movie_info, n_users, n_items, vocab, CCMR["start_date"], CCMR["delta_days"], build=remap),
                      targets)
    g = _graph_of(front, CCMR, seed, build, draws)
    return g, front.r, _split_lines(front, CCMR, CCMR_SPLITS, lambda pt: seed, draws, sample_factor, neg_lists=True)


def ccmr_point_stores(log, movie_info, n_users, n_items, vocab=CCMR_VOCAB, seed=11, dual=True, batch_size=None, build="device",
                      device=None, targets="host", draws="stream", sample_factor=None, remap="host"):
    """Raw CCMR rating log -> ({'train' | 'validation' | 'test': PointLogStore}, remap dict), like tmall_point_stores, on
    ccmr_pipeline's lines (the same seed, draws and targets give the same lines).  Histories are ordered by (entity, day),
    stable in log order -- gen_user_item_hist_dict_ccmr's stable sorted on time_int (gen_target.py:149-152) --, which is what
    PointLogStore does with the remap's time_key, and cut at the reference's 300.  batch_size: a dict per split or one number;
    default 200 for train and CCMR's eval_batch_size for the others (multiples of 1 + 99)."""
    _check_targets(targets, draws, sample_factor)
    _check_remap(remap, build)
    front = _LogFront(remap_ccmr_log(log, movie_info, n_users, n_items, vocab, CCMR["start_date"], CCMR["delta_days"], build=remap,
                                     device=device), targets, device)
    return _split_lines(front, CCMR, CCMR_SPLITS, lambda pt: seed, draws, sample_factor, neg_lists=True,
                        store=_point_store_of(front, CCMR, batch_size, dual, build)), front.r


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


def tmall_point_stores(log, seed=11, dual=True, batch_size=None, build="device", device=None, targets="host", draws="stream",
                       sample_factor=None, remap="host"):
    """Raw Tmall log -> ({'train' | 'validation' | 'test': PointLogStore}, remap dict): the point baselines' data path on the
    log SCoRe trains from (tmall_pipeline's target lines: the same seed, draws and targets give the same lines).  Train lines
    carry 1 negative, validation / test lines 99; histories are cut at the reference's 300.  batch_size: a dict per split or
    one number; default 200 for train (a multiple of 2) and TMALL's eval_batch_size for the others.  targets / draws /
    sample_factor: tmall_pipeline's -- with targets="device" the lines are built on the device and handed over as tensors.
    remap: tmall_pipeline's -- with remap="device" (needs build="device") the raw log is uploaded once and the remap's device
    columns, time_key among them, serve the lines and the histories."""
    _check_targets(targets, draws, sample_factor)
    _check_remap(remap, build)
    front = _LogFront(remap_tmall_log(log, build=remap, device=device), targets, device, raw_log=log)
    return _split_lines(front, TMALL, TMALL_SPLITS, lambda pt: seed + pt, draws, sample_factor,
                        store=_point_store_of(front, TMALL, batch_size, dual, build)), front.r
