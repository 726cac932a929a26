"""The raw log's remap on the device (csrc/logremap.hip, csrc/ccmr.hip): thin wrappers of score_log_remap, score_log_slices,
score_log_compact and score_ccmr_prep over int32 tensors, which dataprep.remap_tmall_log / remap_taobao_log / remap_ccmr_log
(build="device") put together.  Replaces the id numbering, the feature dictionaries and the time slices of
feateng_tmall.py:30-133, feateng_taobao.py:16-88 and feateng_ccmr.py:24-171 for a log that is uploaded once.
"""
import ctypes as C

import numpy as np

from .placement import device_of                                   # (tools take it from here)


def upload_columns(log, n_cols, dev):
    """the first n_cols columns of an integer array [n, >= n_cols] in ONE upload, as it lies in memory (no pass over it on
    the host); transposed and narrowed on the device -> (int32 tensor [n_cols, n], row c column c, each on a 256-byte
    boundary; a 0-dim int64 tensor on the device, non-zero iff a value lies outside int32 -- the caller folds it into a
    read-back it makes anyway and raises ValueError)"""
    import torch
    a = np.asarray(log)
    if a.ndim != 2 or a.shape[1] < n_cols or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("the log must be an integer array [n, >= %d]: got %s %r" % (n_cols, a.dtype, a.shape))
    if a.dtype not in (np.int32, np.int64):
        a = a.astype(np.int64)
    n = int(a.shape[0])
    raw = torch.from_numpy(np.ascontiguousarray(a)).to(dev)[:, :n_cols]
    wide = torch.zeros((), dtype=torch.int64, device=dev)
    if raw.dtype == torch.int64 and n:
        wide = ((raw.amin() < -2 ** 31) | (raw.amax() >= 2 ** 31)).to(torch.int64)
    out = torch.empty((n_cols, _pitch(n)), dtype=torch.int32, device=dev)
    out[:, :n] = raw.t()
    return out[:, :n], wide


WIDE_MESSAGE = "the device remap takes int32 columns: a value lies outside"


def _pitch(n):
    """words between two columns of one allocation: every column starts on a 256-byte boundary"""
    return (n + 63) // 64 * 64


def key_bits_of(lo, hi):
    """bits that hold the unsigned patterns of int32 values in [lo, hi]: a negative value needs all 32"""
    return 32 if lo < 0 else max(1, int(hi).bit_length())


def log_slices_tmall(mmdd, status):
    """MMDD int32 tensor -> t_idx int32 tensor; status: zeroed int32 tensor [1], set to 1 by an invalid date (no wait here)"""
    import torch
    from . import _lib
    lib, dev = _lib.load(), mmdd.device
    t_idx = torch.empty_like(mmdd)
    with torch.cuda.device(dev):
        _lib.check(lib.score_log_slices(_lib.LOG_SLICES_TMALL, mmdd.data_ptr(), None, int(mmdd.numel()), 0, 0, 0,
                                        t_idx.data_ptr(), None, status.data_ptr(), _lib.current_stream(dev)),
                   "score_log_slices (tmall)")
    return t_idx


def log_slices_epoch(ts, flag, start_ts, end_ts, delta):
    """-> (t_idx, keep) int32 tensors: keep = start_ts <= ts <= end_ts and flag != 0 (flag None: the window alone)"""
    import torch
    from . import _lib
    lib, dev = _lib.load(), ts.device
    t_idx, keep = torch.empty_like(ts), torch.empty_like(ts)
    with torch.cuda.device(dev):
        _lib.check(lib.score_log_slices(_lib.LOG_SLICES_EPOCH, ts.data_ptr(), None if flag is None else flag.data_ptr(),
                                        int(ts.numel()), int(start_ts), int(end_ts), int(delta), t_idx.data_ptr(), keep.data_ptr(),
                                        None, _lib.current_stream(dev)), "score_log_slices (epoch)")
    return t_idx, keep


def log_compact(cols, keep):
    """stable compaction of up to 8 int32 tensors [n] by keep -> ([compacted columns], kept positions int32): one wait"""
    import torch
    from . import _lib
    lib, dev = _lib.load(), keep.device
    n, k = int(keep.numel()), len(cols)
    with torch.cuda.device(dev):
        out = torch.empty((k + 1, _pitch(n)), dtype=torch.int32, device=dev)
        temp, temp_bytes = _lib.workspace("score_log_compact", dev, n)
        cin = (C.c_void_p * k)(*[c.data_ptr() for c in cols])
        cout = (C.c_void_p * k)(*[out[j].data_ptr() for j in range(k)])
        n_kept = C.c_int64(-1)
        _lib.check(lib.score_log_compact(cin, cout, k, keep.data_ptr(), n, out[k].data_ptr(), n, C.byref(n_kept),
                                         temp.data_ptr(), temp_bytes, _lib.current_stream(dev)), "score_log_compact")
        m = int(n_kept.value)
        if m:
            torch.cuda.current_stream(dev).synchronize()          # (temp is released behind this)
    return [out[j, :m] for j in range(k)], out[k, :m]


def log_remap(cols, key_bits, tables=(), download=True):
    """score_log_remap on int32 tensors [n] of one device: cols, one vocabulary each; tables: (entity column, [feature
    columns]) -> ([ids per column] int32 tensors, counts tuple, [rows per table] numpy int32 [count, 1 + features], downloaded
    once -- download=False: int32 tensors on the device).  One wait for the counts, one for the rows."""
    import torch
    from . import _lib
    lib, dev = _lib.load(), cols[0].device
    n, k = int(cols[0].numel()), len(cols)
    if n == 0 or any(int(c.numel()) != n for c in cols):
        raise ValueError("log_remap: the columns must be non-empty and of one length")
    with torch.cuda.device(dev):
        ids = torch.empty((k, _pitch(n)), dtype=torch.int32, device=dev)
        temp, temp_bytes = _lib.workspace("score_log_remap", dev, n, k)
        a = _lib.LogRemap()
        a.struct_bytes, a.n_events, a.n_cols, a.key_bits, a.n_tables = C.sizeof(_lib.LogRemap), n, k, int(key_bits), len(tables)
        for c in range(k):
            a.cols[c], a.ids[c] = cols[c].data_ptr(), ids[c].data_ptr()
        for t, (ent, feats) in enumerate(tables):
            a.tables[t].entity, a.tables[t].n_feat = int(ent), len(feats)
            for j, f in enumerate(feats):
                a.tables[t].feat[j] = int(f)
        counts = (C.c_int64 * k)()
        stream = _lib.current_stream(dev)
        _lib.check(lib.score_log_remap(C.byref(a), None, None, counts, temp.data_ptr(), temp_bytes, stream),
                   "score_log_remap (count)")
        counts = tuple(int(x) for x in counts)
        rows = []
        if tables:
            widths = [1 + len(f) for _, f in tables]
            sizes = [counts[e] * w for (e, _), w in zip(tables, widths)]
            flat = torch.empty((sum(sizes) + 4 * len(tables),), dtype=torch.int32, device=dev)
            offs, o = [], 0
            for s in sizes:                                        # every table starts on a 16-byte boundary
                offs.append(o)
                o += (s + 3) // 4 * 4
            ptrs = (C.c_void_p * len(tables))(*[flat.data_ptr() + 4 * o for o in offs])
            caps = (C.c_int64 * len(tables))(*[counts[e] for e, _ in tables])
            _lib.check(lib.score_log_remap(C.byref(a), ptrs, caps, None, temp.data_ptr(), temp_bytes, stream),
                       "score_log_remap (fill)")
            if download:
                host = flat.cpu().numpy()                          # (the one download; temp is released behind it)
                rows = [host[o:o + s].reshape(-1, w).copy() for o, s, w in zip(offs, sizes, widths)]
            else:
                torch.cuda.current_stream(dev).synchronize()      # (temp is released behind this)
                rows = [flat[o:o + s].view(-1, w) for o, s, w in zip(offs, sizes, widths)]
    return [ids[c, :n] for c in range(k)], counts, rows


def ccmr_prep(raw, movie, n_users, n_items, vocab, start_day, delta_days):
    """score_ccmr_prep on the uploaded columns: raw int32 [4, n] (user, item, rating, YYYYMMDD), movie int32 [5, m] ->
    ([uid, iid, t_idx, day, keep_pos, keep_neg] int32 tensors [n], flat int32 tensor [8 + n_items * 5]: the status words with
    the item rows behind them, so one download brings both).  No wait here."""
    import torch
    from . import _lib
    lib, dev = _lib.load(), raw.device
    n, m, I = int(raw.shape[1]), int(movie.shape[1]), int(n_items)
    with torch.cuda.device(dev):
        out = torch.empty((6, _pitch(n)), dtype=torch.int32, device=dev)
        flat = torch.empty((_lib.CCMR_STATUS_WORDS + I * 5,), dtype=torch.int32, device=dev)
        temp, temp_bytes = _lib.workspace("score_ccmr_prep", dev, m, I)
        a = _lib.CcmrPrep()
        a.struct_bytes, a.n_events, a.n_movies, a.n_users, a.n_items = C.sizeof(_lib.CcmrPrep), n, m, int(n_users), I
        a.user, a.item, a.rating, a.date = (raw[j].data_ptr() for j in range(4))
        for k in range(5):
            a.movie[k] = movie[k].data_ptr() if m else None
        for k in range(4):
            a.vocab[k] = int(vocab[k])
        a.start_day, a.delta_days = int(start_day), int(delta_days)
        a.uid, a.iid, a.t_idx, a.day, a.keep_pos, a.keep_neg = (out[j].data_ptr() for j in range(6))
        a.status, a.item_rows = flat.data_ptr(), flat.data_ptr() + 4 * _lib.CCMR_STATUS_WORDS
        _lib.check(lib.score_ccmr_prep(C.byref(a), temp.data_ptr(), temp_bytes, _lib.current_stream(dev)), "score_ccmr_prep")
    # (temp goes back to the allocator of the stream the launches are on: whatever reuses it is ordered behind them)
    return [out[j, :n] for j in range(6)], flat
