"""The point models' data loader (the reference's point_models/data_loader.py:15-87, DataLoaderUserSeq): a target file, a
file of flat user histories and two optional feature dictionaries -> the 5-tuple score_amd.model.GRU4Rec trains on,

    (user_seq [B, max_len, Fi], user_seq_length [B], target_user [B, Fu], target_item [B, Fi], label [B])

as int32 arrays holding exactly the values of the reference's nested lists.  Its habits are kept, because a model trained
through it must see the same batches:

* a batch is batch_size / (1 + neg_sample_num) target lines; line i of the target file goes with line i of the history
  file; every target line contributes 1 + neg_sample_num samples -- its positive item first (label 1), then its
  negatives (label 0) -- which all share the line's user and history;
* a target line is "uid,iid,neg,neg,...": only the first 1 + neg_sample_num items are used;
* a history shorter than max_len is padded by REPEATING ITS LAST ITEM (not with 0), a longer one keeps its last max_len
  items; the reported length is the untruncated one (so it may exceed max_len: the model treats that as max_len);
* a line's last character is dropped unseen (the newline -- or, in a file that does not end with one, the last digit);
* feature dictionaries are pickled dicts keyed by the id AS A STRING, values the feature ids that follow the id itself;
* a target file that ends inside a batch drops that partial batch.

batch_size % (1 + neg_sample_num) != 0 raises ValueError (the reference prints and exits).

DataLoaderDualSeq (data_loader.py:89-185) adds a third file, the item histories: line i holds one user sequence per item of
target line i -- the positive's first, then each negative's --, sequences separated by tabs, ids by commas; each is padded /
truncated like the user history and reported with its untruncated length.  It yields the 7-tuple score_amd.model.DELF trains on,

    (user_seq [B, max_len, Fi], user_seq_length [B], item_seq [B, max_len, Fu], item_seq_length [B], target_user [B, Fu],
     target_item [B, Fi], label [B]).

PointSeqStore parses the same files once into flat arrays that live on the device, and DeviceDataLoaderUserSeq /
DeviceDataLoaderDualSeq -- the same constructors -- assemble every batch from them in one kernel launch (csrc/pointloader.hip):
the same batches, as device tensors.

PointLogStore holds what those files are made from instead -- one history per user and per item, built from the remapped
interaction log on the device (csrc/pointhist.hip) or in numpy -- and the same two device loaders take it as `store=`: the
batches of the reference's whole chain (history dictionaries -> history files -> loader) without writing a file."""
import pickle

import numpy as np

from .placement import NO_CPU_PATH, check_build, device_as, device_i32, device_of, is_tensor, to_host, upload_named


class DataLoaderUserSeq(object):
    def __init__(self, batch_size, max_len, target_file, user_seq_file, neg_sample_num, user_feat_dict_file,
                 item_feat_dict_file):
        self.batch_size, self.max_len, self.neg_sample_num = int(batch_size), int(max_len), int(neg_sample_num)
        per_line = 1 + self.neg_sample_num
        if self.batch_size % per_line != 0:
            raise ValueError("batch size should be a multiple of %d (1 + neg_sample_num)" % per_line)
        self.lines_per_batch = self.batch_size // per_line
        self.target_f = open(target_file)
        self.user_seq_f = open(user_seq_file)
        self.user_feat_dict = self._load(user_feat_dict_file)
        self.item_feat_dict = self._load(item_feat_dict_file)
        self._item_rows = {}        # item id (str) -> its feature row [Fi], built on first use

    @staticmethod
    def _load(path):
        if path is None:
            return None
        with open(path, "rb") as f:
            return pickle.load(f)

    def _item_row(self, key):
        row = self._item_rows.get(key)
        if row is None:
            row = [int(key)] + (list(self.item_feat_dict[key]) if self.item_feat_dict is not None else [])
            self._item_rows[key] = row = np.asarray(row, dtype=np.int32)
        return row

    def _user_row(self, uid):
        return [int(uid)] + (list(self.user_feat_dict[uid]) if self.user_feat_dict is not None else [])

    def close(self):
        self.target_f.close()
        self.user_seq_f.close()

    def __iter__(self):
        return self

    def __next__(self):
        per_line, L = 1 + self.neg_sample_num, self.max_len
        seqs, lens, users, items, labels = [], [], [], [], []
        for _ in range(self.lines_per_batch):
            target_line = self.target_f.readline()
            if target_line == "":
                raise StopIteration
            fields = target_line[:-1].split(",")
            uid, iids = fields[0], fields[1:1 + per_line]
            hist = self.user_seq_f.readline()[:-1].split(",")
            n = len(hist)
            kept = [str(int(i)) for i in (hist[-L:] if n >= L else hist + [hist[-1]] * (L - n))]
            seq = np.stack([self._item_row(k) for k in kept])            # [max_len, Fi]
            urow = self._user_row(uid)
            for j, iid in enumerate(iids):
                labels.append(1 if j == 0 else 0)
                seqs.append(seq)
                lens.append(n)
                users.append(urow)
                items.append(self._item_row(iid))
        return (np.stack(seqs).astype(np.int32, copy=False), np.asarray(lens, dtype=np.int32),
                np.asarray(users, dtype=np.int32), np.stack(items).astype(np.int32, copy=False), np.asarray(labels, dtype=np.int32))

    next = __next__


class DataLoaderDualSeq(DataLoaderUserSeq):
    """data_loader.py:89-185 as it is.  Its loop `for uid in seq` rebinds `uid`, so a line's target_user rows are built from the
    LAST user id of the line's LAST item sequence (as written in the file, before padding or truncation), not from the target
    line's user; that is reproduced."""

    def __init__(self, batch_size, max_len, target_file, user_seq_file, item_seq_file, neg_sample_num, user_feat_dict_file,
                 item_feat_dict_file):
        DataLoaderUserSeq.__init__(self, batch_size, max_len, target_file, user_seq_file, neg_sample_num, user_feat_dict_file,
                                   item_feat_dict_file)
        self.item_seq_f = open(item_seq_file)
        self._user_rows = {}        # user id (str(int)) -> its feature row [Fu], built on first use

    def _user_seq_row(self, key):
        row = self._user_rows.get(key)
        if row is None:
            row = [int(key)] + (list(self.user_feat_dict[key]) if self.user_feat_dict is not None else [])
            self._user_rows[key] = row = np.asarray(row, dtype=np.int32)
        return row

    def close(self):
        DataLoaderUserSeq.close(self)
        self.item_seq_f.close()

    def _padded(self, hist):
        """the last max_len ids of a history, or the history padded by repeating its last id, as str(int(id)) keys"""
        L, n = self.max_len, len(hist)
        return [str(int(i)) for i in (hist[-L:] if n >= L else hist + [hist[-1]] * (L - n))]

    def __next__(self):
        per_line = 1 + self.neg_sample_num
        useqs, ulens, iseqs, ilens, users, items, labels = [], [], [], [], [], [], []
        for _ in range(self.lines_per_batch):
            target_line = self.target_f.readline()
            if target_line == "":
                raise StopIteration
            fields = target_line[:-1].split(",")
            uid, iids = fields[0], fields[1:1 + per_line]
            hist = self.user_seq_f.readline()[:-1].split(",")
            item_hists = [h.split(",") for h in self.item_seq_f.readline()[:-1].split("\t")]
            useq = np.stack([self._item_row(k) for k in self._padded(hist)])                    # [max_len, Fi]
            item_seqs = [np.stack([self._user_seq_row(k) for k in self._padded(h)]) for h in item_hists]      # each [max_len, Fu]
            for h in item_hists:       # (the reference's rebinding of `uid`: the last id of the last sequence read)
                for u in h:
                    uid = u
            urow = self._user_row(uid)
            for j, iid in enumerate(iids):
                labels.append(1 if j == 0 else 0)
                users.append(urow)
                items.append(self._item_row(iid))
                ulens.append(len(hist))
                useqs.append(useq)
                ilens.append(len(item_hists[j]))
                iseqs.append(item_seqs[j])
        i32 = np.int32
        return (np.stack(useqs).astype(i32, copy=False), np.asarray(ulens, dtype=i32), np.stack(iseqs).astype(i32, copy=False),
                np.asarray(ilens, dtype=i32), np.asarray(users, dtype=i32), np.stack(items).astype(i32, copy=False),
                np.asarray(labels, dtype=i32))

    next = __next__


# ---- the same batches from a device-resident store ------------------------------------------------------------------------
class PointSeqStore(object):
    """The files of DataLoaderUserSeq / DataLoaderDualSeq parsed ONCE on the host into flat integer arrays that
    `.to_device()` uploads; csrc/pointloader.hip then assembles a batch from them in one launch (DeviceDataLoaderUserSeq /
    DeviceDataLoaderDualSeq below).  item_seq_file=None is the single form, a path the dual form.

    Row tables, COMPACTED over the ids that occur in the parsed lines (memory follows the files, not the id range: CCMR has
    about 5 M ids): user_rows [n_user_rows, Fu] and item_rows [n_item_rows, Fi] hold [id, features...] per entity, one row
    per distinct dictionary KEY, in order of first use.  A history id's key is str(int(id)), a target id's key the text as
    written -- what the host loaders look up -- so '7' and '07' are two rows where a target line writes the latter.  Everything
    else names a row of these tables, never an id (column 0 of the row is the id):
      user_off int64 [n_lines + 1], user_seq int32: line l's history is user_seq[user_off[l]:user_off[l + 1]], the rows (in
          item_rows) of the LAST max_len ids of the line; user_len int32 [n_lines] its untruncated length;
      item_off / item_seq / item_len: the same per sample l * per_line + c (rows in user_rows), dual form only, else None;
      target_user int32 [n_lines] (DualSeq's rebinding kept: the row of the last id of the line's last item sequence as
          written), target_item int32 [n_lines * per_line].
    Only the lines of whole batches are parsed (n_lines = lines in the target file // lines_per_batch * lines_per_batch); the
    tail of the history files is never read.  Per batch, from parse time: batch_max_user_len, and in the dual form
    batch_max_len / batch_min_len over both length arrays (in the single form they are the user side's), so no batch needs a
    read-back to know its active slices.

    Malformed input raises here what the host loader raises at that batch: ValueError for an empty history or a history file
    shorter than the target file (int('')), IndexError for fewer item sequences than 1 + neg_sample_num, KeyError for an id
    missing from a dictionary; ValueError for batch_size % (1 + neg_sample_num) != 0.  A target line with fewer than
    1 + neg_sample_num items, which the host loader turns into a short batch, is a ValueError: a batch here has one size."""

    def __init__(self, target_file, user_seq_file, item_seq_file, max_len, neg_sample_num, batch_size,
                 user_feat_dict_file=None, item_feat_dict_file=None):
        self.batch_size, self.max_len, self.neg_sample_num = int(batch_size), int(max_len), int(neg_sample_num)
        self.per_line = per_line = 1 + self.neg_sample_num
        if self.batch_size % per_line != 0:
            raise ValueError("batch size should be a multiple of %d (1 + neg_sample_num)" % per_line)
        if self.max_len <= 0:
            raise ValueError("max_len must be positive")
        self.lines_per_batch = self.batch_size // per_line
        self.dual = item_seq_file is not None
        self.files = (target_file, user_seq_file, item_seq_file, user_feat_dict_file, item_feat_dict_file)
        user_dict = DataLoaderUserSeq._load(user_feat_dict_file)
        item_dict = DataLoaderUserSeq._load(item_feat_dict_file)
        L = self.max_len
        u_rows, i_rows, u_map, i_map = [], [], {}, {}

        def row_of(key, table, rows, dct):
            r = table.get(key)
            if r is None:
                row = [int(key)] + (list(dct[key]) if dct is not None else [])
                r = table[key] = len(rows)
                rows.append(row)
            return r

        def kept(hist):        # (the pad repeats the last id: converting it again could not raise anything new)
            return [str(int(i)) for i in hist[-L:]]
        with open(target_file) as f:
            n_total = sum(1 for _ in f)
        self.n_batches = n_total // self.lines_per_batch
        self.n_lines = n_lines = self.n_batches * self.lines_per_batch
        user_seq, user_len, item_seq, item_len, t_user, t_item = [], [], [], [], [], []
        user_off, item_off = [0], [0]
        tf, uf = open(target_file), open(user_seq_file)
        itf = open(item_seq_file) if self.dual else None
        try:
            for _ in range(n_lines):
                fields = tf.readline()[:-1].split(",")
                uid, iids = fields[0], fields[1:1 + per_line]
                hist = uf.readline()[:-1].split(",")
                if self.dual:
                    item_hists = [h.split(",") for h in itf.readline()[:-1].split("\t")]
                user_seq += [row_of(k, i_map, i_rows, item_dict) for k in kept(hist)]
                user_off.append(len(user_seq))
                user_len.append(len(hist))
                if self.dual:
                    resolved = [[row_of(k, u_map, u_rows, user_dict) for k in kept(h)] for h in item_hists]
                    uid = item_hists[-1][-1]          # (the reference's rebinding of `uid`)
                t_user.append(row_of(uid, u_map, u_rows, user_dict))
                if len(iids) < per_line:
                    raise ValueError("a target line holds %d items, fewer than 1 + neg_sample_num = %d" % (len(iids), per_line))
                for j, iid in enumerate(iids):
                    t_item.append(row_of(iid, i_map, i_rows, item_dict))
                    if self.dual:
                        item_len.append(len(item_hists[j]))
                        item_seq += resolved[j]
                        item_off.append(len(item_seq))
        finally:
            tf.close()
            uf.close()
            if itf is not None:
                itf.close()
        i32 = np.int32
        self.user_off, self.user_seq = np.asarray(user_off, dtype=np.int64), np.asarray(user_seq, dtype=i32)
        self.user_len = np.asarray(user_len, dtype=i32)
        self.target_user, self.target_item = np.asarray(t_user, dtype=i32), np.asarray(t_item, dtype=i32)
        if self.dual:
            self.item_off, self.item_seq = np.asarray(item_off, dtype=np.int64), np.asarray(item_seq, dtype=i32)
            self.item_len = np.asarray(item_len, dtype=i32)
        else:
            self.item_off = self.item_seq = self.item_len = None
        # (rows of unequal width: the ValueError np.stack raises in the host loader)
        self.user_rows = np.asarray(u_rows, dtype=i32).reshape(len(u_rows), -1) if u_rows else np.zeros((0, 1), dtype=i32)
        self.item_rows = np.asarray(i_rows, dtype=i32).reshape(len(i_rows), -1) if i_rows else np.zeros((0, 1), dtype=i32)
        self.Fu, self.Fi = int(self.user_rows.shape[1]), int(self.item_rows.shape[1])
        per_batch = self.user_len.reshape(self.n_batches, self.lines_per_batch)
        self.batch_max_user_len = per_batch.max(axis=1) if self.n_batches else np.zeros((0,), dtype=i32)
        self.batch_max_len, self.batch_min_len = self.batch_max_user_len, (per_batch.min(axis=1) if self.n_batches else self.batch_max_user_len)
        if self.dual and self.n_batches:
            other = self.item_len.reshape(self.n_batches, self.batch_size)
            self.batch_max_len = np.maximum(self.batch_max_len, other.max(axis=1))
            self.batch_min_len = np.minimum(self.batch_min_len, other.min(axis=1))
        self._dev = self.device = self.struct = None

    def check(self, batch_size, max_len, neg_sample_num, dual):
        """ValueError unless a loader with these arguments would cut this store's lines into this store's batches"""
        got = (int(batch_size), int(max_len), int(neg_sample_num), bool(dual))
        have = (self.batch_size, self.max_len, self.neg_sample_num, self.dual)
        if got != have:
            raise ValueError("the store was built for (batch_size, max_len, neg_sample_num, dual) = %r, the loader asks for %r"
                             % (have, got))

    def to_device(self, device=None):
        import ctypes as C
        from . import _lib
        dev = device_of(device, "PointSeqStore.to_device", instead=NO_CPU_PATH)
        names = ("user_off", "user_seq", "user_len", "item_off", "item_seq", "item_len", "target_user", "target_item",
                 "user_rows", "item_rows")
        d = upload_named(names, lambda k: getattr(self, k), dev)
        ptr = lambda k: C.c_void_p(d[k].data_ptr()) if k in d else C.c_void_p(0)
        self._dev, self.device = d, dev
        self.struct = _lib.PointStore(C.sizeof(_lib.PointStore), *[ptr(k) for k in names], self.n_lines,
                                      len(self.user_rows), len(self.item_rows), self.per_line, self.max_len)
        return self


def host_hist_csr(ent, other, time_key, t_idx, start_time, pred_time, id_lo, n_ent, hist_max_len):
    """score_point_hist_build (csrc/pointhist.hip) in numpy: one side's histories from the log.  -> (off int64 [n_ent + 1],
    seq int32, len int32 [n_ent]): entity e = id - id_lo has the history seq[off[e]:off[e + 1]], its events of slices
    [start_time, pred_time) ordered by (time_key, position in the log); len[e] = min(its count, hist_max_len), and the kept
    history is the last len[e] ids of it."""
    ent, other, time_key, t_idx = (np.asarray(a) for a in (ent, other, time_key, t_idx))
    e = ent.astype(np.int64) - id_lo
    keep = np.flatnonzero((t_idx >= start_time) & (t_idx < pred_time) & (e >= 0) & (e < n_ent))
    order = keep[np.lexsort((keep, time_key[keep], e[keep]))]
    off = np.zeros(n_ent + 1, dtype=np.int64)
    np.cumsum(np.bincount(e[keep], minlength=n_ent), out=off[1:])
    return off, other[order].astype(np.int32), np.minimum(np.diff(off), hist_max_len).astype(np.int32)


class PointLogStore(object):
    """The point baselines' histories straight from the remapped interaction log -- ONE history per user and one per item,
    bounded by the log, instead of the file form's one sequence per sample -- and the target lines; the device loaders below
    take it as `store=` and yield, integer for integer, the batches the reference's chain yields from the same log and lines:
    gen_target.py:223-275 (hist dicts) -> gen_history_point.py:22-65 (files; dataprep.point_history_lines restates both) ->
    DataLoaderUserSeq / DataLoaderDualSeq.

    uid / iid / time_key / t_idx [n]: the log as dataprep.remap_tmall_log returns it, or (build="device") the same four columns as
    int32 tensors already on the device (users 1 .. U, items U + 1 .. U + I,
    U and I the row counts of user_rows [U, Fu] / item_rows [I, Fi], whose column 0 is the id) and a non-negative key that
    orders events as the reference's time_int does (Tmall: the MMDD column).  target_lines: (uid, [items...]) as
    dataprep.gen_target_lines yields them, or a targets.TargetStore: its arrays are taken as they are, and under build="device" a
    store on the device is never downloaded.

    Arrays (numpy with build="host", device tensors with build="device"; .arrays() gives numpy either way):
      user_hist_off int64 [U + 1], user_hist_seq int32, user_hist_len int32 [U]: user u's events of slices
          [start_time, pred_time) ordered by (time_key, position in the log) are the ITEM IDS
          user_hist_seq[off[u - 1]:off[u]]; len = min(count, hist_max_len), the length the loaders report, and the kept
          history the last len ids of the segment; a batch at max_len T reads the last min(len, T) of those;
      item_hist_off / _seq / _len: the same over the items (user ids), dual form only, else None;
      line_user int32 [n_lines], line_items int32 [n_lines * per_line], line_last_item int32 [n_lines] (the line's last item
          AS WRITTEN: in the dual form target_user is the last id of ITS kept history, DataLoaderDualSeq's rebinding, 0 if none).
    Only the lines of whole batches are kept.  batch_max_user_len / batch_max_len / batch_min_len as PointSeqStore's.  The
    store does not depend on max_len: one store serves models of different max_time_len.

    build="host" is numpy and needs no GPU; build="device" sorts the log on the device (csrc/pointhist.hip) and reads back
    once, the per-batch length extremes and the shortest user history of a target line; no batch reads anything back.

    An item without history has the reference's stand-in history [0]: a sequence of zero rows, length 1.  Id 0 is a row of
    ZEROS here; the reference's loader raises KeyError for it unless its feature dictionary has a key '0' -- that failure is
    deliberately not reproduced (dataprep.write_point_files writes the key).
    ValueError: batch_size % (1 + neg_sample_num) != 0; a log or target id outside its range; a target line with fewer than
    1 + neg_sample_num items; a target line whose user has no history (the reference: exit(1)), naming the line."""

    def __init__(self, uid, iid, time_key, t_idx, target_lines, start_time, pred_time, hist_max_len, neg_sample_num, batch_size,
                 user_rows, item_rows, dual, build="device", device=None):
        i32 = np.int32
        self.batch_size, self.neg_sample_num, self.hist_max_len = int(batch_size), int(neg_sample_num), int(hist_max_len)
        self.per_line = per_line = 1 + self.neg_sample_num
        if self.batch_size % per_line != 0:
            raise ValueError("batch size should be a multiple of %d (1 + neg_sample_num)" % per_line)
        if self.hist_max_len <= 0:
            raise ValueError("hist_max_len must be positive")
        check_build(build, "build must be 'device' or 'host'")
        self.lines_per_batch = self.batch_size // per_line
        self.dual, self.build = bool(dual), build
        self.start_time, self.pred_time = int(start_time), int(pred_time)
        self.user_rows = np.ascontiguousarray(user_rows, dtype=i32)
        self.item_rows = np.ascontiguousarray(item_rows, dtype=i32)
        if self.user_rows.ndim != 2 or self.item_rows.ndim != 2 or not len(self.user_rows) or not len(self.item_rows):
            raise ValueError("user_rows / item_rows must be non-empty [n, F] tables")
        self.n_users, self.n_items = U, I = len(self.user_rows), len(self.item_rows)
        self.Fu, self.Fi = int(self.user_rows.shape[1]), int(self.item_rows.shape[1])
        if not (np.array_equal(self.user_rows[:, 0], np.arange(1, U + 1)) and
                np.array_equal(self.item_rows[:, 0], np.arange(U + 1, U + I + 1))):
            raise ValueError("column 0 of user_rows / item_rows must be the ids 1 .. U / U + 1 .. U + I")
        if all(is_tensor(a) and a.is_cuda for a in (uid, iid, time_key, t_idx)):
            # the log as int32 tensors already on the device (one upload serves the graph, the targets and the histories):
            # the range checks read six extremes back
            import torch
            if build != "device":
                raise ValueError("a log on the device needs build='device'")
            if device is None:
                device = uid.device
            cols = [device_i32(a, device) for a in (uid, iid, time_key, t_idx)]
            sizes = [int(c.numel()) for c in cols]
            ext = torch.stack([f(c) for c in cols[:3] for f in (torch.amin, torch.amax)]).cpu().tolist() if min(sizes) else None
        else:
            cols = [np.ascontiguousarray(np.asarray(to_host(a)).reshape(-1)) for a in (uid, iid, time_key, t_idx)]
            sizes = [len(c) for c in cols]
            ext = [int(f()) for c in cols[:3] for f in (c.min, c.max)] if min(sizes) else None
        if ext is None or any(n != sizes[0] for n in sizes) or sizes[0] >= 2 ** 31:
            raise ValueError("uid, iid, time_key and t_idx must be equally long, with 1 .. 2^31 - 1 events")
        if ext[0] < 1 or ext[1] > U or ext[2] < U + 1 or ext[3] > U + I:
            raise ValueError("the log's uid must lie in 1 .. %d and its iid in %d .. %d" % (U, U + 1, U + I))
        if ext[4] < 0 or ext[5] >= 2 ** 31:
            raise ValueError("time_key must be a non-negative 31-bit integer")
        self._log = cols if not isinstance(cols[0], np.ndarray) else [c.astype(i32) for c in cols]
        self.time_bits = max(1, int(ext[5]).bit_length())
        from .targets import TargetStore
        self.n_batches = (target_lines.n_lines if isinstance(target_lines, TargetStore) else len(target_lines)) // self.lines_per_batch
        self.n_lines = n_lines = self.n_batches * self.lines_per_batch
        self._first_bad_line = None
        if isinstance(target_lines, TargetStore):
            self._lines_from_store(target_lines, build, device)
        else:
            line_user, line_items, line_last = [], [], []
            for l, (u, items) in enumerate(target_lines[:n_lines]):
                if len(items) < per_line:
                    raise ValueError("target line %d holds %d items, fewer than 1 + neg_sample_num = %d" % (l, len(items), per_line))
                line_user.append(int(u))
                line_items += [int(i) for i in items[:per_line]]
                line_last.append(int(items[-1]))
                if not 1 <= line_user[-1] <= U or min(int(i) for i in items) < U + 1 or max(int(i) for i in items) > U + I:
                    raise ValueError("target line %d: an id outside users 1 .. %d / items %d .. %d" % (l, U, U + 1, U + I))
            self.line_user, self.line_items = np.asarray(line_user, dtype=i32), np.asarray(line_items, dtype=i32)
            self.line_last_item = np.asarray(line_last, dtype=i32)
        self._dev = self.device = self.struct = None
        if build == "host":
            self._build_host()
        else:
            self._build_device(device)
        self._log = None
        if n_lines and self._line_min_user_len[0] <= 0:
            l = int(self._line_min_user_len[1])
            raise ValueError("target line %d: user %d has no history in slices [%d, %d)"
                             % (l, int(self.line_user[l]), self.start_time, self.pred_time))

    def _lines_from_store(self, store, build, device):
        """line_user / line_items / line_last_item from a targets.TargetStore's arrays, whole batches only.  A store on the
        device stays there under build="device": its id-range check rides in the build's one read-back (_first_bad_line)."""
        U, I, per_line, n_lines = self.n_users, self.n_items, self.per_line, self.n_lines
        if store.per_line < per_line:
            raise ValueError("target line 0 holds %d items, fewer than 1 + neg_sample_num = %d" % (store.per_line, per_line))
        if build == "device" and store.on_device:
            import torch
            dev = torch.device(device if device is not None else store.line_user.device)
            lu, li = (a[:n_lines] for a in store.device_tensors(dev))
            self.line_user, self.line_items = lu.contiguous(), li[:, :per_line].contiguous().view(-1)
            self.line_last_item = li[:, -1].contiguous()
            if n_lines:
                bad = (lu < 1) | (lu > U) | (li.amin(dim=1) < U + 1) | (li.amax(dim=1) > U + I)
                lines = torch.arange(n_lines, device=dev)
                self._first_bad_line = torch.where(bad, lines, torch.full_like(lines, n_lines)).amin().reshape(1)
            return
        lu, li = (a[:n_lines] for a in store.arrays())
        bad = np.flatnonzero((lu < 1) | (lu > U) | (li.min(axis=1, initial=U + 1) < U + 1) | (li.max(axis=1, initial=U + 1) > U + I))
        if len(bad):
            raise ValueError("target line %d: an id outside users 1 .. %d / items %d .. %d" % (int(bad[0]), U, U + 1, U + I))
        self.line_user = np.ascontiguousarray(lu, dtype=np.int32)
        self.line_items = np.ascontiguousarray(li[:, :per_line], dtype=np.int32).reshape(-1)
        self.line_last_item = np.ascontiguousarray(li[:, -1], dtype=np.int32)

    def _line_rows(self):
        """the 0-based rows of the lines' users and items in the length arrays: numpy, or (a store on the device) long tensors
        clamped into range -- an id outside it is reported from the read-back, not looked up"""
        if isinstance(self.line_user, np.ndarray):
            return self.line_user.astype(np.int64) - 1, self.line_items.astype(np.int64) - 1 - self.n_users
        return ((self.line_user.long() - 1).clamp(0, self.n_users - 1),
                (self.line_items.long() - 1 - self.n_users).clamp(0, self.n_items - 1))

    HIST = ("user_hist_off", "user_hist_seq", "user_hist_len", "item_hist_off", "item_hist_seq", "item_hist_len")

    def _extremes(self, user_len, item_len, take, maximum, minimum, amax, amin):
        """per batch: the longest user history, the longest and the shortest history of both sides; and the shortest user
        history of any line with its line -- in numpy or torch, whichever the five functions belong to"""
        nb, lpb = self.n_batches, self.lines_per_batch
        rows_u, rows_i = self._line_rows()
        lu = take(user_len, rows_u)
        per = lu.reshape(nb, lpb)
        mx_u, mn = amax(per), amin(per)
        mx = mx_u
        if self.dual:
            li = take(item_len, rows_i).reshape(nb, self.batch_size)
            li = maximum(li, li * 0 + 1)                                       # (no history: the stand-in [0], length 1)
            mx, mn = maximum(mx, amax(li)), minimum(mn, amin(li))
        return mx_u, mx, mn, lu.min().reshape(1), lu.argmin().reshape(1)

    def _set_extremes(self, parts):
        nb = self.n_batches
        parts = [np.asarray(p).astype(np.int64) for p in parts]
        self.batch_max_user_len, self.batch_max_len, self.batch_min_len = (p.astype(np.int32) for p in parts[:3])
        self._line_min_user_len = (int(parts[3][0]), int(parts[4][0])) if nb else (1, 0)     # (length, line)

    def _build_host(self):
        uid, iid, time_key, t_idx = self._log
        U, I, H = self.n_users, self.n_items, self.hist_max_len
        self.user_hist_off, self.user_hist_seq, self.user_hist_len = host_hist_csr(uid, iid, time_key, t_idx, self.start_time,
                                                                                   self.pred_time, 1, U, H)
        if self.dual:
            self.item_hist_off, self.item_hist_seq, self.item_hist_len = host_hist_csr(iid, uid, time_key, t_idx, self.start_time,
                                                                                       self.pred_time, U + 1, I, H)
        else:
            self.item_hist_off = self.item_hist_seq = self.item_hist_len = None
        if self.n_batches:
            self._set_extremes(self._extremes(self.user_hist_len, self.item_hist_len, lambda a, i: a[i], np.maximum, np.minimum,
                                              lambda a: a.max(axis=1), lambda a: a.min(axis=1)))
        else:
            self._set_extremes([np.zeros((0,))] * 5)

    def _build_device(self, device):
        import ctypes as C
        import torch
        from . import _lib
        dev = device_of(device, "PointLogStore(build='device')")
        lib = _lib.load()
        uid, iid, time_key, t_idx = [device_i32(c, dev) for c in self._log]
        n, U, I = int(uid.numel()), self.n_users, self.n_items
        temp, temp_bytes = _lib.workspace("score_point_hist", dev, n)
        stream = _lib.current_stream(dev)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        out = {}
        for side, ent, other, id_lo, n_ent in (("user", uid, iid, 1, U), ("item", iid, uid, U + 1, I)):
            if side == "item" and not self.dual:
                out.update(item_hist_off=None, item_hist_seq=None, item_hist_len=None)
                continue
            off = torch.empty((n_ent + 1,), dtype=torch.int64, device=dev)
            seq = torch.empty((n,), dtype=torch.int32, device=dev)
            ln = torch.empty((n_ent,), dtype=torch.int32, device=dev)
            rc = lib.score_point_hist_build(ptr(ent), ptr(other), ptr(time_key), ptr(t_idx), n, self.start_time, self.pred_time,
                                            id_lo, n_ent, self.time_bits, self.hist_max_len, ptr(off), ptr(seq), ptr(ln),
                                            ptr(temp), temp_bytes, stream)
            _lib.check(rc, "score_point_hist_build")
            out.update({side + "_hist_off": off, side + "_hist_seq": seq, side + "_hist_len": ln})
        for k, v in out.items():
            setattr(self, k, v)
        if self.n_batches:       # the one read-back of the build
            parts = self._extremes(self.user_hist_len, self.item_hist_len,
                                   lambda a, i: a[device_as(i, dev)],
                                   torch.maximum, torch.minimum, lambda a: a.amax(dim=1), lambda a: a.amin(dim=1))
            if self._first_bad_line is not None:                   # (a target store on the device: its id-range check)
                parts = tuple(parts) + (self._first_bad_line.to(dev),)
            sizes = [len(p) for p in parts]
            host = np.split(torch.cat([p.to(torch.int64) for p in parts]).cpu().numpy(), np.cumsum(sizes)[:-1])
            if self._first_bad_line is not None and int(host[5][0]) < self.n_lines:
                raise ValueError("target line %d: an id outside users 1 .. %d / items %d .. %d"
                                 % (int(host[5][0]), U, U + 1, U + I))
            self._set_extremes(host[:5])
        else:
            torch.cuda.current_stream(dev).synchronize()
            self._set_extremes([np.zeros((0,))] * 5)
        del temp
        self._upload(dev, out)

    def arrays(self):
        """the six history arrays as numpy (None for a missing item side), the seq arrays cut to the words in use"""
        out = {}
        for k in self.HIST:
            a = getattr(self, k)
            out[k] = a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()
        for side in ("user", "item"):
            if out[side + "_hist_seq"] is not None:
                out[side + "_hist_seq"] = out[side + "_hist_seq"][:int(out[side + "_hist_off"][-1])]
        return out

    def check(self, batch_size, max_len, neg_sample_num, dual):
        """ValueError unless a loader with these arguments cuts this store's lines into this store's batches and its max_len
        fits the assembly kernel (T * F <= 8192 words on both sides)"""
        got = (int(batch_size), int(neg_sample_num), bool(dual))
        have = (self.batch_size, self.neg_sample_num, self.dual)
        if got != have:
            raise ValueError("the store was built for (batch_size, neg_sample_num, dual) = %r, the loader asks for %r" % (have, got))
        if int(max_len) <= 0 or int(max_len) * max(self.Fu, self.Fi) > 8192:
            raise ValueError("max_len %d: max_len * max(Fu, Fi) must lie in 1 .. 8192" % int(max_len))

    def _upload(self, dev, have):
        import ctypes as C
        from . import _lib
        names = self.HIST + ("line_user", "line_items", "line_last_item", "user_rows", "item_rows")
        d = upload_named(names, lambda k: have.get(k, getattr(self, k)), dev)
        ptr = lambda k: C.c_void_p(d[k].data_ptr()) if k in d else C.c_void_p(0)
        self._dev, self.device = d, dev
        self.struct = _lib.PointLogStore(C.sizeof(_lib.PointLogStore), *[ptr(k) for k in names], self.n_lines, self.n_users,
                                         self.n_items, self.per_line, self.hist_max_len)

    def to_device(self, device=None):
        dev = device_of(device, "PointLogStore.to_device", instead=NO_CPU_PATH)
        have = {}
        if self._dev is not None:                # (a device build on another device: its tensors move)
            have = {k: v.to(dev) for k, v in self._dev.items() if k in self.HIST}
            for k, v in have.items():
                setattr(self, k, v)
        self._upload(dev, have)
        return self

    # ---- lines for arbitrary users (csrc/pointloader.hip: score_point_user_lines) ----------------------------------------
    def _user_extremes(self):
        """(longest user segment, longest kept length): one read-back per store, at the first ask, then cached"""
        ext = getattr(self, "_user_ext", None)
        if ext is None:
            off, ln = self.user_hist_off, self.user_hist_len
            if isinstance(off, np.ndarray):
                ext = (int(np.diff(off).max()), int(ln.max()))
            else:
                import torch
                ext = tuple(int(v) for v in torch.stack([(off[1:] - off[:-1]).amax(), ln.amax().to(off.dtype)]).cpu().tolist())
            self._user_ext = ext
        return ext

    @property
    def max_user_events(self):
        """the longest user segment of user_hist_seq (all events of the window, not only the kept ones)"""
        return self._user_extremes()[0]

    @property
    def max_user_len(self):
        """the longest kept length, max(user_hist_len)"""
        return self._user_extremes()[1]

    def _check_max_len(self, max_len):
        T = int(max_len)
        if T <= 0 or T * self.Fi > 8192:
            raise ValueError("max_len %d: max_len * Fi must lie in 1 .. 8192" % T)
        return T

    def host_user_lines(self, user_ids, max_len):
        """user_lines in numpy, from .arrays(): (user_seq [L, T, Fi], length [L], target_user [L, Fu], known [L]) int32.  Line
        l is what the loaders write for the first sample of a target line of user user_ids[l] at max_len T: the last
        min(user_hist_len, T) ids of the kept history as rows of item_rows, padded by repeating the last; the untruncated kept
        length; the user's row.  A user without events: zeros, length 0, known 1; an id outside 1 .. n_users: zeros, length 0,
        known 0.  Needs no GPU."""
        T = self._check_max_len(max_len)
        a = self.arrays()
        off, seq, ln = a["user_hist_off"], a["user_hist_seq"], a["user_hist_len"]
        U, I = self.n_users, self.n_items
        u = np.asarray(to_host(user_ids)).reshape(-1).astype(np.int64)
        known = (u >= 1) & (u <= U)
        e = np.where(known, u - 1, 0)
        length = np.where(known, ln[e], 0).astype(np.int64)
        m = np.clip(np.minimum(length, T), 0, None)
        b = np.maximum(off[e + 1] - m, off[e])
        m = np.minimum(m, off[e + 1] - b)
        pos = b[:, None] + np.minimum(np.arange(T)[None, :], np.maximum(m - 1, 0)[:, None])
        ids = seq[np.clip(pos, 0, max(len(seq) - 1, 0))].astype(np.int64) if len(seq) else np.zeros(pos.shape, dtype=np.int64)
        row = ids - (U + 1)
        ok = (m > 0)[:, None] & (row >= 0) & (row < I)
        user_seq = np.where(ok[:, :, None], self.item_rows[np.clip(row, 0, I - 1)], 0).astype(np.int32)
        target_user = np.where(known[:, None], self.user_rows[e], 0).astype(np.int32)
        return user_seq, length.astype(np.int32), target_user, known.astype(np.int32)

    def user_lines(self, user_ids, max_len):
        """(user_seq [L, T, Fi], length [L], target_user [L, Fu], known [L]) int32 device tensors for ANY users of the store --
        what model.lines_of takes from a loader batch, without a target line, an expanded batch or a read-back: one launch
        (score_point_user_lines) on the current stream into one buffer.  user_ids: a device tensor or host array [L]; the same
        user may occur several times.  The contract is host_user_lines'.  The store must be on a device (build="device" or
        .to_device()): RuntimeError otherwise."""
        import ctypes as C
        import torch
        from . import _lib
        if self._dev is None:
            raise RuntimeError("PointLogStore.user_lines: the store is not on a device (build='device' or .to_device() first)")
        T = self._check_max_len(max_len)
        uid = device_i32(user_ids, self.device).reshape(-1)
        L = int(uid.numel())
        if L == 0:
            raise ValueError("no users")
        Fu, Fi = self.Fu, self.Fi
        flat = torch.empty((L * (T * Fi + Fu + 2),), dtype=torch.int32, device=self.device)
        sizes = (L * T * Fi, L * Fu, L, L)
        user_seq, target_user, length, known = torch.split(flat, sizes)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        rc = _lib.load().score_point_user_lines(C.byref(self.struct), ptr(uid), L, T, Fu, Fi, ptr(user_seq), ptr(length),
                                                ptr(target_user), ptr(known), _lib.current_stream(self.device))
        _lib.check(rc, "score_point_user_lines")
        return user_seq.view(L, T, Fi), length, target_user.view(L, Fu), known

    def store_bytes(self):
        """bytes of the arrays a batch reads (the row tables excluded: both forms hold them)"""
        total = 0
        for k in self.HIST + ("line_user", "line_items", "line_last_item"):
            a = getattr(self, k)
            if a is not None:
                total += int(a.numel() * a.element_size()) if not isinstance(a, np.ndarray) else int(a.nbytes)
        return total


class _Shape(object):
    """the fields of a model's cfg that say how large a batch's tensors are (a loader without a model has no cfg)"""

    def __init__(self, T, Fu, Fi):
        self.max_time_len, self.obj_per_time_slice, self.user_fnum, self.item_fnum = T, 1, Fu, Fi


class DeviceDataLoaderUserSeq(object):
    """DataLoaderUserSeq's constructor (point_models/data_loader.py:16), its batches assembled on the device: every batch is one
    torch.empty and one launch (score_point_batch_assemble) on the current stream, and what comes out is a DeviceBatch that
    train / eval / harness.evaluate take as it is and that still indexes like the reference's 5-tuple (batch_data[3]: the target
    items).  The files are parsed once, by a PointSeqStore: the reference builds a fresh loader per epoch and per validation
    pass, and `store=previous.store` skips the parse and the upload (ValueError if batch_size, max_len or neg_sample_num are
    not the store's).  store= a PointLogStore: the same batches from per-entity histories built from the log
    (score_point_batch_assemble_log); the file arguments may then be None, max_len is free (one store serves every T with
    T * F <= 8192) and batch_size, neg_sample_num and the form are checked.  model=: the batches carry the active_slices DeviceBatch(model, host_tuple) would compute, from the
    store's per-batch length extremes -- no device value is read; max_len and the two feature counts are checked against
    model.cfg.  Without a model active_slices is 0 (all T).  Needs a GPU (RuntimeError); a PointSeqStore alone does not."""
    dual = False

    def __init__(self, batch_size, max_len, target_file, user_seq_file, neg_sample_num, user_feat_dict_file,
                 item_feat_dict_file, model=None, store=None, device=None):
        self._setup(batch_size, max_len, target_file, user_seq_file, None, neg_sample_num, user_feat_dict_file,
                    item_feat_dict_file, model, store, device)

    def _setup(self, batch_size, max_len, target_file, user_seq_file, item_seq_file, neg_sample_num, user_feat_dict_file,
               item_feat_dict_file, model, store, device):
        import torch
        from . import _lib
        from . import model as M
        self.batch_size, self.max_len, self.neg_sample_num = int(batch_size), int(max_len), int(neg_sample_num)
        per_line = 1 + self.neg_sample_num
        if self.batch_size % per_line != 0:
            raise ValueError("batch size should be a multiple of %d (1 + neg_sample_num)" % per_line)
        if store is not None:
            store.check(batch_size, max_len, neg_sample_num, self.dual)
        device_of(what=type(self).__name__, instead=NO_CPU_PATH)           # (which device: the model's or the store's, below)
        if store is None:
            store = PointSeqStore(target_file, user_seq_file, item_seq_file, max_len, neg_sample_num, batch_size,
                                  user_feat_dict_file, item_feat_dict_file)
        self.store = store
        self.from_log = isinstance(store, PointLogStore)      # (its histories are not cut to one max_len: T is the loader's)
        T = self.max_len if self.from_log else store.max_len
        self.spec = M.DUAL_FEED if self.dual else M.POINT_FEED
        if model is not None:
            cfg = model.cfg
            if model.feed_spec.n != self.spec.n:
                raise ValueError("the model is fed %s, this loader yields %s" % (model.feed_spec.what, self.spec.what))
            if store.n_batches and (int(cfg.max_time_len), int(cfg.user_fnum), int(cfg.item_fnum)) != (T, store.Fu, store.Fi):
                raise ValueError("the model has (max_time_len, user_fnum, item_fnum) = %r, the files give %r"
                                 % ((cfg.max_time_len, cfg.user_fnum, cfg.item_fnum), (T, store.Fu, store.Fi)))
            if device is None:
                device = model.device
            if self.dual:
                self._active = [M.active_slices(model, a, b) for a, b in zip(store.batch_max_len, store.batch_min_len)]
            else:
                self._active = [M.active_slices(model, a) for a in store.batch_max_user_len]
        else:
            self._active = [0] * store.n_batches
        if store._dev is None or (device is not None and torch.device(device) != store.device):
            store.to_device(device)
        self.device, self.lib = store.device, _lib.load()
        self.lines_per_batch = store.lines_per_batch
        self._T = T
        self._shape = _Shape(T, store.Fu, store.Fi)
        self._shapes = self.spec.device_shapes(self._shape, self.batch_size)
        self._n_flat = M.flat_batch_size(self._shapes)
        self._feed_shapes = self.spec.shapes(self._shape, self.batch_size)
        self._batch_no = 0

    def close(self):
        """the host loaders close their files here; the store read them to their end and holds none open"""
        return None

    def __iter__(self):
        return self

    def __len__(self):
        return self.store.n_batches

    def __next__(self):
        import ctypes as C
        import torch
        from . import _lib
        from . import model as M
        i, st = self._batch_no, self.store
        if i >= st.n_batches:
            raise StopIteration
        flat = torch.empty((self._n_flat,), dtype=torch.int32, device=self.device)
        tens = M.carve_batch(flat, self._shapes)
        out = _lib.BatchOut(*[M._ptr(t) for t in tens[:8]])
        call = self.lib.score_point_batch_assemble_log if self.from_log else self.lib.score_point_batch_assemble
        rc = call(C.byref(st.struct), i * self.lines_per_batch, self.lines_per_batch, st.per_line, self._T, st.Fu, st.Fi,
                  C.byref(out), M._ptr(tens[8]) if self.dual else None,
                  _lib.current_stream(self.device))
        _lib.check(rc, "score_point_batch_assemble_log" if self.from_log else "score_point_batch_assemble")
        self._batch_no = i + 1
        return _point_batch_class()(tens, flat, self.batch_size, self._active[i], self.spec, self._feed_shapes)

    next = __next__


class DeviceDataLoaderDualSeq(DeviceDataLoaderUserSeq):
    """DataLoaderDualSeq's constructor (data_loader.py:90) over the same store and kernel: the 7-tuple's item_seq rides as
    item_1hop and item_seq_length as the ninth tensor, length2; batch_data[5] are the target items.  With model=, active_slices
    follows both length arrays (DELF: a length <= 0 anywhere in the batch computes all T; DEEMS: it does not)."""
    dual = True

    def __init__(self, batch_size, max_len, target_file, user_seq_file, item_seq_file, neg_sample_num, user_feat_dict_file,
                 item_feat_dict_file, model=None, store=None, device=None):
        if item_seq_file is None and store is None:
            raise ValueError("DeviceDataLoaderDualSeq needs an item_seq_file")
        self._setup(batch_size, max_len, target_file, user_seq_file, item_seq_file, neg_sample_num, user_feat_dict_file,
                    item_feat_dict_file, model, store, device)


_POINT_BATCH = None


def _point_batch_class():
    """the DeviceBatch subclass the device loaders yield (made on first use: score_amd.model imports torch, this module's host
    loaders do not need it)"""
    global _POINT_BATCH
    if _POINT_BATCH is None:
        from .model import DeviceBatch, _batch_struct

        class PointDeviceBatch(DeviceBatch):
            """a point batch assembled on the device (views of one flat buffer, like every DeviceBatch); indexable like the
            reference's 5- / 7-tuple, field i in the tuple's own shape"""

            def __init__(self, tensors, flat, B, active, spec, feed_shapes):
                self.tensors, self.flat, self.B, self.active_slices = tensors, flat, B, int(active)
                self._spec, self._feed_shapes = spec, feed_shapes
                self.struct = _batch_struct(tensors, B, self.active_slices)

            def __len__(self):
                return self._spec.n

            def __getitem__(self, i):
                if not -self._spec.n <= i < self._spec.n:
                    raise IndexError(i)
                i %= self._spec.n
                for k, sl in enumerate(self._spec.slots):
                    if sl[0] == i:
                        return self.tensors[k].view(self._feed_shapes[k])
        _POINT_BATCH = PointDeviceBatch
    return _POINT_BATCH
