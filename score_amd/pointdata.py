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
     target_item [B, Fi], label [B])."""
import pickle

import numpy as np


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
