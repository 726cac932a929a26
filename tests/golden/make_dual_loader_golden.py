"""G8: golden batches from the REFERENCE dual-sequence loader (code/point_models/data_loader.py DataLoaderDualSeq, imported in
the build container).  Commits only data: small synthetic target lines, user-history lines, item-history lines (one user
sequence per item of the target line, tab separated) and feature dictionaries, and the nested lists the reference produced
from them, as arrays.

Cases: with and without each feature dictionary; histories shorter than, equal to and longer than max_len on both sides;
neg_sample_num 1 and 99; a target file that ends inside a batch (the partial batch is dropped).  The reference builds a
line's target_user rows from the last user id of the line's last item sequence (its loop rebinds `uid`): the expected
arrays hold that.

Run (where the reference is checked out):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dual_loader_golden.py <reference>/code/point_models"""
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ("user_seq", "user_seq_length", "item_seq", "item_seq_length", "target_user", "target_item", "label")

# tag: (batch_size, max_len, neg_sample_num, target lines, user features, item features)
CASES = {"both": (8, 6, 1, 14, 2, 3), "nouser": (6, 5, 1, 10, 0, 2), "noitem": (4, 4, 1, 7, 1, 0), "none": (4, 7, 1, 7, 0, 0),
         "neg99": (200, 5, 99, 3, 2, 1)}
N_USER, N_ITEM = 30, 60          # users 1 .. 30, items 31 .. 90, feature ids above


def make_case(rng, tag):
    B, L, neg, lines, fu, fi = CASES[tag]
    users = list(range(1, N_USER + 1))
    items = list(range(N_USER + 1, N_USER + N_ITEM + 1))
    target, hist, ihist = [], [], []
    edge = [1, L - 1, L, L + 1, 3 * L]

    def length(i):
        return edge[i] if i < len(edge) else int(rng.integers(1, 3 * L))
    for i in range(lines):
        uid = int(rng.choice(users))
        per = 1 + neg
        iids = rng.choice(items, per + (2 if neg == 1 else 0), replace=neg != 1 and per > len(items))   # (neg 1: two unused extras)
        target.append(",".join([str(uid)] + [str(int(x)) for x in iids]))
        hist.append(",".join(str(int(x)) for x in rng.choice(items, length(i))))
        # one user sequence per item the loader uses; the edge lengths fall on different lines than the user history's
        seqs = [",".join(str(int(x)) for x in rng.choice(users, length((i + 2 + j) % (len(edge) + 3)) if j < 2 else int(rng.integers(1, 2 * L))))
                for j in range(per)]
        ihist.append("\t".join(seqs))
    ufeat = {str(u): [int(x) for x in rng.integers(100, 120, fu)] for u in users} if fu else None
    ifeat = {str(i): [int(x) for x in rng.integers(120, 150, fi)] for i in items} if fi else None
    return B, L, neg, target, hist, ihist, ufeat, ifeat


def write_files(d, target, hist, ihist, ufeat, ifeat):
    paths = [os.path.join(d, n) for n in ("target.txt", "hist.txt", "ihist.txt", "ufeat.pkl", "ifeat.pkl")]
    for p, lines in zip(paths[:3], (target, hist, ihist)):
        with open(p, "w") as f:
            f.write("".join(l + "\n" for l in lines))
    for p, dct in zip(paths[3:], (ufeat, ifeat)):
        if dct is not None:
            with open(p, "wb") as f:
                pickle.dump(dct, f)
    return paths[0], paths[1], paths[2], paths[3] if ufeat is not None else None, paths[4] if ifeat is not None else None


def dict_arrays(dct):
    """a feature dictionary as data: its keys (ints) and its rows"""
    keys = sorted(dct, key=int)
    return np.array([int(k) for k in keys], dtype=np.int32), np.array([dct[k] for k in keys], dtype=np.int32)


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "data_loader.py")):
        raise SystemExit("usage: make_dual_loader_golden.py <reference>/code/point_models")
    sys.path.insert(0, sys.argv[1])
    import data_loader as dl
    rng = np.random.Generator(np.random.PCG64(8))
    blob = {"tags": np.array(sorted(CASES))}
    for tag in sorted(CASES):
        B, L, neg, target, hist, ihist, ufeat, ifeat = make_case(rng, tag)
        with tempfile.TemporaryDirectory() as d:
            tf, hf, ihf, uf, itf = write_files(d, target, hist, ihist, ufeat, ifeat)
            batches = list(dl.DataLoaderDualSeq(B, L, tf, hf, ihf, neg, uf, itf))
        assert batches and len(target) % (B // (1 + neg)) != 0, tag       # (the file ends inside a batch)
        blob[tag + "/cfg"] = np.array([B, L, neg], dtype=np.int32)
        blob[tag + "/target"] = np.array(target)
        blob[tag + "/hist"] = np.array(hist)
        blob[tag + "/ihist"] = np.array(ihist)
        for nm, dct in (("ufeat", ufeat), ("ifeat", ifeat)):
            if dct is not None:
                blob["%s/%s_keys" % (tag, nm)], blob["%s/%s_rows" % (tag, nm)] = dict_arrays(dct)
        blob[tag + "/n_batches"] = np.int32(len(batches))
        for i, b in enumerate(batches):
            for nm, x in zip(FIELDS, b):
                blob["%s/b%d/%s" % (tag, i, nm)] = np.asarray(x, dtype=np.int32)
    out = os.path.join(HERE, "g8_dual_loader.npz")
    np.savez_compressed(out, **blob)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
