"""G7: golden batches from the REFERENCE point-model loader (code/point_models/data_loader.py DataLoaderUserSeq, imported in
the build container).  Commits only data: small synthetic target lines, history lines and feature dictionaries, and the
nested lists the reference produced from them, as arrays.

Cases: with and without each feature dictionary; histories shorter than, equal to and longer than max_len; neg_sample_num 1
and 99; a target file that ends inside a batch (the partial batch is dropped).

Run (container only):  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_point_loader_golden.py"""
import os
import pickle
import sys
import tempfile

import numpy as np

REF = "/root/reference/code/point_models"
HERE = os.path.dirname(os.path.abspath(__file__))

# tag: (batch_size, max_len, neg_sample_num, target lines, user features, item features)
CASES = {"both": (8, 6, 1, 14, 2, 3), "nouser": (6, 5, 1, 10, 0, 2), "noitem": (4, 4, 1, 7, 1, 0), "none": (4, 7, 1, 7, 0, 0),
         "neg99": (200, 5, 99, 5, 2, 3)}
N_USER, N_ITEM = 30, 60          # users 1 .. 30, items 31 .. 90, feature ids above


def make_case(rng, tag):
    B, L, neg, lines, fu, fi = CASES[tag]
    users = list(range(1, N_USER + 1))
    items = list(range(N_USER + 1, N_USER + N_ITEM + 1))
    target, hist = [], []
    lens = [1, L - 1, L, L + 1, 3 * L] + [int(rng.integers(1, 3 * L)) for _ in range(lines)]
    for i in range(lines):
        uid = int(rng.choice(users))
        iids = rng.choice(items, 1 + neg + (2 if neg == 1 else 0), replace=neg != 1 and 1 + neg > len(items))   # (neg 1: two unused extras)
        target.append(",".join([str(uid)] + [str(int(x)) for x in iids]))
        hist.append(",".join(str(int(x)) for x in rng.choice(items, lens[i])))
    ufeat = {str(u): [int(x) for x in rng.integers(100, 120, fu)] for u in users} if fu else None
    ifeat = {str(i): [int(x) for x in rng.integers(120, 150, fi)] for i in items} if fi else None
    return B, L, neg, target, hist, ufeat, ifeat


def write_files(d, target, hist, ufeat, ifeat):
    paths = [os.path.join(d, n) for n in ("target.txt", "hist.txt", "ufeat.pkl", "ifeat.pkl")]
    for p, lines in zip(paths[:2], (target, hist)):
        with open(p, "w") as f:
            f.write("".join(l + "\n" for l in lines))
    for p, dct in zip(paths[2:], (ufeat, ifeat)):
        if dct is not None:
            with open(p, "wb") as f:
                pickle.dump(dct, f)
    return paths[0], paths[1], paths[2] if ufeat is not None else None, paths[3] if ifeat is not None else None


def dict_arrays(dct):
    """a feature dictionary as data: its keys (ints) and its rows"""
    keys = sorted(dct, key=int)
    return np.array([int(k) for k in keys], dtype=np.int32), np.array([dct[k] for k in keys], dtype=np.int32)


def main():
    sys.path.insert(0, REF)
    import data_loader as dl
    rng = np.random.Generator(np.random.PCG64(7))
    blob = {"tags": np.array(sorted(CASES))}
    for tag in sorted(CASES):
        B, L, neg, target, hist, ufeat, ifeat = make_case(rng, tag)
        with tempfile.TemporaryDirectory() as d:
            tf, hf, uf, itf = write_files(d, target, hist, ufeat, ifeat)
            batches = list(dl.DataLoaderUserSeq(B, L, tf, hf, neg, uf, itf))
        assert batches and len(target) % (B // (1 + neg)) != 0, tag       # (the file ends inside a batch)
        blob[tag + "/cfg"] = np.array([B, L, neg], dtype=np.int32)
        blob[tag + "/target"] = np.array(target)
        blob[tag + "/hist"] = np.array(hist)
        for nm, dct in (("ufeat", ufeat), ("ifeat", ifeat)):
            if dct is not None:
                blob["%s/%s_keys" % (tag, nm)], blob["%s/%s_rows" % (tag, nm)] = dict_arrays(dct)
        blob[tag + "/n_batches"] = np.int32(len(batches))
        for i, b in enumerate(batches):
            for nm, x in zip(("user_seq", "user_seq_length", "target_user", "target_item", "label"), b):
                blob["%s/b%d/%s" % (tag, i, nm)] = np.asarray(x, dtype=np.int32)
    out = os.path.join(HERE, "g7_point_loader.npz")
    np.savez_compressed(out, **blob)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
