"""G11: the Taobao feature engineering on a small synthetic UserBehavior.csv, decided by the REFERENCE's own code:
code/feateng_taobao.py preprocess_raw_data (the time window, the 'pv' filter, the one-day slices, the three remapped
vocabularies, item_feat_dict).  Commits only data: the raw integer columns of the log (user, item, category, is_pv, unix time),
the START / END the reference derived, the four columns of its remapped file and item_feat_dict as an array [I, 2] =
[item id, category id].

The reference takes START_TIME / END_TIME from time.mktime, which follows the machine's time zone: TZ is set to UTC (and
time.tzset() called) BEFORE the import, so the fixture does not depend on where it is made.  Its vocabularies are numbered in
set order, which differs from run to run; the test compares through the bijection the two numberings define.

The log holds events at exactly START and exactly END, one second outside each bound, non-'pv' rows inside the window, an
item whose category changes between its first and its last kept event, and a user all of whose events are dropped.

Run (where the reference is checked out):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_taobao_remap_golden.py <reference>/code"""
import os
import pickle
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
BTYPES = ("pv", "buy", "cart", "fav")


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "feateng_taobao.py")):
        raise SystemExit("usage: make_taobao_remap_golden.py <reference>/code")
    os.environ["TZ"] = "UTC"
    time.tzset()
    sys.path.insert(0, sys.argv[1])
    import feateng_taobao as ft
    start, end, day = ft.START_TIME, ft.END_TIME, ft.TIME_DELTA
    assert (start, end, day) == (1511568000, 1512345600, 86400)
    rng = np.random.Generator(np.random.PCG64(11))
    n = 400
    user = 100000 + rng.integers(0, 40, n)
    item = 5000000 + rng.integers(0, 70, n)
    cat = 2000 + item % 9
    btype = rng.choice(4, n, p=[0.7, 0.1, 0.1, 0.1])
    t = rng.integers(start - 2 * day, end + 2 * day, n)
    # the window's edges, both sides
    t[3], t[4], t[5], t[6] = start, end, start - 1, end + 1
    btype[3:7] = 0
    # an item whose category changes between its first and its last kept event (and once more behind the window)
    item[10], item[200], item[390] = 5999999, 5999999, 5999999
    cat[10], cat[200], cat[390] = 2100, 2101, 2102
    t[10], t[200], t[390] = start + 5, start + 3 * day, end + 10
    btype[[10, 200, 390]] = 0
    # a user all of whose events are dropped: outside the window, or inside and not 'pv'
    user[20], user[21], user[22] = 199999, 199999, 199999
    t[20], t[21], t[22] = start - 50, end + 50, start + day
    btype[20], btype[21], btype[22] = 0, 0, 1
    with tempfile.TemporaryDirectory() as d:
        p = lambda name: os.path.join(d, name)
        with open(p("UserBehavior.csv"), "w") as f:
            f.write("".join("%d,%d,%d,%s,%d\n" % (u, i, c, BTYPES[b], s) for u, i, c, b, s in zip(user, item, cat, btype, t)))
        ft.preprocess_raw_data(p("UserBehavior.csv"), p("filtered.txt"), p("remaped.txt"), p("distri.png"), p("remap.pkl"),
                               p("item_feat.pkl"))
        remapped = np.asarray([[int(x) for x in l.strip().split(",")] for l in open(p("remaped.txt"))], dtype=np.int32)
        with open(p("item_feat.pkl"), "rb") as f:
            feat = pickle.load(f)
    item_feat = np.asarray(sorted([int(k)] + v for k, v in feat.items()), dtype=np.int32)
    raw = np.stack([user, item, cat, (btype == 0).astype(np.int64), t], axis=1).astype(np.int64)
    keep = (t >= start) & (t <= end) & (btype == 0)
    assert len(remapped) == keep.sum() and keep[3] and keep[4] and not keep[5] and not keep[6]
    assert ((btype != 0) & (t >= start) & (t <= end)).sum() >= 10 and keep[10] and keep[200] and not keep[390]
    assert not keep[user == 199999].any() and (user == 199999).sum() == 3
    out = os.path.join(HERE, "g11_taobao_remap.npz")
    np.savez_compressed(out, raw=raw, start_end=np.asarray([start, end, day], dtype=np.int64), remapped=remapped, item_feat=item_feat)
    print(out, os.path.getsize(out), "bytes;", len(remapped), "of", n, "events kept;", len(item_feat), "items")


if __name__ == "__main__":
    main()
