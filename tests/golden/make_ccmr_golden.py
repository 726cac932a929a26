"""G12: CCMR's first offline step and its target rule on a small synthetic rating log, decided by the REFERENCE's own code:
code/feateng_ccmr.py pos_neg_split, time2idx, remap_ids, gen_user_neg and code/gen_target.py
TargetGen.gen_user_item_hist_dict_ccmr and gen_target_file for three prediction times in the reference's order (largest
first) on ONE TargetGen, whose user_neg_dict therefore carries the random pads from one split to the next.  Commits only data:
the raw log and movie_info as integer arrays, the two halves and the slice of every event, the movie dictionary, the
user_neg_dict, the history dictionaries and, per split, the users, positives and negatives of the lines.

The log is written as the CSV files those functions read.  The module constants (USER_NUM, ..., START_TIME stays the
reference's 1116432000) are set on the imported modules; the time zone is set to UTC+8 with the POSIX string "CST-8", which
needs no zone files; matplotlib and pymongo, imported at the top of the reference's modules and not needed by these functions,
are stubbed in sys.modules.  The TargetGen object is made with __new__ and given fake collections (documents {'uid', '1hop':
one list per slice} from the reference's own remapped positive file), so no database client is opened.

Run (where the reference is checked out):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ccmr_golden.py <reference>/code"""
import datetime
import os
import pickle
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
U, I, VOCAB, S, NEG = 60, 40, (7, 9, 4, 5), 6, 5
PREDS = (4, 3, 2)                               # the reference's order: the largest first
START = datetime.date(2005, 5, 19)


class Coll(object):
    """what TargetGen reads of a collection: find({}) -> the documents"""

    def __init__(self, docs):
        self.docs = docs

    def find(self, query):
        return iter(self.docs)


def make_log(rng):
    """[n, 4] raw user, raw item, rating, YYYYMMDD and [m, 5] movie_info; item I - 1 is rated only negatively and has no line"""
    ev = []
    for _ in range(420):                                           # positives, days -200 .. 90 * S - 1
        ev.append((int(rng.integers(0, U)), int(rng.integers(0, I - 1)), int(rng.integers(4, 6)), int(rng.integers(-200, 90 * S))))
    for d in (-1, -89, -90, -91, 0, 89, 90):                       # both sides of the start and of the first slice edge
        ev.append((int(rng.integers(0, U)), int(rng.integers(0, I - 1)), 5, d))
    counts = [0, 2, NEG, NEG + 3, 1, NEG - 1, NEG + 1, 0, 3, NEG]  # negative events per user, cycled over the users
    for u in range(U):
        k = counts[u % len(counts)]
        items = [int(rng.integers(0, I)) for _ in range(k)]
        if k >= 2 and u % 3 == 0:
            items[1] = items[0]                                    # a duplicate
        for it in items:
            ev.append((u, it, int(rng.integers(1, 4)), int(rng.integers(-200, 90 * S))))
    ev.append((1, I - 1, 2, 17))
    ev = [ev[j] for j in rng.permutation(len(ev))]
    date = lambda d: int((START + datetime.timedelta(days=d)).strftime("%Y%m%d"))
    log = np.asarray([(u, i, r, date(d)) for u, i, r, d in ev], dtype=np.int64)
    lines = []
    for i in rng.permutation(I - 1).tolist():
        f = [int(rng.integers(0, v - 1)) if rng.random() > 0.25 else -1 for v in VOCAB]
        lines.append([i] + f)
    for i in (3, 11, 20):                                          # a second line with other features: the first wins
        lines.append([i] + [(lines[[l[0] for l in lines].index(i)][1 + k] + 2) % (VOCAB[k] - 1) for k in range(4)])
    return log, np.asarray(lines, dtype=np.int64)


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "feateng_ccmr.py")):
        raise SystemExit("usage: make_ccmr_golden.py <reference>/code")
    os.environ["TZ"] = "CST-8"
    time.tzset()
    mpl = types.ModuleType("matplotlib")
    mpl.use = lambda *a, **k: None
    sys.modules.setdefault("matplotlib", mpl)
    sys.modules.setdefault("matplotlib.pyplot", types.ModuleType("matplotlib.pyplot"))
    sys.modules.setdefault("pymongo", types.ModuleType("pymongo"))
    sys.path.insert(0, sys.argv[1])
    import feateng_ccmr as fc
    import gen_target as gt
    fc.USER_NUM, fc.ITEM_NUM = U, I
    fc.DIRECTOR_NUM, fc.ACTOR_NUM, fc.GENRE_NUM, fc.NATION_NUM = VOCAB
    assert fc.START_TIME == 1116432000 and fc.TIME_DELTA == 90 and gt.START_TIME_CCMR == 1116432000

    log, movie = make_log(np.random.Generator(np.random.PCG64(12)))
    n = len(log)
    # what the log must hold
    day = np.asarray([(datetime.date(v // 10000, v // 100 % 100, v % 100) - START).days for v in log[:, 3].tolist()])
    assert set(log[:, 2].tolist()) == {1, 2, 3, 4, 5}
    assert ((day < 0) & (day > -90)).any() and (day <= -90).any() and {-1, -89, -90, -91, 0, 89, 90} <= set(day.tolist())
    is_pos = log[:, 2] >= 4
    negs_of = np.bincount(log[~is_pos, 0], minlength=U)
    assert (np.bincount(movie[:, 0], minlength=I) == 2).sum() == 3 and all((movie[:, 1 + k] == -1).any() for k in range(4))

    blob = {"log": log, "movie_info": movie, "dims": np.asarray([U, I, S, NEG] + list(VOCAB) + list(PREDS), dtype=np.int32)}
    with tempfile.TemporaryDirectory() as d:
        p = lambda name: os.path.join(d, name)
        iso = lambda v: "%04d-%02d-%02d" % (v // 10000, v // 100 % 100, v % 100)
        with open(p("rating_logs.csv"), "w") as f:
            f.write("user,item,rating,time\n" + "".join("%d,%d,%d,%s\n" % (a, b, c, iso(v)) for a, b, c, v in log.tolist()))
        field = lambda x, k: "" if x < 0 else "%d;%d" % (x, (x + 1) % (VOCAB[k] - 1)) if x % 2 else "%d" % x     # (multi-valued: the first counts)
        with open(p("movie_info.csv"), "w") as f:
            f.write("".join("%d,%s,x\n" % (l[0], ",".join(field(l[1 + k], k) for k in range(4))) for l in movie.tolist()))
        fc.pos_neg_split(p("rating_logs.csv"), p("rating_pos.csv"), p("rating_neg.csv"))
        fc.time2idx(p("rating_pos.csv"), p("rating_pos_idx.csv"))
        fc.time2idx(p("rating_neg.csv"), p("rating_neg_idx.csv"))
        fc.remap_ids(p("rating_pos_idx.csv"), p("remap_pos.csv"), p("movie_info.csv"), p("movie.pkl"))
        fc.remap_ids(p("rating_neg_idx.csv"), p("remap_neg.csv"))
        fc.gen_user_neg(p("remap_neg.csv"), p("user_neg_dict.pkl"))
        # the halves: the log positions of the raw lines each file kept, and the reference's remapped columns
        raw_lines = open(p("rating_logs.csv")).read().splitlines()[1:]
        for tag in ("pos", "neg"):
            kept = open(p("rating_%s.csv" % tag)).read().splitlines()
            at, q = [], 0
            for l in kept:                                         # (both files keep the log order)
                while raw_lines[q] != l:
                    q += 1
                at.append(q)
                q += 1
            rows = np.asarray([[int(x) for x in l.split(",")] for l in open(p("remap_%s.csv" % tag)).read().splitlines()])
            blob[tag + "_at"], blob[tag + "_uid"], blob[tag + "_iid"], blob[tag + "_t"] = (np.asarray(at), rows[:, 0], rows[:, 1],
                                                                                           rows[:, 3])
        assert len(blob["pos_at"]) + len(blob["neg_at"]) == n
        with open(p("movie.pkl"), "rb") as f:
            md = pickle.load(f)
        keys = sorted(md, key=int)
        blob["movie_keys"] = np.asarray([int(k) for k in keys])
        blob["movie_vals"] = np.asarray([md[k] for k in keys])
        with open(p("user_neg_dict.pkl"), "rb") as f:
            und = pickle.load(f)
        keys = sorted(und, key=int)
        blob["und_users"] = np.asarray([int(k) for k in keys])
        blob["und_off"] = np.cumsum([0] + [len(und[k]) for k in keys])
        blob["und_items"] = np.asarray([int(x) for k in keys for x in und[k]])

        tg = gt.TargetGen.__new__(gt.TargetGen)
        with open(p("user_neg_dict.pkl"), "rb") as f:
            tg.user_neg_dict = pickle.load(f)
        tg.user_num, tg.item_num = U, I
        tg.start_time, tg.start_time_idx, tg.time_delta = gt.START_TIME_CCMR, gt.START_TIME_IDX_CCMR, gt.TIME_DELTA_CCMR
        cells = [[[] for _ in range(S)] for _ in range(U)]
        for u, i, t in zip(blob["pos_uid"].tolist(), blob["pos_iid"].tolist(), blob["pos_t"].tolist()):
            if 0 <= t < S:
                cells[u - 1][t].append(i)
        users = [{"uid": u + 1, "1hop": cells[u]} for u in range(U)]
        tg.user_colls = [Coll(users[:U // 2]), Coll(users[U // 2:])]
        for pt in PREDS:
            tg.gen_user_item_hist_dict_ccmr(p("rating_pos.csv"), p("uh%d.pkl" % pt), p("ih%d.pkl" % pt), pt)
            for side, name in (("user", "uh"), ("item", "ih")):
                with open(p("%s%d.pkl" % (name, pt)), "rb") as f:
                    h = pickle.load(f)
                keys = sorted(h, key=int)
                blob["%s_hist%d_keys" % (side, pt)] = np.asarray([int(k) for k in keys])
                blob["%s_hist%d_off" % (side, pt)] = np.cumsum([0] + [len(h[k]) for k in keys])
                blob["%s_hist%d_vals" % (side, pt)] = np.asarray([int(x) for k in keys for x in h[k]])
        for pt in PREDS:                                           # ONE TargetGen: its dict keeps the pads of the split before
            tg.gen_target_file(NEG, p("target.txt"), p("uh%d.pkl" % pt), pt, None)
            rows = np.asarray([[int(x) for x in l.strip().split(",")] for l in open(p("target.txt"))], dtype=np.int32)
            assert rows.shape[1] == 2 + NEG and len(rows) >= 5
            blob["lines%d_users" % pt], blob["lines%d_pos" % pt], blob["lines%d_neg" % pt] = rows[:, 0], rows[:, 1], rows[:, 2:]
    lined = set(blob["lines%d_users" % PREDS[0]].tolist())
    own = {u: negs_of[u - 1] for u in lined}
    assert 0 in own.values() and NEG in own.values() and any(0 < v < NEG for v in own.values()) and any(v > NEG for v in own.values())
    everywhere = set().union(*[set(blob["lines%d_users" % pt].tolist()) for pt in PREDS])
    assert any(negs_of[u] and (u + 1) not in everywhere for u in range(U))              # negatives and no line
    o, it = blob["und_off"], blob["und_items"]
    assert any(len(set(it[o[k]:o[k + 1]].tolist())) < o[k + 1] - o[k] for k in range(len(o) - 1))     # duplicate negatives
    assert (blob["pos_t"] < 0).any() and (blob["pos_t"] == 0).any()
    blob = {k: np.asarray(v).astype(np.int32) if k != "log" and k != "movie_info" else v for k, v in blob.items()}
    out = os.path.join(HERE, "g12_ccmr.npz")
    np.savez_compressed(out, **blob)
    print(out, os.path.getsize(out), "bytes;", n, "events;", [len(blob["lines%d_users" % pt]) for pt in PREDS], "lines")


if __name__ == "__main__":
    main()
