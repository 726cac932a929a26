"""G10: who gets a target line, its positive, and the popular-item list, on a small synthetic Tmall-style log, decided by the
REFERENCE's own code: code/gen_target.py TargetGen.gen_user_item_hist_dict_tmall (the history dictionary), gen_target_file
(lines, without and with a pop list) and gen_pop_items.  Commits only data: the remapped integer columns of the log, the
users and positives of the lines, the negatives the reference drew (Python's `random`: pinned by the test only as count and
range) and the pop lists.

The TargetGen object is made with __new__ and given fake collections -- lists of documents {'uid' | 'iid', '1hop': one list
per slice} made from the log-order 1-hop lists of TemporalGraph.from_log --, so no database client is opened.  The log is
remapped by score_amd.dataprep.remap_tmall_log and handed to the reference as its remap dictionaries.

The log holds users with a slice-PRED event and no history, users whose earlier events all lie before START, users with a
history and no slice-PRED event, and users with several slice-PRED events.

Run (where the reference is checked out):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_target_golden.py <reference>/code"""
import datetime
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
START, PRED, S, NEG = 1, 4, 6, 5
POP = ((5, None), (6, None), (5, "mid"))        # (pop_standard, max_iid)


class Coll(object):
    """what TargetGen reads of a collection: find({}) -> the documents"""

    def __init__(self, docs):
        self.docs = docs

    def find(self, query):
        return iter(self.docs)


def mmdd(day):
    d = datetime.date(2015, 5, 1) + datetime.timedelta(days=int(day))
    return d.month * 100 + d.day


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "gen_target.py")):
        raise SystemExit("usage: make_target_golden.py <reference>/code")
    sys.path.insert(0, sys.argv[1])
    import gen_target as gt
    from score_amd import dataprep as dp
    from score_amd.graph import TemporalGraph
    rng = np.random.Generator(np.random.PCG64(10))
    n = 700
    ev = np.stack([3000 + rng.integers(0, 120, n), 7000 + rng.integers(0, 60, n), rng.integers(0, 15 * S, n)], axis=1)
    days = np.asarray([mmdd(d) for d in ev[:, 2]], dtype=np.int64)
    raw = np.stack([ev[:, 0], ev[:, 1], ev[:, 1] % 7, ev[:, 1] % 5, ev[:, 1] % 3, days], axis=1)
    r = dp.remap_tmall_log(raw)
    uid, iid, t_idx, U, I = r["uid"], r["iid"], r["t_idx"], r["n_users"], r["n_items"]
    assert t_idx.max() == S - 1
    g = TemporalGraph.from_log(uid, iid, t_idx, U, I, S, r["user_rows"], r["item_rows"], max_1hop=10 ** 6, max_2hop=10 ** 6)
    cells = lambda side, e: [g.cell(side, 1, e, t).tolist() for t in range(S)]          # (no cap hit: log order)
    tg = gt.TargetGen.__new__(gt.TargetGen)
    tg.user_neg_dict, tg.user_num, tg.item_num = {}, U, I
    tg.start_time, tg.start_time_idx, tg.time_delta = gt.START_TIME_Tmall, START, gt.TIME_DELTA_Tmall
    # two collections per side, as the reference shards them; a scan visits them in order
    users = [{"uid": u + 1, "1hop": cells("user", u)} for u in range(U)]
    items = [{"iid": U + 1 + i, "1hop": cells("item", i)} for i in range(I)]
    tg.user_colls = [Coll(users[:U // 2]), Coll(users[U // 2:])]
    tg.item_colls = [Coll(items[:I // 3]), Coll(items[I // 3:])]
    blob = {"uid": uid, "iid": iid, "t_idx": t_idx, "dims": np.asarray([U, I, S, START, PRED, NEG], dtype=np.int32)}
    with tempfile.TemporaryDirectory() as d:
        p = lambda name: os.path.join(d, name)
        with open(p("joined.csv"), "w") as f:
            f.write("header\n" + "".join("%d,%d,0,0,0,%04d,0,0,0\n" % (a, b, c) for a, b, c in zip(raw[:, 0], raw[:, 1], days)))
        with open(p("remap.pkl"), "wb") as f:
            pickle.dump({str(int(a)): str(int(b)) for a, b in zip(raw[:, 0], uid)}, f)
            pickle.dump({str(int(a)): str(int(b)) for a, b in zip(raw[:, 1], iid)}, f)
        tg.gen_user_item_hist_dict_tmall(p("joined.csv"), p("uh.pkl"), p("ih.pkl"), p("remap.pkl"), PRED)
        for k, (standard, max_iid) in enumerate(POP):
            max_iid = 1 + U + I if max_iid is None else U + I // 2
            tg.gen_pop_items(p("pop%d.pkl" % k), standard, max_iid)
            with open(p("pop%d.pkl" % k), "rb") as f:
                blob["pop%d" % k] = np.asarray([int(x) for x in pickle.load(f)], dtype=np.int32)
            blob["pop%d_args" % k] = np.asarray([standard, max_iid], dtype=np.int32)
        assert 0 < len(blob["pop1"]) < len(blob["pop0"]) and 0 < len(blob["pop2"]) < len(blob["pop0"])
        for tag, pop_file in (("plain", None), ("pop", p("pop1.pkl"))):
            tg.gen_target_file(NEG, p("target.txt"), p("uh.pkl"), PRED, pop_file)
            rows = np.asarray([[int(x) for x in l.strip().split(",")] for l in open(p("target.txt"))], dtype=np.int32)
            blob[tag + "_users"], blob[tag + "_pos"], blob[tag + "_neg"] = rows[:, 0], rows[:, 1], rows[:, 2:]
    lu = blob["plain_users"]
    at = set(uid[t_idx == PRED].tolist())
    hist = set(uid[(t_idx >= START) & (t_idx < PRED)].tolist())
    early = set(uid[t_idx < START].tolist())
    assert set(lu.tolist()) == at & hist and (at - hist) and ((at & early) - hist) and (hist - at)
    assert max(np.bincount(uid[t_idx == PRED])) >= 3
    out = os.path.join(HERE, "g10_targets.npz")
    np.savez_compressed(out, **blob)
    print(out, os.path.getsize(out), "bytes;", len(lu), "lines; pop lists", [len(blob["pop%d" % k]) for k in range(len(POP))])


if __name__ == "__main__":
    main()
