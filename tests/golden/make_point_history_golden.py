"""G9: the point baselines' whole data chain on a small synthetic Tmall-style log, run with the REFERENCE's own code:
code/gen_target.py TargetGen.gen_user_item_hist_dict_tmall (the history dictionaries), code/gen_history_point.py
gen_user_hist_seq_file / gen_item_hist_seq_file (the history files) and code/point_models/data_loader.py DataLoaderUserSeq /
DataLoaderDualSeq (the batches).  Commits only data: the remapped integer columns of the log, the target lines, the feature
tables, the lines of both history files and the batches of both loaders at two max_len.

The TargetGen object is made with __new__ and given only start_time, start_time_idx and time_delta, so no database client is
opened.  The log is remapped by score_amd.dataprep.remap_tmall_log (first-appearance order; the reference's own order depends
on the process's string hashing) and handed to the reference as its remap dictionaries; the maker asserts that
dataprep.tmall_slice_index selects, user by user, the events the reference's time_idx selected.

Cases (hist_max_len H = 6, max_len T in {4, 7}):
  several events per day per entity, written out of time order; events before start_time and at or after pred_time;
  histories of 1, 3, 4, 5, 6, 7 and 8 events on both sides (1, T - 1, T, T + 1, H, H + 1 for both T);
  candidate items without history, one of them as a line's last item; the highest user id and the highest item id with one;
  'neg1': 1 negative and two more items on every line; 'neg99': 99 negatives, and 100 * 7 * Fu > 8192 words (the item side
  of a line does not fit the assembly kernel's LDS in one piece); both target files end inside a batch;
  Fu, Fi odd, so that T * Fu and T * Fi are odd at T = 7: spans start off a 16-byte boundary.
The feature dictionaries carry a key '0' with zeros: the reference's loader looks it up for the stand-in history '0' of an
item without one.

Run (where the reference is checked out):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_point_history_golden.py <reference>/code"""
import datetime
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
H, TS = 6, (4, 7)
EDGE = (1, 3, 4, 5, 6, 7, 8)
START, PRED = 1, 5            # slices 1 .. 4 count: days 15 .. 74 after 2015-05-01
# tag: (batch_size, neg_sample_num, items on a target line, target lines, Fu, Fi)
CASES = {"neg1": (8, 1, 4, 18, 3, 5), "neg99": (200, 99, 100, 5, 13, 3)}
SINGLE = ("user_seq", "user_seq_length", "target_user", "target_item", "label")
DUAL = ("user_seq", "user_seq_length", "item_seq", "item_seq_length", "target_user", "target_item", "label")


def mmdd(day):
    d = datetime.date(2015, 5, 1) + datetime.timedelta(days=int(day))
    return d.month * 100 + d.day


def make_log(rng, n_fill_users, n_fill_items):
    """raw (user, item, day) events: 'edge' users / items with exactly EDGE[k] events inside the window (and some outside),
    filler entities with random ones, entities seen only outside the window, all shuffled; the last event introduces a new
    user and a new item inside the window (they get the highest ids)"""
    inside = lambda n: rng.choice([16, 17, 30, 31, 44, 59, 60, 74], n)          # few days: ties are the rule
    outside = lambda n: rng.choice([0, 3, 14, 75, 76, 89], n)
    fill_u = 1000 + np.arange(n_fill_users)
    fill_i = 5000 + np.arange(n_fill_items)
    ev = []
    for k, n in enumerate(EDGE):
        ev += [(2000 + k, int(i), int(d)) for i, d in zip(rng.choice(fill_i[: n_fill_items // 2], n), inside(n))]
        ev += [(2000 + k, int(i), int(d)) for i, d in zip(rng.choice(fill_i, 2), outside(2))]
        # (the edge items draw their users from the SECOND half of the fillers, the edge users their items from the first: an
        #  edge entity's count is exactly EDGE[k])
        ev += [(int(u), 6000 + k, int(d)) for u, d in zip(rng.choice(fill_u[n_fill_users // 2:], n), inside(n))]
        ev += [(int(u), 6000 + k, int(d)) for u, d in zip(rng.choice(fill_u, 2), outside(2))]
    for u in fill_u[: n_fill_users // 2]:
        n = int(rng.integers(0, 10))
        ev += [(int(u), int(i), int(d)) for i, d in zip(rng.choice(fill_i[n_fill_items // 2:], n), inside(n))]
    for k in range(6):           # items (and users) that exist only outside the window
        ev += [(3000 + k, 7000 + k, int(d)) for d in outside(2)]
        ev += [(int(rng.choice(fill_u)), 7000 + k, int(outside(1)[0]))]
    ev = [ev[j] for j in rng.permutation(len(ev))]
    ev.append((3999, 7999, 44))
    return np.asarray(ev, dtype=np.int64)


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "gen_history_point.py")):
        raise SystemExit("usage: make_point_history_golden.py <reference>/code")
    sys.path.insert(0, sys.argv[1])
    sys.path.insert(0, os.path.join(sys.argv[1], "point_models"))
    import data_loader as dl
    import gen_history_point as ghp
    import gen_target as gt
    from score_amd import dataprep as dp
    rng = np.random.Generator(np.random.PCG64(9))
    blob = {"tags": np.array(sorted(CASES)), "hist_max_len": np.int32(H), "max_lens": np.asarray(TS, dtype=np.int32),
            "window": np.asarray([START, PRED], dtype=np.int32)}
    for tag in sorted(CASES):
        B, neg, n_on_line, n_lines, Fu, Fi = CASES[tag]
        ev = make_log(rng, 24, 40 if tag == "neg1" else 150)
        days = np.asarray([mmdd(d) for d in ev[:, 2]], dtype=np.int64)
        raw = np.stack([ev[:, 0], ev[:, 1], ev[:, 1] % 7, ev[:, 1] % 5, ev[:, 1] % 3, days], axis=1)
        r = dp.remap_tmall_log(raw)
        uid, iid, t_idx, U, I = r["uid"], r["iid"], r["t_idx"], r["n_users"], r["n_items"]
        assert uid[-1] == U and iid[-1] == U + I and START <= t_idx[-1] < PRED       # the highest ids carry a history
        user_rows = np.concatenate([np.arange(1, U + 1)[:, None], rng.integers(U + I + 1, U + I + 50, (U, Fu - 1))], axis=1)
        item_rows = np.concatenate([np.arange(U + 1, U + I + 1)[:, None], rng.integers(U + I + 50, U + I + 99, (I, Fi - 1))], axis=1)
        inwin = (t_idx >= START) & (t_idx < PRED)
        ucount = np.bincount(uid[inwin], minlength=U + I + 1)
        icount = np.bincount(iid[inwin], minlength=U + I + 1)
        assert set(EDGE) <= set(ucount[1:U + 1].tolist()) and set(EDGE) <= set(icount[U + 1:].tolist())
        # target lines: every user with a history in turn (the edge users and the highest id among them); items drawn from
        # all items, the edge items, the highest item and the history-less ones forced in
        with_hist = [u for u in range(1, U + 1) if ucount[u]]
        edge_users = [int(np.flatnonzero(ucount[:U + 1] == n)[0]) for n in EDGE] + [U]
        edge_items = [int(U + 1 + np.flatnonzero(icount[U + 1:] == n)[0]) for n in EDGE] + [U + I]
        bare = [int(i) for i in range(U + 1, U + I + 1) if not icount[i]]
        assert len(bare) >= 6 and len(with_hist) > len(edge_users)
        order = edge_users + [u for u in with_hist if u not in edge_users]
        lines = []
        for l in range(n_lines):
            items = [int(x) for x in rng.choice(np.arange(U + 1, U + I + 1), n_on_line, replace=I < n_on_line)]
            if neg == 1:         # the used items (columns 0, 1) take the edge items in turn; a bare one among them and last
                items[l % 2] = edge_items[l % len(edge_items)]
                if l % 3 == 0:
                    items[1 - l % 2] = bare[l % len(bare)]
                if l % 4 == 1:
                    items[-1] = bare[(l + 1) % len(bare)]
            else:
                items[:len(edge_items)] = edge_items[l % 2:] + edge_items[:l % 2]
                items[20], items[95] = bare[l], bare[l + 1]                # (95: behind the chunk seam at sample 90)
                if l % 2 == 0:
                    items[-1] = bare[2]
            lines.append((order[l % len(order)], items))
        assert n_lines % (B // (1 + neg)) != 0                               # the file ends inside a batch
        with tempfile.TemporaryDirectory() as d:
            p = lambda n: os.path.join(d, n)
            # the reference's inputs: the joined log (header + 'uid,iid,cid,sid,bid,date,btype,aid,gid') and the remap dicts
            with open(p("joined.csv"), "w") as f:
                f.write("header\n" + "".join("%d,%d,0,0,0,%04d,0,0,0\n" % (a, b, c) for a, b, c in zip(raw[:, 0], raw[:, 1], days)))
            with open(p("remap.pkl"), "wb") as f:
                pickle.dump({str(int(a)): str(int(b)) for a, b in zip(raw[:, 0], uid)}, f)
                pickle.dump({str(int(a)): str(int(b)) for a, b in zip(raw[:, 1], iid)}, f)
            tg = gt.TargetGen.__new__(gt.TargetGen)
            tg.start_time, tg.start_time_idx, tg.time_delta = gt.START_TIME_Tmall, START, gt.TIME_DELTA_Tmall
            tg.gen_user_item_hist_dict_tmall(p("joined.csv"), p("uh.pkl"), p("ih.pkl"), p("remap.pkl"), PRED)
            with open(p("uh.pkl"), "rb") as f:
                uh = pickle.load(f)
            for u in range(1, U + 1):      # tmall_slice_index selects the events the reference's time_idx selected
                assert sorted(int(x) for x in uh.get(str(u), [])) == sorted(iid[inwin & (uid == u)].tolist()), u
            tf, _, _, uf, itf = dp.write_point_files(d, lines, [], [], user_rows, item_rows)
            ghp.gen_user_hist_seq_file(tf, p("user_hist.txt"), p("uh.pkl"), H)
            ghp.gen_item_hist_seq_file(tf, p("item_hist.txt"), p("ih.pkl"), H)
            user_hist = [l[:-1] for l in open(p("user_hist.txt"))]
            item_hist = [l[:-1] for l in open(p("item_hist.txt"))]
            ulen = [len(l.split(",")) for l in user_hist]
            ilen = [len(s.split(",")) for l in item_hist for s in l.split("\t")[:1 + neg]]
            assert {1, 3, 4, 5, 6} <= set(ulen) and max(ulen) == H and {1, 3, 4, 5, 6} <= set(ilen) and max(ilen) == H
            assert any(l.split("\t")[-1] == "0" for l in item_hist) and any("0" in l.split("\t")[:1 + neg] for l in item_hist)
            for T in TS:
                for form, fields, loader in (("single", SINGLE, dl.DataLoaderUserSeq(B, T, tf, p("user_hist.txt"), neg, uf, itf)),
                                             ("dual", DUAL, dl.DataLoaderDualSeq(B, T, tf, p("user_hist.txt"), p("item_hist.txt"),
                                                                                 neg, uf, itf))):
                    batches = list(loader)
                    assert len(batches) == n_lines // (B // (1 + neg)) > 0
                    blob["%s/n_batches" % tag] = np.int32(len(batches))
                    for i, b in enumerate(batches):
                        for nm, x in zip(fields, b):
                            blob["%s/T%d/%s/b%d/%s" % (tag, T, form, i, nm)] = np.asarray(x, dtype=np.int32)
        blob[tag + "/cfg"] = np.asarray([B, neg], dtype=np.int32)
        blob[tag + "/uid"], blob[tag + "/iid"], blob[tag + "/t_idx"] = uid, iid, t_idx
        blob[tag + "/time_key"] = days.astype(np.int32)
        blob[tag + "/target"] = np.asarray([[u] + items for u, items in lines], dtype=np.int32)
        blob[tag + "/user_rows"], blob[tag + "/item_rows"] = user_rows.astype(np.int32), item_rows.astype(np.int32)
        blob[tag + "/user_hist"], blob[tag + "/item_hist"] = np.array(user_hist), np.array(item_hist)
    out = os.path.join(HERE, "g9_point_history.npz")
    np.savez_compressed(out, **blob)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
