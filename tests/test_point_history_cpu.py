"""The point baselines' histories from the interaction log, without a GPU (score_amd/dataprep.py: point_history_lines,
write_point_files; score_amd/pointdata.py: PointLogStore(build="host")).  The yardstick is tests/golden/g9_point_history.npz:
what the reference's own chain -- gen_target.py's history dictionaries, gen_history_point.py's files, data_loader.py's loaders
-- produced from the recorded log and target lines (tests/golden/make_point_history_golden.py).  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import point_hist_cases as phc
from helpers import GOLDEN
from score_amd import dataprep as dp
from score_amd.pointdata import DataLoaderDualSeq, DataLoaderUserSeq, PointLogStore, host_hist_csr

SINGLE = ("user_seq", "user_seq_length", "target_user", "target_item", "label")
DUAL = ("user_seq", "user_seq_length", "item_seq", "item_seq_length", "target_user", "target_item", "label")


def load_case(z, tag):
    """a g9 case: the log's columns, the target lines, the tables, the window and the loaders' arguments"""
    c = {k: z["%s/%s" % (tag, k)] for k in ("uid", "iid", "time_key", "t_idx", "user_rows", "item_rows", "user_hist", "item_hist")}
    c["lines"] = [(int(r[0]), [int(x) for x in r[1:]]) for r in z[tag + "/target"]]
    c["B"], c["neg"] = (int(x) for x in z[tag + "/cfg"])
    c["start"], c["pred"] = (int(x) for x in z["window"])
    c["H"], c["Ts"], c["n_batches"] = int(z["hist_max_len"]), [int(t) for t in z["max_lens"]], int(z[tag + "/n_batches"])
    return c


def log_store(c, dual, build="host", **kw):
    a = dict(c, **kw)
    return PointLogStore(a["uid"], a["iid"], a["time_key"], a["t_idx"], a["lines"], a["start"], a["pred"], a["H"], a["neg"], a["B"],
                         a["user_rows"], a["item_rows"], dual, build=build)


def _window(off, seq, ln, e, T, rows, row_lo):
    """[T, F]: the last min(len, T) ids of entity e's segment, the last one repeated; no history (or no such entity): [0]"""
    ids = seq[off[e + 1] - min(int(ln[e]), T):off[e + 1]] if 0 <= e < len(ln) else seq[:0]
    ids = np.concatenate([ids, np.repeat(ids[-1:], T - len(ids))]) if len(ids) else np.zeros(T, dtype=np.int64)
    out = rows[np.maximum(ids - row_lo, 0)].copy()
    out[ids == 0] = 0
    return out


def rebuild_batch(st, a, b, T):
    """batch b of a PointLogStore (its arrays `a` as numpy) at max_len T as the host loaders' tuple"""
    per, lpb, U = st.per_line, st.lines_per_batch, st.n_users
    lines = np.repeat(np.arange(b * lpb, (b + 1) * lpb), per)
    samples = np.arange(b * lpb * per, (b + 1) * lpb * per)
    users, items = st.line_user[lines].astype(np.int64), st.line_items[samples].astype(np.int64)
    out = [np.stack([_window(a["user_hist_off"], a["user_hist_seq"], a["user_hist_len"], u - 1, T, st.item_rows, U + 1) for u in users]),
           a["user_hist_len"][users - 1]]
    tu = users
    if st.dual:
        off, seq, ln = a["item_hist_off"], a["item_hist_seq"], a["item_hist_len"]
        out += [np.stack([_window(off, seq, ln, i - 1 - U, T, st.user_rows, 1) for i in items]), np.maximum(ln[items - 1 - U], 1)]
        last = st.line_last_item[lines].astype(np.int64) - 1 - U
        tu = np.where(ln[last] > 0, seq[np.maximum(off[last + 1] - 1, 0)], 0)       # (the reference's rebinding of `uid`)
    urows = st.user_rows[np.maximum(tu - 1, 0)].copy()
    urows[tu == 0] = 0
    out += [urows, st.item_rows[items - 1 - U], (samples % per == 0).astype(np.int32)]
    return tuple(out)


@pytest.fixture(scope="module")
def g9():
    z = np.load(os.path.join(GOLDEN, "g9_point_history.npz"))
    tags = [str(t) for t in z["tags"]]
    assert tags == ["neg1", "neg99"]
    return z, {t: load_case(z, t) for t in tags}


@pytest.mark.parametrize("tag", ["neg1", "neg99"])
def test_history_lines_equal_the_reference_files(g9, tag):
    c = g9[1][tag]
    users, items = dp.point_history_lines(c["uid"], c["iid"], c["time_key"], c["t_idx"], c["lines"], c["start"], c["pred"], c["H"])
    assert users == [str(l) for l in c["user_hist"]]
    assert items == [str(l) for l in c["item_hist"]]
    # the cases the fixture is there for: ties written out of time order, both window edges, the cut at H, bare items
    inwin = (c["t_idx"] >= c["start"]) & (c["t_idx"] < c["pred"])
    assert (c["t_idx"] < c["start"]).any() and (c["t_idx"] >= c["pred"]).any()
    assert (np.diff(c["time_key"][inwin]) < 0).any() and len(np.unique(c["time_key"][inwin])) < inwin.sum() // 4
    assert np.bincount(c["uid"][inwin]).max() > c["H"] and np.bincount(c["iid"][inwin]).max() > c["H"]
    assert any(l.split("\t")[-1] == "0" for l in items)


@pytest.mark.parametrize("tag", ["neg1", "neg99"])
def test_host_loaders_over_the_written_files_equal_the_reference_batches(g9, tag, tmp_path):
    z, c = g9[0], g9[1][tag]
    users, items = dp.point_history_lines(c["uid"], c["iid"], c["time_key"], c["t_idx"], c["lines"], c["start"], c["pred"], c["H"])
    tf, uf, itf, ud, idd = dp.write_point_files(str(tmp_path), c["lines"], users, items, c["user_rows"], c["item_rows"])
    for T in c["Ts"]:
        for form, fields, loader in (("single", SINGLE, DataLoaderUserSeq(c["B"], T, tf, uf, c["neg"], ud, idd)),
                                     ("dual", DUAL, DataLoaderDualSeq(c["B"], T, tf, uf, itf, c["neg"], ud, idd))):
            got = list(loader)
            assert len(got) == c["n_batches"]
            for i, b in enumerate(got):
                for nm, x in zip(fields, b):
                    assert np.array_equal(x, z["%s/T%d/%s/b%d/%s" % (tag, T, form, i, nm)]), (T, form, i, nm)


@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("tag", ["neg1", "neg99"])
def test_host_store_rebuilds_the_reference_batches(g9, tag, dual):
    z, c = g9[0], g9[1][tag]
    st = log_store(c, dual)
    a = st.arrays()
    per = 1 + c["neg"]
    assert st.n_batches == c["n_batches"] > 0 and st.n_lines == st.n_batches * (c["B"] // per) < len(c["lines"])
    assert (a["item_hist_off"] is not None) == dual
    assert a["user_hist_off"][-1] == len(a["user_hist_seq"]) == ((c["t_idx"] >= c["start"]) & (c["t_idx"] < c["pred"])).sum()
    assert a["user_hist_len"].max() == c["H"] < np.diff(a["user_hist_off"]).max()
    assert a["user_hist_len"][-1] > 0 and (not dual or a["item_hist_len"][-1] > 0)          # the highest ids carry a history
    form, fields = ("dual", DUAL) if dual else ("single", SINGLE)
    for T in c["Ts"]:                                                                      # one store, both max_len
        lens = []
        for b in range(st.n_batches):
            got = rebuild_batch(st, a, b, T)
            for nm, x in zip(fields, got):
                want = z["%s/T%d/%s/b%d/%s" % (tag, T, form, b, nm)]
                assert x.shape == want.shape and np.array_equal(x, want), (T, b, nm)
            lens.append([got[1]] + ([got[3]] if dual else []))
        assert st.batch_max_user_len.tolist() == [int(l[0].max()) for l in lens]
        assert st.batch_max_len.tolist() == [max(int(x.max()) for x in l) for l in lens]
        assert st.batch_min_len.tolist() == [min(int(x.min()) for x in l) for l in lens]
        st.check(c["B"], T, c["neg"], dual)
    if dual:
        seen = np.concatenate([z["%s/T4/dual/b%d/item_seq_length" % (tag, b)] for b in range(st.n_batches)])
        assert {1, 3, 4, 5, 6} <= set(seen.tolist())
        bare = a["item_hist_len"][st.line_items.astype(np.int64) - 1 - st.n_users] == 0
        assert bare.any() and (a["item_hist_len"][st.line_last_item.astype(np.int64) - 1 - st.n_users] == 0).any()
        if c["neg"] == 99:
            assert per * 7 * st.Fu > 8192 and bare.reshape(-1, per)[:, 8192 // (7 * st.Fu):].any()    # behind the chunk seam


def test_malformed_input_is_refused_at_build(g9):
    c = g9[1]["neg1"]
    U, I = len(c["user_rows"]), len(c["item_rows"])
    inwin = (c["t_idx"] >= c["start"]) & (c["t_idx"] < c["pred"])
    no_hist = int(np.setdiff1d(np.arange(1, U + 1), c["uid"][inwin])[0])
    bad = list(c["lines"])
    bad[5] = (no_hist, bad[5][1])
    with pytest.raises(ValueError, match="line 5"):                    # a user without history (the reference: exit(1))
        log_store(c, False, lines=bad)
    with pytest.raises(ValueError, match="line 5"):
        dp.point_history_lines(c["uid"], c["iid"], c["time_key"], c["t_idx"], bad, c["start"], c["pred"], c["H"])
    bad[5] = (no_hist, bad[5][1])
    log_store(c, False, lines=bad[:5] + bad[6:])                       # (and not a word without that line)
    for line in ((0, c["lines"][2][1]), (U + 1, c["lines"][2][1]), (1, [U] + c["lines"][2][1][1:]),
                 (1, c["lines"][2][1][:3] + [U + I + 1])):              # a target id outside its range, used or not
        lines = list(c["lines"])
        lines[2] = line
        with pytest.raises(ValueError, match="line 2"):
            log_store(c, True, lines=lines)
    with pytest.raises(ValueError):                                    # a log id outside its range
        log_store(c, False, iid=np.where(np.arange(len(c["iid"])) == 3, U, c["iid"]))
    with pytest.raises(ValueError):                                    # batch_size % (1 + neg_sample_num) != 0
        log_store(c, False, B=7)
    with pytest.raises(ValueError):
        log_store(c, False, build="file")
    with pytest.raises(ValueError):                                    # a table whose column 0 is not the id
        log_store(c, False, user_rows=c["user_rows"][::-1])
    # the store's own consistency check: batch_size, neg_sample_num, the form and T * F <= 8192; max_len is free otherwise
    st = log_store(c, True)
    st.check(c["B"], 50, c["neg"], True)
    st.check(c["B"], 8192 // max(st.Fu, st.Fi), c["neg"], True)
    for args in ((c["B"] * 2, 4, c["neg"], True), (c["B"], 4, 3, True), (c["B"], 4, c["neg"], False),
                 (c["B"], 8192 // max(st.Fu, st.Fi) + 1, c["neg"], True), (c["B"], 0, c["neg"], True)):
        with pytest.raises(ValueError):
            st.check(*args)


def test_device_loaders_refuse_a_log_store_with_other_arguments_before_any_device(g9):
    import torch
    from score_amd.pointdata import DeviceDataLoaderDualSeq, DeviceDataLoaderUserSeq
    c = g9[1]["neg1"]
    st, dual = log_store(c, False), log_store(c, True)
    with pytest.raises(ValueError):
        DeviceDataLoaderUserSeq(c["B"] * 2, 4, None, None, c["neg"], None, None, store=st)
    with pytest.raises(ValueError):
        DeviceDataLoaderUserSeq(c["B"], 4, None, None, c["neg"], None, None, store=dual)
    with pytest.raises(ValueError):
        DeviceDataLoaderDualSeq(c["B"], 4, None, None, None, c["neg"], None, None, store=st)
    with pytest.raises(ValueError):
        DeviceDataLoaderDualSeq(c["B"], 8192, None, None, None, c["neg"], None, None, store=dual)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):                               # matching arguments get as far as the device
            DeviceDataLoaderDualSeq(c["B"], 4, None, None, None, c["neg"], None, None, store=dual)
        with pytest.raises(RuntimeError):
            log_store(c, True, build="device")


def test_tmall_sample_stores_without_a_gpu():
    """the bundled sample through tmall_point_stores: the lines tmall_pipeline yields, histories cut at the reference's 300"""
    log = np.load(os.path.join(GOLDEN, "tmall_sample_log.npz"))["log"]
    stores, r = dp.tmall_point_stores(log, build="host", batch_size={"train": 20, "validation": 200, "test": 100})
    _, _, targets = dp.tmall_pipeline(log)
    for name, st in stores.items():
        assert st.dual and st.hist_max_len == 300 and st.neg_sample_num == (1 if name == "train" else 99)
        n = st.n_lines
        assert n == len(targets[name]) // st.lines_per_batch * st.lines_per_batch > 0
        assert st.line_user.tolist() == [u for u, _ in targets[name][:n]]
        assert st.line_items.tolist() == [i for _, items in targets[name][:n] for i in items]
        assert 1 <= st.batch_min_len.min() and st.batch_max_len.max() <= 300
    users, _ = dp.point_history_lines(r["uid"], r["iid"], log[:, 5], r["t_idx"], targets["test"], 0, dp.TMALL["pred_time_test"])
    a = stores["test"].arrays()
    for l, u in enumerate(stores["test"].line_user.tolist()):
        kept = a["user_hist_seq"][a["user_hist_off"][u] - a["user_hist_len"][u - 1]:a["user_hist_off"][u]]
        assert ",".join(str(x) for x in kept) == users[l]


def test_abi_entries_and_struct():
    from score_amd import _lib
    lib = _lib.load()
    for name in ("score_point_hist_build", "score_point_hist_temp_bytes", "score_point_batch_assemble_log"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert C.sizeof(_lib.PointLogStore) == 8 + 11 * 8 + 3 * 8 + 2 * 4
    # the struct's own size check and the argument checks in front of the launch (host only: nothing is launched)
    st, out = _lib.PointLogStore(), _lib.BatchOut()
    assert lib.score_point_batch_assemble_log(C.byref(st), 0, 1, 2, 4, 1, 1, C.byref(out), None, None) == -1
    st.struct_bytes = C.sizeof(_lib.PointLogStore) + 8
    assert lib.score_point_batch_assemble_log(C.byref(st), 0, 1, 2, 4, 1, 1, C.byref(out), None, None) == -1
    st.struct_bytes = C.sizeof(_lib.PointLogStore)
    assert lib.score_point_batch_assemble_log(C.byref(st), 0, 1, 2, 4, 1, 1, C.byref(out), None, None) == -1      # null arrays
    # the build's workspace: four arrays of n words and the sort's histogram matrix; the sort's limit on n
    assert lib.score_point_hist_temp_bytes(0) == -1 and lib.score_point_hist_temp_bytes(2 ** 31) == -1
    for n in (1, 8192, 54925330):                                       # (the full Tmall log)
        assert lib.score_point_hist_temp_bytes(n) == 16 * ((n + 63) // 64 * 64) + lib.score_sort_pairs_temp_bytes(n)
    assert lib.score_point_hist_build(None, None, None, None, 10, 0, 1, 1, 5, 11, 6, None, None, None, None, 0, None) == -1


# ---- the build's edge cases (tests/point_hist_cases.py): the numpy build against the plain-Python restatement ----------------
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("name", phc.NAMES)
def test_host_hist_csr_equals_the_restatement(name, swap):
    c = phc.swapped(phc.case(name)) if swap else phc.case(name)
    off, seq, ln = phc.expected(name, swap)
    got = host_hist_csr(*[c[k] for k in phc.ARGS])
    assert off.shape == (c["n_ent"] + 1,) and ln.shape == (c["n_ent"],) and seq.shape == (int(off[-1]),)
    for g, w in zip(got, (off, seq, ln)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


@pytest.mark.parametrize("name", phc.NAMES)
def test_hist_cases_are_worth_running(name):
    """what each case is in the table for, on the restatement alone"""
    n, n_ent, id_lo, time_bits, H, _, key_bits, sorts, npass = phc.CASES[name]
    c = phc.case(name)
    off, seq, ln = phc.expected(name)
    count = np.diff(off)
    # the pass structure of the table, and the side of 32 bits it stands for
    assert phc.structure(n_ent, time_bits) == (key_bits, sorts, npass) and (key_bits <= 32) == (sorts == 1)
    # ... and another one for the second build into the same workspace
    assert phc.structure(phc.swap_n_ent(name), time_bits)[1:] != (sorts, npass)
    tiles = -(-n // phc.TILE)
    assert (tiles > phc.FUSED_MAX_TILES) == (name == "past_fused") and (name != "fused_limit" or n == phc.FUSED_MAX_TILES * phc.TILE)
    assert len(c["ent"]) == n and int(c["time_key"].max()) == 2 ** time_bits - 1 and int(c["time_key"].min()) == 0
    assert len(np.unique(c["time_key"])) <= 12 and set(np.unique(c["t_idx"]).tolist()) == set(range(7))
    # ids outside the range on both sides, inside the window too
    inwin = (c["t_idx"] >= c["start"]) & (c["t_idx"] < c["pred"])
    below, above = c["ent"] < id_lo, c["ent"].astype(np.int64) >= id_lo + n_ent
    assert below.any() and above.any() and (name == "empty_window" or ((below & inwin).any() and (above & inwin).any()))
    assert (id_lo != 1 or (c["ent"] < 0).any()) and int(off[-1]) == int((inwin & ~below & ~above).sum())
    if name == "empty_window":
        assert not inwin.any() and not off.any() and not ln.any() and len(seq) == 0
        return
    assert off[-1] > 0
    if n_ent > 1:
        assert (count > H).any() and (count == 0).any() and (ln == H).any()
        assert count[n_ent - 2] == 0 and count[n_ent - 1] > 0 and (n_ent < 4 or count[n_ent - 3] > 0)
    else:
        assert count[0] > H
    if name == "pack32_top_bit":                    # keys of real entities with the top bit set, not the sink's alone
        assert count[2 ** 20:].sum() > 0 and n_ent > n
    # equal (entity, time) with different payloads: what shows a sort that is not stable; over the tile seam where there is one
    hist = phc.histories(*[c[k] for k in phc.ARGS[:-1]])
    tied = seam = False
    for l in hist.values():
        runs = {}
        for o, tk, pos in l:
            runs.setdefault(tk, []).append((o, pos))
        for r in runs.values():
            if len(set(o for o, _ in r)) >= 2:
                tied = True
                seam = seam or (min(p for _, p in r) < phc.TILE <= max(p for _, p in r))
    assert tied and (seam or n <= phc.TILE)
