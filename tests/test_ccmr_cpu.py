"""CCMR from its raw rating log, the host rules (dataprep.remap_ccmr_log, targets.UserNegLists, gen_target_lines' neg_lists,
ccmr_pipeline / ccmr_point_stores) against tests/golden/g12_ccmr.npz, which the REFERENCE's own feateng_ccmr.py and
gen_target.py wrote (tests/golden/make_ccmr_golden.py).  Pinned exactly: the split, the slices, the ids, the item rows, the
negative lists, who gets a line and its positive, every negative that comes from a list, the history orders.  The reference's
random pads (Python's `random`) are pinned as count, range and equality ACROSS the three splits for a user that has an entry in
the user_neg_dict: the reference appends the pads to the list inside the dict (gen_target.py:89-95), but for a user WITHOUT an
entry it pads a fresh [] that is never stored (:82-83), so that user's negatives differ from split to split there."""
import functools
import os

import numpy as np
import pytest

from score_amd import dataprep as dp
from score_amd.pointdata import host_hist_csr
from score_amd.targets import TargetStore, UserNegLists

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_ccmr.npz")


@functools.lru_cache(maxsize=None)
def gold():
    g = dict(np.load(GOLDEN))
    for a in g.values():
        a.setflags(write=False)
    d = g["dims"].tolist()
    g.update(U=d[0], I=d[1], S=d[2], NEG=d[3], vocab=tuple(d[4:8]), preds=tuple(d[8:11]))
    return g


@functools.lru_cache(maxsize=None)
def remap():
    g = gold()
    return dp.remap_ccmr_log(g["log"], g["movie_info"], g["U"], g["I"], g["vocab"])


def neg_lists():
    r = remap()
    return UserNegLists.from_events(r["neg_uid"], r["neg_iid"], r["n_users"])


def csr_dict(keys, off, vals):
    return {int(k): vals[off[j]:off[j + 1]].tolist() for j, k in enumerate(keys.tolist())}


def test_split_slices_and_ids_equal_the_references():
    g, r = gold(), remap()
    assert np.array_equal(r["pos"], g["pos_at"]) and np.array_equal(r["neg"], g["neg_at"])
    assert np.array_equal(r["uid"], g["pos_uid"]) and np.array_equal(r["iid"], g["pos_iid"]) and np.array_equal(r["t_idx"], g["pos_t"])
    assert np.array_equal(r["neg_uid"], g["neg_uid"]) and np.array_equal(r["neg_iid"], g["neg_iid"])
    # the slice of EVERY event, the negative half included; slices 0 (from before the start) and below 0 both occur
    date = g["log"][:, 3]
    day = np.asarray([dp._ordinal(v) for v in date.tolist()])
    t_all = dp.ccmr_slice_index(day, dp._ordinal(dp.CCMR_START_DATE))
    assert np.array_equal(t_all[g["neg_at"]], g["neg_t"]) and np.array_equal(t_all[g["pos_at"]], g["pos_t"])
    before = day < dp._ordinal(dp.CCMR_START_DATE)
    assert (t_all[before] == 0).any() and (t_all[before] < 0).any()
    assert np.array_equal(r["time_key"], day[g["pos_at"]])
    U, I = g["U"], g["I"]
    assert r["feature_size"] == 1 + U + I + sum(g["vocab"]) and r["vocab_sizes"] == (U, I) + g["vocab"]
    assert np.array_equal(r["user_rows"], np.arange(1, U + 1).reshape(U, 1))


def test_item_rows_equal_the_movie_dict():
    g, r = gold(), remap()
    U, I = g["U"], g["I"]
    rows = r["item_rows"]
    assert rows.shape == (I, 5) and rows.dtype == np.int32 and np.array_equal(rows[:, 0], np.arange(U + 1, U + I + 1))
    assert np.array_equal(rows[g["movie_keys"] - U - 1, 1:], g["movie_vals"])
    none = [U + I + sum(g["vocab"][:k + 1]) for k in range(4)]
    unlined = sorted(set(range(U + 1, U + I + 1)) - set(g["movie_keys"].tolist()))
    assert unlined == [U + I] and rows[I - 1, 1:].tolist() == none           # no line and no positive event: the "none" ids
    assert all((rows[:, 1 + k] == none[k]).any() for k in range(4))           # each field empty at least once
    # the first line wins: the items with two lines differ between their lines
    mi = g["movie_info"]
    twice = [i for i in range(I) if (mi[:, 0] == i).sum() == 2]
    assert len(twice) == 3
    for i in twice:
        first, second = mi[mi[:, 0] == i]
        assert (first[1:] != second[1:]).any()
        want = dp._ccmr_field_ids(first[None, 1:].astype(np.int64), U, I, g["vocab"])[0]
        assert rows[i, 1:].tolist() == want.tolist()


def test_negative_lists_equal_the_user_neg_dict():
    g = gold()
    nl = neg_lists()
    assert nl.lists() == csr_dict(g["und_users"], g["und_off"], g["und_items"])
    off, items = nl.arrays()
    assert off.shape == (g["U"] + 1,) and off.dtype == np.int64 and items.dtype == np.int32 and off[-1] == len(items) == len(g["neg_at"])
    assert any(len(set(l)) < len(l) for l in nl.lists().values())             # duplicates are kept
    assert UserNegLists.empty(g["U"]).lists() == {}
    # an event with a uid outside 1 .. U joins no list
    r = remap()
    more = UserNegLists.from_events(np.concatenate([[0, g["U"] + 1], r["neg_uid"]]), np.concatenate([[g["U"] + 1] * 2, r["neg_iid"]]), g["U"])
    assert more.lists() == nl.lists()


@pytest.mark.parametrize("draws", ["cell", "stream"])
def test_lines_against_the_references_three_splits(draws):
    """eligibility, positives and every negative that comes from a list exactly; the pads as count, range and equality across
    the splits -- the reference's by its mutated dict and the stream rule's by mutating neg_lists (users with an entry), the
    cell rule's by construction (every user)"""
    g, r = gold(), remap()
    U, I, NEG = g["U"], g["I"], g["NEG"]
    nl = neg_lists()
    own = nl.lists()
    seen = {}
    ref_seen, fresh = {}, {}
    for pt in g["preds"]:                                           # the reference's order
        lines = dp.gen_target_lines(r["uid"], r["iid"], r["t_idx"], U, I, pt, NEG, 0, 11, draws=draws, neg_lists=nl)
        assert [u for u, _ in lines] == g["lines%d_users" % pt].tolist()
        assert [its[0] for _, its in lines] == g["lines%d_pos" % pt].tolist()
        for (u, its), ref in zip(lines, g["lines%d_neg" % pt].tolist()):
            k = min(len(own.get(u, [])), NEG)
            assert len(its) == 1 + NEG and len(ref) == NEG
            assert its[1:1 + k] == ref[:k] == own.get(u, [])[:k], (pt, u)
            assert all(U + 1 <= x <= U + I for x in its[1 + k:] + ref[k:])
            if draws == "cell" or u in own:                                 # a user's negatives are the same in every split
                assert seen.setdefault(u, its[1:]) == its[1:], (pt, u)
            if u in own:
                assert ref_seen.setdefault(u, ref) == ref, (pt, u)
            else:
                fresh.setdefault(u, []).append(tuple(ref))
    lens = [len(own.get(u, [])) for u in g["lines%d_users" % g["preds"][0]].tolist()]
    assert 0 in lens and NEG in lens and any(0 < l < NEG for l in lens) and any(l > NEG for l in lens)
    assert set(own) - set(seen)                                                 # a user with negatives and no line
    assert any(len(set(v)) > 1 for v in fresh.values())                         # (no entry: the reference draws anew per split)
    if draws == "stream":                                                       # the lists were mutated, as documented
        after = nl.lists()
        for u, negs in seen.items():
            assert after[u] == own[u] + negs[len(own[u]):] and len(after[u]) == max(NEG, len(own[u])), u
        assert all(after[u] == own[u] for u in set(own) - set(seen)) and set(after) == set(own)
        assert sum(map(len, after.values())) > sum(map(len, own.values()))
    else:
        assert nl.lists() == own


@pytest.mark.parametrize("draws", ["cell", "stream"])
@pytest.mark.parametrize("pop", [False, True])
def test_empty_lists_equal_no_lists(draws, pop):
    g, r = gold(), remap()
    pop_items = np.arange(g["U"] + 3, g["U"] + 20, 2) if pop else None
    for pt in g["preds"]:
        args = (r["uid"], r["iid"], r["t_idx"], g["U"], g["I"], pt, 7, 1, 5)
        a = dp.gen_target_lines(*args, draws=draws, pop_items=pop_items)
        b = dp.gen_target_lines(*args, draws=draws, pop_items=pop_items, neg_lists=UserNegLists.empty(g["U"]))
        assert a == b != []
    a = TargetStore.from_log(*args, build="host", sample_factor=2)
    b = TargetStore.from_log(*args, build="host", sample_factor=2, neg_lists=UserNegLists.empty(g["U"]))
    assert a.lines() == b.lines() != []


def test_cell_pads_are_the_draws_of_the_same_position_and_the_pop_list_is_honoured():
    g, r = gold(), remap()
    U, I = g["U"], g["I"]
    nl, own = neg_lists(), neg_lists().lists()
    pop = np.arange(U + 2, U + 30, 3)
    for pop_items in (None, pop):
        for neg in (1, 5, 6, 99):
            args = (r["uid"], r["iid"], r["t_idx"], U, I, 4, neg, 0, 23)
            plain = dp.gen_target_lines(*args, draws="cell", pop_items=pop_items)
            with_lists = dp.gen_target_lines(*args, draws="cell", pop_items=pop_items, neg_lists=nl)
            assert len(plain) == len(with_lists) > 0
            for (u, a), (v, b) in zip(plain, with_lists):
                k = min(len(own.get(u, [])), neg)
                assert u == v and a[0] == b[0] and b[1:1 + k] == own.get(u, [])[:k] and b[1 + k:] == a[1 + k:]
                assert pop_items is None or set(b[1 + k:]) <= set(pop.tolist())
    with pytest.raises(ValueError, match="neg_lists is over"):
        dp.gen_target_lines(*args, draws="cell", neg_lists=UserNegLists.empty(U + 1))


def test_history_orders_equal_the_references():
    g, r = gold(), remap()
    U, I = g["U"], g["I"]
    for pt in g["preds"]:
        for side, ent, other, lo, n_ent in (("user", r["uid"], r["iid"], 1, U), ("item", r["iid"], r["uid"], U + 1, I)):
            off, seq, _ = host_hist_csr(ent, other, r["time_key"], r["t_idx"], 0, pt, lo, n_ent, 300)
            got = {lo + e: seq[off[e]:off[e + 1]].tolist() for e in range(n_ent) if off[e + 1] > off[e]}
            want = csr_dict(g["%s_hist%d_keys" % (side, pt)], g["%s_hist%d_off" % (side, pt)], g["%s_hist%d_vals" % (side, pt)])
            assert got == want, (side, pt)
    # (some user has two events of one day in another order than their items': the stable order is what is pinned)
    days = {}
    for u, k in zip(r["uid"].tolist(), r["time_key"].tolist()):
        days.setdefault((u, k), 0)
        days[(u, k)] += 1
    assert max(days.values()) >= 2


def test_pipeline_and_point_stores_on_the_host():
    g = gold()
    small = dict(dp.CCMR, graph_time_slice_num=g["S"], time_slice_num=g["S"], pred_time_test=4, pred_time_validation=3, pred_time_train=2,
                 train_neg=g["NEG"], test_neg=g["NEG"])
    saved = dict(dp.CCMR)
    dp.CCMR.update(small)
    try:
        graph, r, lines = dp.ccmr_pipeline(g["log"], g["movie_info"], g["U"], g["I"], g["vocab"], draws="cell")
        for name, pt in (("test", 4), ("validation", 3), ("train", 2)):
            assert [u for u, _ in lines[name]] == g["lines%d_users" % pt].tolist()
            assert [its[0] for _, its in lines[name]] == g["lines%d_pos" % pt].tolist()
        assert graph.U == g["U"] and graph.I == g["I"] and graph.S == g["S"]
        assert np.array_equal(np.asarray(graph.item_rows), r["item_rows"])
        stores, _ = dp.ccmr_point_stores(g["log"], g["movie_info"], g["U"], g["I"], g["vocab"], draws="cell", build="host",
                                         batch_size=2 * (1 + g["NEG"]))
        for name in ("train", "validation", "test"):
            n = stores[name].n_lines
            assert n >= 2 and stores[name].line_user.tolist() == [u for u, _ in lines[name]][:n]
            assert stores[name].line_items.reshape(n, -1).tolist() == [its for _, its in lines[name]][:n]
    finally:
        dp.CCMR.clear()
        dp.CCMR.update(saved)
    assert dp.CCMR["graph_time_slice_num"] == 41 and dp.CCMR["max_1hop"] == 10 and dp.CCMR["max_2hop"] == 100
    assert [dp.CCMR[k] for k in ("pred_time_train", "pred_time_validation", "pred_time_test")] == [38, 39, 40]
    assert dp.CCMR["train_neg"] == dp.CCMR["test_neg"] == 99 and dp.CCMR["start_time"] == 0


def test_value_errors():
    g = gold()
    log, mi, U, I, v = g["log"], g["movie_info"], g["U"], g["I"], g["vocab"]

    def bad(row, col, value, movie=False):
        a = (mi if movie else log).copy()
        a[row, col] = value
        return (log, a) if movie else (a, mi)

    for value in (20050230, 20051301, 20050100, 19000229, 0, -20050519, 100000101):
        with pytest.raises(ValueError, match="calendar date"):
            dp.remap_ccmr_log(*bad(5, 3, value), U, I, v)
    dp.remap_ccmr_log(*bad(5, 3, 20040229), U, I, v)                 # a leap day is a date
    for value in (-1, U):
        with pytest.raises(ValueError, match="raw user id"):
            dp.remap_ccmr_log(*bad(7, 0, value), U, I, v)
    for value in (-1, I):
        with pytest.raises(ValueError, match="raw item id"):
            dp.remap_ccmr_log(*bad(7, 1, value), U, I, v)
    with pytest.raises(ValueError, match="movie_info: a raw item id"):
        dp.remap_ccmr_log(*bad(2, 0, I, movie=True), U, I, v)
    for k in range(4):
        for value in (-2, v[k] - 1):                                 # (the last id of a vocabulary is its "none")
            with pytest.raises(ValueError, match="outside its vocabulary"):
                dp.remap_ccmr_log(*bad(2, 1 + k, value, movie=True), U, I, v)
    pos_item = int(log[np.flatnonzero(log[:, 2] >= 4)[0], 1])
    with pytest.raises(ValueError, match="1 items occur among the positive events and have no movie_info line"):
        dp.remap_ccmr_log(log, mi[mi[:, 0] != pos_item], U, I, v)
    with pytest.raises(ValueError, match="build is"):
        dp.remap_ccmr_log(log, mi, U, I, v, build="gpu")
    nl = neg_lists()
    r = remap()
    with pytest.raises(ValueError, match="needs draws='cell'"):
        dp.ccmr_pipeline(log, mi, U, I, v, targets="device")
    assert nl.n_users == U and r["n_users"] == U
