"""The target lines' per-user draw rule (dataprep.gen_target_lines(draws="cell"), gen_pop_items, sample_target_lines) on the
host: against a plain-Python restatement, against a copy of the function as it was before the rule existed (defaults
unchanged), against the reference's own code (tests/golden/g10_targets.npz) and for uniformity; the errors; TargetStore's
host form."""
import os

import numpy as np
import pytest

import target_cases as tc
from score_amd import dataprep as dp
from score_amd.graph import TemporalGraph
from score_amd.targets import TargetStore

M64 = 2 ** 64 - 1
G = 0x9E3779B97F4A7C15


# ---- the restatement: dicts and loops, keys from Python integers ----------------------------------------------------------
def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, tag, c, j):
    h = mix(((seed & M64) + G * ((tag << 40) + c + 1)) & M64)
    return mix((h + G * (j + 1)) & M64) >> 32


def plain_lines(c):
    U, I = c["U"], c["I"]
    first, hist = {}, set()
    for u, i, t in zip(c["uid"].tolist(), c["iid"].tolist(), c["t_idx"].tolist()):
        if not (1 <= u <= U and U + 1 <= i <= U + I and t >= 0):
            continue
        if t == c["pred"] and u not in first:
            first[u] = i
        if c["start"] <= t < c["pred"]:
            hist.add(u)
    pop = None if c["pop"] is None else [int(x) for x in c["pop"]]
    lines = []
    for u in sorted(first):
        if u not in hist:
            continue
        if c["factor"] > 1 and (key(c["seed"], 6, u, 0) * c["factor"]) >> 32 != 0:
            continue
        if pop is None:
            negs = [U + 1 + ((key(c["seed"], 4, u, j) * I) >> 32) for j in range(c["neg"])]
        else:
            negs = [pop[(key(c["seed"], 5, u, j) * len(pop)) >> 32] for j in range(c["neg"])]
        lines.append((u, [first[u]] + negs))
    return lines


@pytest.mark.parametrize("name", tc.CASES)
def test_cell_rule_equals_plain_python(name):
    c = tc.case(name)
    assert tc.host_lines(c) == plain_lines(c)


def test_cases_hold_what_they_are_for():
    assert [u for u, _ in plain_lines(tc.case("edges"))] == [1, 4, 6, 8, 9]
    assert dict(plain_lines(tc.case("edges")))[4][0] == 15 and dict(plain_lines(tc.case("edges")))[6][0] == 14
    assert plain_lines(tc.case("no_pred_slice")) == []
    assert len(plain_lines(tc.case("all_eligible"))) == 130
    assert [u for u, _ in plain_lines(tc.case("highest_user_only"))] == [200]
    assert {its[1] for _, its in plain_lines(tc.case("one_item"))} == {71}
    assert 0 < len(plain_lines(tc.case("factor4"))) < 150 and len(plain_lines(tc.case("edges_factor4_seed3"))) == 2
    assert set(x for _, its in plain_lines(tc.case("pop_list")) for x in its[1:]) <= set(tc.case("pop_list")["pop"].tolist())


@pytest.mark.parametrize("n_items", tc.POP_ITEM_COUNTS[-2:])
def test_pop_items_equal_plain_python(n_items):
    U, I, S, ev, want = tc.pop_graph_log(n_items)
    ur, ir = tc.rows(U, I)
    g = TemporalGraph.from_log(ev[:, 0], ev[:, 1], ev[:, 2], U, I, S, ur, ir, draws="cell")
    slices = {}
    for _, i, t in ev.tolist():
        slices.setdefault(i, set()).add(t)
    for standard, max_iid in ((1, None), (S, None), (S + 1, None), (2, U + I // 2), (0, None)):
        plain = [i for i in range(U + 1, U + I + 1)
                 if len(slices.get(i, ())) >= standard and (max_iid is None or i <= max_iid)]
        got = dp.gen_pop_items(g, standard, max_iid)
        assert got.dtype == np.int32 and got.tolist() == plain, (standard, max_iid)
    assert len(dp.gen_pop_items(g, S + 1)) == 0 and len(dp.gen_pop_items(g, 0)) == I
    assert {U + 1, U + I} <= set(dp.gen_pop_items(g, S).tolist())


def test_sample_rule_equals_plain_python():
    lines = [(u, [u + 1000]) for u in range(1, 3001, 3)]
    for f, seed in ((1, 11), (2, 11), (12, 5), (4, 2 ** 63 + 9)):
        plain = [l for l in lines if f == 1 or (key(seed, 6, l[0], 0) * f) >> 32 == 0]
        assert dp.sample_target_lines(lines, f, seed, draws="cell") == plain
    # "stream": one draw per line, in line order, from one PCG64 stream
    rng = np.random.Generator(np.random.PCG64(7))
    assert dp.sample_target_lines(lines, 5, 7) == [l for l in lines if int(rng.integers(1, 6)) == 1]
    assert dp.sample_target_lines(lines, 1, 7) == lines


# ---- defaults unchanged ---------------------------------------------------------------------------------------------------
def gen_target_lines_before(uid, iid, t_idx, n_users, n_items, pred_time, neg_sample_num, start_time=0, seed=11):
    """dataprep.gen_target_lines as it was before draws= and pop_items= were added"""
    rng = np.random.Generator(np.random.PCG64(seed))
    uid, iid, t_idx = np.asarray(uid), np.asarray(iid), np.asarray(t_idx)
    has_hist = np.zeros(n_users + 1, dtype=bool)
    has_hist[uid[(t_idx >= start_time) & (t_idx < pred_time)]] = True
    first_pos = {}
    for u, i, t in zip(uid.tolist(), iid.tolist(), t_idx.tolist()):
        if t == pred_time and u not in first_pos:
            first_pos[u] = i
    lines = []
    for u in sorted(first_pos):
        if has_hist[u]:
            negs = rng.integers(n_users + 1, n_users + n_items + 1, neg_sample_num).tolist()
            lines.append((u, [first_pos[u]] + negs))
    return lines


@pytest.fixture(scope="module")
def sample():
    return dp.remap_tmall_log(np.load(os.path.join(tc.GOLDEN, "tmall_sample_log.npz"))["log"])


def test_defaults_unchanged(sample):
    r = sample
    for pt, neg, seed in ((9, 1, 20), (10, 99, 21), (11, 99, 22)):
        args = (r["uid"], r["iid"], r["t_idx"], r["n_users"], r["n_items"], pt, neg, 0, seed)
        assert dp.gen_target_lines(*args) == gen_target_lines_before(*args) != []
    for name in ("tile_4097", "all_eligible"):
        c = tc.case(name)
        args = (c["uid"], c["iid"], c["t_idx"], c["U"], c["I"], c["pred"], c["neg"], c["start"], c["seed"])
        assert dp.gen_target_lines(*args) == gen_target_lines_before(*args) != []
    raw = np.load(os.path.join(tc.GOLDEN, "tmall_sample_log.npz"))["log"]
    _, _, t = dp.tmall_pipeline(raw)
    assert t["validation"] == gen_target_lines_before(r["uid"], r["iid"], r["t_idx"], r["n_users"], r["n_items"], 10, 99, 0, 21)


def test_stream_rule_with_a_pop_list():
    c = tc.case("pop_list")
    pop = c["pop"]
    lines = dp.gen_target_lines(c["uid"], c["iid"], c["t_idx"], c["U"], c["I"], c["pred"], c["neg"], c["start"], 3, pop_items=pop)
    rng = np.random.Generator(np.random.PCG64(3))
    assert [(u, its[0]) for u, its in lines] == [(u, its[0]) for u, its in plain_lines(c)]
    for _, its in lines:
        assert its[1:] == pop[rng.integers(0, len(pop), c["neg"])].tolist()


# ---- the reference's own code ---------------------------------------------------------------------------------------------
def test_lines_and_pop_lists_equal_the_references():
    z = np.load(os.path.join(tc.GOLDEN, "g10_targets.npz"))
    U, I, S, start, pred, neg = (int(x) for x in z["dims"])
    uid, iid, t = z["uid"], z["iid"], z["t_idx"]
    ur, ir = tc.rows(U, I)
    g = TemporalGraph.from_log(uid, iid, t, U, I, S, ur, ir, draws="cell")
    pops = []
    for k in range(3):
        standard, max_iid = (int(x) for x in z["pop%d_args" % k])
        pops.append(dp.gen_pop_items(g, standard, max_iid))
        assert np.array_equal(pops[k], z["pop%d" % k]) and len(pops[k]), k
    assert np.array_equal(dp.gen_pop_items(g, int(z["pop0_args"][0])), z["pop0"])           # (max_iid default: all)
    for tag, pop in (("plain", None), ("pop", pops[1])):
        ref_neg = z[tag + "_neg"]
        allowed = set(range(U + 1, U + I + 1)) if pop is None else set(pop.tolist())
        assert ref_neg.shape == (len(z[tag + "_users"]), neg) and set(ref_neg.ravel().tolist()) <= allowed
        for draws in ("stream", "cell"):
            lines = dp.gen_target_lines(uid, iid, t, U, I, pred, neg, start, 11, draws=draws, pop_items=pop)
            assert [u for u, _ in lines] == z[tag + "_users"].tolist(), (tag, draws)
            assert [its[0] for _, its in lines] == z[tag + "_pos"].tolist(), (tag, draws)
            assert all(len(its) == 1 + neg and set(its[1:]) <= allowed for _, its in lines), (tag, draws)


# ---- uniformity: a condition on the rule as specified ---------------------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 20, 1111])
def test_negatives_are_uniform(seed):
    U, neg, I = 400, 99, 64
    uid = np.repeat(np.arange(1, U + 1), 2)
    t = np.tile([0, 1], U)
    lines = dp.gen_target_lines(uid, np.full(2 * U, U + 1), t, U, I, 1, neg, 0, seed, draws="cell")
    negs = np.asarray([its[1:] for _, its in lines])
    assert negs.shape == (U, neg)
    counts = np.bincount(negs.ravel() - U - 1, minlength=I)
    expect = U * neg / I
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print("seed %d: chi-square %.1f over %d draws, %d bins" % (seed, chi2, U * neg, I))
    assert chi2 < 103.44                                            # the 99.9 % point at 63 degrees of freedom
    assert negs.min() == U + 1 and negs.max() == U + I
    assert not (negs[1:] == negs[:-1]).all(axis=1).any()            # no two consecutive users share a row


def test_down_sampling_keeps_its_share():
    lines = [(u, [20001]) for u in range(1, 20001)]
    kept = len(dp.sample_target_lines(lines, 12, 11, draws="cell"))
    print("factor 12, seed 11: %d of 20000 lines kept" % kept)
    assert abs(kept - 20000 / 12) <= 157                            # four standard deviations of the binomial
    assert kept == 1607


def test_tile_constants_are_the_headers():
    """the tile sizes the cases are built around are the ones include/score_hip.h documents (the kernels' own constants are
    tied to those by static_assert in csrc/targetgen.hip and csrc/sort.hip)"""
    import re
    from score_amd import _lib
    src = open(os.path.join(os.path.dirname(tc.GOLDEN), os.pardir, "include", "score_hip.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define\s+SCORE_TARGET_(SCAN|SORT)_TILE\s+(\d+)", src)}
    assert got == {"SCAN": _lib.TARGET_SCAN_TILE, "SORT": _lib.TARGET_SORT_TILE} == {"SCAN": tc.SCAN_TILE, "SORT": tc.SORT_TILE}
    assert len(tc.TILE_COUNTS) == 7


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_errors(sample):
    c = tc.case("pop_list")                                         # (every id in range: the stream rule drops nothing)
    args = (c["uid"], c["iid"], c["t_idx"], c["U"], c["I"], c["pred"], c["neg"], c["start"], 11)
    for draws in ("stream", "cell"):
        with pytest.raises(ValueError):
            dp.gen_target_lines(*args, draws=draws, pop_items=[])
        n = tc.case("no_pred_slice")                                # nobody eligible: an empty pop list is never read
        assert dp.gen_target_lines(n["uid"], n["iid"], n["t_idx"], n["U"], n["I"], n["pred"], 3, n["start"], 11, draws=draws,
                                   pop_items=[]) == []
        with pytest.raises(ValueError):
            dp.sample_target_lines([(1, [2])], 0, draws=draws)
    with pytest.raises(ValueError):
        dp.gen_target_lines(*args, draws="other")
    with pytest.raises(ValueError):
        TargetStore.from_log(*args[:7], start_time=c["start"], build="host", sample_factor=0)
    with pytest.raises(ValueError):
        TargetStore.from_log(*args[:7], start_time=c["start"], build="host", pop_items=np.zeros((0,), dtype=np.int32))
    # a loader that asks for more negatives than the store holds (refused before the graph is touched)
    from score_amd.graph import DeviceGraphLoader
    store = TargetStore.from_log(*args[:7], start_time=c["start"], build="host")
    with pytest.raises(ValueError, match="negatives"):
        DeviceGraphLoader(None, 18, store, c["start"], c["pred"], c["neg"] + 1, 3, 2)
    raw = np.load(os.path.join(tc.GOLDEN, "tmall_sample_log.npz"))["log"]
    with pytest.raises(ValueError, match="draws='cell'"):
        dp.tmall_pipeline(raw, targets="device", draws="stream")
    with pytest.raises(ValueError, match="draws='cell'"):
        dp.tmall_point_stores(raw, targets="device")
    with pytest.raises(ValueError):
        dp.tmall_pipeline(raw, targets="host", sample_factor=4)


# ---- TargetStore(build="host") --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges", "pop_list_factor4_neg99", "no_pred_slice"])
def test_target_store_host_round_trip(name, tmp_path):
    c = tc.case(name)
    s = TargetStore.from_log(c["uid"], c["iid"], c["t_idx"], c["U"], c["I"], c["pred"], c["neg"], c["start"], c["seed"],
                             build="host", pop_items=c["pop"], sample_factor=c["factor"] or None)
    want = tc.host_lines(c)
    assert s.lines() == want and s.n_lines == len(want) and s.per_line == 1 + c["neg"]
    assert s.line_user.dtype == np.int32 and s.line_items.shape == (len(want), 1 + c["neg"])
    path = s.save(str(tmp_path / "target_4.txt"))
    assert open(path).read() == "".join("%d,%s\n" % (u, ",".join(str(i) for i in its)) for u, its in want)
    if want:
        back = TargetStore.load(path)
        assert back.lines() == want and back.per_line == s.per_line
        assert np.array_equal(back.line_user, s.line_user) and np.array_equal(back.line_items, s.line_items)
    else:
        with pytest.raises(ValueError):
            TargetStore.load(path)


def test_point_log_store_takes_a_host_target_store():
    from score_amd.pointdata import PointLogStore
    c = tc.case("all_eligible")
    ur, ir = tc.rows(c["U"], c["I"])
    s = TargetStore.from_log(c["uid"], c["iid"], c["t_idx"], c["U"], c["I"], c["pred"], 5, c["start"], 3, build="host")
    key = np.arange(len(c["uid"]))
    mk = lambda lines, neg: PointLogStore(c["uid"], c["iid"], key, c["t_idx"], lines, c["start"], c["pred"], 6, neg, 4 * (1 + neg),
                                          ur, ir, True, build="host")
    for neg in (5, 2):                                              # (fewer negatives than the store: the first columns)
        a, b = mk(s, neg), mk(s.lines(), neg)
        assert a.n_lines == b.n_lines == 128
        for k in ("line_user", "line_items", "line_last_item", "batch_max_len", "batch_min_len"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
    with pytest.raises(ValueError, match="fewer"):
        mk(s, 6)
    bad = TargetStore(s.line_user.copy(), s.line_items.copy())
    bad.line_items[7, 3] = c["U"] + c["I"] + 1
    with pytest.raises(ValueError, match="target line 7"):
        mk(bad, 5)
