"""CCMR's data path ON THE DEVICE (csrc/ccmr.hip: score_ccmr_prep, score_neg_lists_build; csrc/targetgen.hip:
score_target_build_lists) against the host rules -- dataprep.remap_ccmr_log, targets.UserNegLists.from_events,
gen_target_lines(draws="cell", neg_lists=...) --, themselves pinned to the reference's own code in test_ccmr_cpu.py.  Exact
integers; the outputs are poisoned first."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ccmr_cases as cc
import target_cases as tc
from score_amd import _lib
from score_amd import dataprep as dp
from score_amd.graph import DeviceGraphLoader
from score_amd.targets import TargetStore, UserNegLists

pytestmark = pytest.mark.gpu
POISON = -0x5A5A5A5B
E_BADARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
PAD = 3


def up(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


@functools.lru_cache(maxsize=None)
def host_lists(name):
    c = cc.case(name)
    return UserNegLists.from_events(c["neg_uid"], c["neg_iid"], c["U"])


@functools.lru_cache(maxsize=None)
def host_arrays(name):
    """the host rule's lines as two arrays (computed once, never modified)"""
    c = cc.case(name)
    st = TargetStore.from_log(c["uid"], c["iid"], c["t_idx"], c["U"], c["I"], c["pred"], c["neg"], c["start"], c["seed"],
                              build="host", pop_items=c["pop"], sample_factor=c["factor"] if c["factor"] > 1 else None,
                              neg_lists=host_lists(name))
    lu, li = st.arrays()
    lu.setflags(write=False)
    li.setflags(write=False)
    return lu, li


# ---- score_neg_lists_build ------------------------------------------------------------------------------------------------
def lists_call(c, temp_short=0):
    lib = _lib.load()
    n, U = len(c["neg_uid"]), c["U"]
    need = int(lib.score_neg_lists_temp_bytes(n))
    assert need > 0
    temp = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    off = torch.full((U + 1 + PAD,), POISON, dtype=torch.int64, device="cuda")
    items = torch.full((n + PAD,), POISON, dtype=torch.int32, device="cuda")
    u, i = up(c["neg_uid"]), up(c["neg_iid"])
    rc = lib.score_neg_lists_build(u.data_ptr() if n else None, i.data_ptr() if n else None, n, U, off.data_ptr(), items.data_ptr(),
                                   temp.data_ptr(), need - temp_short, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, off.cpu().numpy(), items.cpu().numpy()


@pytest.mark.parametrize("name", cc.LIST_CASES)
def test_negative_lists_equal_the_host_csr(name):
    c = cc.case(name)
    n, U = len(c["neg_uid"]), c["U"]
    rc, off, items = lists_call(c)
    h_off, h_items = host_lists(name).arrays()
    assert rc == 0 and np.array_equal(off[:U + 1], h_off) and (off[U + 1:] == POISON).all(), name
    used = int(h_off[-1])
    assert np.array_equal(items[:used], h_items) and (items[used:n] == 0).all() and (items[n:] == POISON).all(), name
    d = UserNegLists.from_events(up(c["neg_uid"]), up(c["neg_iid"]), U, build="device")
    assert d.on_device and d.lists() == host_lists(name).lists(), name


def test_negative_list_guards():
    c = cc.case("lens_neg5")
    rc, off, items = lists_call(c, temp_short=1)
    assert rc == E_WORKSPACE and (off == POISON).all() and (items == POISON).all()
    lib = _lib.load()
    assert lib.score_neg_lists_temp_bytes(2 ** 31) == -1 and lib.score_neg_lists_temp_bytes(-1) == -1
    assert lib.score_neg_lists_build(None, None, 5, 3, None, None, None, 0, None) == E_BADARG


# ---- score_target_build_lists ---------------------------------------------------------------------------------------------
class Build(object):
    """one device build through the C ABI into poisoned outputs"""

    def __init__(self, c, lists, temp_short=0):
        self.lib, self.c = _lib.load(), c
        self.log = [up(c["uid"]), up(c["iid"]), up(c["t_idx"])]
        self.pop = None if c["pop"] is None else up(c["pop"])
        off, items = lists.arrays()
        self.off, self.items = up(off, np.int64), up(items)
        n = len(c["uid"])
        need = int(self.lib.score_target_build_temp_bytes(n, c["U"]))
        assert need > 0
        self.temp = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
        self.temp_bytes = need - temp_short
        build = _lib.TargetBuild(C.sizeof(_lib.TargetBuild), self.log[0].data_ptr(), self.log[1].data_ptr(), self.log[2].data_ptr(),
                                 n, c["U"], c["I"], c["start"], c["pred"], c["neg"], c["factor"], c["seed"],
                                 None if self.pop is None else self.pop.data_ptr(), 0 if self.pop is None else int(self.pop.numel()))
        self.args = _lib.TargetLists(C.sizeof(_lib.TargetLists), build, self.off.data_ptr(),
                                     self.items.data_ptr() if len(items) else None, len(items))
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.n_lines = C.c_int64(-77)
        self.per = 1 + c["neg"]
        self.out(16)

    def out(self, rows):
        self.line_user = torch.full((rows,), POISON, dtype=torch.int32, device="cuda")
        self.line_items = torch.full((rows * self.per,), POISON, dtype=torch.int32, device="cuda")

    def count(self):
        return self.lib.score_target_build_lists(C.byref(self.args), None, None, 0, C.byref(self.n_lines), self.temp.data_ptr(),
                                                 self.temp_bytes, self.stream)

    def fill(self, cap):
        return self.lib.score_target_build_lists(C.byref(self.args), self.line_user.data_ptr(), self.line_items.data_ptr(), cap,
                                                 None, self.temp.data_ptr(), self.temp_bytes, self.stream)

    def run(self, cap_short=0):
        assert self.count() == 0
        L = int(self.n_lines.value)
        self.out(L + PAD)
        if L - cap_short > 0:
            assert self.fill(L - cap_short) == 0
        torch.cuda.synchronize()
        return self

    def all_poison(self):
        torch.cuda.synchronize()
        return bool((self.line_user == POISON).all()) and bool((self.line_items == POISON).all()) and self.n_lines.value == -77


def assert_equals(b, want, name, written=None):
    lu, li = want
    L = len(lu)
    assert int(b.n_lines.value) == L, name
    w = L if written is None else written
    got_u, got_i = b.line_user.cpu().numpy(), b.line_items.cpu().numpy().reshape(L + PAD, b.per)
    assert np.array_equal(got_u[:w], lu[:w]) and np.array_equal(got_i[:w], li[:w]), name
    assert (got_u[w:] == POISON).all() and (got_i[w:] == POISON).all(), name


@pytest.mark.parametrize("name", cc.LIST_CASES)
def test_device_build_with_lists_equals_the_host_rule(name):
    assert_equals(Build(cc.case(name), host_lists(name)).run(), host_arrays(name), name)


def test_cases_hold_what_they_are_for():
    assert {len(cc.case("nneg_%d" % n)["neg_uid"]) for n in cc.NEG_COUNTS} == {0, 1, cc.SCAN_TILE - 1, cc.SCAN_TILE + 1,
                                                                              cc.SORT_TILE - 1, cc.SORT_TILE + 1}
    assert list(host_lists("one_owner").lists()) == [77] and len(host_lists("one_owner").lists()[77]) == 500
    assert 77 in host_arrays("one_owner")[0].tolist()
    lens = lambda name: np.diff(host_lists(name).arrays()[0])
    assert lens("all_long_neg5").min() >= 5 and cc.case("all_long_neg5")["neg"] == 5
    assert set(lens("lens_neg5").tolist()) == {0, 4, 5, 6} and cc.case("lens_neg5")["neg"] == 5
    c = cc.case("nneg_%d" % (cc.SORT_TILE + 1))                       # (events outside the id range join no list)
    assert c["neg_uid"].min() == 0 and c["neg_uid"].max() == c["U"] + 1 and lens("nneg_%d" % (cc.SORT_TILE + 1)).sum() == cc.SORT_TILE - 1
    for name in cc.LIST_CASES:                                        # lines exist, and lists and draws both occur in them
        lu, li = host_arrays(name)
        assert len(lu) >= 4, name
        own = lens(name)[lu - 1]
        if name != "nneg_0":
            assert (own > 0).any(), name
        if name != "all_long_neg5":
            assert (own < li.shape[1] - 1).any(), name
    assert {host_arrays("width_neg%d" % k)[1].shape[1] for k in cc.WIDTHS} == {2, 6, 7, 100, 101}
    # both sorts of the list path (the lines' and the lists', keys 0 .. U) in one pass and in two: every other case takes one
    assert {tc.sort_passes(cc.case(n)["U"]) for n in cc.LIST_CASES if not n.startswith("users_")} == {1}
    assert (tc.sort_passes(cc.case("users_4095")["U"]), tc.sort_passes(cc.case("users_4096")["U"])) == (1, 2)
    for name in ("users_4095", "users_4096"):
        c = cc.case(name)
        assert len(c["neg_uid"]) == 500 and c["neg_uid"].min() == 0 and c["neg_uid"].max() == c["U"] + 1, name
        assert lens(name).sum() == 498 and 24 <= len(host_arrays(name)[0]) <= 60, name
    # score_ccmr_prep sorts its movie lines by item (keys 0 .. I): the other raw logs take one pass
    assert {tc.sort_passes(cc.raw_log(n)[3]) for n in ("edges", "tenk")} == {1}
    assert [tc.sort_passes(cc.raw_log(n)[3]) for n in cc.PASS_LOGS] == [1, 2]
    for name in cc.PASS_LOGS:
        log, movie, U, I = cc.raw_log(name)
        items, lines = np.unique(movie[:, 0], return_counts=True)
        assert len(log) == 400 and len(movie) == 300 and len(items) == 250 < I // 4 and items[0] == 0 and items[-1] == I - 1, name
        two = items[lines == 2]                                       # the first line counts: the second one differs
        assert len(two) == 50 and all((np.diff(movie[movie[:, 0] == x][:, 1:], axis=0) != 0).any() for x in two), name
        assert set(log[:, 1].tolist()) & set(two.tolist()) and set(log[:, 1].tolist()) <= set(items.tolist()), name
    assert cc.case("pop_lists")["pop"] is not None and cc.case("factor_lists")["factor"] == 4
    plain = tc.host_lines(tc.case("factor4"))
    assert [u for u, _ in plain] == host_arrays("factor_lists")[0].tolist()      # the lists change no line's fate
    # with a pop list every drawn negative is an entry of it, every other one the user's own
    c, (lu, li) = cc.case("pop_lists"), host_arrays("pop_lists")
    own = host_lists("pop_lists").lists()
    for u, row in zip(lu.tolist(), li.tolist()):
        k = min(len(own.get(u, [])), c["neg"])
        assert row[1:1 + k] == own.get(u, [])[:k] and set(row[1 + k:]) <= set(c["pop"].tolist())


def test_lines_start_at_every_offset_from_a_16_byte_boundary():
    starts = set()
    for k in cc.WIDTHS:
        name = "width_neg%d" % k
        b = Build(cc.case(name), host_lists(name)).run()
        starts |= {(b.line_items.data_ptr() + l * b.per * 4) % 16 for l in range(int(b.n_lines.value))}
        assert_equals(b, host_arrays(name), name)
    assert starts == {0, 4, 8, 12}


@pytest.mark.parametrize("name", ["all_eligible", "all_eligible_neg6", "pop_list", "factor4", "edges"])
def test_empty_lists_give_score_target_builds_output(name):
    """word for word the lines of score_target_build -- its own host rule, target_cases.host_lines"""
    c = tc.case(name)
    lines = tc.host_lines(c)
    want = (np.asarray([u for u, _ in lines], dtype=np.int32),
            np.asarray([its for _, its in lines], dtype=np.int32).reshape(len(lines), 1 + c["neg"]))
    assert_equals(Build(c, UserNegLists.empty(c["U"])).run(), want, name)
    dev = TargetStore.from_log(c["uid"], c["iid"], c["t_idx"], c["U"], c["I"], c["pred"], c["neg"], c["start"], c["seed"],
                               pop_items=c["pop"], sample_factor=c["factor"] or None)
    au, ai = dev.arrays()
    assert np.array_equal(au, want[0]) and np.array_equal(ai, want[1])


@pytest.mark.parametrize("name", ["lens_neg5", "width_neg99", "width_neg6", "pop_lists"])
def test_a_cap_one_short_leaves_the_last_line_alone(name):
    b = Build(cc.case(name), host_lists(name)).run(cap_short=1)
    assert_equals(b, host_arrays(name), name, written=len(host_arrays(name)[0]) - 1)


def test_short_workspace_shape_and_struct_sizes_are_refused_before_any_launch():
    name = "lens_neg5"
    c, nl = cc.case(name), host_lists(name)
    b = Build(c, nl, temp_short=1)
    assert b.count() == E_WORKSPACE and b.fill(4) == E_WORKSPACE and b.all_poison()
    b = Build(c, nl)
    b.args.struct_bytes -= 8
    assert b.count() == E_BADARG and b.fill(4) == E_BADARG and b.all_poison()
    b = Build(c, nl)
    b.args.build.struct_bytes -= 8
    assert b.count() == E_BADARG and b.fill(4) == E_BADARG and b.all_poison()
    b = Build(dict(c, neg=4096), nl)
    assert b.count() == E_SHAPE and b.fill(1) == E_SHAPE and b.all_poison()
    b = Build(c, nl)
    b.args.n_neg = 2 ** 31
    assert b.count() == E_SHAPE and b.fill(1) == E_SHAPE and b.all_poison()
    b = Build(c, nl)
    b.args.neg_off = None
    assert b.count() == E_BADARG and b.fill(1) == E_BADARG and b.all_poison()
    b = Build(c, nl)
    b.args.neg_items = None
    assert b.count() == E_BADARG and b.all_poison()


def test_one_wait_per_count_and_the_store_takes_lists_from_either_side():
    name = "width_neg99"
    c, nl, lib = cc.case(name), host_lists(name), _lib.load()
    args = (c["uid"], c["iid"], c["t_idx"], c["U"], c["I"], c["pred"], c["neg"], c["start"], c["seed"])
    w0 = lib.score_target_host_waits()
    a = TargetStore.from_log(*args, neg_lists=nl)                                        # host lists: uploaded
    assert lib.score_target_host_waits() - w0 == 1
    d = UserNegLists.from_events(up(c["neg_uid"]), up(c["neg_iid"]), c["U"], build="device")
    b = TargetStore.from_log(*[up(x) for x in args[:3]], *args[3:], neg_lists=d)
    assert lib.score_target_host_waits() - w0 == 2
    for st in (a, b):
        lu, li = st.arrays()
        assert st.on_device and np.array_equal(lu, host_arrays(name)[0]) and np.array_equal(li, host_arrays(name)[1])
    # under one seed a user's padding is the same at every prediction time
    rows = {}
    for pred in (2, 3, 4):
        st = TargetStore.from_log(*args[:5], pred, *args[6:], neg_lists=d)
        for u, its in st.lines():
            assert rows.setdefault(u, its[1:]) == its[1:]
    with pytest.raises(ValueError, match="neg_lists is over"):
        TargetStore.from_log(*args, neg_lists=UserNegLists.empty(c["U"] + 1))
    with pytest.raises(ValueError, match="host only"):
        dp.gen_target_lines(*args, draws="stream", neg_lists=d)


# ---- score_ccmr_prep ------------------------------------------------------------------------------------------------------
def assert_same_remap(d, h):
    assert set(d) == set(h)
    for k in ("uid", "iid", "t_idx", "time_key", "neg_uid", "neg_iid", "pos", "neg"):
        assert d[k].is_cuda and d[k].dtype == torch.int32 and np.array_equal(d[k].cpu().numpy(), h[k]), k
    for k in ("user_rows", "item_rows"):
        assert isinstance(d[k], np.ndarray) and d[k].dtype == np.int32 and np.array_equal(d[k], h[k]), k
    for k in ("n_users", "n_items", "feature_size", "vocab_sizes"):
        assert d[k] == h[k], k


def test_dates_at_the_calendar_edges_and_on_both_sides_of_the_start():
    log, movie, U, I = cc.raw_log("edges")
    h = dp.remap_ccmr_log(log, movie, U, I, cc.VOCAB)
    lib = _lib.load()
    w0 = lib.score_log_host_waits()
    d = dp.remap_ccmr_log(log, movie, U, I, cc.VOCAB, build="device")
    assert lib.score_log_host_waits() - w0 == 2                      # the two compactions; the third wait is the download
    assert_same_remap(d, h)
    # what the case is for: every edge date among the positives, with the slices the rule asks for
    pos_dates = log[h["pos"], 3]
    assert set(pos_dates.tolist()) == set(cc.EDGE_DATES)
    t_of = dict(zip(pos_dates.tolist(), h["t_idx"].tolist()))
    assert (t_of[20050219], t_of[20050218], t_of[20050518], t_of[20050519], t_of[20050816], t_of[20050817]) == (0, -1, 0, 0, 0, 1)
    assert cc.yyyymmdd(-89) == 20050219 and cc.yyyymmdd(-90) == 20050218 and cc.yyyymmdd(89) == 20050816
    k_of = dict(zip(pos_dates.tolist(), h["time_key"].tolist()))
    assert k_of[20040301] - k_of[20040228] == 2 and k_of[20050301] - k_of[20050228] == 1 and k_of[21000301] - k_of[21000228] == 1
    assert k_of[20000229] + 306 == k_of[20001231] and k_of[10101] == 1 and k_of[99991231] == 3652059
    # another start and slice length; an int32 log
    h = dp.remap_ccmr_log(log, movie, U, I, cc.VOCAB, start_date=20000229, delta_days=7)
    assert_same_remap(dp.remap_ccmr_log(log.astype(np.int32), movie.astype(np.int32), U, I, cc.VOCAB, start_date=20000229,
                                        delta_days=7, build="device"), h)
    # no movie_info at all: every occurring item is missing, on both builds with the same count
    for build in ("host", "device"):
        with pytest.raises(ValueError, match="%d items occur" % len(set(log[h["pos"], 1].tolist()))):
            dp.remap_ccmr_log(log, movie[:0], U, I, cc.VOCAB, build=build)


@pytest.mark.parametrize("name", cc.PASS_LOGS)
def test_movie_lines_sorted_in_one_and_in_two_passes(name):
    """item counts on both sides of the sort's second pass; most items have no line, 50 have two"""
    log, movie, U, I = cc.raw_log(name)
    assert_same_remap(dp.remap_ccmr_log(log, movie, U, I, cc.VOCAB, build="device"), dp.remap_ccmr_log(log, movie, U, I, cc.VOCAB))


def test_bad_dates_ids_and_features_raise_the_hosts_value_error():
    log, movie, U, I = cc.raw_log("edges")

    def both(match, log=log, movie=movie):
        for build in ("host", "device"):
            with pytest.raises(ValueError, match=match):
                dp.remap_ccmr_log(log, movie, U, I, cc.VOCAB, build=build)

    def with_value(a, row, col, value):
        a = a.copy()
        a[row, col] = value
        return a

    for value in (20050230, 20051301, 20050100, 19000229, 21000229, 0, -20050519, 100000101, 20050632):
        both("calendar date", log=with_value(log, 9, 3, value))
    for value in (-1, U):
        both("raw user id", log=with_value(log, len(log) - 1, 0, value))
    for value in (-1, I):
        both("raw item id", log=with_value(log, 0, 1, value))
    both("movie_info: a raw item id", movie=with_value(movie, 1, 0, I))
    for k in range(4):
        for value in (-2, cc.VOCAB[k] - 1):
            both("outside its vocabulary", movie=with_value(movie, len(movie) - 1, 1 + k, value))
    pos_item = int(log[np.flatnonzero(log[:, 2] >= 4)[0], 1])
    both("1 items occur among the positive events", movie=movie[movie[:, 0] != pos_item])
    with pytest.raises(ValueError, match="int32"):
        dp.remap_ccmr_log(with_value(log, 3, 0, 2 ** 31), movie, U, I, cc.VOCAB, build="device")


def test_prep_guards_refuse_before_any_launch():
    lib = _lib.load()
    log, movie, U, I = cc.raw_log("edges")
    n, m = len(log), len(movie)
    raw, mv = up(log.T), up(movie.T)
    out = torch.full((6, n), POISON, dtype=torch.int32, device="cuda")
    flat = torch.full((8 + I * 5,), POISON, dtype=torch.int32, device="cuda")
    need = int(lib.score_ccmr_prep_temp_bytes(m, I))
    temp = torch.empty((need,), dtype=torch.uint8, device="cuda")

    def call(temp_short=0, **kw):
        a = _lib.CcmrPrep()
        a.struct_bytes, a.n_events, a.n_movies, a.n_users, a.n_items = C.sizeof(_lib.CcmrPrep), n, m, U, I
        a.user, a.item, a.rating, a.date = (raw[j].data_ptr() for j in range(4))
        for k in range(5):
            a.movie[k] = mv[k].data_ptr()
        for k in range(4):
            a.vocab[k] = cc.VOCAB[k]
        a.start_day, a.delta_days = 732085, 90
        a.uid, a.iid, a.t_idx, a.day, a.keep_pos, a.keep_neg = (out[j].data_ptr() for j in range(6))
        a.status, a.item_rows = flat.data_ptr(), flat.data_ptr() + 32
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.score_ccmr_prep(C.byref(a), temp.data_ptr(), need - temp_short, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc

    untouched = lambda: bool((out == POISON).all()) and bool((flat == POISON).all())
    assert call(temp_short=1) == E_WORKSPACE and untouched()
    assert call(struct_bytes=C.sizeof(_lib.CcmrPrep) - 8) == E_BADARG and untouched()
    assert call(delta_days=0) == E_BADARG and untouched()
    assert call(n_users=2 ** 31 - 10) == E_SHAPE and untouched()
    assert call(status=None) == E_BADARG and untouched()
    assert lib.score_ccmr_prep_temp_bytes(2 ** 31, 5) == -1 and lib.score_ccmr_prep_temp_bytes(5, 0) == -1
    assert call() == 0 and not untouched() and flat[:8].tolist() == [0] * 8


# ---- end to end on about 10 k events --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tenk():
    log, movie, U, I = cc.raw_log("tenk")
    host = dp.ccmr_pipeline(log, movie, U, I, cc.VOCAB, draws="cell")
    dev = dp.ccmr_pipeline(log, movie, U, I, cc.VOCAB, build="device", draws="cell", targets="device", remap="device")
    return dict(log=log, movie=movie, U=U, I=I, host=host, dev=dev)


def test_device_pipeline_equals_the_all_host_cell_pipeline(tenk):
    (gh, rh, th), (gd, rd, td) = tenk["host"], tenk["dev"]
    assert_same_remap(rd, rh)
    assert 0.1 < len(rh["neg"]) / len(tenk["log"]) < 0.3 and (rh["t_idx"] < 0).any() and rh["t_idx"].max() == 40
    for a, b in ((gd.user_csr, gh.user_csr), (gd.item_csr, gh.item_csr)):
        for k in ("off1", "nbr1", "off2", "nbr2"):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert gd.S == gh.S == 41 and np.array_equal(gd.user_rows, gh.user_rows) and np.array_equal(gd.item_rows, gh.item_rows)
    assert gd.item_rows.shape == (tenk["I"], 5) and gd.user_rows.shape == (tenk["U"], 1)
    own = UserNegLists.from_events(rh["neg_uid"], rh["neg_iid"], tenk["U"]).lists()
    pads = {}
    for name in ("train", "validation", "test"):
        st = td[name]
        assert isinstance(st, TargetStore) and st.on_device and st.per_line == 100
        assert st.lines() == th[name] and len(th[name]) >= 4, name
        for u, its in th[name]:                                      # the user's own negatives first; one padding in every split
            k = min(len(own.get(u, [])), 99)
            assert its[1:1 + k] == own.get(u, [])[:k] and pads.setdefault(u, its[1:]) == its[1:]
    assert any(own.get(u) for u in pads) and any(not own.get(u) for u in pads)


def _graph_batch(g, lines, pred):
    c = dp.CCMR
    return next(iter(DeviceGraphLoader(g, 200, lines, c["start_time"], pred, 99, c["time_slice_num"] - c["start_time"] - 1,
                                       c["obj_per_time_slice"], seed=77)))


def test_loader_batches_and_one_training_step_are_equal(tenk):
    from score_amd import model as M
    from score_amd.pointdata import DeviceDataLoaderDualSeq
    (gh, rh, th), (gd, rd, td) = tenk["host"], tenk["dev"]
    c = dp.CCMR
    pt = c["pred_time_validation"]
    a, b = _graph_batch(gd, td["validation"], pt), _graph_batch(gh, th["validation"], pt)
    assert len(a.tensors) == len(b.tensors) == 8 and a.B == b.B == 200
    assert all(torch.equal(x, y) for x, y in zip(a.tensors, b.tensors))
    kw = dict(draws="cell", batch_size=200)
    sd, _ = dp.ccmr_point_stores(tenk["log"], tenk["movie"], tenk["U"], tenk["I"], cc.VOCAB, targets="device", remap="device", **kw)
    sh, _ = dp.ccmr_point_stores(tenk["log"], tenk["movie"], tenk["U"], tenk["I"], cc.VOCAB, build="host", **kw)
    for name in ("train", "validation", "test"):
        ha, hb = sd[name].arrays(), sh[name].arrays()
        assert sd[name].n_lines == sh[name].n_lines >= 2 and all(np.array_equal(ha[k], hb[k]) for k in ha), name
    sb, _ = dp.ccmr_point_stores(tenk["log"], tenk["movie"], tenk["U"], tenk["I"], cc.VOCAB, **kw)      # host remap and lines
    mk = lambda st: next(iter(DeviceDataLoaderDualSeq(200, 20, None, None, None, 99, None, None, store=st)))
    x, y = mk(sd["test"]), mk(sb["test"])
    assert len(x) == len(y) == 7 and all(torch.equal(x[k], y[k]) for k in range(7))
    losses = []
    for g, lines in ((gd, td["validation"]), (gh, th["validation"])):
        m = M.SCORE(rh["feature_size"], 8, 16, c["time_slice_num"] - c["start_time"] - 1, c["obj_per_time_slice"], c["user_fnum"],
                    c["item_fnum"], seed=3)
        losses.append(m.train(None, _graph_batch(g, lines, pt), 1e-3, 1e-4))
    torch.cuda.synchronize()
    print("losses: %r %r" % tuple(losses))
    assert np.isfinite(losses).all() and losses[0] == losses[1] and c["item_fnum"] == 5
