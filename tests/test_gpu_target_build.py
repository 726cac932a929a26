"""The target lines built from the log ON THE DEVICE (csrc/targetgen.hip: score_target_build, score_pop_items;
targets.TargetStore.from_log(build="device")) against the host rule, dataprep.gen_target_lines(draws="cell") / gen_pop_items /
sample_target_lines(draws="cell") -- itself pinned to a plain-Python restatement and to the reference's own code in
test_target_cell_draws.py.  Exact integers; the outputs are poisoned first."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import target_cases as tc
from score_amd import _lib
from score_amd import dataprep as dp
from score_amd.graph import DeviceGraphLoader, TemporalGraph
from score_amd.targets import TargetStore, pop_items_device

pytestmark = pytest.mark.gpu
POISON = -0x5A5A5A5B
E_BADARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
PAD = 3                                            # poisoned lines behind the last: nothing may be written there


@functools.lru_cache(maxsize=None)
def host_arrays(name):
    """the host rule's lines as two arrays (computed once, never modified)"""
    c = tc.case(name)
    lines = tc.host_lines(c)
    lu = np.asarray([u for u, _ in lines], dtype=np.int32)
    li = np.asarray([its for _, its in lines], dtype=np.int32).reshape(len(lines), 1 + c["neg"])
    lu.setflags(write=False)
    li.setflags(write=False)
    return lu, li


class Build(object):
    """one device build through the C ABI into poisoned outputs"""

    def __init__(self, c, temp_short=0):
        self.lib, self.dev, self.c = _lib.load(), torch.device("cuda"), c
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.dev)
        self.log = [up(c["uid"]), up(c["iid"]), up(c["t_idx"])]
        self.pop = None if c["pop"] is None else up(c["pop"])
        n = len(c["uid"])
        need = int(self.lib.score_target_build_temp_bytes(n, c["U"]))
        assert need > 0
        self.temp = torch.full((need,), 0x5A, dtype=torch.uint8, device=self.dev)
        self.temp_bytes = need - temp_short
        self.args = _lib.TargetBuild(C.sizeof(_lib.TargetBuild), self.log[0].data_ptr(), self.log[1].data_ptr(),
                                     self.log[2].data_ptr(), n, c["U"], c["I"], c["start"], c["pred"], c["neg"], c["factor"],
                                     c["seed"], None if self.pop is None else self.pop.data_ptr(),
                                     0 if self.pop is None else int(self.pop.numel()))
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.n_lines = C.c_int64(-77)
        self.per = 1 + c["neg"]
        self.out(16)

    def out(self, rows):
        self.line_user = torch.full((rows,), POISON, dtype=torch.int32, device=self.dev)
        self.line_items = torch.full((rows * self.per,), POISON, dtype=torch.int32, device=self.dev)

    def count(self):
        return self.lib.score_target_build(C.byref(self.args), None, None, 0, C.byref(self.n_lines), self.temp.data_ptr(),
                                           self.temp_bytes, self.stream)

    def fill(self, cap):
        return self.lib.score_target_build(C.byref(self.args), self.line_user.data_ptr(), self.line_items.data_ptr(), cap, None,
                                           self.temp.data_ptr(), self.temp_bytes, self.stream)

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


def assert_equals_host(b, name, written=None):
    lu, li = host_arrays(name)
    L = len(lu)
    assert int(b.n_lines.value) == L, name
    w = L if written is None else written
    got_u, got_i = b.line_user.cpu().numpy(), b.line_items.cpu().numpy().reshape(L + PAD, b.per)
    assert np.array_equal(got_u[:w], lu[:w]) and np.array_equal(got_i[:w], li[:w]), name
    assert (got_u[w:] == POISON).all() and (got_i[w:] == POISON).all(), name


@pytest.mark.parametrize("name", tc.CASES)
def test_device_build_equals_the_host_rule(name):
    assert_equals_host(Build(tc.case(name)).run(), name)


def test_cases_hold_what_they_are_for():
    assert len(host_arrays("no_pred_slice")[0]) == 0 and len(host_arrays("all_eligible")[0]) == 130
    assert host_arrays("edges")[0].tolist() == [1, 4, 6, 8, 9] and host_arrays("highest_user_only")[0].tolist() == [200]
    assert host_arrays("edges_neg4095")[1].shape == (5, 4096) and host_arrays("edges_neg0")[1].shape == (5, 1)
    assert 0 < len(host_arrays("factor4")[0]) < len(host_arrays("factor1")[0])
    assert {tc.SCAN_TILE + d for d in (-1, 0, 1)} | {tc.SORT_TILE + d for d in (-1, 0, 1)} <= set(tc.TILE_COUNTS)
    assert host_arrays("pop_list_factor4_neg99")[1].shape[1] == 100 and len(host_arrays("pop_list_factor4_neg99")[0]) >= 4
    # (lines of 100 words all start on a 16-byte boundary; the odd widths are the ones that start off it)
    for name in tc.ODD_WIDTH_CASES:
        lu, li = host_arrays(name)
        per = li.shape[1]
        assert per > 4 and per % 4 != 0 and len(lu) >= 8, name
        assert {(l * per * 4) % 16 for l in range(len(lu))} == {0, 4, 8, 12}, name
    assert {host_arrays(n)[1].shape[1] for n in tc.ODD_WIDTH_CASES} == {5, 7, 11, 101}
    # the sort's result lands in either pair of arrays: every other case sorts in one pass (keys 0 .. U below 4,096)
    assert tc.sort_passes(4095) == 1 and tc.sort_passes(4096) == 2 and tc.sort_passes(2 ** 24) == 3
    assert {tc.sort_passes(tc.case(n)["U"]) for n in tc.CASES if n not in tc.PASS_CASES} == {1}
    assert [tc.sort_passes(tc.case(n)["U"]) for n in tc.PASS_CASES] == [1, 2, 2]
    for name in tc.PASS_CASES:
        c, (lu, _) = tc.case(name), host_arrays(name)
        assert c["I"] == 50 and len(c["uid"]) == 600 and len(set(c["uid"].tolist())) < c["U"] // 4, name      # most users absent
        assert 24 <= len(lu) <= 60 and lu[0] == 1 and lu[-1] == c["U"], name
    assert tc.case("users_4096_pop")["pop"] is not None and tc.case("users_4096")["pop"] is None


@pytest.mark.parametrize("name", tc.ODD_WIDTH_CASES)
def test_lines_start_at_every_offset_from_a_16_byte_boundary(name):
    """the output the kernel fills really has line starts 0, 4, 8 and 12 bytes past a boundary, and all are filled right"""
    b = Build(tc.case(name)).run()
    starts = {(b.line_items.data_ptr() + l * b.per * 4) % 16 for l in range(int(b.n_lines.value))}
    assert starts == {0, 4, 8, 12}, name
    assert_equals_host(b, name)


def test_two_builds_share_nothing():
    """a second build into a workspace the first one used (no clearing in between) gives its own lines"""
    a = Build(tc.case("all_eligible")).run()
    b = Build(tc.case("factor4"))
    b.temp[:min(a.temp.numel(), b.temp.numel())] = a.temp[:min(a.temp.numel(), b.temp.numel())]
    assert_equals_host(b.run(), "factor4")


# ---- guards ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all_eligible", "pop_list_factor4_neg99", "all_eligible_neg6", "all_eligible_neg100", "pop_list_neg10"])
def test_a_cap_one_short_leaves_the_last_line_alone(name):
    b = Build(tc.case(name)).run(cap_short=1)
    assert_equals_host(b, name, written=len(host_arrays(name)[0]) - 1)


def test_short_workspace_shape_and_struct_size_are_refused_before_any_launch():
    c = tc.case("edges")
    b = Build(c, temp_short=1)
    assert b.count() == E_WORKSPACE and b.fill(4) == E_WORKSPACE and b.all_poison()
    b = Build(c)
    b.args.struct_bytes -= 8
    assert b.count() == E_BADARG and b.fill(4) == E_BADARG and b.all_poison()
    b = Build(dict(c, neg=4096))                   # 1 + neg > 4096
    assert b.count() == E_SHAPE and b.fill(1) == E_SHAPE and b.all_poison()
    assert _lib.load().score_target_build_temp_bytes(2 ** 31, 5) == -1
    b = Build(dict(c, pop=np.asarray([11], dtype=np.int32)))
    b.args.n_pop = 0                               # a pop list without entries cannot fill a line
    assert b.count() == 0 and b.n_lines.value == 5
    b.n_lines.value = -77
    assert b.fill(5) == E_BADARG and b.all_poison()


# ---- score_pop_items ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pop_graphs(n_items):
    U, I, S, ev, _ = tc.pop_graph_log(n_items)
    ur, ir = tc.rows(U, I)
    host = TemporalGraph.from_log(ev[:, 0], ev[:, 1], ev[:, 2], U, I, S, ur, ir, draws="cell")
    dev = TemporalGraph.from_log(ev[:, 0], ev[:, 1], ev[:, 2], U, I, S, ur, ir, draws="cell", build="device")
    return host, dev


def _pop_call(g, standard, max_iid, temp_short=0, struct_short=0, cap_short=0):
    lib, dev = _lib.load(), torch.device("cuda")
    need = int(lib.score_pop_items_temp_bytes(g.I))
    temp = torch.full((need,), 0x5A, dtype=torch.uint8, device=dev)
    a = _lib.PopItems(C.sizeof(_lib.PopItems) - struct_short, g._built["i_off1"].data_ptr(), g.U, g.I, g.S, standard,
                      max_iid if max_iid is not None else 2 ** 31 - 1, 0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = C.c_int64(-77)
    rc = lib.score_pop_items(C.byref(a), None, 0, C.byref(n), temp.data_ptr(), need - temp_short, stream)
    if rc != 0:
        assert n.value == -77
        return rc, None
    out = torch.full((int(n.value) + PAD,), POISON, dtype=torch.int32, device=dev)
    if n.value - cap_short > 0:
        rc = lib.score_pop_items(C.byref(a), out.data_ptr(), int(n.value) - cap_short, None, temp.data_ptr(), need, stream)
    torch.cuda.synchronize()
    return rc, (int(n.value), out.cpu().numpy())


@pytest.mark.parametrize("n_items", tc.POP_ITEM_COUNTS)
def test_pop_items_equal_the_host_list(n_items):
    host, dev = pop_graphs(n_items)
    S, mid = host.S, host.U + host.I // 2
    for standard, max_iid in ((1, None), (S, None), (S + 1, None), (2, mid), (1, host.U + host.I)):
        want = dp.gen_pop_items(host, standard, max_iid)
        rc, (n, got) = _pop_call(dev, standard, max_iid)
        assert rc == 0 and n == len(want), (standard, max_iid)
        assert np.array_equal(got[:n], want) and (got[n:] == POISON).all(), (standard, max_iid)
        if standard == 1 and max_iid is None:
            assert torch.equal(pop_items_device(dev, standard).cpu(), torch.from_numpy(want))
    assert len(dp.gen_pop_items(host, S + 1)) == 0 and 0 < len(dp.gen_pop_items(host, 2, mid)) < len(dp.gen_pop_items(host, 2))
    assert dp.gen_pop_items(host, 2, mid).max() <= mid < dp.gen_pop_items(host, 2).max()


def test_pop_items_guards():
    host, dev = pop_graphs(50)
    want = dp.gen_pop_items(host, 1)
    rc, (n, got) = _pop_call(dev, 1, None, cap_short=1)
    assert rc == 0 and np.array_equal(got[:n - 1], want[:-1]) and (got[n - 1:] == POISON).all()
    assert _pop_call(dev, 1, None, temp_short=1)[0] == E_WORKSPACE
    assert _pop_call(dev, 1, None, struct_short=8)[0] == E_BADARG


# ---- end to end, on the bundled Tmall sample ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample():
    raw = np.load(os.path.join(tc.GOLDEN, "tmall_sample_log.npz"))["log"]
    g, r, stores = dp.tmall_pipeline(raw, build="device", draws="cell", targets="device")
    _, _, host = dp.tmall_pipeline(raw, draws="cell")
    return dict(raw=raw, g=g, r=r, stores=stores, host=host, c=dp.TMALL)


def _graph_loader(s, lines, pred, neg, batch):
    c = s["c"]
    return DeviceGraphLoader(s["g"], batch, lines, c["start_time"], pred, neg, c["time_slice_num"] - c["start_time"] - 1,
                             c["obj_per_time_slice"], seed=77)


def _same_graph_batches(s, store, pred, neg, batch):
    n = 0
    for a, b in zip(_graph_loader(s, store, pred, neg, batch), _graph_loader(s, store.lines(), pred, neg, batch)):
        assert len(a.tensors) == len(b.tensors) == 8 and a.B == b.B
        assert all(torch.equal(x, y) for x, y in zip(a.tensors, b.tensors))
        n += 1
    assert n >= 2
    assert len(_graph_loader(s, store, pred, neg, batch)) == len(_graph_loader(s, store.lines(), pred, neg, batch)) == n


def test_pipeline_stores_equal_the_host_cell_lines(sample):
    for name in ("train", "validation", "test"):
        st = sample["stores"][name]
        assert isinstance(st, TargetStore) and st.on_device and st.line_items.dtype == torch.int32
        assert st.lines() == sample["host"][name] != [], name
        assert st.per_line == (2 if name == "train" else 100)


def test_graph_loader_takes_the_store_as_it_is(sample):
    c = sample["c"]
    st = sample["stores"]["validation"]
    ld = _graph_loader(sample, st, c["pred_time_validation"], 99, 500)
    assert ld.uids.data_ptr() == st.line_user.data_ptr() and ld.iids.data_ptr() == st.line_items.data_ptr()   # no copy
    _same_graph_batches(sample, st, c["pred_time_validation"], 99, 500)
    _same_graph_batches(sample, sample["stores"]["train"], c["pred_time_train"], 1, 16)
    _same_graph_batches(sample, st, c["pred_time_validation"], 4, 35)            # fewer negatives: the first columns
    with pytest.raises(ValueError, match="negatives"):
        _graph_loader(sample, st, c["pred_time_validation"], 100, 101)


def _point_store(s, lines, pred, neg, batch, dual=True):
    from score_amd.pointdata import PointLogStore
    r = s["r"]
    return PointLogStore(r["uid"], r["iid"], s["raw"][:, 5], r["t_idx"], lines, s["c"]["start_time"], pred, dp.POINT_HIST_MAX_LEN,
                         neg, batch, r["user_rows"], r["item_rows"], dual, build="device")


def _same_point_batches(s, store, pred, neg, batch):
    from score_amd.pointdata import DeviceDataLoaderDualSeq
    a, b = _point_store(s, store, pred, neg, batch), _point_store(s, store.lines(), pred, neg, batch)
    assert a.n_batches == b.n_batches >= 2 and torch.is_tensor(a.line_user)
    for k in ("batch_max_user_len", "batch_max_len", "batch_min_len"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    mk = lambda st: DeviceDataLoaderDualSeq(batch, 20, None, None, None, neg, None, None, store=st)
    n = 0
    for x, y in zip(mk(a), mk(b)):
        assert len(x) == len(y) == 7 and all(torch.equal(x[k], y[k]) for k in range(7))
        n += 1
    assert n == a.n_batches


def test_point_store_takes_the_store_as_it_is(sample):
    c = sample["c"]
    _same_point_batches(sample, sample["stores"]["validation"], c["pred_time_validation"], 99, 200)
    _same_point_batches(sample, sample["stores"]["test"], c["pred_time_test"], 3, 8)
    # the checks that ride in the build's read-back: an id outside its range, a user without history
    st = sample["stores"]["validation"]
    bad = TargetStore(st.line_user.clone(), st.line_items.clone())
    bad.line_items[5, 98] = sample["r"]["n_users"] + sample["r"]["n_items"] + 1
    with pytest.raises(ValueError, match="target line 5: an id outside"):
        _point_store(sample, bad, c["pred_time_validation"], 99, 200)
    r = sample["r"]
    never = sorted(set(range(1, r["n_users"] + 1)) - set(r["uid"][r["t_idx"] < c["pred_time_validation"]].tolist()))
    assert never
    bad = TargetStore(st.line_user.clone(), st.line_items.clone())
    bad.line_user[3] = never[0]
    with pytest.raises(ValueError, match="target line 3: user %d has no history" % never[0]):
        _point_store(sample, bad, c["pred_time_validation"], 99, 200)


def test_point_stores_from_one_upload_equal_the_host_target_form(sample):
    """tmall_point_stores(targets="device"): the log is uploaded once, the lines and the histories are built from those
    tensors; the stores equal those built from numpy columns and host cell lines"""
    B = {"train": 8, "validation": 200, "test": 200}               # (the train slice has 41 lines of 2 items)
    dev, _ = dp.tmall_point_stores(sample["raw"], batch_size=B, targets="device", draws="cell")
    host, _ = dp.tmall_point_stores(sample["raw"], batch_size=B, draws="cell")
    for name in ("train", "validation", "test"):
        a, b = dev[name], host[name]
        assert torch.is_tensor(a.line_user) and a.n_lines == b.n_lines > 0, name
        for k in ("line_user", "line_items", "line_last_item"):
            assert np.array_equal(getattr(a, k).cpu().numpy(), getattr(b, k)), (name, k)
        ha, hb = a.arrays(), b.arrays()
        assert all(np.array_equal(ha[k], hb[k]) for k in ha), name
        for k in ("batch_max_user_len", "batch_max_len", "batch_min_len"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), (name, k)
    from score_amd.pointdata import PointLogStore
    r = sample["r"]
    cols = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda() for x in (r["uid"], r["iid"], sample["raw"][:, 5], r["t_idx"])]
    with pytest.raises(ValueError, match="uid must lie"):
        PointLogStore(cols[0] + r["n_users"], cols[1], cols[2], cols[3], sample["host"]["train"], 0, 9, 300, 1, 2,
                      r["user_rows"], r["item_rows"], True, build="device")
    with pytest.raises(ValueError, match="build='device'"):
        PointLogStore(cols[0], cols[1], cols[2], cols[3], sample["host"]["train"], 0, 9, 300, 1, 2, r["user_rows"], r["item_rows"],
                      True, build="host")


def test_pop_list_and_down_sampling_end_to_end(sample):
    """With pop_items=(graph, 9) the bundled sample's pop list is EMPTY (no item of the 9,999-event sample has more than 7
    non-empty slices), so both builds raise the ValueError the rule asks for; the equalities are asserted at pop_standard 3
    (55 items) as well, where there are lines to compare."""
    c, r, g = sample["c"], sample["r"], sample["g"]
    pt = c["pred_time_test"]                     # (the test slice: 15 of its 44 lines pass the 1-in-4 rule at this seed)
    args = (r["uid"], r["iid"], r["t_idx"], r["n_users"], r["n_items"], pt, 99, c["start_time"], 22)
    assert len(dp.gen_pop_items(g, 9)) == 0
    for build in ("device", "host"):
        with pytest.raises(ValueError, match="pop_items is empty"):
            TargetStore.from_log(*args, build=build, pop_items=(g, 9), sample_factor=4)
    pop = dp.gen_pop_items(g, 3)
    assert torch.equal(pop_items_device(g, 3).cpu(), torch.from_numpy(pop)) and len(pop) > 10
    dev = TargetStore.from_log(*args, build="device", pop_items=(g, 3), sample_factor=4)
    host = TargetStore.from_log(*args, build="host", pop_items=(g, 3), sample_factor=4)
    want = dp.sample_target_lines(dp.gen_target_lines(*args, draws="cell", pop_items=pop), 4, 22, draws="cell")
    assert dev.lines() == host.lines() == want and 4 <= len(want) < len(sample["host"]["test"])     # (two whole batches at least)
    assert set(x for _, its in want for x in its[1:]) <= set(pop.tolist())
    _same_graph_batches(sample, dev, pt, 99, 200)
    _same_point_batches(sample, dev, pt, 99, 200)
    _, _, sampled = dp.tmall_pipeline(sample["raw"], build="device", draws="cell", targets="device", sample_factor=4)
    assert sampled["train"].lines() == sample["host"]["train"]
    assert sampled["validation"].lines() == dp.sample_target_lines(sample["host"]["validation"], 4, 21, draws="cell")
    assert sampled["test"].lines() == dp.sample_target_lines(sample["host"]["test"], 4, 22, draws="cell")


# ---- one training step ----------------------------------------------------------------------------------------------------
def test_one_training_step_gives_the_same_loss_bits(sample):
    from score_amd import model as M
    from score_amd.pointdata import DeviceDataLoaderUserSeq
    c, r = sample["c"], sample["r"]
    st, pt = sample["stores"]["validation"], c["pred_time_validation"]
    T = c["time_slice_num"] - c["start_time"] - 1
    losses = []
    for lines in (st, st.lines()):
        m = M.SCORE(r["feature_size"], 8, 16, T, c["obj_per_time_slice"], c["user_fnum"], c["item_fnum"], seed=3)
        losses.append(m.train(None, next(_graph_loader(sample, lines, pt, 99, 200)), 1e-3, 1e-4))
    for lines in (st, st.lines()):
        m = M.MODELS["GRU4Rec"](r["feature_size"], 16, 32, 20, 3, 4, seed=7)
        ps = _point_store(sample, lines, pt, 99, 200, dual=False)
        losses.append(m.train(None, next(DeviceDataLoaderUserSeq(200, 20, None, None, 99, None, None, model=m, store=ps)), 1e-2, 1e-4))
    torch.cuda.synchronize()
    print("losses: SCORE %r %r, GRU4Rec %r %r" % tuple(losses))
    assert np.isfinite(losses).all() and losses[0] == losses[1] and losses[2] == losses[3]
