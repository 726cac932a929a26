"""The four pipelines over the whole valid grid of build x targets x remap (draws="cell"), each result word for word against
the all-host result of the same functions, which the CPU goldens pin; the pipeline front's own transfers per combination; and
the one store upload (placement.upload_named): no second upload of what was built on the device, a stand-in word for an
empty array, a null pointer for an absent one.

Tmall: the bundled sample log.  CCMR: ccmr_cases' 'items_4095' -- its smallest raw log with events in the three prediction
slices; it has users with own negatives and users with none -- less the movie_info lines of one item that occurs among the
negative events only (none of the case logs has such an item: an item without a line among the positives is an error)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import ccmr_cases as cc
from score_amd import dataprep as dp
from score_amd import placement
from score_amd.graph import TemporalGraph
from score_amd.pointdata import PointLogStore, PointSeqStore
from score_amd.targets import TargetStore

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 11
GRID = [(b, t, r) for b in ("host", "device") for t in ("host", "device") for r in ("host", "device")
        if not (r == "device" and b == "host")]
SPLITS = ("train", "validation", "test")


@functools.lru_cache(maxsize=None)
def inputs(kind):
    if kind == "tmall":
        log = np.load(os.path.join(GOLDEN, "tmall_sample_log.npz"))["log"]
        log.setflags(write=False)
        return (log,)
    log, movie, U, I = cc.raw_log("items_4095")
    pos = log[:, 2] >= 4
    only_neg = sorted(set(log[~pos, 1].tolist()) - set(log[pos, 1].tolist()))
    movie = movie[movie[:, 0] != only_neg[0]]
    movie.setflags(write=False)
    with_neg = set(log[~pos, 0].tolist())
    assert with_neg and set(range(U)) - with_neg and only_neg[0] not in movie[:, 0]
    return log, movie, U, I, cc.VOCAB


def pipeline(kind, **kw):
    return (dp.tmall_pipeline if kind == "tmall" else dp.ccmr_pipeline)(*inputs(kind), seed=SEED, draws="cell", **kw)


# Tmall's train split has 41 lines of 2 items: the default batch of 200 holds no whole batch of them; CCMR takes the default
BATCH = {"tmall": {"train": 8, "validation": 200, "test": 200}, "ccmr": None}


def point_stores(kind, **kw):
    return (dp.tmall_point_stores if kind == "tmall" else dp.ccmr_point_stores)(*inputs(kind), seed=SEED, draws="cell",
                                                                                batch_size=BATCH[kind], **kw)


@functools.lru_cache(maxsize=None)
def host_pipeline(kind):
    """the all-host result: (graph's saved arrays, remap dict, {split: (line_user, line_items)}, graph)"""
    g, r, lines = pipeline(kind)
    return graph_arrays(g), r, {k: line_arrays(v) for k, v in lines.items()}, g


@functools.lru_cache(maxsize=None)
def host_stores(kind, dual):
    stores, r = point_stores(kind, dual=dual, build="host")
    return {k: store_arrays(s) for k, s in stores.items()}, r


@functools.lru_cache(maxsize=None)
def sampled_host_lines(kind, factor):
    """the all-host lines after sample_target_lines(draws="cell"), the split's seed; the train split is never sampled"""
    c, splits = (dp.TMALL, dp.TMALL_SPLITS) if kind == "tmall" else (dp.CCMR, dp.CCMR_SPLITS)
    _, _, lines = pipeline(kind)
    out = {}
    for name, pt, _ in splits:
        seed = SEED + c[pt] if kind == "tmall" else SEED
        out[name] = lines[name] if name == "train" else dp.sample_target_lines(lines[name], factor, seed, draws="cell")
    return out


def graph_arrays(g):
    """the arrays save() writes (a graph built on the device downloads them here)"""
    a = {"dims": np.asarray([g.U, g.I, g.S]), "user_rows": g.user_rows, "item_rows": g.item_rows,
         "u_deg2": np.asarray(g.user_degrees), "i_deg2": np.asarray(g.item_degrees)}
    for side, c in (("u", g.user_csr), ("i", g.item_csr)):
        a.update({"%s_%s" % (side, k): np.asarray(c[k]) for k in ("off1", "nbr1", "off2", "nbr2")})
    return a


def line_arrays(lines):
    if isinstance(lines, TargetStore):
        return lines.arrays()
    return (np.asarray([u for u, _ in lines], dtype=np.int32),
            np.asarray([its for _, its in lines], dtype=np.int32).reshape(len(lines), -1))


def store_arrays(s):
    a = {k: v for k, v in s.arrays().items() if v is not None}
    for k in ("line_user", "line_items", "line_last_item", "batch_max_user_len", "batch_max_len", "batch_min_len"):
        a[k] = placement.to_host(getattr(s, k))
    a["dims"] = np.asarray([s.n_batches, s.n_lines, s.batch_size, s.per_line, s.hist_max_len, int(s.dual), s.n_users, s.n_items])
    return a


def assert_same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


PER_EVENT = ("uid", "iid", "t_idx", "time_key", "neg_uid", "neg_iid", "pos", "neg")


def assert_same_remap(r, want, remap):
    """the host remap's keys (Tmall's device remap adds time_key), the same integers; per-event columns live where remap says"""
    assert set(want) <= set(r) and set(r) - set(want) <= {"time_key"}
    for k, v in r.items():
        if k in PER_EVENT:
            assert placement.is_tensor(v) == (remap == "device"), k
            if remap == "device":
                assert v.is_cuda and v.dtype == torch.int32, k
        if k in want:
            if k in PER_EVENT or k.endswith("_rows"):
                assert k in PER_EVENT or isinstance(v, np.ndarray), k               # (the row tables stay on the host)
                assert np.array_equal(placement.to_host(v), want[k]), k
            else:
                assert v == want[k], k


@pytest.fixture
def transfers(monkeypatch):
    """counts the pipeline front's own copies of log columns: [uploads, downloads]"""
    n = [0, 0]
    up, down = dp.device_i32, dp.to_host

    def device_i32(a, dev):
        n[0] += not placement.is_tensor(a)
        return up(a, dev)

    def to_host(a):
        n[1] += placement.is_tensor(a)
        return down(a)
    monkeypatch.setattr(dp, "device_i32", device_i32)
    monkeypatch.setattr(dp, "to_host", to_host)
    return n


def front_transfers(build, targets, remap, n_cols):
    """what the front itself copies (a device stage that is handed host arrays uploads them itself: not counted here)"""
    if remap == "device":
        return [0, 3 if targets == "host" else 0]
    if targets == "device":
        return [n_cols if build == "device" else 3, 0]
    return [0, 0]


def combo_id(c):
    return "build=%s-targets=%s-remap=%s" % c


@pytest.mark.parametrize("combo", GRID, ids=combo_id)
@pytest.mark.parametrize("kind", ["tmall", "ccmr"])
def test_pipeline_equals_the_all_host_result(kind, combo, transfers):
    build, targets, remap = combo
    want_g, want_r, want_lines, host_g = host_pipeline(kind)
    g, r, lines = pipeline(kind, build=build, targets=targets, remap=remap)
    assert transfers == front_transfers(build, targets, remap, 3)
    assert (g._built is not None) == (build == "device")
    assert_same(graph_arrays(g), want_g, "graph")
    e, t = int(want_r["uid"][0]) - 1, int(want_r["t_idx"][0])
    assert len(host_g.cell("user", 1, e, t)) and all(np.array_equal(g.cell(s, h, e, t), host_g.cell(s, h, e, t))
                                                     for s, h in (("user", 1), ("user", 2)))
    assert_same_remap(r, want_r, remap)
    assert list(lines) == [s[0] for s in (dp.TMALL_SPLITS if kind == "tmall" else dp.CCMR_SPLITS)]
    for name in SPLITS:
        assert isinstance(lines[name], TargetStore) == (targets == "device") and len(want_lines[name][0]) > 0
        if targets == "device":
            assert lines[name].on_device
        got = line_arrays(lines[name])
        assert np.array_equal(got[0], want_lines[name][0]) and np.array_equal(got[1], want_lines[name][1]), name


@pytest.mark.parametrize("combo", GRID, ids=combo_id)
@pytest.mark.parametrize("kind", ["tmall", "ccmr"])
def test_point_stores_equal_the_all_host_result(kind, combo, transfers):
    build, targets, remap = combo
    dual = combo != ("device", "host", "host")                      # (one combination in the single form)
    want, want_r = host_stores(kind, dual)
    stores, r = point_stores(kind, dual=dual, build=build, targets=targets, remap=remap)
    assert transfers == front_transfers(build, targets, remap, 4)
    assert_same_remap(r, want_r, remap)
    for name in SPLITS:
        s = stores[name]
        assert s.n_batches > 0 and s.build == build and (s._dev is not None) == (build == "device")
        assert placement.is_tensor(s.line_user) == (build == "device" and targets == "device")
        assert_same(store_arrays(s), want[name], name)


@pytest.mark.parametrize("kind", ["tmall", "ccmr"])
def test_sample_factor_4_equals_the_sampled_host_lines(kind):
    want = sampled_host_lines(kind, 4)
    _, _, lines = pipeline(kind, build="device", targets="device", remap="device", sample_factor=4)
    stores, r = point_stores(kind, build="device", targets="device", remap="host", sample_factor=4)
    c = dp.TMALL if kind == "tmall" else dp.CCMR
    _, host_r = host_stores(kind, True)
    time_key = inputs(kind)[0][:, 5] if kind == "tmall" else host_r["time_key"]
    for name, pt, neg in (dp.TMALL_SPLITS if kind == "tmall" else dp.CCMR_SPLITS):
        w = line_arrays(want[name])
        assert 0 < len(w[0]) and (name == "train" or len(w[0]) < len(host_pipeline(kind)[2][name][0]))
        got = line_arrays(lines[name])
        assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1]), name
        s = stores[name]
        ref = PointLogStore(host_r["uid"], host_r["iid"], time_key, host_r["t_idx"], want[name], c["start_time"], c[pt],
                            dp.POINT_HIST_MAX_LEN, c[neg], s.batch_size, host_r["user_rows"], host_r["item_rows"], True, build="host")
        assert s.n_batches > 0
        assert_same(store_arrays(s), store_arrays(ref), name)


# ---- the one store upload ---------------------------------------------------------------------------------------------------
def struct_pointers(struct):
    return {n: getattr(struct, n) for n, t in struct._fields_ if t is C.c_void_p}


def test_to_device_of_a_device_build_uploads_nothing_again():
    dev = torch.device("cuda:%d" % torch.cuda.current_device())
    g, _, _ = pipeline("tmall", build="device", targets="device", remap="device")
    assert g._built_device == dev and g.device == dev
    built = {k: v.data_ptr() for k, v in g._built.items()}
    for mode in ("is", "rs"):
        g.to_device(dev, mode=mode)
        assert set(g._dev) == {k for k in built if mode == "is" or not k.endswith("_deg2")}
        assert all(v.data_ptr() == built[k] for k, v in g._dev.items()) and not g.__dict__.get("_downloaded")
    for dual in (True, False):
        stores, _ = point_stores("tmall", dual=dual, build="device", targets="device", remap="device")
        s = stores["test"]
        from_build = PointLogStore.HIST[:3 if not dual else 6] + ("line_user", "line_items", "line_last_item")
        own = {k: getattr(s, k).data_ptr() for k in from_build}
        assert s.device == dev and all(s._dev[k].data_ptr() == own[k] for k in from_build)
        s.to_device(dev)
        assert all(s._dev[k].data_ptr() == own[k] and getattr(s, k).data_ptr() == own[k] for k in from_build)
        ptrs = struct_pointers(s.struct)
        assert all(ptrs[k] == own[k] for k in from_build)


def test_empty_arrays_get_a_stand_in_word_and_absent_ones_a_null_pointer(tmp_path):
    """(the single form's item side is ABSENT -- None, a null pointer, as the assembly kernels expect; an EMPTY item side is
    the dual form's over a window without events)"""
    # a graph without a 2-hop entry: no cell has a neighbour of degree > 1
    n = 6
    uid, iid, t_idx = np.arange(1, n + 1), np.arange(n + 1, 2 * n + 1), np.arange(n) % 2
    rows = lambda lo: np.arange(lo, lo + n, dtype=np.int32).reshape(n, 1)
    g = TemporalGraph.from_log(uid, iid, t_idx, n, n, 2, rows(1), rows(n + 1), draws="cell")
    assert len(g.user_csr["nbr2"]) == 0 and len(g.item_csr["nbr2"]) == 0 and len(g.user_degrees) == 0
    for mode in ("rs", "is"):
        g.to_device(mode=mode)
        ptrs = struct_pointers(g.struct)
        empty = ("u_nbr2", "i_nbr2") + (("u_deg2", "i_deg2") if mode == "is" else ())
        for k, v in g._dev.items():
            assert (v.numel() == 1 and v.dtype == torch.int32 and int(v[0]) == 0) == (k in empty), k
        assert all(ptrs[k] for k in ptrs if not k.endswith("_deg2"))
        assert bool(ptrs["user_deg2"]) == bool(ptrs["item_deg2"]) == (mode == "is") and ("u_deg2" in g._dev) == (mode == "is")
        assert ptrs["user_nbr2"] == g._dev["u_nbr2"].data_ptr() and ptrs["item_nbr2"] == g._dev["i_nbr2"].data_ptr()
    # log stores: no event in the window [3, 3) and no line -- both sides' sequences and the three line arrays are empty
    for dual in (True, False):
        s = PointLogStore(uid, iid, t_idx, t_idx, [], 3, 3, 5, 1, 2, rows(1), rows(n + 1), dual, build="host")
        assert s.n_lines == 0 and len(s.user_hist_seq) == 0 and (not dual or len(s.item_hist_seq) == 0)
        s.to_device()
        ptrs = struct_pointers(s.struct)
        for k in ("user_hist_seq", "line_user", "line_items", "line_last_item") + (("item_hist_seq",) if dual else ()):
            assert s._dev[k].numel() == 1 and s._dev[k].dtype == torch.int32 and ptrs[k] == s._dev[k].data_ptr() != 0, k
        for k in ("item_hist_off", "item_hist_seq", "item_hist_len"):
            assert (k in s._dev) == dual and bool(ptrs[k]) == dual, k
        assert all(ptrs[k] for k in ptrs if not k.startswith("item_hist"))
    # a file store in the single form: the item side is absent
    r = dp.remap_tmall_log(inputs("tmall")[0])
    log = inputs("tmall")[0]
    lines = dp.gen_target_lines(r["uid"], r["iid"], r["t_idx"], r["n_users"], r["n_items"], 9, 1, draws="cell")[:4]
    hists = dp.point_history_lines(r["uid"], r["iid"], log[:, 5], r["t_idx"], lines, 0, 9)
    files = dp.write_point_files(str(tmp_path), lines, hists[0], hists[1], r["user_rows"], r["item_rows"])
    for dual in (True, False):
        s = PointSeqStore(files[0], files[1], files[2] if dual else None, 6, 1, 4, files[3], files[4]).to_device()
        ptrs = struct_pointers(s.struct)
        for k in ("item_off", "item_seq", "item_len"):
            assert (k in s._dev) == dual and bool(ptrs[k]) == dual, k
        assert all(ptrs[k] == s._dev[k].data_ptr() != 0 for k in s._dev)
