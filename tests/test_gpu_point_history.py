"""The point baselines' histories built from the interaction log ON THE DEVICE (csrc/pointhist.hip; score_amd/pointdata.py
PointLogStore(build="device")) and the batches assembled from them (score_point_batch_assemble_log).  Yardsticks, all exact:
the numpy build of the same store for the arrays; for the batches the host loaders over the files dataprep.point_history_lines /
write_point_files write -- pinned to the reference's own chain by tests/golden/g9_point_history.npz in
tests/test_point_history_cpu.py.  Nothing here is malformed: bad input is refused on the host (the CPU tests)."""
import itertools
import os

import numpy as np
import pytest
import torch

import point_hist_cases as phc
from helpers import GOLDEN
from score_amd import dataprep as dp
from score_amd.pointdata import (DataLoaderDualSeq, DataLoaderUserSeq, DeviceDataLoaderDualSeq, DeviceDataLoaderUserSeq,
                                 PointLogStore)
from test_point_history_cpu import load_case, log_store

pytestmark = pytest.mark.gpu
TAGS = ("neg1", "neg99")


def synth_case(time_scale=1):
    """a seeded log of a few thousand events: 'edge' users and items with exactly 1, 49, 50, 51, 64 and 65 events inside the
    window (T - 1, T, T + 1 at Caser's T = 50; H, H + 1 at hist_max_len 64), the rest random, days drawn from a dozen so that
    ties are the rule; Fu = 3, Fi = 4 (150- and 200-word spans at T = 50).  time_scale stretches the time key past 11 bits:
    entity and time no longer pack into one 32-bit sort key."""
    rng = np.random.default_rng(17)
    U, I, H, edge = 300, 500, 64, (1, 49, 50, 51, 64, 65)
    days = np.asarray([501, 502, 516, 517, 601, 602, 615, 616, 630, 701, 714, 715, 801], dtype=np.int64)
    ev = []
    for k, n in enumerate(edge):
        ev += [(1 + k, int(i), int(d)) for i, d in zip(rng.integers(U + 1 + 10, U + 1 + I // 2, n), rng.choice(days[2:11], n))]
        ev += [(int(u), U + 1 + k, int(d)) for u, d in zip(rng.integers(1 + 10, 1 + U // 2, n), rng.choice(days[2:11], n))]
    n_rest = 3000
    ev += list(zip(rng.integers(1 + U // 2, U + 1, n_rest).tolist(), rng.integers(U + 1 + I // 2, U + I + 1, n_rest).tolist(),
                   rng.choice(days, n_rest).tolist()))
    ev = np.asarray(ev, dtype=np.int64)[rng.permutation(len(ev))]
    ev = np.concatenate([ev, [[U, U + I, 601]]])
    t_idx = dp.tmall_slice_index(ev[:, 2])
    start, pred = 1, 5
    inwin = (t_idx >= start) & (t_idx < pred)
    with_hist = np.unique(ev[inwin, 0])
    per, n_lines = 2, 31                                               # B = 10: six batches and a line left over
    lines = []
    for l in range(n_lines):
        u = 1 + l if l < len(edge) else int(rng.choice(with_hist))
        items = [int(x) for x in rng.integers(U + 1, U + I + 1, per + 1)]
        if l < 10:                                                     # (the later batches hold no long item history)
            items[l % per] = U + 1 + l % len(edge)
        lines.append((u, items))
    user_rows = np.concatenate([np.arange(1, U + 1)[:, None], rng.integers(U + I + 1, U + I + 40, (U, 2))], axis=1)
    item_rows = np.concatenate([np.arange(U + 1, U + I + 1)[:, None], rng.integers(U + I + 40, U + I + 90, (I, 3))], axis=1)
    return dict(uid=ev[:, 0], iid=ev[:, 1], time_key=ev[:, 2] * time_scale, t_idx=t_idx, lines=lines, start=start, pred=pred,
                H=H, neg=per - 1, B=10, user_rows=user_rows, item_rows=item_rows, Ts=[50], N=U + I + 90)


def _files_and_host(c, root, Ts):
    """the case's files (written from point_history_lines) and the host loaders' batches per (dual, T)"""
    users, items = dp.point_history_lines(c["uid"], c["iid"], c["time_key"], c["t_idx"], c["lines"], c["start"], c["pred"], c["H"])
    paths = dp.write_point_files(root, c["lines"], users, items, c["user_rows"], c["item_rows"])
    tf, uf, itf, ud, idd = paths
    host = {}
    for T in Ts:
        host[(False, T)] = list(DataLoaderUserSeq(c["B"], T, tf, uf, c["neg"], ud, idd))
        host[(True, T)] = list(DataLoaderDualSeq(c["B"], T, tf, uf, itf, c["neg"], ud, idd))
    return paths, host


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """every g9 case and the synthetic log: files, host batches (computed once, never modified) and both builds of the store"""
    root = tmp_path_factory.mktemp("point_history")
    z = np.load(os.path.join(GOLDEN, "g9_point_history.npz"))
    out = {}
    for tag in TAGS + ("synth", "synth_wide"):
        c = load_case(z, tag) if tag in TAGS else synth_case(1 if tag == "synth" else 1000003)
        if tag == "synth_wide":
            out[tag] = dict(c=c)
            continue
        paths, host = _files_and_host(c, str(root / tag), c["Ts"])
        out[tag] = dict(c=c, paths=paths, host=host)
    return out


def _same_arrays(dev, host):
    a, b = dev.arrays(), host.arrays()
    for k in PointLogStore.HIST:
        if b[k] is None:
            assert a[k] is None, k
            continue
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(a[k], b[k]), k
    for k in ("batch_max_user_len", "batch_max_len", "batch_min_len"):
        assert np.array_equal(getattr(dev, k), getattr(host, k)), k


@pytest.mark.parametrize("tag", TAGS + ("synth", "synth_wide"))
def test_device_build_equals_the_host_build(cases, tag):
    c = cases[tag]["c"]
    for dual in (False, True):
        dev, host = log_store(c, dual, build="device"), log_store(c, dual, build="host")
        _same_arrays(dev, host)
        assert dev.time_bits == int(np.max(c["time_key"])).bit_length() and (dev.time_bits > 23) == (tag == "synth_wide")
    if tag.startswith("synth"):
        a = host.arrays()
        U = host.n_users
        assert np.diff(a["user_hist_off"])[:6].tolist() == [1, 49, 50, 51, 64, 65] == np.diff(a["item_hist_off"])[:6].tolist()
        assert a["user_hist_len"][:6].tolist() == [1, 49, 50, 51, 64, 64] and a["user_hist_len"][U - 1] > 0
        assert (np.diff(a["user_hist_off"]) == 0).any() and (np.diff(a["item_hist_off"]) == 0).any()
        # one sort where entity and time pack into 32 bits, two where they do not: the same histories either way
        assert int(U).bit_length() + dev.time_bits > 32 or tag == "synth"
        _same_arrays(dev, log_store(cases["synth"]["c"], True, build="host"))


def _models(dual, N, T, Fu, Fi):
    from score_amd import model as M
    kinds = (M.DELF, M.DEEMS) if dual else ((M.GRU4Rec, M.Caser) if T >= M.Caser.CONV_L else (M.GRU4Rec,))
    return [k(N, 4, 16, T, Fu, Fi, seed=3) for k in kinds]


def _device(dual, c, T, store, **kw):
    if dual:
        return DeviceDataLoaderDualSeq(c["B"], T, None, None, None, c["neg"], None, None, store=store, **kw)
    return DeviceDataLoaderUserSeq(c["B"], T, None, None, c["neg"], None, None, store=store, **kw)


def _check_batches(dual, loader, host):
    """every batch of `loader`, copied back, against the host loader's tuples: the fields, the unused tensors, the count"""
    from score_amd.model import DeviceBatch
    n = 7 if dual else 5
    assert len(loader) == len(host) > 0
    got = list(loader)
    assert len(got) == len(host)
    for i, (db, want) in enumerate(zip(got, host)):
        assert isinstance(db, DeviceBatch) and len(db) == n and db.B == len(want[-1]) and len(db.tensors) == (9 if dual else 8)
        for k in range(n):
            x = db[k]
            assert x.dtype == torch.int32 and tuple(x.shape) == want[k].shape, (i, k)
            assert np.array_equal(x.cpu().numpy(), want[k]), (i, k)
        for k in ((1, 3) if dual else (1, 2, 3)):
            assert not bool(db.tensors[k].any()), (i, k)
        assert db.active_slices == 0
    with pytest.raises(StopIteration):
        next(loader)


@pytest.mark.parametrize("tag", TAGS + ("synth",))
@pytest.mark.parametrize("dual", [False, True])
def test_loaders_over_a_log_store_equal_the_host_loaders_over_the_files(cases, dual, tag):
    from score_amd.model import DeviceBatch
    c, host = cases[tag]["c"], cases[tag]["host"]
    store = log_store(c, dual, build="device")              # ONE store, read at every T of the case without a rebuild
    seen = set()
    for T in c["Ts"]:
        want = host[(dual, T)]
        first = _device(dual, c, T, store)
        assert first.store is store
        _check_batches(dual, first, want)
        N = c.get("N", 1 + int(max(c["user_rows"].max(), c["item_rows"].max())))
        for m in _models(dual, N, T, store.Fu, store.Fi):       # (no step runs: the table's size does not matter)
            again = _device(dual, c, T, store, model=m)
            for db, w in zip(again, want):
                assert db.active_slices == DeviceBatch(m, w).active_slices, (type(m).__name__, tag, T)
                seen.add((type(m).__name__, db.active_slices > 0))
        with pytest.raises(ValueError):                         # a model of another T is refused
            _device(dual, c, T, store, model=_models(dual, N, T + 1, store.Fu, store.Fi)[0])
    for kind in (("DELF", "DEEMS") if dual else ("GRU4Rec",)):  # batches below T exist, and batches at T
        assert (kind, True) in seen and (tag == "neg99" or (kind, False) in seen)
    assert dual or tag != "synth" or ("Caser", False) in seen and ("Caser", True) not in seen


@pytest.mark.parametrize("dual", [False, True])
def test_an_uploaded_host_build_yields_the_same_batches(cases, dual):
    c, host = cases["neg1"]["c"], cases["neg1"]["host"]
    store = log_store(c, dual, build="host")
    for T in c["Ts"]:
        _check_batches(dual, _device(dual, c, T, store), host[(dual, T)])


@pytest.mark.parametrize("kind", ["GRU4Rec", "DEEMS"])
def test_training_on_the_tmall_sample_from_the_log_equals_training_from_the_files(tmp_path, kind):
    """five steps at B = 200 on the bundled sample, fed from the log store and from the file-based device loader over the
    written files: the batches are equal, so losses and variables are bit-identical.  (The sample's train slice has 41 lines
    -- no batch of 200 at one negative --, so the steps run on the validation slice's lines, 99 negatives each.)"""
    from score_amd import model as M
    dual = kind == "DEEMS"
    log = np.load(os.path.join(GOLDEN, "tmall_sample_log.npz"))["log"]
    stores, r = dp.tmall_point_stores(log, dual=dual, batch_size=200)
    st = stores["validation"]
    assert st.n_batches >= 5 and st.hist_max_len == 300
    _, _, targets = dp.tmall_pipeline(log)
    pt = dp.TMALL["pred_time_validation"]
    users, items = dp.point_history_lines(r["uid"], r["iid"], log[:, 5], r["t_idx"], targets["validation"], 0, pt)
    tf, uf, itf, ud, idd = dp.write_point_files(str(tmp_path), targets["validation"], users, items, r["user_rows"], r["item_rows"])
    T, B, neg = 20, 200, 99
    runs = []
    for fed in ("log", "files"):
        m = M.MODELS[kind](r["feature_size"], 16, 32, T, 3, 4, seed=7)
        if fed == "log":
            loader = (DeviceDataLoaderDualSeq(B, T, None, None, None, neg, None, None, model=m, store=st) if dual else
                      DeviceDataLoaderUserSeq(B, T, None, None, neg, None, None, model=m, store=st))
        else:
            loader = (DeviceDataLoaderDualSeq(B, T, tf, uf, itf, neg, ud, idd, model=m) if dual else
                      DeviceDataLoaderUserSeq(B, T, tf, uf, neg, ud, idd, model=m))
        batches = list(itertools.islice(loader, 5))
        losses = [m.train(None, b, 1e-2, 1e-4) for b in batches]
        torch.cuda.synchronize()
        runs.append((np.asarray(losses, dtype=np.float64), m.get_params(), batches))
    (la, pa, ba), (lb, pb, bb) = runs
    print("losses log-fed", la.tolist(), "file-fed", lb.tolist())
    for x, y in zip(ba, bb):
        assert x.active_slices == y.active_slices
        for k in range(len(x)):
            assert torch.equal(x[k], y[k]), k
    assert len(la) == 5 and np.isfinite(la).all() and np.array_equal(la, lb)
    assert sorted(pa) == sorted(pb)
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k


# ---- score_point_hist_build itself at the sort's pass, tile and id-range edges (tests/point_hist_cases.py) -------------------
POISON = -7


def _build_call(lib, ent, other, d, c, temp, temp_bytes):
    """one score_point_hist_build of the arguments c over the device columns (ent, other, d["time_key"], d["t_idx"]), on the
    current stream, into poisoned outputs"""
    import ctypes as C
    ptr = lambda t: C.c_void_p(t.data_ptr())
    off = torch.full((c["n_ent"] + 1,), POISON, dtype=torch.int64, device="cuda")
    seq = torch.full((c["n"],), POISON, dtype=torch.int32, device="cuda")
    ln = torch.full((c["n_ent"],), POISON, dtype=torch.int32, device="cuda")
    rc = lib.score_point_hist_build(ptr(ent), ptr(other), ptr(d["time_key"]), ptr(d["t_idx"]),
                                    c["n"], c["start"], c["pred"], c["id_lo"], c["n_ent"], c["time_bits"], c["H"], ptr(off), ptr(seq),
                                    ptr(ln), ptr(temp), temp_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, off, seq, ln


@pytest.mark.parametrize("name", phc.NAMES)
def test_hist_build_equals_the_restatement_at_the_sorts_edges(name):
    """the build called directly, twice back to back into ONE workspace -- the case, then the two id columns exchanged, as
    PointLogStore._build_device does for the two sides --, against the plain-Python restatement: off, len, the window's words of
    seq, zeros behind them (the header's promise), nothing left unwritten; and a workspace one byte short is refused untouched"""
    from score_amd import _lib
    lib = _lib.load()
    first = phc.case(name)
    second = phc.swapped(first)
    d = {k: torch.from_numpy(first[k].copy()).cuda() for k in ("ent", "other", "time_key", "t_idx")}   # (read-only arrays)
    temp_bytes = int(lib.score_point_hist_temp_bytes(first["n"]))
    assert temp_bytes > 0
    temp = torch.empty((temp_bytes,), dtype=torch.uint8, device="cuda")
    rc, off, seq, ln = _build_call(lib, d["ent"], d["other"], d, first, temp, temp_bytes - 1)
    torch.cuda.synchronize()
    assert rc == -3                                                  # SCORE_E_WORKSPACE
    assert bool((off == POISON).all()) and bool((seq == POISON).all()) and bool((ln == POISON).all())
    runs = [_build_call(lib, d["ent"], d["other"], d, first, temp, temp_bytes),
            _build_call(lib, d["other"], d["ent"], d, second, temp, temp_bytes)]
    torch.cuda.synchronize()
    for which, (c, (rc, off, seq, ln)) in enumerate(zip((first, second), runs)):
        want_off, want_seq, want_len = phc.expected(name, swap=bool(which))
        assert rc == 0, which
        off, seq, ln = off.cpu().numpy(), seq.cpu().numpy(), ln.cpu().numpy()
        used = int(want_off[-1])
        print(name, "build", which, "structure", phc.structure(c["n_ent"], c["time_bits"]), "words in the window", used)
        assert np.array_equal(off, want_off), which
        assert np.array_equal(ln, want_len), which
        assert np.array_equal(seq[:used], want_seq), which
        assert not seq[used:].any(), which


# ---- the loaders at the assembly kernel's edges: T = 1; T > H; T * Fu > 4,096 (one sample per chunk); T * Fi = 8,192 (all LDS) --
EDGE_TS = (1, 65, 1400, 2048)


@pytest.fixture(scope="module")
def edge(cases, tmp_path_factory):
    """the synthetic case's files and the host loaders' batches at every edge T (computed once, never modified), and ONE
    device-built store per form, read at every T"""
    c = cases["synth"]["c"]
    _, host = _files_and_host(c, str(tmp_path_factory.mktemp("point_history_edges")), EDGE_TS)
    stores = {dual: log_store(c, dual, build="device") for dual in (False, True)}
    return c, host, stores


@pytest.mark.parametrize("T", EDGE_TS)
@pytest.mark.parametrize("dual", [False, True])
def test_loaders_at_the_assembly_kernels_edges(edge, dual, T):
    c, host, stores = edge
    store = stores[dual]
    assert (store.Fu, store.Fi, store.hist_max_len, c["B"]) == (3, 4, 64, 10)
    assert 1400 * store.Fu > 4096 and 2048 * store.Fi == 8192 and 65 > store.hist_max_len
    _check_batches(dual, _device(dual, c, T, store), host[(dual, T)])


@pytest.mark.parametrize("dual", [False, True])
def test_a_max_len_past_the_assembly_kernels_lds_is_refused(edge, dual):
    c, _, stores = edge
    with pytest.raises(ValueError, match="max_len 2049"):   # T * Fi = 8,196 words: the store's check, in front of any launch
        _device(dual, c, 2049, stores[dual])
