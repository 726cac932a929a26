"""The temporal graph store built from the log ON THE DEVICE (csrc/graphbuild.hip; TemporalGraph.from_log(build="device"))
against the host build of the same rule, from_log(build="host", draws="cell") -- itself pinned to a plain-Python restatement
and to the reference's documents in test_graph_cell_draws.py.  Exact integers; the outputs are poisoned first."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import graph_cell_cases as cc
from score_amd import _lib
from score_amd.graph import DeviceGraphLoader, TemporalGraph

pytestmark = pytest.mark.gpu
POISON = -0x5A5A5A5B
E_SHAPE, E_WORKSPACE = -2, -3


@functools.lru_cache(maxsize=None)
def host_arrays(name):
    """the host build's arrays per side (computed once, never modified)"""
    uid, iid, t, U, I, S, m1, m2, seed = cc.case(name)
    ur, ir = cc.rows(U, I)
    g = TemporalGraph.from_log(uid, iid, t, U, I, S, ur, ir, max_1hop=m1, max_2hop=m2, seed=seed, draws="cell")
    out = {}
    for p, csr, deg in (("u", g.user_csr, g.user_degrees), ("i", g.item_csr, g.item_degrees)):
        out[p] = dict(off1=csr["off1"], nbr1=csr["nbr1"], off2=csr["off2"], nbr2=csr["nbr2"], deg2=deg)
        for a in out[p].values():
            a.setflags(write=False)
    return out


class Build(object):
    """one device build through the C ABI into poisoned outputs; temp may be shared between builds"""

    def __init__(self, c, temp=None, temp_short=0):
        uid, iid, t, U, I, S, m1, m2, seed = c
        self.lib, self.dev = _lib.load(), torch.device("cuda")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.dev)
        self.log = [up(uid), up(iid), up(t)]
        self.n, self.ncell = len(uid), {"u": U * S, "i": I * S}
        need = int(self.lib.score_graph_build_temp_bytes(self.n, U, I, S))
        assert need > 0
        self.temp = temp if temp is not None else torch.empty((need,), dtype=torch.uint8, device=self.dev)
        assert self.temp.numel() >= need
        self.temp_bytes = need - temp_short
        poison = lambda n, dt: torch.full((n,), POISON, dtype=dt, device=self.dev)
        self.out = {}
        for p in "ui":
            self.out[p] = dict(off1=poison(self.ncell[p] + 1, torch.int64), nbr1=poison(self.n, torch.int32),
                               off2=poison(self.ncell[p] + 1, torch.int64))
        ptr = lambda x: x.data_ptr()
        self.args = _lib.GraphBuild(C.sizeof(_lib.GraphBuild), ptr(self.log[0]), ptr(self.log[1]), ptr(self.log[2]), self.n, U, I,
                                    S, m1, m2, 0, seed, ptr(self.out["u"]["off1"]), ptr(self.out["u"]["nbr1"]),
                                    ptr(self.out["i"]["off1"]), ptr(self.out["i"]["nbr1"]))
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def hop1(self):
        return self.lib.score_graph_build_1hop(C.byref(self.args), self.temp.data_ptr(), self.temp_bytes, self.stream)

    def hop2(self, p):
        o, total = self.out[p], C.c_int64(-1)
        rc = self.lib.score_graph_build_2hop(C.byref(self.args), int(p == "i"), o["off2"].data_ptr(), None, None, 0,
                                             C.byref(total), self.temp.data_ptr(), self.temp_bytes, self.stream)
        if rc != 0:
            return rc
        o["total"] = int(total.value)
        pad = 64                                   # poison behind the used range: nothing may be written there
        o["nbr2"] = torch.full((o["total"] + pad,), POISON, dtype=torch.int32, device=self.dev)
        o["deg2"] = torch.full((o["total"] + pad,), POISON, dtype=torch.int32, device=self.dev)
        return self.lib.score_graph_build_2hop(C.byref(self.args), int(p == "i"), o["off2"].data_ptr(), o["nbr2"].data_ptr(),
                                               o["deg2"].data_ptr(), max(o["total"], 1), None, self.temp.data_ptr(),
                                               self.temp_bytes, self.stream)

    def run(self):
        assert self.hop1() == 0
        assert self.hop2("i") == 0                 # the reference's pass order: items, then users
        assert self.hop2("u") == 0
        torch.cuda.synchronize()
        return self

    def all_poison(self):
        torch.cuda.synchronize()
        return all(bool((a == POISON).all()) for o in self.out.values() for a in o.values() if torch.is_tensor(a))


def assert_equals_host(b, name):
    host = host_arrays(name)
    for p in "ui":
        o, h = b.out[p], host[p]
        n1 = len(h["nbr1"])
        assert torch.equal(o["off1"].cpu(), torch.from_numpy(h["off1"].copy())), (name, p, "off1")
        assert np.array_equal(o["nbr1"][:n1].cpu().numpy(), h["nbr1"]), (name, p, "nbr1")
        assert not bool((o["nbr1"] == POISON).any()), (name, p, "nbr1 poison")       # (the sink's words are zero)
        assert torch.equal(o["off2"].cpu(), torch.from_numpy(h["off2"].copy())), (name, p, "off2")
        assert o["total"] == len(h["nbr2"]) == int(h["off2"][-1]), (name, p, "total")
        for k in ("nbr2", "deg2"):
            got = o[k].cpu().numpy()
            assert np.array_equal(got[:o["total"]], h[k]), (name, p, k)
            assert not (got[:o["total"]] == POISON).any() and (got[o["total"]:] == POISON).all(), (name, p, k)


@pytest.mark.parametrize("name", cc.SMALL_CASES + cc.BIG_CASES)
def test_device_build_equals_host_cell_build(name):
    assert_equals_host(Build(cc.case(name)).run(), name)


def test_cases_hold_what_they_are_for():
    # (what the shared logs exercise is asserted from the restatement in test_graph_cell_draws.py; here: the host arrays the
    # device is compared with really have over-long cells, capped lists and a skipped shuffle where the names say so)
    e, n = host_arrays("edges"), host_arrays("no_over_long")
    assert (np.diff(e["i"]["off1"]) > 3).any() and (np.diff(e["u"]["off2"]) == 5).any()
    assert not (np.diff(n["i"]["off1"]) > 64).any() and not (np.diff(n["u"]["off1"]) > 64).any()
    s = host_arrays("tile_seam")
    assert {8192, 8193} <= set(np.diff(s["i"]["off1"]).tolist())
    k = host_arrays("sink")
    assert 0 < int(k["u"]["off1"][-1]) < len(cc.case("sink")[0])


def test_two_builds_back_to_back_in_one_workspace():
    lib = _lib.load()
    ca, cb = cc.case("tile_seam"), cc.case("edges")
    need = max(int(lib.score_graph_build_temp_bytes(len(c[0]), c[3], c[4], c[5])) for c in (ca, cb))
    temp = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    a = Build(ca, temp=temp)
    b = Build(cb, temp=temp)
    a.run()
    b.run()                                        # (no wait, no clearing in between: what the first left is in temp)
    assert_equals_host(a, "tile_seam")
    assert_equals_host(b, "edges")
    a2 = Build(ca, temp=temp).run()
    assert_equals_host(a2, "tile_seam")


def test_short_workspace_and_shape_are_refused_before_any_launch():
    c = cc.case("edges")
    b = Build(c, temp_short=1)
    assert b.hop1() == E_WORKSPACE
    assert b.hop2("i") == E_WORKSPACE
    assert b.all_poison()
    wide = c[:6] + (65, 100, 1)                    # max_1hop^2 > 4096
    b = Build(wide)
    assert b.hop1() == E_SHAPE and b.hop2("u") == E_SHAPE
    assert b.all_poison()
    assert Build(c[:6] + (64, 100, 1)).hop1() == 0
    torch.cuda.synchronize()
    bad = Build(c)
    bad.args.struct_bytes -= 8
    assert bad.hop1() == -1 and bad.all_poison()


# ---- downstream, on the bundled Tmall sample ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sample():
    from score_amd import dataprep as dp
    raw = np.load(cc.GOLDEN + "/tmall_sample_log.npz")["log"]
    r = dp.remap_tmall_log(raw)
    c = dp.TMALL
    kw = dict(max_1hop=c["max_1hop"], max_2hop=c["max_2hop"], seed=11, draws="cell")
    args = (r["uid"], r["iid"], r["t_idx"], r["n_users"], r["n_items"], c["graph_time_slice_num"], r["user_rows"], r["item_rows"])
    host = TemporalGraph.from_log(*args, **kw)
    dev = TemporalGraph.from_log(*args, build="device", **kw)
    lines = dp.gen_target_lines(r["uid"], r["iid"], r["t_idx"], r["n_users"], r["n_items"], c["pred_time_train"], 1,
                                c["start_time"], 5)
    return dict(host=host, dev=dev, lines=lines, r=r, c=c)


def _loader(g, s, batch=16):
    c = s["c"]
    return DeviceGraphLoader(g, batch, s["lines"], c["start_time"], c["pred_time_train"], 1, c["time_slice_num"] - c["start_time"] - 1,
                             c["obj_per_time_slice"], seed=77)


@pytest.mark.parametrize("mode", ["rs", "is"])
def test_loader_batches_equal_over_both_builds(sample, mode):
    d, h = sample["dev"], sample["host"]
    assert d._built is not None and d._dev is not None and not d.__dict__.get("_downloaded")    # born resident
    ptrs = {k: v.data_ptr() for k, v in d._built.items()}
    d.to_device(mode=mode)
    h.to_device(mode=mode)
    assert all(d._dev[k].data_ptr() == ptrs[k] for k in d._dev) and not d.__dict__.get("_downloaded")   # no upload, no download
    assert ("u_deg2" in d._dev) == (mode == "is") and d.struct.sample_mode == (1 if mode == "is" else 0)
    n = 0
    for a, b in zip(_loader(d, sample), _loader(h, sample)):
        assert len(a.tensors) == len(b.tensors) == 8
        assert all(torch.equal(x, y) for x, y in zip(a.tensors, b.tensors))
        n += 1
    assert n >= 2


def test_three_training_steps_equal_over_both_builds(sample):
    from score_amd.model import SCORE
    c, r = sample["c"], sample["r"]
    T = c["time_slice_num"] - c["start_time"] - 1
    runs = []
    for g in (sample["dev"], sample["host"]):
        g.to_device(mode="rs")
        m = SCORE(r["feature_size"], 8, 16, T, c["obj_per_time_slice"], c["user_fnum"], c["item_fnum"], seed=3)
        losses = [m.train(None, b, 1e-3, 1e-4) for b, _ in zip(_loader(g, sample), range(3))]
        torch.cuda.synchronize()
        runs.append((losses, m.table.clone(), m.w.clone()))
    assert len(runs[0][0]) == 3 and all(np.isfinite(runs[0][0]))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


def test_save_of_the_device_built_graph_loads_as_the_host_build(sample, tmp_path):
    d, h = sample["dev"], sample["host"]
    g = TemporalGraph.load(d.save(str(tmp_path / "g.npz")))
    for a, b in ((g.user_csr, h.user_csr), (g.item_csr, h.item_csr)):
        for k in ("off1", "nbr1", "off2", "nbr2"):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert np.array_equal(g.user_degrees, h.user_degrees) and np.array_equal(g.item_degrees, h.item_degrees)
    assert np.array_equal(g.user_rows, h.user_rows) and np.array_equal(g.item_rows, h.item_rows)
    assert (g.U, g.I, g.S) == (h.U, h.I, h.S)
    # the host view of the device-built graph itself
    assert np.array_equal(d.cell("user", 2, 0, 3), h.cell("user", 2, 0, 3))
    assert np.array_equal(d.user_degrees, h.user_degrees) and np.array_equal(d.item_degrees, h.item_degrees)
