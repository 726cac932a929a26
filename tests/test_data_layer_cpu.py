"""The data layer's shared rules without a GPU (score_amd/placement.py, dataprep._LogFront): the four pipelines check their
switches before they touch the log, every device entry point names itself in the one RuntimeError a machine without a GPU
gets, and the pipeline front hands out the remap's own host arrays."""
import os
import re

import numpy as np
import pytest
import torch

from score_amd import dataprep as dp
from score_amd import placement
from score_amd.graph import TemporalGraph
from score_amd.pointdata import DeviceDataLoaderDualSeq, DeviceDataLoaderUserSeq, PointLogStore, PointSeqStore
from score_amd.targets import TargetStore, UserNegLists

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Untouchable(object):
    """a log that fails the test as soon as anything reads it"""

    def _touched(self, *a, **k):
        raise AssertionError("the log was read before the switches were checked")
    __array__ = __getitem__ = __len__ = __iter__ = _touched
    shape = dtype = ndim = property(_touched)


LOG = Untouchable()
PIPELINES = {"tmall_pipeline": lambda **kw: dp.tmall_pipeline(LOG, **kw),
             "ccmr_pipeline": lambda **kw: dp.ccmr_pipeline(LOG, LOG, 5, 7, **kw),
             "tmall_point_stores": lambda **kw: dp.tmall_point_stores(LOG, **kw),
             "ccmr_point_stores": lambda **kw: dp.ccmr_point_stores(LOG, LOG, 5, 7, **kw)}
BAD_SWITCHES = [(dict(targets="device", draws="stream", build="host"), "targets='device' needs draws='cell'"),
                (dict(targets="host", sample_factor=4, build="host"), "sample_factor= needs targets='device'"),
                (dict(remap="device", build="host"), "remap='device' needs build='device'"),
                (dict(remap="gpu", build="host"), "remap is 'host' or 'device'"),
                (dict(targets="gpu", build="host"), "targets is 'host' or 'device'"),
                # targets is checked before remap, and both before build reaches a stage
                (dict(targets="gpu", remap="gpu", build="gpu"), "targets is 'host' or 'device'"),
                (dict(remap="gpu", build="gpu"), "remap is 'host' or 'device'")]


@pytest.mark.parametrize("kw,text", BAD_SWITCHES, ids=[t for _, t in BAD_SWITCHES[:5]] + ["targets first", "remap before build"])
@pytest.mark.parametrize("name", sorted(PIPELINES))
def test_switches_are_checked_before_the_log_is_read(name, kw, text):
    with pytest.raises(ValueError) as e:
        PIPELINES[name](**kw)
    assert str(e.value).startswith(text)


@pytest.fixture(scope="module")
def sample():
    log = np.load(os.path.join(GOLDEN, "tmall_sample_log.npz"))["log"]
    log.setflags(write=False)
    return log, dp.remap_tmall_log(log)


def test_check_build_and_the_callers_own_texts(sample):
    _, r = sample
    placement.check_build("host")
    placement.check_build("device")
    with pytest.raises(ValueError, match="^build is 'host' or 'device': got 'gpu'$"):
        placement.check_build("gpu")
    args = (r["uid"], r["iid"], r["t_idx"], r["n_users"], r["n_items"])
    for build, draws in (("gpu", "cell"), ("host", "block")):
        with pytest.raises(ValueError, match="^build is 'host' or 'device', draws 'stream' or 'cell': got %r, %r$" % (build, draws)):
            TemporalGraph.from_log(*args, 14, r["user_rows"], r["item_rows"], build=build, draws=draws)
    with pytest.raises(ValueError, match="^build must be 'device' or 'host'$"):
        PointLogStore(*args[:3], r["t_idx"], [], 0, 9, 300, 1, 2, r["user_rows"], r["item_rows"], True, build="gpu")
    for call in (lambda: TargetStore.from_log(*args, 9, 1, build="gpu"), lambda: UserNegLists.from_events([], [], 3, build="gpu"),
                 lambda: dp.remap_taobao_log(LOG, 0, 1, build="gpu"), lambda: dp.remap_ccmr_log(LOG, LOG, 5, 7, build="gpu")):
        with pytest.raises(ValueError, match="^build is 'host' or 'device': got 'gpu'$"):
            call()


def test_moved_names_stay_importable():
    from score_amd import logremap, targets
    assert logremap.device_of is placement.device_of and callable(logremap.upload_columns) and logremap.WIDE_MESSAGE
    assert targets.device_i32 is placement.device_i32 and targets._host is placement.to_host
    assert targets._is_tensor is placement.is_tensor
    assert placement.is_tensor(torch.zeros(1)) and not placement.is_tensor(np.zeros(1)) and not placement.is_tensor([1])
    a = np.arange(3)
    assert placement.to_host(a) is a and np.array_equal(placement.to_host(torch.arange(3)), a)


def needs(what, instead):
    return "^" + re.escape("%s needs an AMD GPU (HIP); %s" % (what, instead)) + "$"


def test_every_device_entry_point_names_itself_without_a_gpu(sample, tmp_path, monkeypatch):
    """(a machine with a GPU is told it has none: every one of these raises before it touches the device)"""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    log, r = sample
    c = dp.TMALL
    cols = (r["uid"], r["iid"], r["t_idx"])
    args = cols + (r["n_users"], r["n_items"])
    lines = dp.gen_target_lines(*args, c["pred_time_train"], 1, draws="cell")
    graph = TemporalGraph.from_log(*args, c["graph_time_slice_num"], r["user_rows"], r["item_rows"], draws="cell")
    log_store = PointLogStore(r["uid"], r["iid"], log[:, 5], r["t_idx"], lines, 0, c["pred_time_train"], 300, 1, 4, r["user_rows"],
                              r["item_rows"], True, build="host")
    hists = dp.point_history_lines(r["uid"], r["iid"], log[:, 5], r["t_idx"], lines, 0, c["pred_time_train"])
    files = dp.write_point_files(str(tmp_path), lines, hists[0], hists[1], r["user_rows"], r["item_rows"])
    seq_store = PointSeqStore(files[0], files[1], files[2], 6, 1, 4, files[3], files[4])
    g12 = np.load(os.path.join(GOLDEN, "g12_ccmr.npz"))
    d = g12["dims"].tolist()
    ccmr = (g12["log"], g12["movie_info"], d[0], d[1], tuple(d[4:8]))
    no_host, no_cpu = "build='host' does not", "batch assembly has no CPU path"
    entries = [
        ("TemporalGraph.from_log(build='device')", no_host,
         lambda: TemporalGraph.from_log(*args, 14, r["user_rows"], r["item_rows"], build="device", draws="cell")),
        ("TemporalGraph.to_device", no_cpu, graph.to_device),
        ("TargetStore.from_log(build='device')", no_host, lambda: TargetStore.from_log(*args, 9, 1, build="device")),
        ("UserNegLists.from_events(build='device')", no_host, lambda: UserNegLists.from_events([1], [4], 3, build="device")),
        ("PointSeqStore.to_device", no_cpu, seq_store.to_device),
        ("PointLogStore(build='device')", no_host,
         lambda: PointLogStore(r["uid"], r["iid"], log[:, 5], r["t_idx"], lines, 0, c["pred_time_train"], 300, 1, 4, r["user_rows"],
                               r["item_rows"], True, build="device")),
        ("PointLogStore.to_device", no_cpu, log_store.to_device),
        ("DeviceDataLoaderUserSeq", no_cpu, lambda: DeviceDataLoaderUserSeq(4, 6, files[0], files[1], 1, files[3], files[4])),
        ("DeviceDataLoaderDualSeq", no_cpu, lambda: DeviceDataLoaderDualSeq(4, 6, None, None, None, 1, None, None, store=log_store)),
        ("remap_tmall_log(build='device')", no_host, lambda: dp.remap_tmall_log(log, build="device")),
        ("remap_taobao_log(build='device')", no_host, lambda: dp.remap_taobao_log(LOG, 0, 1, build="device")),
        ("remap_ccmr_log(build='device')", no_host, lambda: dp.remap_ccmr_log(LOG, LOG, 5, 7, build="device")),
        # the pipelines: the remap raises where it runs on the device; else the stage that first needs the device
        ("remap_tmall_log(build='device')", no_host, lambda: dp.tmall_pipeline(log, build="device", draws="cell", remap="device")),
        ("remap_ccmr_log(build='device')", no_host, lambda: dp.ccmr_point_stores(*ccmr, build="device", remap="device")),
        ("targets='device'", "targets='host' does not", lambda: dp.tmall_pipeline(log, targets="device", draws="cell")),
        ("targets='device'", "targets='host' does not",
         lambda: dp.tmall_point_stores(log, build="device", targets="device", draws="cell")),
        ("targets='device'", "targets='host' does not", lambda: dp.ccmr_pipeline(*ccmr, build="device", targets="device", draws="cell")),
        ("TemporalGraph.from_log(build='device')", no_host, lambda: dp.tmall_pipeline(log, build="device", draws="cell")),
        ("PointLogStore(build='device')", no_host, lambda: dp.tmall_point_stores(log, build="device")),
    ]
    for what, instead, call in entries:
        with pytest.raises(RuntimeError, match=needs(what, instead)):
            call()
    assert graph._dev is None and seq_store._dev is None and log_store._dev is None


def test_front_hands_out_the_remaps_own_arrays(sample, monkeypatch):
    log, r = sample
    front = dp._LogFront(r, "host", raw_log=log)
    cols = front.host()
    assert cols[0] is r["uid"] and cols[1] is r["iid"] and cols[2] is r["t_idx"]               # the very arrays: no copy
    u, i, k, t = front.host(front.LOG4)
    assert u is r["uid"] and i is r["iid"] and t is r["t_idx"]
    assert "time_key" not in r and np.array_equal(k, log[:, 5]) and front.host(("time_key",))[0] is k      # made once
    # host targets on a host remap: every stage takes the host arrays, a device stage too (it uploads them itself)
    assert all(a is b for a, b in zip(front.stage("device", front.LOG4), (u, i, k, t)))
    assert all(a is b for a, b in zip(front.stage("host"), cols))
    # a remap that returns time_key (CCMR's) is asked for it, not the raw log
    r2 = dict(r, time_key=np.arange(len(r["uid"]), dtype=np.int32))
    assert dp._LogFront(r2, "host", raw_log=LOG).host(("time_key",))[0] is r2["time_key"]
    # device targets: a device stage shares the targets' upload -- which a machine without a GPU cannot make
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    shared = dp._LogFront(r, "device", raw_log=log)
    assert shared.stage("host")[0] is r["uid"]
    for ask in (shared.device, lambda: shared.stage("device")):
        with pytest.raises(RuntimeError, match=needs("targets='device'", "targets='host' does not")):
            ask()
