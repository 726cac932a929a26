"""The raw log's remap on the host (dataprep.remap_tmall_log, remap_taobao_log(build="host"), tmall_slice_index) against a
plain-Python dict restatement of the two scripts (remap_cases.py) and, for Taobao, against the reference's own code through
g11_taobao_remap.npz (tests/golden/make_taobao_remap_golden.py).  The device build is pinned to these host builds in
test_gpu_log_remap.py."""
import numpy as np
import pytest

import remap_cases as rc
from score_amd import dataprep as dp


def _same(got, want, keys):
    for k in keys:
        g, w = got[k], want[k]
        if isinstance(w, (int, tuple)):
            assert g == w, k
        else:
            assert np.array_equal(np.asarray(g), np.asarray(w).reshape(np.asarray(g).shape)), k


def test_tmall_host_remap_equals_the_dict_restatement():
    log = rc.tmall_sample()
    got = dp.remap_tmall_log(log)
    want = rc.restate_tmall(log, (log[:, 0] % 9).tolist(), (log[:, 0] % 3).tolist())
    _same(got, want, ("uid", "iid", "t_idx", "n_users", "n_items", "feature_size", "user_rows", "item_rows", "vocab_sizes"))
    assert (got["n_users"], got["n_items"], got["feature_size"]) == (62, 5915, 9274)
    assert sorted(set(got["t_idx"].tolist())) == list(range(13)) and (log[:, 4] == -1).any()
    # a given profile is used as it is
    age, gender = (log[:, 1] % 5), (log[:, 2] % 2)
    _same(dp.remap_tmall_log(log, age=age, gender=gender), rc.restate_tmall(log, age.tolist(), gender.tolist()),
          ("uid", "iid", "feature_size", "user_rows", "item_rows", "vocab_sizes"))


TAOBAO_KEYS = ("uid", "iid", "t_idx", "n_users", "n_items", "feature_size", "item_rows", "user_rows", "vocab_sizes", "kept")


@pytest.mark.parametrize("mode,n", [("mixed", 300), ("all", 50), ("last", 40), ("none", 30)])
def test_taobao_host_remap_equals_the_dict_restatement(mode, n):
    log, start, end, delta = rc.taobao_log(n, mode)
    got = dp.remap_taobao_log(log, start, end, delta)
    want = rc.restate_taobao(log, start, end, delta)
    assert len(want["kept"]) == {"all": n, "last": 1, "none": 0}.get(mode, len(want["kept"]))
    if mode == "mixed":
        assert 0 < len(want["kept"]) < n
    _same(got, want, TAOBAO_KEYS)
    assert got["uid"].dtype == got["iid"].dtype == got["t_idx"].dtype == got["item_rows"].dtype == np.int32
    assert got["item_rows"].shape == (got["n_items"], 2) and got["user_rows"].shape == (got["n_users"], 1)


def test_taobao_host_remap_on_g11_equals_the_dict_restatement():
    g = rc.g11()
    start, end, delta = g["start_end"].tolist()
    _same(dp.remap_taobao_log(g["raw"], start, end, delta), rc.restate_taobao(g["raw"], start, end, delta), TAOBAO_KEYS)
    with pytest.raises(ValueError, match="delta"):
        dp.remap_taobao_log(g["raw"], start, end, 0)
    with pytest.raises(ValueError, match="build"):
        dp.remap_taobao_log(g["raw"], start, end, build="gpu")


def _bijection(ref, ours, lo, size):
    """reference id -> our id is a bijection onto the block lo .. lo + size - 1"""
    m = {}
    for a, b in zip(ref.tolist(), ours.tolist()):
        assert m.setdefault(a, b) == b
    assert sorted(m.values()) == list(range(lo, lo + size)) and len(set(m)) == size
    return m


def test_taobao_host_remap_equals_the_reference():
    """feateng_taobao.preprocess_raw_data numbered the vocabularies in set order: the same kept lines in the same order, equal
    slices, a bijection per vocabulary onto its block (users, then items, then categories), the same item_feat_dict"""
    g = rc.g11()
    raw, ref, feat = g["raw"], g["remapped"], g["item_feat"]
    start, end, delta = g["start_end"].tolist()
    assert (start, end, delta) == (1511568000, 1512345600, dp.TAOBAO_SLICE_SECONDS)      # the reference's dates at UTC
    r = dp.remap_taobao_log(raw, start, end)
    t = raw[:, 4]
    # what the fixture is for
    assert (t == start).any() and (t == end).any() and (t == start - 1).any() and (t == end + 1).any()
    assert ((raw[:, 3] == 0) & (t >= start) & (t <= end)).any()
    kept = r["kept"]
    assert len(kept) == len(ref) and kept[np.isin(t[kept], (start, end))].size >= 2 and (raw[kept, 3] == 1).all()
    assert not np.isin(np.flatnonzero(np.isin(t, (start - 1, end + 1))), kept).any()
    assert set(raw[:, 0].tolist()) - set(raw[kept, 0].tolist())                         # a user all of whose events are dropped
    # the same lines in the same order: as many, and the reference's ids group the kept events exactly as the raw values do
    for j in range(3):
        pairs = set(zip(ref[:, j].tolist(), raw[kept, j].tolist()))
        assert len(pairs) == len(set(ref[:, j].tolist())) == len(set(raw[kept, j].tolist())), j
    assert np.array_equal(r["t_idx"], ref[:, 3]) and r["t_idx"].min() == 0 and r["t_idx"].max() == 9
    U, I, Cn = r["vocab_sizes"]
    assert r["feature_size"] == 1 + U + I + Cn and (r["n_users"], r["n_items"]) == (U, I)
    mu = _bijection(ref[:, 0], r["uid"], 1, U)
    mi = _bijection(ref[:, 1], r["iid"], 1 + U, I)
    # (the dict holds no category id per event: the first-appearance rule over the kept events gives it, and item_rows,
    # compared below, holds what the build itself assigned)
    d, _ = rc.first_appearance_dict(raw[kept, 2].tolist(), 1 + U + I)
    mc = _bijection(ref[:, 2], np.asarray([d[v] for v in raw[kept, 2].tolist()]), 1 + U + I, Cn)
    assert len(mu) == U and np.array_equal(r["user_rows"][:, 0], np.arange(1, U + 1))
    # item_feat_dict through the bijections; an item whose category changed keeps the LAST kept one
    want = np.asarray(sorted([mi[int(a)], mc[int(b)]] for a, b in feat), dtype=np.int32)
    assert np.array_equal(r["item_rows"], want)
    changed = [i for i in set(raw[kept, 1].tolist()) if len(set(raw[kept][raw[kept, 1] == i, 2].tolist())) > 1]
    assert changed
    for i in changed:
        ev = kept[raw[kept, 1] == i]
        row = r["item_rows"][r["iid"][np.flatnonzero(kept == ev[0])[0]] - 1 - U]
        assert row[1] == d[int(raw[ev[-1], 2])] != d[int(raw[ev[0], 2])]


def test_slice_arithmetic():
    """the rule the device evaluates (days before the month + day - 121, floor division by 15), restated in numpy, equals
    tmall_slice_index on every date of 2015; an invalid MMDD raises"""
    v = rc.valid_dates_2015()
    assert len(v) == 365
    before = np.asarray([0, 0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334])
    want = dp.tmall_slice_index(v)
    got = (before[v // 100] + v % 100 - 121) // 15
    assert np.array_equal(got, want) and want.min() == -8 and want[v == 430][0] == -1 and want[v == 501][0] == 0
    assert want[v == 101][0] == -8 and want.max() == 16
    for bad in rc.INVALID_DATES:
        with pytest.raises(ValueError):
            dp.tmall_slice_index(np.asarray([501, bad]))


def test_device_builds_need_a_gpu_and_remap_needs_the_device_build():
    import torch
    log = rc.tmall_sample()
    with pytest.raises(ValueError, match="remap='device' needs build='device'"):
        dp.tmall_pipeline(log, remap="device")
    with pytest.raises(ValueError, match="remap='device' needs build='device'"):
        dp.tmall_point_stores(log, build="host", remap="device")
    with pytest.raises(ValueError, match="remap is 'host' or 'device'"):
        dp.tmall_pipeline(log, remap="gpu")
    with pytest.raises(ValueError, match="build is 'host' or 'device'"):
        dp.remap_tmall_log(log, build="gpu")
    if not torch.cuda.is_available():
        g = rc.g11()
        with pytest.raises(RuntimeError, match="needs an AMD GPU"):
            dp.remap_tmall_log(log, build="device")
        with pytest.raises(RuntimeError, match="needs an AMD GPU"):
            dp.remap_taobao_log(g["raw"], int(g["start_end"][0]), int(g["start_end"][1]), build="device")
