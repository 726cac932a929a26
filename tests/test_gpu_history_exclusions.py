"""History exclusions built on the device (csrc/histexcl.hip: score_catalog_history_exclusions) through the C entry with an id
column only -- no model, no zcat --: torch.equal against the numpy restatement (tests/user_line_cases.py) and against the
parent's route, harness._history_exclusions + ItemCatalog.exclusions, at the stride's and the range's seams; the capacity
report; repeatability."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import user_line_cases as uc

pytestmark = pytest.mark.gpu

CANARY = -12345


def test_the_cases_hit_every_size_the_plan_has_a_seam_at():
    """the plan function is host only: the range a workgroup covers and its stride through a history are what the cases'
    catalogue sizes and segment lengths were chosen around"""
    from score_amd import _lib
    R, TH = uc.EXCL_RANGE, uc.EXCL_THREADS
    for L in (1, 2, 3, 11):
        for N, nr in zip(uc.EXCL_SMALL_N + uc.excl_seam_ns(), (1,) * 6 + (1, 1, 2, 3)):
            rng, n_ranges, threads, nbytes = _lib.history_exclusions_plan(L, N, max(uc.EXCL_SEGMENTS))
            assert (rng, n_ranges, threads) == (R, nr, TH) and nbytes > 0
    assert uc.excl_seam_ns() == (R - 1, R, R + 1, 2 * R + 1)
    assert {0, 1, TH - 1, TH, TH + 1} <= set(uc.EXCL_SEGMENTS) and max(uc.EXCL_SEGMENTS) > 2 * TH
    assert sorted({len(u) for u, _ in uc.excl_calls(uc.excl_world(65))}) == [1, 2, 3, 11]       # 2: one more than a workgroup's line


@functools.lru_cache(maxsize=None)
def _device_world(N):
    """the world's CSR and id column on the device, and a store struct that holds nothing but them"""
    from score_amd import _lib
    w = uc.excl_world(N)
    dev = torch.device("cuda:0")
    off = torch.as_tensor(np.array(w["off"]), device=dev)
    seq = torch.as_tensor(np.array(w["seq"]), device=dev)
    cat = torch.as_tensor(np.array(w["cat_ids"]), device=dev)
    st = _lib.PointLogStore(struct_bytes=C.sizeof(_lib.PointLogStore), user_hist_off=off.data_ptr(), user_hist_seq=seq.data_ptr(),
                            n_users=w["U"])
    return dict(w=w, off=off, seq=seq, cat=cat, struct=st, dev=dev)


def _run(d, users, keep, capacity=None, slack=3):
    """-> (excl_off, excl_idx buffer of capacity + slack words -- the slack holds a canary --, status)"""
    from score_amd import _lib
    lib = _lib.load()
    dev, N = d["dev"], int(d["cat"].numel())
    L = len(users)
    uid = torch.as_tensor(users, dtype=torch.int32, device=dev)
    kp = torch.as_tensor(keep, dtype=torch.int32, device=dev) if keep is not None else None
    if capacity is None:
        capacity = max(1, L * min(max(uc.EXCL_SEGMENTS), N))
    nbytes = _lib.history_exclusions_plan(L, N, max(uc.EXCL_SEGMENTS))[3]
    temp = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    off = torch.full((L + 2,), CANARY, dtype=torch.int64, device=dev)
    idx = torch.full((capacity + slack,), CANARY, dtype=torch.int32, device=dev)
    status = torch.zeros((2,), dtype=torch.int32, device=dev)
    status[1] = CANARY
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    rc = lib.score_catalog_history_exclusions(C.byref(d["struct"]), p(uid), p(kp), L, p(d["cat"]), N, p(off), p(idx), capacity,
                                              p(status), p(temp), nbytes, _lib.current_stream(dev))
    _lib.check(rc, "score_catalog_history_exclusions")
    assert int(off[L + 1]) == CANARY and int(status[1]) == CANARY
    return off[:L + 1], idx, status[:1], capacity


def _parent_route(d, users, keep):
    from score_amd import harness as h
    from score_amd import model as M
    cat = object.__new__(M.ItemCatalog)
    cat.ids, cat.N = d["cat"], int(d["cat"].numel())

    class Hist(object):
        user_hist_off, user_hist_seq = d["off"], d["seq"]
    uid = torch.as_tensor(users, dtype=torch.int32, device=d["dev"])
    kp = torch.as_tensor(keep if keep is not None else np.full(len(users), -1), dtype=torch.int32, device=d["dev"])
    return cat.exclusions(h._history_exclusions(Hist, uid, kp), len(users))


@pytest.mark.parametrize("N", uc.EXCL_SMALL_N + uc.excl_seam_ns(), ids=lambda n: "N%d" % n)
def test_lists_equal_the_restatement_and_the_parents_route(N):
    d = _device_world(N)
    w = d["w"]
    for users, keep in uc.excl_calls(w):
        L = len(users)
        want_off, want_idx = uc.restate_exclusions(w["off"], w["seq"], users, keep, w["cat_ids"])
        off, idx, status, cap = _run(d, users, keep)
        total = int(want_off[-1])
        assert off.dtype == torch.int64 and idx.dtype == torch.int32
        assert torch.equal(off.cpu(), torch.as_tensor(want_off)), (N, users.tolist())
        assert torch.equal(idx[:total].cpu(), torch.as_tensor(want_idx)), (N, users.tolist())
        assert bool((idx[total:] == CANARY).all()) and int(status[0]) == 0          # nothing behind the lists, nothing reported
        poff, pidx = _parent_route(d, users, keep)
        assert torch.equal(off, poff) and torch.equal(idx[:total], pidx[:total])
        # twice for the same bits
        off2, idx2, _, _ = _run(d, users, keep)
        assert torch.equal(off2, off) and torch.equal(idx2, idx)
        # unknown users have empty lists, wherever they stand
        n = np.diff(want_off)
        assert all(n[l] == 0 for l, u in enumerate(users.tolist()) if not 1 <= u <= w["U"])


@pytest.mark.parametrize("N", (33, uc.EXCL_RANGE + 1), ids=lambda n: "N%d" % n)
def test_a_capacity_one_short_is_reported_and_nothing_is_written_past_it(N):
    d = _device_world(N)
    w = d["w"]
    users, keep = uc.excl_calls(w)[3]
    want_off, want_idx = uc.restate_exclusions(w["off"], w["seq"], users, keep, w["cat_ids"])
    total = int(want_off[-1])
    assert total > 2
    off, idx, status, cap = _run(d, users, keep, capacity=total - 1)
    assert int(status[0]) & 1 == 1
    assert torch.equal(off.cpu(), torch.as_tensor(want_off))                         # the offsets stay exact
    assert torch.equal(idx[:total - 1].cpu(), torch.as_tensor(want_idx[:total - 1]))
    assert bool((idx[total - 1:] == CANARY).all())
    # an exact fit reports nothing
    off, idx, status, cap = _run(d, users, keep, capacity=total)
    assert int(status[0]) == 0 and torch.equal(idx[:total].cpu(), torch.as_tensor(want_idx)) and bool((idx[total:] == CANARY).all())
