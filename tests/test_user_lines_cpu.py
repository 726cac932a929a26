"""Recommend by user id, without a GPU: PointLogStore.host_user_lines against the reference-pinned chain (history files ->
DataLoaderUserSeq), the numpy restatement of the exclusion contract against a brute-force loop and against
harness._history_exclusions + ItemCatalog._line_indices on CPU tensors, the cases' properties, and every refusal of the two C
entries and of the Python calls that comes before a launch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import user_line_cases as uc
from helpers import GOLDEN
from score_amd import dataprep as dp
from score_amd.pointdata import DataLoaderUserSeq, PointLogStore

E_BADARG, E_SHAPE, E_WORKSPACE = -1, -2, -3


def _against_the_host_loader(st, lines, log4, window, H, neg, B, tmp):
    """store.host_user_lines(line_user, T) == the first sample of every line of DataLoaderUserSeq's batches over the files the
    reference's chain writes from the same log and lines; T below and above the longest kept history"""
    users, items = dp.point_history_lines(*log4, lines, window[0], window[1], H)
    tf, uf, _, ud, idd = dp.write_point_files(str(tmp), lines, users, items, st.user_rows, st.item_rows)
    longest = st.max_user_len
    assert longest == int(st.arrays()["user_hist_len"].max()) > 2
    for T in (longest - 2, longest + 3):
        batches = list(DataLoaderUserSeq(B, T, tf, uf, neg, ud, idd))
        assert len(batches) == st.n_batches > 0
        want = uc.first_samples(batches, 1 + neg)
        got = st.host_user_lines(st.line_user, T)
        assert got[0].shape == (st.n_lines, T, st.Fi) and all(g.dtype == np.int32 for g in got)
        for g, w, name in zip(got[:3], want, ("user_seq", "length", "target_user")):
            assert np.array_equal(g, w), (T, name)
        assert got[3].tolist() == [1] * st.n_lines
        assert (got[1] > T).any() or T > longest                        # the reported length is the untruncated kept one


def test_host_user_lines_on_the_tmall_sample(tmp_path):
    log = np.load(os.path.join(GOLDEN, "tmall_sample_log.npz"))["log"]
    stores, r = dp.tmall_point_stores(log, build="host", dual=False, batch_size={"train": 20, "validation": 200, "test": 100})
    _, _, targets = dp.tmall_pipeline(log)
    st = stores["test"]
    assert not st.dual and st.max_user_events >= st.max_user_len
    _against_the_host_loader(st, targets["test"][:st.n_lines], (r["uid"], r["iid"], log[:, 5], r["t_idx"]),
                             (0, dp.TMALL["pred_time_test"]), dp.POINT_HIST_MAX_LEN, 99, 100, tmp_path)


def test_host_user_lines_on_a_history_build_case(tmp_path):
    """tests/point_hist_cases.py's tile_exact as a store's log: users cut at H, a user without events, ties"""
    uid, iid, tk, ti, U, window, H = uc.hist_case_log("tile_exact", I=50)
    ur, ir = uc.rows_of(U, 50, 2, 3, 500, seed=2)
    neg = 2
    lines = uc.target_lines(uid, ti, window, U, 50, 1 + neg, 60, seed=4)
    st = PointLogStore(uid, iid, tk, ti, lines, window[0], window[1], H, neg, 30, ur, ir, False, build="host")
    a = st.arrays()
    assert st.max_user_len == H and st.max_user_events == int(np.diff(a["user_hist_off"]).max()) > H
    _against_the_host_loader(st, lines, (uid, iid, tk, ti), window, H, neg, 30, tmp_path)
    # users no line names: one without events (cold: zeros, length 0, known), ids outside 1 .. U (zeros, length 0, unknown),
    # and the same user twice
    cold = int(np.flatnonzero(np.diff(a["user_hist_off"]) == 0)[0]) + 1
    busy = int(st.line_user[0])
    seq, ln, tu, known = st.host_user_lines(np.asarray([busy, cold, 0, U + 1, -3, busy, 1, U]), 9)
    assert known.tolist() == [1, 1, 0, 0, 0, 1, 1, 1] and ln[1:5].tolist() == [0, 0, 0, 0]
    assert not seq[1:5].any() and not tu[2:5].any() and tu[1].tolist() == ur[cold - 1].tolist()
    assert np.array_equal(seq[0], seq[5]) and ln[0] == ln[5] and seq[0].any()
    assert tu[6, 0] == 1 and tu[7, 0] == U
    with pytest.raises(ValueError, match="max_len"):
        st.host_user_lines([1], 8192 // 3 + 1)
    with pytest.raises(RuntimeError, match="not on a device"):
        st.user_lines([1], 9)


# ---- the exclusion contract ----------------------------------------------------------------------------------------------------
def _host_catalog(ids):
    from score_amd import model as M
    cat = object.__new__(M.ItemCatalog)
    cat.ids = torch.as_tensor(np.array(ids), dtype=torch.int32)
    cat.N = int(cat.ids.numel())
    return cat


class _Hist(object):
    def __init__(self, w):
        self.user_hist_off, self.user_hist_seq = w["off"].copy(), w["seq"].copy()


@pytest.mark.parametrize("N", uc.EXCL_SMALL_N + (uc.EXCL_RANGE + 1,))
def test_the_restated_exclusions(N):
    """against the double loop (small catalogues) and against the parent's route on CPU tensors"""
    from score_amd import harness as h
    w = uc.excl_world(N)
    cat = _host_catalog(w["cat_ids"])
    for users, keep in uc.excl_calls(w):
        off, idx = uc.restate_exclusions(w["off"], w["seq"], users, keep, w["cat_ids"])
        assert off.dtype == np.int64 and idx.dtype == np.int32 and off[-1] == len(idx)
        for l in range(len(users)):
            mine = idx[off[l]:off[l + 1]]
            assert (np.diff(mine) > 0).all() and (not len(mine) or (mine[0] >= 0 and mine[-1] < N))
        if N <= 65:
            boff, bidx = uc.brute_exclusions(w["off"], w["seq"], users, keep, w["cat_ids"])
            assert np.array_equal(off, boff) and np.array_equal(idx, bidx)
        keep_t = torch.as_tensor(keep if keep is not None else np.full(len(users), -1, dtype=np.int32))
        poff, pidx = cat._line_indices(h._history_exclusions(_Hist(w), torch.as_tensor(users), keep_t), len(users), "exclude")
        assert poff.tolist() == off.tolist() and pidx[:len(idx)].tolist() == idx.tolist()


def test_the_exclusion_cases_are_worth_running():
    from score_amd import _lib
    R, TH = uc.EXCL_RANGE, uc.EXCL_THREADS
    for N, nr in zip(uc.EXCL_SMALL_N + uc.excl_seam_ns(), (1,) * 6 + (1, 1, 2, 3)):
        assert _lib.history_exclusions_plan(3, N)[:3] == (R, nr, TH), N
    assert uc.excl_seam_ns(R) == (R - 1, R, R + 1, 2 * R + 1)
    assert {0, 1, TH - 1, TH, TH + 1} <= set(uc.EXCL_SEGMENTS) and max(uc.EXCL_SEGMENTS) > 2 * TH
    for N in (65,) + uc.excl_seam_ns():
        w = uc.excl_world(N)
        cat, off, seq = w["cat_ids"], w["off"], w["seq"]
        assert (np.diff(cat) > 0).all() and np.diff(off).tolist() == list(uc.EXCL_SEGMENTS)
        seg = lambda u: seq[off[u - 1]:off[u]]
        pos = lambda u: np.unique(np.searchsorted(cat, seg(u)[np.isin(seg(u), cat)]))
        assert len(np.unique(seg(6))) == 1 and pos(6).tolist() == [N // 2]          # one item through a whole segment
        assert not np.isin(seg(7), cat).any()                                      # a segment with no item of the catalogue
        for u in (5, 8):                                                           # first and last index, both sides of a seam
            p = pos(u)
            assert p[0] == 0 and p[-1] == N - 1
            for s in range(R, N, R):
                assert s - 1 in p and s in p, (N, u, s)
            assert len(seg(u)) > len(np.unique(seg(u)))                            # repeats
            assert (seg(u) < cat[0]).any() and (seg(u) > cat[-1]).any() and (seg(u) % 2 == 1).any()
        keep = w["keep"]
        assert int((seg(8) == keep[7]).sum()) >= 37 and keep[7] in cat              # the keep id many times
        once = uc.keep_present_once(w)
        assert int((seg(8) == once).sum()) == 1 and once in cat                     # ... once
        assert w["absent8"] not in seg(8) and (N == 65 or w["absent8"] in cat)      # ... absent
        assert keep[5] == seg(6)[0]
        calls = uc.excl_calls(w)
        assert sorted({len(u) for u, _ in calls}) == [1, 2, 3, 11] and any(k is None for _, k in calls)
        every = calls[3][0].tolist()
        assert every[3] == 0 and every[6] == w["U"] + 1 and every[9] == -3 and every[2] >= 1 and every[4] >= 1


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_abi_refusals_come_before_any_launch():
    """(host only: nothing is launched; p is a pointer nobody follows)"""
    from score_amd import _lib
    lib = _lib.load()
    for name in ("score_point_user_lines", "score_catalog_history_exclusions", "score_catalog_history_exclusions_plan"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    p = C.c_void_p(4096)
    size = C.sizeof(_lib.PointLogStore)

    def store(struct_bytes=size, **kw):
        f = dict(user_hist_off=p, user_hist_seq=p, user_hist_len=p, user_rows=p, item_rows=p, n_users=5, n_items=7)
        f.update(kw)
        return _lib.PointLogStore(struct_bytes=struct_bytes, **f)      # (the item side and the line arrays stay NULL)

    def lines(st=None, ids=p, L=2, T=4, Fu=2, Fi=3, outs=(p, p, p, p)):
        st = store() if st is None else st
        return lib.score_point_user_lines(C.byref(st) if st is not False else None, ids, L, T, Fu, Fi, *outs, None)
    assert lines(st=False) == E_BADARG and lines(ids=None) == E_BADARG
    for i in range(4):
        assert lines(outs=tuple(None if j == i else p for j in range(4))) == E_BADARG, i
    assert lines(st=store(struct_bytes=size + 8)) == E_BADARG and lines(st=store(struct_bytes=0)) == E_BADARG
    for missing in ("user_hist_off", "user_hist_seq", "user_hist_len", "user_rows", "item_rows"):
        assert lines(st=store(**{missing: None})) == E_BADARG, missing
    assert lines(st=store(n_users=0)) == E_BADARG
    for kw in (dict(L=0), dict(L=-1), dict(T=0), dict(Fu=0), dict(Fi=0)):
        assert lines(**kw) == E_BADARG, kw
    assert lines(T=2049, Fi=4) == E_SHAPE and lines(T=8193, Fi=1) == E_SHAPE
    assert lines(L=2 ** 20, T=2048, Fi=1) == E_SHAPE                             # L * T * Fi = 2^31

    plan = lib.score_catalog_history_exclusions_plan
    n64 = C.c_int64(0)
    assert plan(0, 5, 0, None, None, None, C.byref(n64)) == E_BADARG and plan(3, 0, 0, None, None, None, C.byref(n64)) == E_BADARG
    assert plan(3, 5, -1, None, None, None, None) == E_BADARG and plan(3, 5, 0, None, None, None, None) == 0
    assert plan(2 ** 20, 2 ** 31 - 1, 0, None, None, None, None) == E_SHAPE
    need = _lib.history_exclusions_plan(3, 100)[3]
    assert need > 0 and _lib.history_exclusions_plan(3, 3 * uc.EXCL_RANGE)[3] >= need

    def excl(st=None, ids=p, keep=None, L=3, cat=p, N=100, off=p, idx=p, cap=10, status=p, temp=p, nbytes=need):
        st = store(user_hist_len=None, user_rows=None, item_rows=None) if st is None else st     # (only off / seq / n_users are read)
        return lib.score_catalog_history_exclusions(C.byref(st) if st is not False else None, ids, keep, L, cat, N, off, idx, cap,
                                                    status, temp, nbytes, None)
    for kw in (dict(st=False), dict(ids=None), dict(cat=None), dict(off=None), dict(idx=None), dict(status=None), dict(temp=None)):
        assert excl(**kw) == E_BADARG, kw
    assert excl(st=store(struct_bytes=size - 8)) == E_BADARG
    assert excl(st=store(user_hist_off=None)) == E_BADARG and excl(st=store(user_hist_seq=None)) == E_BADARG
    for kw in (dict(L=0), dict(L=-2), dict(N=0), dict(N=-1), dict(cap=-1)):
        assert excl(**kw) == E_BADARG, kw
    assert excl(nbytes=need - 1) == E_WORKSPACE and excl(nbytes=0) == E_WORKSPACE


def test_python_side_refusals():
    import inspect
    from score_amd import harness as h
    from score_amd import model as M
    why = {"DELF": "conditioned on the target item", "DEEMS": "item history", "SVDpp": "follow-up", "SASRec": "follow-up",
           "SCORE": "neighbour sets"}
    for name, word in why.items():
        m = object.__new__(M.MODELS[name])           # (no device: the refusal comes before anything is touched)
        for call in (lambda: m.recommend_users_async([1], None, None), lambda: m.recommend_users([1], None, None),
                     lambda: h.evaluate_catalog_users(m, None, None)):
            with pytest.raises(NotImplementedError, match=word):
                call()
    m = object.__new__(M.GRU4Rec)
    with pytest.raises(ValueError, match="mutually exclusive"):
        m.recommend_async(None, None, exclude=[[1]], exclude_idx=(None, None))
    with pytest.raises(ValueError, match="candidates must be None or"):
        h.evaluate_catalog_users(m, None, None, candidates="x")
    assert inspect.signature(M.GRU4Rec.recommend_async).parameters["exclude_idx"].default is None
    sig = inspect.signature(M.Caser.recommend_users_async).parameters            # (Caser inherits all of it)
    assert list(sig)[1:] == ["user_ids", "store", "catalog", "k", "exclude_history", "keep", "candidates", "max_candidates",
                             "all_logits"]
    assert sig["k"].default == 10 and sig["exclude_history"].default is True and sig["all_logits"].default is False
    sig = inspect.signature(h.evaluate_catalog_users).parameters
    assert list(sig) == ["model", "store", "catalog", "k", "exclude_history", "candidates", "lines_per_call", "return_lists"]
    assert sig["lines_per_call"].default == 100
