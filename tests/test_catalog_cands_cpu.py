"""Top-K within per-line candidate lists (score_catalog_cands_plan / score_catalog_topk_in; recommend_async(candidates=...))
without a GPU: the symbols and their declarations, the ctypes layout against the header's, the plan against
score_catalog_plan, every host-side refusal, the Python-side refusals, ItemCatalog.candidates' mapping, the cases' lists, and
the restated selection within a list (tests/catalog_cand_cases.py) against a brute-force one."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import catalog_cand_cases as kc
import catalog_cases as cc
from score_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_BADARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
NAMES = ("score_catalog_cands_plan", "score_catalog_topk_in", "score_catalog_cands_struct_sizes")


@pytest.fixture(autouse=True)
def _the_entry_points_are_there():
    """every test here stands on them, the cases' and the restatement's too: without them there is nothing to pin"""
    assert all(name in _lib.EXPORTS for name in NAMES) and hasattr(_lib, "CatalogCands")


def _cfg(mt="GRU4Rec", H=32, T=50):
    return _lib.make_config(3000, 16, H, T, 1 if _lib.MODEL_TYPES[mt] >= 7 else 5, 3, 4, mt)


def _plan(cfg, L, max_count, k):
    chunk, nchunk, n = C.c_int32(-7), C.c_int32(-7), C.c_int64(-7)
    rc_ = _lib.load().score_catalog_cands_plan(C.byref(cfg), L, max_count, k, C.byref(chunk), C.byref(nchunk), C.byref(n))
    return rc_, chunk.value, nchunk.value, n.value


def test_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "score_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert getattr(lib, name).restype is C.c_int
    assert "score_catalog_cands_t" in src
    text = open(os.path.join(ROOT, "include", "score_hip.h")).read()
    assert re.search(r"STRICTLY\s+ASCENDING", text) and "twice" in text          # the list contract is stated


def test_ctypes_layout_matches_the_header():
    lib = _lib.load()
    out = (C.c_int64 * 8)()
    assert lib.score_catalog_cands_struct_sizes(out, 8) == 4
    assert list(out)[:4] == [C.sizeof(_lib.CatalogCands), _lib.CatalogCands.cand_off.offset, _lib.CatalogCands.cand_idx.offset,
                             _lib.CatalogCands.max_count.offset]
    assert lib.score_catalog_cands_struct_sizes(out, 3) == E_BADARG and lib.score_catalog_cands_struct_sizes(None, 8) == E_BADARG
    assert [f[0] for f in _lib.CatalogCands._fields_] == ["cand_off", "cand_idx", "max_count"]
    # the structures of the whole-catalogue call are as they were
    assert lib.score_catalog_struct_sizes(out, 8) == 6
    assert list(out)[:2] == [C.sizeof(_lib.Catalog), C.sizeof(_lib.CatalogLines)]


@pytest.mark.parametrize("mt", ["GRU4Rec", "Caser"])
def test_the_plan_is_score_catalog_plan_with_max_count_for_n(mt):
    cfg = _cfg(mt)
    for L in (1, 3, 10, 100, 1000):
        for M in (1, 31, 32, 33, 100, 255, 256, 257, 1000, 10000, 40000):
            for k in (1, 10, 128):
                got = _plan(cfg, L, M, k)
                assert got[0] == 0 and got[1:] == _lib.catalog_plan(cfg, L, M, k)
                assert _lib.catalog_cands_plan(cfg, L, M, k) == got[1:]
    assert _plan(cfg, 3, 100, 10)[1:3] == (256, 1) and _plan(cfg, 1, 513, 128)[1:3] == (256, 3)      # what the GPU cases stand on


def test_plan_refusals():
    lib = _lib.load()
    for mt in _lib.MODEL_TYPES:
        got = _plan(_cfg(mt), 10, 1000, 10)
        if mt in ("GRU4Rec", "Caser"):
            assert got[0] == 0
        else:
            assert got == (E_SHAPE, -7, -7, -7), mt
    cfg = _cfg()
    for L, M, k in ((0, 100, 10), (-1, 100, 10), (10, 0, 10), (10, -5, 10), (10, 100, 0), (10, 100, 129), (10, 100, -1)):
        assert _plan(cfg, L, M, k) == (E_BADARG, -7, -7, -7), (L, M, k)
    i32, i64 = C.byref(C.c_int32(0)), C.byref(C.c_int64(0))
    assert lib.score_catalog_cands_plan(None, 10, 100, 10, i32, i32, i64) == E_BADARG
    assert lib.score_catalog_cands_plan(C.byref(cfg), 10, 100, 10, None, i32, i64) == E_BADARG
    assert lib.score_catalog_cands_plan(C.byref(cfg), 10, 100, 10, i32, None, i64) == E_BADARG
    assert lib.score_catalog_cands_plan(C.byref(cfg), 10, 100, 10, i32, i32, None) == E_BADARG
    with pytest.raises(_lib.ScoreHipError, match="unsupported shape"):
        _lib.catalog_cands_plan(_cfg("SASRec"), 10, 100, 10)


def test_topk_in_refuses_on_the_host_before_any_launch():
    """no device here: every one of these returns before it would touch one"""
    lib = _lib.load()
    cfg = _cfg()
    p = C.c_void_p(64)                                   # (never dereferenced: the refusals come first)
    st = _lib.State(table=p, w=p, workspace=p, workspace_bytes=0)
    cat = _lib.Catalog(p, 1000, p)
    ln = _lib.CatalogLines(p, p, p, 3, 0, None, None)
    cd = _lib.CatalogCands(p, p, 100)

    def topk(c=cfg, s=st, t=cat, l=ln, d=cd, k=10, idx=p, logit=p, own=None):
        ref = lambda x: C.byref(x) if x else None
        return lib.score_catalog_topk_in(ref(c), ref(s), ref(t), ref(l), ref(d), k, idx, logit, own, None)
    for name in ("c", "s", "t", "l", "d", "idx", "logit"):
        assert topk(**{name: None}) == E_BADARG, name
    assert topk(k=0) == E_BADARG and topk(k=129) == E_BADARG and topk(k=-1) == E_BADARG
    assert topk(d=_lib.CatalogCands(p, p, 0)) == E_BADARG and topk(d=_lib.CatalogCands(p, p, -4)) == E_BADARG
    assert topk(d=_lib.CatalogCands(None, p, 100)) == E_BADARG and topk(d=_lib.CatalogCands(p, None, 100)) == E_BADARG
    assert topk(l=_lib.CatalogLines(p, p, p, 0, 0, None, None)) == E_BADARG
    assert topk(t=_lib.Catalog(p, 0, p)) == E_BADARG
    assert topk(t=_lib.Catalog(None, 1000, p)) == E_BADARG and topk(t=_lib.Catalog(p, 1000, None)) == E_BADARG
    for bad in (_lib.CatalogLines(None, p, p, 3, 0, None, None), _lib.CatalogLines(p, None, p, 3, 0, None, None),
                _lib.CatalogLines(p, p, None, 3, 0, None, None), _lib.CatalogLines(p, p, p, 3, 0, p, None)):
        assert topk(l=bad) == E_BADARG
    assert topk(s=_lib.State(table=p, w=p, workspace=None)) == E_BADARG
    for mt in _lib.MODEL_TYPES:
        if mt not in ("GRU4Rec", "Caser"):
            assert topk(c=_cfg(mt)) == E_SHAPE, mt
    # the workspace is the candidate plan's, not the whole catalogue's: one byte short of it is refused, still before any launch
    need = _lib.catalog_cands_plan(cfg, 3, 100, 10)[2]
    assert topk(s=_lib.State(table=p, w=p, workspace=p, workspace_bytes=need - 1)) == E_WORKSPACE
    assert topk(own=p) == E_WORKSPACE                                      # (workspace_bytes = 0)
    big = _lib.CatalogCands(p, p, 100000)
    assert _lib.catalog_cands_plan(cfg, 3, 100000, 10)[2] > need
    assert topk(d=big, s=_lib.State(table=p, w=p, workspace=p, workspace_bytes=need)) == E_WORKSPACE


def _host_catalog(ids):
    """an ItemCatalog's id map without a model or a device"""
    from score_amd import model as M
    cat = object.__new__(M.ItemCatalog)
    cat.ids = torch.as_tensor(np.asarray(ids), dtype=torch.int32)
    cat.N = int(cat.ids.numel())
    return cat


def test_python_side_refusals():
    from score_amd import harness as h
    from score_amd import model as M
    why = {"DELF": "conditioned on the target item", "DEEMS": "item history", "SVDpp": "follow-up", "SASRec": "follow-up",
           "SCORE": "neighbour sets", "GCMC": "neighbour sets"}
    for name, word in why.items():
        m = object.__new__(M.MODELS[name])           # (no device: the refusal comes before anything is touched)
        for call in (lambda: m.recommend_async(None, None, candidates=[[1]]), lambda: m.recommend(None, None, candidates=[[1]]),
                     lambda: m.recommend_async(None, None, candidates=[[1]], max_candidates=4)):
            with pytest.raises(NotImplementedError, match=word):
                call()
    cat = _host_catalog([3, 5, 9, 12])
    with pytest.raises(ValueError, match=r"candidates must hold one array of item ids per line \(3\)"):
        cat.candidates([[3], [5]], 3)
    with pytest.raises(ValueError, match=r"exclude must hold one array of item ids per line \(3\)"):      # (as before)
        cat.exclusions([[3], [5]], 3)
    with pytest.raises(ValueError, match="candidates must be None or"):
        h.evaluate_catalog(None, [], None, candidates="x")
    with pytest.raises(ValueError, match="candidates must be None or"):
        h.evaluate_catalog(None, [], None, candidates=["line"])
    import inspect
    for fn, tail in ((M.GRU4Rec.recommend_async, ["candidates", "max_candidates"]), (M.GRU4Rec.recommend, ["candidates"]),
                     (h.evaluate_catalog, ["candidates"])):
        names = list(inspect.signature(fn).parameters)
        assert names[-len(tail):] == tail, names                              # the new keywords stand at the end
        assert all(inspect.signature(fn).parameters[n].default is None for n in tail)


def test_candidates_maps_ids_as_exclusions_does():
    """unsorted, repeated and unknown ids; a list per line and the CSR pair; the longest line's count, never below 1"""
    cat = _host_catalog([3, 5, 9, 12, 40])
    per_line = [[12, 3, 3, 7, 40], [], [9, 9], [100, 1]]
    off, idx, longest = cat.candidates(per_line, 4)
    assert off.dtype == torch.int64 and idx.dtype == torch.int32
    assert off.tolist() == [0, 3, 3, 4, 4] and idx.tolist() == [0, 3, 4, 2] and longest == 3
    xo, xi = cat.exclusions(per_line, 4)
    assert torch.equal(xo, off) and torch.equal(xi, idx)
    flat = np.concatenate([np.asarray(x, dtype=np.int64) for x in per_line])
    csr = (np.concatenate([[0], np.cumsum([len(x) for x in per_line])]).astype(np.int64), flat)
    off2, idx2, longest2 = cat.candidates(csr, 4)
    assert torch.equal(off2, off) and torch.equal(idx2, idx) and longest2 == 3
    off3, idx3, longest3 = cat.candidates([[], [77]], 2)
    assert off3.tolist() == [0, 0, 0] and idx3.numel() == 1 and longest3 == 1       # nothing left: a non-null list, a plan of 1
    off4, idx4, longest4 = cat.candidates([[], []], 2)
    assert off4.tolist() == [0, 0, 0] and idx4.numel() == 1 and longest4 == 1


def test_the_cases_lists():
    ch = 256
    N = kc.n_items(ch)
    want = [[1], [15, 16, 17], [31, 32, 33], [0, 1, ch + 1], [ch - 1], [ch], [ch + 1, 2 * ch + 1, 5], [2 * ch + 1], [40, 40], [N]]
    ks = [1, 10, 10, 10, 128, 128, 10, 128, 128, 10]
    assert len(kc.CASES) == len(want) == len(kc.IDS) == len(set(kc.IDS))
    has_first = has_last = False
    for i, (s, counts, k, _) in enumerate(kc.CASES):
        assert counts(ch) == want[i] and k == ks[i] and 0 <= s < len(cc.SHAPES) and len(want[i]) <= kc.LMAX
        lists = kc.lists_of(i, ch)
        assert [len(v) for v in lists] == want[i]
        for v in lists:
            assert v.dtype == np.int32 and (np.diff(v) > 0).all() and (v.size == 0 or (v[0] >= 0 and v[-1] < N))
        if i != kc.EVERY_ITEM_CASE:
            has_first |= any(v.size and v[0] == 0 for v in lists)
            has_last |= any(v.size and v[-1] == N - 1 for v in lists)
    assert has_first and has_last
    assert {s for s, *_ in kc.CASES} == set(range(len(cc.SHAPES)))
    run = kc.lists_of(kc.RUN_CASE, ch)[0]
    assert run.tolist() == list(range(5, 5 + ch)) and (run[0] - 0) % 32 != 0
    assert kc.lists_of(kc.EVERY_ITEM_CASE, ch)[0].tolist() == list(range(N))
    assert kc.CASES[kc.RAGGED_CASE][1](ch) == [ch + 1, 2 * ch + 1, 5]


def test_the_restated_selection_within_a_list_equals_a_brute_force_one():
    rng = np.random.default_rng(6)
    for trial in range(40):
        N = int(rng.integers(1, 80))
        v = rng.standard_normal(N).round(1)                                  # (rounded: many ties)
        if trial % 3 == 0:
            v[rng.integers(0, N, size=2)] = np.nan
        if trial % 4 == 0:
            v[rng.integers(0, N)] = -np.inf
        cand = np.sort(rng.choice(N, size=int(rng.integers(0, N + 1)), replace=False))
        excl = np.unique(rng.integers(0, N, size=int(rng.integers(0, N + 1)))) if trial % 2 else np.zeros((0,), dtype=np.int64)
        for k in (1, 10, 128):
            idx, val = kc.select_in(v, cand, k, excl)
            gone = [p for p, n in enumerate(cand) if n in set(excl.tolist())]
            bpos, bval = cc.select_brute(v[cand], k, gone)
            bidx = [int(cand[p]) if p >= 0 else -1 for p in bpos]
            assert idx.tolist() == bidx, (trial, k)
            assert np.array_equal(val, np.asarray(bval), equal_nan=True)
            got = idx[idx >= 0]
            assert np.isin(got, cand).all() and not np.isin(got, excl).any()
            assert got.size == min(k, np.setdiff1d(cand, excl).size)
            # and it is the whole-catalogue selection with everything outside the list excluded
            widx, wval = cc.select(v, k, np.union1d(np.setdiff1d(np.arange(N), cand), excl))
            assert widx.tolist() == idx.tolist() and np.array_equal(wval, val, equal_nan=True)
    idx, val = kc.select_in(np.asarray([1.0, 2.0, 2.0, np.nan, -np.inf, 2.0, 9.0]), [1, 2, 3, 4, 5], 6)
    assert idx.tolist() == [1, 2, 5, 4, 3, -1] and np.isneginf(val[-1])      # ties by index, -inf in front of NaN, padding
