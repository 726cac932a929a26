"""The exact rank of given items in a catalogue (score_catalog_ranks_plan / score_catalog_ranks / score_catalog_ranks_in;
GRU4Rec.item_ranks_async, harness.rank_quality_device) without a GPU: the restated count (tests/catalog_ranks_cases.py) against a
brute-force count and against the position in catalog_cases.select's unbounded list, the symbols, the ctypes layout, the plan
against score_catalog_plan, every host-side refusal, the Python-side refusals, ItemCatalog.targets' mapping,
rank_quality_device against the reference's metric functions on explicit ranklists, and the GPU cases' seeds: the restatement's
sandwich is tight."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import catalog_cases as cc
import catalog_ranks_cases as kr
from score_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_BADARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
NAMES = ("score_catalog_ranks_plan", "score_catalog_ranks", "score_catalog_ranks_in", "score_catalog_ranks_struct_sizes")


@pytest.fixture(autouse=True)
def _the_entry_points_are_there():
    assert all(name in _lib.EXPORTS for name in NAMES) and hasattr(_lib, "CatalogTargets")


def _cfg(mt="GRU4Rec", H=32, T=50):
    return _lib.make_config(3000, 16, H, T, 1 if _lib.MODEL_TYPES[mt] >= 7 else 5, 3, 4, mt)


def _plan(cfg, L, span):
    chunk, nchunk, n = C.c_int32(-7), C.c_int32(-7), C.c_int64(-7)
    rc_ = _lib.load().score_catalog_ranks_plan(C.byref(cfg), L, span, C.byref(chunk), C.byref(nchunk), C.byref(n))
    return rc_, chunk.value, nchunk.value, n.value


# ---- the restated count
def _random_line(rng, trial):
    N = int(rng.integers(1, 90))
    v = rng.standard_normal(N).round(1).astype(np.float32)                  # (rounded: many ties)
    if trial % 3 == 0:
        v[rng.integers(0, N, size=2)] = np.nan
    if trial % 4 == 0:
        v[rng.integers(0, N)] = -np.inf
    if trial % 5 == 0:
        v[rng.integers(0, N, size=3)] = np.float32(-0.0)
        v[rng.integers(0, N, size=3)] = np.float32(0.0)
    excl = np.unique(rng.integers(0, N, size=int(rng.integers(0, N + 1)))) if trial % 2 else np.zeros((0,), dtype=np.int64)
    t = rng.integers(0, N, size=int(rng.integers(0, kr.TMAX - 3))).tolist()
    t = t + t[:1] + [-1, N]                                                  # a repeat, two outside
    if excl.size:
        t.append(int(excl[0]))                                               # a target that is excluded
    return N, v, excl, np.asarray(t[:kr.TMAX], dtype=np.int64)


def test_the_restated_count_equals_a_brute_force_count_and_the_position_in_the_unbounded_list():
    rng = np.random.default_rng(8)
    seen = set()
    for trial in range(60):
        N, v, excl, t = _random_line(rng, trial)
        ahead, state, n_scored = kr.count(v, t, excl)
        b_ahead, b_state, b_scored = kr.count_brute(v, t, excl)
        assert ahead.tolist() == b_ahead and state.tolist() == b_state and n_scored == b_scored == N - excl.size, trial
        for j, x in enumerate(t.tolist()):
            if not 0 <= x < N:
                assert ahead[j] == -1 and state[j] == -1
                continue
            # the 0-based place x has, or would have were it not excluded, in the unbounded list
            order, _ = cc.select(v, N, np.setdiff1d(excl, [x]))
            assert int(np.nonzero(order == x)[0][0]) == ahead[j], (trial, x)
            assert state[j] == (2 if x in excl else 1)
            seen.add(int(state[j]))
        # the candidate form: a list with an index outside the catalogue; a target that is not listed has state 0
        cand = np.sort(rng.choice(N, size=int(rng.integers(0, N + 1)), replace=False))
        listed = np.concatenate([[-1], cand, [N]])
        ahead, state, n_scored = kr.count(v, t, excl, listed)
        b_ahead, b_state, b_scored = kr.count_brute(v, t, excl, listed)
        assert ahead.tolist() == b_ahead and state.tolist() == b_state and n_scored == b_scored == np.setdiff1d(cand, excl).size
        for j, x in enumerate(t.tolist()):
            if 0 <= x < N:
                want = 0 if x not in cand else (2 if x in excl else 1)
                assert state[j] == want
                seen.add(want)
                # the whole-catalogue count with everything outside the list excluded as well
                others = np.union1d(np.setdiff1d(np.arange(N), cand), excl)
                assert kr.count(v, [x], others)[0][0] == ahead[j]
        full = kr.count(v, t, excl, np.arange(N))
        whole = kr.count(v, t, excl)
        assert full[0].tolist() == whole[0].tolist() and full[1].tolist() == whole[1].tolist() and full[2] == whole[2]
    assert seen == {0, 1, 2}


def test_the_key_order_on_special_values():
    v = np.asarray([1.0, 2.0, 2.0, np.nan, -np.inf, 2.0, 9.0, -0.0, 0.0, np.inf, np.nan], dtype=np.float32)
    ahead, state, n = kr.count(v, list(range(v.size)))
    #              1.0 2.0 2.0 nan -inf 2.0 9.0 -0.0 0.0 inf nan
    assert ahead.tolist() == [5, 2, 3, 9, 8, 4, 1, 6, 7, 0, 10] and n == v.size and (state == 1).all()
    k = kr.keys(v, np.arange(v.size))
    assert k.dtype == np.uint64 and np.unique(k).size == v.size and (k > 0).all()
    assert sorted(range(v.size), key=lambda n_: -int(k[n_])) == [int(x) for x in cc.select(v, v.size)[0]]
    everything = kr.count(v, [0, 3, -1], np.arange(v.size))
    assert everything[0].tolist() == [0, 0, -1] and everything[1].tolist() == [2, 2, -1] and everything[2] == 0


# ---- the C interface
def test_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "score_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert getattr(lib, name).restype is C.c_int
    assert "score_catalog_targets_t" in src
    assert re.search(r"#define\s+SCORE_CATALOG_TMAX\s+32\b", src) and _lib.CATALOG_TMAX == 32 == kr.TMAX
    for word in ("ahead", "tgt_logit", "n_scored", "state", "bit 1"):          # the contract is stated
        assert word in text


def test_ctypes_layout_matches_the_header():
    lib = _lib.load()
    out = (C.c_int64 * 8)()
    assert lib.score_catalog_ranks_struct_sizes(out, 8) == 5
    T = _lib.CatalogTargets
    assert list(out)[:5] == [C.sizeof(T), T.tgt_off.offset, T.tgt_idx.offset, T.max_targets.offset, _lib.CATALOG_TMAX]
    assert lib.score_catalog_ranks_struct_sizes(out, 4) == E_BADARG and lib.score_catalog_ranks_struct_sizes(None, 8) == E_BADARG
    assert [f[0] for f in T._fields_] == ["tgt_off", "tgt_idx", "max_targets"]
    assert lib.score_catalog_struct_sizes(out, 8) == 6 and lib.score_catalog_cands_struct_sizes(out, 8) == 4     # as they were


@pytest.mark.parametrize("mt", ["GRU4Rec", "Caser"])
def test_the_plan_cuts_as_score_catalog_plan_does(mt):
    cfg = _cfg(mt)
    for L in (1, 3, 10, 100, 257, 1000):
        for span in (1, 31, 32, 33, 255, 256, 257, 1000, 10000, 40000):
            got = _plan(cfg, L, span)
            assert got[0] == 0 and got[3] > 0
            for k in (1, 10, 128):
                assert got[1:3] == _lib.catalog_plan(cfg, L, span, k)[:2]
            assert _lib.catalog_ranks_plan(cfg, L, span) == got[1:]
    assert _plan(cfg, 3, 100)[1:3] == (256, 1) and _plan(cfg, 1, 513)[1:3] == (256, 3)        # what the GPU cases stand on
    assert _plan(cfg, 260, 640)[1:3] == (640, 1)                                              # a chunk above 512 items


def test_plan_refusals():
    lib = _lib.load()
    for mt in _lib.MODEL_TYPES:
        got = _plan(_cfg(mt), 10, 1000)
        assert (got[0] == 0) if mt in ("GRU4Rec", "Caser") else (got == (E_SHAPE, -7, -7, -7)), mt
    cfg = _cfg()
    for L, span in ((0, 100), (-1, 100), (10, 0), (10, -5)):
        assert _plan(cfg, L, span) == (E_BADARG, -7, -7, -7), (L, span)
    i32, i64 = C.byref(C.c_int32(0)), C.byref(C.c_int64(0))
    assert lib.score_catalog_ranks_plan(None, 10, 100, i32, i32, i64) == E_BADARG
    assert lib.score_catalog_ranks_plan(C.byref(cfg), 10, 100, None, i32, i64) == E_BADARG
    assert lib.score_catalog_ranks_plan(C.byref(cfg), 10, 100, i32, None, i64) == E_BADARG
    assert lib.score_catalog_ranks_plan(C.byref(cfg), 10, 100, i32, i32, None) == E_BADARG


@pytest.mark.parametrize("form", ["whole", "in"])
def test_the_calls_refuse_on_the_host_before_any_launch(form):
    """no device here: every one of these returns before it would touch one"""
    lib = _lib.load()
    cfg = _cfg()
    p = C.c_void_p(64)                                   # (never dereferenced: the refusals come first)
    st = _lib.State(table=p, w=p, workspace=p, workspace_bytes=0)
    cat = _lib.Catalog(p, 1000, p)
    ln = _lib.CatalogLines(p, p, p, 3, 0, None, None)
    cd = _lib.CatalogCands(p, p, 100)
    tg = _lib.CatalogTargets(p, p, 32)

    def ranks(c=cfg, s=st, t=cat, l=ln, d=cd, g=tg, ahead=p, logit=p, state=p, n_scored=p):
        ref = lambda x: C.byref(x) if x else None
        if form == "whole":
            return lib.score_catalog_ranks(ref(c), ref(s), ref(t), ref(l), ref(g), ahead, logit, state, n_scored, None)
        return lib.score_catalog_ranks_in(ref(c), ref(s), ref(t), ref(l), ref(d), ref(g), ahead, logit, state, n_scored, None)
    for name in ("c", "s", "t", "l", "g", "ahead", "logit", "state", "n_scored") + (("d",) if form == "in" else ()):
        assert ranks(**{name: None}) == E_BADARG, name
    for q in (0, 33, -1, 1 << 20):
        assert ranks(g=_lib.CatalogTargets(p, p, q)) == E_BADARG, q
    assert ranks(g=_lib.CatalogTargets(None, p, 4)) == E_BADARG and ranks(g=_lib.CatalogTargets(p, None, 4)) == E_BADARG
    assert ranks(l=_lib.CatalogLines(p, p, p, 0, 0, None, None)) == E_BADARG
    assert ranks(t=_lib.Catalog(p, 0, p)) == E_BADARG
    assert ranks(t=_lib.Catalog(None, 1000, p)) == E_BADARG and ranks(t=_lib.Catalog(p, 1000, None)) == E_BADARG
    for bad in (_lib.CatalogLines(None, p, p, 3, 0, None, None), _lib.CatalogLines(p, None, p, 3, 0, None, None),
                _lib.CatalogLines(p, p, None, 3, 0, None, None), _lib.CatalogLines(p, p, p, 3, 0, p, None)):
        assert ranks(l=bad) == E_BADARG
    assert ranks(s=_lib.State(table=p, w=p, workspace=None)) == E_BADARG
    if form == "in":
        assert ranks(d=_lib.CatalogCands(p, p, 0)) == E_BADARG
        assert ranks(d=_lib.CatalogCands(None, p, 100)) == E_BADARG and ranks(d=_lib.CatalogCands(p, None, 100)) == E_BADARG
    for mt in _lib.MODEL_TYPES:
        if mt not in ("GRU4Rec", "Caser"):
            assert ranks(c=_cfg(mt)) == E_SHAPE, mt
    # one byte short of the plan's workspace is refused, the plan's own size passes the check (and nothing else is in its way:
    # tried only one byte short, never at the full size -- that would launch)
    need = _lib.catalog_ranks_plan(cfg, 3, 1000 if form == "whole" else 100)[2]
    assert ranks(s=_lib.State(table=p, w=p, workspace=p, workspace_bytes=need - 1)) == E_WORKSPACE
    assert ranks() == E_WORKSPACE                                          # (workspace_bytes = 0)


# ---- Python
def _host_catalog(ids):
    """an ItemCatalog's id map without a model or a device"""
    from score_amd import model as M
    cat = object.__new__(M.ItemCatalog)
    cat.ids = torch.as_tensor(np.asarray(ids), dtype=torch.int32)
    cat.N = int(cat.ids.numel())
    return cat


def test_targets_keeps_order_and_repeats_and_marks_unknown_ids():
    cat = _host_catalog([3, 5, 9, 12, 40])
    per_line = [[12, 3, 3, 7, 40], [], [9, 9], [100, 1]]
    off, idx, longest = cat.targets(per_line, 4)
    assert off.dtype == torch.int64 and idx.dtype == torch.int32
    assert off.tolist() == [0, 5, 5, 7, 9] and idx.tolist() == [3, 0, 0, -1, 4, 2, 2, -1, -1] and longest == 5
    flat = np.concatenate([np.asarray(x, dtype=np.int64) for x in per_line])
    csr = (np.concatenate([[0], np.cumsum([len(x) for x in per_line])]).astype(np.int64), flat)
    off2, idx2, longest2 = cat.targets(csr, 4)
    assert torch.equal(off2, off) and torch.equal(idx2, idx) and longest2 == 5
    off3, idx3, longest3 = cat.targets([[], []], 2)
    assert off3.tolist() == [0, 0, 0] and idx3.tolist() == [-1] and longest3 == 0       # a non-null list
    assert cat.targets([list(range(32))], 1)[2] == 32
    with pytest.raises(ValueError, match="33 on a line, at most 32"):
        cat.targets([[3], list(range(33))], 2)
    with pytest.raises(ValueError, match=r"targets must hold one array of item ids per line \(3\)"):
        cat.targets([[3], [5]], 3)


def test_python_side_refusals():
    from score_amd import harness as h
    from score_amd import model as M
    why = {"DELF": "conditioned on the target item", "DEEMS": "item history", "SVDpp": "follow-up", "SASRec": "follow-up",
           "SCORE": "neighbour sets", "GCMC": "neighbour sets"}
    for name, word in why.items():
        m = object.__new__(M.MODELS[name])           # (no device: the refusal comes before anything is touched)
        for call in (lambda: m.item_ranks_async(None, None, [[1]]), lambda: m.item_ranks(None, None, [[1]]),
                     lambda: m.item_ranks_users_async(None, None, None, [[1]]),
                     lambda: h.evaluate_catalog_ranks_users(m, None, None)):
            with pytest.raises(NotImplementedError, match=word):
                call()
    g = object.__new__(M.GRU4Rec)
    with pytest.raises(ValueError, match="mutually exclusive"):
        g.item_ranks_async(None, None, [[1]], exclude=[[1]], exclude_idx=(None, None))
    other = _host_catalog([3, 5])
    other.model = object.__new__(M.GRU4Rec)
    with pytest.raises(ValueError, match="ItemCatalog built for this model"):
        g.item_ranks_async(None, other, [[1]])
    with pytest.raises(ValueError, match="ItemCatalog built for this model"):
        g.item_ranks_users_async([1], None, other, [[1]])
    with pytest.raises(ValueError, match="ItemCatalog built for this model"):
        g.item_ranks_async(None, "a catalogue", [[1]])
    for fn in (h.evaluate_catalog_ranks, h.evaluate_catalog_ranks_users):
        with pytest.raises(ValueError, match="candidates must be None or"):
            fn(None, [], None, candidates="x")
    assert issubclass(M.Caser, M.GRU4Rec) and M.Caser.item_ranks_async is M.GRU4Rec.item_ranks_async
    names = list(inspect.signature(M.GRU4Rec.item_ranks_async).parameters)
    assert names == ["self", "lines", "catalog", "targets", "exclude", "exclude_idx", "active_slices", "candidates", "max_candidates"]
    names = list(inspect.signature(M.GRU4Rec.item_ranks_users_async).parameters)
    assert names == ["self", "user_ids", "store", "catalog", "targets", "exclude_history", "candidates", "max_candidates"]
    assert list(inspect.signature(h.evaluate_catalog_ranks).parameters) == \
        ["model", "batches", "catalog", "neg_sample_num", "exclude_history", "candidates"]
    assert list(inspect.signature(h.evaluate_catalog_ranks_users).parameters) == \
        ["model", "store", "catalog", "exclude_history", "candidates", "lines_per_call"]
    assert "rank_quality_device" in h.catalog_quality_device.__doc__


# ---- the metrics: the reference's functions (point_models/harness.py getNDCG_at_K / getHR_at_K / getMRR), restated as they are
# written there, applied to explicit full ranklists with the target at place r
def _ref_ndcg(ranklist, target, k):
    rl = ranklist[:k]
    for i in range(len(rl)):
        if rl[i] == target:
            return math.log(2) / math.log(i + 2)
    return 0


def _ref_hr(ranklist, target, k):
    return 1 if target in ranklist[:k] else 0


def _ref_mrr(ranklist, target):
    for i in range(len(ranklist)):
        if ranklist[i] == target:
            return 1.0 / (i + 1)
    return 0


def test_rank_quality_device_against_the_reference_metrics_on_full_ranklists():
    from score_amd import harness as h
    rng = np.random.default_rng(4)
    N = 400
    r = np.concatenate([np.arange(0, 12), rng.integers(0, N, size=50), [N - 1, 127, 128, 129]])
    lists = [rng.permutation(N).tolist() for _ in r]
    tgt = [lst[int(x)] for lst, x in zip(lists, r)]
    want = [np.mean([_ref_ndcg(a, t, 5) for a, t in zip(lists, tgt)]), np.mean([_ref_ndcg(a, t, 10) for a, t in zip(lists, tgt)]),
            np.mean([_ref_hr(a, t, 1) for a, t in zip(lists, tgt)]), np.mean([_ref_hr(a, t, 5) for a, t in zip(lists, tgt)]),
            np.mean([_ref_hr(a, t, 10) for a, t in zip(lists, tgt)]), np.mean([_ref_mrr(a, t) for a, t in zip(lists, tgt)]),
            np.mean(r + 1.0)]
    got = h.rank_quality_device(torch.as_tensor(r, dtype=torch.int32))
    assert len(got) == 7 and np.allclose(got, want, rtol=0, atol=1e-12), (got, want)
    # catalog_quality_device on the same lists cut at 128: the first five equal, its MRR truncated
    top = torch.as_tensor(np.asarray([a[:128] for a in lists]), dtype=torch.int32)
    six = h.catalog_quality_device(top, torch.as_tensor(tgt, dtype=torch.int32))
    assert np.allclose(six[:5], got[:5], rtol=0, atol=1e-12) and six[5] < got[5]
    # a target outside the catalogue (ahead -1) counts 0, as a miss does; so does, with state, one that is not scored
    r2 = np.concatenate([r, [-1, -1]])
    got2 = h.rank_quality_device(torch.as_tensor(r2, dtype=torch.int32))
    assert np.allclose(got2[:6], np.asarray(want[:6]) * len(r) / len(r2), rtol=0, atol=1e-12) and abs(got2[6] - want[6]) < 1e-12
    st = np.ones_like(r2); st[-2:] = -1; st[0] = 0; st[1] = 2
    got3 = h.rank_quality_device(torch.as_tensor(r2, dtype=torch.int32), torch.as_tensor(st, dtype=torch.int32))
    keep = np.arange(len(r)) != 0
    lists3, tgt3 = [a for a, k_ in zip(lists, keep) if k_], [t for t, k_ in zip(tgt, keep) if k_]
    want3 = [sum(_ref_ndcg(a, t, 5) for a, t in zip(lists3, tgt3)) / len(r2), sum(_ref_ndcg(a, t, 10) for a, t in zip(lists3, tgt3)) / len(r2),
             sum(_ref_hr(a, t, 1) for a, t in zip(lists3, tgt3)) / len(r2), sum(_ref_hr(a, t, 5) for a, t in zip(lists3, tgt3)) / len(r2),
             sum(_ref_hr(a, t, 10) for a, t in zip(lists3, tgt3)) / len(r2), sum(_ref_mrr(a, t) for a, t in zip(lists3, tgt3)) / len(r2),
             np.mean(r[keep] + 1.0)]
    assert np.allclose(got3, want3, rtol=0, atol=1e-12), (got3, want3)
    with pytest.raises(ValueError, match="no targets"):
        h.rank_quality_device(torch.zeros((0,), dtype=torch.int32))
    with pytest.raises(ValueError, match="same targets"):
        h.rank_quality_device(torch.zeros((3,), dtype=torch.int32), torch.zeros((2,), dtype=torch.int32))


# ---- the GPU cases
def test_the_cases_targets():
    ch = 256
    want_n = [1, 15, 16, 17, 31, 32, 33, ch - 1, ch, ch + 1, 2 * ch + 1]
    assert [n_of(ch) for _, _, n_of, _, _ in kr.CASES] == want_n and len(set(kr.IDS)) == len(kr.CASES)
    assert {s for s, *_ in kr.CASES} == set(range(len(cc.SHAPES)))
    seen = set()
    for (s, L, n_of, counts, seed) in kr.CASES:
        N = n_of(ch)
        assert len(counts) == L
        t = kr.targets_of(N, ch, counts, seed)
        assert [len(x) for x in t] == counts and all(x.dtype == np.int32 for x in t)
        for x in t:
            if x.size == 32:
                assert {0, N - 1, -1, N} <= set(x.tolist()) and np.unique(x).size < x.size      # both ends, outside, a repeat
                for p in (ch - 1, ch, 2 * ch - 1, 2 * ch):
                    if p < N:
                        assert p in x and (seen.add("seam") is None)
            if x.size == 2:
                seen.add("repeat" if x[0] == x[1] else "outside")
        e = kr.exclusions_of(N, t, seed)
        assert e[-1].tolist() == list(range(N)) and all((np.diff(x) > 0).all() for x in e)
        for x, ex in zip(t, e):
            inside = x[(x >= 0) & (x < N)]
            assert inside.size == 0 or np.isin(inside, ex).any()                                # a target that is excluded
    assert seen == {"seam", "repeat", "outside"}


@pytest.mark.parametrize("i", range(len(kr.CASES)), ids=kr.IDS)
def test_the_restatements_sandwich_is_tight_at_the_cases_seeds(i):
    """the float64 restatement alone bounds a count from both sides (catalog_ranks_cases.sandwich); where the bounds differ by at
    most 2 for three quarters of a case's targets, a wrong count cannot hide between them"""
    d = kr.case_inputs(i, 256)
    _, y = cc.restated(d["kind"], d["c"], d["P"], d["lines"], d["rows"])
    tight = total = 0
    for l in range(d["L"]):
        t = d["targets"][l]
        lo, hi = kr.sandwich(y[l], t)
        inside = (t >= 0) & (t < d["N"])
        assert (lo[~inside] == -1).all() and (hi[~inside] == -1).all() and (lo <= hi).all()
        tight += int(((hi - lo)[inside] <= 2).sum())
        total += int(inside.sum())
    assert total >= 1 and 4 * tight >= 3 * total, (tight, total)
