"""Top-K over an item catalogue (score_catalog_build / _plan / _topk; GRU4Rec.recommend / Caser.recommend) without a GPU: the
symbols and their declarations, the ctypes layouts against the header's, score_catalog_plan, every host-side refusal, the
Python-side refusals, the restatement's selection (tests/catalog_cases.py) against a brute-force one, and
harness.catalog_quality_device's arithmetic against harness.get_ranking_quality."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import catalog_cases as cc
import rank_cases as rc
from score_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_BADARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
NAMES = ("score_catalog_build", "score_catalog_plan", "score_catalog_topk", "score_catalog_struct_sizes")


def _cfg(mt="GRU4Rec", H=32, T=50):
    return _lib.make_config(3000, 16, H, T, 1 if _lib.MODEL_TYPES[mt] >= 7 else 5, 3, 4, mt)


def _plan(cfg, L, N, k):
    chunk, nchunk, n = C.c_int32(-7), C.c_int32(-7), C.c_int64(-7)
    rc_ = _lib.load().score_catalog_plan(C.byref(cfg), L, N, k, C.byref(chunk), C.byref(nchunk), C.byref(n))
    return rc_, chunk.value, nchunk.value, n.value


def test_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "score_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert getattr(lib, name).restype is C.c_int
    assert re.search(r"#define\s+SCORE_CATALOG_KMAX\s+128\b", src) and _lib.CATALOG_KMAX == 128 == cc.KMAX
    assert "score_catalog_t" in src and "score_catalog_lines_t" in src


def test_ctypes_layouts_match_the_header():
    lib = _lib.load()
    out = (C.c_int64 * 8)()
    assert lib.score_catalog_struct_sizes(out, 8) == 6
    assert list(out)[:6] == [C.sizeof(_lib.Catalog), C.sizeof(_lib.CatalogLines), _lib.Catalog.zcat.offset,
                             _lib.CatalogLines.excl_off.offset, _lib.CatalogLines.excl_idx.offset, _lib.CATALOG_KMAX]
    assert lib.score_catalog_struct_sizes(out, 5) == E_BADARG and lib.score_catalog_struct_sizes(None, 8) == E_BADARG
    assert [f[0] for f in _lib.Catalog._fields_] == ["item_rows", "N", "zcat"]
    assert [f[0] for f in _lib.CatalogLines._fields_] == ["user_seq", "length", "target_user", "L", "active_slices", "excl_off", "excl_idx"]


@pytest.mark.parametrize("mt", ["GRU4Rec", "Caser"])
def test_plan_is_deterministic_and_its_chunk_a_positive_multiple_of_16(mt):
    cfg = _cfg(mt)
    base = _lib.workspace_layout(cfg, 10).total_bytes
    for L in (1, 3, 10, 100, 1000):
        for N in (1, 15, 16, 17, 255, 256, 257, 513, 40000, 1000003):
            for k in (1, 10, 128):
                got = _plan(cfg, L, N, k)
                assert got == _plan(cfg, L, N, k)
                rc_, chunk, nchunk, nbytes = got
                assert rc_ == 0 and chunk > 0 and chunk % 16 == 0, got
                assert nchunk == -(-N // chunk) and nchunk >= 1
                # behind the B = L workspace: zline [L, 200], the zero ids [L, T, max(Fu, Fi)], the chunks' lists of 8-byte keys
                own = 4 * (L * 200 + L * 50 * 4) + 8 * L * nchunk * k
                assert own <= nbytes - _lib.workspace_layout(cfg, L).total_bytes < own + 64 and nbytes % 16 == 0
                assert _lib.catalog_plan(cfg, L, N, k) == (chunk, nchunk, nbytes)
    # the sizes the GPU cases stand on: small catalogues are one chunk of 256 for 1 and 3 lines
    assert _plan(cfg, 1, 513, 128)[1:3] == (256, 3) and _plan(cfg, 3, 256, 10)[1:3] == (256, 1)
    assert _plan(cfg, 10, 100, 10)[3] > base


def test_plan_refusals():
    lib = _lib.load()
    for mt in _lib.MODEL_TYPES:
        got = _plan(_cfg(mt), 10, 1000, 10)
        if mt in ("GRU4Rec", "Caser"):
            assert got[0] == 0
        else:
            assert got == (E_SHAPE, -7, -7, -7), mt              # no line form: nothing is written
    cfg = _cfg()
    for L, N, k in ((0, 100, 10), (-1, 100, 10), (10, 0, 10), (10, -5, 10), (10, 100, 0), (10, 100, 129), (10, 100, -1)):
        assert _plan(cfg, L, N, k) == (E_BADARG, -7, -7, -7), (L, N, k)
    assert _plan(cfg, 10, 100, 1)[0] == 0 and _plan(cfg, 10, 100, 128)[0] == 0
    assert _plan(cfg, 10, (1 << 30) + 1, 10)[0] == E_SHAPE
    assert _plan(_cfg(H=30), 10, 100, 10)[0] == E_SHAPE                 # hidden_size % 4, as score_rank_forward
    i32, i64 = C.byref(C.c_int32(0)), C.byref(C.c_int64(0))
    assert lib.score_catalog_plan(None, 10, 100, 10, i32, i32, i64) == E_BADARG
    assert lib.score_catalog_plan(C.byref(cfg), 10, 100, 10, None, i32, i64) == E_BADARG
    assert lib.score_catalog_plan(C.byref(cfg), 10, 100, 10, i32, None, i64) == E_BADARG
    assert lib.score_catalog_plan(C.byref(cfg), 10, 100, 10, i32, i32, None) == E_BADARG
    with pytest.raises(_lib.ScoreHipError, match="unsupported shape"):
        _lib.catalog_plan(_cfg("DELF"), 10, 100, 10)


def test_build_and_topk_refuse_on_the_host_before_any_launch():
    """no device here: every one of these returns before it would touch one"""
    lib = _lib.load()
    cfg = _cfg()
    p = C.c_void_p(64)                                   # (never dereferenced: the refusals come first)
    st = _lib.State(table=p, w=p, workspace=p, workspace_bytes=0)
    cat = _lib.Catalog(p, 100, p)
    ln = _lib.CatalogLines(p, p, p, 3, 0, None, None)
    build = lambda c=cfg, s=st, t=cat: lib.score_catalog_build(C.byref(c) if c else None, C.byref(s) if s else None,
                                                               C.byref(t) if t else None, None)
    assert build(c=None) == E_BADARG and build(s=None) == E_BADARG and build(t=None) == E_BADARG
    assert build(t=_lib.Catalog(None, 100, p)) == E_BADARG and build(t=_lib.Catalog(p, 100, None)) == E_BADARG
    assert build(t=_lib.Catalog(p, 0, p)) == E_BADARG and build(t=_lib.Catalog(p, -3, p)) == E_BADARG
    assert build(s=_lib.State(table=None, w=p)) == E_BADARG and build(s=_lib.State(table=p, w=None)) == E_BADARG
    for mt in _lib.MODEL_TYPES:
        if mt not in ("GRU4Rec", "Caser"):
            assert build(c=_cfg(mt)) == E_SHAPE, mt
    assert build(c=_cfg(H=30)) == E_SHAPE

    def topk(c=cfg, s=st, t=cat, l=ln, k=10, idx=p, logit=p):
        return lib.score_catalog_topk(C.byref(c) if c else None, C.byref(s) if s else None, C.byref(t) if t else None,
                                      C.byref(l) if l else None, k, idx, logit, None, None)
    assert topk(c=None) == E_BADARG and topk(s=None) == E_BADARG and topk(t=None) == E_BADARG and topk(l=None) == E_BADARG
    assert topk(idx=None) == E_BADARG and topk(logit=None) == E_BADARG
    assert topk(k=0) == E_BADARG and topk(k=129) == E_BADARG and topk(k=-1) == E_BADARG
    assert topk(l=_lib.CatalogLines(p, p, p, 0, 0, None, None)) == E_BADARG
    assert topk(t=_lib.Catalog(p, 0, p)) == E_BADARG
    assert topk(t=_lib.Catalog(None, 100, p)) == E_BADARG and topk(t=_lib.Catalog(p, 100, None)) == E_BADARG
    for bad in (_lib.CatalogLines(None, p, p, 3, 0, None, None), _lib.CatalogLines(p, None, p, 3, 0, None, None),
                _lib.CatalogLines(p, p, None, 3, 0, None, None), _lib.CatalogLines(p, p, p, 3, 0, p, None)):
        assert topk(l=bad) == E_BADARG
    assert topk(s=_lib.State(table=p, w=p, workspace=None)) == E_BADARG
    for mt in _lib.MODEL_TYPES:
        if mt not in ("GRU4Rec", "Caser"):
            assert topk(c=_cfg(mt)) == E_SHAPE, mt
    # the workspace: one byte short of the plan's figure is refused, still before any launch
    need = _lib.catalog_plan(cfg, 3, 100, 10)[2]
    assert topk(s=_lib.State(table=p, w=p, workspace=p, workspace_bytes=need - 1)) == E_WORKSPACE
    assert topk() == E_WORKSPACE                                           # (workspace_bytes = 0)


def test_python_side_refusals():
    from score_amd import model as M
    why = {"DELF": "conditioned on the target item", "DEEMS": "item history", "SVDpp": "follow-up", "SASRec": "follow-up",
           "SCORE": "neighbour sets", "RRN": "neighbour sets", "GCMC": "neighbour sets"}
    for name, word in why.items():
        m = object.__new__(M.MODELS[name])           # (no device: the refusal comes before anything is touched)
        for call in (lambda: m.recommend_async(None, None), lambda: m.recommend(None, None), lambda: M.ItemCatalog(m, None),
                     lambda: m.lines_of(None)):
            with pytest.raises(NotImplementedError, match=word):
                call()
    assert M.GRU4Rec.weights_version == 0 and M.Caser.recommend_async is M.GRU4Rec.recommend_async
    from score_amd import harness as h
    with pytest.raises(ValueError, match="k >= 10"):
        h.catalog_quality_device(torch.zeros((2, 9), dtype=torch.int32), torch.zeros((2,), dtype=torch.int32))


def test_the_restatements_selection_equals_a_brute_force_one():
    rng = np.random.default_rng(5)
    for trial in range(40):
        N = int(rng.integers(1, 60))
        v = rng.standard_normal(N).round(1)                                  # (rounded: many ties)
        if trial % 3 == 0:
            v[rng.integers(0, N, size=2)] = np.nan
        if trial % 4 == 0:
            v[rng.integers(0, N)] = -np.inf
        excl = np.unique(rng.integers(0, N, size=int(rng.integers(0, N + 1)))) if trial % 2 else np.zeros((0,), dtype=np.int64)
        for k in (1, 10, 128):
            idx, val = cc.select(v, k, excl)
            bidx, bval = cc.select_brute(v, k, excl)
            assert idx.tolist() == bidx, (trial, k)
            assert np.array_equal(val, np.asarray(bval), equal_nan=True)
            assert not np.isin(idx[idx >= 0], excl).any() and (idx >= 0).sum() == min(k, N - len(excl))
    idx, val = cc.select(np.asarray([1.0, 2.0, 2.0, np.nan, -np.inf, 2.0]), 6)
    assert idx.tolist() == [1, 2, 5, 0, 4, 3]                                # ties by index, -inf in front of NaN


def test_the_restatement_is_split_forward_in_front_of_its_sigmoid():
    kind, dims = cc.SHAPES[0]
    c = rc.cfg_of(kind, dims)
    P = rc.params_of(kind, c, moved=True)
    lines, rows = cc.lines_of(kind, c, 2, 3), cc.catalog_rows(c, 19, 4)
    assert (np.diff(rows[:, 0]) > 0).all() and rows.min() >= 1 and rows.max() < c.N
    logits, y = cc.restated(kind, c, P, lines, rows)
    assert logits.shape == y.shape == (2, 19) and logits.dtype == np.float64
    assert np.abs(1.0 / (1.0 + np.exp(-logits)) - y).max() < 1e-15
    assert torch.sigmoid.__name__ == "sigmoid"                               # (the recorder is gone again)
    b = cc.expanded(lines, rows)
    want, _ = rc.restated(kind, c, P, b, 2, 19)
    assert np.array_equal(want.reshape(2, 19), y)


def test_catalog_quality_agrees_with_get_ranking_quality_on_hand_made_lists():
    """lines of 1 + 11 candidates, the list = all 12 in score order (k = 12): the positive's position is its rank"""
    from score_amd import harness as h
    rng = np.random.default_rng(9)
    n_lines, per = 7, 12
    preds = rng.permuted(np.tile(np.linspace(0.05, 0.95, per), (n_lines, 1)), axis=1)     # distinct scores in every line
    ids = np.tile(np.arange(100, 100 + per), (n_lines, 1))
    want = h.get_ranking_quality(preds.reshape(-1), ids.reshape(-1), per - 1)
    top = np.argsort(-preds, axis=1, kind="stable").astype(np.int32)                      # candidate indices, best first
    got = h.catalog_quality_device(torch.from_numpy(top), torch.zeros((n_lines,), dtype=torch.int32))
    assert len(got) == 6 and np.allclose(got, want, rtol=0, atol=1e-12), (got, want)
    # a positive that is absent counts 0 everywhere; one at position 9 counts for @10 only, MRR 1/10
    top = torch.arange(1, 11, dtype=torch.int32).repeat(2, 1)
    got = h.catalog_quality_device(top, torch.tensor([10, 77], dtype=torch.int32))
    import math
    assert np.allclose(got, (0.0, 0.5 * math.log(2) / math.log(11), 0.0, 0.0, 0.5, 0.05), rtol=0, atol=1e-12), got
