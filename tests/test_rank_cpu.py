"""The line-form ranking pass (score_rank_forward; GRU4Rec.rank / Caser.rank) without a GPU: the two symbols and their
declarations, score_rank_workspace_bytes and its refusals, the split head's column bookkeeping (tests/rank_cases.py) against the
restatements' forward on the expanded batch, the cases' gap condition, and the Python-side argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rank_cases as rc
from score_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_BADARG, E_SHAPE = -1, -2


def _bytes(cfg, L, n_cand):
    n = C.c_int64(-7)
    rc_ = _lib.load().score_rank_workspace_bytes(C.byref(cfg), L, n_cand, C.byref(n))
    return rc_, n.value


def test_symbols_are_exported_declared_and_bound():
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "score_hip.h")).read(), flags=re.S)
    for name in ("score_rank_workspace_bytes", "score_rank_forward"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert getattr(lib, name).restype is C.c_int            # (a status, although the first one's name ends in _bytes)
    assert "score_rank_batch_t" in src
    # five pointers, three int32, padded to the pointers' alignment
    assert C.sizeof(_lib.RankBatch) == 56 and _lib.RankBatch.L.offset == 40 and _lib.RankBatch.active_slices.offset == 48
    assert [f[0] for f in _lib.RankBatch._fields_] == ["user_seq", "length", "target_user", "cand_items", "label", "L", "C", "active_slices"]


@pytest.mark.parametrize("mt", ["GRU4Rec", "Caser"])
def test_workspace_bytes_is_positive_and_never_shrinks(mt):
    cfg = _lib.make_config(3000, 16, 32, 50, 1, 3, 4, mt)
    base = _lib.workspace_layout(cfg, 10).total_bytes
    rc_, n = _bytes(cfg, 10, 100)
    assert rc_ == 0 and n > base        # the B = L workspace and the pass's own regions behind it
    assert _lib.rank_workspace_bytes(cfg, 10, 100) == n
    prev = 0
    for L in (1, 2, 3, 10, 11, 100, 1000):
        rc_, n = _bytes(cfg, L, 100)
        assert rc_ == 0 and n > 0 and n >= prev, (L, n, prev)
        prev = n
    prev = 0
    for n_cand in (1, 2, 15, 16, 17, 100, 101, 5000):
        rc_, n = _bytes(cfg, 10, n_cand)
        assert rc_ == 0 and n > 0 and n >= prev and n % 16 == 0, (n_cand, n, prev)
        prev = n


def test_workspace_bytes_refusals():
    lib = _lib.load()
    for mt, code in _lib.MODEL_TYPES.items():
        point = code >= 7
        cfg = _lib.make_config(3000, 16, 32, 50, 1 if point else 5, 3, 4, mt)
        rc_, n = _bytes(cfg, 10, 100)
        if mt in ("GRU4Rec", "Caser"):
            assert rc_ == 0 and n > 0
        else:
            assert rc_ == E_SHAPE and n == -7, mt         # model types 0 - 6 and 9 - 12: no line form; *bytes untouched
    assert sorted(c for m, c in _lib.MODEL_TYPES.items() if m not in ("GRU4Rec", "Caser")) == [0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12]
    cfg = _lib.make_config(3000, 16, 32, 50, 1, 3, 4, "GRU4Rec")
    assert _bytes(cfg, 0, 100)[0] == E_BADARG and _bytes(cfg, 10, 0)[0] == E_BADARG and _bytes(cfg, -1, -1)[0] == E_BADARG
    assert lib.score_rank_workspace_bytes(C.byref(cfg), 10, 100, None) == E_BADARG
    assert lib.score_rank_workspace_bytes(None, 10, 100, C.byref(C.c_int64(0))) == E_BADARG
    # hidden_size % 4: the item columns of bn1 would not start at a 16-byte group
    assert _bytes(_lib.make_config(3000, 16, 30, 50, 1, 3, 4, "GRU4Rec"), 10, 100)[0] == E_SHAPE
    with pytest.raises(_lib.ScoreHipError, match="unsupported shape"):
        _lib.rank_workspace_bytes(_lib.make_config(3000, 16, 32, 50, 1, 3, 4, "DELF"), 10, 100)
    # score_rank_forward's host-side refusals come before any launch (no device here)
    st, rb = _lib.State(), _lib.RankBatch()
    assert lib.score_rank_forward(C.byref(cfg), C.byref(st), None, 0.0, None, None, None) == E_BADARG
    assert lib.score_rank_forward(C.byref(_lib.make_config(3000, 16, 32, 50, 1, 3, 4, "SASRec")), C.byref(st), C.byref(rb), 0.0,
                                  C.c_void_p(16), C.c_void_p(16), None) == E_SHAPE
    assert lib.score_rank_forward(C.byref(cfg), C.byref(st), C.byref(rb), 0.0, C.c_void_p(16), C.c_void_p(16), None) == E_BADARG    # L = C = 0


@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("i", range(len(rc.CASES)), ids=rc.IDS)
def test_split_head_equals_the_restatements_forward(i, moved):
    """line part + candidate part in float64 == forward on the expanded batch of L * C samples, to 1e-12: the column ranges of
    the library's head input (Caser's three pad rows included), bn1's affine on either side of the split, fc1's bias once"""
    kind, c, P, b, L, n_cand = rc.case(i, moved)
    ref = rc.REF[kind]
    # (a shape the library's pass takes: what is pinned here is what runs there)
    assert _lib.rank_workspace_bytes(_lib.make_config(c.N, c.D, c.H, c.T, 1, c.Fu, c.Fi, kind), L, n_cand) > 0
    for reg in (0.0, 1e-3):
        with torch.no_grad():
            Pt = ref.to_torch(P)
            want = ref.forward(c, Pt, b, reg)
            got = rc.split_forward(kind, c, Pt, b, L, n_cand, reg)
        dy = float((got["y_pred"] - want["y_pred"]).abs().max())
        dl = abs(float(got["loss"]) - float(want["loss"]))
        print(rc.IDS[i], "moved" if moved else "initial", "reg", reg, "max |dy|", dy, "|dloss|", dl)
        assert got["y_pred"].shape == (L * n_cand,) and dy < 1e-12 and dl < 1e-12


def test_split_head_layout_is_the_librarys():
    """head_layout restates csrc/engine.hip's column offsets: the widths must be those of the library's bn1 / fc1 variables"""
    for kind, dims in (("GRU4Rec", (16, 32, 9, 3, 4)), ("Caser", (8, 32, 50, 2, 2)), ("Caser", (16, 32, 51, 3, 4))):
        c = rc.cfg_of(kind, dims)
        Dhead, off_ti, pad = rc.head_layout(kind, c)
        cfg = _lib.make_config(c.N, c.D, c.H, c.T, 1, c.Fu, c.Fi, kind)
        ent = {e[0]: e for e in _lib.param_layout(cfg)[0]}
        assert ent["bn1/gamma"][2] == Dhead and ent["fc1/kernel"][2:4] == (Dhead, 200)
        assert off_ti % 4 == 0 and Dhead == c.Dhead + len(pad)


@pytest.mark.parametrize("i", range(len(rc.CASES)), ids=rc.IDS)
def test_every_case_meets_the_gap_condition(i):
    """what makes 'rank and eval give equal ranks' (tests/test_gpu_rank.py) a condition on the inputs and not a tolerance"""
    kind, c, P, b, L, n_cand = rc.case(i)
    y, _ = rc.restated(kind, c, P, b, L, n_cand)
    gap = float(rc.line_gaps(y, L, n_cand).min())
    print(rc.IDS[i], "seed", rc.CASES[i][4], "smallest positive-to-negative gap %.3g" % gap)
    assert gap >= rc.MIN_GAP
    for k in ("user_seq", "user_seq_length", "target_user"):       # the batch is made of lines, the labels are 1, 0, ..., 0
        v = b[k].reshape((L, n_cand) + b[k].shape[1:])
        assert (v == v[:, :1]).all()
    assert b["label"].reshape(L, n_cand)[:, 0].all() and b["label"].sum() == L


def test_the_issues_seed_for_the_one_tile_shape_misses_the_gap():
    """(16, 64, 20, 3, 4), L = 2, C = 16 at seed 4: 3.5e-4 -- why that row's seed is 5"""
    kind, dims, L, n_cand = "GRU4Rec", (16, 64, 20, 3, 4), 2, 16
    assert rc.CASES[3][:4] == (kind, dims, L, n_cand) and rc.CASES[3][4] == 5
    c = rc.cfg_of(kind, dims)
    y, _ = rc.restated(kind, c, rc.params_of(kind, c), rc.line_batch(kind, c, L, n_cand, 4), L, n_cand)
    assert 3e-4 < rc.line_gaps(y, L, n_cand).min() < 4e-4


def test_python_side_argument_errors():
    from score_amd import model as M
    assert M.rank_lines(1000, 99) == (10, 100) and M.rank_lines(5, 0) == (5, 1)
    for B, neg in ((999, 99), (1001, 99), (7, 1), (50, 99)):
        with pytest.raises(ValueError, match="not made of lines"):
            M.rank_lines(B, neg)
    assert M.GRU4Rec.rank_unsupported is None and M.Caser.rank_unsupported is None
    why = {"DELF": "conditioned on the target item", "DEEMS": "item history", "SVDpp": "follow-up", "SASRec": "follow-up",
           "SCORE": "neighbour sets", "RRN": "neighbour sets", "GCMC": "neighbour sets"}
    for name, word in why.items():
        m = object.__new__(M.MODELS[name])           # (no device: the refusal comes before anything is touched)
        for call in (lambda: m.rank_async(None, 0.0), lambda: m.rank(None, None, 0.0)):
            with pytest.raises(NotImplementedError, match=word):
                call()
    import inspect
    from score_amd import harness as h
    assert inspect.signature(h.evaluate_device).parameters["shared_history"].default is False
    sig = inspect.signature(M.GRU4Rec.rank_async).parameters
    assert sig["neg_sample_num"].default == h.TEST_NEG_SAMPLE_NUM == 99 and sig["verify"].default is False
