"""CPU tests of the C-ABI boundary: the library builds/loads and exports every symbol
include/score_hip.h declares; layouts agree with the oracle's parameter spec.
No compute calls (no GPU here)."""
import os
import re

import numpy as np
import pytest

from oracle import score_oracle as so
from score_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "score_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|int64_t)\s+(score_\w+)\s*\(", src)))


def test_header_symbols_exported():
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 11
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(_lib.EXPORTS) == names


def test_head_forms_query_is_read_only_and_documented():
    """score_head_last_forms: host only, -1 until a pass has run in this process (no pass can run here); the header names every
    field of the packing tests/score_head_cases.py unpacks"""
    lib = _lib.load()
    v = lib.score_head_last_forms()
    assert v == -1 or (0 < v < 1 << 22 and v & (3 << 20))          # (a GPU test of the same process may have run a pass before)
    assert lib.score_head_last_forms() == v
    src = open(os.path.join(ROOT, "include", "score_hip.h")).read()
    doc = src[:src.index("int score_head_last_forms(void);")].rsplit("/*", 1)[1]
    for field in ("bits  0 ..  1", "bits  2 ..  4", "bits  5 ..  7", "bits  8 .. 15", "bits 16 .. 18", "bit  19", "bit  20", "bit 21"):
        assert field in doc, field


def test_gemm_and_gru_form_queries_are_read_only_and_documented():
    """score_gemm_last_form / score_gru_last_form: host only, -1 until a product / a recurrence has been launched in this process
    (none can be here); the header names every field tests/gemm_cases.py and tests/gru_cases.py unpack"""
    import gemm_cases
    import gru_cases
    lib = _lib.load()
    g, r = lib.score_gemm_last_form(), lib.score_gru_last_form()
    # (a GPU test of the same process may have launched before)
    assert g == -1 or (0 < g < 1 << 28 and gemm_cases.unpack(g)[0].family in (gemm_cases.F32, gemm_cases.X3) and gemm_cases.unpack(g)[0].slabs >= 1)
    assert r == -1 or (0 < r < 1 << 9 and 1 <= gru_cases.unpack(r).family <= 5 and gru_cases.unpack(r).waves in (2, 4, 8))
    assert lib.score_gemm_last_form() == g and lib.score_gru_last_form() == r
    src = open(os.path.join(ROOT, "include", "score_hip.h")).read()
    doc = src[:src.index("int score_gemm_last_form(void);")].rsplit("/*", 1)[1]
    for field in ("bits  0 ..  1", "bits  2 ..  3", "bits  4 ..  5", "bits  6 ..  7", "bit   8", "bits 12 .. 27", "-1 before the first"):
        assert field in doc, field
    doc = src[:src.index("int score_gru_last_form(void);")].rsplit("/*", 1)[1]
    for field in ("bits  0 ..  2", "bits  4 ..  7", "bit   8", "-1 before the first"):
        assert field in doc, field
    # the packing of the two case modules is the documented one
    assert gemm_cases.pack(gemm_cases.Form(gemm_cases.X3, 2, 0, 5), 1) == 2 | 2 << 2 | 1 << 6 | 5 << 12
    assert gru_cases.pack(gru_cases.Form(gru_cases.REG, 2, 1)) == 2 | 2 << 4 | 1 << 8


def test_coattn_forms_query_is_read_only_and_documented():
    """score_coattn_last_forms: host only, one word per direction, -1 until that direction has launched in this process (nothing
    can launch here, and a refused call writes nothing); the header names every field tests/coattn_cases.py unpacks"""
    import ctypes as C
    import coattn_cases
    lib = _lib.load()
    f, b = lib.score_coattn_last_forms(0), lib.score_coattn_last_forms(1)
    # (a GPU test of the same process may have launched before)
    assert f == -1 or (0 < f < 1 << 28 and coattn_cases.unpack_fwd(f).kmax in (4, 10, 20, 32) and coattn_cases.unpack_fwd(f).reg in (1, 2, 4))
    assert b == -1 or (0 < b < 1 << 22 and coattn_cases.unpack_bwd(b).kmax in (4, 10, 20, 32) and coattn_cases.unpack_bwd(b).spl in (1, 2, 4)
                       and coattn_cases.unpack_bwd(b).nm in (0, 1, 2, 4) and coattn_cases.unpack_bwd(b).mode in (0, 1))
    z = C.c_void_p(0)
    assert lib.score_coattn_fwd(z, 10, 6, 2, 3, 1, 1, z, z, z, z, z, z, 12, z, 12, z, 6, z, 0, z) == -1      # null table: refused
    assert lib.score_coattn_bwd(z, z, 10, 6, 2, 3, 1, 1, z, z, z, z, z, 12, z, 12, z, 6, z, z, z, 0, 0, z) == -1
    assert lib.score_coattn_last_forms(0) == f and lib.score_coattn_last_forms(1) == b and lib.score_coattn_last_forms(7) == b
    src = open(os.path.join(ROOT, "include", "score_hip.h")).read()
    doc = src[:src.index("int score_coattn_last_forms(")].rsplit("/*", 1)[1]
    for field in ("bit   0", "bits  1 ..  6", "bits  8 .. 10", "bits 12 .. 27", "bits 12 .. 14", "bit  16", "bits 20 .. 21",
                  "-1 before the first"):
        assert field in doc, field
    # the packing of the case module is the documented one
    assert coattn_cases.pack_fwd(coattn_cases.Fwd(1, 10, 1, 2)) == 1 | 10 << 1 | 1 << 8 | 2 << 12
    assert coattn_cases.pack_bwd(coattn_cases.Bwd(32, 2, 0, 1, 0)) == 32 << 1 | 2 << 8 | 1 << 16
    assert coattn_cases.pack_bwd(coattn_cases.Bwd(10, 1, 4, 0, 1)) == 10 << 1 | 1 << 8 | 4 << 12 | 1 << 20


def test_pull_geometry_query_is_host_only_and_documented():
    """score_pull_geometry: what score_launch_pull would use for (n, D), without a GPU and without touching score_pull_last_form;
    the header names the four outputs, the window thresholds and both refusals (tests/scatter_cases.py restates them)"""
    import ctypes as C
    import scatter_cases
    lib = _lib.load()
    before = lib.score_pull_last_form()
    w, l, g, c = (C.c_int32(-1) for _ in range(4))
    for n, D, want in ((1, 4, (8, 1, 256, 16)), (70000, 16, (8, 4, 64, 16)), (1 << 18, 12, (16, 4, 64, 16)),
                       (1 << 19, 20, (32, 8, 32, 16)), (1 << 20, 256, (64, 64, 4, 16)), ((1 << 20) - 1, 128, (32, 32, 8, 16))):
        assert lib.score_pull_geometry(n, D, C.byref(w), C.byref(l), C.byref(g), C.byref(c)) == 0
        assert (w.value, l.value, g.value, c.value) == want == scatter_cases.geometry(n, D), (n, D)
    assert lib.score_pull_geometry(8, 260, C.byref(w), C.byref(l), C.byref(g), C.byref(c)) == -2      # SCORE_E_SHAPE, as the launcher
    assert lib.score_pull_geometry(8, 6, C.byref(w), C.byref(l), C.byref(g), C.byref(c)) == -1
    assert lib.score_pull_geometry(8, 16, None, None, None, None) == -1
    assert (w.value, l.value, g.value, c.value) == (32, 32, 8, 16)                                   # a refusal writes nothing
    assert lib.score_pull_last_form() == before
    src = open(os.path.join(ROOT, "include", "score_hip.h")).read()
    doc = src[:src.index("int score_pull_geometry(")].rsplit("/*", 1)[1]
    for field in ("*window", "*lanes_per_row", "*groups_per_block", "*long_chain", "2^18", "2^19", "2^20", "SCORE_E_BADARG",
                  "SCORE_E_SHAPE", "D above 256", "score_segment_sum_rows"):
        assert field in doc, field


@pytest.mark.parametrize("mt",so.MODEL_TYPES)
def test_param_layout_matches_oracle_spec(mt):
    # same variables, names, shapes, creation order and L2 filter as score.py (oracle param_spec)
    cfg = _lib.make_config(1000, 16, 32, 11, 10, 3, 4, mt)
    entries, n_w, n_reg = _lib.param_layout(cfg)
    spec = so.param_spec(so.Cfg(1000, 16, 32, 11, 10, 3, 4, mt))[1:]
    assert [e[0] for e in entries] == [s[0] for s in spec]
    for e, s in zip(entries, spec):
        shape = (e[2], e[3]) if e[3] else (e[2],)
        assert shape == tuple(s[1]), e[0]
        assert bool(e[4]) == s[3], e[0]
        assert {"zeros": 0, "ones": 1, "glorot": 2}[s[2]] == e[5]
        assert e[1] % 4 == 0
        assert (e[1] < n_reg) == bool(e[4])
    # no overlap
    spans = sorted((e[1], e[1] + e[2] * (e[3] or 1)) for e in entries)
    for a, b in zip(spans, spans[1:]):
        assert a[1] <= b[0]
    assert spans[-1][1] <= n_w


def test_workspace_layout_and_errors():
    cfg = _lib.make_config(1000, 16, 32, 11, 10, 3, 4, "SCORE")
    ws = _lib.workspace_layout(cfg, 200)
    assert ws.total_bytes > 0 and ws.loss > 0
    bad = _lib.make_config(1000, 15, 32, 11, 10, 3, 4, "SCORE")     # D not a multiple of 4
    with pytest.raises(_lib.ScoreHipError):
        _lib.workspace_layout(bad, 200)
    with pytest.raises(_lib.ScoreHipError):
        _lib.workspace_layout(cfg, 0)


def test_model_requires_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from score_amd.model import SCORE
    with pytest.raises(RuntimeError):
        SCORE(100, 4, 8, 3, 2, 3, 4)


def test_stripped_probe_kernels_cannot_reach_the_product_build():
    """the timing probes' wrong-by-design switches (no loads / no matrix instruction / no stores) stop the preprocessor
    unless -DSCORE_PROBE_BUILD is beside them, and build.py refuses that flag"""
    import subprocess
    from score_amd import build as b
    src = os.path.join(b.CSRC, "gru.hip")
    cmd = ["/opt/rocm/bin/hipcc"] + b.FLAGS + ["-E", "-DGRP_NOMFMA", src, "-o", os.devnull]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode != 0 and "SCORE_PROBE_BUILD" in out.stderr
    saved = list(b.FLAGS)
    try:
        b.FLAGS.append("-DSCORE_PROBE_BUILD")
        with pytest.raises(RuntimeError):
            b.build()
    finally:
        b.FLAGS[:] = saved


def test_ctypes_structures_match_the_headers_layout():
    """every ctypes.Structure of score_amd/_lib.py against sizeof / late-field offsets of the C struct it stands for
    (score_abi_struct_sizes, host only): a field added on one side only shows here, not as a wrong pointer on the GPU"""
    import ctypes as C
    lib = _lib.load()
    out = (C.c_int64 * 32)()
    n = lib.score_abi_struct_sizes(out, 32)
    assert n == 14
    got = list(out)[:n]
    want = [None, C.sizeof(_lib.Config), C.sizeof(_lib.ParamEntry), C.sizeof(_lib.Batch), C.sizeof(_lib.Workspace), C.sizeof(_lib.Guard),
            C.sizeof(_lib.AdamTable), C.sizeof(_lib.State), C.sizeof(_lib.TrainStep), C.sizeof(_lib.Graph), C.sizeof(_lib.BatchOut),
            _lib.State.plan_workspace.offset, _lib.TrainStep.plan_stream.offset, _lib.AdamTable.skipped_steps.offset]
    names = ["score_step_scalars_t", "score_config_t", "score_param_entry_t", "score_batch_t", "score_workspace_t", "score_guard_t",
             "score_adam_table_t", "score_state_t", "score_train_step_t", "score_graph_t", "score_batch_out_t",
             "offsetof(score_state_t, plan_workspace)", "offsetof(score_train_step_t, plan_stream)",
             "offsetof(score_adam_table_t, skipped_steps)"]
    for k, (g, w) in enumerate(zip(got, want)):
        assert w is None or g == w, (names[k], g, w)
    assert lib.score_abi_struct_sizes(out, 3) == -1
