"""The inputs of tests/test_gpu_point_edges.py (tests/point_edge_cases.py) judged on the float64 restatements alone, no GPU: every
case has the property it is there for (restated here from the kernels' own tiling rules), its filter stays within the model's
own cap, and the library's host-side layout accepts its shape (the library loads without a device).  For SASRec, the LDS bound
from both sides: (D, T, Fi) = (4, 137, 1) is accepted and (4, 138, 1) refused, by the layout and by the constructor."""
import numpy as np
import pytest
import torch

import point_edge_cases as pe
from score_amd import _lib
from score_amd.model import MODELS

sv_eps = pe.sv.LOGLOSS_EPS
LIB_NAME = {"svdpp": "SVDpp", "delf": "DELF", "caser": "Caser", "sasrec": "SASRec"}
# the issue's table: the shapes are not to be moved
SHAPES = {"svdpp": [(12, 30, 2, 3, 9), (24, 12, 1, 2, 9), (48, 7, 1, 1, 5), (96, 5, 1, 1, 5), (16, 16, 8, 8, 9), (16, 17, 1, 8, 9)],
          "delf": [(16, 65, 1, 1, 5), (4, 257, 1, 1, 3), (16, 9, 5, 5, 9), (32, 5, 4, 3, 5), (4, 9, 3, 3, 9), (8, 10, 3, 3, 9),
                   (16, 12, 3, 4, 40)],
          "caser": [(16, 58, 3, 4, 17), (16, 65, 3, 4, 9), (16, 66, 3, 4, 9), (64, 50, 1, 4, 9), (52, 50, 1, 5, 7), (16, 58, 3, 4, 3)],
          "sasrec": [(4, 130, 1, 1, 2), (4, 137, 1, 1, 1), (8, 8, 1, 2, 5), (8, 16, 1, 2, 5), (8, 17, 1, 2, 5), (4, 16, 1, 3, 5),
                     (20, 6, 1, 5, 5)]}


def _delf_tiling(C):
    """(CW, R, RC) of csrc/delf.hip: the power of two covering C, row groups per workgroup, rows per chunk (DELF_TT = 4 each)"""
    CW = 4
    while CW < C:
        CW <<= 1
    return CW, 256 // CW, 4 * (256 // CW)


def _forward(k):
    with torch.no_grad():
        return k.ref.forward(k.c, k.ref.to_torch(k.P), k.batch)


def test_the_table_holds_the_shapes_of_the_issue():
    for model, shapes in SHAPES.items():
        assert [r.shape for r in pe.CASES.values() if r.model == model] == shapes, model
    assert len(pe.CASES) == sum(len(s) for s in SHAPES.values()) == 26
    assert pe.N == 3000


@pytest.mark.parametrize("name", list(pe.CASES))
def test_filter_cap_and_host_side_layout(name):
    r = pe.CASES[name]
    D, T, Fu, Fi, B = r.shape
    k = pe.case(name)
    print("%s: kept %d of %d, the filter may take %d, the model's cap %d" % (name, k.kept.size, B, r.drop, pe.cap(r.model, B)))
    assert r.drop <= pe.cap(r.model, B) and B - k.kept.size <= r.drop and k.kept.size >= 1
    assert np.array_equal(k.batch_all["label"], np.arange(B) % 2)
    for f, v in k.batch.items():
        assert np.array_equal(v, k.batch_all[f][k.kept]), f
    out = _forward(k)
    assert np.isfinite(float(out["loss"]))
    if r.model == "svdpp":
        assert k.ref.kink_free(k.c, k.P, k.batch).all()
    elif r.model == "sasrec":
        assert k.ref.edge_free(k.c, k.P, k.batch).all()
    else:
        assert (out["relu_margin_per_sample"] > k.ref.RELU_THR).all()
    if r.model == "caser":
        others = np.arange(k.kept.size) != pe.ZERO_HISTORY_SAMPLE if r.forced == "zero_history" else np.ones(k.kept.size, dtype=bool)
        assert (out["window_margin_per_sample"][others] > k.ref.WINDOW_THR).all()
    cfg = _lib.make_config(pe.N, D, pe.H, T, 1, Fu, Fi, LIB_NAME[r.model])
    entries, n_w, n_reg = _lib.param_layout(cfg)
    assert len(entries) == len(k.ref.param_spec(k.c)) and n_w > 0
    assert _lib.workspace_layout(cfg, k.kept.size).total_bytes > 0 and _lib.workspace_layout(cfg, B).total_bytes > 0


@pytest.mark.parametrize("name", [n for n, r in pe.CASES.items() if r.model == "svdpp"])
def test_svdpp_cases_are_what_their_rows_claim(name):
    k = pe.case(name)
    D, T, Fu, Fi, B = k.row.shape
    G, ln = 256 // D, k.batch["user_seq_length"]
    out = _forward(k)
    assert (out["n"].numpy() > 0).all() and ln.min() >= 1
    # This model has no head in front of the sigmoid: a logit beyond +-17 leaves, under log_loss's epsilon, no gradient at all.
    # Where the row loop takes a second trip (T > G), the samples that take it carry a tenth of the batch's |d loss / d logit| at
    # least -- a slip in those rows shows in the gradients at full size; everywhere, the samples of T live rows do
    z, lab = out["z"].numpy(), k.batch["label"]
    y, q = 1 / (1 + np.exp(-z)), 1 / (1 + np.exp(z))
    dz = np.abs((-lab / (y + sv_eps) + (1 - lab) / (q + sv_eps)) * y * q)
    live = np.minimum(ln, T)
    print("%s: G = %d, live rows %s, |d loss / d logit| %s" % (name, G, live.tolist(), np.round(dz / dz.sum(), 3).tolist()))
    assert dz[live == T].sum() >= 0.1 * dz.sum()
    if T > G:
        assert dz[live > G].sum() >= 0.1 * dz.sum() and (live <= G).any()
    idle = {"svdpp_d12": (21, 4), "svdpp_d24": (10, 16), "svdpp_d48": (5, 16), "svdpp_d96": (2, 64)}
    if name in idle:
        assert 256 % D != 0 and (G, 256 - G * D) == idle[name]
    if name == "svdpp_d12":
        assert k.kept[:2].tolist() == [0, 1] and ln[0] == 1 and ln[1] == 3 * T      # a group with no row, a clipped length
        assert G < T <= 2 * G and ((ln > G) & (ln < T)).any()                      # two trips of the row loop, some ragged
    if name == "svdpp_d96":
        assert 64 < D < 128          # svdpp_wave_dsum's upper half partly filled
    if name == "svdpp_fmax":
        assert Fu == Fi == 8 and T == G and (ln >= T).any()
    if name == "svdpp_t17":
        assert T == G + 1 and Fi == 8 and (ln >= T).any()          # the row T - 1 is live somewhere: group 0's second trip


@pytest.mark.parametrize("name", [n for n, r in pe.CASES.items() if r.model == "delf"])
def test_delf_cases_are_what_their_rows_claim(name):
    k = pe.case(name)
    D, T, Fu, Fi, B = k.row.shape
    c, b = k.c, k.batch
    til = {0: _delf_tiling(c.Ci), 1: _delf_tiling(c.Cu)}          # side 0: the user history (Ci wide), side 1: the item history (Cu)
    lens = {0: b["user_seq_length"], 1: b["item_seq_length"]}
    live = {s: np.where(lens[s] <= 0, 0, np.minimum(lens[s], T)) for s in (0, 1)}
    out = _forward(k)
    if name == "delf_seam":
        assert k.kept.size == B and lens[0].tolist() == [64, 65, 1, 63, 130] and lens[1].tolist() == [65, 64, 130, 1, 63]
        for s in (0, 1):
            RC = til[s][2]
            assert RC == 64 and {RC - 1, RC, RC + 1, 1, T} == set(live[s].tolist())
    if name == "delf_t257":
        assert k.kept.size == B and lens[0].tolist() == [257, 256, 0] and lens[1].tolist() == [1, 300, 257]
        assert til[0][2] == til[1][2] == 256 and T == 257
        au = out["att_user"].numpy()
        assert np.array_equal(au[2], np.full(T, 1.0 / T)) and abs(au[2].sum() - 1) < 1e-12      # the zero length: exactly uniform
        assert not au[1, 256:].any() and au[0].all()
    if name == "delf_two_wave":
        assert c.Cu == c.Ci == 80 and til[0][0] == til[1][0] == 128          # CW > 64 on both sides
    if name == "delf_cu128":
        assert c.Cu == 128 and c.Ci == 96 and til[0][0] == til[1][0] == 128
    if name in ("delf_c12", "delf_c24"):
        C = {"delf_c12": 12, "delf_c24": 24}[name]
        assert c.Cu == c.Ci == C and C % 4 == 0 and C % 16 != 0 and C < til[0][0] <= 64      # idle lanes inside a group_sum width
        assert (live[0] < T).any() and (live[0] == T).any()
    if name == "delf_saturated":
        keys, lv = pe.delf_keys(c, k.P, b, 0)
        frac = float((np.abs(keys[lv]) > 0.999).mean())
        au, y = out["att_user"].numpy(), out["y_pred"].numpy()
        one_hot = int(((au.max(1) > 0.999) & (lens[0] >= 2)).sum())          # (a single live position is one-hot whatever the keys are)
        print("saturated: %.1f %% of the user-side keys beyond 0.999, %d of %d samples one-hot, y in [%.4f, %.4f]"
              % (100 * frac, one_hot, k.kept.size, y.min(), y.max()))
        assert frac > 0.5 and one_hot >= 30
        assert y.min() >= 1e-3 and y.max() <= 1 - 1e-3


@pytest.mark.parametrize("name", [n for n, r in pe.CASES.items() if r.model == "caser"])
def test_caser_cases_are_what_their_rows_claim(name):
    k = pe.case(name)
    D, T, Fu, Fi, B = k.row.shape
    out = _forward(k)
    arg, NW = out["arg"], k.c.NW
    assert NW == T - 49 and out["hwin"].shape == (k.kept.size, NW)
    if name == "caser_nw9":
        assert NW == 9 and (arg == 8).any()          # the second sweep's one window holds the maximum somewhere
    if name == "caser_nw16_b9":
        assert NW == 16 and (arg >= 8).any() and k.kept.size == 9          # (9 samples: share 0 of the params kernel holds two)
    if name == "caser_nw17":
        assert NW == 17 and np.unique(arg).size > 1
    if name == "caser_c256":
        assert k.c.C == 256 and NW == 1
    if name == "caser_c260":
        assert k.c.C == 260 and k.c.C - 256 == 4 and NW == 1
    if name == "caser_zero_history":
        z = pe.ZERO_HISTORY_SAMPLE
        assert k.kept.size == 3 and not k.batch["user_seq"][z].any() and k.batch["user_seq"][[0, 2]].all()
        hw = out["hwin"].numpy()
        assert NW == 9 and np.unique(hw[z]).size == 1 and arg[z] == 0
        assert hw[z, 0] == float(k.P["conv2d/bias"][0])
        assert np.unique(hw[0]).size == NW          # (the other samples have no tie)


@pytest.mark.parametrize("name", [n for n, r in pe.CASES.items() if r.model == "sasrec"])
def test_sasrec_cases_are_what_their_rows_claim(name):
    k = pe.case(name)
    D, T, Fu, Fi, B = k.row.shape
    C = k.c.Ci
    assert B != 3 and pe.sas_lds_floats(T, C) <= pe.SAS_LDS_LIMIT_FLOATS
    if name in ("sasrec_t130", "sasrec_t137"):
        assert 2 * T > 256 and k.kept.size == B
    if name == "sasrec_t130":
        assert 2 * T - 2 > 256          # the head's positive and negative rows of a sample
    if name == "sasrec_t137":
        assert C == 4 and pe.sas_lds_floats(137, 4) == 40826 <= 40960 == pe.SAS_LDS_LIMIT_FLOATS < pe.sas_lds_floats(138, 4)
    blocks = {"sasrec_t8": (1, 0), "sasrec_t16": (2, 0), "sasrec_t17": (2, 1)}
    if name in blocks:
        assert divmod(T, 8) == blocks[name]
    if name == "sasrec_c12":
        assert C == 12 and C // 2 == 6
    if name == "sasrec_c100":
        assert C == 100 and C // 2 == 50


def test_sasrec_lds_bound_from_both_sides():
    fits = lambda D, T, Fi: _lib.param_layout(_lib.make_config(pe.N, D, pe.H, T, 1, 1, Fi, "SASRec"))
    assert len(fits(4, 137, 1)[0]) == 14
    assert _lib.workspace_layout(_lib.make_config(pe.N, 4, pe.H, 137, 1, 1, 1, "SASRec"), 1).total_bytes > 0
    with pytest.raises(_lib.ScoreHipError):
        fits(4, 138, 1)
    # ... and at the widest rows, C = 128: T = 63 is the last that fits
    assert pe.sas_lds_floats(63, 128) <= pe.SAS_LDS_LIMIT_FLOATS < pe.sas_lds_floats(64, 128)
    assert len(fits(32, 63, 4)[0]) == 14
    with pytest.raises(_lib.ScoreHipError):
        fits(32, 64, 4)
    # the constructor: refused before anything touches a device, like max_time_len < 3 and item_fnum * eb_dim > 128
    SASRec = MODELS["SASRec"]
    with pytest.raises(ValueError, match="max_time_len = 138"):
        SASRec(pe.N, 4, pe.H, 138, 1, 1)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            SASRec(pe.N, 4, pe.H, 137, 1, 1)          # (the last shape that fits gets as far as the device check)
