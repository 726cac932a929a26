"""Caser without a GPU: the float64 restatement the GPU tests compare against (tests/caser_ref.py) against central finite
differences; the parameter layout the library reports (host code: the library loads without a device) against the variables of
point_model.py:140-164 in TF creation order, with the padded head input's internal row counts; the refusal of max_time_len < 50;
the helper pair that carries arrays across the Python boundary; and the inputs of the GPU tests judged on the restatement alone."""
import math

import numpy as np
import pytest
import torch

import caser_ref as cr
from score_amd import _lib

INIT = {"zeros": 0, "ones": 1, "glorot": 2, "glorot_conv": 3}


def test_restatement_gradients_match_finite_differences():
    D, T, Fu, Fi, B = 4, 52, 2, 2, 6
    c = cr.Cfg(2000, D, 7, T, Fu, Fi)
    assert c.NW == 3
    rng = np.random.default_rng(5)
    P = cr.init_params(c, 9)
    for n in P:            # away from the initial values' symmetries (zero biases, ones)
        P[n] = (P[n] + 0.1 * rng.standard_normal(P[n].shape)).astype(np.float32)
    b = cr.random_batch(rng, c, B)
    b["label"] = np.array([0, 1, 1, 0, 1, 0], dtype=np.int32)
    b, _, kept = cr.away_from_kinks(c, P, b)                  # (the differences move a pre-activation by ~1e-6)
    lam = 1e-2
    out, g = cr.loss_and_grads(c, P, b, lam)
    assert np.unique(out["arg"]).size > 1
    P64 = {k: np.asarray(v, dtype=np.float64) for k, v in P.items()}

    def loss(Q):
        with torch.no_grad():
            return float(cr.forward(c, {k: torch.from_numpy(v) for k, v in Q.items()}, b, lam)["loss"])
    touched = np.unique(np.concatenate([b["user_seq"].ravel(), b["target_user"].ravel(), b["target_item"].ravel()]))
    touched = touched[touched != 0]
    h = 1e-6
    for name in P64:
        flat = P64[name].reshape(-1)
        idx = (touched[:, None] * c.D + np.arange(c.D)[None, :]).ravel() if name == "emb_mtx" else np.arange(flat.size)
        num = np.empty(idx.size)
        for j, i in enumerate(idx):
            keep = flat[i]
            flat[i] = keep + h
            lp = loss(P64)
            flat[i] = keep - h
            lm = loss(P64)
            flat[i] = keep
            num[j] = (lp - lm) / (2 * h)
        ana = g[name].reshape(-1)[idx]
        assert np.abs(ana - num).max() <= 1e-6 + 1e-5 * np.abs(num).max(), (name, np.abs(ana - num).max())
    # the masked row 0 and the rows nothing names get nothing; a row named only by padded positions does get gradient
    assert not g["emb_mtx"][0].any()
    others = np.setdiff1d(np.arange(1, c.N), touched)
    assert others.size and not g["emb_mtx"][others].any()
    short = [i for i in range(len(kept)) if b["user_seq_length"][i] < T]
    assert short and all(np.abs(g["emb_mtx"][b["user_seq"][i, -1]]).max() > 0 for i in short)
    # the length tensor is not read
    out2, g2 = cr.loss_and_grads(c, P, dict(b, user_seq_length=np.ones_like(b["user_seq_length"])), lam)
    assert float(out2["loss"].detach()) == float(out["loss"].detach()) and all(np.array_equal(g[k], g2[k]) for k in g)


@pytest.mark.parametrize("T,Fu,Fi", [(50, 3, 4), (50, 1, 5), (57, 1, 2)])
def test_param_layout_is_the_tf_variable_list_with_a_padded_head(T, Fu, Fi):
    c = cr.Cfg(1000, 16, 32, T, Fu, Fi)
    assert _lib.MODEL_TYPES["Caser"] == 8
    cfg = _lib.make_config(c.N, c.D, c.H, c.T, 1, Fu, Fi, "Caser")
    entries, n_w, n_reg = _lib.param_layout(cfg)
    Di, Du = 16 * Fi, 16 * Fu
    assert c.Dhead == 1 + 2 * Di + Du and c.Dhead % 2 == 1
    Dh = 4 + 2 * Di + Du                      # the library's head input: [h, 0, 0, 0 | v2 | target_item | target_user]
    # (name, the library's (rows, cols), init code, regularised)
    want = [("conv2d/kernel", (50, Di), "glorot_conv", True), ("conv2d/bias", (1,), "zeros", False),
            ("conv2d_1/kernel", (T, 1), "glorot_conv", True), ("conv2d_1/bias", (1,), "zeros", False),
            ("dense/kernel", (1, 1), "glorot", True), ("dense/bias", (1,), "zeros", False),
            ("bn1/gamma", (Dh,), "ones", True), ("bn1/beta", (Dh,), "zeros", True),
            ("fc1/kernel", (Dh, 200), "glorot", True), ("fc1/bias", (200,), "zeros", False),
            ("fc2/kernel", (200, 80), "glorot", True), ("fc2/bias", (80,), "zeros", False),
            ("fc3/kernel", (80, 1), "glorot", True), ("fc3/bias", (1,), "zeros", False)]
    spec = cr.param_spec(c)
    assert [e[0] for e in entries] == [w[0] for w in want] == [s[0] for s in spec]
    for e, (name, shape, init, reg), s in zip(entries, want, spec):
        assert ((e[2], e[3]) if e[3] else (e[2],)) == shape, name
        assert bool(e[4]) == reg == s[3] and e[5] == INIT[init], name
        assert e[1] % 4 == 0 and (e[1] < n_reg) == reg, name                      # 16-byte offsets, regularised tensors first
        # TF's variable has the same number of elements, the three pad rows of the head's variables aside
        pad = 3 * (e[3] or 1) if name in ("bn1/gamma", "bn1/beta", "fc1/kernel") else 0
        assert e[2] * (e[3] or 1) - pad == int(np.prod(s[1])), name
        # the init codes give TF's limits: code 3 = glorot with fan_in = fan_out = rows * cols
        if init == "glorot_conv":
            assert math.isclose(math.sqrt(6.0 / (2 * e[2] * e[3])), cr.glorot_limit(s[1]))
    assert math.isclose(cr.glorot_limit((1, 1)), math.sqrt(3.0)) and math.isclose(cr.glorot_limit((50, Di, 1, 1)), math.sqrt(6.0 / (100 * Di)))
    assert math.isclose(cr.glorot_limit((T, 1, 1, 1)), math.sqrt(6.0 / (2 * T)))
    spans = sorted((e[1], e[1] + e[2] * (e[3] or 1)) for e in entries)
    for a, b in zip(spans, spans[1:]):
        assert a[1] <= b[0]
    assert spans[-1][1] <= n_w
    # the regions the forward pass saves are readable, at the workspace's end; no recurrence region of any size
    B = 64
    total = _lib.workspace_layout(cfg, B).total_bytes // 4
    hw, ar, v = (_lib.workspace_field(cfg, B, f)[0] for f in ("caser_hwin", "caser_arg", "caser_v"))
    assert 0 < hw < ar < v and ar - hw >= B * (T - 49) and v - ar >= B and total - v >= B * Di and total - v < B * Di + 8
    g4r = _lib.make_config(c.N, c.D, c.H, c.T, 1, Fu, Fi, "GRU4Rec")
    assert total < _lib.workspace_layout(g4r, B).total_bytes // 4
    with pytest.raises(_lib.ScoreHipError):
        _lib.workspace_field(g4r, B, "caser_hwin")            # (a region of another model type)
    # user_seq rides as a one-element set per step: any other K is refused
    with pytest.raises(_lib.ScoreHipError):
        _lib.param_layout(_lib.make_config(c.N, c.D, c.H, c.T, 2, Fu, Fi, "Caser"))


def test_max_time_len_below_the_filter_height_is_refused():
    with pytest.raises(_lib.ScoreHipError):
        _lib.param_layout(_lib.make_config(1000, 16, 32, 49, 1, 3, 4, "Caser"))
    assert _lib.param_layout(_lib.make_config(1000, 16, 32, 50, 1, 3, 4, "Caser"))[1] > 0
    with pytest.raises(ValueError):
        cr.Cfg(1000, 16, 32, 49, 3, 4)
    from score_amd.model import Caser
    with pytest.raises(ValueError, match="50"):
        Caser(1000, 16, 32, 49, 3, 4)


def test_models_table_sharded_refusal_and_the_boundary_helpers():
    from score_amd import model
    assert model.MODELS["Caser"] is model.Caser and model.Caser.target_item_field == 3
    assert model.Caser.feed_spec is model.POINT_FEED and model.Caser.reads_length is False and model.GRU4Rec.reads_length is True
    from score_amd.dist import ShardedSCORE
    for name in ("Caser", "GRU4Rec"):
        with pytest.raises(ValueError, match=name):
            ShardedSCORE(100, 16, 32, 50, 1, 3, 4, comm=object(), model_type=name)
    # TF's arrays <-> the library's: pad rows 1..3 dropped / inserted as zeros, the conv kernels reshaped, the rest as it is
    c = cr.Cfg(100, 4, 8, 50, 1, 2)
    P = cr.init_params(c, 1)
    K = model.Caser
    internal = {"bn1/gamma": (c.Dhead + 3,), "bn1/beta": (c.Dhead + 3,), "fc1/kernel": (c.Dhead + 3, 200), "conv2d/kernel": (50, c.C),
                "conv2d_1/kernel": (c.T, 1)}
    for name, shape, _, _ in cr.param_spec(c):
        a = K._import(K, name, P[name], internal.get(name, shape))
        assert a.dtype == np.float32 and a.shape == internal.get(name, shape)
        if name in K.head_pad_vars:
            assert not a[1:4].any() and np.array_equal(a[0], P[name][0]) and np.array_equal(a[4:], P[name][1:])
        back = K._export(K, name, a)
        assert back.shape == shape and np.array_equal(back, P[name]), name


def test_inputs_of_the_gpu_tests_stay_within_the_kink_filters_cap():
    """every seed and shape tests/test_gpu_caser.py runs behind the kink filter, rebuilt from its own constructors and judged on
    the restatement alone (never on a GPU): the filter stays within max(2, B // 50) -- case() asserts that --, a sample
    remains, and where there is more than one window the batch chooses more than one position"""
    import test_gpu_caser as tg
    dropped = {}
    for shape in tg.SHAPES:
        c, P, b, kept = tg.case(*shape)
        B = shape[-1]
        dropped[shape] = B - kept.size
        assert 1 <= kept.size and B - kept.size <= cr.cap(B) == max(2, B // 50)
        with torch.no_grad():
            out = cr.forward(c, cr.to_torch(P), b)
        assert out["hwin"].shape == (kept.size, c.T - 49)
        if c.NW > 1:
            assert np.unique(out["arg"]).size > 1, shape
            assert out["window_margin_per_sample"].min() > cr.WINDOW_THR
    print(dropped)
    assert {s[1] - 49 for s in tg.SHAPES} == {1, 2, 8, 71} and {s[0] * s[3] for s in tg.SHAPES} >= {4, 64, 80, 32, 320}
    c, P, b, masks, kept = tg.dropout_case()
    assert 200 - kept.size <= 4
    # the cap itself holds, and the window filter is what takes a tied sample: a history of one item under three windows
    c = cr.Cfg(200, 4, 8, 52, 1, 1)
    b = cr.random_batch(np.random.default_rng(0), c, 4, min_length=1, max_length=1)
    assert (b["user_seq"] == b["user_seq"][:, :1]).all()
    with pytest.raises(AssertionError):
        cr.away_from_kinks(c, cr.init_params(c, 1), b)
