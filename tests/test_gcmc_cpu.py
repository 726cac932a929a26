"""GCMC without a GPU: the parameter layout the library reports (host code: the library loads without a device) against
the variables of slice_model.py:177-203 in TF creation order, and the float64 restatement the GPU tests compare against
(tests/gcmc_ref.py) against central finite differences."""
import numpy as np
import pytest
import torch

import gcmc_ref as gr
from helpers import random_batch
from score_amd import _lib

INIT = {"zeros": 0, "ones": 1, "glorot": 2}


@pytest.mark.parametrize("Fu,Fi", [(3, 4), (1, 5), (2, 2)])
def test_param_layout_is_the_tf_variable_list(Fu, Fi):
    c = gr.Cfg(1000, 16, 32, 11, 10, Fu, Fi)
    entries, n_w, n_reg = _lib.param_layout(_lib.make_config(*c.args, "GCMC"))
    Di, Du, H = 16 * Fi, 16 * Fu, 32
    want = [("dense/kernel", (Di, Di), "glorot", True), ("dense_1/kernel", (Du, Du), "glorot", True),
            ("dense_2/kernel", (Di, Di), "glorot", True), ("dense_3/kernel", (Du, Du), "glorot", True),
            ("gru1/gru_cell/gates/kernel", (Di + H, 2 * H), "glorot", True), ("gru1/gru_cell/gates/bias", (2 * H,), "ones", False),
            ("gru1/gru_cell/candidate/kernel", (Di + H, H), "glorot", True), ("gru1/gru_cell/candidate/bias", (H,), "zeros", False),
            ("gru2/gru_cell/gates/kernel", (Du + H, 2 * H), "glorot", True), ("gru2/gru_cell/gates/bias", (2 * H,), "ones", False),
            ("gru2/gru_cell/candidate/kernel", (Du + H, H), "glorot", True), ("gru2/gru_cell/candidate/bias", (H,), "zeros", False),
            ("dense_4/kernel", (H, H), "glorot", True), ("dense_5/kernel", (H, H), "glorot", True)]
    assert want == gr.param_spec(c)
    assert [e[0] for e in entries] == [w[0] for w in want]
    for e, (name, shape, init, reg) in zip(entries, want):
        assert ((e[2], e[3]) if e[3] else (e[2],)) == shape, name
        assert bool(e[4]) == reg and e[5] == INIT[init], name
        assert e[1] % 4 == 0 and (e[1] < n_reg) == reg, name
    spans = sorted((e[1], e[1] + e[2] * (e[3] or 1)) for e in entries)
    for a, b in zip(spans, spans[1:]):
        assert a[1] <= b[0]
    assert spans[-1][1] <= n_w
    # the activations the GPU tests read have workspace regions of their own; other model types have none
    for f in ("gcmc_a", "gcmc_z", "gcmc_pn", "gcmc_g", "gcmc_gu"):
        a, b = _lib.workspace_field(_lib.make_config(*c.args, "GCMC"), 64, f)
        assert a > 0
    with pytest.raises(_lib.ScoreHipError):
        _lib.workspace_field(_lib.make_config(*c.args, "RRN"), 64, "gcmc_a")


def test_restatement_gradients_match_finite_differences():
    c = gr.Cfg(40, 4, 6, 4, 3, 2, 3)
    rng = np.random.default_rng(5)
    P = gr.init_params(c, 9)
    for n in P:            # away from the initial values' symmetries (zero biases, ones)
        P[n] = (P[n] + 0.1 * rng.standard_normal(P[n].shape)).astype(np.float32)
    b = random_batch(rng, c, 5)
    b["label"] = np.array([0, 1, 1, 0, 1], dtype=np.int32)
    b, _ = gr.away_from_relu_kinks(c, P, b, thr=1e-3)
    lam = 1e-2
    _, g = gr.loss_and_grads(c, P, b, lam)
    P64 = {k: np.asarray(v, dtype=np.float64) for k, v in P.items()}

    def loss(Q):
        with torch.no_grad():
            return float(gr.forward(c, {k: torch.from_numpy(v) for k, v in Q.items()}, b, lam)["loss"])
    touched = np.unique(np.concatenate([b["user_1hop"].ravel(), b["item_1hop"].ravel()]))
    touched = touched[touched != 0]
    assert touched.size > 3
    h = 1e-6
    for name in P64:
        flat = P64[name].reshape(-1)
        if name == "emb_mtx":
            idx = np.concatenate([touched[:, None] * c.D + np.arange(c.D)[None, :]]).ravel()
        else:
            idx = np.arange(flat.size)
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
    # the masked row 0 and the rows only the unused tensors name get nothing
    assert not g["emb_mtx"][0].any()
    others = np.setdiff1d(np.arange(1, c.N), touched)
    assert not g["emb_mtx"][others].any()


def test_inputs_of_the_gpu_edge_tests_have_the_properties_they_are_run_for():
    """tests/test_gpu_gcmc.py's new inputs, rebuilt from the same constructors (tests/baseline_cases.py) and judged on the
    float64 restatement alone: each assertion is the property whose absence made the older inputs blind."""
    import baseline_cases as bc
    # workgroup edges: the kink filter takes nothing, and B sits one below / one above a multiple of the head kernels' share
    seen = {}
    for D, H, T, K, Fu, Fi, B, seed in bc.GCMC_EDGES:
        c, P, b, kept, _ = bc.gcmc_case(D, H, T, K, Fu, Fi, B, seed)
        SB = bc.gcmc_sb(H)
        assert len(b["label"]) == B == kept.size and (B == 1 or B % SB in (1, SB - 1))
        seen.setdefault(H, set()).add((B > SB) - (B < SB))
    assert seen == {32: {-1, 1}, 48: {-1, 1}, 128: {-1, 1}, 256: {-1, 1}} and [bc.gcmc_sb(h) for h in (32, 48, 128, 256)] == [64, 40, 16, 8]
    assert any(s[6] > 4 * bc.gcmc_sb(s[1]) for s in bc.GCMC_EDGES)                 # more than two workgroups, ragged
    for D, H, T, K, Fu, Fi, B, seed in bc.GCMC_ODD_H:
        c, P, b, kept, _ = bc.gcmc_case(D, H, T, K, Fu, Fi, B, seed)
        assert kept.size == B and H % 16 != 0 and H <= 256 and D % 4 == 0
        _lib.param_layout(_lib.make_config(*c.args, "GCMC"))                       # the configuration check takes the shape
    assert [s[1] % 4 for s in bc.GCMC_ODD_H] == [0, 2]
    # length 0: zero final states, y = 1 / 2, finite gradients, nothing on the rows only those samples name
    c, P, b, kept, B = bc.gcmc_case(*bc.GCMC_ZERO_LEN, zero_len=True, exact=False)
    zero = np.nonzero(b["length"] == 0)[0]
    assert B - kept.size <= bc.cap(B) and zero.size == 3 and zero[0] == 0 and zero[-1] == kept.size - 1
    assert np.unique(b["length"]).size > 4                                         # (the rest: ragged)
    out, g = gr.loss_and_grads(c, P, b, 0.0)
    assert not out["h_u"].detach().numpy()[zero].any() and not out["h_i"].detach().numpy()[zero].any()
    assert np.array_equal(out["y_pred"].detach().numpy()[zero], [0.5] * 3)
    assert np.isfinite(float(out["loss"].detach())) and all(np.isfinite(v).all() for v in g.values())
    fresh = np.arange(c.N - bc.FRESH, c.N)
    live = b["length"] > 0
    assert np.isin(b["user_1hop"][zero], fresh).all() and np.isin(b["item_1hop"][zero], fresh).all()
    assert not np.isin(b["user_1hop"][live], fresh).any() and not np.isin(b["item_1hop"][live], fresh).any()
    assert not g["emb_mtx"][fresh].any() and np.abs(g["emb_mtx"]).max() > 0
    # saturation: both recurrences' states reach 1; the head stays where float64 is a fair yardstick and far from exp's overflow
    for shape, scale in bc.GCMC_SATURATED:
        c, P, b, kept, B = bc.gcmc_case(*shape, scale=scale, exact=False)
        assert B - kept.size <= bc.cap(B)
        with torch.no_grad():
            Pt = gr.to_torch(P)
            out = gr.forward(c, Pt, b)
            a = ((out["h_i"] @ Pt["dense_4/kernel"]) * out["h_u"]).sum(1)
            cc = ((out["h_i"] @ Pt["dense_5/kernel"]) * out["h_u"]).sum(1)
        y = out["y_pred"].numpy()
        assert float(out["h_u"].abs().max()) > 0.999 and float(out["h_i"].abs().max()) > 0.999, shape
        assert 1e-3 <= y.min() and y.max() <= 1 - 1e-3 and float(a.abs().max()) < 80 and float(cc.abs().max()) < 80, (shape, y.min(), y.max())
    # the trajectory: every batch has the listed size and longest sample, and B and TA each fall (alone and together) on the way
    c = gr.Cfg(20011, 16, 32, 11, 10, 3, 4)
    bs = bc.gcmc_trajectory(c)
    assert [(len(b["label"]), int(b["length"].max())) for b in bs] == [(B, ml or c.T) for B, ml in bc.GCMC_TRAJECTORY]
    ta = [ml or c.T for _, ml in bc.GCMC_TRAJECTORY]
    falls = {(bc.GCMC_TRAJECTORY[i + 1][0] < bc.GCMC_TRAJECTORY[i][0], ta[i + 1] < ta[i]) for i in range(len(ta) - 1)}
    assert {(True, True), (True, False), (False, True)} <= falls and len(bs) >= 12 and min(b["length"].min() for b in bs) >= 1


def test_kink_filter_takes_no_more_than_its_cap_from_the_committed_inputs():
    """the inputs of the older parity test under the tighter cap max(2, B // 50): what the restatement alone drops (counted
    here, never on a GPU): 0, 2, 0, 0, 0 of the five shapes"""
    dropped = []
    for D, H, T, K, Fu, Fi, B in [(16, 32, 11, 10, 3, 4, 200), (16, 32, 40, 10, 1, 5, 64), (8, 48, 5, 6, 2, 2, 40), (64, 128, 6, 10, 3, 4, 96),
                                  (32, 256, 4, 4, 2, 2, 32)]:
        c = gr.Cfg(3000, D, H, T, K, Fu, Fi)
        b = random_batch(np.random.default_rng(D + H + T), c, B)
        b["label"] = (np.arange(B) % 2).astype(np.int32)
        _, kept = gr.away_from_relu_kinks(c, gr.init_params(c, 3), b, max_dropped=max(2, B // 50))
        dropped.append(B - kept.size)
    assert dropped == [0, 2, 0, 0, 0], dropped
    with pytest.raises(AssertionError):
        gr.away_from_relu_kinks(c, gr.init_params(c, 3), b, thr=0.05, max_dropped=2)
