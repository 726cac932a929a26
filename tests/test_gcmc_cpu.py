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
