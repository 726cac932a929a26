"""GRU4Rec without a GPU: the parameter layout the library reports (host code: the library loads without a device) against
the variables of point_model.py:123-138 in TF creation order; the float64 restatement the GPU tests compare against
(tests/gru4rec_ref.py) against central finite differences; and the point-data loader (score_amd/pointdata.py) against the
batches the reference's own DataLoaderUserSeq produced (tests/golden/g7_point_loader.npz)."""
import os
import pickle

import numpy as np
import pytest
import torch

import gru4rec_ref as gr
from helpers import GOLDEN
from score_amd import _lib

INIT = {"zeros": 0, "ones": 1, "glorot": 2}


@pytest.mark.parametrize("Fu,Fi", [(3, 4), (1, 5), (1, 2)])
def test_param_layout_is_the_tf_variable_list(Fu, Fi):
    c = gr.Cfg(1000, 16, 32, 50, Fu, Fi)
    assert _lib.MODEL_TYPES["GRU4Rec"] == 7
    cfg = _lib.make_config(c.N, c.D, c.H, c.T, 1, Fu, Fi, "GRU4Rec")
    entries, n_w, n_reg = _lib.param_layout(cfg)
    Di, Du, H = 16 * Fi, 16 * Fu, 32
    Dh = H + Di + Du
    want = [("gru1/gru_cell/gates/kernel", (Di + H, 2 * H), "glorot", True), ("gru1/gru_cell/gates/bias", (2 * H,), "ones", False),
            ("gru1/gru_cell/candidate/kernel", (Di + H, H), "glorot", True), ("gru1/gru_cell/candidate/bias", (H,), "zeros", False),
            ("gru2/gru_cell/gates/kernel", (2 * H, 2 * H), "glorot", True), ("gru2/gru_cell/gates/bias", (2 * H,), "ones", False),
            ("gru2/gru_cell/candidate/kernel", (2 * H, H), "glorot", True), ("gru2/gru_cell/candidate/bias", (H,), "zeros", False),
            ("bn1/gamma", (Dh,), "ones", True), ("bn1/beta", (Dh,), "zeros", True),
            ("fc1/kernel", (Dh, 200), "glorot", True), ("fc1/bias", (200,), "zeros", False),
            ("fc2/kernel", (200, 80), "glorot", True), ("fc2/bias", (80,), "zeros", False),
            ("fc3/kernel", (80, 1), "glorot", True), ("fc3/bias", (1,), "zeros", False)]
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
    # both layers' saved outputs and gates are readable: index 0 = layer 1, 1 = layer 2
    for f in ("gru_out", "gates", "dxproj"):
        a, b = _lib.workspace_field(cfg, 64, f)
        assert 0 < a < b
    # user_seq rides as a one-element set per step: any other K is refused
    with pytest.raises(_lib.ScoreHipError):
        _lib.param_layout(_lib.make_config(c.N, c.D, c.H, c.T, 2, Fu, Fi, "GRU4Rec"))


def test_restatement_gradients_match_finite_differences():
    c = gr.Cfg(40, 4, 6, 5, 2, 3)
    rng = np.random.default_rng(5)
    P = gr.init_params(c, 9)
    for n in P:            # away from the initial values' symmetries (zero biases, ones)
        P[n] = (P[n] + 0.1 * rng.standard_normal(P[n].shape)).astype(np.float32)
    b = gr.random_batch(rng, c, 5)
    b["label"] = np.array([0, 1, 1, 0, 1], dtype=np.int32)
    b["user_seq_length"] = np.array([1, 5, 3, 9, 2], dtype=np.int32)          # (9: above T, behaves as T)
    b, _, _ = gr.away_from_relu_kinks(c, P, b, thr=1e-5)      # (the differences move a pre-activation by ~1e-6)
    lam = 1e-2
    _, g = gr.loss_and_grads(c, P, b, lam)
    P64 = {k: np.asarray(v, dtype=np.float64) for k, v in P.items()}

    def loss(Q):
        with torch.no_grad():
            return float(gr.forward(c, {k: torch.from_numpy(v) for k, v in Q.items()}, b, lam)["loss"])
    live = np.arange(c.T)[None, :] < b["user_seq_length"][:, None]
    touched = np.unique(np.concatenate([b["user_seq"][live].ravel(), b["target_user"].ravel(), b["target_item"].ravel()]))
    touched = touched[touched != 0]
    assert touched.size > 3
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
    # the masked row 0 and the rows no live position names get nothing (ids past a sample's length included)
    assert not g["emb_mtx"][0].any()
    others = np.setdiff1d(np.arange(1, c.N), touched)
    assert others.size and not g["emb_mtx"][others].any()


def _write_case(z, tag, d):
    paths = [os.path.join(str(d), n) for n in ("target.txt", "hist.txt", "ufeat.pkl", "ifeat.pkl")]
    for p, key in zip(paths[:2], ("target", "hist")):
        with open(p, "w") as f:
            f.write("".join(str(l) + "\n" for l in z["%s/%s" % (tag, key)]))
    out = paths[:2]
    for p, nm in zip(paths[2:], ("ufeat", "ifeat")):
        if "%s/%s_keys" % (tag, nm) in z.files:
            dct = {str(int(k)): [int(x) for x in row] for k, row in zip(z["%s/%s_keys" % (tag, nm)], z["%s/%s_rows" % (tag, nm)])}
            with open(p, "wb") as f:
                pickle.dump(dct, f)
            out.append(p)
        else:
            out.append(None)
    return out


def test_loader_yields_the_reference_loaders_batches(tmp_path):
    from score_amd.pointdata import DataLoaderUserSeq
    z = np.load(os.path.join(GOLDEN, "g7_point_loader.npz"))
    tags = [str(t) for t in z["tags"]]
    assert set(tags) == {"both", "nouser", "noitem", "none", "neg99"}
    seen_short = seen_equal = seen_long = False
    for tag in tags:
        d = tmp_path / tag
        d.mkdir()
        B, L, neg = [int(x) for x in z[tag + "/cfg"]]
        tf, hf, uf, itf = _write_case(z, tag, d)
        got = list(DataLoaderUserSeq(B, L, tf, hf, neg, uf, itf))
        assert len(got) == int(z[tag + "/n_batches"]) > 0, tag
        assert len(z[tag + "/target"]) % (B // (1 + neg)) != 0        # the target file ends inside a batch: that one is dropped
        for i, b in enumerate(got):
            assert len(b) == 5
            for nm, x in zip(gr.FEED, b):
                want = z["%s/b%d/%s" % (tag, i, nm)]
                assert isinstance(x, np.ndarray) and x.dtype == np.int32 and x.shape == want.shape, (tag, i, nm)
                assert np.array_equal(x, want), (tag, i, nm)
            ln = b[1]
            seen_short |= bool((ln < L).any()); seen_equal |= bool((ln == L).any()); seen_long |= bool((ln > L).any())
            short = np.nonzero(ln < L)[0]
            for s in short:      # padded by repeating the last item, not with 0
                assert (b[0][s, ln[s]:] == b[0][s, ln[s] - 1]).all() and b[0][s].min() > 0
    assert seen_short and seen_equal and seen_long


def test_loader_refuses_a_batch_size_that_is_no_multiple_of_the_samples_per_line(tmp_path):
    from score_amd.pointdata import DataLoaderUserSeq
    for n in ("t", "h"):
        (tmp_path / n).write_text("1,2,3\n")
    with pytest.raises(ValueError):
        DataLoaderUserSeq(5, 4, str(tmp_path / "t"), str(tmp_path / "h"), 1, None, None)
    assert len(list(DataLoaderUserSeq(2, 4, str(tmp_path / "t"), str(tmp_path / "h"), 1, None, None))) == 1


def test_models_table_and_sharded_refusal():
    from score_amd import model
    assert model.MODELS["GRU4Rec"] is model.GRU4Rec and model.GRU4Rec.target_item_field == 3
    assert [s[1] for s in model.POINT_FEED.slots if s[0] is not None] == ["user_seq", "target_user", "target_item", "label",
                                                                         "user_seq_length"]
    from score_amd.dist import ShardedSCORE
    with pytest.raises(ValueError, match="GRU4Rec"):
        ShardedSCORE(100, 16, 32, 50, 1, 3, 4, comm=object(), model_type="GRU4Rec")
