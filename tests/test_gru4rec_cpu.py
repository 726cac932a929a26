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


def _transitions(traj, T):
    """(B falls, TA falls) pairs seen between consecutive steps of a (B, longest or None) list"""
    ta = [T if ml is None else ml for _, ml in traj]
    return {(traj[i + 1][0] < traj[i][0], ta[i + 1] < ta[i]) for i in range(len(traj) - 1)}


def test_inputs_of_the_gpu_edge_tests_have_the_properties_they_are_run_for():
    """tests/test_gpu_gru4rec.py's new inputs, rebuilt from the same constructors (tests/baseline_cases.py) and judged on the
    float64 restatement alone: each assertion is the property whose absence made the older inputs blind."""
    import baseline_cases as bc
    # short batches: the longest sample is below T; the kink filter takes at most cap(B); the batch that remains sits where it
    # was meant to against the stacked kernel's 16 samples per workgroup
    sizes = {}
    for D, H, T, Fu, Fi, B, ML, seed in bc.G4R_SHORT:
        c, P, b, kept, _ = bc.g4r_case(D, H, T, Fu, Fi, B, ML, seed)
        Bk, longest = len(b["label"]), int(b["user_seq_length"].max())
        assert 1 <= longest <= ML < T and int(b["user_seq_length"].min()) >= 1
        assert B - Bk <= bc.cap(B) and (Bk == B or B > 17)
        assert Bk == B if B % 16 == 0 else Bk % 16 != 0            # a full last workgroup only where one was meant
        sizes.setdefault(H, set()).add(Bk)
    stacked = set().union(*(v for h, v in sizes.items() if h in (16, 32, 64)))
    assert {1, 15, 16, 17} <= stacked and any(16 < x < 32 for x in stacked) and 48 in sizes         # (48: the composed form only)
    assert any(s[6] == 1 for s in bc.G4R_SHORT)                    # layer 2 one step behind a one-step layer 1
    # length 0: three samples, first / middle / last after the filter; zero outputs and final state; finite loss and gradients;
    # nothing on the rows only they name
    c, P, b, kept, B = bc.g4r_case(*bc.G4R_ZERO_LEN, zero_len=True)
    zero = np.nonzero(b["user_seq_length"] == 0)[0]
    assert B - len(kept) <= bc.cap(B) and zero.size == 3 and zero[0] == 0 and zero[-1] == len(kept) - 1
    assert int(b["user_seq_length"].max()) > 1 and np.unique(b["user_seq_length"]).size > 5           # (the rest: ragged)
    out, g = gr.loss_and_grads(c, P, b, 0.0)
    for k in ("o1", "o2", "h2"):
        assert not out[k].detach().numpy()[zero].any(), k
    assert np.isfinite(float(out["loss"].detach())) and all(np.isfinite(v).all() for v in g.values())
    fresh = np.arange(c.N - bc.FRESH, c.N)
    assert np.isin(b["user_seq"][zero], fresh).all() and not np.isin(b["user_seq"][b["user_seq_length"] > 0], fresh).any()
    assert not np.isin(b["target_user"], fresh).any() and not np.isin(b["target_item"], fresh).any()
    assert not g["emb_mtx"][fresh].any() and np.abs(g["emb_mtx"]).max() > 0
    # saturation: the recurrences' states reach 1, the predictions stay where float64 is a fair yardstick for the loss
    for shape, scale in bc.G4R_SATURATED:
        c, P, b, kept, B = bc.g4r_case(*shape, scale=scale)
        assert B - len(kept) <= bc.cap(B)
        with torch.no_grad():
            out = gr.forward(c, gr.to_torch(P), b)
        y = out["y_pred"].numpy()
        assert float(out["o1"].abs().max()) > 0.999 and 1e-3 <= y.min() and y.max() <= 1 - 1e-3, (shape, y.min(), y.max())
    # the trajectory: every batch has the listed size and longest sample, and B and TA each fall (alone and together) on the way
    c = gr.Cfg(20011, 16, 32, 50, 3, 4)
    bs = bc.g4r_trajectory(c)
    assert [(len(b["label"]), int(b["user_seq_length"].max())) for b in bs] == [(B, ml or c.T) for B, ml in bc.G4R_TRAJECTORY]
    assert {(True, True), (True, False), (False, True)} <= _transitions(bc.G4R_TRAJECTORY, c.T)
    assert len(bs) >= 12 and (1, 1) in bc.G4R_TRAJECTORY


def test_kink_filter_takes_no_more_than_its_cap_from_the_committed_inputs():
    """the inputs of the older parity tests under the tighter cap max(2, B // 50): what the restatement alone drops (counted
    here, never on a GPU): 1, 0, 1, 1, 0, 1, 0, 0 of the eight shapes"""
    import test_gpu_gru4rec as tg
    dropped = []
    for D, H, T, Fu, Fi, B in tg.SHAPES:
        c = gr.Cfg(3000, D, H, T, Fu, Fi)
        P = gr.init_params(c, 3)
        b = tg._batches(c, B, 1, D + H + T)[0]
        b["label"] = (np.arange(B) % 2).astype(np.int32)
        _, _, kept = gr.away_from_relu_kinks(c, P, b, max_dropped=max(2, B // 50))
        dropped.append(B - kept.size)
    assert dropped == [1, 0, 1, 1, 0, 1, 0, 0], dropped
    c = gr.Cfg(3000, *tg.TMALL)
    b = tg._batches(c, 200, 1, 21)[0]
    rng = np.random.default_rng(22)
    masks = [(rng.random((200, 200)) < 0.8).astype(np.uint8), (rng.random((200, 80)) < 0.8).astype(np.uint8)]
    _, _, kept = gr.away_from_relu_kinks(c, gr.init_params(c, 3), b, keep_prob=0.8, dropout_masks=masks, max_dropped=4)
    # the argument itself: the cap holds, the default is the old quarter
    with pytest.raises(AssertionError):
        gr.away_from_relu_kinks(c, gr.init_params(c, 3), b, thr=0.05, max_dropped=4)
    gr.away_from_relu_kinks(c, gr.init_params(c, 3), b, thr=1e-4)
