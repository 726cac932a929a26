"""DELF without a GPU: the float64 restatement the GPU tests compare against (tests/delf_ref.py) against central finite
differences, with a sample longer than T and one of length 0; the parameter layout the library reports (host code: the library
loads without a device) against the variables of point_model.py:200-249 in TF creation order; the width limit; the models
table, feed spec and sharded refusal; the restated dual-sequence loader against the batches the reference's own
DataLoaderDualSeq produced (tests/golden/g8_dual_loader.npz); and the inputs of the GPU tests judged on the restatement alone."""
import os
import pickle

import numpy as np
import pytest
import torch

import delf_cases as dc
import delf_ref as dr
from score_amd import _lib
from score_amd.model import DELF, DUAL_FEED            # (the feature under test: nothing here runs without it)
from score_amd.pointdata import DataLoaderDualSeq

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INIT = {"zeros": 0, "ones": 1, "glorot": 2}


def test_restatement_gradients_match_finite_differences():
    D, T, Fu, Fi, B = 4, 5, 2, 1, 6
    c = dr.Cfg(300, D, 7, T, Fu, Fi)
    rng = np.random.default_rng(5)
    P = dr.init_params(c, 9)
    for n in P:            # away from the initial values' symmetries (zero biases)
        P[n] = (P[n] + 0.1 * rng.standard_normal(P[n].shape)).astype(np.float32)
    b = dr.random_batch(rng, c, B)
    b["user_seq_length"] = np.array([9, 0, 3, 5, 1, 2], dtype=np.int32)       # longer than T, all masked, ...
    b["item_seq_length"] = np.array([2, 4, 0, 12, 5, 1], dtype=np.int32)
    b["label"] = np.array([0, 1, 1, 0, 1, 0], dtype=np.int32)
    b, kept = dr.away_from_kinks(c, P, b)                     # (the differences move a pre-activation by ~1e-6)
    assert (b["user_seq_length"] > T).any() and (b["user_seq_length"] == 0).any() and (b["item_seq_length"] == 0).any()
    lam = 1e-2
    out, g = dr.loss_and_grads(c, P, b, lam)
    P64 = {k: np.asarray(v, dtype=np.float64) for k, v in P.items()}

    def loss(Q):
        with torch.no_grad():
            return float(dr.forward(c, {k: torch.from_numpy(v) for k, v in Q.items()}, b, lam)["loss"])
    touched = np.unique(np.concatenate([b[k].ravel() for k in ("user_seq", "item_seq", "target_user", "target_item")]))
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
        assert np.abs(num).max() > 0, name
        assert np.abs(ana - num).max() <= 1e-6 + 1e-5 * np.abs(num).max(), (name, np.abs(ana - num).max())
    assert not g["emb_mtx"][0].any()
    # the masks: a length >= T is all positions; a length 0 is uniform weights over all T; masked positions weigh exactly 0
    au, ai = out["att_user"].detach().numpy(), out["att_item"].detach().numpy()
    for a, ln in ((au, b["user_seq_length"]), (ai, b["item_seq_length"])):
        for i in range(len(ln)):
            if ln[i] <= 0:
                assert np.array_equal(a[i], np.full(T, 1.0 / T))
            else:
                assert (a[i, min(ln[i], T):] == 0).all() and (a[i, :min(ln[i], T)] > 0).all()
            assert abs(a[i].sum() - 1) < 1e-12


@pytest.mark.parametrize("T,Fu,Fi", [(50, 3, 4), (50, 1, 5), (7, 1, 2)])
def test_param_layout_is_the_tf_variable_list(T, Fu, Fi):
    c = dr.Cfg(1000, 16, 32, T, Fu, Fi)
    assert _lib.MODEL_TYPES["DELF"] == 9
    cfg = _lib.make_config(c.N, c.D, c.H, c.T, 1, Fu, Fi, "DELF")
    entries, n_w, n_reg = _lib.param_layout(cfg)
    Ci, Cu = 16 * Fi, 16 * Fu
    kernels = [(Ci, Ci), (Cu, Cu), (Cu + Ci, 10), (10, 4), (Ci + Cu, 10), (10, 4), (2 * Cu, 10), (10, 4), (2 * Ci, 10), (10, 4), (4, 1)]
    want = []
    for i, sh in enumerate(kernels):
        nm = "dense" if i == 0 else "dense_%d" % i
        want += [(nm + "/kernel", sh, "glorot", True), (nm + "/bias", (sh[1],), "zeros", False)]
    spec = dr.param_spec(c)
    assert len(entries) == 22
    assert [e[0] for e in entries] == [w[0] for w in want] == [s[0] for s in spec]
    for e, (name, shape, init, reg), s in zip(entries, want, spec):
        assert ((e[2], e[3]) if e[3] else (e[2],)) == shape == tuple(s[1]), name
        assert bool(e[4]) == reg == s[3] and e[5] == INIT[init] == INIT[s[2]], name
        assert e[1] % 4 == 0 and (e[1] < n_reg) == reg, name                      # 16-byte offsets, regularised tensors first
    spans = sorted((e[1], e[1] + e[2] * (e[3] or 1)) for e in entries)
    for a, b in zip(spans, spans[1:]):
        assert a[1] <= b[0]
    assert spans[-1][1] <= n_w
    # the regions the passes save are readable, per side where they are per side
    B = 64
    total = _lib.workspace_layout(cfg, B).total_bytes // 4
    for f, n0, n1 in (("delf_key", B * T * Ci, B * T * Cu), ("delf_att", B * T, B * T), ("delf_rep", B * Ci, B * Cu),
                      ("delf_ds", B * T, B * T), ("delf_dpre", B * T * Ci, B * T * Cu)):
        a, b2 = _lib.workspace_field(cfg, B, f)
        assert 0 < a and 0 < b2 and a + n0 <= total and b2 + n1 <= total and (b2 >= a + n0 or a >= b2 + n1), f
    for f in ("delf_act", "delf_dact"):
        assert 0 < _lib.workspace_field(cfg, B, f)[0] <= total - B * 64
    g4r = _lib.make_config(c.N, c.D, c.H, c.T, 1, Fu, Fi, "GRU4Rec")
    with pytest.raises(_lib.ScoreHipError):
        _lib.workspace_field(g4r, B, "delf_att")             # (a region of another model type)
    with pytest.raises(_lib.ScoreHipError):
        _lib.param_layout(_lib.make_config(c.N, c.D, c.H, c.T, 2, Fu, Fi, "DELF"))      # obj_per_time_slice must be 1


def test_width_limit():
    ok = _lib.make_config(1000, 32, 32, 50, 1, 4, 4, "DELF")                 # 128 on both sides
    assert len(_lib.param_layout(ok)[0]) == 22
    for D, Fu, Fi in ((44, 1, 3), (44, 3, 1), (4, 33, 1)):                   # 132 on the item side, on the user side, again
        with pytest.raises(_lib.ScoreHipError):
            _lib.param_layout(_lib.make_config(1000, D, 32, 50, 1, Fu, Fi, "DELF"))
    # the other point models are not limited by it
    assert _lib.param_layout(_lib.make_config(1000, 44, 32, 50, 1, 1, 3, "GRU4Rec"))[0]


def test_batch_struct_has_length2_at_its_end():
    import ctypes as C
    names = [f[0] for f in _lib.Batch._fields_]
    assert names[-1] == "length2" and names[:10] == ["user_1hop", "user_2hop", "item_1hop", "item_2hop", "target_user",
                                                     "target_item", "label", "length", "B", "active_slices"]
    b = _lib.Batch(1, 2, 3, 4, 5, 6, 7, 8, 9, 10)           # the positional form every other caller uses
    assert b.active_slices == 10 and b.length2 is None
    out = (C.c_int64 * 32)()
    lib = _lib.load()
    assert lib.score_abi_struct_sizes(out, 32) == 14 and out[3] == C.sizeof(_lib.Batch) == 80


def test_models_table_feed_spec_and_sharded_refusal():
    from score_amd import model
    assert model.MODELS["DELF"] is model.DELF and model.DELF.model_type == "DELF" and issubclass(model.DELF, model.GRU4Rec)
    assert model.DELF.target_item_field == 5 and model.DELF.feed_spec is model.DUAL_FEED and model.DUAL_FEED.n == 7
    by_pos = sorted((s[0], s[1]) for s in model.DUAL_FEED.slots if s[0] is not None)
    assert [n for _, n in by_pos] == list(dr.FEED) and [p for p, _ in by_pos] == list(range(7))
    # which tensor of score_batch_t a field rides in: user_1hop, item_1hop, the targets, label, length, and the ninth: length2
    assert [s[1] for s in model.DUAL_FEED.slots] == ["user_seq", None, "item_seq", None, "target_user", "target_item", "label",
                                                      "user_seq_length", "item_seq_length"]
    cfg = _lib.make_config(100, 16, 32, 50, 1, 3, 4, "DELF")
    assert model.DUAL_FEED.device_shapes(cfg, 6)[8] == (6,) and len(model.DUAL_FEED.device_shapes(cfg, 6)) == 9
    # every other model's flat batch is what it was: eight tensors
    assert len(model.POINT_FEED.device_shapes(cfg, 6)) == len(model.SLICE_FEED.device_shapes(cfg, 6)) == 8
    assert model.flat_batch_size(model.POINT_FEED.device_shapes(cfg, 6)) == model.flat_batch_size(model.batch_shapes(cfg, 6))

    class M(object):
        pass
    m = M()
    m.cfg = cfg
    assert model.active_slices(m, 7, 1) == 7 and model.active_slices(m, 7, 0) == 0 and model.active_slices(m, 70, 3) == 0
    assert model.active_slices(m, 7) == 7
    from score_amd.dist import ShardedSCORE
    with pytest.raises(ValueError, match="DELF"):
        ShardedSCORE(100, 16, 32, 50, 1, 3, 4, comm=object(), model_type="DELF")


def _write_case(z, tag, d):
    paths = [str(d / n) for n in ("target.txt", "hist.txt", "ihist.txt", "ufeat.pkl", "ifeat.pkl")]
    for p, key in zip(paths[:3], ("target", "hist", "ihist")):
        with open(p, "w") as f:
            f.write("".join(str(l) + "\n" for l in z["%s/%s" % (tag, key)]))
    out = paths[:3]
    for p, nm in zip(paths[3:], ("ufeat", "ifeat")):
        if "%s/%s_keys" % (tag, nm) in z.files:
            dct = {str(int(k)): [int(x) for x in row] for k, row in zip(z["%s/%s_keys" % (tag, nm)], z["%s/%s_rows" % (tag, nm)])}
            with open(p, "wb") as f:
                pickle.dump(dct, f)
            out.append(p)
        else:
            out.append(None)
    return out


def test_dual_loader_yields_the_reference_loaders_batches(tmp_path):
    z = np.load(os.path.join(GOLDEN, "g8_dual_loader.npz"))
    tags = [str(t) for t in z["tags"]]
    assert set(tags) == {"both", "nouser", "noitem", "none", "neg99"}
    seen = {(side, k): False for side in (1, 3) for k in ("short", "equal", "long")}
    quirk = 0
    for tag in tags:
        d = tmp_path / tag
        d.mkdir()
        B, L, neg = [int(x) for x in z[tag + "/cfg"]]
        tf, hf, ihf, uf, itf = _write_case(z, tag, d)
        got = list(DataLoaderDualSeq(B, L, tf, hf, ihf, neg, uf, itf))
        assert len(got) == int(z[tag + "/n_batches"]) > 0, tag
        assert len(z[tag + "/target"]) % (B // (1 + neg)) != 0        # the target file ends inside a batch: that one is dropped
        lines_per_batch = B // (1 + neg)
        for i, b in enumerate(got):
            assert len(b) == 7
            for nm, x in zip(dr.FEED, b):
                want = z["%s/b%d/%s" % (tag, i, nm)]
                assert isinstance(x, np.ndarray) and x.dtype == np.int32 and x.shape == want.shape, (tag, i, nm)
                assert np.array_equal(x, want), (tag, i, nm)
            for side in (1, 3):
                ln = b[side]
                seen[(side, "short")] |= bool((ln < L).any()); seen[(side, "equal")] |= bool((ln == L).any())
                seen[(side, "long")] |= bool((ln > L).any())
                for s in np.nonzero(ln < L)[0]:      # padded by repeating the last id, not with 0
                    assert (b[side - 1][s, ln[s]:] == b[side - 1][s, ln[s] - 1]).all() and b[side - 1][s].min() > 0
            # target_user: the last id of the line's last item sequence, not the target line's user
            for j in range(lines_per_batch):
                line = i * lines_per_batch + j
                tline = str(z[tag + "/target"][line]).split(",")
                last = str(z[tag + "/ihist"][line]).split("\t")[-1].split(",")[-1]
                rows = b[4][j * (1 + neg):(j + 1) * (1 + neg), 0]
                assert (rows == int(last)).all(), (tag, line)
                quirk += int(last) != int(tline[0])
    assert all(seen.values()), seen
    assert quirk > 10          # (the fixture does tell the two readings apart)


def test_dual_loader_refuses_a_batch_size_that_is_no_multiple_of_the_samples_per_line(tmp_path):
    (tmp_path / "t").write_text("1,2,3\n")
    (tmp_path / "h").write_text("1,2,3\n")
    (tmp_path / "i").write_text("4,5\t6\n")
    args = (str(tmp_path / "t"), str(tmp_path / "h"), str(tmp_path / "i"))
    with pytest.raises(ValueError):
        DataLoaderDualSeq(5, 4, *args, 1, None, None)
    (b,) = list(DataLoaderDualSeq(2, 4, *args, 1, None, None))
    assert b[2].tolist() == [[[4], [5], [5], [5]], [[6], [6], [6], [6]]] and b[3].tolist() == [2, 1] and b[4].tolist() == [[6], [6]]


@pytest.mark.parametrize("D,T,Fu,Fi,B", list(dc.SHAPES))
def test_inputs_of_the_gpu_tests_stay_inside_the_kink_cap(D, T, Fu, Fi, B):
    c, P, b, kept = dc.case(D, T, Fu, Fi, B)        # (away_from_kinks asserts the cap)
    assert 1 <= kept.size and B - kept.size <= dr.cap(B)
    ul, il = b["user_seq_length"], b["item_seq_length"]
    if (D, T, Fu, Fi, B) == (4, 3, 2, 1, 3):
        assert kept.size == 3 and sorted(ul.tolist()) == [0, 2, 7] and sorted(il.tolist()) == [0, 2, 7]
    if (D, T, Fu, Fi, B) == (16, 7, 3, 4, 33):
        assert max(ul.max(), il.max()) <= 5 and min(ul.min(), il.min()) >= 1
    if T >= 50:
        assert (ul > T).any() and (ul < T).any() and (il > T).any() and (il < T).any()
    with torch.no_grad():
        out = dr.forward(c, dr.to_torch(P), b)
    assert np.isfinite(out["y_pred"].numpy()).all()
