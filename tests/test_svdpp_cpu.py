"""SVD++ without a GPU: the float64 restatement the GPU tests compare against (tests/svdpp_ref.py) against finite differences and
against numpy's matrix 1-norm; the parameter layout the library reports (host code: the library loads without a device) against
the variables of point_model.py:167-198 in TF creation order, and the layouts of model types 0-10 against what they were before
model type 11 existed; the models table, the feed spec and the sharded refusal; a zero length; and the inputs of the GPU tests
judged on the restatement alone."""
import zlib

import numpy as np
import pytest
import torch

import svdpp_cases as sc
import svdpp_ref as sr
from score_amd import _lib
from score_amd.model import GRU4Rec, POINT_FEED, SVDpp          # (the feature under test: nothing here runs without it)


def _small():
    c = sr.Cfg(60, 4, 8, 5, 2, 3)
    P = sr.init_params(c, 9)
    rng = np.random.default_rng(5)
    b = sr.random_batch(rng, c, 6, max_length=9)
    b["user_seq_length"] = np.array([9, 1, 3, 5, 2, 4], dtype=np.int32)       # longer than T, one live row, ...
    b["user_seq"][2, 1] = 0                                                   # a live row of the dummy id: s_t = 0 exactly
    b["label"] = np.array([0, 1, 1, 0, 1, 0], dtype=np.int32)
    return c, P, b


def test_restatement_against_finite_differences():
    c, P, b = _small()
    assert sr.kink_free(c, P, b).all()
    lam = 1e-2
    out, g = sr.loss_and_grads(c, P, b, lam)

    def loss_at(name, idx, delta):
        Q = {k: np.array(v, dtype=np.float64) for k, v in P.items()}
        Q[name][idx] += delta
        with torch.no_grad():
            return float(sr.forward(c, sr.to_torch(Q), b, lam)["loss"])

    eps = 1e-6
    # every scalar weight
    for name, _, _, _ in sr.param_spec(c):
        fd = (loss_at(name, (), eps) - loss_at(name, (), -eps)) / (2 * eps)
        assert g[name].shape == () and abs(fd - float(g[name])) < 1e-7 * max(1.0, abs(fd)), (name, fd, float(g[name]))
        assert abs(float(g[name])) > 0
    # a sample of table rows: history rows (live and masked), target rows, and the dummy row
    rows = sorted(set([int(b["user_seq"][0, 0, 0]), int(b["user_seq"][1, 0, 1]), int(b["user_seq"][1, 4, 0]), int(b["user_seq"][3, 4, 2]),
                       int(b["target_user"][2, 1]), int(b["target_item"][4, 0]), 0]))
    seen = 0
    for r in rows:
        for d in range(c.D):
            fd = (loss_at("emb_mtx", (r, d), eps) - loss_at("emb_mtx", (r, d), -eps)) / (2 * eps)
            assert abs(fd - g["emb_mtx"][r, d]) < 1e-7 * max(1.0, abs(fd)), (r, d, fd, g["emb_mtx"][r, d])
            seen += fd != 0
    assert seen > c.D and not g["emb_mtx"][0].any()
    # the l2 term: lam * w on every scalar, nothing on the table
    _, g0 = sr.loss_and_grads(c, P, b, 0.0)
    for name, _, _, _ in sr.param_spec(c):
        assert abs(float(g[name]) - float(g0[name]) - lam * float(P[name])) < 1e-12
    assert np.array_equal(g["emb_mtx"], g0["emb_mtx"])


def test_the_norm_is_numpys_matrix_one_norm_on_ragged_lengths():
    c = sr.Cfg(300, 8, 8, 7, 2, 3)
    P = sr.init_params(c, 4)
    b = sc.batches(c, 12, 1, 6)[0]
    b["user_seq_length"] = np.array([1, 2, 3, 4, 5, 6, 7, 8, 20, 1, 3, 7], dtype=np.int32)
    with torch.no_grad():
        out = sr.forward(c, sr.to_torch(P), b)
    s, n = out["s"].numpy(), out["n"].numpy()
    want = np.linalg.norm(s, 1, axis=(1, 2))
    # (two float64 sums of at most T = 7 terms in different orders: within 7 * 2^-53 of each other, relatively)
    assert np.allclose(n, want, rtol=1e-14, atol=0)
    assert np.allclose(want, np.abs(s).sum(1).max(1), rtol=1e-14, atol=0)
    assert (want < np.abs(s).sum((1, 2))).all()               # not the sum of all absolute values
    for i, ln in enumerate(b["user_seq_length"]):
        assert not s[i, ln:].any() and s[i, :min(ln, c.T)].any(1).all()
    assert np.allclose(out["q"].numpy(), s.sum(1) / np.sqrt(want)[:, None], rtol=1e-15, atol=0)


def test_reduce_max_shares_the_gradient_among_ties_and_sign_zero_is_zero():
    x = torch.tensor([[1.0, 3.0, 3.0, 0.0]], dtype=torch.float64, requires_grad=True)
    x.abs().amax(1).sum().backward()
    assert x.grad.tolist() == [[0.0, 0.5, 0.5, 0.0]]
    z = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    z.abs().sum().backward()
    assert not z.grad.any()


@pytest.mark.parametrize("T,Fu,Fi", [(50, 3, 4), (50, 1, 5), (7, 1, 1), (9, 8, 8)])
def test_param_layout_is_the_tf_variable_list(T, Fu, Fi):
    c = sr.Cfg(1000, 16, 32, T, Fu, Fi)
    assert _lib.MODEL_TYPES["SVDpp"] == 11
    cfg = _lib.make_config(c.N, c.D, c.H, c.T, 1, Fu, Fi, "SVDpp")
    entries, n_w, n_reg = _lib.param_layout(cfg)
    want = ["user_feat_w_%d" % i for i in range(Fu)] + ["item_feat_w_%d" % j for j in range(Fi)]
    spec = sr.param_spec(c)
    assert len(entries) == len(want) == len(spec) == Fu + Fi
    assert [e[0] for e in entries] == want == [s[0] for s in spec]
    for k, e in enumerate(entries):
        assert (e[2], e[3]) == (1, 0) and e[4] == 1 and e[5] == 4, e          # one float, regularised, truncated normal
        assert e[1] % 4 == 0 and e[1] == 4 * k, e                            # a 4-float cell each, in creation order
    assert n_reg == n_w == 4 * (Fu + Fi)
    # hidden_size is ignored: the layouts do not depend on it
    other = _lib.make_config(c.N, c.D, 48, c.T, 1, Fu, Fi, "SVDpp")
    assert _lib.param_layout(other) == (entries, n_w, n_reg)
    assert _lib.workspace_layout(other, 37).total_bytes == _lib.workspace_layout(cfg, 37).total_bytes
    B = 64
    total = _lib.workspace_layout(cfg, B).total_bytes // 4
    for f, n in (("svdpp_act", B * (4 * c.D + 4)), ("svdpp_dw", B * (Fu + Fi))):
        a, _ = _lib.workspace_field(cfg, B, f)
        assert 0 < a and a + n <= total, f
    g4r = _lib.make_config(c.N, c.D, c.H, c.T, 1, Fu, Fi, "GRU4Rec")
    with pytest.raises(_lib.ScoreHipError):
        _lib.workspace_field(g4r, B, "svdpp_act")            # (a region of another model type)
    with pytest.raises(_lib.ScoreHipError):
        _lib.param_layout(_lib.make_config(c.N, c.D, c.H, c.T, 2, Fu, Fi, "SVDpp"))      # obj_per_time_slice must be 1
    with pytest.raises(_lib.ScoreHipError):
        _lib.param_layout(_lib.make_config(c.N, 132, c.H, c.T, 1, Fu, Fi, "SVDpp"))      # eb_dim <= 128
    assert len(_lib.param_layout(_lib.make_config(c.N, 128, c.H, c.T, 1, Fu, Fi, "SVDpp"))[0]) == Fu + Fi


# (entries, n_floats, n_reg, crc32 of repr([(name, offset, rows, cols, regularised, init)]), workspace bytes at B = 37) of model
# types 0-10 at (N, D, H, T, Fu, Fi) = (3000, 16, 32, 50, 3, 4), K = 5 for the slice models: computed on the commit before model
# type 11 was added
LAYOUTS_BEFORE = {"SCORE": (28, 119836, 119144, 1974196070, 90060016), "RIA": (20, 80100, 79616, 3742273075, 78480720),
                  "RCA": (24, 110832, 110168, 499961094, 86713552), "SCORE_USER": (28, 113372, 112680, 4232724520, 88742000),
                  "SCORE_ITEM": (28, 113372, 112680, 4232724520, 88742000), "RRN": (16, 69004, 68528, 3278371364, 76350288),
                  "GCMC": (14, 31936, 31744, 3106040884, 72567536), "GRU4Rec": (16, 61004, 60528, 3618869701, 71278800),
                  "Caser": (14, 55992, 55696, 3432233196, 64016992), "DELF": (22, 11224, 11044, 16721512, 57084176),
                  "DEEMS": (46, 96592, 95652, 3479580423, 78219168)}


def test_the_other_model_types_layouts_are_what_they_were():
    assert sorted(_lib.MODEL_TYPES[n] for n in LAYOUTS_BEFORE) == list(range(11))
    for name, want in LAYOUTS_BEFORE.items():
        K = 1 if name in ("GRU4Rec", "Caser", "DELF", "DEEMS") else 5
        cfg = _lib.make_config(3000, 16, 32, 50, K, 3, 4, name)
        ent, nf, nr = _lib.param_layout(cfg)
        crc = zlib.crc32(repr([tuple(e) for e in ent]).encode())
        assert (len(ent), nf, nr, crc, _lib.workspace_layout(cfg, 37).total_bytes) == want, name


def test_abi_structs_are_what_they_were():
    import ctypes as C
    out = (C.c_int64 * 32)()
    assert _lib.load().score_abi_struct_sizes(out, 32) == 14 and out[3] == C.sizeof(_lib.Batch) == 80


def test_models_table_feed_spec_and_sharded_refusal():
    from score_amd import model
    assert model.MODELS["SVD++"] is model.MODELS["SVDpp"] is SVDpp
    assert SVDpp.model_type == "SVDpp" and issubclass(SVDpp, GRU4Rec)
    assert SVDpp.feed_spec is POINT_FEED and SVDpp.target_item_field == 3 and SVDpp.zero_length_reads_all is False
    # the 8-tensor device batch of GRU4Rec
    cfg = _lib.make_config(100, 16, 32, 50, 1, 3, 4, "SVDpp")
    g4r = _lib.make_config(100, 16, 32, 50, 1, 3, 4, "GRU4Rec")
    shapes = POINT_FEED.device_shapes(cfg, 6)
    assert len(shapes) == 8 and shapes == POINT_FEED.device_shapes(g4r, 6)

    class M(object):
        zero_length_reads_all = SVDpp.zero_length_reads_all
    m = M()
    m.cfg = cfg
    # a zero length does not turn into "all slices"
    assert model.active_slices(m, 7, 0) == 7 and model.active_slices(m, 7, 1) == 7 and model.active_slices(m, 70, 0) == 0
    from score_amd.dist import ShardedSCORE
    for name in ("SVDpp", "SVD++"):
        with pytest.raises(ValueError, match="SVD"):
            ShardedSCORE(100, 16, 32, 50, 1, 3, 4, comm=object(), model_type=name)
    # TF's shape () at the Python boundary, from and to the library's one-float view
    x = SVDpp._export(None, "user_feat_w_0", np.array([1.5], dtype=np.float32))
    assert x.shape == () and x.dtype == np.float32 and float(x) == 1.5
    y = SVDpp._import(None, "user_feat_w_0", np.float64(2.5), (1,))
    assert y.shape == (1,) and y.dtype == np.float32 and y[0] == 2.5


def test_a_zero_length_sample_is_nan_and_the_others_stay_finite():
    c, P, b = sc.degenerate_case()
    assert b["user_seq_length"].tolist() == [3, 9, 0, 20, 1]
    with torch.no_grad():
        out = sr.forward(c, sr.to_torch(P), b, 1e-3)
    y = out["y_pred"].numpy()
    assert np.isnan(y[2]) and np.isfinite(y[[0, 1, 3, 4]]).all()
    assert float(out["n"][2]) == 0.0 and not out["nb"][2].any()
    assert np.isnan(float(out["loss"]))
    # ... and so is a sample whose live rows are all the dummy id
    b2 = {k: v.copy() for k, v in b.items()}
    b2["user_seq_length"][2] = 2
    b2["user_seq"][2, :2] = 0
    with torch.no_grad():
        y2 = sr.forward(c, sr.to_torch(P), b2)["y_pred"].numpy()
    assert np.isnan(y2[2]) and np.array_equal(y2[[0, 1, 3, 4]], y[[0, 1, 3, 4]])


@pytest.mark.parametrize("D,T,Fu,Fi,B", list(sc.SHAPES))
def test_inputs_of_the_gpu_tests_stay_inside_the_kink_cap(D, T, Fu, Fi, B):
    c, P, b, kept = sc.case(D, T, Fu, Fi, B)        # (away_from_kinks asserts the cap)
    print("kept", kept.size, "of", B)
    assert 1 <= kept.size and B - kept.size <= sr.cap(B) and (B > 3 or kept.size == B)
    ln = b["user_seq_length"]
    assert ln.min() >= 1
    if B == 3:
        assert ln.tolist() == [1, 3, 7]
    if (T, B) == (7, 33):
        assert ln.max() <= 5
    if T >= 9:
        assert (ln > T).any() and (ln < T).any()
    with torch.no_grad():
        out = sr.forward(c, sr.to_torch(P), b)
    assert np.isfinite(float(out["loss"])) and (out["n"].numpy() > 0).all()
    assert sr.kink_free(c, P, b).all()


def test_the_kink_filter_finds_both_kinds_and_keeps_exact_ties():
    c = sr.Cfg(50, 4, 8, 3, 1, 1)
    P = sr.init_params(c, 1)
    P["item_feat_w_0"] = np.float32(1.0)
    emb = np.zeros((c.N, c.D), dtype=np.float32)
    emb[1] = [1.0, 0.5, 0.25, 0.125]           # a clear maximum
    emb[2] = [1.0, 1.0, 0.25, 0.125]           # an exact tie
    emb[3] = [1.0, 1.0 - 5e-5, 0.25, 0.125]    # a runner-up within 1e-4
    emb[4] = [1.0, 0.5, 0.25, 0.125]
    emb[5] = [1e-7, 0.0, 0.0, 0.0]             # a tiny entry in the maximal column
    P["emb_mtx"] = emb
    seq = np.array([[[1], [1], [1]], [[2], [2], [2]], [[3], [3], [3]], [[4], [5], [4]], [[4], [5], [4]]], dtype=np.int32)
    b = {"user_seq": seq, "user_seq_length": np.array([3, 3, 3, 3, 1], dtype=np.int32), "target_user": np.ones((5, 1), dtype=np.int32),
         "target_item": np.ones((5, 1), dtype=np.int32), "label": np.array([0, 1, 0, 1, 0], dtype=np.int32)}
    assert sr.kink_free(c, P, b).tolist() == [True, True, False, False, True]      # (the last: the tiny row is past the length)
    with torch.no_grad():
        assert sr.forward(c, sr.to_torch(P), b)["ties"].tolist() == [1, 2, 1, 1, 1]
    with pytest.raises(AssertionError):
        sr.away_from_kinks(c, P, {k: v[:3] for k, v in b.items()})                # B <= 3: none may go
    kept = sr.away_from_kinks(c, P, b)[1]
    assert kept.tolist() == [0, 1, 4]


def test_masked_tie_and_degenerate_cases_are_what_the_gpu_tests_expect():
    c, P, b, kept = sc.masked_case()
    ln, seq = b["user_seq_length"], b["user_seq"]
    live = np.arange(c.T)[None, :] < ln[:, None]
    assert 33 - kept.size <= sr.cap(33)
    assert ((seq == 0).all(2) & live).sum() > 10 and ((seq == 0).any(2) & ~(seq == 0).all(2) & live).sum() > 10
    out, g = sr.loss_and_grads(c, P, b, 0.0)
    assert np.isfinite(float(out["loss"].detach())) and not g["emb_mtx"][0].any()
    c, P, b, kept = sc.tie_case()
    assert 33 - kept.size <= sr.cap(33)
    out, g = sr.loss_and_grads(c, P, b, 0.0)
    assert (out["ties"].numpy() == 2).all()
    col, n = out["col"].detach().numpy(), out["n"].detach().numpy()
    assert np.array_equal(col[:, 0], n) and np.array_equal(col[:, 1], n)


def test_the_restatement_trains_scalars_of_shape_empty_tuple():
    c, P, b = _small()
    ref = sr.RefModel(c, P)
    for _ in range(2):
        assert np.isfinite(ref.train(None, sr.batch_tuple(b), 1e-3, 1e-2))
    for name, _, _, _ in sr.param_spec(c):
        # Adam's first steps move a variable by about lr per step, whatever its gradient's size
        assert ref.params[name].shape == () and 1e-3 < abs(float(ref.params[name]) - float(P[name])) < 2.1e-3, name
    assert np.array_equal(ref.params["emb_mtx"][0], P["emb_mtx"][0]) and not np.array_equal(ref.params["emb_mtx"], P["emb_mtx"])
