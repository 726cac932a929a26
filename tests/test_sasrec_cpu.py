"""SASRec without a GPU: the float64 restatement the GPU tests compare against (tests/sasrec_ref.py) against finite differences
at the smallest shape; the edge filter's caps over the inputs of the GPU tests; the parameter layout the library reports (host
code: the library loads without a device) against the variables of point_model.py:313-469 in TF creation order, and the layouts
of model types 0-11 against what they were before model type 12 existed; the models table, the constructor's refusals and the
sharded refusal."""
import zlib

import numpy as np
import pytest
import torch

import sasrec_cases as sc
import sasrec_ref as sr
from score_amd import _lib
from score_amd.model import GRU4Rec, MODELS, POINT_FEED          # (MODELS["SASRec"]: the feature under test)


def _small():
    c = sr.Cfg(40, 4, 8, 3, 1, 1)
    P = sr.init_params(c, 9, perturbed=True)
    rng = np.random.default_rng(5)
    b = sr.random_batch(rng, c, 4, max_length=5)
    b["user_seq_length"] = np.array([5, 1, 2, 3], dtype=np.int32)
    b["user_seq"][2, 1] = 0                                                   # an all-zero row: its key is masked
    b["label"] = np.array([0, 1, 1, 0], dtype=np.int32)
    return c, P, b


def test_restatement_against_finite_differences():
    c, P, b = _small()
    assert sr.edge_free(c, P, b).all()
    lam = 1e-2
    out, g = sr.loss_and_grads(c, P, b, lam)
    assert float(out["att"].detach()[2, :, :, 1].abs().max()) == 0.0 and float(out["att"].detach()[2].sum(-1).min()) > 0.999      # the masked key

    def loss_at(name, idx, delta):
        Q = {k: np.array(v, dtype=np.float64) for k, v in P.items()}
        Q[name][idx] += delta
        with torch.no_grad():
            return float(sr.forward(c, sr.to_torch(Q), b, lam)["loss"])

    eps = 1e-6
    rng = np.random.default_rng(0)
    for name, shape, _, _ in sr.param_spec(c):
        n = int(np.prod(shape))
        for flat in rng.choice(n, size=min(n, 6), replace=False):
            idx = np.unravel_index(int(flat), shape)
            fd = (loss_at(name, idx, eps) - loss_at(name, idx, -eps)) / (2 * eps)
            assert abs(fd - g[name][idx]) < 2e-7 * max(1.0, abs(fd)), (name, idx, fd, g[name][idx])
        assert np.abs(g[name]).max() > 0, name
    rows = sorted(set(int(x) for x in np.concatenate([b["user_seq"].reshape(-1), b["target_user"].reshape(-1), b["target_item"].reshape(-1)])))
    seen = 0
    for r in rows:
        for d in range(c.D):
            fd = (loss_at("emb_mtx", (r, d), eps) - loss_at("emb_mtx", (r, d), -eps)) / (2 * eps)
            assert abs(fd - g["emb_mtx"][r, d]) < 2e-7 * max(1.0, abs(fd)), (r, d, fd, g["emb_mtx"][r, d])
            seen += fd != 0
    assert 0 in rows and seen > c.D and not g["emb_mtx"][0].any()
    # the l2 term reaches both layer-norm variables and no bias
    _, g0 = sr.loss_and_grads(c, P, b, 0.0)
    for name, _, _, reg in sr.param_spec(c):
        want = lam * P[name].astype(np.float64) if reg else 0.0
        assert np.abs(g[name] - g0[name] - want).max() < 1e-12, name
    assert sum(r for _, _, _, r in sr.param_spec(c)) == 8
    # gamma's ones alone contribute C / 2 to the l2 sum at TF's initial values
    P0 = sr.init_params(c, 9)
    with torch.no_grad():
        l2 = float(sr.forward(c, sr.to_torch(P0), b)["l2"])
    others = sum(float((P0[n].astype(np.float64) ** 2).sum()) * 0.5 for n, _, i, r in sr.param_spec(c) if r and i == "glorot")
    assert abs(l2 - others - c.Ci / 2) < 1e-12


def test_dropout_masks_reach_all_three_uses_and_the_negative_rows_equal_the_positive_ones_without_them():
    c, P, b = _small()
    B = 4
    with torch.no_grad():
        out = sr.forward(c, sr.to_torch(P), b)
    pos = out["p_pos"].reshape(B, c.T - 1)
    neg = out["p_neg"].reshape(B, c.T - 2)
    assert torch.equal(pos[:, 1:], neg)
    masks = sr.random_masks(np.random.default_rng(1), c, B, 0.5)
    nP, nN, _ = sr.rows(c, B)
    assert masks[0].shape == (nP + nN + B, 200) and masks[1].shape == (nP + nN + B, 80) and masks[2].shape == (2, B, c.T, c.T)
    with torch.no_grad():
        base = sr.forward(c, sr.to_torch(P), b, 0.0, 0.5, masks)
    for i, part in ((0, slice(0, nP)), (0, slice(nP, nP + nN)), (0, slice(nP + nN, None)), (1, slice(0, nP)), (2, None)):
        m = [x.copy() for x in masks]
        if part is None:
            m[i][:] = 1 - m[i]
        else:
            m[i][part] = 1 - m[i][part]
        with torch.no_grad():
            o = sr.forward(c, sr.to_torch(P), b, 0.0, 0.5, m)
        assert float(o["loss"]) != float(base["loss"]), (i, part)
    kept = np.array([0, 2])
    sel = sr.select_masks(c, masks, B, kept)
    bb = {k: v[kept] for k, v in b.items()}
    with torch.no_grad():
        o = sr.forward(c, sr.to_torch(P), bb, 0.0, 0.5, sel)
    assert torch.equal(o["y_pred"], base["y_pred"][kept]) and torch.equal(o["Y"], base["Y"][kept])
    assert torch.equal(o["p_neg"].reshape(2, -1), base["p_neg"].reshape(B, -1)[kept])


@pytest.mark.parametrize("D,T,Fu,Fi,B", list(sc.SHAPES))
def test_inputs_of_the_gpu_tests_stay_inside_the_edge_cap(D, T, Fu, Fi, B):
    c, P, b, kept = sc.case(D, T, Fu, Fi, B)        # (away_from_edges asserts the cap)
    print("kept", kept.size, "of", B)
    assert kept.size >= max(1, (3 * B) // 4)
    if B == 3:
        assert b["user_seq_length"].tolist() == [1, 4, 9]
    with torch.no_grad():
        out = sr.forward(c, sr.to_torch(P), b)
    assert np.isfinite(float(out["loss"])) and sr.edge_free(c, P, b).all()
    assert float(out["qsum"].abs().min()) > 0.1 * c.Ci / 2          # the query mask: decided by a wide margin


def test_named_cases_are_what_the_gpu_tests_expect():
    for beta_zero in (False, True):
        c, P, b, kept = sc.masked_case(beta_zero)
        assert kept.size >= 25
        seq = b["user_seq"]
        zero = (seq == 0).all(2)
        assert zero.sum() > 10 and ((seq == 0).any(2) & ~zero).sum() > 10
        out, g = sr.loss_and_grads(c, P, b, 0.0)
        att = out["att"].detach().numpy()
        assert not att[np.broadcast_to(zero[:, None, None, :], att.shape)].any()           # masked keys
        qs = out["qsum"].numpy()
        if beta_zero:
            assert not P["ln/Variable"].any() and (qs[zero] == 0).all() and (np.abs(qs[~zero]) > sr.MASK_THR).all()
            assert not att[np.broadcast_to(zero[:, None, :, None], att.shape)].any()       # masked queries
        else:
            assert (np.abs(qs) > 1.0).all()
        assert np.isfinite(float(out["loss"].detach())) and not g["emb_mtx"][0].any()
    c, P, b = sc.all_masked_case()
    assert len(b["label"]) == 3 and not b["user_seq"][1].any()
    out, g = sr.loss_and_grads(c, P, b, 0.0)
    assert np.allclose(out["att"][1].detach().numpy(), 1.0 / c.T, rtol=1e-12, atol=0)
    assert np.isfinite(float(out["loss"].detach())) and all(np.isfinite(v).all() for v in g.values())
    c, P, b, masks, kept = sc.dropout_case()
    assert kept.size >= 25
    nP, nN, nF = sr.rows(c, kept.size)
    assert masks[0].shape == (nP + nN + nF, 200) and masks[2].shape == (2, kept.size, c.T, c.T)
    assert sr.edge_free(c, P, b, 0.8, masks).all()
    c, P, bs = sc.trajectory_case()
    assert c.args == (20011,) + sc.TMALL and len(bs) == 5 and len(bs[0]["label"]) == 24


@pytest.mark.parametrize("D,T,Fu,Fi", [(16, 50, 3, 4), (16, 50, 1, 5), (4, 3, 1, 1), (32, 5, 1, 4)])
def test_param_layout_is_the_tf_variable_list(D, T, Fu, Fi):
    c = sr.Cfg(1000, D, 32, T, Fu, Fi)
    assert _lib.MODEL_TYPES["SASRec"] == 12
    cfg = _lib.make_config(c.N, c.D, c.H, c.T, 1, Fu, Fi, "SASRec")
    entries, n_w, n_reg = _lib.param_layout(cfg)
    spec = sr.param_spec(c)
    assert len(entries) == len(spec) == 14
    assert [e[0] for e in entries] == [s[0] for s in spec]
    assert [e[0] for e in entries][:4] == ["ln/Variable", "ln/Variable_1", "multihead_attention/dense/kernel", "multihead_attention/dense/bias"]
    init_code = {"zeros": 0, "ones": 1, "glorot": 2}
    for e, (name, shape, init, reg) in zip(entries, spec):
        assert (e[2], e[3]) == (shape[0], shape[1] if len(shape) > 1 else 0), e
        assert e[4] == int(reg) and e[5] == init_code[init] and e[1] % 4 == 0, e
        assert (e[1] < n_reg) == bool(reg), e
    assert entries[0][4] == 1 and entries[1][4] == 1 and entries[1][5] == 1          # both ln variables regularised; gamma ones
    assert sum(e[4] for e in entries) == 8
    # hidden_size is ignored: the layouts do not depend on it
    other = _lib.make_config(c.N, c.D, 48, c.T, 1, Fu, Fi, "SASRec")
    assert _lib.param_layout(other) == (entries, n_w, n_reg)
    assert _lib.workspace_layout(other, 37).total_bytes == _lib.workspace_layout(cfg, 37).total_bytes
    B = 9
    total = _lib.workspace_layout(cfg, B).total_bytes // 4
    R = B * (T - 1) + B * (T - 2) + B
    for f, n in (("sasrec_y", B * T * c.Ci), ("sasrec_final", B * c.Ci), ("sasrec_att", 2 * B * T * T), ("sasrec_p", 2 * B * T * T),
                 ("sasrec_qin", B * T * c.Ci), ("sasrec_hin", B * T * c.Dh), ("sasrec_logit", R)):
        a, _ = _lib.workspace_field(cfg, B, f)
        assert 0 < a and a + n <= total, f
    g4r = _lib.make_config(c.N, c.D, c.H, c.T, 1, Fu, Fi, "GRU4Rec")
    with pytest.raises(_lib.ScoreHipError):
        _lib.workspace_field(g4r, B, "sasrec_att")            # (a region of another model type)


def test_the_library_refuses_what_the_kernels_do_not_cover():
    ok = lambda *a: _lib.param_layout(_lib.make_config(*a))
    assert len(ok(1000, 16, 32, 3, 1, 3, 4, "SASRec")[0]) == 14
    assert len(ok(1000, 32, 32, 50, 1, 3, 4, "SASRec")[0]) == 14          # C = 128, T = 50: inside one workgroup's LDS
    for args in ((1000, 16, 32, 2, 1, 3, 4),          # max_time_len < 3
                 (1000, 16, 32, 50, 2, 3, 4),         # obj_per_time_slice must be 1
                 (1000, 44, 32, 9, 1, 3, 3),          # C = 132 > 128
                 (1000, 32, 32, 400, 1, 3, 4)):       # a sample's buffers beyond 160 KiB of LDS
        with pytest.raises(_lib.ScoreHipError):
            ok(*args, "SASRec")


# (entries, n_floats, n_reg, crc32 of repr([(name, offset, rows, cols, regularised, init)]), workspace bytes at B = 37) of model
# types 0-11 at (N, D, H, T, Fu, Fi) = (3000, 16, 32, 50, 3, 4), K = 5 for the slice models: computed on the commit before model
# type 12 was added
LAYOUTS_BEFORE = {"SCORE": (28, 119836, 119144, 1974196070, 90060016), "RIA": (20, 80100, 79616, 3742273075, 78480720),
                  "RCA": (24, 110832, 110168, 499961094, 86713552), "SCORE_USER": (28, 113372, 112680, 4232724520, 88742000),
                  "SCORE_ITEM": (28, 113372, 112680, 4232724520, 88742000), "RRN": (16, 69004, 68528, 3278371364, 76350288),
                  "GCMC": (14, 31936, 31744, 3106040884, 72567536), "GRU4Rec": (16, 61004, 60528, 3618869701, 71278800),
                  "Caser": (14, 55992, 55696, 3432233196, 64016992), "DELF": (22, 11224, 11044, 16721512, 57084176),
                  "DEEMS": (46, 96592, 95652, 3479580423, 78219168), "SVDpp": (7, 28, 28, 2778035981, 53222896)}

# float offsets of a few workspace regions from the front, the middle and the end of the layout at B = 37, same configs, same commit
OFFSET_FIELDS = ("xside", "head_inp", "f1", "dhead", "dxside", "dtgt", "dgstage", "S")
OFFSETS_BEFORE = {"SCORE": (0, 474048, 1973668, 2001240, 3331796, 20418664, 10416424, 3749900),
                  "RIA": (0, 474048, 1545532, 1573104, 2566504, 17523840, 9428928, 2984608),
                  "RCA": (0, 474048, 1871728, 1899300, 3149576, 19582048, 10012000, 3567680),
                  "SCORE_USER": (0, 474048, 1971300, 1997688, 3327060, 20089160, 10398376, 3745164),
                  "SCORE_ITEM": (0, 474048, 1971300, 1997688, 3327060, 20089160, 10398376, 3745164),
                  "RRN": (0, 474048, 1545532, 1573104, 2566504, 16991232, 9428928, 2984608),
                  "GCMC": (0, 474048, 1545532, 1573104, 2566504, 15211968, 9428928, 2984608),
                  "GRU4Rec": (0, 429648, 1498764, 1525152, 2487768, 16497712, 9350192, 2905872),
                  "Caser": (0, 429648, 670292, 698012, 943088, 14679812, 7783820, 1361192),
                  "DELF": (0, 429648, 665260, 690464, 933024, 12518368, 7773756, 1351128),
                  "DEEMS": (0, 429648, 1501132, 1528704, 2492504, 18211856, 9354928, 2910608),
                  "SVDpp": (0, 429648, 665260, 690464, 933024, 11980960, 7773756, 1351128)}


def test_the_other_model_types_layouts_are_what_they_were():
    assert sorted(_lib.MODEL_TYPES[n] for n in LAYOUTS_BEFORE) == list(range(12))
    for name, want in LAYOUTS_BEFORE.items():
        K = 1 if name in ("GRU4Rec", "Caser", "DELF", "DEEMS", "SVDpp") else 5
        cfg = _lib.make_config(3000, 16, 32, 50, K, 3, 4, name)
        ent, nf, nr = _lib.param_layout(cfg)
        crc = zlib.crc32(repr([tuple(e) for e in ent]).encode())
        assert (len(ent), nf, nr, crc, _lib.workspace_layout(cfg, 37).total_bytes) == want, name
        got = tuple(_lib.workspace_field(cfg, 37, f)[0] for f in OFFSET_FIELDS)
        assert got == OFFSETS_BEFORE[name], (name, got)


def test_abi_structs_are_what_they_were():
    import ctypes as C
    out = (C.c_int64 * 32)()
    lib = _lib.load()
    assert lib.score_abi_struct_sizes(out, 32) == 14 and out[3] == C.sizeof(_lib.Batch) == 80
    # drop_mask2 took the slot of two reserved 32-bit words behind plan_workspace: same size, same offsets
    assert _lib.State.drop_mask2.offset == _lib.State.plan_workspace.offset + 8 and _lib.State.drop_mask2.size == 8
    assert C.sizeof(_lib.State) == _lib.State.drop_mask2.offset + 8 and C.sizeof(_lib.State) in list(out)


def test_models_table_constructor_refusals_and_sharded_refusal():
    SASRec = MODELS["SASRec"]
    assert SASRec.model_type == "SASRec" and issubclass(SASRec, GRU4Rec)
    assert SASRec.feed_spec is POINT_FEED and SASRec.target_item_field == 3 and SASRec.reads_length is False
    # the refusals come before anything touches a device
    with pytest.raises(ValueError, match="max_time_len"):
        SASRec(100, 16, 32, 2, 3, 4)
    with pytest.raises(ValueError, match="item_fnum"):
        SASRec(100, 44, 32, 9, 3, 3)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            SASRec(100, 16, 32, 9, 3, 4)           # (a legal shape gets as far as the device check)

    class M(object):
        reads_length = SASRec.reads_length
        skip_masked_slices = True
        _mask_shapes = SASRec._mask_shapes
    m = M()
    m.cfg = _lib.make_config(100, 16, 32, 9, 1, 3, 4, "SASRec")
    from score_amd import model
    assert model.active_slices(m, 3, 1) == 0          # every batch computes all T positions
    assert m._mask_shapes(5) == ((5 * 8 + 5 * 7 + 5, 200), (5 * 8 + 5 * 7 + 5, 80), (2, 5, 9, 9))
    from score_amd.dist import ShardedSCORE
    with pytest.raises(ValueError, match="SASRec"):
        ShardedSCORE(100, 16, 32, 50, 1, 3, 4, comm=object(), model_type="SASRec")
