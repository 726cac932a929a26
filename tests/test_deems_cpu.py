"""DEEMS without a GPU: the parameter layout the library reports (host code: the library loads without a device) against the
variables of point_model.py:281-311 in TF creation order, and the layouts of model types 0-9 against what they were before model
type 10 existed; the models table, the zero-length rule of the device batch and the sharded refusal; the float64 restatement the
GPU tests compare against (tests/deems_ref.py) against autograd of ITS two losses -- the one the reference trains on and the one
it reports -- and the dormant DELF variables; a length 0; and the inputs of the GPU tests judged on the restatement alone."""
import zlib

import numpy as np
import pytest
import torch

import deems_cases as ec
import deems_ref as er
from score_amd import _lib
from score_amd.model import DEEMS, DELF, DUAL_FEED          # (the feature under test: nothing here runs without it)

INIT = {"zeros": 0, "ones": 1, "glorot": 2}


@pytest.mark.parametrize("H,T,Fu,Fi", [(32, 50, 3, 4), (32, 50, 1, 5), (16, 7, 1, 2)])
def test_param_layout_is_the_tf_variable_list(H, T, Fu, Fi):
    c = er.Cfg(1000, 16, H, T, Fu, Fi)
    assert _lib.MODEL_TYPES["DEEMS"] == 10
    cfg = _lib.make_config(c.N, c.D, c.H, c.T, 1, Fu, Fi, "DEEMS")
    entries, n_w, n_reg = _lib.param_layout(cfg)
    Ci, Cu = 16 * Fi, 16 * Fu
    names = ["dense" if i == 0 else "dense_%d" % i for i in range(11)]
    want = [n + s for n in names for s in ("/kernel", "/bias")]
    want += ["%s/gru_cell/%s/%s" % (g, p, v) for g in ("gru1", "gru2") for p in ("gates", "candidate") for v in ("kernel", "bias")]
    want += ["batch_normalization/gamma", "batch_normalization/beta"] + ["dense_%d/%s" % (i, v) for i in (11, 12, 13) for v in ("kernel", "bias")]
    want += ["batch_normalization_1/gamma", "batch_normalization_1/beta"] + ["dense_%d/%s" % (i, v) for i in (14, 15, 16) for v in ("kernel", "bias")]
    spec = er.param_spec(c)
    assert len(entries) == len(want) == len(spec) == 46
    assert [e[0] for e in entries] == want == [s[0] for s in spec]
    shapes = {"gru1/gru_cell/gates/kernel": (Ci + H, 2 * H), "gru2/gru_cell/candidate/kernel": (Cu + H, H),
              "batch_normalization/gamma": (H + Cu,), "dense_11/kernel": (H + Cu, 200), "dense_13/kernel": (80, 1),
              "batch_normalization_1/beta": (H + Ci,), "dense_14/kernel": (H + Ci, 200), "dense_15/kernel": (200, 80),
              "dense/kernel": (Ci, Ci), "dense_10/bias": (1,)}
    for e, (name, shape, init, reg) in zip(entries, spec):
        assert ((e[2], e[3]) if e[3] else (e[2],)) == tuple(shape), name
        if name in shapes:
            assert tuple(shape) == shapes[name], name
        # the regularised flag is the reference's name filter (point_model.py:58-60)
        assert bool(e[4]) == reg == ("bias" not in name and "emb" not in name), name
        assert e[5] == INIT[init], name
        assert e[1] % 4 == 0 and (e[1] < n_reg) == reg, name                      # 16-byte offsets, regularised tensors first
    spans = sorted((e[1], e[1] + e[2] * (e[3] or 1)) for e in entries)
    for a, b in zip(spans, spans[1:]):
        assert a[1] <= b[0]
    assert spans[-1][1] <= n_w
    # the regions the passes save are readable, per tower
    B = 64
    total = _lib.workspace_layout(cfg, B).total_bytes // 4
    for f, n in (("deems_y", B), ("deems_logit", B), ("deems_dlogit", B), ("deems_f1", B * 200), ("deems_f2", B * 80),
                 ("deems_dz1", B * 200), ("deems_dz2", B * 80), ("gru_final", B * H)):
        a, b2 = _lib.workspace_field(cfg, B, f)
        assert 0 < a and 0 < b2 and a + n <= total and b2 + n <= total and (b2 >= a + n or a >= b2 + n), f
    delf = _lib.make_config(c.N, c.D, c.H, c.T, 1, Fu, Fi, "DELF")
    with pytest.raises(_lib.ScoreHipError):
        _lib.workspace_field(delf, B, "deems_y")             # (a region of another model type)
    with pytest.raises(_lib.ScoreHipError):
        _lib.workspace_field(delf, B, "deems_f1")
    with pytest.raises(_lib.ScoreHipError):
        _lib.workspace_field(cfg, B, "delf_att")             # (the DELF kernels do not run: no region of theirs)
    with pytest.raises(_lib.ScoreHipError):
        _lib.param_layout(_lib.make_config(c.N, c.D, c.H, c.T, 2, Fu, Fi, "DEEMS"))      # obj_per_time_slice must be 1
    with pytest.raises(_lib.ScoreHipError):
        _lib.param_layout(_lib.make_config(c.N, c.D, 30, c.T, 1, Fu, Fi, "DEEMS"))       # hidden_size: a multiple of 4


# (entries, n_floats, n_reg, crc32 of repr([(name, offset, rows, cols, regularised, init)]), workspace bytes at B = 37) of model
# types 0-9 at (N, D, H, T, Fu, Fi) = (3000, 16, 32, 50, 3, 4), K = 5 for the slice models: computed on the commit before model
# type 10 was added
LAYOUTS_BEFORE = {"SCORE": (28, 119836, 119144, 1974196070, 90060016), "RIA": (20, 80100, 79616, 3742273075, 78480720),
                  "RCA": (24, 110832, 110168, 499961094, 86713552), "SCORE_USER": (28, 113372, 112680, 4232724520, 88742000),
                  "SCORE_ITEM": (28, 113372, 112680, 4232724520, 88742000), "RRN": (16, 69004, 68528, 3278371364, 76350288),
                  "GCMC": (14, 31936, 31744, 3106040884, 72567536), "GRU4Rec": (16, 61004, 60528, 3618869701, 71278800),
                  "Caser": (14, 55992, 55696, 3432233196, 64016992), "DELF": (22, 11224, 11044, 16721512, 57084176)}


def test_the_other_model_types_layouts_are_what_they_were():
    assert sorted(_lib.MODEL_TYPES[n] for n in LAYOUTS_BEFORE) == list(range(10))
    for name, want in LAYOUTS_BEFORE.items():
        K = 1 if name in ("GRU4Rec", "Caser", "DELF") else 5
        cfg = _lib.make_config(3000, 16, 32, 50, K, 3, 4, name)
        ent, nf, nr = _lib.param_layout(cfg)
        crc = zlib.crc32(repr([tuple(e) for e in ent]).encode())
        assert (len(ent), nf, nr, crc, _lib.workspace_layout(cfg, 37).total_bytes) == want, name


def test_abi_structs_are_what_they_were():
    import ctypes as C
    out = (C.c_int64 * 32)()
    assert _lib.load().score_abi_struct_sizes(out, 32) == 14 and out[3] == C.sizeof(_lib.Batch) == 80


def test_models_table_zero_length_rule_and_sharded_refusal():
    from score_amd import model
    assert model.MODELS["DEEMS"] is DEEMS and DEEMS.model_type == "DEEMS" and issubclass(DEEMS, DELF)
    assert DEEMS.target_item_field == 5 and DEEMS.feed_spec is DUAL_FEED and DEEMS.dropout_towers == 2 and DELF.dropout_towers == 1
    cfg = _lib.make_config(100, 16, 32, 50, 1, 3, 4, "DEEMS")
    assert len(DUAL_FEED.device_shapes(cfg, 6)) == 9

    class M(object):
        zero_length_reads_all = DEEMS.zero_length_reads_all
    m = M()
    m.cfg = cfg
    # a zero length does not turn into "all slices" (DELF's rule: test_delf_cpu.py); the maximum over both tensors decides
    assert model.active_slices(m, 7, 0) == 7 and model.active_slices(m, 7, 1) == 7 and model.active_slices(m, 70, 0) == 0
    assert model.active_slices(m, 0, 0) == 1
    from score_amd.dist import ShardedSCORE
    with pytest.raises(ValueError, match="DEEMS"):
        ShardedSCORE(100, 16, 32, 50, 1, 3, 4, comm=object(), model_type="DEEMS")


def _small():
    c = er.Cfg(300, 4, 8, 5, 2, 1)
    P = er.init_params(c, 9, bias_scale=0.1)
    rng = np.random.default_rng(5)
    b = er.random_batch(rng, c, 6)
    b["user_seq_length"] = np.array([9, 0, 3, 5, 1, 2], dtype=np.int32)       # longer than T, never runs, ...
    b["item_seq_length"] = np.array([2, 4, 0, 12, 5, 1], dtype=np.int32)
    b["label"] = np.array([0, 1, 1, 0, 1, 0], dtype=np.int32)
    return c, P, b


def test_restatement_trains_on_train_loss_and_reports_loss():
    c, P, b = _small()
    lam = 1e-2
    out, g = er.loss_and_grads(c, P, b, lam)
    # the gradient is autograd of train_loss = log_loss + lam * l2 ...
    Q = er.to_torch(P, requires_grad=True)
    o2 = er.forward(c, Q, b, lam)
    want = torch.autograd.grad(o2["log_loss"] + lam * o2["l2"], [Q[k] for k in sorted(Q)], allow_unused=True)
    for k, w in zip(sorted(Q), want):
        w = np.zeros_like(g[k]) if w is None else w.numpy()
        assert np.array_equal(g[k], w), k
    assert float(out["train_loss"].detach()) == float((out["log_loss"] + lam * out["l2"]).detach())
    # ... and the reported loss is train_loss + 0.05 * SUM (y_i - y_u)^2, a sum over the batch
    yu, yi = out["y_u"].detach().numpy(), out["y_i"].detach().numpy()
    assert np.abs(yu - yi).min() > 0
    cons = 0.05 * float(((yi - yu) ** 2).sum())
    assert abs(float(out["consistency"].detach()) - cons) < 1e-15 and abs(float((out["loss"] - out["train_loss"]).detach()) - cons) < 1e-15
    assert np.array_equal(out["y_pred"].detach().numpy(), 0.5 * (yu + yi))
    # ... whose own gradient is another one wherever y_u != y_i
    _, g_rep = er.loss_and_grads(c, P, b, lam, of="loss")
    for k in ("dense_13/kernel", "dense_16/bias", "gru1/gru_cell/gates/kernel", "batch_normalization_1/gamma", "emb_mtx"):
        assert np.abs(g_rep[k] - g[k]).max() > 1e-6 * np.abs(g[k]).max() > 0, k
    # DELF's variables: the kernels get exactly lam * W, the biases nothing
    for i in range(11):
        nm = "dense" if i == 0 else "dense_%d" % i
        assert np.array_equal(g[nm + "/kernel"], lam * P[nm + "/kernel"].astype(np.float64)), nm
        assert not g[nm + "/bias"].any(), nm
        assert np.array_equal(g_rep[nm + "/kernel"], g[nm + "/kernel"])
    assert not g["emb_mtx"][0].any()
    # the ten variables the prediction reads all get a gradient from the log-loss
    _, g0 = er.loss_and_grads(c, P, b, 0.0)
    for name, _, _, _ in er.param_spec(c)[22:]:
        assert np.abs(g0[name]).max() > 0, name


def test_a_zero_length_gives_a_zero_state_and_a_finite_loss():
    c, P, b = _small()
    with torch.no_grad():
        out = er.forward(c, er.to_torch(P), b, 1e-3)
    hu, hi = out["h_u"].numpy(), out["h_i"].numpy()
    assert not hu[1].any() and hu[[0, 2, 3, 4, 5]].any(1).all()
    assert not hi[2].any() and hi[[0, 1, 3, 4, 5]].any(1).all()
    assert np.isfinite(float(out["loss"])) and np.isfinite(out["y_pred"].numpy()).all()
    # a length above T is all T positions
    b2 = dict(b, user_seq_length=np.minimum(b["user_seq_length"], c.T), item_seq_length=np.minimum(b["item_seq_length"], c.T))
    with torch.no_grad():
        out2 = er.forward(c, er.to_torch(P), b2, 1e-3)
    assert float(out2["loss"]) == float(out["loss"])
    # swapping the two length tensors is another model input
    b3 = dict(b, user_seq_length=b["item_seq_length"], item_seq_length=b["user_seq_length"])
    with torch.no_grad():
        out3 = er.forward(c, er.to_torch(P), b3, 1e-3)
    assert float(out3["loss"]) != float(out["loss"])


@pytest.mark.parametrize("D,H,T,Fu,Fi,B", list(ec.SHAPES))
def test_inputs_of_the_gpu_tests_stay_inside_the_kink_cap(D, H, T, Fu, Fi, B):
    c, P, b, kept = ec.case(D, H, T, Fu, Fi, B)        # (away_from_kinks asserts the cap)
    print("kept", kept.size, "of", B)
    assert 1 <= kept.size and B - kept.size <= er.cap(B)
    ul, il = b["user_seq_length"], b["item_seq_length"]
    if B == 3:
        assert kept.size == 3 and ul.tolist() == [0, 2, 7] and il.tolist() == [7, 0, 2]
    if B in (33, 37):
        assert kept.size % 16 != 0           # the last 16-row tile stays ragged behind the filter
    if (T, B) == (7, 33):
        assert max(ul.max(), il.max()) <= 5 and min(ul.min(), il.min()) >= 1
    if T >= 50:
        assert (ul > T).any() and (ul < T).any() and (il > T).any() and (il < T).any()
    with torch.no_grad():
        out = er.forward(c, er.to_torch(P), b)
    assert np.isfinite(float(out["loss"]))
    assert (out["relu_margin_per_sample"] > er.RELU_THR).all()


def test_dropout_case_stays_inside_the_kink_cap():
    c, P, b, masks, kept = ec.dropout_case()
    B = ec.DROPOUT_SHAPE[-1]
    assert B - kept.size <= er.cap(B) and masks[0].shape == (2, kept.size, 200) and masks[1].shape == (2, kept.size, 80)
    assert not np.array_equal(masks[0][0], masks[0][1])
    for m in masks:
        assert 0.7 < m.mean() < 0.9


def test_consistency_case_is_more_than_a_hundredth_of_the_loss():
    c, P, b, _ = ec.case(16, 32, 50, 3, 4, 200)
    with torch.no_grad():
        out = er.forward(c, er.to_torch(P), b)
    assert float(out["consistency"]) > 0.01 * float(out["loss"])
