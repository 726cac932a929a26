"""The four fused kernels of the launch-stream pass (csrc/head_fused.hip, head_tiles.h: head_fwd_fused_kernel in one and in two
launches, head_bwd_fused_kernel, attn_fwd_fused_kernel<KQ>, attn_inp_bwd_fused_kernel) at their loop edges (tests/score_head_cases.py:
the chunks of hf_tiles, the head forward's split, the shares of the head backward's grid, samples per workgroup, row tiles, widths
and LDS bound of the attention, lengths past T, explicit dropout masks, saturated parameters).  Per row: the forms the pass took
(score_head_last_forms) are the ones the row names; loss, predictions, logits, attention weights, the head's input and every
gradient against the float64 oracle; the same bits from a fresh model; the layered pass at the bounds of
test_fused_and_layerwise_paths_agree; two optimizer steps and the predictions against the oracle model.  The parameter cases are
compared at operator level, in float64, from the kernels' own fp32 inputs.  tests/test_score_head_cases_cpu.py judges the same
inputs on the oracle alone (run with -s: every row prints its largest errors)."""
import numpy as np
import pytest
import torch

from oracle import score_oracle as so
from score_amd import _lib
from helpers import batch_tuple
from test_gpu_model import make_model, close, LOGIT_TOL
import score_head_cases as hc

pytestmark = pytest.mark.gpu

LOGLOSS_EPS = np.float32(1e-7)          # SCORE_LOGLOSS_EPS (csrc/cell.h), a float32 constant


def _pass(m, c, flags, fields=()):
    """one forward + backward pass of a case (reg_lambda 0) -> the forms it took, loss, y_pred, logit, att_score [B, T], head_inp
    [B, Dh], the dense and the table gradient as device tensors, further workspace regions by name"""
    r, B = c.row, c.row.B
    m.debug_flags = flags
    lay, ws = m.forward_backward(batch_tuple(c.batch), 0.0, r.keep, c.masks)
    torch.cuda.synchronize()
    forms = _lib.load().score_head_last_forms()
    Dh = c.cfg.Dhead
    out = dict(forms=forms, loss=float(ws[lay.loss].item()), y=ws[lay.y_pred:lay.y_pred + B].clone(),
               logit=ws[lay.logit:lay.logit + B].clone(), att=ws[lay.att_score:lay.att_score + B * r.T].clone().view(B, r.T),
               head_inp=ws[lay.head_inp:lay.head_inp + B * Dh].clone().view(B, Dh), w_g=m.w_g.clone(),
               table_g=m.dense_table_grad().clone())
    for name, n in fields:
        off = _lib.workspace_field(m.cfg, B, name)[0]
        out[name] = ws[off:off + n].clone()
    m.debug_flags = hc.FLAGS
    return out


def _same_bits(a, b):
    return a["loss"] == b["loss"] and all(torch.equal(a[k], b[k]) for k in ("y", "logit", "att", "head_inp", "w_g", "table_g"))


def _grads(m, p):
    g = {e[0]: m._view(p["w_g"], e).cpu().numpy() for e in m.entries}
    g["emb_mtx"] = p["table_g"].cpu().numpy()
    return g


def _softmax_rows_are_masked(att, L, T):
    """slices behind a sample's length weigh exactly 0; a length <= 0 gives exactly 1 / T (a softmax over an all-masked row)"""
    for i in range(att.shape[0]):
        if L[i] <= 0:
            assert np.all(att[i] == np.float32(1) / np.float32(T)), i
        else:
            assert np.all(att[i, min(int(L[i]), T):] == 0), i
    assert np.abs(att.astype(np.float64).sum(1) - 1).max() < 1e-5


def _shape_case(name, c):
    r, b, B = c.row, c.batch, c.row.B
    lib = _lib.load()
    m = make_model(c.cfg, c.P)
    m.debug_flags = hc.FLAGS
    assert m.device_batch(batch_tuple(b)).active_slices == 0            # (every slice is computed: T is the configuration's)
    # a. the forms
    p = _pass(m, c, hc.FLAGS)
    assert p["forms"] == hc.pack(r.forms), (name, hc.unpack(p["forms"]), r.forms)
    # b. against the float64 oracle
    oo, go = so.loss_and_grads(c.cfg, c.P, b, 0.0, r.keep, [torch.as_tensor(x) for x in c.masks] if c.masks is not None else None,
                               dtype=torch.float64)
    want_loss = float(oo["loss"].detach())
    g = _grads(m, p)
    dl = abs(p["loss"] - want_loss) / max(1.0, abs(want_loss))
    dy = float(np.abs(p["y"].cpu().numpy() - oo["y_pred"].detach().numpy()).max())
    dz = float(np.abs(p["logit"].cpu().numpy() - oo["logit"].detach().numpy()).max())
    att = p["att"].cpu().numpy()
    res = {"att_score": close(att, oo["att_score"].detach().numpy(), rtol=hc.RTOL, atol=hc.ATOL),
           "head_inp": close(p["head_inp"].cpu().numpy(), oo["head_inp"].detach().numpy(), rtol=hc.RTOL, atol=hc.ATOL)}
    for k in go:
        res[k] = close(g[k].reshape(np.asarray(go[k]).shape), go[k], rtol=hc.RTOL, atol=hc.ATOL)
    worst = max(res, key=lambda k: res[k][1])
    print("%s vs float64: loss %.2e, y_pred %.2e, logit %.2e, worst array %s %.2e" % (name, dl, dy, dz, worst, res[worst][1]))
    assert dl < hc.LOSS_TOL, (p["loss"], want_loss)
    assert dy < hc.Y_TOL and dz < hc.Y_TOL, (dy, dz)
    for k, (ok, err) in res.items():
        assert ok, (k, err)
    for k in go:
        assert np.isfinite(g[k]).all(), k
    assert np.isfinite(p["loss"]) and np.isfinite(att).all() and bool(torch.isfinite(p["head_inp"]).all())
    assert np.all(g["emb_mtx"][0] == 0)
    _softmax_rows_are_masked(att, b["length"], r.T)
    # c. the same pass on a fresh model: the same bits (fixed-order sums; stale LDS or an idle lane in a reduction shows here)
    assert _same_bits(p, _pass(make_model(c.cfg, c.P), c, hc.FLAGS)), name
    # d. head and attention layer by layer / as separate launches
    q = _pass(m, c, hc.FLAGS_LAYERED)
    assert q["forms"] == hc.pack(hc.LAYERED), (name, hc.unpack(q["forms"]))
    dyl = float((p["y"] - q["y"]).abs().max())
    gl = _grads(m, q)
    resl = {k: close(g[k], gl[k], rtol=2e-5, atol=1e-9) for k in g}
    worst = max(resl, key=lambda k: resl[k][1])
    print("    vs the layered pass: y_pred %.2e, worst gradient %s %.2e" % (dyl, worst, resl[worst][1]))
    assert dyl < 2e-6
    for k, (ok, err) in resl.items():
        assert ok, (k, err)
    # e. two TF-Adam steps and the predictions against the oracle model
    om = so.OracleModel(c.cfg.N, c.cfg.D, c.cfg.H, c.cfg.T, c.cfg.K, c.cfg.Fu, c.cfg.Fi, c.cfg.model_type,
                        params={k: v.copy() for k, v in c.P.items()})
    for step in range(2):
        lg = m.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=r.keep, dropout_masks=c.masks)
        lo = om.train(None, batch_tuple(b), 1e-3, 1e-4, keep_prob=r.keep, dropout_masks=c.masks)
        assert lib.score_head_last_forms() == hc.pack(r.forms)
        assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo)), (step, lg, lo)
    pg, _, _ = m.eval(None, batch_tuple(b), 1e-4)
    po, _, _ = om.eval(None, batch_tuple(b), 1e-4)
    torch.cuda.synchronize()
    assert np.abs(np.asarray(pg) - np.asarray(po)).max() < LOGIT_TOL


def _param_case(name, c):
    """the saturated cases at operator level: every operator's output in float64 from the fp32 inputs the kernel itself read"""
    r, b, B, T = c.row, c.batch, c.row.B, c.row.T
    m = make_model(c.cfg, c.P)
    p = _pass(m, c, hc.FLAGS, fields=(("a2", B * T * hc.AT2), ("lossb", B), ("dlogit", B), ("f1", B * hc.FC1), ("a1", B * T * hc.AT1)))
    assert p["forms"] == hc.pack(r.forms), (name, hc.unpack(p["forms"]), r.forms)
    assert _same_bits(p, _pass(make_model(c.cfg, c.P), c, hc.FLAGS)), name
    L = b["length"]
    att = p["att"].cpu().numpy()
    y, logit = p["y"].cpu().numpy(), p["logit"].cpu().numpy()
    g = _grads(m, p)
    for k in g:
        assert np.isfinite(g[k]).all(), k
    assert np.isfinite(p["loss"]) and np.isfinite(att).all() and np.isfinite(y).all() and np.isfinite(logit).all()
    assert np.all(g["emb_mtx"][0] == 0)
    _softmax_rows_are_masked(att, L, T)
    # att_score from the kernel's a2, dense_5 and the lengths.  delta: the per-score bound of the project's GEMM tests; a score error
    # becomes that relative error of a weight
    a2 = p["a2"].cpu().numpy().astype(np.float64).reshape(B, T, hc.AT2)
    w5, b5 = c.P["dense_5/kernel"].astype(np.float64).reshape(-1), float(c.P["dense_5/bias"].reshape(-1)[0])
    s = a2 @ w5 + b5
    live = np.arange(T)[None, :] < L[:, None]
    delta = np.where(live, 2e-6 * (np.abs(a2) @ np.abs(w5) + abs(b5)) + 1e-6, 0.0).max(1, keepdims=True)      # (a row's largest)
    s = np.where(live, s, float(so.PAD_SCORE))
    e = np.exp(s - s.max(1, keepdims=True))
    w = e / e.sum(1, keepdims=True)
    excess = np.abs(att - w) - (w * (2 * delta + 1e-5) + 1e-7)
    print("%s: att_score against its float64 restatement: |d| %.2e (bound excess %.2e, delta %.2e)"
          % (name, float(np.abs(att - w).max()), float(excess.max()), float(delta.max())))
    assert excess.max() <= 0
    # y_pred against the sigmoid of the kernel's logit; the loss term and its gradient from the kernel's y_pred (the sums with
    # SCORE_LOGLOSS_EPS in float32, as the kernel forms them -- they are exact or single roundings --, the rest in float64)
    z = logit.astype(np.float64)
    want_y = np.where(z >= 0, 1 / (1 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1 + np.exp(-np.abs(z))))
    assert np.all(np.abs(y - want_y) <= 1e-7 + 1e-6 * np.abs(want_y)), float(np.abs(y - want_y).max())
    lab = b["label"].astype(np.float64)
    pe = (y + LOGLOSS_EPS).astype(np.float64)
    qe = ((np.float32(1) - y) + LOGLOSS_EPS).astype(np.float64)
    want_lossb = -lab * np.log(pe) - (1 - lab) * np.log(qe)
    want_dlogit = (-lab / pe + (1 - lab) / qe) / B * y.astype(np.float64) * (np.float32(1) - y).astype(np.float64)
    lossb, dlogit = p["lossb"].cpu().numpy(), p["dlogit"].cpu().numpy()
    print("    lossb %.2e, dlogit %.2e (relative)" % (float((np.abs(lossb - want_lossb) / np.maximum(np.abs(want_lossb), 1e-300)).max()),
                                                    float((np.abs(dlogit - want_dlogit) / np.maximum(np.abs(want_dlogit), 1e-300)).max())))
    # (1e-37: below float32's normal range -- a saturated y_pred is a denormal before it is 0 -- a product has no relative precision)
    assert np.all(np.abs(lossb - want_lossb) <= 1e-6 * np.abs(want_lossb) + 1e-37)
    assert np.all(np.abs(dlogit - want_dlogit) <= 1e-6 * np.abs(want_dlogit) + 1e-37)
    assert abs(p["loss"] - want_lossb.mean()) <= 2e-6 * max(1.0, abs(want_lossb.mean()))
    if name == "sigmoid_01":
        assert (y == 0.0).any() and (y == 1.0).any()
    elif name == "softmax_onehot":
        multi = L > 1
        assert np.all((att[multi] > 0.999).sum(1) == 1)
    elif name == "softmax_uniform":
        for i in range(B):
            n = min(int(L[i]), T)
            assert np.all(att[i, :n] == np.float32(1) / np.float32(n)) and np.all(att[i, n:] == 0), i
    elif name == "dead_relus":
        assert not p["f1"].any() and not p["a1"].any()
        for k in g:
            if not k.startswith(("fc2", "fc3")) and k != "fc1/bias":
                assert np.all(g[k] == 0), k
        assert np.abs(g["fc3/bias"]).max() > 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", list(hc.CASES))
def test_edge_case_takes_its_forms_and_matches_the_references(name):
    c = hc.case(name)
    if c.row.params:
        _param_case(name, c)
    else:
        _shape_case(name, c)
