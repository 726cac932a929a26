"""The SASRec point baseline (point_models/point_model.py:313-469, on PointBaseModel :9-63) restated literally in float64 torch:
the reference the SASRec tests compare the HIP model against.  It follows TF's graph op for op -- the masked table, normalize
(:441-469: population variance over the last axis, epsilon 1e-8, beta = ln/Variable created before gamma = ln/Variable_1),
multihead_attention (:362-439: Q from the normalised rows, K and V from the raw ones, split into two heads along the channels
and stacked along the batch, the scale, the key mask with -2^32 + 1, softmax over all keys, the query mask, tf.nn.dropout on the
[2 B, T, T] weights, the residual), rep / final under tf.sequence_mask (:318-322), the positive rows t = 1 .. T - 1, the
"negative" rows t = 2 .. T - 1 (the same expression) and the final row through the shared prediction_layer (:353-360: no batch
norm), the three tf.losses.log_loss means and tf.nn.l2_loss over every variable whose name holds neither "bias" nor "emb" -- the
two layer-norm variables among them -- and borrows only TF's Adam from the oracle.

Dropout masks are explicit: (m0 [R, 200], m1 [R, 80], ma [2, B, T, T]) with R = B (T - 1) + B (T - 2) + B rows ordered positive
(b-major, t = 1 .. T - 1), negative (t = 2 .. T - 1), final; ma[h, b] is row h B + b of TF's [2 B, T, T] weights."""
import math

import numpy as np
import torch

from gru4rec_ref import FEED, batch_to_arrays, batch_tuple, random_batch      # the 5-tuple and its batches are GRU4Rec's
from helpers import check_dropped
from oracle.score_oracle import TFAdam

LOGLOSS_EPS = 1e-7          # tf.losses.log_loss's default epsilon
LN_EPS = 1e-8               # normalize's epsilon
PAD_SCORE = float(-2 ** 32 + 1)
RELU_THR = 1e-5             # an fc1 / fc2 pre-activation this close to 0: a kink of the relu
MASK_THR = 1e-4             # a row sum this close to 0 (and not exactly 0): the key / query mask could flip in fp32


class Cfg(object):
    """PointBaseModel's constructor arguments (point_model.py:10-11) plus derived widths; H is accepted and ignored."""
    model_type = "SASRec"

    def __init__(self, N, D, H, T, Fu, Fi):
        self.N, self.D, self.H, self.T, self.Fu, self.Fi = N, D, H, T, Fu, Fi
        self.Cu, self.Ci = Fu * D, Fi * D
        self.Dh = 2 * self.Ci + self.Cu

    @property
    def args(self):
        return (self.N, self.D, self.H, self.T, self.Fu, self.Fi)


def rows(c, B):
    """(positive, negative, final) row counts of the head's three applications"""
    return B * (c.T - 1), B * (c.T - 2), B


def param_spec(c):
    """Trainable variables in TF creation order -> (name, shape, init, l2-regularised); emb_mtx not included."""
    C = c.Ci
    out = [("ln/Variable", (C,), "zeros", True), ("ln/Variable_1", (C,), "ones", True)]
    for s in ("dense", "dense_1", "dense_2"):
        out += [("multihead_attention/%s/kernel" % s, (C, C), "glorot", True), ("multihead_attention/%s/bias" % s, (C,), "zeros", False)]
    for s, i, o in (("fc1", c.Dh, 200), ("fc2", 200, 80), ("fc3", 80, 1)):
        out += [("prediction_layer/%s/kernel" % s, (i, o), "glorot", True), ("prediction_layer/%s/bias" % s, (o,), "zeros", False)]
    return out


def init_params(c, seed, perturbed=False):
    """Values of TF's initialiser families (truncated normal table, glorot uniform kernels, zeros, ones), float32.  perturbed:
    gamma = 1 + 0.1 n, beta = 0.5 + 0.1 n, biases 0.1 n (n standard normal) -- every sum_c Qin is then of order C / 2, so the
    query mask is decided by a wide margin, and no bias gradient is tested against an all-zero bias."""
    rng = np.random.Generator(np.random.PCG64(seed))
    emb = rng.standard_normal((c.N, c.D))
    bad = np.abs(emb) > 2.0
    while bad.any():
        emb[bad] = rng.standard_normal(int(bad.sum()))
        bad = np.abs(emb) > 2.0
    out = {"emb_mtx": emb.astype(np.float32)}
    for name, shape, init, _ in param_spec(c):
        if init == "glorot":
            lim = math.sqrt(6.0 / (shape[0] + shape[1]))
            v = rng.uniform(-lim, lim, shape)
        else:
            v = np.ones(shape) if init == "ones" else np.zeros(shape)
        out[name] = np.ascontiguousarray(v, dtype=np.float32)
    if perturbed:
        for name, shape, init, _ in param_spec(c):
            if name == "ln/Variable_1":
                out[name] = (1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
            elif name == "ln/Variable":
                out[name] = (0.5 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
            elif name.endswith("/bias"):
                out[name] = (0.1 * rng.standard_normal(shape)).astype(np.float32)
    return out


def random_masks(rng, c, B, keep_prob):
    P, Nn, F = rows(c, B)
    R = P + Nn + F
    return [(rng.random((R, 200)) < keep_prob).astype(np.uint8), (rng.random((R, 80)) < keep_prob).astype(np.uint8),
            (rng.random((2, B, c.T, c.T)) < keep_prob).astype(np.uint8)]


def select_masks(c, masks, B, keep):
    """the masks of the samples `keep` of a batch of B"""
    if masks is None:
        return None
    P, Nn, _ = rows(c, B)
    keep = np.asarray(keep)
    idx = np.concatenate([(keep[:, None] * (c.T - 1) + np.arange(c.T - 1)[None, :]).reshape(-1),
                          P + (keep[:, None] * (c.T - 2) + np.arange(c.T - 2)[None, :]).reshape(-1), P + Nn + keep])
    return [np.ascontiguousarray(np.asarray(masks[0])[idx]), np.ascontiguousarray(np.asarray(masks[1])[idx]),
            np.ascontiguousarray(np.asarray(masks[2])[:, keep])]


def forward(c, P, batch, reg_lambda=0.0, keep_prob=1.0, dropout_masks=None):
    """P: name -> torch tensor; batch: name -> integer arrays / tensors.  Returns the named intermediates."""
    dt = P["emb_mtx"].dtype
    emb_mask = torch.ones((c.N, 1), dtype=dt)
    emb_mask[0] = 0
    emb = P["emb_mtx"] * emb_mask                                         # point_model.py:31-34
    ids = lambda k: torch.as_tensor(np.asarray(batch[k]).astype(np.int64))
    look = lambda k, F: torch.nn.functional.embedding(ids(k), emb).reshape(tuple(ids(k).shape[:-1]) + (F * c.D,))
    X, t_item, t_user = look("user_seq", c.Fi), look("target_item", c.Fi), look("target_user", c.Fu)
    B, T, C = X.shape
    dh = C // 2
    mask_t = lambda i: None if dropout_masks is None else torch.as_tensor(np.asarray(dropout_masks[i])).to(dt)
    # normalize (:441-469)
    mean = X.mean(-1, keepdim=True)
    var = ((X - mean) ** 2).mean(-1, keepdim=True)
    Nrm = (X - mean) / ((var + LN_EPS) ** 0.5)
    Qin = P["ln/Variable_1"] * Nrm + P["ln/Variable"]
    # multihead_attention (:362-439)
    ma = lambda s: (P["multihead_attention/%s/kernel" % s], P["multihead_attention/%s/bias" % s])
    Q = Qin @ ma("dense")[0] + ma("dense")[1]
    K = X @ ma("dense_1")[0] + ma("dense_1")[1]
    V = X @ ma("dense_2")[0] + ma("dense_2")[1]
    split = lambda M: torch.cat(torch.split(M, dh, dim=2), dim=0)          # [2 B, T, C / 2]
    Q_, K_, V_ = split(Q), split(K), split(V)
    S = Q_ @ K_.transpose(1, 2) / (dh ** 0.5)
    xsum = X.sum(-1)
    key_masks = torch.sign(torch.abs(xsum)).repeat(2, 1)[:, None, :].expand(2 * B, T, T)
    S = torch.where(key_masks == 0, torch.full_like(S, PAD_SCORE), S)
    Pw = torch.softmax(S, dim=-1)
    qsum = Qin.sum(-1)
    query_masks = torch.sign(torch.abs(qsum)).repeat(2, 1)[:, :, None]
    A = Pw * query_masks
    if dropout_masks is not None:
        A = A * mask_t(2).reshape(2 * B, T, T) / keep_prob
    O = A @ V_
    O = torch.cat(torch.split(O, B, dim=0), dim=2)
    Y = O + Qin
    # (:318-331)
    length = ids("user_seq_length")
    m = (torch.arange(T)[None, :] < length[:, None]).to(dt)[:, :, None]
    rep = Y * m
    final = rep.sum(1)
    tu_t = t_user[:, None, :].expand(B, T, c.Cu)
    pos_in = torch.cat([rep[:, 1:], Y[:, 1:], tu_t[:, 1:]], 2).reshape(B * (T - 1), c.Dh)
    neg_in = torch.cat([rep[:, 2:], Y[:, 2:], tu_t[:, 2:]], 2).reshape(B * (T - 2), c.Dh)
    fin_in = torch.cat([final, t_item, t_user], 1)
    nP, nN, _ = rows(c, B)
    m0, m1 = mask_t(0), mask_t(1)
    fc = lambda s: (P["prediction_layer/%s/kernel" % s], P["prediction_layer/%s/bias" % s])

    def head(inp, lo, hi):                                                # (:353-360)
        z1 = inp @ fc("fc1")[0] + fc("fc1")[1]
        f1 = torch.relu(z1)
        if m0 is not None:
            f1 = f1 * m0[lo:hi] / keep_prob
        z2 = f1 @ fc("fc2")[0] + fc("fc2")[1]
        f2 = torch.relu(z2)
        if m1 is not None:
            f2 = f2 * m1[lo:hi] / keep_prob
        z3 = (f2 @ fc("fc3")[0] + fc("fc3")[1]).reshape(-1)
        return torch.sigmoid(z3), z1, z2, z3

    p_pos, z1p, z2p, z3p = head(pos_in, 0, nP)
    p_neg, z1n, z2n, z3n = head(neg_in, nP, nP + nN)
    y, z1f, z2f, z3f = head(fin_in, nP + nN, nP + nN + B)
    loss_pos = (-torch.log(p_pos + LOGLOSS_EPS)).mean()                   # log_loss(ones, preds_pos)  (:338)
    loss_neg = (-torch.log(1 - p_neg + LOGLOSS_EPS)).mean()               # log_loss(zeros, preds_neg)
    lab = ids("label").to(dt)
    log_loss = (-lab * torch.log(y + LOGLOSS_EPS) - (1 - lab) * torch.log(1 - y + LOGLOSS_EPS)).mean()    # (:345)
    l2 = sum((P[n] ** 2).sum() * 0.5 for n in P if "bias" not in n and "emb" not in n)
    # per sample: the smallest |pre-activation| of fc1 / fc2 over the rows of its three applications
    mn = lambda z, k: z.detach().abs().amin(1).reshape(B, k).amin(1)
    relu_margin = torch.stack([mn(z1p, T - 1), mn(z2p, T - 1), mn(z1n, T - 2), mn(z2n, T - 2), mn(z1f, 1), mn(z2f, 1)]).amin(0)
    return dict(X=X, Qin=Qin, Y=Y, att=A.reshape(2, B, T, T).transpose(0, 1), softmax=Pw.reshape(2, B, T, T).transpose(0, 1),
                final=final, y_pred=y, p_pos=p_pos, p_neg=p_neg, logit=torch.cat([z3p, z3n, z3f]), loss_pos=loss_pos, loss_neg=loss_neg,
                log_loss=log_loss, l2=l2, loss=loss_pos + loss_neg + log_loss + reg_lambda * l2, xsum=xsum.detach(), qsum=qsum.detach(),
                relu_margin_per_sample=relu_margin.double().numpy())


def to_torch(params, dtype=torch.float64, requires_grad=False):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=requires_grad) for k, v in params.items()}


def loss_and_grads(c, params, batch, reg_lambda, keep_prob=1.0, dropout_masks=None, dtype=torch.float64):
    """Forward + autograd backward: (out, grads); the emb_mtx gradient is dense [N, D] with row 0 zero."""
    P = to_torch(params, dtype, requires_grad=True)
    out = forward(c, P, batch, reg_lambda, keep_prob, dropout_masks)
    out["loss"].backward()
    return out, {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().numpy() for k, v in P.items()}


def edge_free(c, params, batch, keep_prob=1.0, dropout_masks=None):
    """per sample: True where no non-smooth point is near.  (1) an fc1 / fc2 pre-activation within RELU_THR of 0 in any of the
    three applications, under the masks in use; (2) a row that is not all id 0 with |sum_c Qin| < MASK_THR (the query mask), or
    an all-zero row whose sum_c Qin (= sum beta) is that small without being exactly 0 -- exactly 0 (beta = 0) is decided alike
    in every precision; (3) a row with 0 < |sum_c X| < MASK_THR (the key mask)."""
    with torch.no_grad():
        out = forward(c, to_torch(params), batch, 0.0, keep_prob, dropout_masks)
    xs, qs = out["xsum"].numpy(), out["qsum"].numpy()
    zero_row = (np.asarray(batch["user_seq"]) == 0).all(2)
    q_edge = np.where(zero_row, (qs != 0) & (np.abs(qs) < MASK_THR), np.abs(qs) < MASK_THR)
    x_edge = (xs != 0) & (np.abs(xs) < MASK_THR)
    return (out["relu_margin_per_sample"] > RELU_THR) & ~q_edge.any(1) & ~x_edge.any(1)


def away_from_edges(c, params, batch, keep_prob=1.0, dropout_masks=None, max_dropped=None):
    """The batch (and its masks) without the samples that own an edge (edge_free).  At most max_dropped samples may go -- the
    project's default: a quarter of the batch, one sample at least kept (helpers.check_dropped).  -> (batch, masks, kept)"""
    ok = edge_free(c, params, batch, keep_prob, dropout_masks)
    keep = np.nonzero(ok)[0]
    check_dropped(ok.size, keep.size, max_dropped)
    b = {k: np.ascontiguousarray(np.asarray(v)[keep]) for k, v in batch.items()}
    return b, select_masks(c, dropout_masks, ok.size, keep), keep


class RefModel(object):
    """The restatement behind the reference's train / eval signatures (point_model.py:88-112): float64 gradients, cast to
    float32, then TF's Adam on float32 variables.  min_qsum: the smallest |sum_c Qin| any training step has seen."""

    def __init__(self, c, params):
        self.cfg = c
        self.params = {k: np.array(v, dtype=np.float32) for k, v in params.items()}
        self.opt = TFAdam(self.params)
        self.min_qsum = float("inf")

    def train(self, sess, batch_data, lr, reg_lambda, keep_prob=1.0, dropout_masks=None):
        assert keep_prob == 1.0 or dropout_masks is not None, "the restatement draws no masks of its own"
        out, grads = loss_and_grads(self.cfg, self.params, batch_to_arrays(batch_data), reg_lambda, keep_prob, dropout_masks)
        self.min_qsum = min(self.min_qsum, float(out["qsum"].abs().min()))
        self.opt.step(self.params, {k: g.astype(np.float32) for k, g in grads.items()}, lr)
        return float(out["loss"].detach())

    def eval(self, sess, batch_data, reg_lambda):
        b = batch_to_arrays(batch_data)
        with torch.no_grad():
            out = forward(self.cfg, to_torch(self.params), b, reg_lambda)
        return out["y_pred"].numpy().reshape(-1).tolist(), np.asarray(b["label"]).reshape(-1).tolist(), float(out["loss"])
