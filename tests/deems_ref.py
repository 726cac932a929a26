"""The DEEMS point baseline (point_models/point_model.py:281-311, on DELF :200-249, on PointBaseModel :9-63) restated literally in
float64 torch: the reference the DEEMS tests compare the HIP model against.  It follows TF's graph op for op -- the masked table,
the two dynamic_rnn's (gru1 over user_seq under user_seq_length, gru2 over item_seq under item_seq_length), build_fc_net twice
(batch normalisation in inference form, dense 200 relu, tf.nn.dropout, dense 80 relu, tf.nn.dropout, dense 1, sigmoid) on
[h_u | target_user] and [h_i | target_item], y_pred = 0.5 (y_u + y_i), tf.losses.log_loss with its epsilon, tf.nn.l2_loss over
every variable whose name holds neither "bias" nor "emb" -- and borrows only the GRU cell and TF's Adam from the oracle.

Two things of the reference are restated as they are, not as one might expect them:
  * build_logloss() creates train_step from log_loss + reg_lambda * l2 (`train_loss` here), and only AFTERWARDS does :300 add
    0.05 * reduce_sum((y_i - y_u) ** 2) to self.loss.  train() / eval() return `loss`, which has the term (a SUM over the batch);
    the gradient Adam applies is that of `train_loss`, which has not.
  * DELF.__init__ runs first, so its 22 variables (dense .. dense_10) exist.  The prediction never reads them; through the L2
    filter their kernels add to the loss and get reg_lambda * W, their biases get no gradient at all (taken as zero)."""
import math

import numpy as np
import torch

import delf_ref
from delf_ref import FEED, batch_to_arrays, batch_tuple, cap, random_batch      # the 7-tuple and its batches are DELF's
from helpers import check_dropped
from oracle.score_oracle import TFAdam, _gru

LOGLOSS_EPS = 1e-7          # tf.losses.log_loss's default epsilon
BN_EPS = 1e-3               # tf.layers.batch_normalization's default epsilon (moving mean 0, variance 1: inference form)
CONSISTENCY = 0.05          # point_model.py:300
RELU_THR = 1e-5
FC1, FC2 = 200, 80
TOWERS = (("batch_normalization", ("dense_11", "dense_12", "dense_13")),       # user tower: [h_u | target_user]
          ("batch_normalization_1", ("dense_14", "dense_15", "dense_16")))     # item tower: [h_i | target_item]


class Cfg(object):
    """PointBaseModel's constructor arguments (point_model.py:10-11) plus derived widths."""
    model_type = "DEEMS"

    def __init__(self, N, D, H, T, Fu, Fi):
        self.N, self.D, self.H, self.T, self.Fu, self.Fi = N, D, H, T, Fu, Fi
        self.Cu, self.Ci = Fu * D, Fi * D

    @property
    def args(self):
        return (self.N, self.D, self.H, self.T, self.Fu, self.Fi)


def param_spec(c):
    """Trainable variables in TF creation order -> (name, shape, init, l2-regularised); emb_mtx not included.  DELF's 22, the two
    GRU cells, then per tower batch_normalization[_1]/{gamma, beta} and its three denses: 46 entries."""
    H = c.H
    out = list(delf_ref.param_spec(c))
    for scope, I in (("gru1", c.Ci), ("gru2", c.Cu)):
        out += [(scope + "/gru_cell/gates/kernel", (I + H, 2 * H), "glorot", True),
                (scope + "/gru_cell/gates/bias", (2 * H,), "ones", False),
                (scope + "/gru_cell/candidate/kernel", (I + H, H), "glorot", True),
                (scope + "/gru_cell/candidate/bias", (H,), "zeros", False)]
    for (bn, dense), Dh in zip(TOWERS, (H + c.Cu, H + c.Ci)):
        out += [(bn + "/gamma", (Dh,), "ones", True), (bn + "/beta", (Dh,), "zeros", True)]
        for nm, sh in zip(dense, ((Dh, FC1), (FC1, FC2), (FC2, 1))):
            out += [(nm + "/kernel", sh, "glorot", True), (nm + "/bias", (sh[1],), "zeros", False)]
    assert len(out) == 46
    return out


def init_params(c, seed, bias_scale=0.0):
    """Values of TF's initialiser families (truncated normal table, glorot uniform kernels, gate biases one, the rest zero),
    float32; bias_scale moves every bias and beta by bias_scale * N(0, 1) (a test that wants every bias gradient to matter)."""
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
            v = (np.ones(shape) if init == "ones" else np.zeros(shape))
            if "bias" in name or "beta" in name:
                v = v + bias_scale * rng.standard_normal(shape)
        out[name] = np.ascontiguousarray(v, dtype=np.float32)
    return out


def tower(P, bn, dense, inp, keep_prob, masks):
    """build_fc_net (point_model.py:302-311); masks: None or this tower's two 0/1 arrays [B, 200], [B, 80].
    -> (y [B], the 280 relu pre-activations [B, 280])"""
    dt = inp.dtype
    x = inp * (P[bn + "/gamma"] / math.sqrt(1.0 + BN_EPS)) + P[bn + "/beta"]
    z1 = x @ P[dense[0] + "/kernel"] + P[dense[0] + "/bias"]
    f1 = torch.relu(z1)
    if masks is not None:
        f1 = f1 * torch.as_tensor(np.asarray(masks[0])).to(dt) / keep_prob
    z2 = f1 @ P[dense[1] + "/kernel"] + P[dense[1] + "/bias"]
    f2 = torch.relu(z2)
    if masks is not None:
        f2 = f2 * torch.as_tensor(np.asarray(masks[1])).to(dt) / keep_prob
    y = torch.sigmoid((f2 @ P[dense[2] + "/kernel"] + P[dense[2] + "/bias"]).reshape(-1))
    return y, torch.cat([z1, z2], 1).detach()


def forward(c, P, batch, reg_lambda=0.0, keep_prob=1.0, dropout_masks=None):
    """P: name -> torch tensor; batch: name -> integer arrays / tensors; dropout_masks: None or two 0/1 arrays [2, B, 200],
    [2, B, 80], the user tower first (tf.nn.dropout(x, keep) = x / keep * mask).  Returns the named intermediates."""
    dt = P["emb_mtx"].dtype
    emb_mask = torch.ones((c.N, 1), dtype=dt)
    emb_mask[0] = 0
    emb = P["emb_mtx"] * emb_mask                                         # point_model.py:31-34
    ids = lambda k: torch.as_tensor(np.asarray(batch[k]).astype(np.int64))
    look = lambda k, F: torch.nn.functional.embedding(ids(k), emb).reshape(tuple(ids(k).shape[:-1]) + (F * c.D,))
    xu, xi = look("user_seq", c.Fi), look("item_seq", c.Fu)                # [B, T, Ci], [B, T, Cu]
    ti, tu = look("target_item", c.Fi), look("target_user", c.Fu)
    gp = lambda s, n: P[s + "/gru_cell/" + n]
    _, h_u = _gru(xu, ids("user_seq_length"), gp("gru1", "gates/kernel"), gp("gru1", "gates/bias"), gp("gru1", "candidate/kernel"),
                  gp("gru1", "candidate/bias"), c.H)                         # (:287-288)
    _, h_i = _gru(xi, ids("item_seq_length"), gp("gru2", "gates/kernel"), gp("gru2", "gates/bias"), gp("gru2", "candidate/kernel"),
                  gp("gru2", "candidate/bias"), c.H)                         # (:289-290)
    m = lambda k: None if dropout_masks is None else (np.asarray(dropout_masks[0])[k], np.asarray(dropout_masks[1])[k])
    y_u, pre_u = tower(P, TOWERS[0][0], TOWERS[0][1], torch.cat([h_u, tu], 1), keep_prob, m(0))      # (:292, 295)
    y_i, pre_i = tower(P, TOWERS[1][0], TOWERS[1][1], torch.cat([h_i, ti], 1), keep_prob, m(1))      # (:293, 296)
    y = 0.5 * (y_u + y_i)                                                                           # (:297)
    lab = ids("label").to(dt)
    log_loss = (-lab * torch.log(y + LOGLOSS_EPS) - (1 - lab) * torch.log(1 - y + LOGLOSS_EPS)).mean()    # (:54-63)
    l2 = sum((P[n] ** 2).sum() * 0.5 for n in P if "bias" not in n and "emb" not in n)
    train_loss = log_loss + reg_lambda * l2                 # what train_step minimises (:299)
    consistency = CONSISTENCY * ((y_i - y_u) ** 2).sum()    # (:300)
    allpre = torch.cat([pre_u, pre_i], 1)                   # [B, 560]: every relu's argument
    assert allpre.shape[1] == 560
    return dict(h_u=h_u, h_i=h_i, y_u=y_u, y_i=y_i, y_pred=y, log_loss=log_loss, l2=l2, consistency=consistency,
                train_loss=train_loss, loss=train_loss + consistency,
                relu_margin_per_sample=allpre.abs().amin(1).double().numpy())


def to_torch(params, dtype=torch.float64, requires_grad=False):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=requires_grad) for k, v in params.items()}


def loss_and_grads(c, params, batch, reg_lambda, keep_prob=1.0, dropout_masks=None, dtype=torch.float64, of="train_loss"):
    """Forward + autograd backward of `train_loss` (of="loss": of the reported loss, which the reference never differentiates):
    (out, grads); out["loss"] is the reported loss either way.  The emb_mtx gradient is dense [N, D] with row 0 zero; a variable
    the differentiated loss does not reach (DELF's biases) has a zero gradient."""
    P = to_torch(params, dtype, requires_grad=True)
    out = forward(c, P, batch, reg_lambda, keep_prob, dropout_masks)
    out[of].backward()
    return out, {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().numpy() for k, v in P.items()}


def away_from_kinks(c, params, batch, keep_prob=1.0, dropout_masks=None, max_dropped=None):
    """The batch without the samples that own one of the 560 relu pre-activations (two towers x (200 + 80)) within 1e-5 of 0
    (the gradient of a relu network jumps there).  At most cap(B) = max(2, B // 50) samples may go, enforced by assertion.
    -> (batch, masks, kept)"""
    with torch.no_grad():
        out = forward(c, to_torch(params), batch, 0.0, keep_prob, dropout_masks)
    ok = out["relu_margin_per_sample"] > RELU_THR
    keep = np.nonzero(ok)[0]
    limit = cap(ok.size) if max_dropped is None else max_dropped
    assert limit <= cap(ok.size)
    check_dropped(ok.size, keep.size, limit)
    b = {k: np.ascontiguousarray(np.asarray(v)[keep]) for k, v in batch.items()}
    dm = [np.ascontiguousarray(np.asarray(m)[:, keep]) for m in dropout_masks] if dropout_masks is not None else None
    return b, dm, keep


class RefModel(object):
    """The restatement behind the reference's train / eval signatures (point_model.py:251-279): float64 gradients of train_loss,
    cast to float32, then TF's Adam on float32 variables; the loss returned is the reported one."""

    def __init__(self, c, params):
        self.cfg = c
        self.params = {k: np.array(v, dtype=np.float32) for k, v in params.items()}
        self.opt = TFAdam(self.params)

    def train(self, sess, batch_data, lr, reg_lambda, keep_prob=1.0, dropout_masks=None):
        assert keep_prob == 1.0 or dropout_masks is not None, "the restatement draws no masks of its own"
        out, grads = loss_and_grads(self.cfg, self.params, batch_to_arrays(batch_data), reg_lambda, keep_prob, dropout_masks)
        self.opt.step(self.params, {k: g.astype(np.float32) for k, g in grads.items()}, lr)
        return float(out["loss"].detach())

    def eval(self, sess, batch_data, reg_lambda):
        b = batch_to_arrays(batch_data)
        with torch.no_grad():
            out = forward(self.cfg, to_torch(self.params), b, reg_lambda)
        return out["y_pred"].numpy().reshape(-1).tolist(), np.asarray(b["label"]).reshape(-1).tolist(), float(out["loss"])
