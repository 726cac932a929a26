"""The DELF point baseline (point_models/point_model.py:200-279, base class :9-63) restated literally in float64 torch: the
reference the DELF tests compare the HIP model against.  It follows TF's graph op for op -- the masked table, the two
tf.sequence_mask masks, attention() with its dense + tanh keys, `queries * key * mask` summed over the width plus the
(1 - mask) * (-2 ** 32 + 1) paddings, softmax over the time axis, the weighted sum of the VALUE (the history itself), the four
pairwise concatenations, fusion_mlp (dense 10 relu, dense 4 relu), their sum, dense(1, sigmoid), tf.losses.log_loss with its
epsilon, tf.nn.l2_loss over every variable whose name holds neither "bias" nor "emb" -- and borrows only TF's Adam from the
oracle.  There is no batch norm and no dropout; hidden_size is accepted and ignored."""
import math

import numpy as np
import torch

from helpers import check_dropped
from oracle.score_oracle import TFAdam

LOGLOSS_EPS = 1e-7          # tf.losses.log_loss's default epsilon
FEED = ("user_seq", "user_seq_length", "item_seq", "item_seq_length", "target_user", "target_item", "label")    # data_loader.py:185
PAD = float(-2 ** 32 + 1)   # point_model.py:246
RELU_THR = 1e-5


class Cfg(object):
    """PointBaseModel's constructor arguments (point_model.py:10-11) plus derived widths; H is accepted and ignored."""
    model_type = "DELF"

    def __init__(self, N, D, H, T, Fu, Fi):
        self.N, self.D, self.H, self.T, self.Fu, self.Fi = N, D, H, T, Fu, Fi
        self.Cu, self.Ci = Fu * D, Fi * D

    @property
    def args(self):
        return (self.N, self.D, self.H, self.T, self.Fu, self.Fi)


def param_spec(c):
    """Trainable variables in TF creation order -> (name, shape, init, l2-regularised); emb_mtx not included.  dense / dense_1:
    the attention keys of user_seq / item_seq; dense_2 .. dense_9: fusion_mlp of inter1 .. inter4; dense_10: the output unit."""
    Cu, Ci = c.Cu, c.Ci
    kernels = [(Ci, Ci), (Cu, Cu), (Cu + Ci, 10), (10, 4), (Ci + Cu, 10), (10, 4), (2 * Cu, 10), (10, 4), (2 * Ci, 10), (10, 4),
               (4, 1)]
    out = []
    for i, sh in enumerate(kernels):
        nm = "dense" if i == 0 else "dense_%d" % i
        out += [(nm + "/kernel", sh, "glorot", True), (nm + "/bias", (sh[1],), "zeros", False)]
    return out


def init_params(c, seed, bias_scale=0.0):
    """Values of TF's initialiser families (truncated normal table, glorot uniform kernels, zero biases), float32; bias_scale
    moves the biases by bias_scale * N(0, 1) (a test that wants every bias gradient to matter)."""
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
            v = bias_scale * rng.standard_normal(shape)
        out[name] = np.ascontiguousarray(v, dtype=np.float32)
    return out


def _history(rng, c, B, F, lo, hi):
    ln = rng.integers(lo, hi + 1, B)
    seq = rng.integers(1, c.N, (B, c.T, F))
    for i in range(B):
        if 0 < ln[i] < c.T:       # (the loader pads by repeating the last id; a length 0 does not come from the loader)
            seq[i, ln[i]:] = seq[i, ln[i] - 1]
    return seq.astype(np.int32), ln.astype(np.int32)


def random_batch(rng, c, B, min_length=(1, 1), max_length=(None, None)):
    """A batch as the loader shapes it: ids in [1, N), per side (user history, item history) lengths in [min_length, max_length
    or T] -- the loader reports lengths above T as they are, so max_length may exceed T -- and past a sample's length its last
    id repeated (score_amd/pointdata.py)."""
    us, ul = _history(rng, c, B, c.Fi, min_length[0], max_length[0] or c.T)
    its, il = _history(rng, c, B, c.Fu, min_length[1], max_length[1] or c.T)
    return {"user_seq": us, "user_seq_length": ul, "item_seq": its, "item_seq_length": il,
            "target_user": rng.integers(1, c.N, (B, c.Fu)).astype(np.int32),
            "target_item": rng.integers(1, c.N, (B, c.Fi)).astype(np.int32),
            "label": rng.integers(0, 2, (B,)).astype(np.int32)}


def batch_tuple(b):
    return tuple(b[n] for n in FEED)


def batch_to_arrays(batch_data):
    return {n: np.asarray(batch_data[i]).astype(np.int32) for i, n in enumerate(FEED)}


def attention(c, key, value, query, mask, W, b):
    """point_model.py:240-249; mask [B, T, 1].  -> (output [B, C], weights [B, T])"""
    queries = query[:, None, :].expand(-1, c.T, -1)
    key = torch.tanh(key @ W + b)
    paddings = (1 - mask) * PAD
    att = torch.softmax((queries * key * mask).sum(2, keepdim=True) + paddings, dim=1)
    return (value * att).sum(1), att[:, :, 0]


def forward(c, P, batch, reg_lambda=0.0):
    """P: name -> torch tensor; batch: name -> integer arrays / tensors.  Returns the named intermediates."""
    dt = P["emb_mtx"].dtype
    emb_mask = torch.ones((c.N, 1), dtype=dt)
    emb_mask[0] = 0
    emb = P["emb_mtx"] * emb_mask                                         # point_model.py:31-34
    ids = lambda k: torch.as_tensor(np.asarray(batch[k]).astype(np.int64))
    look = lambda k, F: torch.nn.functional.embedding(ids(k), emb).reshape(tuple(ids(k).shape[:-1]) + (F * c.D,))
    xu, xi = look("user_seq", c.Fi), look("item_seq", c.Fu)                # [B, T, Ci], [B, T, Cu]
    ti, tu = look("target_item", c.Fi), look("target_user", c.Fu)
    pos = torch.arange(c.T)[None, :]
    mask = lambda k: (pos < ids(k)[:, None]).to(dt)[:, :, None]           # tf.sequence_mask (:213-214)
    ru, au = attention(c, xu, xu, ti, mask("user_seq_length"), P["dense/kernel"], P["dense/bias"])          # (:216)
    ri, ai = attention(c, xi, xi, tu, mask("item_seq_length"), P["dense_1/kernel"], P["dense_1/bias"])      # (:217)
    inters = [torch.cat([tu, ti], 1), torch.cat([ru, ri], 1), torch.cat([tu, ri], 1), torch.cat([ti, ru], 1)]    # (:220-223)
    f, pre = 0, []
    for k, x in enumerate(inters):                                        # fusion_mlp (:235-238)
        z1 = x @ P["dense_%d/kernel" % (2 + 2 * k)] + P["dense_%d/bias" % (2 + 2 * k)]
        z2 = torch.relu(z1) @ P["dense_%d/kernel" % (3 + 2 * k)] + P["dense_%d/bias" % (3 + 2 * k)]
        f = f + torch.relu(z2)
        pre += [z1, z2]
    y = torch.sigmoid(f @ P["dense_10/kernel"] + P["dense_10/bias"]).reshape(-1)       # (:232)
    lab = ids("label").to(dt)
    log_loss = (-lab * torch.log(y + LOGLOSS_EPS) - (1 - lab) * torch.log(1 - y + LOGLOSS_EPS)).mean()    # (:54-63)
    l2 = sum((P[n] ** 2).sum() * 0.5 for n in P if "bias" not in n and "emb" not in n)
    allpre = torch.cat(pre, 1).detach()                                   # [B, 56]: every relu's argument
    assert allpre.shape[1] == 56
    return dict(att_user=au, att_item=ai, ru=ru, ri=ri, y_pred=y, log_loss=log_loss, l2=l2, loss=log_loss + reg_lambda * l2,
                relu_margin_per_sample=allpre.abs().amin(1).double().numpy())


def to_torch(params, dtype=torch.float64, requires_grad=False):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=requires_grad) for k, v in params.items()}


def loss_and_grads(c, params, batch, reg_lambda, dtype=torch.float64):
    """Forward + autograd backward: (out, grads); the emb_mtx gradient is dense [N, D] with row 0 zero."""
    P = to_torch(params, dtype, requires_grad=True)
    out = forward(c, P, batch, reg_lambda)
    out["loss"].backward()
    return out, {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().numpy() for k, v in P.items()}


def cap(B):
    """the project's cap on what a kink filter may take from a batch of B"""
    return max(2, B // 50)


def away_from_kinks(c, params, batch, max_dropped=None):
    """The batch without the samples that own one of the 56 fusion pre-activations within 1e-5 of 0 (the gradient of a relu
    network jumps there).  At most cap(B) samples may go, enforced by assertion.  -> (batch, kept)"""
    with torch.no_grad():
        out = forward(c, to_torch(params), batch, 0.0)
    ok = out["relu_margin_per_sample"] > RELU_THR
    keep = np.nonzero(ok)[0]
    limit = cap(ok.size) if max_dropped is None else max_dropped
    assert limit <= cap(ok.size)
    check_dropped(ok.size, keep.size, limit)
    return {k: np.ascontiguousarray(np.asarray(v)[keep]) for k, v in batch.items()}, keep


class RefModel(object):
    """The restatement behind the reference's train / eval signatures (point_model.py:251-279): float64 gradients, cast to
    float32, then TF's Adam on float32 variables."""

    def __init__(self, c, params):
        self.cfg = c
        self.params = {k: np.array(v, dtype=np.float32) for k, v in params.items()}
        self.opt = TFAdam(self.params)

    def train(self, sess, batch_data, lr, reg_lambda, keep_prob=1.0, dropout_masks=None):
        out, grads = loss_and_grads(self.cfg, self.params, batch_to_arrays(batch_data), reg_lambda)
        self.opt.step(self.params, {k: g.astype(np.float32) for k, g in grads.items()}, lr)
        return float(out["loss"].detach())

    def eval(self, sess, batch_data, reg_lambda):
        b = batch_to_arrays(batch_data)
        with torch.no_grad():
            out = forward(self.cfg, to_torch(self.params), b, reg_lambda)
        return out["y_pred"].numpy().reshape(-1).tolist(), np.asarray(b["label"]).reshape(-1).tolist(), float(out["loss"])
