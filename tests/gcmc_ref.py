"""The GCMC slice baseline (slice_models/slice_model.py:177-203, base class :11-152) restated literally in float64 torch:
the reference the GCMC tests compare the HIP model against.  It follows TF's graph op for op -- the dense on every
neighbour and then the sum over K, the exp ratio, tf.losses.log_loss with its epsilon, tf.nn.l2_loss over every variable
whose name holds neither "bias" nor "emb" -- and borrows only the GRU cell and TF's Adam from the oracle."""
import math

import numpy as np
import torch

from helpers import check_dropped
from oracle.score_oracle import TFAdam, _gru, batch_to_arrays

LOGLOSS_EPS = 1e-7          # tf.losses.log_loss's default epsilon


class Cfg(object):
    """SliceBaseModel's constructor arguments (slice_model.py:12-13) plus derived widths."""
    model_type = "GCMC"

    def __init__(self, N, D, H, T, K, Fu, Fi):
        self.N, self.D, self.H, self.T, self.K, self.Fu, self.Fi = N, D, H, T, K, Fu, Fi
        self.Du, self.Di = Fu * D, Fi * D

    @property
    def args(self):
        return (self.N, self.D, self.H, self.T, self.K, self.Fu, self.Fi)


def param_spec(c):
    """Trainable variables in TF creation order -> (name, shape, init, l2-regularised); emb_mtx not included."""
    Di, Du, H = c.Di, c.Du, c.H
    out = [("dense/kernel", (Di, Di), "glorot", True), ("dense_1/kernel", (Du, Du), "glorot", True),
           ("dense_2/kernel", (Di, Di), "glorot", True), ("dense_3/kernel", (Du, Du), "glorot", True)]
    for scope, I in (("gru1", Di), ("gru2", Du)):
        out += [(scope + "/gru_cell/gates/kernel", (I + H, 2 * H), "glorot", True),
                (scope + "/gru_cell/gates/bias", (2 * H,), "ones", False),
                (scope + "/gru_cell/candidate/kernel", (I + H, H), "glorot", True),
                (scope + "/gru_cell/candidate/bias", (H,), "zeros", False)]
    out += [("dense_4/kernel", (H, H), "glorot", True), ("dense_5/kernel", (H, H), "glorot", True)]
    return out


def init_params(c, seed):
    """Values of TF's initialiser families (truncated normal table, glorot uniform kernels), float32."""
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
    return out


def forward(c, P, batch, reg_lambda=0.0):
    """P: name -> torch tensor; batch: name -> integer arrays / tensors.  Returns the named intermediates."""
    dt = P["emb_mtx"].dtype
    emb_mask = torch.ones((c.N, 1), dtype=dt)
    emb_mask[0] = 0
    emb = P["emb_mtx"] * emb_mask                                         # slice_model.py:42-45
    ids = lambda k: torch.as_tensor(np.asarray(batch[k]).astype(np.int64))
    look = lambda k, F: torch.nn.functional.embedding(ids(k), emb).reshape(tuple(ids(k).shape[:-1]) + (F * c.D,))
    user_1hop, item_1hop = look("user_1hop", c.Fi), look("item_1hop", c.Fu)
    length = ids("length")
    pre_au = (user_1hop @ P["dense/kernel"]).sum(2)                        # a dense on every neighbour, then the sum (:182-187)
    pre_ai = (item_1hop @ P["dense_1/kernel"]).sum(2)
    a_u, a_i = torch.relu(pre_au), torch.relu(pre_ai)
    pre_zu, pre_zi = a_u @ P["dense_2/kernel"], a_i @ P["dense_3/kernel"]    # (:189-190)
    z_u, z_i = torch.relu(pre_zu), torch.relu(pre_zi)
    gp = lambda s, n: P[s + "/gru_cell/" + n]
    _, h_u = _gru(z_u, length, gp("gru1", "gates/kernel"), gp("gru1", "gates/bias"), gp("gru1", "candidate/kernel"),
                  gp("gru1", "candidate/bias"), c.H)                          # (:194-197)
    _, h_i = _gru(z_i, length, gp("gru2", "gates/kernel"), gp("gru2", "gates/bias"), gp("gru2", "candidate/kernel"),
                  gp("gru2", "candidate/bias"), c.H)
    pos = torch.exp(((h_i @ P["dense_4/kernel"]) * h_u).sum(1))              # (:199-201)
    neg = torch.exp(((h_i @ P["dense_5/kernel"]) * h_u).sum(1))
    y = pos / (pos + neg)
    lab = ids("label").to(dt)
    log_loss = (-lab * torch.log(y + LOGLOSS_EPS) - (1 - lab) * torch.log(1 - y + LOGLOSS_EPS)).mean()    # (:77-86)
    l2 = sum((P[n] ** 2).sum() * 0.5 for n in P if "bias" not in n and "emb" not in n)
    # per sample: the smallest |pre-activation| of the four relus over its live slices, exact zeros left out (an all-zero
    # slice gives 0 on every side, and relu's gradient there is 0 everywhere)
    live = (torch.arange(c.T)[None, :] < length[:, None])[..., None]

    def margin(pre):
        a = pre.detach().abs().double()
        a = torch.where((a == 0) | ~live, torch.full_like(a, float("inf")), a)
        return a.amin(dim=(1, 2))
    per = torch.minimum(torch.minimum(margin(pre_au), margin(pre_ai)), torch.minimum(margin(pre_zu), margin(pre_zi)))
    return dict(a_u=a_u, a_i=a_i, z_u=z_u, z_i=z_i, h_u=h_u, h_i=h_i, y_pred=y, log_loss=log_loss, l2=l2,
                loss=log_loss + reg_lambda * l2, relu_margin_per_sample=per.numpy())


def to_torch(params, dtype=torch.float64, requires_grad=False):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=requires_grad) for k, v in params.items()}


def loss_and_grads(c, params, batch, reg_lambda, dtype=torch.float64):
    """Forward + autograd backward: (out, grads); the emb_mtx gradient is dense [N, D] with row 0 zero."""
    P = to_torch(params, dtype, requires_grad=True)
    out = forward(c, P, batch, reg_lambda)
    out["loss"].backward()
    return out, {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().numpy() for k, v in P.items()}


def away_from_relu_kinks(c, params, batch, thr=1e-5, max_dropped=None):
    """The batch without the samples that have a live relu pre-activation within thr of 0 (and not exactly 0): the gradient
    of a relu network jumps there (tests/helpers.py away_from_relu_kinks).  At most max_dropped samples may go (default: a quarter
    of the batch)."""
    with torch.no_grad():
        per = forward(c, to_torch(params), batch)["relu_margin_per_sample"]
    keep = np.nonzero(per > thr)[0]
    check_dropped(per.size, keep.size, max_dropped)
    return {k: np.ascontiguousarray(np.asarray(v)[keep]) for k, v in batch.items()}, keep


class RefModel(object):
    """The restatement behind the reference's train / eval signatures (slice_model.py:101-133 via SliceBaseModel):
    float64 gradients, cast to float32, then TF's Adam on float32 variables."""

    def __init__(self, c, params):
        self.cfg = c
        self.params = {k: np.array(v, dtype=np.float32) for k, v in params.items()}
        self.opt = TFAdam(self.params)

    def train(self, sess, batch_data, lr, reg_lambda, keep_prob=0.8):
        out, grads = loss_and_grads(self.cfg, self.params, batch_to_arrays(batch_data), reg_lambda)
        self.opt.step(self.params, {k: g.astype(np.float32) for k, g in grads.items()}, lr)
        return float(out["loss"].detach())

    def eval(self, sess, batch_data, reg_lambda):
        b = batch_to_arrays(batch_data)
        with torch.no_grad():
            out = forward(self.cfg, to_torch(self.params), b, reg_lambda)
        return out["y_pred"].numpy().reshape(-1).tolist(), np.asarray(b["label"]).reshape(-1).tolist(), float(out["loss"])
