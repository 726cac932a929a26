"""The Caser point baseline (point_models/point_model.py:140-164, base class :9-121) restated literally in float64 torch: the
reference the Caser tests compare the HIP model against.  It follows TF's graph op for op -- the masked table, conv2d ([50, C]
kernel, VALID) and its max over every position, conv2d_1 ([T, 1] kernel) and the dense on its trailing axis of size 1, bn1 in
inference form, fc1 / fc2 with tf.nn.dropout, fc3, sigmoid, tf.losses.log_loss with its epsilon, tf.nn.l2_loss over every
variable whose name holds neither "bias" nor "emb" -- and borrows only TF's Adam from the oracle.  user_seq_length is part of the
feed and is not read, as in the reference."""
import math

import numpy as np
import torch

from helpers import check_dropped
from oracle.score_oracle import TFAdam

LOGLOSS_EPS = 1e-7          # tf.losses.log_loss's default epsilon
BN_EPS = 1e-3               # tf.layers.batch_normalization's default epsilon (moving mean 0, variance 1: inference form)
FEED = ("user_seq", "user_seq_length", "target_user", "target_item", "label")      # data_loader.py:87
L = 50                      # conv2d's kernel height (point_model.py:147): a constant of the reference, not max_time_len
RELU_THR, WINDOW_THR = 1e-5, 1e-4


class Cfg(object):
    """PointBaseModel's constructor arguments (point_model.py:10-11) plus derived widths; H is accepted and ignored."""
    model_type = "Caser"

    def __init__(self, N, D, H, T, Fu, Fi):
        if T < L:
            raise ValueError("max_time_len %d < %d: conv2d with VALID padding has no output" % (T, L))
        self.N, self.D, self.H, self.T, self.Fu, self.Fi = N, D, H, T, Fu, Fi
        self.Du, self.Di = Fu * D, Fi * D
        self.C, self.NW = self.Di, T - L + 1
        self.Dhead = 1 + 2 * self.Di + self.Du

    @property
    def args(self):
        return (self.N, self.D, self.H, self.T, self.Fu, self.Fi)


def param_spec(c):
    """Trainable variables in TF creation order -> (name, TF's shape, init, l2-regularised); emb_mtx not included."""
    return [("conv2d/kernel", (L, c.C, 1, 1), "glorot", True), ("conv2d/bias", (1,), "zeros", False),
            ("conv2d_1/kernel", (c.T, 1, 1, 1), "glorot", True), ("conv2d_1/bias", (1,), "zeros", False),
            ("dense/kernel", (1, 1), "glorot", True), ("dense/bias", (1,), "zeros", False),
            ("bn1/gamma", (c.Dhead,), "ones", True), ("bn1/beta", (c.Dhead,), "zeros", True),
            ("fc1/kernel", (c.Dhead, 200), "glorot", True), ("fc1/bias", (200,), "zeros", False),
            ("fc2/kernel", (200, 80), "glorot", True), ("fc2/bias", (80,), "zeros", False),
            ("fc3/kernel", (80, 1), "glorot", True), ("fc3/bias", (1,), "zeros", False)]


def glorot_limit(shape):
    """TF's glorot_uniform: fan_in / fan_out of a kernel [..., in, out] are in / out times the receptive field (the product of
    the leading axes): sqrt(6 / (100 C)) for conv2d, sqrt(6 / (2 T)) for conv2d_1, sqrt(3) for the [1, 1] dense."""
    field = int(np.prod(shape[:-2]))
    return math.sqrt(6.0 / (field * shape[-2] + field * shape[-1]))


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
            lim = glorot_limit(shape)
            v = rng.uniform(-lim, lim, shape)
        else:
            v = np.ones(shape) if init == "ones" else np.zeros(shape)
        out[name] = np.ascontiguousarray(v, dtype=np.float32)
    return out


def random_batch(rng, c, B, max_length=None, min_length=None):
    """A batch as the loader shapes it: ids in [1, N), lengths in [min_length, max_length or T] (the loader reports lengths above
    T as they are), and past a sample's length its last item repeated (score_amd/pointdata.py).  min_length defaults to the
    number of windows + 1 where there is more than one window: a history of p + 1 items or fewer makes the windows p, p + 1, ...
    read the same rows, an exact tie of their sums, and where the tied windows hold the maximum the gradient is a matter of
    convention (away_from_kinks would drop the sample)."""
    if min_length is None:
        min_length = 1 if c.NW == 1 else c.NW + 1
    ln = rng.integers(min_length, (max_length or c.T) + 1, B)
    seq = rng.integers(1, c.N, (B, c.T, c.Fi))
    for i in range(B):
        if ln[i] < c.T:
            seq[i, ln[i]:] = seq[i, ln[i] - 1]
    return {"user_seq": seq.astype(np.int32), "user_seq_length": ln.astype(np.int32),
            "target_user": rng.integers(1, c.N, (B, c.Fu)).astype(np.int32),
            "target_item": rng.integers(1, c.N, (B, c.Fi)).astype(np.int32),
            "label": rng.integers(0, 2, (B,)).astype(np.int32)}


def batch_tuple(b):
    return tuple(b[n] for n in FEED)


def batch_to_arrays(batch_data):
    return {n: np.asarray(batch_data[i]).astype(np.int32) for i, n in enumerate(FEED)}


def forward(c, P, batch, reg_lambda=0.0, keep_prob=1.0, dropout_masks=None):
    """P: name -> torch tensor (TF's shapes); batch: name -> integer arrays / tensors; dropout_masks: None or two 0/1 arrays
    [B,200], [B,80] (tf.nn.dropout(x, keep) = x / keep * mask).  Returns the named intermediates."""
    dt = P["emb_mtx"].dtype
    emb_mask = torch.ones((c.N, 1), dtype=dt)
    emb_mask[0] = 0
    emb = P["emb_mtx"] * emb_mask                                         # point_model.py:31-34
    ids = lambda k: torch.as_tensor(np.asarray(batch[k]).astype(np.int64))
    look = lambda k, F: torch.nn.functional.embedding(ids(k), emb).reshape(tuple(ids(k).shape[:-1]) + (F * c.D,))
    x, t_item, t_user = look("user_seq", c.Fi), look("target_item", c.Fi), look("target_user", c.Fu)     # x: [B, T, C]
    # conv2d (:147-149): one [50, C] filter, VALID -> [B, T - 49]; max over all positions -> [B]
    win = x.unfold(1, L, 1)                                               # [B, NW, C, 50]
    hwin = torch.einsum("bpci,ic->bp", win, P["conv2d/kernel"].reshape(L, c.C)) + P["conv2d/bias"].reshape(())
    h = hwin.max(1).values
    # conv2d_1 (:152-154): one [T, 1] filter -> [B, C]; dense on the trailing axis of size 1 (:155-157)
    v = torch.einsum("btc,t->bc", x, P["conv2d_1/kernel"].reshape(c.T)) + P["conv2d_1/bias"].reshape(())
    v2 = v * P["dense/kernel"].reshape(()) + P["dense/bias"].reshape(())
    inp = torch.cat([h[:, None], v2, t_item, t_user], 1)                    # (:160)
    bn = inp * (P["bn1/gamma"] / math.sqrt(1.0 + BN_EPS)) + P["bn1/beta"]    # (:44-52)
    z1 = bn @ P["fc1/kernel"] + P["fc1/bias"]
    f1 = torch.relu(z1)
    if dropout_masks is not None:
        f1 = f1 * torch.as_tensor(np.asarray(dropout_masks[0])).to(dt) / keep_prob
    z2 = f1 @ P["fc2/kernel"] + P["fc2/bias"]
    f2 = torch.relu(z2)
    if dropout_masks is not None:
        f2 = f2 * torch.as_tensor(np.asarray(dropout_masks[1])).to(dt) / keep_prob
    y = torch.sigmoid((f2 @ P["fc3/kernel"] + P["fc3/bias"]).reshape(-1))
    lab = ids("label").to(dt)
    log_loss = (-lab * torch.log(y + LOGLOSS_EPS) - (1 - lab) * torch.log(1 - y + LOGLOSS_EPS)).mean()    # (:54-63)
    l2 = sum((P[n] ** 2).sum() * 0.5 for n in P if "bias" not in n and "emb" not in n)
    # per sample: the smallest |pre-activation| of fc1 / fc2 (the only relus of the model), and the distance between the two
    # largest window sums (infinite where there is one window)
    per = torch.minimum(z1.detach().abs().amin(1), z2.detach().abs().amin(1)).double().numpy()
    hw = hwin.detach().double().numpy()
    top = np.sort(hw, 1)
    wmargin = top[:, -1] - top[:, -2] if c.NW > 1 else np.full(hw.shape[0], np.inf)
    return dict(hwin=hwin, arg=np.argmax(hw, 1).astype(np.int32), v=v, y_pred=y, log_loss=log_loss, l2=l2,
                loss=log_loss + reg_lambda * l2, relu_margin_per_sample=per, window_margin_per_sample=wmargin)


def to_torch(params, dtype=torch.float64, requires_grad=False):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=requires_grad) for k, v in params.items()}


def loss_and_grads(c, params, batch, reg_lambda, keep_prob=1.0, dropout_masks=None, dtype=torch.float64):
    """Forward + autograd backward: (out, grads); the emb_mtx gradient is dense [N, D] with row 0 zero."""
    P = to_torch(params, dtype, requires_grad=True)
    out = forward(c, P, batch, reg_lambda, keep_prob, dropout_masks)
    out["loss"].backward()
    return out, {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().numpy() for k, v in P.items()}


def cap(B):
    """the project's cap on what a kink filter may take from a batch of B"""
    return max(2, B // 50)


def away_from_kinks(c, params, batch, keep_prob=1.0, dropout_masks=None, max_dropped=None):
    """The batch without the samples that own an fc1 / fc2 pre-activation within 1e-5 of 0 (tests/helpers.py
    away_from_relu_kinks: the gradient of a relu network jumps there) or whose two largest window sums are within 1e-4 of each
    other (the max-pool's gradient jumps from one window to the other there).  At most max_dropped samples may go (default:
    cap(B)).  -> (batch, masks, kept)"""
    with torch.no_grad():
        out = forward(c, to_torch(params), batch, 0.0, keep_prob, dropout_masks)
    ok = (out["relu_margin_per_sample"] > RELU_THR) & (out["window_margin_per_sample"] > WINDOW_THR)
    keep = np.nonzero(ok)[0]
    check_dropped(ok.size, keep.size, cap(ok.size) if max_dropped is None else max_dropped)
    b = {k: np.ascontiguousarray(np.asarray(v)[keep]) for k, v in batch.items()}
    dm = [np.ascontiguousarray(np.asarray(m)[keep]) for m in dropout_masks] if dropout_masks is not None else None
    return b, dm, keep


class RefModel(object):
    """The restatement behind the reference's train / eval signatures (point_model.py:88-112): float64 gradients, cast to
    float32, then TF's Adam on float32 variables."""

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
