"""The SVD++ point baseline (point_models/point_model.py:167-198, on PointBaseModel :9-63) restated literally in float64 torch:
the reference the SVD++ tests compare the HIP model against.  It follows TF's graph op for op -- the masked table, one scalar
variable per feature field (user_feat_w_i, item_feat_w_j, shape [], truncated normal), the weighted field sums of the target rows
and of the history, tf.sequence_mask, reduce_sum over T, tf.norm(x, 1, (1, 2)), the division by its square root, the dot product,
sigmoid, tf.losses.log_loss with its epsilon, tf.nn.l2_loss over every variable whose name holds neither "bias" nor "emb" (all
the scalars, not the table) -- and borrows only TF's Adam from the oracle.

tf.norm with ord = 1 and a two-element axis is the MATRIX 1-norm (linalg_ops.norm: reduce_max over the second named axis of
the reduce_sum of |x| over the first): here max over the D columns of sum_t |s_t,d|, np.linalg.norm(s, 1, axis=(1, 2)).
reduce_max's gradient is shared equally among the entries that attain the maximum, which is what torch.amax does; abs has
gradient sign(x), 0 at 0.  A sample whose masked history is all zero has n = 0: 0 / sqrt(0) = NaN, as in TF."""
import numpy as np
import torch

from gru4rec_ref import FEED, batch_to_arrays, batch_tuple, random_batch      # the 5-tuple and its batches are GRU4Rec's
from helpers import check_dropped
from oracle.score_oracle import TFAdam

LOGLOSS_EPS = 1e-7          # tf.losses.log_loss's default epsilon
TIE_REL = 1e-4              # a runner-up column sum this close to n (relative), and not equal to it: a kink of the maximum
ABS_THR = 1e-6              # a live |s_t,d| of a maximal column below this, and not zero: a kink of the absolute value


class Cfg(object):
    """PointBaseModel's constructor arguments (point_model.py:10-11) plus derived widths; H is accepted and ignored."""
    model_type = "SVDpp"

    def __init__(self, N, D, H, T, Fu, Fi):
        self.N, self.D, self.H, self.T, self.Fu, self.Fi = N, D, H, T, Fu, Fi
        self.Cu, self.Ci = Fu * D, Fi * D

    @property
    def args(self):
        return (self.N, self.D, self.H, self.T, self.Fu, self.Fi)


def cap(B):
    """how many samples of a batch of B the kink filter may drop"""
    return 0 if B <= 3 else max(2, B // 50)


def param_spec(c):
    """Trainable variables in TF creation order -> (name, shape, init, l2-regularised); emb_mtx not included."""
    return ([("user_feat_w_%d" % i, (), "truncated_normal", True) for i in range(c.Fu)] +
            [("item_feat_w_%d" % j, (), "truncated_normal", True) for j in range(c.Fi)])


def _truncated_normal(rng, shape):
    v = rng.standard_normal(shape)
    bad = np.abs(v) > 2.0
    while bad.any():
        v[bad] = rng.standard_normal(int(bad.sum()))
        bad = np.abs(v) > 2.0
    return v


def init_params(c, seed):
    """Values of TF's initialiser (truncated normal(0, 1) for the table and for every scalar), float32."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {"emb_mtx": _truncated_normal(rng, (c.N, c.D)).astype(np.float32)}
    for name, shape, _, _ in param_spec(c):
        out[name] = np.asarray(_truncated_normal(rng, (1,))[0], dtype=np.float32).reshape(shape)
    return out


def forward(c, P, batch, reg_lambda=0.0):
    """P: name -> torch tensor; batch: name -> integer arrays / tensors.  Returns the named intermediates."""
    dt = P["emb_mtx"].dtype
    emb_mask = torch.ones((c.N, 1), dtype=dt)
    emb_mask[0] = 0
    emb = P["emb_mtx"] * emb_mask                                         # point_model.py:31-34
    ids = lambda k: torch.as_tensor(np.asarray(batch[k]).astype(np.int64))
    look = lambda k, F: torch.nn.functional.embedding(ids(k), emb).reshape(tuple(ids(k).shape[:-1]) + (F * c.D,))
    user_seq, t_item, t_user = look("user_seq", c.Fi), look("target_item", c.Fi), look("target_user", c.Fu)
    D = c.D
    wu = [P["user_feat_w_%d" % i] for i in range(c.Fu)]
    wi = [P["item_feat_w_%d" % j] for j in range(c.Fi)]
    p_u = t_user[:, :D] * wu[0]                                           # (:175-177)
    for i in range(1, c.Fu):
        p_u = p_u + t_user[:, i * D:(i + 1) * D] * wu[i]
    p_i = t_item[:, :D] * wi[0]                                           # (:183-187)
    s = user_seq[:, :, :D] * wi[0]
    for j in range(1, c.Fi):
        p_i = p_i + t_item[:, j * D:(j + 1) * D] * wi[j]
        s = s + user_seq[:, :, j * D:(j + 1) * D] * wi[j]
    length = ids("user_seq_length")
    mask = (torch.arange(c.T)[None, :] < length[:, None]).to(dt)[:, :, None]      # tf.sequence_mask(length, T)  (:190)
    s = s * mask                                                          # (:191)
    nb = s.sum(1)                                                         # (:192)
    col = s.abs().sum(1)                                                  # [B, D]: the absolute column sums
    n = col.amax(1)                                                       # tf.norm(s, 1, (1, 2))  (:193)
    q = nb / torch.sqrt(n[:, None])
    z = (p_i * (p_u + q)).sum(1)                                          # (:195)
    y = torch.sigmoid(z)
    lab = ids("label").to(dt)
    log_loss = (-lab * torch.log(y + LOGLOSS_EPS) - (1 - lab) * torch.log(1 - y + LOGLOSS_EPS)).mean()    # (:54-63)
    l2 = sum((P[k] ** 2).sum() * 0.5 for k in P if "bias" not in k and "emb" not in k)
    return dict(p_u=p_u, p_i=p_i, s=s, nb=nb, col=col, n=n, q=q, z=z, y_pred=y, log_loss=log_loss, l2=l2,
                loss=log_loss + reg_lambda * l2, ties=(col == n[:, None]).sum(1))


def to_torch(params, dtype=torch.float64, requires_grad=False):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=requires_grad) for k, v in params.items()}


def loss_and_grads(c, params, batch, reg_lambda, dtype=torch.float64):
    """Forward + autograd backward: (out, grads); the emb_mtx gradient is dense [N, D] with row 0 zero."""
    P = to_torch(params, dtype, requires_grad=True)
    out = forward(c, P, batch, reg_lambda)
    out["loss"].backward()
    return out, {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().numpy() for k, v in P.items()}


def kink_free(c, params, batch):
    """per sample: True where neither kind of non-smooth point is near.  (1) a runner-up column sum within relative TIE_REL of
    n -- an exact tie is no kink: both sides split the gradient equally; (2) a live |s_t,d| in a maximal column that is not
    zero and below ABS_THR."""
    with torch.no_grad():
        out = forward(c, to_torch(params), batch)
    col, n, s = out["col"].numpy(), out["n"].numpy(), out["s"].numpy()
    length = np.asarray(batch["user_seq_length"])
    ok = np.ones(n.shape[0], dtype=bool)
    for b in range(n.shape[0]):
        top = col[b] == n[b]
        near = (~top) & (col[b] >= n[b] * (1.0 - TIE_REL))
        live = s[b, :max(0, min(int(length[b]), c.T))][:, top]
        small = (live != 0) & (np.abs(live) < ABS_THR)
        ok[b] = not near.any() and not small.any()
    return ok


def away_from_kinks(c, params, batch, max_dropped=None):
    """The batch without the samples that own a kink (kink_free).  At most cap(B) = max(2, B // 50) samples may go, none at all
    when B <= 3; enforced by assertion.  -> (batch, kept)"""
    ok = kink_free(c, params, batch)
    keep = np.nonzero(ok)[0]
    limit = cap(ok.size) if max_dropped is None else max_dropped
    assert limit <= cap(ok.size)
    check_dropped(ok.size, keep.size, limit)
    return {k: np.ascontiguousarray(np.asarray(v)[keep]) for k, v in batch.items()}, keep


class RefModel(object):
    """The restatement behind the reference's train / eval signatures (point_model.py:88-112): float64 gradients, cast to
    float32, then TF's Adam on float32 variables."""

    def __init__(self, c, params):
        self.cfg = c
        self.params = {k: np.array(v, dtype=np.float32) for k, v in params.items()}
        # TFAdam works in place on arrays of at least one dimension: it gets 1-d views of the variables (a scalar's shape () as (1,))
        self._flat = {k: v.reshape(-1) for k, v in self.params.items()}
        self.opt = TFAdam(self._flat)

    def train(self, sess, batch_data, lr, reg_lambda, keep_prob=1.0):
        out, grads = loss_and_grads(self.cfg, self.params, batch_to_arrays(batch_data), reg_lambda)
        self.opt.step(self._flat, {k: g.astype(np.float32).reshape(-1) for k, g in grads.items()}, lr)
        return float(out["loss"].detach())

    def eval(self, sess, batch_data, reg_lambda):
        b = batch_to_arrays(batch_data)
        with torch.no_grad():
            out = forward(self.cfg, to_torch(self.params), b, reg_lambda)
        return out["y_pred"].numpy().reshape(-1).tolist(), np.asarray(b["label"]).reshape(-1).tolist(), float(out["loss"])
