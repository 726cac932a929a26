"""Cases and the float64 restatement of the line-form ranking pass (GRU4Rec.rank / Caser.rank; include/score_hip.h:
score_rank_forward).  A target line is one user and C = 1 + neg_sample_num candidates: the history encoder runs once per line and
fc1's pre-activation is the sum of a per-line part and a per-candidate part.  split_forward restates exactly that -- on the
library's head-input layout, Caser's three pad columns included -- in float64, from the restatements' own encoders
(tests/gru4rec_ref.py, tests/caser_ref.py); tests/test_rank_cpu.py pins it to their forward on the expanded batch."""
import math

import numpy as np
import torch

import caser_ref as cr
import gru4rec_ref as gr

N_FEATURES = 3000
PARAM_SEED = 3
REF = {"GRU4Rec": gr, "Caser": cr}
MIN_GAP = 1e-3          # every line's smallest |positive - negative| score gap: what makes "equal ranks" a condition on the inputs

# (model, (D, H, T, Fu, Fi), L, C, batch seed, why).  The smallest shapes at which the tile and stride logic can go wrong; a tile
# is 16 candidates.  A GRU4Rec row's seed is its number in the table, a Caser row's is 1; where that batch misses MIN_GAP on the
# restatement (row 4: seed 4 gives 3.5e-4) it is the next seed that meets it (test_rank_cpu.py checks all of them without a GPU)
CASES = [
    ("GRU4Rec", (16, 32, 9, 3, 4), 3, 10, 1, "one ragged tile"),
    ("GRU4Rec", (16, 32, 9, 3, 4), 2, 100, 2, "six tiles + 4, the reference's C"),
    ("GRU4Rec", (16, 16, 9, 3, 4), 3, 17, 3, "a full tile + 1"),
    ("GRU4Rec", (16, 64, 20, 3, 4), 2, 16, 5, "exactly one tile"),
    ("GRU4Rec", (8, 48, 7, 2, 2), 4, 33, 5, "composed recurrences, narrow D"),
    ("GRU4Rec", (16, 32, 50, 1, 2), 2, 100, 6, "Fu = 1, Tmall point T"),
    ("GRU4Rec", (16, 32, 9, 3, 4), 5, 1, 7, "no negatives"),
    ("Caser", (8, 32, 50, 2, 2), 3, 10, 1, "pad rows, one window"),
    ("Caser", (8, 32, 50, 2, 2), 2, 100, 1, "pad rows, one window, the reference's C"),
    ("Caser", (16, 32, 51, 3, 4), 3, 10, 1, "pad rows, two windows"),
    ("Caser", (16, 32, 51, 3, 4), 2, 100, 1, "pad rows, two windows, the reference's C"),
]
IDS = ["%s-%s-L%d-C%d" % (k, "x".join(str(x) for x in dims), L, C) for k, dims, L, C, _, _ in CASES]


def cfg_of(kind, dims, N=N_FEATURES):
    return REF[kind].Cfg(N, *dims)


def params_of(kind, c, moved=False):
    """TF's initial values; moved: the biases and bn1 off their zeros / ones, so that no term of the split is blind to a slip"""
    P = REF[kind].init_params(c, PARAM_SEED)
    rng = np.random.default_rng(1000 + PARAM_SEED)
    for n in P:
        if moved and ("bias" in n or n.startswith("bn1")):
            P[n] = (P[n] + 0.1 * rng.standard_normal(P[n].shape)).astype(np.float32)
    return P


def as_lines(b, L, C):
    """the batch with each line's first user_seq, user_seq_length and target_user copied over the line, labels 1, 0, ..., 0"""
    out = {k: np.array(v) for k, v in b.items()}
    for k in ("user_seq", "user_seq_length", "target_user"):
        v = out[k].reshape((L, C) + out[k].shape[1:])
        out[k] = np.repeat(v[:, :1], C, axis=1).reshape(out[k].shape)
    out["label"] = (np.arange(L * C) % C == 0).astype(np.int32)
    return out


def line_batch(kind, c, L, C, seed):
    return as_lines(REF[kind].random_batch(np.random.default_rng(seed), c, L * C), L, C)


def case(i, moved=False):
    """-> kind, cfg, params, batch, L, C of CASES[i]"""
    kind, dims, L, C, seed, _ = CASES[i]
    c = cfg_of(kind, dims)
    return kind, c, params_of(kind, c, moved), line_batch(kind, c, L, C, seed), L, C


def head_layout(kind, c):
    """The library's head-input layout (csrc/engine.hip make_dims): -> (Dhead, off_ti, pad) with the item columns at
    [off_ti, off_ti + Di), the target-user columns behind them, and pad = the columns TF does not have (Caser's h is padded to
    one 16-byte group: [h, 0, 0, 0 | v2 | target_item | target_user])"""
    if kind == "GRU4Rec":
        return c.H + c.Di + c.Du, c.H, ()
    return 4 + 2 * c.Di + c.Du, 4 + c.Di, (1, 2, 3)


def _padded(a, pad):
    """a head variable with zero rows at the pad columns (score_amd/model.py Caser._import)"""
    return a if not pad else torch.cat([a[:1], torch.zeros((len(pad),) + tuple(a.shape[1:]), dtype=a.dtype), a[1:]], 0)


def split_forward(kind, c, P, batch, L, C, reg_lambda=0.0):
    """P: name -> float64 torch tensors (TF's shapes); batch: a batch of L * C samples made of lines.  The encoder on the L
    lines, z_line = fc1/bias + bn1(x_line) . W1[line rows] once per line, bn1(target_item) . W1[item rows] per candidate."""
    ref = REF[kind]
    Dhead, off_ti, pad = head_layout(kind, c)
    lines = {k: np.asarray(v).reshape((L, C) + np.asarray(v).shape[1:])[:, 0] for k, v in batch.items()}
    enc = ref.forward(c, P, lines)
    dt = P["emb_mtx"].dtype
    emb = P["emb_mtx"].clone()
    emb[0] = 0
    rows = lambda a, F: torch.nn.functional.embedding(torch.as_tensor(np.asarray(a).astype(np.int64)), emb).reshape(-1, F * c.D)
    t_user, t_item = rows(lines["target_user"], c.Fu), rows(batch["target_item"], c.Fi)
    no_item = torch.zeros((L, c.Di), dtype=dt)
    if kind == "GRU4Rec":
        x_line = torch.cat([enc["h2"], no_item, t_user], 1)
    else:
        h = enc["hwin"].max(1).values
        v2 = enc["v"] * P["dense/kernel"].reshape(()) + P["dense/bias"].reshape(())
        x_line = torch.cat([h[:, None], torch.zeros((L, 3), dtype=dt), v2, no_item, t_user], 1)
    assert x_line.shape == (L, Dhead)
    gamma, beta, W1 = (_padded(P[n], pad) for n in ("bn1/gamma", "bn1/beta", "fc1/kernel"))
    scale = gamma / math.sqrt(1.0 + ref.BN_EPS)
    item = np.arange(off_ti, off_ti + c.Di)
    line = np.setdiff1d(np.arange(Dhead), item)
    z_line = P["fc1/bias"] + (x_line[:, line] * scale[line] + beta[line]) @ W1[line]            # [L, 200]
    z_cand = (t_item * scale[item] + beta[item]) @ W1[item]                                    # [L * C, 200]
    f1 = torch.relu(z_line.repeat_interleave(C, 0) + z_cand)
    f2 = torch.relu(f1 @ P["fc2/kernel"] + P["fc2/bias"])
    y = torch.sigmoid((f2 @ P["fc3/kernel"] + P["fc3/bias"]).reshape(-1))
    lab = torch.as_tensor(np.asarray(batch["label"]).astype(np.int64)).to(dt)
    log_loss = (-lab * torch.log(y + ref.LOGLOSS_EPS) - (1 - lab) * torch.log(1 - y + ref.LOGLOSS_EPS)).mean()
    l2 = sum((P[n] ** 2).sum() * 0.5 for n in P if "bias" not in n and "emb" not in n)
    return dict(y_pred=y, log_loss=log_loss, l2=l2, loss=log_loss + reg_lambda * l2)


def restated(kind, c, P, batch, L, C, reg_lambda=0.0):
    """split_forward on float32-valued parameters -> (y_pred float64 array, loss)"""
    with torch.no_grad():
        out = split_forward(kind, c, REF[kind].to_torch(P), batch, L, C, reg_lambda)
    return out["y_pred"].numpy(), float(out["loss"])


def line_gaps(y, L, C):
    """per line, the smallest |score of the positive (column 0) - score of a negative|; inf for a line without negatives"""
    y = np.asarray(y, dtype=np.float64).reshape(L, C)
    return np.abs(y[:, :1] - y[:, 1:]).min(1) if C > 1 else np.full(L, np.inf)
