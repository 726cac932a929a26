"""Cases and the float64 restatement of top-K over a whole item catalogue (GRU4Rec.recommend / Caser.recommend; include/score_hip.h:
score_catalog_topk).  The restated logits of all L * N (line, item) pairs are rank_cases.split_forward on the expanded batch --
every line against every catalogue row, imported and not copied -- taken in front of its sigmoid; the reference selection is a
stable sort of (-logit, index) with the exclusions removed."""
import contextlib

import numpy as np
import torch

import rank_cases as rc

KMAX = 128

# the small shapes of rank_cases.CASES: (model, (D, H, T, Fu, Fi))
SHAPES = [("GRU4Rec", (16, 32, 9, 3, 4)), ("GRU4Rec", (8, 48, 7, 2, 2)), ("Caser", (8, 32, 50, 2, 2)), ("Caser", (16, 32, 51, 3, 4))]
assert all(any(s == (k, d) for k, d, *_ in rc.CASES) for s in SHAPES)

# (shape, L, N as a function of the plan's chunk, k, why).  tests/test_gpu_catalog.py asserts through score_catalog_plan that
# the Ns are 1, 15, 16, 17, chunk - 1, chunk, chunk + 1 and 2 chunk + 1, and which rows have k > N or a short last chunk.
CASES = [
    (0, 1, lambda ch: 1, 1, "one item"),
    (0, 3, lambda ch: 15, 10, "a ragged tile"),
    (1, 1, lambda ch: 16, 128, "one tile, k > N"),
    (1, 3, lambda ch: 17, 10, "a tile + 1"),
    (2, 3, lambda ch: ch - 1, 10, "a chunk - 1"),
    (2, 1, lambda ch: ch, 128, "exactly one chunk"),
    (3, 3, lambda ch: ch + 1, 10, "a chunk + 1: the last chunk holds fewer than k"),
    (3, 1, lambda ch: 2 * ch + 1, 128, "two chunks + 1, k of 128 against a last chunk of one"),
    (0, 3, lambda ch: 2 * ch + 1, 1, "two chunks + 1, k = 1"),
]
IDS = ["%s-L%d-%s-k%d" % (SHAPES[s][0], L, why.split(":")[0].replace(" ", "_"), k) for s, L, _, k, why in CASES]


def catalog_rows(c, N, seed):
    """item_rows [N, Fi]: column 0 the item ids, strictly ascending, the other columns any feature ids of the table"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(1, c.N, size=(N, c.Fi)).astype(np.int32)
    rows[:, 0] = np.sort(rng.choice(np.arange(1, c.N), size=N, replace=False)).astype(np.int32)
    return rows


def lines_of(kind, c, L, seed):
    """L lines: a batch of L samples whose target_item is not used"""
    return rc.REF[kind].random_batch(np.random.default_rng(seed), c, L)


def expanded(lines, rows):
    """every line against every catalogue row: the batch of L * N samples made of L lines of N candidates"""
    L, N = len(lines["user_seq_length"]), len(rows)
    out = {k: np.repeat(np.asarray(lines[k]), N, axis=0) for k in ("user_seq", "user_seq_length", "target_user")}
    out["target_item"] = np.tile(rows, (L, 1)).astype(np.int32)
    out["label"] = (np.arange(L * N) % N == 0).astype(np.int32)
    return out


@contextlib.contextmanager
def _sigmoid_arguments(seen):
    """records what torch.sigmoid is called with: split_forward's logits, in front of its sigmoid"""
    real = torch.sigmoid

    def spy(x):
        seen.append(x.detach().clone())
        return real(x)
    torch.sigmoid = spy
    try:
        yield
    finally:
        torch.sigmoid = real


def restated(kind, c, P, lines, rows):
    """-> (logits float64 [L, N], y = sigmoid(logits) float64 [L, N]) of rank_cases.split_forward on the expanded batch"""
    L, N = len(lines["user_seq_length"]), len(rows)
    seen = []
    with torch.no_grad(), _sigmoid_arguments(seen):
        out = rc.split_forward(kind, c, rc.REF[kind].to_torch(P), expanded(lines, rows), L, N)
    assert len(seen) >= 1 and seen[-1].shape == (L * N,)
    return seen[-1].numpy().reshape(L, N), out["y_pred"].numpy().reshape(L, N)


def select(logits, k, excluded=None):
    """The reference selection of one line: indices and logits of the k first items in the order (logit descending, index
    ascending, NaN behind every number) -- a stable sort of (-logit, index) --, excluded indices removed, padded with -1 / -inf"""
    v = np.asarray(logits)
    n = np.arange(v.size)
    order = np.lexsort((n, -np.where(np.isnan(v), -np.inf, v), np.isnan(v)))       # last key first: numbers, then by -logit, then index
    if excluded is not None and len(excluded):
        order = order[~np.isin(order, np.asarray(excluded))]
    order = order[:k]
    idx = np.full((k,), -1, dtype=np.int32)
    val = np.full((k,), -np.inf, dtype=v.dtype)
    idx[:order.size], val[:order.size] = order, v[order]
    return idx, val


def select_brute(logits, k, excluded=()):
    """the same selection by repeated search for the best remaining item"""
    v = [float(x) for x in logits]
    left = [n for n in range(len(v)) if n not in set(int(e) for e in excluded)]
    idx, val = [], []
    while left and len(idx) < k:
        best = left[0]
        for n in left[1:]:
            # a number beats NaN; a larger logit beats a smaller; an equal logit: the lower index
            if (v[n] == v[n] and v[best] != v[best]) or (v[n] == v[n] and v[n] > v[best]) or \
                    ((v[n] == v[best] or (v[n] != v[n] and v[best] != v[best])) and n < best):
                best = n
        idx.append(best); val.append(v[best]); left.remove(best)
    return idx + [-1] * (k - len(idx)), val + [-np.inf] * (k - len(val))


def tie_case(chunk, L=2, k=KMAX, seed=21):
    """A catalogue with one item copied across a tile seam (16), a step seam (32) and a chunk seam: positions 15, 16, 31, 32,
    chunk - 1, chunk and the last one hold the feature columns of the source row and item ids whose table rows EQUAL the source
    id's row, so the copies' inputs are equal bit for bit.  The copies' ids occur nowhere else -- not in the lines, not in another
    row's feature columns -- and the source is the restated best item of line 0 before the copies are placed, so the copies
    share line 0's best logit (up to the library's error against the restatement, they lead its list).
    -> kind, cfg, params, lines, rows, the copies' positions (the source among them, ascending)"""
    kind, dims = SHAPES[0]
    c = rc.cfg_of(kind, dims)
    P = rc.params_of(kind, c)
    lines = lines_of(kind, c, L, seed)
    N = chunk + 44
    rng = np.random.default_rng(seed + 1)
    used = np.union1d(lines["user_seq"].reshape(-1), lines["target_user"].reshape(-1))
    free = np.setdiff1d(np.arange(c.N // 2, c.N), used)
    rows = rng.integers(1, c.N // 2, size=(N, c.Fi)).astype(np.int32)            # (feature columns below every item id)
    rows[:, 0] = np.sort(rng.choice(free, size=N, replace=False)).astype(np.int32)
    before, _ = restated(kind, c, P, lines, rows)
    src = int(np.argmax(before[0]))
    seams = [p for p in (15, 16, 31, 32, chunk - 1, chunk, N - 1) if p != src]
    P = dict(P)
    P["emb_mtx"] = P["emb_mtx"].copy()
    for p in seams:
        rows[p, 1:] = rows[src, 1:]
        P["emb_mtx"][rows[p, 0]] = P["emb_mtx"][rows[src, 0]]
    return kind, c, P, lines, rows, sorted(seams + [src])
