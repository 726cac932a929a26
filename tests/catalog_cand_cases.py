"""Cases of top-K within per-line candidate lists (recommend_async(candidates=...); include/score_hip.h: score_catalog_topk_in).
The models, catalogue rows, lines and the float64 restatement are those of tests/catalog_cases.py and tests/rank_cases.py,
imported and not copied.  One catalogue of N = 3 chunk + 7 rows per model shape; a case is a shape, the per-line list lengths
and k.  The lists are drawn without replacement and ascending; the reference selection of a line is catalog_cases.select over
the list's logits, mapped back to catalogue indices (the list is ascending, so "ties to the lower index" carries over)."""
import numpy as np

import catalog_cases as cc
import rank_cases as rc

LMAX = 3                     # every shape's lines are drawn once, for three users; a case takes the first L


def n_items(ch):
    return 3 * ch + 7


# (shape, the lines' counts as a function of the plan's chunk, k, why)
CASES = [
    (0, lambda ch: [1], 1, "one candidate"),
    (1, lambda ch: [15, 16, 17], 10, "round a tile"),
    (2, lambda ch: [31, 32, 33], 10, "a step seam"),
    (3, lambda ch: [0, 1, ch + 1], 10, "an empty line: workgroups with nothing to do"),
    (0, lambda ch: [ch - 1], 128, "a chunk - 1"),
    (1, lambda ch: [ch], 128, "exactly one chunk"),
    (2, lambda ch: [ch + 1, 2 * ch + 1, 5], 10, "a last chunk shorter than k"),
    (3, lambda ch: [2 * ch + 1], 128, "two chunks + 1"),
    (0, lambda ch: [40, 40], 128, "k above the count: padding"),
    (1, lambda ch: [n_items(ch)], 10, "every item"),
]
IDS = ["%s-%s-k%d" % (cc.SHAPES[s][0], why.split(":")[0].replace(" ", "_"), k) for s, _, k, why in CASES]
FIRST_INDEX_CASE, LAST_INDEX_CASE, RUN_CASE, EVERY_ITEM_CASE, RAGGED_CASE = 1, 2, 5, 9, 6
RUN_START = 5                # RUN_CASE's list is the contiguous run [5, 5 + chunk): positions and indices disagree modulo 32


def lists_of(i, ch):
    """case i's lists: per line an ascending int32 array of distinct catalogue indices in [0, N)"""
    _, counts, _, _ = CASES[i]
    N = n_items(ch)
    rng = np.random.default_rng(300 + i)
    out = []
    for l, n in enumerate(counts(ch)):
        if i == RUN_CASE:
            v = np.arange(RUN_START, RUN_START + n)
        else:
            v = np.sort(rng.choice(N, size=n, replace=False))
            if i == FIRST_INDEX_CASE and l == 0:
                v[0] = 0                              # (the smallest entry lowered to 0: still ascending and distinct)
            if i == LAST_INDEX_CASE and l == 2:
                v[-1] = N - 1
        out.append(v.astype(np.int32))
    return out


def shape_of(s, ch):
    """kind, cfg, params, LMAX lines and the N catalogue rows of shape s"""
    kind, dims = cc.SHAPES[s]
    c = rc.cfg_of(kind, dims)
    return kind, c, rc.params_of(kind, c), cc.lines_of(kind, c, LMAX, 400 + s), cc.catalog_rows(c, n_items(ch), 500 + s)


def first_lines(lines, L):
    return tuple(np.asarray(lines[n])[:L] for n in ("user_seq", "user_seq_length", "target_user"))


def select_in(logits, cand, k, excluded=None):
    """The reference selection of one line WITHIN its list: catalog_cases.select over the listed items' logits (excluded:
    catalogue indices), the positions mapped back to catalogue indices -> (idx [k] int32, -1 padded; val [k], -inf padded)"""
    cand = np.asarray(cand, dtype=np.int64)
    gone = None
    if excluded is not None and len(excluded):
        gone = np.nonzero(np.isin(cand, np.asarray(excluded)))[0]
    pos, val = cc.select(np.asarray(logits)[cand], k, gone)
    idx = np.where(pos >= 0, cand[np.maximum(pos, 0)] if cand.size else -1, -1).astype(np.int32)
    return idx, val
