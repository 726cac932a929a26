"""Cases and the restatement of the exact rank of given items in a catalogue (GRU4Rec.item_ranks_async; include/score_hip.h:
score_catalog_ranks / score_catalog_ranks_in).  The order is catalog.hip's ct_key restated in numpy -- one 64-bit key per
(logit, index) whose unsigned comparison is (logit descending, index ascending, NaN behind every number, -0 as +0) -- and
`count` applies the definition to a line's logits: how many scored, non-excluded items stand ahead of each target.  The float64
restatement of the logits themselves is catalog_cases.restated (imported, not copied); `sandwich` gives the bounds it alone
puts on a count."""
import numpy as np

import catalog_cases as cc
import rank_cases as rc

TMAX = 32
Y_TOL = 1e-4              # max |dy| of the library against the restatement: tests/test_gpu_catalog.py


def keys(logits, index):
    """ct_key of float32 logits at catalogue indices `index`: uint64, larger = further ahead"""
    v = np.asarray(logits, dtype=np.float32)
    n = np.asarray(index, dtype=np.int64)
    b = v.view(np.uint32).astype(np.uint64)
    b = np.where(v == 0, np.uint64(0), b)
    neg = (b & np.uint64(0x80000000)) != 0
    u = np.where(neg, ~b & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))
    u = np.where(np.isnan(v), np.uint64(0), u)
    low = (~n.astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    return (u << np.uint64(32)) | low


def count(logits, targets, excluded=(), scored=None):
    """One line: logits [N] of every catalogue item (float32: the order is on their bits), targets a list of catalogue indices,
    excluded the line's exclusions, scored None (the whole catalogue) or the line's candidate list (indices outside [0, N) are
    not scored).  -> (ahead int32 [len(targets)], state int32 [len(targets)], n_scored)"""
    v = np.asarray(logits, dtype=np.float32)
    N = v.size
    S = np.arange(N) if scored is None else np.asarray(scored, dtype=np.int64)
    S = S[(S >= 0) & (S < N)]
    E = np.asarray(excluded, dtype=np.int64)
    live = S[~np.isin(S, E)]
    kl = keys(v[live], live)
    ahead, state = [], []
    for t in targets:
        t = int(t)
        if t < 0 or t >= N:
            ahead.append(-1); state.append(-1)
            continue
        ahead.append(int((kl > keys(v[t:t + 1], [t])[0]).sum()))
        state.append(0 if t not in S else (2 if t in E else 1))
    return np.asarray(ahead, dtype=np.int32), np.asarray(state, dtype=np.int32), int(live.size)


def _before(v, n, t):
    """item n stands in front of item t: a number beats NaN, a larger logit a smaller, equal logits the lower index
    (catalog_cases.select_brute's comparison)"""
    a, b = float(v[n]), float(v[t])
    if a != a or b != b:
        return (a == a and b != b) or (a != a and b != b and n < t)
    return a > b or (a == b and n < t)


def count_brute(logits, targets, excluded=(), scored=None):
    """the same by pairwise comparison in Python floats"""
    v = [float(x) for x in np.asarray(logits, dtype=np.float32)]
    N = len(v)
    S = [n for n in (range(N) if scored is None else [int(x) for x in scored]) if 0 <= n < N]
    E = set(int(e) for e in excluded)
    live = [n for n in S if n not in E]
    ahead, state = [], []
    for t in (int(x) for x in targets):
        if t < 0 or t >= N:
            ahead.append(-1); state.append(-1)
            continue
        ahead.append(sum(1 for n in live if n != t and _before(v, n, t)))
        state.append(0 if t not in S else (2 if t in E else 1))
    return ahead, state, len(live)


def sandwich(y, targets, excluded=(), scored=None, tol=Y_TOL):
    """What the float64 restatement alone says about a line's counts, the library's scores being within tol of y [N]: among the
    scored, non-excluded items other than the target, at least those whose y exceeds the target's by more than 2 tol are ahead
    and at most those whose y is no less than the target's minus 2 tol.  -> (lower, upper), -1 / -1 for a target outside"""
    y = np.asarray(y, dtype=np.float64)
    N = y.size
    S = np.arange(N) if scored is None else np.asarray(scored, dtype=np.int64)
    S = S[(S >= 0) & (S < N)]
    live = S[~np.isin(S, np.asarray(excluded, dtype=np.int64))]
    lo, hi = [], []
    for t in (int(x) for x in targets):
        if t < 0 or t >= N:
            lo.append(-1); hi.append(-1)
            continue
        others = live[live != t]
        lo.append(int((y[others] > y[t] + 2 * tol).sum()))
        hi.append(int((y[others] >= y[t] - 2 * tol).sum()))
    return np.asarray(lo), np.asarray(hi)


# ---- the GPU cases: (shape of catalog_cases.SHAPES, L, N from the plan's chunk, targets per line, seed)
# every N the plan has a seam at, L in {1, 3}, 0 / 1 / 2 / 32 targets on a line.  The seeds are chosen so that the restatement's
# sandwich is tight (tests/test_catalog_ranks_cpu.py asserts it)
CASES = [
    (0, 1, lambda ch: 1, [2], 1),
    (0, 3, lambda ch: 15, [0, 1, 32], 2),
    (1, 1, lambda ch: 16, [32], 3),
    (1, 3, lambda ch: 17, [2, 32, 1], 4),
    (2, 3, lambda ch: 31, [32, 0, 2], 5),
    (3, 1, lambda ch: 32, [1], 6),
    (0, 3, lambda ch: 33, [1, 2, 32], 7),
    (2, 3, lambda ch: ch - 1, [32, 1, 0], 8),
    (2, 1, lambda ch: ch, [32], 9),
    (3, 3, lambda ch: ch + 1, [2, 0, 32], 10),
    (0, 3, lambda ch: 2 * ch + 1, [32, 2, 1], 11),
]
IDS = ["%s-L%d-case%d" % (cc.SHAPES[s][0], L, i) for i, (s, L, _, _, _) in enumerate(CASES)]
assert {L for _, L, *_ in CASES} == {1, 3} and {q for c in CASES for q in c[3]} == {0, 1, 2, 32}


def targets_of(N, chunk, counts, seed):
    """Per line `counts[l]` target indices.  A line of 32 starts with index 0, N - 1, the last index of the first chunk and the
    first of the second and of the third (where N has them), a -1, N itself (outside) and a repeat of N - 1, then random
    indices; a line of 2 is (N - 1, -1) or a repeat (0, 0); a line of 1 is one of the seam indices"""
    rng = np.random.default_rng(1000 + seed)
    seams = [0, N - 1] + [p for p in (chunk - 1, chunk, 2 * chunk - 1, 2 * chunk) if p < N]
    out = []
    for l, q in enumerate(counts):
        if q == 0:
            t = []
        elif q == 1:
            t = [seams[(seed + l) % len(seams)]]
        elif q == 2:
            t = [N - 1, -1] if (seed + l) % 2 else [0, 0]
        else:
            t = seams + [-1, N, N - 1]
            t = t + rng.integers(0, N, size=q - len(t)).tolist()
        assert len(t) == q <= TMAX
        out.append(np.asarray(t, dtype=np.int32))
    return out


def exclusions_of(N, targets, seed):
    """Per line a third of the catalogue, the line's first in-range target among them (a target that is excluded); the LAST
    line excludes everything"""
    rng = np.random.default_rng(2000 + seed)
    out = []
    for l, t in enumerate(targets):
        e = np.nonzero(rng.random(N) < 1 / 3)[0]
        inside = [int(x) for x in t if 0 <= x < N]
        if inside:
            e = np.union1d(e, inside[:1])
        if l == len(targets) - 1:
            e = np.arange(N)
        out.append(e.astype(np.int64))
    return out


def case_inputs(i, chunk):
    """kind, cfg, params, lines, rows, N, targets of case i (no restatement: catalog_cases.restated gives it)"""
    s, L, n_of, counts, seed = CASES[i]
    kind, dims = cc.SHAPES[s]
    c = rc.cfg_of(kind, dims)
    N = n_of(chunk)
    P = rc.params_of(kind, c, True)
    lines, rows = cc.lines_of(kind, c, L, 300 + seed), cc.catalog_rows(c, N, 400 + seed)
    return dict(kind=kind, c=c, P=P, lines=lines, rows=rows, L=L, N=N, chunk=chunk, targets=targets_of(N, chunk, counts, seed),
                seed=seed)
