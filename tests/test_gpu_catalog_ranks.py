"""The exact rank of given items in a catalogue on the GPU (GRU4Rec.item_ranks_async / Caser's; csrc/catalog.hip, the counting
form of catalog_score_kernel; score_catalog_ranks / score_catalog_ranks_in): the targets' logits bit for bit against
recommend_async(all_logits=True), the counts, states and n_scored exactly against the restated count
(tests/catalog_ranks_cases.py) applied to those same library logits, with and without exclusions, the float64 restatement's
sandwich without a gap condition, recommend_async's own lists ranked 0, 1, 2, ..., ties across the seams, the candidate form, two
runs, a catalogue gone stale, the route by user id, and harness.evaluate_catalog_ranks on the bundled Tmall sample."""
import functools
import os

import numpy as np
import pytest
import torch

import catalog_cases as cc
import catalog_ranks_cases as kr
import rank_cases as rc
import user_line_cases as uc
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

Y_TOL = kr.Y_TOL          # that of tests/test_gpu_catalog.py


def _cfg_of(kind, c):
    from score_amd import _lib
    return _lib.make_config(c.N, c.D, c.H, c.T, 1, c.Fu, c.Fi, kind)


def _lines(lines):
    return tuple(lines[n] for n in ("user_seq", "user_seq_length", "target_user"))


def _csr(lists, dev, dtype=torch.int32):
    """per-line index lists as the library takes them: (off int64 [L + 1], idx, longest), idx never empty"""
    off = torch.as_tensor(np.concatenate([[0], np.cumsum([len(v) for v in lists])]), dtype=torch.int64, device=dev)
    flat = np.concatenate([np.asarray(v, dtype=np.int64) for v in lists]) if sum(len(v) for v in lists) else np.asarray([-1])
    return off, torch.as_tensor(flat, dtype=dtype, device=dev), max(len(v) for v in lists)


@functools.lru_cache(maxsize=None)
def _case(i):
    """case i: the model, its catalogue, the library's own logits of every pair and the restatement (computed once)"""
    from score_amd import _lib
    from score_amd import model as M
    s, L, n_of, counts, seed = kr.CASES[i]
    kind, dims = cc.SHAPES[s]
    c = rc.cfg_of(kind, dims)
    ch = _lib.catalog_ranks_plan(_cfg_of(kind, c), L, 1)[0]
    d = kr.case_inputs(i, ch)
    chunk, nchunk, _ = _lib.catalog_ranks_plan(_cfg_of(kind, c), L, d["N"])
    assert chunk == ch and nchunk == -(-d["N"] // ch)                  # the seams are where the case says they are
    assert (chunk, nchunk) == _lib.catalog_plan(_cfg_of(kind, c), L, d["N"], 10)[:2]
    m = M.MODELS[kind](*c.args)
    m.set_params(d["P"])
    cat = M.ItemCatalog(m, d["rows"])
    full = m.recommend_async(_lines(d["lines"]), cat, k=1, all_logits=True)[2].clone()
    _, y = cc.restated(kind, c, d["P"], d["lines"], d["rows"])
    y.setflags(write=False)
    d.update(m=m, cat=cat, full=full, full_h=full.cpu().numpy(), y=y, nchunk=nchunk)
    return d


def _hold(what, out, full_h, targets, excl=None, scored=None):
    """the call's five tensors against the restated count on the library's own logits: exactly"""
    ahead, logit, state, n_scored, off = (t.cpu().numpy() for t in out)
    L, N = full_h.shape
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(t) for t in targets])]).tolist(), what
    assert ahead.dtype == np.int32 and state.dtype == np.int32 and n_scored.dtype == np.int32 and logit.dtype == np.float32
    for l in range(L):
        t = np.asarray(targets[l], dtype=np.int64)
        a, b = int(off[l]), int(off[l + 1])
        want = kr.count(full_h[l], t, () if excl is None else excl[l], None if scored is None else scored[l])
        assert ahead[a:b].tolist() == want[0].tolist(), (what, l, ahead[a:b].tolist(), want[0].tolist())
        assert state[a:b].tolist() == want[1].tolist(), (what, l, state[a:b].tolist(), want[1].tolist())
        assert int(n_scored[l]) == want[2], (what, l)
        inside = (t >= 0) & (t < N)
        assert np.isnan(logit[a:b][~inside]).all(), (what, l)
        assert np.array_equal(logit[a:b][inside].view(np.int32), full_h[l][t[inside]].view(np.int32)), (what, l)      # bit for bit


def test_the_cases_hit_every_size_the_plan_has_a_seam_at():
    got = []
    for i in range(len(kr.CASES)):
        d = _case(i)
        got.append((d["N"], d["chunk"]))
    ch = got[0][1]
    assert all(c == ch for _, c in got) and ch % 32 == 0
    assert [n for n, _ in got] == [1, 15, 16, 17, 31, 32, 33, ch - 1, ch, ch + 1, 2 * ch + 1]


@pytest.mark.parametrize("i", range(len(kr.CASES)), ids=kr.IDS)
def test_counts_logits_and_the_restatement(i):
    d = _case(i)
    m, cat, L, N, full_h = d["m"], d["cat"], d["L"], d["N"], d["full_h"]
    targets = d["targets"]
    ids = d["rows"][:, 0]
    tg = _csr(targets, m.device)
    ln = _lines(d["lines"])
    excl = kr.exclusions_of(N, targets, d["seed"])
    for what, ex in (("plain", None), ("excluded", excl)):
        kw = {} if ex is None else dict(exclude=[ids[e] for e in ex])
        out = [t.clone() for t in m.item_ranks_async(ln, cat, tg, **kw)]
        _hold((kr.IDS[i], what), out, full_h, targets, ex)
        again = m.item_ranks_async(ln, cat, tg, **kw)                       # two runs: the same bits
        for a, b in zip(out, again):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b), what
        # the float64 restatement alone, no gap condition, nothing dropped
        ahead, off = out[0].cpu().numpy(), out[4].cpu().numpy()
        for l in range(L):
            lo, hi = kr.sandwich(d["y"][l], targets[l], () if ex is None else ex[l])
            got = ahead[off[l]:off[l + 1]]
            print(kr.IDS[i], what, "line", l, "ahead - lower", (got - lo).tolist(), "upper - ahead", (hi - got).tolist())
            assert (lo <= got).all() and (got <= hi).all(), (what, l, lo.tolist(), got.tolist(), hi.tolist())
        # recommend_async's own list, ranked: 0, 1, 2, ...
        n_scored = out[3].cpu().numpy()
        for l in range(L):
            assert n_scored[l] == N - (0 if ex is None else ex[l].size)
        k = int(min(128, n_scored.max()))
        if k >= 1:
            top = m.recommend_async(ln, cat, k=k, **kw)[0].cpu().numpy()
            for a in range(0, k, kr.TMAX):
                part = [top[l][a:a + kr.TMAX] for l in range(L)]
                got = m.item_ranks_async(ln, cat, _csr(part, m.device), **kw)
                g_ahead, g_state = got[0].cpu().numpy().reshape(L, -1), got[2].cpu().numpy().reshape(L, -1)
                for l in range(L):
                    real = part[l] >= 0
                    assert g_ahead[l][real].tolist() == list(range(a, a + int(real.sum()))), (what, l, a)
                    assert (g_state[l][real] == 1).all() and (g_ahead[l][~real] == -1).all() and (g_state[l][~real] == -1).all()
    assert cat.builds == 1
    m.check_ids()                                                           # nothing was reported
    # the synchronous form and item ids as targets: an id the catalogue does not hold is a target outside
    absent = int(np.setdiff1d(np.arange(1, d["c"].N), ids)[0])
    by_id = [[int(ids[x]) if 0 <= x < N else absent for x in t] for t in targets]
    a_l, g_l, s_l, n_l = m.item_ranks(ln, cat, by_id)
    want = [t.cpu().numpy() for t in m.item_ranks_async(ln, cat, by_id)]
    off = want[4]
    assert [len(x) for x in a_l] == [len(t) for t in targets] and n_l == want[3].tolist()
    assert sum(a_l, []) == want[0][:off[-1]].tolist() and sum(s_l, []) == want[2][:off[-1]].tolist()
    _hold((kr.IDS[i], "by id"), [torch.as_tensor(x) for x in want], full_h,
          [[x if 0 <= x < N else -1 for x in t] for t in targets])


def test_a_chunk_with_more_exclusions_than_are_staged_and_a_line_with_too_many_targets():
    """the whole form: 260 lines make the plan one chunk of 640 items, line 0 excludes 600 of them (the kernel stages 512 in
    LDS); then the caller's error: a line with more targets than max_targets says"""
    from score_amd import _lib
    from score_amd import model as M
    kind, dims = cc.SHAPES[0]
    c = rc.cfg_of(kind, dims)
    L, N = 260, 640
    assert _lib.catalog_ranks_plan(_cfg_of(kind, c), L, N)[:2] == (640, 1)
    lines, rows = cc.lines_of(kind, c, L, 77), cc.catalog_rows(c, N, 78)
    m = M.MODELS[kind](*c.args)
    m.set_params(rc.params_of(kind, c, True))
    cat = M.ItemCatalog(m, rows)
    ln = _lines(lines)
    full_h = m.recommend_async(ln, cat, k=1, all_logits=True)[2].cpu().numpy()
    rng = np.random.default_rng(5)
    targets = [rng.integers(0, N, size=(32 if l < 3 else 1)).astype(np.int32) for l in range(L)]
    none = np.zeros((0,), dtype=np.int64)
    excl = [none] * L
    excl[0] = np.sort(rng.choice(N, size=600, replace=False))
    excl[1] = np.sort(rng.choice(N, size=512, replace=False))               # exactly what is staged
    excl[2] = np.sort(rng.choice(N, size=513, replace=False))
    targets[0][:4] = excl[0][[0, 1, 300, 599]]
    ids = rows[:, 0]
    out = m.item_ranks_async(ln, cat, _csr(targets, m.device), exclude=[ids[e] for e in excl])
    _hold("many exclusions", out, full_h, targets, excl)
    assert out[3][:3].tolist() == [40, 128, 127]
    m.check_ids()
    # three targets on line 1, max_targets = 2: the first two are counted, the third is marked, bit 1 of the status word is set
    few = [targets[0][:2], targets[1][:3], targets[2][:1]] + [t[:1] for t in targets[3:]]
    off, idx, longest = _csr(few, m.device)
    assert longest == 3
    out = [t.cpu().numpy() for t in m.item_ranks_async(ln, cat, (off, idx, 2))]
    want = [t.cpu().numpy() for t in m.item_ranks_async(ln, cat, (off, idx, 3))]
    assert int(m._id_status[0].item()) == 1 << 1
    m._id_status.zero_()
    a = int(off[1]) + 2
    assert out[0][a] == -1 and out[2][a] == -1 and np.isnan(out[1][a])
    keep = np.arange(out[0].size) != a
    assert np.array_equal(out[0][keep], want[0][keep]) and np.array_equal(out[2][keep], want[2][keep])
    assert np.array_equal(out[1][keep].view(np.int32), want[1][keep].view(np.int32)) and np.array_equal(out[3], want[3])


def test_equal_logits_get_consecutive_counts_in_index_order_across_the_seams():
    from score_amd import _lib
    from score_amd import model as M
    kind, dims = cc.SHAPES[0]
    ch = _lib.catalog_ranks_plan(_cfg_of(kind, rc.cfg_of(kind, dims)), 2, 1)[0]
    kind, c, P, lines, rows, copies = cc.tie_case(ch)
    N = len(rows)
    assert _lib.catalog_ranks_plan(_cfg_of(kind, c), 2, N)[:2] == (ch, 2)
    assert {15, 16, 31, 32, ch - 1, ch, N - 1} <= set(copies)
    m = M.MODELS[kind](*c.args)
    m.set_params(P)
    cat = M.ItemCatalog(m, rows)
    ln = _lines(lines)
    full_h = m.recommend_async(ln, cat, k=1, all_logits=True)[2].cpu().numpy()
    targets = [np.asarray(copies[::-1], dtype=np.int32), np.asarray(copies, dtype=np.int32)]       # (in any order)
    out = m.item_ranks_async(ln, cat, _csr(targets, m.device))
    _hold("ties", out, full_h, targets)
    ahead = out[0].cpu().numpy().reshape(2, -1)
    assert ahead[0][::-1].tolist() == list(range(len(copies)))              # line 0: they share its best logit
    assert np.diff(ahead[1]).tolist() == [1] * (len(copies) - 1)            # any line: consecutive, in index order
    bits = out[1].cpu().numpy().reshape(2, -1).view(np.int32)
    assert (bits == bits[:, :1]).all()
    # with one of the copies excluded the ones behind it move up by one, the excluded one keeps its place
    gone = copies[3]
    out = m.item_ranks_async(ln, cat, _csr(targets, m.device), exclude=[[rows[gone, 0]], []])
    _hold("ties, one excluded", out, full_h, targets, [[gone], []])
    assert out[0].cpu().numpy().reshape(2, -1)[0][::-1].tolist() == [0, 1, 2, 3, 3, 4, 5, 6][:len(copies)]


def test_the_candidate_form():
    d = _case(10)                                                           # GRU4Rec, L = 3, two chunks + 1
    m, cat, L, N, ch, full_h = d["m"], d["cat"], d["L"], d["N"], d["chunk"], d["full_h"]
    assert L == 3 and N == 2 * ch + 1
    ln = _lines(d["lines"])
    ids = d["rows"][:, 0]
    rng = np.random.default_rng(9)
    run = np.arange(5, 5 + ch + 40)                                         # crosses the list's chunk seam off the catalogue's
    lists = [np.zeros((0,), dtype=np.int64), run, np.sort(rng.choice(N, size=70, replace=False))]
    listed, unlisted = int(lists[2][0]), int(np.setdiff1d(np.arange(N), lists[2])[0])
    targets = [np.asarray([0, N - 1, -1], dtype=np.int32),
               np.concatenate([[5, 4, 5 + ch - 1, 5 + ch, 5 + ch + 39, 5 + ch + 40, -1, N], rng.integers(0, N, size=24)]).astype(np.int32),
               np.asarray([listed, unlisted], dtype=np.int32)]
    tg = _csr(targets, m.device)
    cands = [ids[v] for v in lists]
    out = m.item_ranks_async(ln, cat, tg, candidates=cands)
    _hold("lists", out, full_h, targets, None, lists)
    st = out[2].cpu().numpy()
    assert st[:3].tolist() == [0, 0, -1] and out[0][:3].tolist() == [0, 0, -1] and out[3].tolist() == [0, run.size, 70]
    assert st[-2:].tolist() == [1, 0]
    # max_candidates larger than needed, and smaller (the last chunk's workgroup walks to the list's end)
    for M_ in (4 * ch, 1):
        again = m.item_ranks_async(ln, cat, tg, candidates=cands, max_candidates=M_)
        for a, b in zip(out, again):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b), M_
    # with exclusions, a listed target among them
    excl = [np.asarray([3]), run[::3], np.asarray([listed, unlisted])]
    out_x = m.item_ranks_async(ln, cat, tg, candidates=cands, exclude=[ids[e] for e in excl])
    _hold("lists, excluded", out_x, full_h, targets, excl, lists)
    assert out_x[2][-2:].tolist() == [2, 0]
    # an entry outside [0, N) in a list is not scored (handed over as ItemCatalog.candidates would hand it)
    bad = [np.asarray([-1, N]), np.concatenate([[-1], run, [N]]), np.concatenate([lists[2], [N]])]
    off, cidx, longest = _csr(bad, m.device)
    out_b = m.item_ranks_async(ln, cat, tg, candidates=(off, cidx, longest))
    _hold("lists with entries outside", out_b, full_h, targets, None, bad)
    for a, b in zip(out, out_b):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)
    # with all N items listed it is the whole form
    every = [np.arange(N)] * L
    whole = m.item_ranks_async(ln, cat, tg, exclude=[ids[e] for e in excl])
    whole = [t.clone() for t in whole]
    listed_all = m.item_ranks_async(ln, cat, tg, candidates=[ids[v] for v in every], exclude=[ids[e] for e in excl])
    for a, b in zip(whole, listed_all):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)
    _hold("every item listed", listed_all, full_h, targets, excl, every)
    m.check_ids()


def test_a_catalogue_built_before_a_train_step_is_rebuilt():
    from score_amd import model as M
    d = kr.case_inputs(3, 256)                                              # GRU4Rec (8, 48, 7, 2, 2), L = 3, N = 17
    kind, c = d["kind"], d["c"]
    m = M.MODELS[kind](*c.args)
    m.set_params(d["P"])
    cat = M.ItemCatalog(m, d["rows"])
    ln = _lines(d["lines"])
    tg = _csr(d["targets"], m.device)
    before = [t.clone() for t in m.item_ranks_async(ln, cat, tg)]
    assert cat.builds == 1 and cat.version == m.weights_version
    bt = rc.REF[kind].batch_tuple(cc.expanded(d["lines"], d["rows"]))
    for _ in range(3):
        m.train(None, bt, 1e-2, 1e-4)
    assert cat.version != m.weights_version
    got = m.item_ranks_async(ln, cat, tg)
    assert cat.builds == 2 and cat.version == m.weights_version
    full_h = m.recommend_async(ln, M.ItemCatalog(m, d["rows"]), k=1, all_logits=True)[2].cpu().numpy()
    _hold("rebuilt", got, full_h, d["targets"])
    assert not torch.equal(got[1].view(torch.int32), before[1].view(torch.int32))


def test_by_user_id_equals_the_lines_and_history_exclusions_route():
    from score_amd import model as M
    from score_amd.pointdata import PointLogStore
    s = 0
    kind, dims = cc.SHAPES[s]
    c = rc.cfg_of(kind, dims)
    U, I, NEG, H = 40, 2 * 256 + 1, 9, 30
    rng = np.random.default_rng(40)
    counts = rng.integers(0, 2 * H, U)
    counts[:4] = (3, 0, c.T, 2 * H + 7)
    log = uc.crafted_log(counts.tolist(), I, seed=50)
    ur, ir = uc.rows_of(U, I, c.Fu, c.Fi, c.N, seed=60)
    per = 1 + NEG
    lines = uc.target_lines(log[0], log[3], uc.WINDOW, U, I, per, 12, seed=70)
    st = PointLogStore(*log, lines, uc.WINDOW[0], uc.WINDOW[1], H, NEG, 12 * per, ur, ir, False, build="device")
    m = M.MODELS[kind](*c.args)
    m.set_params(rc.params_of(kind, c))
    cat = M.ItemCatalog(m, ir)
    users = [1, 2, U + 5, 4, 0, 3]
    L = len(users)
    arr = st.arrays()
    hist = [arr["user_hist_seq"][arr["user_hist_off"][u - 1]:arr["user_hist_off"][u]] if 1 <= u <= U else np.zeros((0,), np.int32)
            for u in users]
    ids = np.asarray(ir)[:, 0]
    # per line: an item of the user's own history (where there is one), two others, an id the catalogue does not hold
    tl = [([int(h[0])] if len(h) else []) + [int(ids[7]), int(ids[I - 1]), int(ids[-1]) + 1000] for h in hist]
    tg = cat.targets(tl, L)
    got = m.item_ranks_users_async(users, st, cat, tg)
    assert len(got) == 6 and got[5].tolist() == [1, 1, 0, 1, 0, 1]
    got = [t.clone() for t in got]
    ul = st.user_lines(np.asarray(users, dtype=np.int32), c.T)
    xi = cat.history_exclusions(st, torch.as_tensor(users, dtype=torch.int32, device=m.device), None)
    want = m.item_ranks_async(ul[:3], cat, tg, exclude_idx=xi)
    for a, b in zip(got[:5], want):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)
    # against the restated count on the call's own logits, the histories as exclusions
    full_h = m.recommend_async(ul[:3], cat, k=1, all_logits=True)[2].cpu().numpy()
    excl = [np.unique(np.searchsorted(ids, h[np.isin(h, ids)])) for h in hist]
    t_idx = [[int(np.searchsorted(ids, x)) if x in ids else -1 for x in t] for t in tl]
    _hold("by user id", got[:5], full_h, t_idx, excl)
    state, off = got[2].cpu().numpy(), got[4].cpu().numpy()
    for l, h in enumerate(hist):
        if len(h):
            assert state[off[l]] == 2                                       # inside the history: ranked against the rest
        assert state[off[l + 1] - 1] == -1
    assert sum(len(h) > 0 for h in hist) >= 3
    none = m.item_ranks_users_async(users, st, cat, tg, exclude_history=False)
    _hold("by user id, nothing excluded", none[:5], full_h, t_idx)
    m.check_ids()


def test_evaluate_catalog_ranks_on_the_tmall_sample():
    from score_amd import dataprep as dp
    from score_amd import harness as h
    from score_amd import model as M
    from score_amd.pointdata import DeviceDataLoaderUserSeq
    log = np.load(os.path.join(GOLDEN, "tmall_sample_log.npz"))["log"]
    stores, r = dp.tmall_point_stores(log, dual=False, batch_size=1000)
    st = stores["validation"]
    T, neg = 50, 99
    m = M.GRU4Rec(r["feature_size"], 16, 32, T, 3, 4, seed=7)
    batches = list(DeviceDataLoaderUserSeq(1000, T, None, None, neg, None, None, model=m, store=st))
    for s in range(10):
        m.train(None, batches[s % len(batches)], 1e-2, 1e-4)
    cat = M.ItemCatalog(m, st.item_rows)
    assert cat.N > 128
    for kw_old, kw_new in ((dict(), dict(exclude_history=False)), (dict(exclude_history=st), dict(exclude_history=True)),
                           (dict(candidates="line"), dict(exclude_history=False, candidates="line")),
                           (dict(exclude_history=st, candidates="line"), dict(exclude_history=True, candidates="line"))):
        six = h.evaluate_catalog(m, batches, cat, neg, k=128, **kw_old)
        seven = h.evaluate_catalog_ranks(m, batches, cat, neg, **kw_old)
        print("tmall sample", kw_old.keys(), six, seven)
        assert len(seven) == 7 and np.allclose(seven[:5], six[:5], rtol=0, atol=1e-12), (six, seven)
        assert seven[5] >= six[5] - 1e-12 and seven[6] >= 1.0
        if "candidates" in kw_old:                                          # at most 100 items a line: nothing is truncated at 128
            assert abs(seven[5] - six[5]) <= 1e-12
        assert h.evaluate_catalog_ranks_users(m, st, cat, **kw_new) == seven
        assert h.evaluate_catalog_ranks_users(m, st, cat, lines_per_call=7, **kw_new) == seven
    assert cat.builds == 1
    # N <= 128: all six are equal, whatever the targets (line l's: item l % 100 of a catalogue of 100)
    small = M.ItemCatalog(m, np.asarray(st.item_rows)[:100])
    tops, aheads, tgts = [], [], []
    for b in batches:
        ln = m.lines_of(b, neg)
        L = int(ln[1].numel())
        tgt = (torch.arange(L, device=m.device) % 100).to(torch.int32)
        tops.append(m.recommend_async(ln, small, k=128, active_slices=b.active_slices)[0].clone())
        out = m.item_ranks_async(ln, small, (torch.arange(L + 1, device=m.device, dtype=torch.int64), tgt, 1),
                                 active_slices=b.active_slices)
        assert bool((out[2] == 1).all()) and bool((out[3] == 100).all())
        aheads.append(out[0].clone()); tgts.append(tgt)
    six = h.catalog_quality_device(torch.cat(tops), torch.cat(tgts))
    seven = h.rank_quality_device(torch.cat(aheads))
    assert np.allclose(seven[:6], six, rtol=0, atol=1e-12), (six, seven)
