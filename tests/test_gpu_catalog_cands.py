"""Top-K within per-line candidate lists on the GPU (recommend_async(candidates=...); csrc/catalog.hip, score_catalog_topk_in):
the listed pairs' logits against the float64 restatement (tests/catalog_cases.py) and, bit for bit, against the whole-catalogue
call's all_logits; the selection against a stable sort of the call's own logits; the full list against the whole-catalogue
call; repeatability; under- and overstated plan sizes; exclusions; ties across the LIST's seams; indices outside the
catalogue; and harness.evaluate_catalog(candidates="line") on the bundled Tmall sample."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import catalog_cand_cases as kc
import catalog_cases as cc
import rank_cases as rc
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

Y_TOL = 1e-4              # max |dy|: tests/test_gpu_catalog.py, from tests/test_gpu_gru4rec.py::_check


def _cfg_of(kind, c):
    from score_amd import _lib
    return _lib.make_config(c.N, c.D, c.H, c.T, 1, c.Fu, c.Fi, kind)


@functools.lru_cache(maxsize=None)
def _chunk():
    """the plan's chunk at the cases' sizes: 256 for every shape, 1 to 3 lines and every k (asserted, as test_gpu_catalog.py
    does for its seams)"""
    from score_amd import _lib
    got = set()
    for kind, dims in cc.SHAPES:
        cfg = _cfg_of(kind, rc.cfg_of(kind, dims))
        for L in (1, 2, 3):
            for k in (1, 10, 128):
                for M in (1, 33, 256, 257, 513, kc.n_items(256)):
                    ch, nch, _ = _lib.catalog_cands_plan(cfg, L, M, k)
                    assert nch == -(-M // ch)
                    got.add(ch)
    assert got == {256}
    return 256


@functools.lru_cache(maxsize=None)
def _shape(s):
    """shape s: the model, its catalogue, the lines, the restatement [LMAX, N] (computed once, never modified) and the
    whole-catalogue call's all_logits"""
    from score_amd import model as M
    ch = _chunk()
    kind, c, P, lines, rows = kc.shape_of(s, ch)
    logits, y = cc.restated(kind, c, P, lines, rows)
    logits.setflags(write=False); y.setflags(write=False)
    m = M.MODELS[kind](*c.args)
    m.set_params(P)
    cat = M.ItemCatalog(m, rows)
    full = m.recommend_async(kc.first_lines(lines, kc.LMAX), cat, k=10, all_logits=True)[2].clone()
    return dict(kind=kind, c=c, m=m, cat=cat, lines=lines, rows=rows, N=len(rows), y=y, full=full)


def _own_selection(off, cidx, own, L, k, excl=None):
    """per line the stable sort of the call's OWN logits by (-logit, index) on the device -- the list is ascending, so a
    stable sort by -logit is that order --, excluded catalogue indices removed, -1 / -inf padding"""
    dev = own.device
    idx = torch.full((L, k), -1, dtype=torch.int32, device=dev)
    val = torch.full((L, k), float("-inf"), dtype=torch.float32, device=dev)
    off = off.tolist()
    for l in range(L):
        mine, v = cidx[off[l]:off[l + 1]], own[off[l]:off[l + 1]]
        order = torch.sort(-v, stable=True).indices
        if excl is not None and len(excl[l]):
            gone = torch.isin(mine.long(), torch.as_tensor(np.asarray(excl[l]), device=dev).long())
            order = order[~gone[order]]
        order = order[:k]
        idx[l, :order.numel()] = mine[order]
        val[l, :order.numel()] = v[order]
    return idx, val


def _hold(what, idx, val, want):
    assert torch.equal(idx, want[0]), (what, idx.tolist(), want[0].tolist())
    assert torch.equal(val.view(torch.int32), want[1].view(torch.int32)), what      # bit for bit


def _call(d, i, **kw):
    s, counts, k, _ = kc.CASES[i]
    lists = kc.lists_of(i, _chunk())
    L = len(lists)
    ids = [d["rows"][v, 0] for v in lists]
    kw.setdefault("k", k)
    return lists, L, d["m"].recommend_async(kc.first_lines(d["lines"], L), d["cat"], candidates=ids, **kw)


@pytest.mark.parametrize("i", range(len(kc.CASES)), ids=kc.IDS)
def test_logits_and_selection(i):
    """(1) sigmoid(cand_logits) against the restatement at the listed pairs within Y_TOL; the bits are those of the
    whole-catalogue call's all_logits; the lists are the stable sort of the call's own logits; -1 / -inf padding"""
    s, counts, k, _ = kc.CASES[i]
    d = _shape(s)
    lists, L, (idx, val, (off, cidx, own)) = _call(d, i, all_logits=True)
    assert idx.shape == val.shape == (L, k) and idx.dtype == torch.int32 and off.dtype == torch.int64 and cidx.dtype == torch.int32
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(v) for v in lists])]).tolist()
    total = int(off[-1])
    assert cidx[:total].tolist() == np.concatenate(lists).tolist()
    line = np.repeat(np.arange(L), [len(v) for v in lists])
    flat = np.concatenate(lists).astype(np.int64)
    got_y = torch.sigmoid(own[:total].double()).cpu().numpy()
    dy = float(np.abs(got_y - d["y"][line, flat]).max())
    print(kc.IDS[i], "max |dy| vs restatement", dy)
    assert dy < Y_TOL
    same = d["full"][torch.as_tensor(line, device=own.device), torch.as_tensor(flat, device=own.device)]
    assert torch.equal(own[:total].view(torch.int32), same.view(torch.int32))          # wherever the item stands in a list
    _hold(kc.IDS[i], idx, val, _own_selection(off, cidx, own, L, k))
    idx_h, val_h = idx.cpu().numpy(), val.cpu().numpy()
    for l in range(L):
        n = min(k, len(lists[l]))
        assert (idx_h[l][:n] >= 0).all() and np.isin(idx_h[l][:n], lists[l]).all() and np.unique(idx_h[l][:n]).size == n
        assert (idx_h[l][n:] == -1).all() and np.isneginf(val_h[l][n:]).all()
        ridx, _ = kc.select_in(d["y"][l], lists[l], k)                # the restatement's own selection, without a gap condition:
        rest = np.setdiff1d(lists[l], idx_h[l][:n])                   # nothing listed and left out beats the last returned by > 2 Y_TOL
        if rest.size:
            assert d["y"][l][rest].max() <= d["y"][l][idx_h[l][n - 1]] + 2 * Y_TOL
        assert (ridx >= 0).sum() == n


def test_the_full_list_equals_the_whole_catalogue_call():
    i = kc.EVERY_ITEM_CASE
    s, counts, k, _ = kc.CASES[i]
    d = _shape(s)
    lists, L, (idx, val) = _call(d, i)
    assert len(lists[0]) == d["N"]
    widx, wval = d["m"].recommend_async(kc.first_lines(d["lines"], L), d["cat"], k=k)
    assert torch.equal(idx, widx) and torch.equal(val.view(torch.int32), wval.view(torch.int32))
    for k2 in (1, 128):
        a = _call(d, i, k=k2)[2]
        b = d["m"].recommend_async(kc.first_lines(d["lines"], L), d["cat"], k=k2)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.mark.parametrize("i", [3, kc.RAGGED_CASE, 7], ids=[kc.IDS[3], kc.IDS[kc.RAGGED_CASE], kc.IDS[7]])
def test_repeatability_and_the_plan_size(i):
    """(3) a second call and a call without cand_logits give the same bits, the catalogue is built once; (4) an understated
    (1) and an overstated (N) max_candidates give the lists of the exact value"""
    d = _shape(kc.CASES[i][0])
    lists, L, (idx, val, (off, cidx, own)) = _call(d, i, all_logits=True)
    idx, val, own = idx.clone(), val.clone(), own.clone()
    idx2, val2, (_, _, own2) = _call(d, i, all_logits=True)[2]
    idx3, val3 = _call(d, i)[2]
    for a in (idx2, idx3):
        assert torch.equal(a, idx)
    for a, b in ((val2, val), (val3, val), (own2, own)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert d["cat"].builds == 1
    for M in (1, d["N"]):
        idx4, val4, (_, _, own4) = _call(d, i, all_logits=True, max_candidates=M)[2]
        assert torch.equal(idx4, idx) and torch.equal(val4.view(torch.int32), val.view(torch.int32)), M
        assert torch.equal(own4.view(torch.int32), own.view(torch.int32)), M
    # what ItemCatalog.candidates returns is taken as it is
    pre = d["cat"].candidates([d["rows"][v, 0] for v in lists], L)
    assert pre[2] == max(1, max(len(v) for v in lists))
    idx5, val5 = d["m"].recommend_async(kc.first_lines(d["lines"], L), d["cat"], k=kc.CASES[i][2], candidates=pre)
    assert torch.equal(idx5, idx) and torch.equal(val5.view(torch.int32), val.view(torch.int32))


def test_exclusions():
    """every third candidate, some items that are no candidates, and line 0's best candidate: none is returned, and the lists
    are the own-logit sort without them; excluded candidates keep their cand_logits"""
    i = kc.RAGGED_CASE
    d = _shape(kc.CASES[i][0])
    ids = d["rows"][:, 0]
    lists, L, (idx0, val0, (off, cidx, own0)) = _call(d, i, all_logits=True)
    own0 = own0.clone()
    best = int(idx0[0, 0])
    rng = np.random.default_rng(11)
    excl = []
    for l in range(L):
        others = np.setdiff1d(np.arange(d["N"]), lists[l])
        e = np.concatenate([lists[l][::3], rng.choice(others, size=20, replace=False)])
        excl.append(np.unique(np.concatenate([e, [best]]) if l == 0 else e))
    assert best in lists[0] and all(np.isin(e, v).any() and not np.isin(e, v).all() for e, v in zip(excl, lists))
    for k in (10, 128):
        _, _, (idx, val, (_, _, own)) = _call(d, i, all_logits=True, exclude=[rng.permutation(ids[e]) for e in excl], k=k)
        assert torch.equal(own.view(torch.int32), own0.view(torch.int32))
        _hold("exclusions k=%d" % k, idx, val, _own_selection(off, cidx, own, L, k, excl))
        got = idx.cpu().numpy()
        for l in range(L):
            assert not np.isin(got[l][got[l] >= 0], excl[l]).any()
            assert (got[l] >= 0).sum() == min(k, np.setdiff1d(lists[l], excl[l]).size)
        assert best not in got[0]
    # more exclusions between a chunk's first and last candidate than the kernel stages in LDS (512): every item up to line 0's
    # 256th candidate but four of its candidates
    keep = lists[0][[0, 7, 100, 255]]
    none = np.zeros((0,), dtype=np.int64)
    many = [np.setdiff1d(np.arange(int(lists[0][255]) + 1), keep), none, none]
    assert np.isin(lists[0][:256], many[0]).sum() == 252 and int((many[0] >= lists[0][0]).sum()) > 512
    _, _, (idx, val, (_, _, own)) = _call(d, i, all_logits=True, exclude=[ids[e] for e in many], k=128)
    assert sorted(idx[0][idx[0] >= 0].tolist()) == sorted(keep.tolist() + [int(lists[0][256])])
    _hold("a chunk all but excluded", idx, val, _own_selection(off, cidx, own, L, 128, many))


def test_equal_logits_come_back_in_ascending_index_order_across_the_lists_seams():
    """catalog_cases.tie_case: line 0's list is the copies plus 40 other items, placed so that copies stand either side of the
    LIST's tile seam (positions 15 | 16) and step seam (31 | 32) at catalogue indices that are not those positions; 48 items
    are one chunk of the list, so line 1 lists every item but one (two chunks: copies on both sides of the list's chunk seam)"""
    from score_amd import model as M
    ch = _chunk()
    kind, c, P, lines, rows, copies = cc.tie_case(ch)
    N = len(rows)
    free = np.setdiff1d(np.arange(N), copies)
    below = lambda lo, hi: free[(free >= lo) & (free < hi)]
    n_copies = lambda lo, hi: sum(lo <= p < hi for p in copies)
    a = below(0, 31)[:15 - n_copies(0, 31)]                          # catalogue 31 | 32 -> list positions 15 | 16
    b = below(33, ch - 1)[:31 - 17 - n_copies(33, ch - 1)]           # catalogue ch - 1 | ch -> list positions 31 | 32
    tail = below(ch + 1, N)[:40 - a.size - b.size]
    line0 = np.sort(np.concatenate([copies, a, b, tail])).astype(np.int32)
    assert line0.size == len(copies) + 40 and np.unique(line0).size == line0.size
    at = {int(p): int(np.nonzero(line0 == p)[0][0]) for p in copies}
    assert (at[31], at[32]) == (15, 16) and (at[ch - 1], at[ch]) == (31, 32)
    line1 = np.setdiff1d(np.arange(N), [3]).astype(np.int32)
    assert line1.size > ch and 3 not in copies and line1[ch - 1] == ch          # copy `ch` ends the list's first chunk
    m = M.MODELS[kind](*c.args)
    m.set_params(P)
    cat = M.ItemCatalog(m, rows)
    ln = tuple(lines[n] for n in ("user_seq", "user_seq_length", "target_user"))
    ids = rows[:, 0]
    idx, val, (off, cidx, own) = m.recommend_async(ln, cat, k=cc.KMAX, candidates=[ids[line0], ids[line1]], all_logits=True)
    pos = torch.as_tensor([at[p] for p in copies], device=own.device)
    eq = own[:line0.size][pos].view(torch.int32)
    assert bool((eq == eq[0]).all())                                 # the copies' logits are equal bit for bit
    _hold("ties", idx, val, _own_selection(off, cidx, own, 2, cc.KMAX))
    assert idx[0, :len(copies)].tolist() == copies                   # they share line 0's best logit: they lead, ascending
    assert int((idx[0] >= 0).sum()) == line0.size
    got = idx[1].tolist()                                            # line 1: those in the list are adjacent and ascending
    where = [got.index(p) for p in copies if p in got]
    assert where == list(range(where[0], where[0] + len(where))) if where else True
    for k in (1, 3, 10):                                             # a list that ends inside the run of equal logits
        i2, v2 = m.recommend_async(ln, cat, k=k, candidates=[ids[line0], ids[line1]])
        assert i2[0, :len(copies)].tolist() == copies[:k]
        _hold("ties k=%d" % k, i2, v2, _own_selection(off, cidx, own, 2, k))


def test_an_index_outside_the_catalogue_is_never_returned_and_reads_nothing():
    """-1 in front of and N behind an ascending list, handed over as ItemCatalog.candidates would hand it (the mapping itself
    cannot produce them): never selected, NaN in cand_logits, every other result as without them"""
    i = kc.RAGGED_CASE
    d = _shape(kc.CASES[i][0])
    lists, L, (idx0, val0, (off0, cidx0, own0)) = _call(d, i, all_logits=True, k=128)
    idx0, val0, own0 = idx0.clone(), val0.clone(), own0.clone()
    N = d["N"]
    bad = [np.concatenate([[-1], lists[0], [N]]), np.concatenate([lists[1], [N]]), np.concatenate([[-1], lists[2]])]
    off = torch.as_tensor(np.concatenate([[0], np.cumsum([len(v) for v in bad])]), dtype=torch.int64, device=own0.device)
    cidx = torch.as_tensor(np.concatenate(bad), dtype=torch.int32, device=own0.device)
    for M in (max(len(v) for v in bad), 1):
        idx, val, (_, _, own) = d["m"].recommend_async(kc.first_lines(d["lines"], L), d["cat"], k=128, candidates=(off, cidx, M),
                                                       all_logits=True)
        assert torch.equal(idx, idx0) and torch.equal(val.view(torch.int32), val0.view(torch.int32))
        outside = (cidx < 0) | (cidx >= N)
        assert int(outside.sum()) == 4 and bool(torch.isnan(own[outside]).all())
        assert torch.equal(own[~outside].view(torch.int32), own0[:int(off0[-1])].view(torch.int32))
    # with exclusions: the window into the line's exclusions is found from the indices inside the catalogue
    excl = [lists[l][::2] for l in range(L)]
    ids = d["rows"][:, 0]
    want = _call(d, i, k=128, exclude=[ids[e] for e in excl])[2]
    got = d["m"].recommend_async(kc.first_lines(d["lines"], L), d["cat"], k=128, candidates=(off, cidx, 1),
                                 exclude=[ids[e] for e in excl])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    d["m"].check_ids()                                               # nothing was reported


def test_evaluate_catalog_within_each_lines_own_candidates_on_the_tmall_sample():
    from score_amd import dataprep as dp
    from score_amd import harness as h
    from score_amd import model as M
    from score_amd.pointdata import DeviceDataLoaderUserSeq
    log = np.load(os.path.join(GOLDEN, "tmall_sample_log.npz"))["log"]
    stores, r = dp.tmall_point_stores(log, dual=False, batch_size=1000)
    st = stores["validation"]
    T, neg, k = 50, 99, 100
    m = M.GRU4Rec(r["feature_size"], 16, 32, T, 3, 4, seed=7)
    batches = list(DeviceDataLoaderUserSeq(1000, T, None, None, neg, None, None, model=m, store=st))
    for s in range(10):
        m.train(None, batches[s % len(batches)], 1e-2, 1e-4)
    cat = M.ItemCatalog(m, st.item_rows)
    whole = h.evaluate_catalog(m, batches, cat, neg, k=k, return_lists=True)
    six, top, tgt = h.evaluate_catalog(m, batches, cat, neg, k=k, return_lists=True, candidates="line")
    assert h.evaluate_catalog(m, batches, cat, neg, k=k, candidates="line") == six and len(six) == 6
    # every line's list: the own-logit sort of the line's distinct candidate indices
    ids = np.asarray(st.item_rows)[:, 0]
    at, n_lines, collapsed = 0, 0, 0
    for b in batches:
        lines = m.lines_of(b, neg)
        L = int(lines[1].numel())
        items = b.tensors[5].view(L, neg + 1, -1)[:, :, 0]
        per_line = [np.unique(x) for x in items.cpu().numpy()]
        collapsed += sum(v.size < neg + 1 for v in per_line)
        assert all(np.isin(v, ids).all() for v in per_line)
        idx, val, (off, cidx, own) = m.recommend_async(lines, cat, k=k, candidates=[v for v in per_line], all_logits=True,
                                                       active_slices=b.active_slices)
        assert np.diff(off.cpu().numpy()).tolist() == [v.size for v in per_line]
        assert cidx.tolist() == np.concatenate([np.searchsorted(ids, v) for v in per_line]).tolist()
        want = _own_selection(off, cidx, own, L, k)
        assert torch.equal(top[at:at + L], want[0]) and torch.equal(idx, want[0])
        pos = tgt[at:at + L]
        assert bool((top[at:at + L] == pos[:, None]).any(1).all())           # the positive is always in its line's list
        at += L
        n_lines += L
    assert at == top.shape[0] == tgt.shape[0] and torch.equal(tgt, whole[2])
    print("tmall sample: %d lines, %d with repeated negatives" % (n_lines, collapsed), six, whole[0])
    assert six == h.catalog_quality_device(top, tgt)
    # without candidates: as before -- the whole catalogue's lists, through the same arithmetic
    assert h.evaluate_catalog(m, batches, cat, neg, k=k) == whole[0] == h.catalog_quality_device(whole[1], whole[2])
    tops = [m.recommend_async(m.lines_of(b, neg), cat, k=k, active_slices=b.active_slices)[0].clone() for b in batches]
    assert torch.equal(torch.cat(tops), whole[1])
    assert all(a >= b for a, b in zip(six, whole[0]))                        # fewer rivals: the positive stands no lower
