"""Top-K over a whole item catalogue on the GPU (GRU4Rec.recommend / Caser.recommend; csrc/catalog.hip, score_catalog_topk): the
logits of every (line, item) pair against the float64 restatement (tests/catalog_cases.py) and against rank_async on the expanded
batch, the selection against a stable sort of the call's own logits -- bit for bit --, ties across tile and chunk seams,
exclusions, the restatement's selection without a gap condition, a catalogue gone stale, ids at their edges, and
harness.evaluate_catalog on the bundled Tmall sample."""
import functools
import os

import numpy as np
import pytest
import torch

import catalog_cases as cc
import rank_cases as rc
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

Y_TOL = 1e-4              # max |dy|: tests/test_gpu_rank.py, from tests/test_gpu_gru4rec.py::_check


def _model(kind, c, P):
    from score_amd import model as M
    m = M.MODELS[kind](*c.args)
    m.set_params(P)
    return m


def _cfg_of(kind, c):
    from score_amd import _lib
    return _lib.make_config(c.N, c.D, c.H, c.T, 1, c.Fu, c.Fi, kind)


def _chunk(kind, c, L, k):
    """the plan's chunk for a small catalogue of this case, and N of the case from it (asserted to be self-consistent)"""
    from score_amd import _lib
    return _lib.catalog_plan(_cfg_of(kind, c), L, 1, k)[0]


@functools.lru_cache(maxsize=None)
def _case(i, moved=False):
    """case i: inputs, the restatement (computed once, never modified)"""
    from score_amd import _lib
    s, L, n_of, k, _ = cc.CASES[i]
    kind, dims = cc.SHAPES[s]
    c = rc.cfg_of(kind, dims)
    ch = _chunk(kind, c, L, k)
    N = n_of(ch)
    chunk, nchunk, _ = _lib.catalog_plan(_cfg_of(kind, c), L, N, k)
    assert chunk == ch and nchunk == -(-N // ch)              # the seams are where the case says they are
    P = rc.params_of(kind, c, moved)
    lines, rows = cc.lines_of(kind, c, L, 100 + i), cc.catalog_rows(c, N, 200 + i)
    logits, y = cc.restated(kind, c, P, lines, rows)
    logits.setflags(write=False); y.setflags(write=False)
    return dict(kind=kind, c=c, P=P, lines=lines, rows=rows, L=L, N=N, k=k, chunk=ch, nchunk=nchunk, logits=logits, y=y)


def _lines(d):
    return tuple(d["lines"][n] for n in ("user_seq", "user_seq_length", "target_user"))


def _own_selection(full, k, excl=None):
    """the stable sort of the call's OWN logits by (-logit, index) on the device, exclusions removed, -1 / -inf padding"""
    L, N = full.shape
    idx = torch.full((L, k), -1, dtype=torch.int32, device=full.device)
    val = torch.full((L, k), float("-inf"), dtype=torch.float32, device=full.device)
    for l in range(L):
        order = torch.sort(-full[l], stable=True).indices
        if excl is not None and len(excl[l]):
            gone = torch.zeros((N,), dtype=torch.bool, device=full.device)
            gone[torch.as_tensor(np.asarray(excl[l]), device=full.device).long()] = True
            order = order[~gone[order]]
        order = order[:k]
        idx[l, :order.numel()] = order.to(torch.int32)
        val[l, :order.numel()] = full[l][order]
    return idx, val


def _hold_selection(what, idx, val, full, k, excl=None):
    widx, wval = _own_selection(full, k, excl)
    assert torch.equal(idx, widx), (what, idx.tolist(), widx.tolist())
    assert torch.equal(val.view(torch.int32), wval.view(torch.int32)), what      # bit for bit


def test_the_cases_hit_every_size_the_plan_has_a_seam_at():
    sizes, k_above_n, short_last = set(), 0, 0
    for i in range(len(cc.CASES)):
        d = _case(i)
        ch, N = d["chunk"], d["N"]
        assert ch > 0 and ch % 16 == 0
        for name, v in (("1", 1), ("15", 15), ("16", 16), ("17", 17), ("chunk-1", ch - 1), ("chunk", ch), ("chunk+1", ch + 1),
                        ("2chunk+1", 2 * ch + 1)):
            if N == v:
                sizes.add(name)
        k_above_n += d["k"] > N
        short_last += d["nchunk"] > 1 and N - (d["nchunk"] - 1) * ch < d["k"]
    assert sizes == {"1", "15", "16", "17", "chunk-1", "chunk", "chunk+1", "2chunk+1"}
    assert k_above_n >= 1 and short_last >= 1
    assert {cc.CASES[i][1] for i in range(len(cc.CASES))} == {1, 3} and {cc.CASES[i][3] for i in range(len(cc.CASES))} == {1, 10, 128}


@pytest.mark.parametrize("i,moved", [(i, False) for i in range(len(cc.CASES))] + [(1, True), (4, True), (7, True)],
                         ids=cc.IDS + [cc.IDS[i] + "-moved" for i in (1, 4, 7)])
def test_logits_selection_and_the_restatement(i, moved):
    """(1) sigmoid(all_logits) against the restatement and against rank_async on the expanded batch, within Y_TOL; (2) the lists
    equal the stable sort of the call's own logits, with and without all_logits and on a second call; (5) against the
    restatement's scores without a gap condition: nothing left out beats the K-th returned item by more than 2 Y_TOL"""
    from score_amd import model as M
    d = _case(i, moved)
    kind, c, L, N, k = d["kind"], d["c"], d["L"], d["N"], d["k"]
    m = _model(kind, c, d["P"])
    cat = M.ItemCatalog(m, d["rows"])
    idx, val, full = m.recommend_async(_lines(d), cat, k=k, all_logits=True)
    assert idx.shape == val.shape == (L, k) and full.shape == (L, N) and idx.dtype == torch.int32
    y = torch.sigmoid(full.double()).cpu().numpy()
    dy = float(np.abs(y - d["y"]).max())
    bt = rc.REF[kind].batch_tuple(cc.expanded(d["lines"], d["rows"]))
    ry = m.rank_async(bt, 0.0, neg_sample_num=N - 1)[0].double().cpu().numpy().reshape(L, N)
    dr = float(np.abs(y - ry).max())
    print(cc.IDS[i], "moved" if moved else "initial", "max |dy| vs restatement", dy, "vs rank_async", dr)
    assert dy < Y_TOL and dr < Y_TOL
    # (2)
    _hold_selection(cc.IDS[i], idx, val, full, k)
    idx2, val2 = m.recommend_async(_lines(d), cat, k=k)
    idx3, val3, full3 = m.recommend_async(_lines(d), cat, k=k, all_logits=True)
    for a, b in ((idx, idx2), (idx, idx3)):
        assert torch.equal(a, b)
    for a, b in ((val, val2), (val, val3), (full, full3)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert cat.builds == 1
    # (5)
    idx_h, val_h = idx.cpu().numpy(), val.cpu().numpy()
    for l in range(L):
        got = idx_h[l][idx_h[l] >= 0]
        assert got.size == min(k, N) and np.unique(got).size == got.size
        assert (np.diff(val_h[l][:got.size]) <= 0).all()
        assert (idx_h[l][got.size:] == -1).all() and np.isneginf(val_h[l][got.size:]).all()
        rest = np.setdiff1d(np.arange(N), got)
        if rest.size:
            assert d["y"][l][rest].max() <= d["y"][l][got[-1]] + 2 * Y_TOL, (l, d["y"][l][rest].max(), d["y"][l][got[-1]])


def test_equal_logits_come_back_in_ascending_index_order_across_tile_and_chunk_seams():
    from score_amd import _lib
    from score_amd import model as M
    kind, dims = cc.SHAPES[0]
    ch = _chunk(kind, rc.cfg_of(kind, dims), 2, cc.KMAX)
    kind, c, P, lines, rows, copies = cc.tie_case(ch)
    N = len(rows)
    assert _lib.catalog_plan(_cfg_of(kind, c), 2, N, cc.KMAX)[:2] == (ch, 2)
    assert {15, 16, 31, 32, ch - 1, ch, N - 1} <= set(copies)         # either side of a tile, a step and the chunk seam
    m = _model(kind, c, P)
    cat = M.ItemCatalog(m, rows)
    ln = tuple(lines[n] for n in ("user_seq", "user_seq_length", "target_user"))
    idx, val, full = m.recommend_async(ln, cat, k=cc.KMAX, all_logits=True)
    at = full[:, torch.as_tensor(copies, device=full.device)].view(torch.int32)
    assert bool((at == at[:, :1]).all())                             # the copies' logits are equal bit for bit, on every line
    _hold_selection("ties", idx, val, full, cc.KMAX)
    # line 0: the copies share its best logit (catalog_cases.tie_case), so they lead the list, ascending
    assert idx[0, :len(copies)].tolist() == copies
    for l in range(2):                                               # any line: the copies that are in the list are adjacent and ascending
        got = idx[l].tolist()
        pos = [got.index(p) for p in copies if p in got]
        assert pos == list(range(pos[0], pos[0] + len(pos))) if pos else True
    for k in (1, 3, 10):                                             # a list that ends inside the run of equal logits (or just behind it)
        i2, v2 = m.recommend_async(ln, cat, k=k)
        assert i2[0, :len(copies)].tolist() == copies[:k]
        _hold_selection("ties k=%d" % k, i2, v2, full, k)


def test_exclusions():
    """empty lists, a list that removes a line's current best, one that removes a whole chunk, one that leaves fewer than k
    items; given unsorted and with repeats and ids the catalogue does not hold; as a list per line and as a CSR pair"""
    from score_amd import model as M
    d = _case(8)                                                     # GRU4Rec, L = 3, two chunks + 1
    kind, c, L, N, ch = d["kind"], d["c"], d["L"], d["N"], d["chunk"]
    assert L == 3 and N == 2 * ch + 1
    m = _model(kind, c, d["P"])
    cat = M.ItemCatalog(m, d["rows"])
    ids = d["rows"][:, 0]
    k = 10
    idx0, val0, full = m.recommend_async(_lines(d), cat, k=k, all_logits=True)
    best = idx0[:, 0].tolist()
    rng = np.random.default_rng(3)
    absent = np.setdiff1d(np.arange(1, c.N), ids)[:5]
    keep = rng.choice(N, size=4, replace=False)                      # line 2 keeps four items: fewer than k
    excl_idx = [np.zeros((0,), dtype=np.int64),
                np.concatenate([[best[1]], np.arange(ch, 2 * ch)]),  # line 1: its best, and the whole second chunk
                np.setdiff1d(np.arange(N), keep)]
    unsorted = [np.concatenate([rng.permutation(ids[e]), ids[e][:3], absent]).astype(np.int64) for e in excl_idx]
    idx, val, full2 = m.recommend_async(_lines(d), cat, k=k, exclude=unsorted, all_logits=True)
    assert torch.equal(full.view(torch.int32), full2.view(torch.int32))          # excluded items keep their logits
    _hold_selection("exclusions", idx, val, full, k, excl_idx)
    got = idx.cpu().numpy()
    assert torch.equal(idx[0], idx0[0]) and best[1] not in got[1] and not ((got[1] >= ch) & (got[1] < 2 * ch)).any()
    assert sorted(got[2][:4].tolist()) == sorted(keep.tolist()) and (got[2][4:] == -1).all()
    off = np.concatenate([[0], np.cumsum([len(u) for u in unsorted])]).astype(np.int64)
    idx_c, val_c = m.recommend_async(_lines(d), cat, k=k, exclude=(off, np.concatenate(unsorted)))
    assert torch.equal(idx_c, idx) and torch.equal(val_c.view(torch.int32), val.view(torch.int32))
    idx_e, val_e = m.recommend_async(_lines(d), cat, k=k, exclude=[[], [], []])
    assert torch.equal(idx_e, idx0) and torch.equal(val_e.view(torch.int32), val0.view(torch.int32))
    # the synchronous form: item ids and scores, the padding dropped
    rec_ids, rec_y = m.recommend(_lines(d), cat, k=k, exclude=unsorted)
    assert [len(x) for x in rec_ids] == [10, 10, 4] == [len(x) for x in rec_y]
    assert rec_ids[1] == ids[got[1]].tolist()
    assert np.allclose(rec_y[1], torch.sigmoid(val[1]).cpu().numpy(), rtol=0, atol=1e-6)
    # k = 128 against a chunk that is excluded entirely and a last chunk of one item
    idx128, val128 = m.recommend_async(_lines(d), cat, k=128, exclude=unsorted)
    _hold_selection("exclusions k=128", idx128, val128, full, 128, excl_idx)


def test_a_catalogue_built_before_a_train_step_is_rebuilt():
    from score_amd import model as M
    d = _case(3)                                                     # GRU4Rec (8, 48, 7, 2, 2), L = 3, N = 17
    kind, c, k = d["kind"], d["c"], 5
    m = _model(kind, c, d["P"])
    cat = M.ItemCatalog(m, d["rows"])
    before = [t.clone() for t in m.recommend_async(_lines(d), cat, k=k, all_logits=True)]
    stale = cat.zcat.clone()
    assert cat.builds == 1 and cat.version == m.weights_version
    bt = rc.REF[kind].batch_tuple(cc.expanded(d["lines"], d["rows"]))
    for _ in range(3):
        m.train(None, bt, 1e-2, 1e-4)
    assert cat.version != m.weights_version
    got = m.recommend_async(_lines(d), cat, k=k, all_logits=True)
    assert cat.builds == 2 and cat.version == m.weights_version
    fresh = m.recommend_async(_lines(d), M.ItemCatalog(m, d["rows"]), k=k, all_logits=True)
    for a, b in zip(got, fresh):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(cat.zcat, stale) and not torch.equal(got[2], before[2])
    cat.zcat.copy_(stale)                                            # what the stale catalogue would give
    old = m.recommend_async(_lines(d), cat, k=k, all_logits=True)
    assert cat.builds == 2 and not torch.equal(old[2], fresh[2])
    m.set_params(d["P"])                                             # set_params moves the counter too: back at the first answer
    again = m.recommend_async(_lines(d), cat, k=k, all_logits=True)
    assert cat.builds == 3
    for a, b in zip(again, before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("s", [0, 2], ids=["GRU4Rec", "Caser"])
def test_the_dummy_id_and_lengths_at_their_edges(s):
    """id 0 as an item id, as a feature of another row and in a history; lengths 1, T and above T in one call"""
    from score_amd import model as M
    kind, dims = cc.SHAPES[s]
    c = rc.cfg_of(kind, dims)
    P = rc.params_of(kind, c, moved=True)
    L, N, k = 3, 33, 10
    lines, rows = cc.lines_of(kind, c, L, 31), cc.catalog_rows(c, N, 32)
    rows[0, :] = 0                                                   # (0 is the lowest id: column 0 stays ascending)
    rows[N - 1, c.Fi - 1] = 0
    lines["user_seq"][1, 0, :] = 0
    lines["user_seq"][2, 2, 0] = 0
    lines["user_seq_length"][:] = np.asarray([1, c.T, c.T + 3], dtype=np.int32)
    logits, y = cc.restated(kind, c, P, lines, rows)
    m = _model(kind, c, P)
    cat = M.ItemCatalog(m, rows)
    ln = tuple(lines[n] for n in ("user_seq", "user_seq_length", "target_user"))
    idx, val, full = m.recommend_async(ln, cat, k=k, all_logits=True)
    dy = float(np.abs(torch.sigmoid(full.double()).cpu().numpy() - y).max())
    print(kind, "id 0, lengths 1 / T / T + 3: max |dy|", dy)
    assert dy < Y_TOL
    _hold_selection("id 0", idx, val, full, k)
    m.check_ids()                                                    # nothing was reported


def test_an_id_outside_the_table_in_item_rows_sets_bit_5_and_recommend_raises():
    from score_amd import model as M
    d = _case(1)                                                     # GRU4Rec, L = 3, N = 15
    kind, c, k = d["kind"], d["c"], 10
    m, clean = _model(kind, c, d["P"]), _model(kind, c, d["P"])
    bad = d["rows"].copy()
    bad[d["N"] - 1, 1] = c.N                                         # feature_size itself, in the ragged tile's last row
    with pytest.raises(ValueError, match="strictly ascending"):
        M.ItemCatalog(m, d["rows"][::-1].copy())
    cat = M.ItemCatalog(m, bad)
    m.recommend_async(_lines(d), cat, k=k)
    assert int(m._id_status[0].item()) == 1 << 5
    with pytest.raises(ValueError, match=r"batch_data\[3\] \(target_item\)"):
        m.check_ids()
    with pytest.raises(ValueError, match=r"batch_data\[3\] \(target_item\)"):
        m.recommend(_lines(d), M.ItemCatalog(m, bad), k=k)                   # (a new catalogue: its build reports again)
    assert torch.equal(m.table, clean.table) and torch.equal(m.w, clean.w)
    # a bad id in a line tensor: bit 0; then a good call gives what a fresh model gives
    lines = {n: v.copy() for n, v in d["lines"].items()}
    lines["user_seq"][1, 0, 0] = c.N
    good = M.ItemCatalog(m, d["rows"])
    with pytest.raises(ValueError, match=r"batch_data\[0\] \(user_seq\)"):
        m.recommend(tuple(lines[n] for n in ("user_seq", "user_seq_length", "target_user")), good, k=k)
    assert m.recommend(_lines(d), good, k=k) == clean.recommend(_lines(d), M.ItemCatalog(clean, d["rows"]), k=k)


# ---- end to end: the bundled Tmall sample's validation lines against the store's whole item table ---------------------------
def _quality_on_the_host(full, target, k, excl=None):
    """the six numbers from all_logits [n_lines, N] on the host: the positive's position in the order (logit descending, index
    ascending) among the items that are not excluded, counted only inside the first k"""
    import math
    r = []
    for l in range(full.shape[0]):
        idx, _ = cc.select(full[l], k, None if excl is None else excl[l])
        hit = np.nonzero(idx == target[l])[0]
        r.append(int(hit[0]) if hit.size else -1)
    r = np.asarray(r, dtype=np.float64)
    found = r >= 0
    r = np.maximum(r, 0)
    gain = np.where(found, math.log(2) / np.log(r + 2), 0.0)
    return (float(np.mean(np.where(r < 5, gain, 0.0))), float(np.mean(np.where(r < 10, gain, 0.0))), float(np.mean(found & (r < 1))),
            float(np.mean(found & (r < 5))), float(np.mean(found & (r < 10))), float(np.mean(np.where(found, 1.0 / (r + 1), 0.0))))


def test_evaluate_catalog_on_the_tmall_sample():
    from score_amd import dataprep as dp
    from score_amd import harness as h
    from score_amd import model as M
    from score_amd.pointdata import DeviceDataLoaderUserSeq
    log = np.load(os.path.join(GOLDEN, "tmall_sample_log.npz"))["log"]
    stores, r = dp.tmall_point_stores(log, dual=False, batch_size=1000)
    st = stores["validation"]
    T, neg, k = 50, 99, 10
    m = M.GRU4Rec(r["feature_size"], 16, 32, T, 3, 4, seed=7)
    batches = list(DeviceDataLoaderUserSeq(1000, T, None, None, neg, None, None, model=m, store=st))
    for s in range(60):                                              # (as test_gpu_rank.py's trained row: the positives stand out)
        m.train(None, batches[s % len(batches)], 1e-2, 1e-4)
    cat = M.ItemCatalog(m, st.item_rows)
    N = cat.N
    assert N == len(st.item_rows) and N > 100
    six, top, tgt = h.evaluate_catalog(m, batches, cat, neg, k=k, return_lists=True)
    assert h.evaluate_catalog(m, batches, cat, neg, k=k) == six and len(six) == 6
    # the same from all_logits, on the host
    fulls, users, pos = [], [], []
    for b in batches:
        lines = m.lines_of(b, neg)
        fulls.append(m.recommend_async(lines, cat, k=k, all_logits=True, active_slices=b.active_slices)[2].cpu().numpy())
        users.append(lines[2][:, 0].cpu().numpy())
        pos.append(b.tensors[5].view(-1, neg + 1, 4)[:, 0, 0].cpu().numpy())
    full, users, pos = np.concatenate(fulls), np.concatenate(users), np.concatenate(pos)
    ids = np.asarray(st.item_rows)[:, 0]
    target = np.searchsorted(ids, pos)
    assert (ids[target] == pos).all() and np.array_equal(target, tgt.cpu().numpy())
    want = _quality_on_the_host(full, target, k)
    print("tmall sample: %d lines against %d items" % (full.shape[0], N), six, want)
    assert np.allclose(six, want, rtol=0, atol=1e-6), (six, want)
    # the same arithmetic where every position occurs, whatever the model has learnt: line l's "positive" is the item at
    # position l % 12 of its own order (10 and 11: behind the list)
    alt = np.asarray([cc.select(full[l], 12)[0][l % 12] for l in range(full.shape[0])], dtype=np.int32)
    six_alt = h.catalog_quality_device(top, torch.from_numpy(alt).to(top.device))
    want_alt = _quality_on_the_host(full, alt, k)
    print("positions 0 .. 11 in turn", six_alt, want_alt)
    assert np.allclose(six_alt, want_alt, rtol=0, atol=1e-6) and 0.7 < want_alt[4] < 0.9 and want_alt[2] > 0.05
    # with the users' histories excluded: no returned item lies in its user's history (the positive may)
    arr = st.arrays()
    off, seq = arr["user_hist_off"], arr["user_hist_seq"]
    hist = [seq[off[u - 1]:off[u]] for u in users]
    six_x, top_x, tgt_x = h.evaluate_catalog(m, batches, cat, neg, k=k, exclude_history=st, return_lists=True)
    top_x = top_x.cpu().numpy()
    assert (top_x >= 0).all() and np.array_equal(tgt_x.cpu().numpy(), target)
    excl = []
    for l in range(len(users)):
        mine = np.setdiff1d(hist[l], [pos[l]])
        assert not np.isin(ids[top_x[l]], mine).any(), l
        excl.append(np.searchsorted(ids, mine))
    assert sum(len(e) for e in excl) > 0
    want_x = _quality_on_the_host(full, target, k, excl)
    print("with the histories excluded", six_x, want_x)
    assert np.allclose(six_x, want_x, rtol=0, atol=1e-6), (six_x, want_x)
