"""Recommend by user id on the GPU: PointLogStore.user_lines (csrc/pointloader.hip: score_point_user_lines) integer for integer
against host_user_lines and against lines_of(device loader batch); recommend_users_async bit for bit against the parent's route
(loader batch -> lines_of -> harness._history_exclusions -> recommend_async(exclude=)); harness.evaluate_catalog_users against
evaluate_catalog on the bundled Tmall sample.  The scoring kernels' inputs are integer-identical on both routes, so nothing
here has a tolerance."""
import functools
import os

import numpy as np
import pytest
import torch

import catalog_cases as cc
import rank_cases as rc
import user_line_cases as uc
from helpers import GOLDEN

pytestmark = pytest.mark.gpu


# ---- the lines --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lines_store(Fu, Fi):
    return uc.store_of(uc.lines_world(Fu, Fi), "device")


def _same(got, want, what):
    for g, w, name in zip(got, want, ("user_seq", "length", "target_user", "known")):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (what, name)


@pytest.mark.parametrize("T", uc.T_LINES)
@pytest.mark.parametrize("Fu,Fi", uc.SHAPES_LINES)
def test_user_lines_equal_the_host_form_and_the_loaders_lines(Fu, Fi, T):
    from score_amd import model as M
    from score_amd.pointdata import DeviceDataLoaderUserSeq
    st = _lines_store(Fu, Fi)
    U, counts = st.n_users, list(uc.COUNTS_LINES)
    assert st.hist_max_len == uc.H_LINES and st.max_user_len == uc.H_LINES and st.max_user_events == max(counts)
    assert np.diff(st.arrays()["user_hist_off"]).tolist() == counts
    assert {0, 1, T - 1, T, T + 1} <= set(counts) and max(counts) > uc.H_LINES and counts[0] > 0 and counts[-1] > 0
    every = np.arange(1, U + 1, dtype=np.int32)
    # L = 1 (each user alone), L = 5, every user, the same user twice, ids 1 and U, unknown ids between known ones
    calls = [[u] for u in every.tolist()] + [[4, 2, 8, 5, 3], every.tolist(), [6, 6], [1, U], [3, 0, U + 1, -3, 7]]
    for users in calls:
        got = st.user_lines(np.asarray(users, dtype=np.int32), T)
        assert got[0].shape == (len(users), T, Fi) and all(g.is_cuda and g.dtype == torch.int32 for g in got)
        _same(got, st.host_user_lines(users, T), users)
    seq, ln, tu, known = (g.cpu().numpy() for g in st.user_lines(torch.as_tensor([3, 0, U + 1, -3, 7, 2], device=st.device), T))
    assert known.tolist() == [1, 0, 0, 0, 1, 1] and ln[[1, 2, 3, 5]].tolist() == [0, 0, 0, 0]
    assert not seq[[1, 2, 3, 5]].any() and not tu[1:4].any() and tu[5, 0] == 2 and seq[0].any() and seq[4].any()
    # the store's own lines: what lines_of takes from the device loader's batch
    m = M.GRU4Rec(100, 8, 8, T, Fu, Fi, seed=3)
    batches = list(DeviceDataLoaderUserSeq(st.batch_size, T, None, None, uc.NEG_LINES, None, None, model=m, store=st))
    assert len(batches) == 1
    want = m.lines_of(batches[0], uc.NEG_LINES)
    got = st.user_lines(st._dev["line_user"], T)
    for g, w in zip(got[:3], want):
        assert torch.equal(g, w)
    assert bool(got[3].all())


# ---- end to end ---------------------------------------------------------------------------------------------------------------
U_E2E, I_E2E, NEG_E2E, H_E2E, K_E2E = 40, 2 * 256 + 1, 9, 30, 10


@functools.lru_cache(maxsize=None)
def _e2e(s):
    """shape s of catalog_cases.SHAPES: the model, a store of a few thousand events whose users and items are rows of its table,
    the catalogue over the store's items, and the store's one loader batch"""
    from score_amd import model as M
    from score_amd.pointdata import DeviceDataLoaderUserSeq, PointLogStore
    kind, dims = cc.SHAPES[s]
    c = rc.cfg_of(kind, dims)
    rng = np.random.default_rng(40 + s)
    counts = rng.integers(0, 2 * H_E2E, U_E2E)
    counts[:4] = (3, 0, c.T, 2 * H_E2E + 7)
    log = uc.crafted_log(counts.tolist(), I_E2E, seed=50 + s)
    ur, ir = uc.rows_of(U_E2E, I_E2E, c.Fu, c.Fi, c.N, seed=60 + s)
    per = 1 + NEG_E2E
    lines = uc.target_lines(log[0], log[3], uc.WINDOW, U_E2E, I_E2E, per, 12, seed=70 + s)
    st = PointLogStore(*log, lines, uc.WINDOW[0], uc.WINDOW[1], H_E2E, NEG_E2E, 12 * per, ur, ir, False, build="device")
    m = M.MODELS[kind](*c.args)
    m.set_params(rc.params_of(kind, c))
    cat = M.ItemCatalog(m, ir)
    batch = next(iter(DeviceDataLoaderUserSeq(12 * per, c.T, None, None, NEG_E2E, None, None, model=m, store=st)))
    return dict(m=m, st=st, cat=cat, batch=batch, c=c, per=per)


def _bits(a, b, what):
    assert torch.equal(a[0], b[0]), what
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), what


@pytest.mark.parametrize("s", (0, 1, 2), ids=lambda s: "%s-%s" % (cc.SHAPES[s][0], "x".join(str(x) for x in cc.SHAPES[s][1])))
def test_recommend_users_equals_the_parents_route_bit_for_bit(s):
    from score_amd import harness as h
    d = _e2e(s)
    m, st, cat, batch, per = d["m"], d["st"], d["cat"], d["batch"], d["per"]
    lines = m.lines_of(batch, NEG_E2E)
    L = int(lines[1].numel())
    users = st._dev["line_user"]
    items = batch.tensors[5].view(L, per, -1)[:, :, 0]
    pos = items[:, 0].contiguous()
    assert torch.equal(lines[2][:, 0], users) and L == 12
    excl = h._history_exclusions(st, users, pos)
    assert int(excl[0][-1]) > L                                             # there is something to exclude
    own = (torch.arange(L + 1, device=pos.device, dtype=torch.int64) * per, items.reshape(-1).contiguous())
    for k in (K_E2E, 128):
        # with the history excluded
        want = [t.clone() for t in m.recommend_async(lines, cat, k=k, exclude=excl, active_slices=batch.active_slices)]
        got = m.recommend_users_async(users, st, cat, k=k, exclude_history=True, keep=pos)
        assert len(got) == 3 and bool(got[2].all())
        _bits(got, want, ("exclude", k))
        # ... and the bound on active_slices does not show: the same lines and lists at active_slices=None
        ul = st.user_lines(users, d["c"].T)
        xi = cat.history_exclusions(st, users, pos)
        _bits(m.recommend_async(ul[:3], cat, k=k, exclude_idx=xi, active_slices=None), want, ("active_slices=None", k))
        # without exclusion
        want = [t.clone() for t in m.recommend_async(lines, cat, k=k, active_slices=batch.active_slices)]
        _bits(m.recommend_users_async(users, st, cat, k=k, exclude_history=False), want, ("no exclusion", k))
        # within each line's own candidates, with and without the history excluded
        want = [t.clone() for t in m.recommend_async(lines, cat, k=k, exclude=excl, active_slices=batch.active_slices, candidates=own)]
        _bits(m.recommend_users_async(users, st, cat, k=k, keep=pos, candidates=own), want, ("candidates", k))
        _bits(m.recommend_users_async(users, st, cat, k=k, keep=pos, candidates=own, max_candidates=per), want, ("max_candidates", k))
    full = m.recommend_users_async(users, st, cat, k=K_E2E, exclude_history=False, all_logits=True)
    assert len(full) == 4 and full[3].shape == (L, cat.N)
    assert cat.builds == 1
    with pytest.raises(ValueError, match="mutually exclusive"):
        m.recommend_async(lines, cat, exclude=excl, exclude_idx=xi)


def test_unknown_users_and_a_stale_catalogue():
    d = _e2e(0)
    m, st, cat, batch = d["m"], d["st"], d["cat"], d["batch"]
    U = st.n_users
    users = [1, 2, U + 5, 4, 0]
    idx, logit, known = m.recommend_users_async(users, st, cat, k=K_E2E)          # raises nothing: known says so
    assert known.tolist() == [1, 1, 0, 1, 0] and bool((idx >= 0).all())
    assert torch.equal(idx[2], idx[4]) and torch.equal(logit[2], logit[4])           # both a cold user with a zero user row
    with pytest.raises(ValueError, match="user id %d " % (U + 5)):
        m.recommend_users(users, st, cat, k=K_E2E)
    ids, scores = m.recommend_users([1, 2, 4], st, cat, k=K_E2E)
    want = m.recommend((st.user_lines([1, 2, 4], d["c"].T)[:3]), cat, k=K_E2E,
                       exclude=[st.arrays()["user_hist_seq"][st.arrays()["user_hist_off"][u - 1]:st.arrays()["user_hist_off"][u]]
                                for u in (1, 2, 4)])
    assert ids == want[0] and scores == want[1] and all(len(x) == K_E2E for x in ids)
    # the catalogue goes stale between two calls: one rebuild, however many calls follow
    builds = cat.builds
    m.train(None, batch, 1e-2, 1e-4)
    a = m.recommend_users_async(users, st, cat, k=K_E2E)
    a = [t.clone() for t in a]
    b = m.recommend_users_async(users, st, cat, k=K_E2E)
    assert cat.builds == builds + 1 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # a store that does not go with the model or the catalogue
    other = uc.store_of(uc.lines_world(1, 1), "device")
    with pytest.raises(ValueError, match="user_fnum, item_fnum"):
        m.recommend_users_async([1], other, cat)
    w = uc.lines_world(d["c"].Fu, d["c"].Fi)
    with pytest.raises(ValueError, match="catalogue holds an item"):
        m.recommend_users_async([1], uc.store_of(w, "device"), cat)


def test_evaluate_catalog_users_on_the_tmall_sample():
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
    for s in range(3):
        m.train(None, batches[s % len(batches)], 1e-2, 1e-4)
    cat = M.ItemCatalog(m, st.item_rows)
    for kw_old, kw_new in ((dict(exclude_history=st), dict(exclude_history=True)), (dict(), dict(exclude_history=False)),
                           (dict(exclude_history=st, candidates="line"), dict(exclude_history=True, candidates="line")),
                           (dict(candidates="line"), dict(exclude_history=False, candidates="line"))):
        six, top, tgt = h.evaluate_catalog(m, batches, cat, neg, k=k, return_lists=True, **kw_old)
        got = h.evaluate_catalog_users(m, st, cat, k=k, return_lists=True, **kw_new)
        assert got[0] == six and torch.equal(got[1], top) and torch.equal(got[2], tgt), kw_new
        assert h.evaluate_catalog_users(m, st, cat, k=k, lines_per_call=7, **kw_new) == six
    assert top.shape[0] == st.n_lines and cat.builds == 1
