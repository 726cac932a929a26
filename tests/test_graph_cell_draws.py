"""TemporalGraph.from_log(draws="cell"): the per-cell, counter-based draw rule (host build) against its plain-Python
restatement (graph_cell_cases.py) and against the documents the reference's GraphStore wrote (g5).  Exact integers."""
from collections import Counter

import numpy as np
import pytest

import graph_cell_cases as cc
from score_amd.graph import TemporalGraph


def build(c, **kw):
    uid, iid, t, U, I, S, m1, m2, seed = c
    ur, ir = cc.rows(U, I)
    return TemporalGraph.from_log(uid, iid, t, U, I, S, ur, ir, max_1hop=m1, max_2hop=m2, seed=seed, **kw)


@pytest.mark.parametrize("name", cc.SMALL_CASES + cc.BIG_CASES[-1:])
def test_cell_draws_equal_the_restatement(name):
    c = cc.case(name)
    sides, stats = cc.restate(*c)
    cc.assert_graph_equals_restatement(build(c, draws="cell"), sides, *c[3:6])
    m1, m2 = c[6], c[7]
    if name == "edges":                # the log really holds what it is there for
        assert {m1, m1 + 1} <= stats["len1"] and {m2, m2 + 1} <= stats["cand"] and {1, 2} <= stats["d"]
        assert stats["permuted_cut"] > 0
    if name == "tile_seam":
        assert {8192, 8193} <= stats["len1"]
    if name == "rank_4096":
        assert 4096 in stats["cand"]
    if name == "no_over_long":
        assert stats["shuffled"] == 0 and max(stats["cand"]) > m2
    if name == "sink":
        n_in = sum(len(l) for l in sides["user"][0].values())
        assert 0 < n_in < len(c[0]) - 40


def test_key_function_is_the_rule():
    from score_amd.graph import _cell_keys
    cs = np.array([0, 1, 5, 2 ** 31 - 2, 123456789], dtype=np.int64)
    js = np.array([0, 7, 8192, 4095, 99999], dtype=np.int64)
    for seed in (0, 11, 2 ** 64 - 1):
        for tag in range(4):
            got = _cell_keys(seed, tag, cs, js)
            assert got.dtype == np.uint32
            assert got.tolist() == [cc.key(seed, tag, int(a), int(b)) for a, b in zip(cs, js)]


def _docs(z, tag, side, field):
    a = z["%s/%s_%s" % (tag, side, field)]
    n = z["%s/%s_%s_len" % (tag, side, "2hop" if field == "degrees" else field)]
    return [[a[e, t, :n[e, t]].tolist() for t in range(a.shape[1])] for e in range(a.shape[0])]


def test_g5_sparse_equals_reference_documents_and_the_stream_build():
    # no cap is hit: no draw is taken, so both rules give the reference's documents
    z = np.load(cc.GOLDEN + "/g5_graph_store.npz")
    c = cc.case("g5_sparse")
    U, I, S = c[3:6]
    g, s = build(c, draws="cell"), build(c, draws="stream")
    for side, n in (("user", U), ("item", I)):
        one, two, deg = (_docs(z, "sparse", side, f) for f in ("1hop", "2hop", "degrees"))
        gd = g.user_degrees if side == "user" else g.item_degrees
        off2 = (g.user_csr if side == "user" else g.item_csr)["off2"]
        for e in range(n):
            for t in range(S):
                assert g.cell(side, 1, e, t).tolist() == one[e][t], (side, e, t)
                assert g.cell(side, 2, e, t).tolist() == two[e][t], (side, e, t)
                assert gd[off2[e * S + t]:off2[e * S + t + 1]].tolist() == deg[e][t]
    for a, b in ((g.user_csr, s.user_csr), (g.item_csr, s.item_csr)):
        for k in ("off1", "nbr1", "off2", "nbr2"):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert np.array_equal(g.user_degrees, s.user_degrees) and np.array_equal(g.item_degrees, s.item_degrees)


@pytest.mark.parametrize("seed", [3, 4])
def test_g5_dense_vs_reference_documents(seed):
    # every cap is hit (max_1hop 3, max_2hop 8): what test_graph_store.test_dense_log_vs_reference_documents asserts of the
    # stream build holds of the cell build -- cells the reference fills without a random choice are equal, the others have
    # the reference's size and draw from the same support
    z = np.load(cc.GOLDEN + "/g5_graph_store.npz")
    c = cc.g5_case("dense", seed)
    U, I, S, m1, m2 = c[3:8]
    g = build(c, draws="cell")
    ref1 = {s: _docs(z, "dense", s, "1hop") for s in ("user", "item")}
    ref2 = {s: _docs(z, "dense", s, "2hop") for s in ("user", "item")}
    refd = {s: _docs(z, "dense", s, "degrees") for s in ("user", "item")}
    raw = {"user": [[[] for _ in range(S)] for _ in range(U)], "item": [[[] for _ in range(S)] for _ in range(I)]}
    for u, i, t in z["dense/log"].tolist():
        raw["user"][u - 1][t].append(i)
        raw["item"][i - U - 1][t].append(u)
    exact = sampled = 0
    for side, other, n, obase in (("item", "user", I, 1), ("user", "item", U, U + 1)):
        gd = g.user_degrees if side == "user" else g.item_degrees
        off2 = (g.user_csr if side == "user" else g.item_csr)["off2"]
        for e in range(n):
            for t in range(S):
                mine1, r1 = g.cell(side, 1, e, t).tolist(), ref1[side][e][t]
                assert sorted(mine1) == sorted(r1) == sorted(raw[side][e][t])
                if len(r1) <= m1:
                    assert mine1 == r1 == raw[side][e][t]
                mine2, r2 = g.cell(side, 2, e, t).tolist(), ref2[side][e][t]
                nbs = raw[side][e][t]
                lists = [raw[other][x - obase][t] for x in nbs]
                cut_random = side == "user" and any(len(l) > m1 for l in lists)
                if len(nbs) <= m1 and not cut_random:
                    full = [y for l in lists if len(l) > 1 for y in l[:m1]]
                    fdeg = [len(l) for l in lists if len(l) > 1 for _ in l[:m1]]
                    if len(full) <= m2:
                        assert mine2 == r2 == full, (side, e, t)
                        assert gd[off2[e * S + t]:off2[e * S + t + 1]].tolist() == refd[side][e][t] == fdeg
                        exact += 1
                        continue
                    assert len(mine2) == len(r2) == m2
                    assert not (Counter(mine2) - Counter(full)) and not (Counter(r2) - Counter(full))
                    sampled += 1
                    continue
                support = Counter(y for l in lists if len(l) > 1 for y in l)
                assert len(mine2) <= m2 and len(r2) <= m2
                assert not (Counter(mine2) - support) and not (Counter(r2) - support)
                sampled += 1
    assert exact >= 10 and sampled > 20         # a property of the fixture, not of the build


def test_equal_keys_keep_position_order(monkeypatch):
    # the tie rule: with every key equal, "the random order" is the position order -- a shuffled cell keeps log order, a
    # down-sample keeps the first max_2hop candidates
    import score_amd.graph as gm
    monkeypatch.setattr(gm, "_cell_keys", lambda seed, tag, c, j: np.full(np.shape(c), 7, dtype=np.uint32))
    for name in ("edges", "g5_dense"):
        c = cc.case(name)
        sides, stats = cc.restate(*c, key=lambda seed, tag, cell, j: 7)
        assert stats["shuffled"] > 0 and max(stats["cand"]) > c[7]
        g = build(c, draws="cell")
        cc.assert_graph_equals_restatement(g, sides, *c[3:6])
        uid, iid, t, U, I, S, m1, m2, _ = c
        for e in range(U):
            for s in range(S):
                assert g.cell("user", 1, e, s).tolist() == np.asarray(iid)[(np.asarray(uid) == e + 1) & (np.asarray(t) == s)].tolist()


def test_build_and_draws_errors(monkeypatch):
    import torch
    c = cc.case("edges")
    with pytest.raises(ValueError):
        build(c, build="device", draws="stream")
    with pytest.raises(ValueError):
        build(c, build="device")                       # (the default draws="stream")
    with pytest.raises(ValueError):
        build(c, draws="pcg")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError):
        build(c, build="device", draws="cell")


def test_tmall_pipeline_passes_build_and_draws_through():
    from score_amd import dataprep as dp
    raw = np.load(cc.GOLDEN + "/tmall_sample_log.npz")["log"]
    a, r, _ = dp.tmall_pipeline(raw, seed=11, draws="cell")
    b = TemporalGraph.from_log(r["uid"], r["iid"], r["t_idx"], r["n_users"], r["n_items"], dp.TMALL["graph_time_slice_num"],
                               r["user_rows"], r["item_rows"], max_1hop=dp.TMALL["max_1hop"], max_2hop=dp.TMALL["max_2hop"],
                               seed=11, draws="cell")
    for k in ("off1", "nbr1", "off2", "nbr2"):
        assert np.array_equal(a.user_csr[k], b.user_csr[k]) and np.array_equal(a.item_csr[k], b.item_csr[k])
    with pytest.raises(ValueError):
        dp.tmall_pipeline(raw, seed=11, build="device", draws="stream")
