"""CPU twin of tests/test_gpu_scatter_edges.py: the case tables of tests/scatter_cases.py reach what they claim, their restatement
of the launch geometry is the library's (score_pull_geometry, host only), the references stay inside their own bounds, and the
judges reject what they are there to reject.  No GPU."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from score_amd import _lib
import scatter_cases as sc


def _geometry(n, D):
    v = [C.c_int32(-5) for _ in range(4)]
    rc = _lib.load().score_pull_geometry(n, D, *[C.byref(x) for x in v])
    return rc, tuple(x.value for x in v)


@pytest.mark.parametrize("name", list(sc.SCATTER_ROWS))
def test_row_reaches_what_it_claims(name):
    r = sc.SCATTER_ROWS[name]
    inp = sc.scatter_inputs(r)
    assert np.array_equal(inp.keys, sc.sorted_keys(r)) and inp.keys.max() < inp.n_out
    st = sc.structure(inp.keys, r.D)
    sc.check_claim(r, st)
    # the restatement's geometry is the launcher's
    rc, got = _geometry(st.n, r.D)
    assert rc == 0 and got == (st.window, st.lanes, st.gpb, sc.LONG_CHAIN) == sc.geometry(st.n, r.D)
    # every partial sum of the exact fill is an integer float32 holds: no association can change a bit
    assert st.n * 4 < 1 << 24


def test_rows_together_reach_every_seam():
    sts = {n: sc.structure(sc.sorted_keys(r), r.D) for n, r in sc.SCATTER_ROWS.items()}
    assert {s.window for s in sts.values()} == set(sc.WINDOWS)
    assert {(s.lanes, sc.SCATTER_ROWS[n].D // 4) for n, s in sts.items()} >= {(1, 1), (2, 2), (4, 3), (4, 4), (8, 5), (16, 16),
                                                                             (32, 32), (64, 64)}
    Ls = set(int(l) for s in sts.values() for l in np.unique(s.L))
    assert {0, 1, 2, 15, 16, 17} <= Ls                                          # both sides of LONG_CHAIN
    chunks = {c for s in sts.values() for c in s.chunks}
    assert {1, 2, 5, 8, 9, 16, 17} <= chunks                                    # both sides of 8 and of 16
    assert any(s.full_trip for s in sts.values()) and any(s.n_long and not s.full_trip for s in sts.values())
    # a full trip with a tail behind it, and one without
    tails = {int(t) for s in sts.values() for c in s.longs for t in c.tails[c.trips > 0]}
    assert 0 in tails and tails - {0}
    assert any((c.counts == 0).any() for s in sts.values() for c in s.longs)    # idle groups
    assert max(s.max_per_wg for s in sts.values()) >= 4
    assert any(s.partial_end and s.n_long for s in sts.values())
    gallops = set(int(g) for s in sts.values() if s.window == 8 for g in s.gallop[s.L > 0])
    assert {1, 2, 3, 4, 7, 8, 9, 15, 16, 17} <= gallops
    # runs that end exactly at n and one short of it
    assert any(s.ends[-1] == s.n and s.L[-1] > 0 for s in sts.values())
    assert any(len(s.ends) > 1 and s.ends[-2] == s.n - 1 and s.L[-2] > 0 for s in sts.values())
    # row 0 as a one-slot run, a short and a long chain
    zero = {"one slot" if s.ends[0] == 1 else int(s.cls[0]) for n, s in sts.items() if n.startswith("row0_")}
    assert all(s.ids[0] == 0 for n, s in sts.items() if n.startswith("row0_")) and zero == {"one slot", sc.SHORT, sc.LONG}


@pytest.mark.parametrize("n,D", [(0, 4), (1, 4), ((1 << 18) - 1, 16), (1 << 18, 16), ((1 << 19) - 1, 64), (1 << 19, 64),
                                 ((1 << 20) - 1, 128), (1 << 20, 256), (1 << 28, 12), (5, 20), (5, 252)])
def test_geometry_query_at_the_window_thresholds(n, D):
    rc, got = _geometry(n, D)
    assert rc == 0 and got == sc.geometry(n, D)
    assert got[1] * got[2] == 256 and got[1] >= D // 4 > got[1] // 2


def test_geometry_query_refusals():
    assert sc.geometry(8, 260) is None
    for D in (260, 512, 1 << 20):
        rc, got = _geometry(8, D)
        assert rc == sc.E_SHAPE and got == (-5,) * 4                            # nothing written
    for n, D in ((8, 6), (8, 0), (8, -4), (-1, 16)):
        rc, got = _geometry(n, D)
        assert rc == sc.E_BADARG and got == (-5,) * 4
    v = C.c_int32(0)
    lib = _lib.load()
    assert lib.score_pull_geometry(8, 16, None, C.byref(v), C.byref(v), C.byref(v)) == sc.E_BADARG
    assert lib.score_pull_geometry(8, 16, C.byref(v), C.byref(v), C.byref(v), None) == sc.E_BADARG


_WORST = [0.0, 0.0]


@pytest.mark.parametrize("name", list(sc.SCATTER_ROWS))
def test_reference_alone_meets_both_judges(name):
    """the int64 sum through the exact judge, a plain float32 left-to-right sum through the rounding bound"""
    r = sc.SCATTER_ROWS[name]
    inp = sc.scatter_inputs(r)
    flags = np.where(np.isin(np.arange(inp.n_out), inp.keys), 2, inp.flags0).astype(np.uint8)
    src = sc.scatter_fill(r, "exact")
    assert np.abs(src).max() <= 4 and np.array_equal(src, np.round(src))
    out = sc.plain_float32_sums(r, src)
    assert sc.scatter_judge(r, "exact", src, out, flags).all == 0.0
    if not r.big:
        assert np.array_equal(sc.simulate(r, src).view(np.uint32), out.view(np.uint32))       # the window model agrees
    src = sc.scatter_fill(r, "rounding")
    worst = sc.scatter_judge(r, "rounding", src, sc.plain_float32_sums(r, src), None)
    _WORST[:] = [max(a, b) for a, b in zip(_WORST, worst)]
    print("%s: a plain float32 sum at %.6f of the bound, %.3f in runs of three and more (worst so far %.6f, %.3f)"
          % ((name,) + tuple(worst) + tuple(_WORST)))
    assert worst.all <= 1.0


# the row each perturbation is applied to
_PERTURBED = {"pfirst_left_out": "chain_L2_o3_mid", "pfirst_twice": "chain_L16_o0_last", "total_to_next_row": "gallop_9",
              "last_slot_ignored": "gallop_11_to_n", "row0_dropped": "row0_long_chain", "last_group_left_out": "split_d256_L33"}


@pytest.mark.parametrize("perturb", sc.PERTURBATIONS)
def test_judge_rejects_perturbed_results_of_the_exact_fill(perturb):
    hit = 0
    for name in {_PERTURBED[perturb], "width_d12", "split_d16_L513"}:
        r = sc.SCATTER_ROWS[name]
        inp = sc.scatter_inputs(r)
        if perturb == "row0_dropped" and inp.keys[0] != 0:
            continue
        src = sc.scatter_fill(r, "exact")
        flags = np.where(np.isin(np.arange(inp.n_out), inp.keys), 2, inp.flags0).astype(np.uint8)
        assert sc.scatter_judge(r, "exact", src, sc.simulate(r, src), flags).all == 0.0
        bad = sc.simulate(r, src, perturb)
        with pytest.raises(AssertionError):
            sc.scatter_judge(r, "exact", src, bad, flags)
        hit += 1
    assert hit >= 1


def test_judge_rejects_a_touched_bystander_and_a_wrong_flag():
    r = sc.SCATTER_ROWS["n_out_1025_highest_unnamed"]
    inp = sc.scatter_inputs(r)
    src = sc.scatter_fill(r, "exact")
    flags = np.where(np.isin(np.arange(inp.n_out), inp.keys), 2, inp.flags0).astype(np.uint8)
    good = sc.simulate(r, src)
    bad = good.copy()
    bad[1024, 3] += 1.0
    with pytest.raises(AssertionError):
        sc.scatter_judge(r, "exact", src, bad, flags)
    for row, v in ((1024, 2), (3, 0), (1000, 1)):
        f = flags.copy()
        f[row] = v
        assert f[row] != flags[row]
        with pytest.raises(AssertionError):
            sc.scatter_judge(r, "exact", src, good, f)
    # the rounding judge: one ulp is inside the bound of a run of nine, two of a run's sum outside that of a run of one
    src = sc.scatter_fill(r, "rounding")
    out = sc.plain_float32_sums(r, src)
    sc.scatter_judge(r, "rounding", src, out, flags)
    bad = out.copy()
    bad[0, 0] = np.nextafter(bad[0, 0], np.float32(np.inf))                     # row 0: a one-slot run, bound 0
    with pytest.raises(AssertionError):
        sc.scatter_judge(r, "rounding", src, bad, flags)


# ---------------------------------------------------------------------------------------------- accumulate, plan, AUC
@pytest.mark.parametrize("name", list(sc.ACC_ROWS))
def test_accumulate_reference_and_judge(name):
    r = sc.ACC_ROWS[name]
    src, out0, flags0 = sc.acc_inputs(r)
    want, wf = sc.acc_reference(r, src, out0, flags0)
    sc.acc_judge(r, want, wf, want.copy(), wf.copy())
    named = np.zeros(r.n_out, bool)
    for l in r.lists:
        named[l] = True
    assert np.array_equal(wf, np.where(named, 2, flags0)) and np.isfinite(want[named]).all()
    assert np.array_equal(want[~named].view(np.uint32), out0[~named].view(np.uint32))
    if named.any():
        # one element an ulp off, one state byte
        bad = want.copy()
        i = int(np.flatnonzero(named)[-1])
        bad[i, -1] = np.nextafter(bad[i, -1], np.float32(np.inf))
        with pytest.raises(AssertionError):
            sc.acc_judge(r, want, wf, bad, wf)
        f = wf.copy()
        f[i] = 1
        with pytest.raises(AssertionError):
            sc.acc_judge(r, want, wf, want, f)


def test_accumulate_rows_cover_the_issue():
    rows = sc.ACC_ROWS.values()
    assert {len(r.lists) for r in rows} >= {1, 2, 8, 64} and {r.D for r in rows} >= {4, 12, 20, 256}
    r = sc.ACC_ROWS["eight_sources_named_rows_d12"]
    count = np.zeros(r.n_out, int)
    for l in r.lists:
        count[l] += 1
    assert count[7] == 8 and count[33] == 1 and 33 in r.lists[-1] and count[2] == 2 and 2 in r.lists[0] and 2 in r.lists[-1]
    assert 2 % 3 == 2                                                         # row 2 enters in state 2: added to
    # with what is there added LAST the sum of a row named twice is other bits: the judge tells the two associations apart
    src, out0, flags0 = sc.acc_inputs(r)
    want, wf = sc.acc_reference(r, src, out0, flags0)
    other = out0[2] + (src[0] + src[len(np.concatenate(r.lists[:-1]))])
    assert not np.array_equal(other, want[2])


@pytest.mark.parametrize("name", list(sc.PLAN_ROWS))
def test_plan_reference_and_judge(name):
    c = sc.PLAN_ROWS[name]
    t = sc.plan_inputs(c)
    want = sc.plan_reference(c, t)
    sc.plan_judge(c, t, want)
    assert want.unique_rows[0] == 0 and want.offsets[0] == 0 and want.offsets[-1] == want.U <= sc.plan_occurrences(c)
    if c.ids == "bad_all":
        assert want.U == 1 and want.id_status == 63
    if c.ids == "mixed":
        assert want.id_status == (1 << 1 | 1 << 4)
    if c.ids == "distinct":
        assert want.U == sc.plan_occurrences(c)
    if c.ids == "equal":
        assert want.U == 2
    # one flipped element of each product
    if want.U > 1:
        u = want.unique_rows.copy()
        u[-1] += 1
        with pytest.raises(AssertionError):
            sc.plan_judge(c, t, want._replace(unique_rows=u))
    o = want.offsets.copy()
    o[-1] += 1
    with pytest.raises(AssertionError):
        sc.plan_judge(c, t, want._replace(offsets=o))
    with pytest.raises(AssertionError):
        sc.plan_judge(c, t, want._replace(id_status=want.id_status ^ 4))
    for seg in (0, 5):
        rm = [x.copy() for x in want.remap]
        rm[seg].reshape(-1)[0] = (rm[seg].reshape(-1)[0] + 1) % max(want.U, 2)
        with pytest.raises(AssertionError):
            sc.plan_judge(c, t, want._replace(remap=rm))
    if sc.plan_active(c) < c.T:
        rm = [x.copy() for x in want.remap]
        rm[2][0, -1, 0, 0] = 0                                                 # a masked slice written
        with pytest.raises(AssertionError):
            sc.plan_judge(c, t, want._replace(remap=rm))


def test_plan_rows_cover_the_issue():
    rows = list(sc.PLAN_ROWS.values())
    assert {c.G for c in rows} == {1, 2, 3, 8, 64} and {c.N for c in rows} >= {7, 64, 1024, 1025, 3001}
    assert any(c.G == 8 and c.N == 7 for c in rows)
    assert {(c.B, c.T, c.K) for c in rows} >= {(1, 1, 1), (3, 2, 2)}
    assert any(sc.plan_occurrences(c) % 256 == 1 for c in rows)
    assert {c.Fu for c in rows} == {1, 8} == {c.Fi for c in rows}
    assert {c.ids for c in rows} == {"random", "equal", "distinct", "bad_all", "mixed"}
    assert any(c.active == 1 for c in rows) and any(c.active == c.T - 1 > 1 for c in rows)


@pytest.mark.parametrize("name", list(sc.AUC_ROWS))
def test_auc_reference_and_judge(name):
    r = sc.AUC_ROWS[name]
    p, y = sc.auc_inputs(r)
    assert len(p) == r.n and p.dtype == np.float32 and p.min() >= 0.0 and p.max() <= 1.0
    auc, ll = sc.auc_reference(p, y)
    sc.auc_judge(r, auc, ll, float("nan") if auc is None else float(auc), ll)
    with pytest.raises(AssertionError):
        sc.auc_judge(r, auc, ll, float("nan") if auc is None else float(auc), ll + 3e-12)
    with pytest.raises(AssertionError):
        sc.auc_judge(r, auc, ll, 0.5 if auc is None else float(auc) + 3e-12, ll)
    if r.kind == "all_equal":
        assert auc == Fraction(1, 2)
    if r.kind in ("pos_only", "neg_only") or r.n == 1:
        assert auc is None
    if r.kind == "tie_60000_70000":
        ps = np.sort(p)
        assert ps[59999] < ps[60000] == ps[70000] < ps[70001] and len(np.unique(ps)) == r.n - 10000
    if r.kind == "saturated":
        assert {(0.0, 0), (0.0, 1), (1.0, 0), (1.0, 1)} <= set(zip(p.tolist(), y.tolist()))
        assert ll > 36.0 * ((p == 1.0) & (y == 0)).sum() / r.n                   # the clipped terms are -log(2^-52) = 36.04
    if r.kind == "labels":
        assert set(np.unique(y)) == {-1, 0, 2, 7}
    if r.n <= 257 and auc is not None:
        # pair counting, the definition: P(score of a positive > score of a negative) + P(equal) / 2
        pos, neg = p[y != 0].astype(np.float64), p[y == 0].astype(np.float64)
        wins = int((pos[:, None] > neg[None, :]).sum()) * 2 + int((pos[:, None] == neg[None, :]).sum())
        assert auc == Fraction(wins, 2 * len(pos) * len(neg))
