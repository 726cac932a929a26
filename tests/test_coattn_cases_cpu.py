"""CPU twin of tests/test_gpu_coattn_edges.py: the case table of tests/coattn_cases.py without a GPU.  Every row's forms come
from the mirror and agree with the forms stated for it; the rows reach every instance of coattn_bwd_kernel_t, coattn_fwd_kernel
and coattn_fwd_kernel_units the launch rules can reach (the others are printed); the unit-count and active / inactive conditions
hold; a float32 restatement stays within a quarter of the bounds; the float64 backward restatement equals torch autograd of the
oracle; the judge rejects six perturbed results.  Run with -s for the coverage list and every row's float32 ratios."""
import itertools

import numpy as np
import pytest

import coattn_cases as cc

SINGLE = [n for n, r in cc.ROWS.items() if r.mode == 0 and not r.planted]
# the compiled instances (csrc/embed.hip): 40 of coattn_bwd_kernel_t<KMAX, SPL, ATOMIC, NM>, 10 + 3 of the forward
BWD_COMPILED = {(k, s, a, 0) for a in (0, 1) for k, s in ((4, 1), (10, 1), (20, 1), (32, 1), (4, 2), (10, 2), (20, 2), (32, 2), (10, 4), (20, 4))} \
    | {(k, s, a, nm) for a in (0, 1) for s in (1, 2) for k, nm in ((4, 1), (4, 2), (10, 1), (10, 2), (10, 4))}
FWD_COMPILED = {(0, k, s) for k, s in ((4, 1), (10, 1), (20, 1), (32, 1), (4, 2), (10, 2), (20, 2), (32, 2), (10, 4), (20, 4))} \
    | {(1, 4, 1), (1, 4, 2), (1, 10, 1)}
# what no legal shape reaches, pinned (test_rows_reach_every_reachable_instance prints and asserts it).  ATOMIC = false is the
# model's pull-form pass alone (score_coattn_bwd always adds the rows itself), whose plan path takes Fu, Fi <= 8: at two
# slots per lane that is a 64-lane group with at least eight neighbours per id register and 3 K <= 30 scalars in one, so
# the lists need one register at K <= 4 and at most two at K <= 10 -- never none, never four, and two only from K = 9 on;
# and RCA (mode 1, always NM 0) launches no backward in the pull form.
BWD_UNREACHED = {(4, 2, 0, 0), (10, 2, 0, 0), (4, 2, 0, 2), (10, 2, 0, 4)}


def _key(b):
    return (b.kmax, b.spl, b.atomic, b.nm)


def test_forms_are_the_mirrors_and_the_stated_ones():
    assert len(cc.STATED) == 48
    for (D, F, K), ((spl, kmax, nm), fwd) in cc.STATED.items():
        r = cc.ROWS["d%d_f%d_k%d" % (D, F, K)]
        assert cc.check(True, cc.N_ROWS, D, F, K, 1, 1) == 0
        assert r.bwd == cc.bwd_form(D, (F,), K, 0) == cc.Bwd(kmax, spl, nm, 1, 0), (D, F, K, r.bwd)      # the ABI wrapper: ATOMIC
        assert r.fwd == cc.fwd_form(D, (F,), K, 0) and cc.fwd_name(r.fwd).startswith(fwd), (D, F, K, cc.fwd_name(r.fwd), fwd)
        assert cc.unpack_bwd(cc.pack_bwd(r.bwd)) == r.bwd and cc.unpack_fwd(cc.pack_fwd(r.fwd)) == r.fwd
    for r in cc.ROWS.values():
        assert r.bwd == cc.bwd_form(r.D, (r.F,), r.K, r.mode)
        if r.mode == 1:                                    # pure summation: the one-unit kernels, every lane its own ids
            assert r.bwd.nm == 0 and r.fwd.units == 0 and r.bwd.mode == 1
    assert {(cc.ROWS["rca_d%d_f%d_k%d" % s].bwd.spl, cc.ROWS["rca_d%d_f%d_k%d" % s].bwd.kmax) for s in cc.MODE1_SHAPES} \
        == {(b[0], b[1]) for b, _ in cc.STATED.values()}
    # geometry facts the rows are named for
    assert cc.geom(4, 1)[0] == 1 and cc.geom(4, 2)[0] == 2 and cc.geom(4, 65) == (64, 2, 65) and cc.ksh(64, 65) == -1
    assert cc.geom(64, 9) == (64, 3, 144) and cc.launch_spl(64, (9,)) == 4                          # spl == 3 -> 4
    assert cc.meta_regs(*[cc.geom(16, 3)[0], 3, 10]) == 3 and cc.bwd_form(16, (3,), 10, 0).nm == 4   # need 3 -> NM 4
    assert cc.meta_regs(64, 64, 3) == 3 and cc.bwd_form(4, (64,), 3, 0).nm == 0                     # K <= 4 with need > 2 -> NM 0


def test_refusals_of_the_mirror():
    for name, (D, F, K, pad, null, short, code) in cc.REFUSALS.items():
        got = cc.check(null != "table", cc.N_ROWS, D, F, K, 2, 3)
        if name in ("d6", "d260", "slots257", "k33", "k21_slots129", "null_table"):
            assert got == code, name
        else:                                              # refused by the wrapper / the launcher behind coattn_check
            assert got == 0, name


def test_model_rows_promise_what_the_issue_names():
    f = lambda n, m: cc.model_forms(n, m)[1]
    assert f("spl1_in_spl2", 0) == cc.Bwd(10, 2, 1, 0, 0) and cc.geom(128, 1)[1] == 1 and cc.geom(128, 4)[1] == 2
    assert f("spl1_in_spl4", 1) == cc.Bwd(10, 4, 0, 1, 0) and cc.geom(256, 1)[1] == 1 and cc.geom(256, 4)[1] == 4
    assert f("spl4_k20", 0) == cc.Bwd(20, 4, 0, 0, 0) and cc.geom(256, 3)[2] == 192 and cc.geom(256, 4)[2] == 256
    assert f("spl2_k4", 0) == cc.Bwd(4, 2, 1, 0, 0)
    assert f("spl2_k32", 0) == cc.Bwd(32, 2, 0, 0, 0) and f("spl1_k32", 0) == cc.Bwd(32, 1, 0, 0, 0)
    # (32, 5, 8, 8): both calls one slot per lane and one register per list (eight neighbours per id register): NM 1
    assert f("need_of_two_calls", 0) == cc.Bwd(10, 1, 1, 0, 0) and cc.MODEL_ROWS["need_of_two_calls"][6] < cc.MODEL_ROWS["need_of_two_calls"][5]
    assert f("rca", 1) == cc.Bwd(10, 1, 0, 1, 1)
    assert f("spl2_nm2", 0) == cc.Bwd(10, 2, 2, 0, 0) and cc.meta_regs(64, 3, 10) == 1 and cc.meta_regs(64, 5, 10) == 2
    for name, row in cc.MODEL_ROWS.items():
        assert row[1] <= 8 and row[2] <= 8 and 12 <= row[4] * row[6] <= 48, name         # a few dozen units


def test_rows_reach_every_reachable_instance():
    # what score_coattn_bwd / score_coattn_fwd reach over every shape coattn_check accepts
    abi_b, abi_f = set(), set()
    for D in range(4, 257, 4):
        for F in range(1, 256 // (D // 4) + 1):
            for K in range(1, 33):
                if cc.check(True, 1, D, F, K, 1, 1) != 0:
                    continue
                for mode in (0, 1):
                    abi_b.add(_key(cc.bwd_form(D, (F,), K, mode)))
                    f = cc.fwd_form(D, (F,), K, mode)
                    abi_f.add((f.units, f.kmax, f.reg))
    # what the model's two-call launches reach (Fu, Fi <= 8; RCA's pull form launches no backward)
    mod_b, mod_f = set(), set()
    for D in range(4, 257, 4):
        for Fu, Fi in itertools.combinations_with_replacement(range(1, 9), 2):
            for K in range(1, 33):
                if cc.check(True, 1, D, Fu, K, 1, 1) or cc.check(True, 1, D, Fi, K, 1, 1):
                    continue
                for mode, atomic in ((0, 0), (0, 1), (1, 1)):
                    mod_b.add(_key(cc.bwd_form(D, (Fi, Fu), K, mode, atomic)))
                    f = cc.fwd_form(D, (Fi, Fu), K, mode)
                    mod_f.add((f.units, f.kmax, f.reg))
    reach_b, reach_f = abi_b | mod_b, abi_f | mod_f
    assert reach_b <= BWD_COMPILED and reach_f <= FWD_COMPILED and len(BWD_COMPILED) == 40 and len(FWD_COMPILED) == 13
    rows_b = {_key(r.bwd) for r in cc.ROWS.values()}
    rows_f = {(r.fwd.units, r.fwd.kmax, r.fwd.reg) for r in cc.ROWS.values() if r.fwd is not None}
    for name in cc.MODEL_ROWS:
        for sm in (0, 1):
            if cc.MODEL_ROWS[name][7] == "RCA" and sm == 0:
                continue
            f, b = cc.model_forms(name, sm)
            rows_b.add(_key(b))
            rows_f.add((f.units, f.kmax, f.reg))
    unreached = sorted(BWD_COMPILED - reach_b)
    print("backward instances (KMAX, SPL, ATOMIC, NM) no legal shape reaches: %r" % (unreached,))
    print("forward instances no legal shape reaches: %r" % (sorted(FWD_COMPILED - reach_f),))
    print("the rows reach %d of 40 backward and %d of 13 forward instances" % (len(rows_b), len(rows_f)))
    assert set(unreached) == BWD_UNREACHED and FWD_COMPILED == reach_f
    assert rows_b == reach_b, sorted(reach_b - rows_b)
    assert rows_f == reach_f, sorted(reach_f - rows_f)


@pytest.mark.parametrize("name", list(cc.ROWS))
def test_unit_counts_and_inputs(name):
    r = cc.ROWS[name]
    GS = cc.geom(r.D, r.F)[0]
    upw = 64 // GS
    assert cc.dims(r, "one") == (1, 1)
    B, T = cc.dims(r, "big")
    n = B * T
    assert T == 3 and 8 * upw < n <= 520 and n % (4 * upw) and (upw == 1 or n % upw), (n, upw)
    for count in cc.COUNTS:
        inp = cc.inputs(name, count)
        assert inp.table.shape == (cc.N_ROWS, r.D) and not inp.table[0].any()
        assert inp.ld1 == r.F * r.D + 4 and inp.ldi == 2 * r.K + 1
        if count == "one":
            continue
        a, b = inp.idx1.reshape(n, r.K, r.F), inp.idx2.reshape(n, r.K, r.F)
        assert (a == 0).any() and (b == 0).any()
        assert ((a < 0) | (a >= cc.N_ROWS)).sum() >= 2 and ((b < 0) | (b >= cc.N_ROWS)).sum() >= 2
        # one id in both lists of a unit, an id repeated inside a unit (but for the few units whose ids were put outside the table)
        assert (b[::2, 0] == a[::2, r.K - 1]).all(1).mean() >= 0.5
        assert r.K == 1 or (a[1::3, r.K - 1] == a[1::3, 0]).all(1).mean() >= 0.5
        if r.mode == 0 and not r.planted:
            ref = cc.forward_ref(inp, r.K, r.F, 0)
            assert np.abs(ref.z).min() >= cc.MARGIN
            act = float((ref.z > 0).mean())
            assert 0.25 <= act <= 0.75, act
            assert np.array_equal(inp.rsave > 0, ref.r > 0)                              # rounding to float32 keeps the decisions
        if r.planted:
            rs = inp.rsave
            assert not rs[0].any() and (rs[1] > 0).all() and (rs[2] == rs[2, 0]).all() and rs[2, 0] > 0
            assert rs[3].max() == 90 and np.sort(rs[3])[-2] < 1.2 and n >= 9


@pytest.mark.parametrize("name", SINGLE + [n for n, r in cc.ROWS.items() if r.planted])
def test_float32_restatement_within_a_quarter_of_the_bounds(name):
    r = cc.ROWS[name]
    Dx = r.F * r.D
    worst = {}
    for count in cc.COUNTS:
        inp = cc.inputs(name, count)
        o1, o2, info, rs, gt, dW, dzs = cc.restate_f32(inp, r.K, r.F, r.D)
        bref = cc.backward_ref(inp, r.K, r.F, 0)
        e = {"gtable": cc._share_b(gt, bref.gtable), "dW": cc._share_b(dW[Dx:], bref.dW[Dx:]), "dzsum": cc._share_b(dzs, bref.dzsum)}
        if not r.planted:
            fref = cc.forward_ref(inp, r.K, r.F, 0)
            e.update(out1=cc._share(o1, fref.out1), out2=cc._share(o2, fref.out2), info=cc._share(info, fref.info), rsave=cc._share(rs, fref.r))
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("%s: float32 restatement as shares of the bounds: %s" % (name, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) <= 0.25, worst


@pytest.mark.parametrize("name", SINGLE)
def test_backward_restatement_equals_autograd(name):
    r = cc.ROWS[name]
    Dx = r.F * r.D
    for count in cc.COUNTS:
        inp = cc.inputs(name, count)
        fref = cc.forward_ref(inp, r.K, r.F, 0)
        bref = cc.backward_ref(inp, r.K, r.F, 0, rsave=fref.r)                           # the float64 scores: autograd's own decisions
        gt, dW, dtg = cc.autograd_ref(inp, r.K, r.F)
        scale = lambda a: max(1.0, float(np.abs(a).max()))
        assert np.abs(bref.gtable - gt).max() <= 1e-10 * scale(gt)
        assert np.abs(bref.dW[Dx:] - dW[Dx:]).max() <= 1e-10 * scale(dW)
        want = bref.dzsum[:, None] * inp.W[:Dx].astype(np.float64)[None, :]
        assert np.abs(want - dtg).max() <= 1e-10 * scale(dtg)


@pytest.mark.parametrize("name", [n for n, r in cc.ROWS.items() if r.mode == 1])
def test_mode1_sums_are_exact_in_float32(name):
    r = cc.ROWS[name]
    for count in cc.COUNTS:
        inp = cc.inputs(name, count)
        f, b = cc.forward_ref(inp, r.K, r.F, 1), cc.backward_ref(inp, r.K, r.F, 1)
        for a in (f.out1, f.out2, b.gtable):
            assert np.array_equal(a, np.rint(a)) and np.abs(a).max() < 2 ** 20           # every partial sum is an integer float32 holds


def _perfect(name, count="big"):
    """(inputs, references, the references' own values in the buffers the kernels would leave)"""
    r = cc.ROWS[name]
    Dx, inp = r.F * r.D, cc.inputs(name, count)
    n = inp.B * inp.T
    fref, bref = cc.forward_ref(inp, r.K, r.F, 0), cc.backward_ref(inp, r.K, r.F, 0)
    gf = cc.fwd_buffers(inp, r.K, Dx)
    gf.out1[:n, :Dx], gf.out2[:n, :Dx], gf.rsave[:n] = fref.out1, fref.out2, fref.r
    gf.info[:n, :2 * r.K] = fref.info
    gf.info[:n, :r.K] = np.float32(r.K) * gf.rsave[:n]
    gb = cc.bwd_buffers(inp, bref, Dx)
    gb.gtable[bref.named] = bref.gtable[bref.named]
    gb.dW[Dx:] = bref.dW[Dx:]
    gb.dzsum[:n] = bref.dzsum
    return r, inp, fref, bref, gf, gb


@pytest.mark.parametrize("name", ["d128_f4_k20", "d256_f4_k10", "d8_f3_k7"])
def test_judge_rejects_perturbed_results(name):
    r, inp, fref, bref, gf, gb = _perfect(name)
    Dx, K, n = r.F * r.D, r.K, inp.B * inp.T
    GS, SPL, _ = cc.geom(r.D, r.F)
    cc.judge_fwd(inp, K, Dx, 0, gf, fref)                  # the references pass
    cc.judge_bwd(inp, Dx, 0, gb, bref)
    rejected = 0

    def fwd_with(**kw):
        g = gf._replace(**{k: v.copy() for k, v in gf._asdict().items()})
        for k, fn in kw.items():
            fn(getattr(g, k))
        return g

    def bwd_with(**kw):
        g = gb._replace(**{k: v.copy() for k, v in gb._asdict().items()})
        for k, fn in kw.items():
            fn(getattr(g, k))
        return g

    def drop_k_fwd(o1):                                    # one k dropped from out1's sum
        o1[:n, :Dx] -= (fref.p[:, K - 1, None] * fref.s1[:, K - 1]).astype(np.float32)

    def drop_k_bwd(gt):                                    # ... and its seq1 rows from the table gradient
        less = cc.backward_ref(inp._replace(idx1=np.where(np.arange(K)[None, None, :, None] == K - 1, 0, inp.idx1)), K, r.F, 0)
        gt[bref.named] = less.gtable[bref.named]

    def drop_slot(a):                                      # lane 0's slot of the last register (columns of one float4)
        lo = (SPL - 1) * GS * 4 if (SPL - 1) * GS * 4 < Dx else 0
        if a.ndim == 2:
            a[:n, lo:lo + 4] = 0
        else:
            a[Dx + lo:Dx + lo + 4] = 0

    def unnormalised(o1):
        o1[:n, :Dx] = (o1[:n, :Dx].astype(np.float64) * fref.den).astype(np.float32)

    def no_relu_mask(gt):
        allon = cc.backward_ref(inp, K, r.F, 0, rsave=np.maximum(inp.rsave, np.float32(1e-30)))
        gt[bref.named] = allon.gtable[bref.named]

    def pad_written(o1):
        o1[n // 2, Dx] = 0

    def row0(gt):
        gt[0] = 0

    for what, side, got in (("one k dropped (forward)", 0, fwd_with(out1=drop_k_fwd)),
                            ("one k dropped (backward)", 1, bwd_with(gtable=drop_k_bwd)),
                            ("a slot of the last register dropped (out1)", 0, fwd_with(out1=drop_slot)),
                            ("a slot of the last register dropped (out2)", 0, fwd_with(out2=drop_slot)),
                            ("a slot of the last register dropped (dW)", 1, bwd_with(dW=drop_slot)),
                            ("p not normalised", 0, fwd_with(out1=unnormalised)),
                            ("dz without the relu mask", 1, bwd_with(gtable=no_relu_mask)),
                            ("a padding column written", 0, fwd_with(out1=pad_written)),
                            ("row 0 given a gradient", 1, bwd_with(gtable=row0))):
        with pytest.raises(cc.Rejected):
            if side == 0:
                cc.judge_fwd(inp, K, Dx, 0, got, fref)
            else:
                cc.judge_bwd(inp, Dx, 0, got, bref)
        rejected += 1
    assert rejected >= 6
