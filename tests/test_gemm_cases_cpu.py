"""The rows of tests/test_gpu_gemm_edges.py (tests/gemm_cases.py) judged without a GPU: the restated launch rule gives every row
the form and the K chunks it names, the set of forms reached covers every kernel instance and every epilogue bit behind split-K,
the plain float32 numpy product meets the bound on every row (so the bound can be met: it is not vacuous), the skipped share
stays under its cap, and the bound rejects each of five subtly wrong results, evaluated in float64 alone."""
import numpy as np
import pytest

import gemm_cases as gc

ROWS = gc.ROWS


def test_every_row_has_the_form_and_the_k_chunks_it_names():
    for name, r in ROWS.items():
        f, kc = gc.mirror(r)
        assert f == r.form, (name, f, r.form)
        assert gc.slab_lengths(r.K, kc) == r.kslabs and len(r.kslabs) == r.form.slabs, (name, kc, r.kslabs)
        assert gc.unpack(gc.pack(f, r.trans)) == (f, r.trans, 0)
        assert gc.pack(f, r.trans) > 0
        if r.same_bits_as:
            o = ROWS[r.same_bits_as]
            assert o.form == r.form == gc.Form(gc.F32, r.form.wm, r.form.wn, r.form.slabs) and gc._operand_seed(o) == gc._operand_seed(r)
        # ragged against the tile: no row's M and N are both multiples of its block
        if name.startswith(("seam", "kloop", "ep_", "ld_")):
            assert r.M % 64 or r.N % 64, name


def test_the_seams_sit_where_the_rule_puts_them():
    """one M to either side of each seam of the f32 tile choice, from the rule alone (K = 16, no scratch)"""
    f = lambda M, N: gc.decide(0, M, N, 16, 16, N, 0, None)[0][1:3]
    assert [f(M, 65) for M in (24448, 24449, 24512, 24513, 49024, 49025)] == [(1, 1), (2, 1), (2, 1), (1, 2), (1, 2), (2, 2)]
    assert f(49025, 64) == (2, 1) and f(49025, 5) == (2, 1) and f(49024, 64) == (1, 1)
    # the scratch-limited loop: one float short of four slabs gives three, re-rounded to chunks of 192
    assert gc.decide(0, 6081, 65, 512, 512, 65, 0, 4 * 6081 * 65)[0].slabs == 4
    assert gc.decide(0, 6081, 65, 512, 512, 65, 0, 4 * 6081 * 65 - 1) == (gc.Form(gc.F32, 1, 2, 3), 192)
    assert gc.decide(0, 6081, 65, 512, 512, 65, 0, None)[0] == gc.Form(gc.F32, 1, 1, 1)          # no scratch: no cap, no (1,2)


def test_the_forms_reached_are_complete():
    reached = {(r.form.family, r.trans, r.form.wm, r.form.wn) for r in ROWS.values()}
    assert reached == gc.ALL_INSTANCES
    for fam in (gc.F32, gc.X3):
        for t in (0, 1, 2):
            split = [r for r in ROWS.values() if r.form.family == fam and r.trans == t and r.form.slabs > 1]
            direct = [r for r in ROWS.values() if r.form.family == fam and r.trans == t and r.form.slabs == 1]
            for rows in (split, direct):          # every epilogue bit, the row group and both mask kinds, in both places
                for bit in (1, 2, 4, 8, 64):
                    assert any(r.eflags & bit for r in rows), (fam, t, bit)
                assert any(r.g for r in rows) and {"byte", "hash", "y"} <= {r.mask for r in rows}
    # both sides of every refusal, every flag-16 threshold
    assert sum(r.route == 32 and r.form.family == gc.F32 for r in ROWS.values()) >= 3 * 4 + 5
    assert sum(r.route == 16 for r in ROWS.values()) == 7
    for r in ROWS.values():
        if r.g:
            assert r.M % r.g != 0


def test_hash_restated():
    u = gc.hash_uniform(1234, np.arange(1 << 16, dtype=np.uint64))
    assert u.dtype == np.float32 and 0 <= u.min() and u.max() < 1 and abs(float((u < np.float32(0.8)).mean()) - 0.8) < 0.01
    assert int(gc.hash_uniform(0, np.zeros(1, dtype=np.uint64))[0] * 16777216) == (0xE220A8397B1DCDAF >> 40)   # splitmix64's first output
    rows = [r for r in ROWS.values() if r.mask == "hash" and (r.M, r.N) == (200, 72)]
    assert len(rows) == 3 * 4 and {(r.form.family, r.form.slabs > 1) for r in rows} == {(1, False), (1, True), (2, False), (2, True)}


@pytest.mark.parametrize("name", list(ROWS))
def test_fp32_product_meets_the_bound_and_the_skips_stay_under_the_cap(name):
    r = ROWS[name]
    inp = gc.inputs(r)
    want, tol, skip = gc.reference(r, inp)
    assert skip.mean() <= gc.SKIP_CAP, (name, skip.mean())
    got, _ = gc.epilogue64(r, inp.a @ inp.b, inp)                  # the float32 product, float32 store
    worst = gc.judge(got.astype(np.float32), want, tol, skip)
    print("%s: fp32 numpy at %.3f of the bound, %d of %d skipped" % (name, worst, int(skip.sum()), skip.size))
    assert worst <= 1.0
    # the stored operands are the logical ones, everything around them NaN
    lda, ldb = gc.ld(r)
    A, B = inp.A[1], inp.B[1]
    assert A.shape[1] == lda and B.shape[1] == ldb and np.isnan(inp.A[0][:r.a_off]).all() and np.isnan(inp.B[0][:r.b_off]).all()
    assert np.array_equal(A[:, :lda - r.lda_pad], inp.a.T if r.trans == 2 else inp.a) and np.isnan(A[:, lda - r.lda_pad:]).all()
    assert np.array_equal(B[:, :ldb - r.ldb_pad], inp.b.T if r.trans == 1 else inp.b) and np.isnan(B[:, ldb - r.ldb_pad:]).all()
    if r.mask in ("byte", "hash"):
        assert 0.7 < inp.keepmask.mean() < 0.9
    elif r.mask == "y":
        assert 0.25 < inp.keepmask.mean() < 0.45 and (inp.y == 0).mean() > 0.25 and (inp.y < 0).any()


# ------------------------------------------------------------------------------------------ the bound catches a wrong kernel
def _bf16_rne(x):
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _two_terms(x):
    hi = _bf16_rne(x)
    return (hi.astype(np.float64) + _bf16_rne(x - hi).astype(np.float64))


def _rejected(rows, perturbed):
    """names of the rows whose perturbed float64 result the bound rejects; every unperturbed float64 result passes"""
    out = []
    for r in rows:
        inp = gc.inputs(r)
        want, tol, skip = gc.reference(r, inp)
        assert gc.judge(want, want, tol, skip) == 0.0
        got = perturbed(r, inp, want)
        if got is not None and gc.judge(got, want, tol, skip) > 1.0:
            out.append(r.name)
    return out


SMALL = [r for r in ROWS.values() if r.M <= 4096]


def test_bound_rejects_a_dropped_k_quad():
    def drop(r, inp, want):
        if r.K < 8:
            return None
        k0 = (r.K // 4 - 1) * 4
        a = inp.a.astype(np.float64).copy()
        a[:64, k0:k0 + 4] = 0                                   # one quad of one row tile never staged
        return gc.epilogue64(r, a @ inp.b.astype(np.float64), inp)[0]
    rows = [r for r in SMALL if r.name.startswith(("kloop", "ep_plain", "ep_bias_relu", "ep_relugrad_x3"))]
    rej = _rejected(rows, drop)
    assert len(rej) == len([r for r in rows if r.K >= 8]), sorted(set(r.name for r in rows) - set(rej))


def test_bound_rejects_the_bias_row_of_the_next_output_row():
    rows = [r for r in ROWS.values() if r.g == 3]
    assert len(rows) == 12
    rej = _rejected(rows, lambda r, inp, want: gc.epilogue64(r, inp.a.astype(np.float64) @ inp.b.astype(np.float64), inp, bias_shift=1)[0])
    assert len(rej) == len(rows)


def test_bound_rejects_a_mask_or_y_indexed_with_ldc():
    def wrong(r, inp, want):
        e = (np.arange(r.M)[:, None] * (r.N + 3) + np.arange(r.N)[None, :]) % (r.M * r.N)
        return gc.epilogue64(r, inp.a.astype(np.float64) @ inp.b.astype(np.float64), inp, keepmask=inp.keepmask.reshape(-1)[e])[0]
    rows = [r for r in ROWS.values() if r.mask in ("byte", "y")]
    assert len(rows) == 3 * 3 * 4
    assert len(_rejected(rows, wrong)) == len(rows)


def test_bound_rejects_a_duplicated_last_row():
    def dup(r, inp, want):
        got = want.copy()
        got[r.M - 2] = got[r.M - 1]
        return got
    rows = [r for r in SMALL if r.name.startswith(("ep_", "kloop", "refuse", "ld_"))]
    assert len(_rejected(rows, dup)) == len(rows)


def test_bound_rejects_operands_of_two_bf16_terms():
    def two(r, inp, want):
        return gc.epilogue64(r, _two_terms(inp.a) @ _two_terms(inp.b), inp)[0]
    rows = [r for r in SMALL if r.form.family == gc.X3 and r.form.slabs == 1]
    rej = _rejected(rows, two)
    print("two-term operands rejected on %d of %d bf16x3 rows" % (len(rej), len(rows)))
    assert len(rej) >= len(rows) // 2 and any(n.startswith("x3rule") for n in rej)
