"""score_gemm at every dispatch form and epilogue (the rows of tests/gemm_cases.py; their CPU twin is tests/test_gemm_cases_cpu.py).
Every row first asserts the form score_gemm_last_form reports -- a row that fell back to another kernel fails, it does not test that
kernel --, then that nothing was written past column N, that two runs give the same bits, and the float64 bound of
tests/test_gpu_ops.py::test_gemm_fp32 with the epilogue applied in float64.  Rows that name another row of the same operands
(aligned against misaligned copies) must match it bit for bit; the hashed dropout mask must keep the same elements wherever it is
computed.  Run with -s: each row prints the kernel's worst error as a share of the bound."""
import ctypes as C

import numpy as np
import pytest
import torch

from score_amd import _lib
import gemm_cases as gc

pytestmark = pytest.mark.gpu

_SCRATCH = []
_KEPT = {}                                                              # outputs other rows are compared with
_KEEP_NAMES = {r.same_bits_as for r in gc.ROWS.values() if r.same_bits_as} | {n for n, r in gc.ROWS.items() if r.mask == "hash"}


def _ptr(t, off_floats=0):
    return C.c_void_p(t.data_ptr() + 4 * off_floats) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _scratch():
    if not _SCRATCH:
        _SCRATCH.append(torch.empty((gc.SCRATCH_FULL,), device="cuda"))
    return _SCRATCH[0]


def _call(r, inp, flags, mask_t, dev):
    """one score_gemm call on a fresh copy of c0; returns (status, form word, C [M, N + 3] on the host)"""
    lib = _lib.load()
    lda, ldb = gc.ld(r)
    c = dev["c0"].clone()
    sf = gc.scratch_floats(r)
    scr = None
    if sf is not None:
        scr = _scratch()
        scr.fill_(float("nan"))                                         # a slab element read before it was written shows
    rc = lib.score_gemm(r.trans, r.M, r.N, r.K, _ptr(dev["A"], r.a_off), lda, _ptr(dev["B"], r.b_off), ldb, _ptr(c), r.N + 3,
                        _ptr(dev["bias"]), flags, r.keep, _ptr(mask_t), gc.HASH_SEED, _ptr(scr), sf or 0, _stream())
    word = lib.score_gemm_last_form()
    torch.cuda.synchronize()
    return rc, word, c.cpu().numpy()


def _device(r, inp):
    dev = {k: torch.from_numpy(v).cuda() for k, v in (("A", inp.A[0]), ("B", inp.B[0]), ("bias", inp.bias), ("c0", inp.c0))}
    mask_t = None
    if inp.mask is not None:
        mask_t = torch.from_numpy(inp.mask).cuda()
    elif inp.y is not None:
        mask_t = torch.from_numpy(inp.y).cuda()
    return dev, mask_t


def _run(name):
    if name in _KEPT:
        return _KEPT[name]
    r = gc.ROWS[name]
    inp = gc.inputs(r)
    dev, mask_t = _device(r, inp)
    rc, word, c = _call(r, inp, gc.kernel_flags(r), mask_t, dev)
    assert rc == 0, (name, rc)
    # the form first: the kernel instance, its tile and the K slabs the row names
    assert gc.unpack(word) == (r.form, r.trans, 0), (name, gc.unpack(word), r.form)
    rc2, word2, c2 = _call(r, inp, gc.kernel_flags(r), mask_t, dev)
    assert rc2 == 0 and word2 == word
    assert np.array_equal(c.view(np.uint32), c2.view(np.uint32)), "two runs differ"
    assert np.array_equal(c[:, r.N:].view(np.uint32), inp.c0[:, r.N:].view(np.uint32)), "wrote past column N"
    out = (r, inp, c[:, :r.N].copy())
    if name in _KEEP_NAMES:
        _KEPT[name] = out
    return out


@pytest.mark.parametrize("name", list(gc.ROWS))
def test_row(name):
    r, inp, got = _run(name)
    want, tol, skip = gc.reference(r, inp)
    worst = gc.judge(got, want, tol, skip)
    print("%s: form %s, kernel at %.3f of the bound (%d of %d skipped)" % (name, tuple(r.form), worst, int(skip.sum()), skip.size))
    assert worst <= 1.0, (name, worst)
    if r.eflags & (gc.GF_DROP | gc.GF_RELUGRAD) and not r.eflags & gc.GF_ACC:
        assert not got[~inp.keepmask].any()                             # dropped elements are exact zeros
    if r.same_bits_as:
        _, _, other = _run(r.same_bits_as)
        assert np.array_equal(got.view(np.uint32), other.view(np.uint32)), (name, r.same_bits_as)


@pytest.mark.parametrize("trans", [0, 1, 2])
def test_hashed_mask_keeps_the_same_elements_wherever_it_is_computed(trans):
    """one (M, N, seed): the f32 kernel's epilogue, splitk_reduce_kernel behind either family, the bf16x3 kernel's own epilogue --
    and the splitmix64 finaliser restated on the host"""
    names = ["%s-t%d" % (n, trans) for n in ("hash_f32_direct", "ep_drop_hash_f32_split", "hash_x3_direct", "ep_drop_hash_x3_split")]
    want = gc.hashed_keep(gc.HASH_SEED, 200, 72, 0.8)
    for n in names:
        r, inp, got = _run(n)
        assert (r.M, r.N, r.mask) == (200, 72, "hash")
        assert np.array_equal(got != 0, want), n


@pytest.mark.parametrize("trans", [0, 1, 2])
def test_relu_gradient_flag_refuses_dropout_and_a_null_mask(trans):
    r = gc.ROWS["ep_relugrad_f32_direct-t%d" % trans]
    inp = gc.inputs(r)
    dev, y = _device(r, inp)
    before = _lib.load().score_gemm_last_form()
    for name, flags, mask in gc.BADARG_ROWS:
        rc, word, c = _call(r, inp, flags, y if mask == "y" else None, dev)
        assert rc == gc.E_BADARG, (name, rc)
        assert word == before and np.array_equal(c.view(np.uint32), inp.c0.view(np.uint32)), name      # nothing launched
