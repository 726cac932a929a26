"""score_gru_fwd / score_gru_bwd at their kernels' tile, step-count, length and stride edges (the rows of tests/gru_cases.py; their
CPU twin is tests/test_gru_cases_cpu.py).  Every row asserts the family, waves and direction score_gru_last_form reports before
it compares: out (exactly 0 past the length), final, the saved r, u, c at live steps, dxproj (exactly 0 at dead steps), rh and
hprev at live steps, and dWg / dWc formed in float64 from the kernel's dxproj, rh and hprev -- against the oracle's _gru with
autograd in float64, at the bounds of tests/test_gpu_ops.py::test_gru_fwd_bwd; canary columns beside out's and dout's H columns and
a canary row behind B * T in every output.  Run with -s: every row prints the kernels' errors as shares of the bounds."""
import ctypes as C

import numpy as np
import pytest
import torch

from score_amd import _lib
import gru_cases as gc

pytestmark = pytest.mark.gpu


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _canary(*shape):
    return torch.full(shape, float(gc.CANARY), device="cuda")


def _is_canary(t):
    return bool((t == float(gc.CANARY)).all())


@pytest.mark.parametrize("name", list(gc.ROWS))
def test_row(name):
    lib = _lib.load()
    r = gc.ROWS[name]
    inp = gc.inputs(r)
    H, B, T, n = r.H, r.B, r.T, r.B * r.T
    ref, ref_dwg, ref_dwc = gc.recurrence(r, inp, torch.float64)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    xproj, Wg, Wc, length = cu(inp.xproj.reshape(n, 3 * H)), cu(inp.Wg), cu(inp.Wc), cu(inp.length)
    out, gates = _canary(n + 1, inp.ldo), _canary(n + 1, 3 * H)
    fin = None if r.null_final else _canary(B + 1, H)
    rc = lib.score_gru_fwd(B, T, H, _ptr(xproj), _ptr(Wg), 2 * H, _ptr(Wc), H, _ptr(length), _ptr(out), inp.ldo, _ptr(gates),
                           _ptr(fin), _stream())
    word = lib.score_gru_last_form()
    torch.cuda.synchronize()
    assert rc == 0, (name, rc)
    assert gc.unpack(word) == r.fwd, (name, gc.unpack(word), r.fwd)                    # the form first
    assert _is_canary(out[:, H:]) and _is_canary(out[n:]) and _is_canary(gates[n:]) and (fin is None or _is_canary(fin[B:]))
    got_out = out[:n, :H].cpu().numpy().reshape(B, T, H)
    got = gc.Result(got_out, None if fin is None else fin[:B].cpu().numpy(), gates[:n].cpu().numpy().reshape(B, T, 3 * H), None, None, None)
    e = gc.compare(r, inp, got, ref, ref_dwg, ref_dwc, backward=False)

    dout = torch.full((n, inp.lddo), float("nan"), device="cuda")                      # (the padding is never read)
    dout[:, :H] = cu(inp.dout.reshape(n, H))
    dfinal = None if inp.dfinal is None else cu(inp.dfinal)
    dxproj, rh = _canary(n + 1, 3 * H), _canary(n + 1, H)
    hprev = _canary(n * H + 3 * H * H + H)             # (the LDS-state backward keeps its transposed weights in the 3 H H floats)
    rc = lib.score_gru_bwd(B, T, H, _ptr(Wg), 2 * H, _ptr(Wc), H, _ptr(length), _ptr(out), inp.ldo, _ptr(gates), _ptr(dout), inp.lddo,
                           _ptr(dfinal), _ptr(dxproj), _ptr(rh), _ptr(hprev), _stream())
    word = lib.score_gru_last_form()
    torch.cuda.synchronize()
    if r.bwd is None:
        # refused: SCORE_E_SHAPE, the word still names the forward, nothing written
        assert rc == gc.E_SHAPE and gc.unpack(word) == r.fwd
        assert _is_canary(dxproj) and _is_canary(rh) and _is_canary(hprev)
        print("%s: forward %s; backward refused" % (name, ", ".join("%s %.3f" % kv for kv in sorted(e.items()))))
        assert max(e.values()) <= 1.0, (name, e)
        return
    assert rc == 0, (name, rc)
    assert gc.unpack(word) == r.bwd, (name, gc.unpack(word), r.bwd)
    assert _is_canary(dxproj[n:]) and _is_canary(rh[n:]) and _is_canary(hprev[n * H + 3 * H * H:])
    assert r.bwd.family == gc.LDS or _is_canary(hprev[n * H:])
    assert torch.equal(out[:n, :H].cpu(), torch.from_numpy(got_out.reshape(n, H))) and _is_canary(out[:, H:])      # inputs untouched
    got = got._replace(dxproj=dxproj[:n].cpu().numpy().reshape(B, T, 3 * H), rh=rh[:n].cpu().numpy().reshape(B, T, H),
                       hprev=hprev[:n * H].cpu().numpy().reshape(B, T, H))
    e = gc.compare(r, inp, got, ref, ref_dwg, ref_dwc)
    print("%s: kernel errors as shares of the bounds: %s" % (name, ", ".join("%s %.3f" % kv for kv in sorted(e.items()))))
    assert max(e.values()) <= 1.0, (name, e)
