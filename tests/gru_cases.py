"""The rows of tests/test_gpu_gru_edges.py and their CPU twin (tests/test_gru_cases_cpu.py): which recurrence score_gru_fwd /
score_gru_bwd (csrc/gru.hip) take for a shape, restated in Python in the terms of score_gru_last_form (include/score_hip.h); a
table of shapes at the kernels' tile, step-count and length edges; the rows' inputs from fixed seeds; the float64 reference (the
oracle's _gru with autograd, x entering through selector kernels so that x . Wx is xproj itself, as
tests/test_gpu_ops.py::test_gru_three_steps_over_the_saturation_grid does) and the comparison both tests share.  No GPU and no
library is needed here.

Bounds: the suite's own (test_gru_fwd_bwd) -- forward rtol 1e-5, atol 2e-6; backward rtol 2e-4, atol 2e-5."""
from collections import namedtuple

import numpy as np
import torch

from oracle import score_oracle as so

X3, REG, STREAM, STEPS, LDS = 1, 2, 3, 4, 5              # the family field of score_gru_last_form
FWD_TOL = (1e-5, 2e-6)
BWD_TOL = (2e-4, 2e-5)
E_SHAPE = -2
CANARY = np.float32(-12345.5)

Form = namedtuple("Form", "family waves backward")


def pack(f):
    return f.family | f.waves << 4 | f.backward << 8


def unpack(word):
    return Form(word & 7, word >> 4 & 15, word >> 8 & 1)


def route(H, T, backward):
    """the Form score_gru_fwd / score_gru_bwd launch for (H, T), or None where they refuse (SCORE_E_SHAPE).  The two extern
    entries allow the bf16x3 recurrence and eight waves at H = 128; H = 256 has no register-resident form and, outside the
    engine, no streamed one: it keeps its state in LDS like every other width"""
    if H == 128:
        return Form(X3, 8, backward)
    if H in (16, 32, 64):
        return Form(REG, 2 if backward and H == 32 and T >= 20 else 4, backward)
    lds = 32 * (4 * H + 3) * 4 if backward else 3 * 32 * (H + 1) * 4       # 32 rows of state per workgroup
    return Form(LDS, 4, backward) if lds <= 160 * 1024 else None


# lengths: "mixed" = 0 at the first, a middle and the last sample, one exactly T, one T + 3 (behaves as T), the rest random in
# [1, T] (a batch of fewer than five: all T); "zero": an all-zero batch; "full": all T.
# pad: ldo = H + 4 and lddo = H + 8 with canary columns (else H); scale: the recurrent weights are N(0, 1) scale / sqrt(H)
Row = namedtuple("Row", "name H B T lengths pad null_final null_dfinal scale fwd bwd why")
ROWS = {}


def _row(H, B, T, fwd, bwd, lengths="mixed", pad=True, null_final=False, null_dfinal=False, scale=1.0, why="", tag=""):
    name = "h%d_b%d_t%d%s" % (H, B, T, tag)
    assert name not in ROWS, name
    ROWS[name] = Row(name, H, B, T, lengths, pad, null_final, null_dfinal, scale,
                     Form(fwd[0], fwd[1], 0) if fwd else None, Form(bwd[0], bwd[1], 1) if bwd else None, why)


# -- the 16-row families: a workgroup owns 16 samples, rows past the batch duplicate the last one
for H in (16, 32, 64):
    for B in (1, 15, 16, 17, 33):
        _row(H, B, 4, (REG, 4), (REG, 4), pad=B != 16, why="register form, four waves, batch edge of the 16-row tile")
    _row(H, 17, 50, (REG, 4), (REG, 2 if H == 32 else 4), why="the point models' length")
for B, T in ((1, 1), (15, 2), (16, 3), (17, 4), (33, 5)):
    _row(128, B, T, (X3, 8), (X3, 8), pad=B != 16, why="bf16x3 recurrence: its three-step prefetch at T = %d, batch edge" % T)
_row(128, 17, 50, (X3, 8), (X3, 8), why="the point models' length")
# -- H = 32 backward: four waves below 20 slices, two from 20 on (gru_bwd_reg_kernel<32, 2>)
_row(32, 17, 19, (REG, 4), (REG, 4), why="last T of the four-wave backward")
_row(32, 17, 20, (REG, 4), (REG, 2), why="first T of the two-wave backward")
_row(32, 33, 21, (REG, 4), (REG, 2), pad=False, why="two-wave backward, three workgroups")
# -- state in LDS: a workgroup owns 32 samples
for H in (20, 48, 256):
    for B in (1, 31, 32, 33):
        _row(H, B, 2 if H == 256 else 3, (LDS, 4), (LDS, 4), pad=B != 32, why="LDS-state form, batch edge of the 32-row tile")
_row(48, 33, 50, (LDS, 4), (LDS, 4), why="the point models' length")
# -- lengths and null pointers, one row per family
for H, B, fam, w in ((32, 17, REG, 4), (128, 17, X3, 8), (20, 33, LDS, 4)):
    _row(H, B, 3, (fam, w), (fam, w), lengths="zero", tag="_zero", why="an all-zero batch: nothing live")
    _row(H, B, 3, (fam, w), (fam, w), lengths="full", pad=False, tag="_full", why="every length exactly T, ldo = lddo = H")
    _row(H, B, 3, (fam, w), (fam, w), null_final=True, tag="_nofinal", why="final_state NULL")
    _row(H, B, 3, (fam, w), (fam, w), null_dfinal=True, tag="_nodfinal", why="dfinal NULL")
# -- the forward's LDS rule (3 x 32 x (H + 1) floats) admits H = 320, the backward's (32 x (4 H + 3)) does not
_row(320, 2, 2, (LDS, 4), None, lengths="full", why="forward runs, backward refuses with SCORE_E_SHAPE and writes nothing")


def lengths(r):
    rng = np.random.default_rng([r.H, r.B, r.T, 1])
    if r.lengths == "zero":
        return np.zeros(r.B, dtype=np.int32)
    if r.lengths == "full" or r.B < 5:
        return np.full(r.B, r.T, dtype=np.int32)
    L = rng.integers(1, r.T + 1, r.B).astype(np.int32)
    L[0] = L[r.B // 2] = L[r.B - 1] = 0
    L[1] = r.T
    L[2] = r.T + 3
    return L


Inputs = namedtuple("Inputs", "xproj Wg Wc length dout dfinal ldo lddo")


def inputs(r):
    """xproj [B, T, 3H], Wg [H, 2H], Wc [H, H] (the h rows of the two kernels), dout [B, T, H], dfinal [B, H] or None: float32"""
    rng = np.random.default_rng([r.H, r.B, r.T, 2])
    H = r.H
    xproj = rng.standard_normal((r.B, r.T, 3 * H)).astype(np.float32)
    Wg = (rng.standard_normal((H, 2 * H)) * (r.scale / np.sqrt(H))).astype(np.float32)
    Wc = (rng.standard_normal((H, H)) * (r.scale / np.sqrt(H))).astype(np.float32)
    dout = rng.standard_normal((r.B, r.T, H)).astype(np.float32)
    dfinal = None if r.null_dfinal else rng.standard_normal((r.B, H)).astype(np.float32)
    return Inputs(xproj, Wg, Wc, lengths(r), dout, dfinal, H + 4 if r.pad else H, H + 8 if r.pad else H)


Result = namedtuple("Result", "out final gates dxproj rh hprev")      # [B,T,H] [B,H] [B,T,3H] [B,T,3H] [B,T,H] [B,T,H]


def recurrence(r, inp, dtype):
    """the oracle's _gru and autograd in `dtype` from the fp32 inputs: everything the kernels compute or save, plus the weight
    gradients (dWg [H, 2H], dWc [H, H]) autograd gives"""
    H, B, T = r.H, r.B, r.T
    eye = torch.eye(3 * H, dtype=dtype)
    x = torch.tensor(inp.xproj, dtype=dtype, requires_grad=True)
    Wg = torch.cat([eye[:, :2 * H], torch.tensor(inp.Wg, dtype=dtype)], 0).requires_grad_(True)
    Wc = torch.cat([eye[:, 2 * H:], torch.tensor(inp.Wc, dtype=dtype)], 0).requires_grad_(True)
    outs, hfin = so._gru(x, torch.as_tensor(inp.length.astype(np.int64)), Wg, torch.zeros(2 * H, dtype=dtype), Wc,
                         torch.zeros(H, dtype=dtype), H)
    loss = (outs * torch.tensor(inp.dout, dtype=dtype)).sum()
    if inp.dfinal is not None:
        loss = loss + (hfin * torch.tensor(inp.dfinal, dtype=dtype)).sum()
    loss.backward()
    np_t = np.float64 if dtype == torch.float64 else np.float32
    out = outs.detach().numpy()
    # the saved activations, from the states the oracle returned (a live step's h_{t-1} is the previous output: lengths are prefixes)
    hprev = np.concatenate([np.zeros((B, 1, H), dtype=np_t), out[:, :-1]], 1)
    live = live_mask(r, inp)[:, :, None]
    hprev = np.where(live, hprev, 0)
    wg, wc = inp.Wg.astype(np_t), inp.Wc.astype(np_t)
    xp = inp.xproj.astype(np_t)
    g = 1 / (1 + np.exp(-(xp[:, :, :2 * H] + hprev @ wg)))
    rh = g[:, :, :H] * hprev
    c = np.tanh(xp[:, :, 2 * H:] + rh @ wc)
    res = Result(out, hfin.detach().numpy(), np.concatenate([g, c], 2).astype(np_t), x.grad.numpy(), rh.astype(np_t), hprev.astype(np_t))
    return res, Wg.grad.numpy()[3 * H:], Wc.grad.numpy()[3 * H:]


def live_mask(r, inp):
    return np.arange(r.T)[None, :] < inp.length[:, None]            # [B, T]; a length above T behaves as T


def weight_grads(r, res):
    """dWg = hprev^T dxproj[:, :2H], dWc = rh^T dxproj[:, 2H:], summed in float64 from what the kernel (or the fp32 oracle) left"""
    H = r.H
    d = res.dxproj.reshape(-1, 3 * H).astype(np.float64)
    return res.hprev.reshape(-1, H).astype(np.float64).T @ d[:, :2 * H], res.rh.reshape(-1, H).astype(np.float64).T @ d[:, 2 * H:]


def _ratio(got, want, tol, where=None):
    """worst |got - want| / (atol + rtol |want|) over `where`; a non-finite element counts as infinitely wrong"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    e = np.abs(got - want) / (tol[1] + tol[0] * np.abs(want))
    e = np.where(np.isfinite(got), e, np.inf)
    if where is not None:
        e = np.where(np.broadcast_to(where, e.shape), e, 0.0)
    return float(e.max()) if e.size else 0.0


def compare(r, inp, got, ref, ref_dwg, ref_dwc, backward=True):
    """every quantity's worst error as a share of its bound (<= 1 passes), and the exact properties asserted outright: out and
    dxproj exactly 0 past the length, rh and hprev finite everywhere"""
    live = live_mask(r, inp)[:, :, None]
    dead = ~np.broadcast_to(live, got.out.shape)
    assert not got.out[dead].any(), "out is not exactly 0 past the length"
    e = {"out": _ratio(got.out, ref.out, FWD_TOL), "gates": _ratio(got.gates, ref.gates, FWD_TOL, live)}
    if got.final is not None:
        e["final"] = _ratio(got.final, ref.final, FWD_TOL)
    if backward:
        assert not got.dxproj[np.broadcast_to(~live, got.dxproj.shape)].any(), "dxproj is not exactly 0 past the length"
        assert np.isfinite(got.rh).all() and np.isfinite(got.hprev).all()
        e["dxproj"] = _ratio(got.dxproj, ref.dxproj, BWD_TOL)
        e["rh"] = _ratio(got.rh, ref.rh, FWD_TOL, live)
        e["hprev"] = _ratio(got.hprev, ref.hprev, FWD_TOL, live)
        dwg, dwc = weight_grads(r, got)
        e["dWg"] = _ratio(dwg, ref_dwg, BWD_TOL)
        e["dWc"] = _ratio(dwc, ref_dwc, BWD_TOL)
    return e
