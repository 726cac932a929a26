"""score_coattn_fwd / score_coattn_bwd and the model's two-call launches at every instance, geometry and K seam of the fused
gather + co-attention kernels (csrc/embed.hip): the rows of tests/coattn_cases.py; their CPU twin is
tests/test_coattn_cases_cpu.py.  Every row asserts the instance score_coattn_last_forms reports before its numbers, at one unit
and at a ragged count above two workgroups; outputs, padding and untouched gradient rows against float64 restatements at the
bounds of tests/test_gpu_ops.py::test_coattn_fwd_bwd (mode 1: the int64 sums, bit for bit); the forward's outputs, dzsum and
dW bit for bit between two runs.  Model rows: gradients against the oracle's autograd, pull-form and atomic scatter, as
tests/test_gpu_coattn_bwd_prefetch.py builds its cases.  Run with -s: every row prints its errors as shares of the bounds."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import score_oracle as so
from score_amd import _lib
import coattn_cases as cc
from helpers import NAMES, away_from_relu_kinks, random_batch

H, N_MODEL = 16, 1500
HOPS = ("user_1hop", "user_2hop", "item_1hop", "item_2hop")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _padded(a, ld):
    """[n, ld] with a in the leading columns and NaN in the padding, which no kernel reads"""
    out = np.full((a.shape[0], ld), np.nan, np.float32)
    out[:, :a.shape[1]] = a
    return _cu(out)


def _forward(lib, r, inp):
    n, Dx = inp.B * inp.T, r.F * r.D
    host = cc.fwd_buffers(inp, r.K, Dx)
    out1, out2, info, rs = (_cu(a) for a in host)
    table, i1, i2 = _cu(inp.table), _cu(inp.idx1), _cu(inp.idx2)
    m0 = r.mode == 0
    tgt, W, bias = (_cu(inp.tgt), _cu(inp.W), _cu(inp.bias)) if m0 else (None, None, None)
    rc = lib.score_coattn_fwd(_ptr(table), cc.N_ROWS, r.D, r.F, r.K, inp.B, inp.T, _ptr(i1), _ptr(i2), _ptr(tgt), _ptr(W), _ptr(bias),
                              _ptr(out1), inp.ld1, _ptr(out2), inp.ld1, _ptr(info if m0 else None), inp.ldi, _ptr(rs if m0 else None),
                              r.mode, _stream())
    word = lib.score_coattn_last_forms(0)
    torch.cuda.synchronize()
    assert rc == 0, (r.name, rc)
    return word, cc.GotFwd(out1.cpu().numpy(), out2.cpu().numpy(), info.cpu().numpy(), rs.cpu().numpy())


def _backward(lib, r, inp, ref):
    n, Dx = inp.B * inp.T, r.F * r.D
    host = cc.bwd_buffers(inp, ref, Dx)
    gt, dW, dzs = (_cu(a) for a in host)
    table, i1, i2 = _cu(inp.table), _cu(inp.idx1), _cu(inp.idx2)
    g1, g2 = _padded(inp.g1, inp.ld1), _padded(inp.g2, inp.ld1)
    m0 = r.mode == 0
    W, rs, gi = (_cu(inp.W), _cu(inp.rsave), _padded(inp.ginfo, inp.ldi)) if m0 else (None, None, None)
    scratch = torch.empty((1 << 20,), device="cuda") if m0 else None
    rc = lib.score_coattn_bwd(_ptr(table), _ptr(gt), cc.N_ROWS, r.D, r.F, r.K, inp.B, inp.T, _ptr(i1), _ptr(i2), _ptr(W), _ptr(rs),
                              _ptr(g1), inp.ld1, _ptr(g2), inp.ld1, _ptr(gi), inp.ldi, _ptr(dzs if m0 else None), _ptr(dW if m0 else None),
                              _ptr(scratch), 1 << 20 if m0 else 0, r.mode, _stream())
    word = lib.score_coattn_last_forms(1)
    torch.cuda.synchronize()
    assert rc == 0, (r.name, rc)
    return word, cc.GotBwd(gt.cpu().numpy(), dW.cpu().numpy(), dzs.cpu().numpy())


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cc.ROWS))
def test_row(name):
    lib = _lib.load()
    r = cc.ROWS[name]
    Dx = r.F * r.D
    worst = {}
    for count in cc.COUNTS:
        inp = cc.inputs(name, count)
        if not r.planted:
            ch = lib.score_coattn_fwd_chunk(r.D, r.K, inp.B, inp.T, r.F, 0)
            want = r.fwd._replace(ch=ch) if r.fwd.units else r.fwd
            assert (ch > 0) == bool(r.fwd.units), (name, ch)
            fref = cc.forward_ref(inp, r.K, r.F, r.mode)
            word, got = _forward(lib, r, inp)
            assert cc.unpack_fwd(word) == want, (name, count, cc.unpack_fwd(word), want)                 # the form first
            e = cc.judge_fwd(inp, r.K, Dx, r.mode, got, fref)
            _, again = _forward(lib, r, inp)
            assert all(_same_bits(a, b) for a, b in zip(got, again)), (name, count)
            for k, v in e.items():
                worst[k] = max(worst.get(k, 0.0), v)
        bref = cc.backward_ref(inp, r.K, r.F, r.mode)
        word, got = _backward(lib, r, inp, bref)
        assert cc.unpack_bwd(word) == r.bwd, (name, count, cc.unpack_bwd(word), r.bwd)
        e = cc.judge_bwd(inp, Dx, r.mode, got, bref)
        _, again = _backward(lib, r, inp, bref)
        assert _same_bits(got.dzsum, again.dzsum) and _same_bits(got.dW[Dx:], again.dW[Dx:]), (name, count)
        if r.mode == 1:                                    # integer sums: the atomics' order cannot show
            assert _same_bits(got.gtable, again.gtable)
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("%s: errors as shares of the bounds: %s" % (name, ", ".join("%s %.3f" % kv for kv in sorted(worst.items())) or "exact"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cc.REFUSALS))
def test_refusal(name):
    """host only: the code, nothing launched (both form words and every buffer as before)"""
    lib = _lib.load()
    D, F, K, pad, null, short, code = cc.REFUSALS[name]
    B, T, Dx = 2, 3, F * D
    n, ld1, ldi = B * T, F * D + pad, 2 * K + 1
    words = lib.score_coattn_last_forms(0), lib.score_coattn_last_forms(1)
    can = lambda *s: torch.full(s, float(cc.CANARY), device="cuda")
    table = torch.zeros((cc.N_ROWS, max(D, 4)), device="cuda")
    idx = torch.ones((n, K, F), dtype=torch.int32, device="cuda")
    tgt, W, bias = torch.ones((B, Dx), device="cuda"), torch.ones((3 * Dx,), device="cuda"), torch.zeros((1,), device="cuda")
    out1, out2, info, rs = can(n, ld1), can(n, ld1), can(n, ldi), can(n, K)
    g = torch.ones((n, ld1), device="cuda")
    gi = torch.ones((n, ldi), device="cuda")
    gt, dzs, dW = can(cc.N_ROWS, max(D, 4)), can(n), can(3 * Dx)
    # one below what the slabs of the launch take: blocks * 2 * Dx floats, blocks = ceil(ceil(n / upw) / 4)
    upw = 64 // cc.geom(D, F)[0] if D % 4 == 0 else 1
    blocks = -(-(-(-n // upw)) // 4)
    floats = blocks * 2 * Dx - 1 if short else 1 << 20
    scratch = torch.empty((1 << 20,), device="cuda")
    p = lambda t, what: _ptr(None if null == what else t)
    mode0 = lambda t: _ptr(None if null == "mode0" else t)
    if not short:
        rc = lib.score_coattn_fwd(p(table, "table"), cc.N_ROWS, D, F, K, B, T, p(idx, "idx1"), _ptr(idx), _ptr(tgt), mode0(W), _ptr(bias),
                                  _ptr(out1), ld1, _ptr(out2), ld1, _ptr(info), ldi, _ptr(rs), 0, _stream())
        assert rc == code, (name, rc)
    rc = lib.score_coattn_bwd(p(table, "table"), _ptr(gt), cc.N_ROWS, D, F, K, B, T, p(idx, "idx1"), _ptr(idx), mode0(W), _ptr(rs),
                              _ptr(g), ld1, _ptr(g), ld1, _ptr(gi), ldi, _ptr(dzs), _ptr(dW), _ptr(scratch), floats, 0, _stream())
    assert rc == code, (name, rc)
    if null == "mode0":                                    # ... and legal in mode 1, which reads neither
        assert lib.score_coattn_bwd(_ptr(table), _ptr(gt), cc.N_ROWS, D, F, K, B, T, _ptr(idx), _ptr(idx), None, None, _ptr(g), ld1,
                                    _ptr(g), ld1, None, ldi, None, None, None, 0, 1, _stream()) == 0
        torch.cuda.synchronize()
        assert cc.unpack_bwd(lib.score_coattn_last_forms(1)) == cc.bwd_form(D, (F,), K, 1)
        return
    torch.cuda.synchronize()
    assert (lib.score_coattn_last_forms(0), lib.score_coattn_last_forms(1)) == words
    for t in (out1, out2, info, rs, gt, dzs, dW):
        assert bool((t == float(cc.CANARY)).all()), name


# ------------------------------------------------------------------------------------------------ model rows
@functools.lru_cache(maxsize=None)
def model_batch(name):
    """(cfg, params, batch): read-only (tests/test_gpu_coattn_bwd_prefetch.py batch_of, without its ids outside the table)"""
    D, Fu, Fi, K, B, T, slices, mt, seed = cc.MODEL_ROWS[name]
    cfg = so.Cfg(N_MODEL, D, H, T, K, Fu, Fi, mt)
    P = so.init_params(cfg, 5)
    rng = np.random.default_rng(seed)
    b = random_batch(rng, cfg, B)
    if slices < T:
        b["length"] = rng.integers(1, slices + 1, (B,)).astype(np.int32)
    b["length"][0] = slices
    for n in HOPS:                           # ids equal to 0 inside live slices
        b[n][rng.random(b[n].shape) < 0.1] = 0
    b, _, keep = away_from_relu_kinks(cfg, P, b)      # (asserts that three quarters of the batch stay)
    if keep[0] != 0:
        pytest.fail("%s: the sample that keeps every slice computed sits on a relu kink: another batch seed" % name)
    for v in list(P.values()) + list(b.values()):
        v.setflags(write=False)
    return cfg, P, b


@functools.lru_cache(maxsize=None)
def model_oracle_grads(name):
    cfg, P, b = model_batch(name)
    _, go = so.loss_and_grads(cfg, P, b, 0.0)
    for v in go.values():
        v.setflags(write=False)
    return go


@pytest.mark.parametrize("name", list(cc.MODEL_ROWS))
def test_model_row_has_its_unit_count(name):
    """the oracle alone: the kink filter leaves the row a few dozen units per call and its slice count"""
    cfg, _, b = model_batch(name)
    slices = cc.MODEL_ROWS[name][6]
    assert int(b["length"].max()) == slices and int(b["length"][0]) == slices
    units = len(b["label"]) * slices
    print("%s: %d samples, %d units per call" % (name, len(b["label"]), units))
    assert 9 <= units <= 48


@pytest.mark.gpu
@pytest.mark.parametrize("scatter_mode", [0, 1])
@pytest.mark.parametrize("name", list(cc.MODEL_ROWS))
def test_model_row(name, scatter_mode):
    from score_amd.model import MODELS
    lib = _lib.load()
    cfg, P, b = model_batch(name)
    D, Fu, Fi, K, _, T, slices, mt, _ = cc.MODEL_ROWS[name]
    m = MODELS[cfg.model_type](cfg.N, cfg.D, cfg.H, cfg.T, cfg.K, cfg.Fu, cfg.Fi)
    m.set_params({k: v.copy() for k, v in P.items()})
    m.scatter_mode = scatter_mode
    db = m.device_batch(tuple(b[n] for n in NAMES))
    assert (db.active_slices or cfg.T) == slices
    assert not m.persample_form(db.B, db.active_slices)      # the layer-by-layer pass: the co-attention kernels
    before = lib.score_coattn_last_forms(1)
    m.forward_backward(db, 0.0, 1.0)
    torch.cuda.synchronize()
    ch = lib.score_coattn_fwd_chunk(D, K, db.B, slices, Fi, Fu)
    fwd, bwd = cc.model_forms(name, scatter_mode, ch)
    got_f, got_b = lib.score_coattn_last_forms(0), lib.score_coattn_last_forms(1)
    assert cc.unpack_fwd(got_f) == fwd, (name, cc.unpack_fwd(got_f), fwd)
    if mt == "RCA" and scatter_mode == 0:      # the pull form has nothing to prepare in mode 1: no backward launch
        assert got_b == before
    else:
        assert cc.unpack_bwd(got_b) == bwd, (name, cc.unpack_bwd(got_b), bwd)
    assert int(m._id_status[0].item()) == 0
    go, g = model_oracle_grads(name), m.get_grads()
    worst = 0.0
    for n in sorted(go):
        got, want = np.asarray(g[n]).reshape(go[n].shape), go[n]
        worst = max(worst, float((np.abs(got - want) / (cc.ATOL + cc.RTOL * np.abs(want))).max()))
        assert np.allclose(got, want, rtol=cc.RTOL, atol=cc.ATOL), (name, n, float(np.abs(got - want).max()))
    print("%s scatter_mode %d: worst gradient error as a share of the bound: %.3f" % (name, scatter_mode, worst))
    assert not g["emb_mtx"][0].any() and g["emb_mtx"].any()
