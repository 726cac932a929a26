"""The fused gather + co-attention forward in its several-units-per-wave form (csrc/embed.hip coattn_fwd_kernel_units:
mode 0, K <= 10, one float4 per lane, id lists that fit an instance): a group of lanes works through a chunk of CH
consecutive time slices of one sample, holds a unit's ids one element per lane, and requests the next unit's ids behind
the current unit's rows.  debug_flags bit 17 runs coattn_fwd_kernel, one unit per wave, instead: the two must write the
same bits, for every input.

Bitwise tests, through a SCORE model's forward pass at the smallest shapes at which the chunk loop can go wrong (the
regions xside, atten_info, rsave and y_pred of the workspace, and the id_status word):

* chunk edges: 1, 2, CH - 1, CH, CH + 1 and 2 CH + 1 computed slices for the CH that the launcher picks
  (score_coattn_fwd_chunk: a function of the shape, so the batch is large enough for it to pick more than one slice --
  two full rounds of resident waves), all with fewer computed slices than the index tensors hold;
* wave edges at D = 16, K = 4 (GS = 16: four groups, each with a chunk of another sample, share a wave): one sample,
  a chunk count that is no multiple of the groups per wave, and one that is one above a multiple of a workgroup's;
  here the rule picks one slice per chunk, so every case also runs with a chunk length of 3 asked for in bits 20 .. 23;
* D = 64 with F = 4 (64 live lanes) and F = 3 (48) -- the model's two calls --, D = 16, K in {1, 4, 5, 10}, and K = 20,
  which like (D = 16, K > 4) keeps coattn_fwd_kernel under either flag;
* row 0, ids repeated inside a unit, ids >= n_rows and < 0 in idx1, idx2 and the target ids.

Tolerance tests, through score_coattn_fwd (the cc.tgt path, which the model does not take) against the oracle's collapsed
co-attention at test_gpu_ops.py test_coattn_fwd_bwd's bound, 1e-5 of the largest reference magnitude, with padded leading
dimensions whose padding stays zero.  H = 16 keeps the model off the per-sample whole-model kernels."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import score_oracle as so
from helpers import NAMES, random_batch

pytestmark = pytest.mark.gpu

ONE_UNIT = 131072      # score_state_t.debug_flags bit 17
CH_SHIFT = 20          # bits 20 .. 23: a chunk length to take instead of the rule's
H, N = 16, 1500
HOPS = ("user_1hop", "user_2hop", "item_1hop", "item_2hop")
REGIONS = ("xside", "atten_info", "rsave", "y_pred")

# name -> (D, Fu, Fi, K, B, T of the index tensors, computed slices: a number or a function of CH, chunk lengths asked for
#          besides the rule's, ids outside the table)
CASES = {
    "slices_1": (64, 3, 4, 10, 4096, 14, lambda ch: 1, (), False),
    "slices_2": (64, 3, 4, 10, 4096, 14, lambda ch: 2, (), False),
    "slices_ch_minus_1": (64, 3, 4, 10, 4096, 14, lambda ch: ch - 1, (), False),
    "slices_ch": (64, 3, 4, 10, 4096, 14, lambda ch: ch, (), False),
    "slices_ch_plus_1": (64, 3, 4, 10, 4096, 14, lambda ch: ch + 1, (), False),
    "slices_2ch_plus_1": (64, 3, 4, 10, 4096, 14, lambda ch: 2 * ch + 1, (), False),
    "one_sample": (16, 3, 4, 4, 1, 7, 5, (3,), False),                 # 2 chunks of 3 slices: half a wave's groups
    "chunks_not_per_wave": (16, 3, 4, 4, 7, 7, 7, (3,), False),        # 21 chunks of 3, 49 of 1: no multiple of 4
    "chunks_one_over_block": (16, 3, 4, 4, 11, 8, 7, (3,), False),     # 33 = 2 * 16 + 1 chunks of 3: a workgroup with one group
    "d64_k1": (64, 3, 4, 1, 5, 7, 7, (2, 3), False),
    "d64_k4": (64, 3, 4, 4, 5, 7, 7, (2, 3), False),
    "d64_k5": (64, 3, 4, 5, 5, 7, 7, (2, 3), False),
    "d64_k10": (64, 3, 4, 10, 5, 7, 6, (2, 3, 4), False),
    "d16_k1": (16, 3, 4, 1, 9, 7, 7, (2, 3), False),
    "d16_k5": (16, 3, 4, 5, 9, 7, 7, (3,), False),                     # two id registers at KMAX = 10: coattn_fwd_kernel
    "d16_k10": (16, 3, 4, 10, 9, 7, 7, (3,), False),
    "k20_fallback": (64, 3, 4, 20, 5, 5, 5, (3,), False),
    "bad_ids_d64": (64, 3, 4, 10, 37, 9, 7, (2, 3), True),
    "bad_ids_d16": (16, 3, 4, 4, 37, 9, 7, (2, 3), True),
}
BAD_BITS = 0x3f      # the four hop tensors (feed positions 0 .. 3), target_user (4), target_item (5)


def fwd_chunk(D, K, B, A, F0, F1):
    from score_amd import _lib
    return int(_lib.load().score_coattn_fwd_chunk(D, K, B, A, F0, F1))


@functools.lru_cache(maxsize=None)
def batch_of(name):
    """(cfg, params, fed batch, computed slices, the launcher's chunk length for them): read-only"""
    D, Fu, Fi, K, B, T, slices, _, bad = CASES[name]
    cfg = so.Cfg(N, D, H, T, K, Fu, Fi, "SCORE")
    P = so.init_params(cfg, 5)
    rng = np.random.default_rng(len(name) + D + K)
    b = random_batch(rng, cfg, B)            # ragged length; a fifth of the slices all-zero ids
    if callable(slices):
        slices = slices(fwd_chunk(D, K, B, T, Fi, Fu))
    assert 1 <= slices <= T
    b["length"] = rng.integers(1, slices + 1, (B,)).astype(np.int32)
    b["length"][0] = slices
    for n in HOPS:
        b[n][rng.random(b[n].shape) < 0.1] = 0                 # row 0 inside live slices
        b[n][:, :, 1:3] = b[n][:, :, :1]                        # the same id several times in a unit (K >= 2)
    if bad:
        vals = np.array([N, N + 5, 10 ** 6, -3, -2 ** 31, 2 ** 31 - 1], dtype=np.int64).astype(np.int32)
        for n in HOPS:
            flat = b[n][:, :slices].reshape(-1)
            hit = rng.choice(flat.size, 12, replace=False)
            flat[hit] = np.resize(vals, hit.size)
            b[n][:, :slices] = flat.reshape(b[n][:, :slices].shape)
        for n in ("target_user", "target_item"):
            b[n][::5, 0] = np.resize(vals, b[n][::5, 0].shape)
    for v in list(P.values()) + list(b.values()):
        v.setflags(write=False)
    return cfg, P, b, slices, fwd_chunk(D, K, B, slices, Fi, Fu)


def run(name, flags):
    """the forward pass under `flags`: the four regions' computed parts and the id_status word"""
    from score_amd.model import MODELS
    cfg, P, b, slices, _ = batch_of(name)
    m = MODELS[cfg.model_type](cfg.N, cfg.D, cfg.H, cfg.T, cfg.K, cfg.Fu, cfg.Fi)
    m.set_params({k: v.copy() for k, v in P.items()})
    m.debug_flags = flags
    db = m.device_batch(tuple(b[n] for n in NAMES))
    assert (db.active_slices or cfg.T) == slices
    assert not m.persample_form(db.B, db.active_slices)      # the layer-by-layer pass: score_coattn_fwd_multi
    lay, ws, _ = m._forward(db, 0.0, 1.0, None)
    torch.cuda.synchronize()
    B, I = db.B, cfg.Di + cfg.Du
    size = {"xside": None, "atten_info": B * slices * 4 * cfg.K, "rsave": None, "y_pred": B}
    out = {}
    for r in REGIONS:
        if r == "xside":      # two sides, [B * T * I] apart, [B * slices, I] computed of each
            t = m.ws_tensor(B, r, (2, B * cfg.T * I))[:, :B * slices * I]
        elif r == "rsave":    # two calls, [B * T * K] apart, each region starting at a multiple of four floats
            n, stride = B * slices * cfg.K, -(-B * cfg.T * cfg.K // 4) * 4
            flat = m.ws_tensor(B, r, (stride + n,))
            t = torch.stack([flat[:n], flat[stride:stride + n]])
        else:
            t = m.ws_tensor(B, r, (size[r],))
        out[r] = t.clone()
    return out, int(m._id_status[0].item())


@pytest.mark.parametrize("name", list(CASES))
def test_bitwise_equal_to_one_unit_per_wave(name):
    D, Fu, Fi, K, B, T, _, asked, bad = CASES[name]
    cfg, _, _, slices, ch = batch_of(name)
    print("%s: %d samples, %d of %d slices computed, chunk length %d by the rule" % (name, B, slices, T, ch))
    if name.startswith("slices_"):
        assert ch >= 2, "the batch is too small for the launcher to pick a chunk of several slices"
        assert ch == fwd_chunk(D, K, B, T, Fi, Fu)      # (the chunk length the case's slice count was derived from)
    if name in ("k20_fallback", "d16_k5", "d16_k10"):
        assert ch == 0
    elif name != "k20_fallback":
        assert ch >= 1
    want, status = run(name, ONE_UNIT)
    assert status == (BAD_BITS if bad else 0)
    for r in REGIONS:
        assert bool(torch.isfinite(want[r]).all()) and bool(want[r].any()), r
    for flags in (0,) + tuple(c << CH_SHIFT for c in asked):
        got, st = run(name, flags)
        for r in REGIONS:
            assert torch.equal(got[r], want[r]), (r, flags)
        assert st == status, flags


def P_(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("D,F,K,B,T", [(64, 4, 10, 3, 7), (64, 3, 5, 1, 1), (16, 4, 10, 5, 19), (8, 1, 4, 6, 5)])
def test_coattn_fwd_against_oracle(D, F, K, B, T):
    from score_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(D + F + K)
    Nr = 500
    Dx = F * D
    table = rng.standard_normal((Nr, D)).astype(np.float32)
    table[0] = 0
    idx1 = rng.integers(0, Nr, (B, T, K, F)).astype(np.int32)
    idx2 = rng.integers(0, Nr, (B, T, K, F)).astype(np.int32)
    idx1[0, 0] = 0
    idx2[0, 0] = 0
    if K > 2:
        idx1[-1, :, 2:] = idx1[-1, :, :1]
    tgt = table[rng.integers(1, Nr, (B, F))].reshape(B, Dx)
    W = (rng.standard_normal((3 * Dx, 1)) * 0.2).astype(np.float32)
    bias = np.asarray([0.1], dtype=np.float32)
    tt = torch.tensor(table)
    s1 = tt[torch.as_tensor(idx1).long()].reshape(B, T, K, Dx)
    s2 = tt[torch.as_tensor(idx2).long()].reshape(B, T, K, Dx)
    o1, o2, info = so._co_attention_collapsed(s1, s2, torch.tensor(tgt), torch.tensor(W), torch.tensor(bias))

    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    dt, di1, di2, dtg, dW, db = dev(table), dev(idx1), dev(idx2), dev(tgt), dev(W.reshape(-1)), dev(bias)
    ld1, ldi = Dx + 4, 2 * K + 1
    out1 = torch.zeros((B * T, ld1), device="cuda")
    out2 = torch.zeros((B * T, Dx), device="cuda")
    oinfo = torch.zeros((B * T, ldi), device="cuda")
    rs = torch.zeros((B * T, K), device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.score_coattn_fwd(P_(dt), Nr, D, F, K, B, T, P_(di1), P_(di2), P_(dtg), P_(dW), P_(db), P_(out1), ld1,
                                    P_(out2), Dx, P_(oinfo), ldi, P_(rs), 0, st), "coattn_fwd")
    torch.cuda.synchronize()

    def relerr(got, want):       # max abs error relative to the largest reference magnitude
        want = want.detach().numpy().reshape(got.shape)
        return float(np.abs(got.cpu().numpy() - want).max() / max(np.abs(want).max(), 1e-30))
    errs = (relerr(out1[:, :Dx], o1), relerr(out2, o2), relerr(oinfo[:, :2 * K], info))
    print("D %d F %d K %d B %d T %d: chunk length %d, relative errors %.2e %.2e %.2e"
          % ((D, F, K, B, T, fwd_chunk(D, K, B, T, F, 0)) + errs))
    assert max(errs) < 1e-5
    assert float(out1[:, Dx:].abs().max()) == 0 and float(oinfo[:, 2 * K:].abs().max()) == 0
    # rsave holds the relu'd scores r_i; atten_info's first K columns are K * r_i
    assert torch.equal(oinfo[:, :K], rs * float(K))
