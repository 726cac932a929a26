// GRU4Rec's two GRUs stacked in depth (point_model.py:129-132: o1 = gru1(x), h2 = gru2(o1)) as ONE persistent kernel each
// way, H in {16, 32, 64}, in the style of the register-resident recurrences of gru.hip.
//
// A workgroup = 8 waves owns 16 batch rows: waves 0-3 work for layer 1, waves 4-7 for layer 2 (wave-uniform; the barriers are
// shared).  The layers are skewed by one step: in forward iteration s = 0 .. T layer 1 computes its step s and layer 2 its step
// s - 1.  Both read the same LDS rows h1[s-1] -- layer 1 as its recurrent operand, layer 2 as its INPUT, against the x rows of
// the whole gru2 kernels ([x, h] row order) -- so layer 2 has no hoisted projection: no [B*T, 3H] buffer, no GEMM to fill it, no
// launch boundary between the layers.  Layer 1's state is double-buffered (its candidate epilogue writes h1[s] while layer 2's
// candidate phase still reads h1[s-1]).  What layer 2 reads is the CARRIED state, which differs from o1 (zero) only past the
// sample's length, where layer 2 copies its own state through and discards what it computed.
// Backward, mirrored: iteration s = T-1 .. -1, layer 2 does step s, layer 1 step s + 1; layer 2's pre-activation gradients
// against the x rows of its kernels give layer 1's dout[s], handed over in LDS.
// Every wave keeps the B operands (v_mfma_f32_16x16x4_f32) of its output tiles in registers for the whole loop; rows past the
// batch duplicate the last sample (same values to the same addresses), so the loops hold no predicated memory operation.
#include <string.h>
#include "common.h"
#include "kernels.h"
#include "cell.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define SRB 16      // batch rows per workgroup
#define SNW 4       // waves per layer
#define ST_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ float st_elem(const float4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// acc[tt] += A[16 x KN] . w[tt]: K is dealt to the four lane quarters in contiguous runs of KN / 4 (quarter lq owns
// k in [lq * KN/4, (lq+1) * KN/4)), so a lane reads its A operands of four MFMA steps with one 16-byte LDS read.
// w[tt][w0 + ks] is the B operand of step ks.
template <int KN, int TW, int WN>
__device__ __forceinline__ void st_chain(const float* A, int lda, const float (&w)[TW][WN], int w0, f32x4 (&acc)[TW], int lc, int lq) {
  constexpr int KQ = KN / 4;
  float4 av4[KQ / 4];
#pragma unroll
  for (int q = 0; q < KQ / 4; ++q) av4[q] = *reinterpret_cast<const float4*>(&A[lc * lda + lq * KQ + 4 * q]);
#pragma unroll
  for (int ks = 0; ks < KQ; ++ks) {
    const float av = st_elem(av4[ks >> 2], ks & 3);
#pragma unroll
    for (int tt = 0; tt < TW; ++tt) acc[tt] = ST_MFMA(av, w[tt][w0 + ks], acc[tt]);
  }
}
// two independent chains interleaved (their MFMAs alternate: a dependent f32 MFMA waits 40 cycles, an independent one 32)
template <int KN, int TW, int WN>
__device__ __forceinline__ void st_chain2(const float* A0, const float* A1, int lda, const float (&w)[TW][WN], f32x4 (&acc)[TW],
                                          int lc, int lq) {
  constexpr int KQ = KN / 4;
  float4 a0[KQ / 4], a1[KQ / 4];
#pragma unroll
  for (int q = 0; q < KQ / 4; ++q) {
    a0[q] = *reinterpret_cast<const float4*>(&A0[lc * lda + lq * KQ + 4 * q]);
    a1[q] = *reinterpret_cast<const float4*>(&A1[lc * lda + lq * KQ + 4 * q]);
  }
  f32x4 acc1[TW];
#pragma unroll
  for (int tt = 0; tt < TW; ++tt) acc1[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < KQ; ++ks) {
    const float v0 = st_elem(a0[ks >> 2], ks & 3), v1 = st_elem(a1[ks >> 2], ks & 3);
#pragma unroll
    for (int tt = 0; tt < TW; ++tt) {
      acc[tt] = ST_MFMA(v0, w[tt][ks], acc[tt]);
      acc1[tt] = ST_MFMA(v1, w[tt][KQ + ks], acc1[tt]);
    }
  }
#pragma unroll
  for (int tt = 0; tt < TW; ++tt) acc[tt] += acc1[tt];
}

template <int H>
__global__ __launch_bounds__(128 * SNW) void gru_stack_fwd_kernel(const GruStackArgs a) {
  constexpr int KS = H / 4;                 // k-steps of 4 over K = H
  constexpr int NTG = 2 * H / 16, NTC = H / 16;
  constexpr int TGW = (NTG + SNW - 1) / SNW, TCW = (NTC + SNW - 1) / SNW;
  constexpr int LD = H + 4;                 // row stride: 16-B aligned, the 16 rows of a read land on 64 banks
  __shared__ float h1s[2][SRB * LD], h2s[SRB * LD], rhs[2][SRB * LD], us[2][SRB * LD];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int layer = wave / SNW;
  // the tiles a wave owns: (tw + SNW * tt).  Layer 2 counts its waves from the top, so that where a phase has fewer tiles than
  // waves (the candidate at H = 32, everything at H = 16) the two layers' MFMA chains sit on different SIMDs
  const int tw = layer ? SNW - 1 - (wave % SNW) : wave % SNW;
  const GruSide& sd = a.l[layer];
  const int b0 = blockIdx.x * SRB;
  const int lc = lane & 15, lq = lane >> 4;  // column inside a tile / k-quarter == output row group
  const int T = a.T;

  // B operands.  Layer 1: [0, KS) the h rows of its kernels.  Layer 2: [0, KS) the x rows, [KS, 2 KS) the h rows of the whole kernels
  float wg[TGW][2 * KS], wc[TCW][2 * KS];
#pragma unroll
  for (int tt = 0; tt < TGW; ++tt) {
    const int tile = tw + SNW * tt, col = tile * 16 + lc;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = lq * KS + ks;
      if (layer == 0) {
        wg[tt][ks] = tile < NTG ? sd.Wg[(int64_t)k * sd.ldwg + col] : 0.f;
        wg[tt][KS + ks] = 0.f;
      } else {
        wg[tt][ks] = tile < NTG ? a.Wg2[(int64_t)k * 2 * H + col] : 0.f;
        wg[tt][KS + ks] = tile < NTG ? a.Wg2[(int64_t)(H + k) * 2 * H + col] : 0.f;
      }
    }
  }
#pragma unroll
  for (int tt = 0; tt < TCW; ++tt) {
    const int tile = tw + SNW * tt, col = tile * 16 + lc;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = lq * KS + ks;
      if (layer == 0) {
        wc[tt][ks] = tile < NTC ? sd.Wc[(int64_t)k * sd.ldwc + col] : 0.f;
        wc[tt][KS + ks] = 0.f;
      } else {
        wc[tt][ks] = tile < NTC ? a.Wc2[(int64_t)k * H + col] : 0.f;
        wc[tt][KS + ks] = tile < NTC ? a.Wc2[(int64_t)(H + k) * H + col] : 0.f;
      }
    }
  }
  int len[4];
  int64_t rowb[4];                // row of (sample, t = 0)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int bc = min(b0 + lq * 4 + r, a.B - 1);
    len[r] = a.length[bc];
    rowb[r] = (int64_t)bc * T;
  }
  for (int e = tid; e < SRB * LD; e += 128 * SNW) { h1s[0][e] = 0.f; h1s[1][e] = 0.f; h2s[e] = 0.f; }

  // what is added to the products: layer 1's hoisted x-projection rows, read about one step ahead (clamped addresses, each half
  // fetched again right after its last use); layer 2's biases, constant
  float xg[TGW][4], xc[TCW][4];
  auto fetch_xg = [&](int t) {
    const int tc = min(t, T - 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* xr = sd.xproj + (rowb[r] + tc) * 3 * H;
#pragma unroll
      for (int tt = 0; tt < TGW; ++tt) xg[tt][r] = xr[min(tw + SNW * tt, NTG - 1) * 16 + lc];
    }
  };
  auto fetch_xc = [&](int t) {
    const int tc = min(t, T - 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* xr = sd.xproj + (rowb[r] + tc) * 3 * H;
#pragma unroll
      for (int tt = 0; tt < TCW; ++tt) xc[tt][r] = xr[2 * H + min(tw + SNW * tt, NTC - 1) * 16 + lc];
    }
  };
  if (layer == 0) {
    fetch_xg(0); fetch_xc(0);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int tt = 0; tt < TGW; ++tt) xg[tt][r] = a.bg2[min(tw + SNW * tt, NTG - 1) * 16 + lc];
#pragma unroll
      for (int tt = 0; tt < TCW; ++tt) xc[tt][r] = a.bc2[min(tw + SNW * tt, NTC - 1) * 16 + lc];
    }
  }
  __syncthreads();

  float* const rh = rhs[layer];
  float* const uu = us[layer];
  for (int s = 0; s <= T; ++s) {
    const int t = layer ? s - 1 : s;                  // this layer's step
    const bool on = layer ? s >= 1 : s < T;           // (wave-uniform)
    const float* h1 = h1s[s & 1];                     // h1[s-1]: layer 1's state, layer 2's input
    const float* hrd = layer ? h2s : h1;              // this layer's own state ...
    float* hwr = layer ? h2s : h1s[(s & 1) ^ 1];      // ... and where its next one goes
    if (on) {
      // gates = sigmoid(x . Wx + b + h . Wh)
      f32x4 acc[TGW];
#pragma unroll
      for (int tt = 0; tt < TGW; ++tt) acc[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (layer == 0) st_chain<H, TGW, 2 * KS>(h1, LD, wg, 0, acc, lc, lq);
      else st_chain2<H, TGW, 2 * KS>(h1, h2s, LD, wg, acc, lc, lq);
#pragma unroll
      for (int tt = 0; tt < TGW; ++tt) {
        const int tile = tw + SNW * tt;
        if (tile >= NTG) continue;
        const int j = tile * 16 + lc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = lq * 4 + r;
          const float g = gru_sigmoid(acc[tt][r] + xg[tt][r]);
          sd.gates[(rowb[r] + t) * 3 * H + j] = g;
          if (j < H) rh[i * LD + j] = g * hrd[i * LD + j];
          else uu[i * LD + (j - H)] = g;
        }
      }
      if (layer == 0) {
        __builtin_amdgcn_sched_barrier(0);
        fetch_xg(t + 1);
      }
    }
    __syncthreads();
    if (on) {
      // c = tanh(x . Wx + b + (r*h) . Wh) ; h' = u*h + (1-u)*c
      f32x4 acc[TCW];
#pragma unroll
      for (int tt = 0; tt < TCW; ++tt) acc[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (layer == 0) st_chain<H, TCW, 2 * KS>(rh, LD, wc, 0, acc, lc, lq);
      else st_chain2<H, TCW, 2 * KS>(h1, rh, LD, wc, acc, lc, lq);
#pragma unroll
      for (int tt = 0; tt < TCW; ++tt) {
        const int tile = tw + SNW * tt;
        if (tile >= NTC) continue;
        const int j = tile * 16 + lc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = lq * 4 + r;
          const float c = gru_tanh(acc[tt][r] + xc[tt][r]);
          const float u = uu[i * LD + j], h = hrd[i * LD + j];
          const float hn = gru_blend(u, h, c);
          const bool live = t < len[r];
          const int64_t row = rowb[r] + t;
          sd.gates[row * 3 * H + 2 * H + j] = c;
          sd.out[row * sd.ldo + j] = live ? hn : 0.f;      // dynamic_rnn: zero output past the length ...
          hwr[i * LD + j] = live ? hn : h;                 // ... and the state is carried through
        }
      }
      if (layer == 0) {
        __builtin_amdgcn_sched_barrier(0);
        fetch_xc(t + 1);
      }
    }
    __syncthreads();
  }
  if (layer == 1 && sd.final_state)
    for (int e = tid - 64 * SNW; e < SRB * H; e += 64 * SNW) {
      const int i = e / H, j = e - i * H;
      if (b0 + i < a.B) sd.final_state[(int64_t)(b0 + i) * H + j] = h2s[i * LD + j];
    }
}

template <int H>
__global__ __launch_bounds__(128 * SNW) void gru_stack_bwd_kernel(const GruStackArgs a) {
  constexpr int KS = H / 4;
  constexpr int NT = H / 16;
  constexpr int TW = (NT + SNW - 1) / SNW;
  constexpr int LD = H + 4, LD2 = 2 * H + 4;
  // per layer: dh (gradient of the carried state), dpc (candidate pre-activation gradient), dpg = [dpr | dpu]; d1: layer 2's input
  // gradient of the step it has just done = layer 1's dout of the step it does next
  __shared__ float dhs[2][SRB * LD], dpcs[2][SRB * LD], dpgs[2][SRB * LD2], d1[SRB * LD];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int layer = wave / SNW;
  const int tw = layer ? SNW - 1 - (wave % SNW) : wave % SNW;      // (as in the forward)
  const GruSide& sd = a.l[layer];
  const int b0 = blockIdx.x * SRB;
  const int lc = lane & 15, lq = lane >> 4;
  const int T = a.T;
  float* const dh = dhs[layer];
  float* const dpc = dpcs[layer];
  float* const dpg = dpgs[layer];

  // B operands of the transposed products, B[k][j] = W[j][k].  Both layers: wct (K = H) and wgt (K = 2H) over the h rows of the
  // candidate / gates kernels -> d(r*h), dh_prev.  Layer 2 also: wxc, wxg over the x rows -> its input gradient
  float wct[TW][KS], wgt[TW][2 * KS], wxc[TW][KS], wxg[TW][2 * KS];
#pragma unroll
  for (int tt = 0; tt < TW; ++tt) {
    const int tile = tw + SNW * tt, j = tile * 16 + lc;
    const bool ok = tile < NT;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int k = lq * KS + ks;
      wct[tt][ks] = !ok ? 0.f : layer ? a.Wc2[(int64_t)(H + j) * H + k] : sd.Wc[(int64_t)j * sd.ldwc + k];
      wxc[tt][ks] = ok && layer ? a.Wc2[(int64_t)j * H + k] : 0.f;
    }
#pragma unroll
    for (int ks = 0; ks < 2 * KS; ++ks) {
      const int k = lq * 2 * KS + ks;
      wgt[tt][ks] = !ok ? 0.f : layer ? a.Wg2[(int64_t)(H + j) * 2 * H + k] : sd.Wg[(int64_t)j * sd.ldwg + k];
      wxg[tt][ks] = ok && layer ? a.Wg2[(int64_t)j * 2 * H + k] : 0.f;
    }
  }
  // every thread owns the elements (row i = lq*4 + r, column j = (tw + SNW*tt)*16 + lc) in all three phases
  int len[4], bcs[4];
  int64_t rowb[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    bcs[r] = min(b0 + lq * 4 + r, a.B - 1);
    len[r] = a.length[bcs[r]];
    rowb[r] = (int64_t)bcs[r] * T;
  }
#pragma unroll
  for (int tt = 0; tt < TW; ++tt) {
    const int tile = tw + SNW * tt;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = lq * 4 + r, j = tile * 16 + lc;
      if (tile < NT) dh[i * LD + j] = sd.dfinal ? sd.dfinal[(int64_t)bcs[r] * H + j] : 0.f;
    }
  }
  for (int e = tid; e < SRB * LD; e += 128 * SNW) d1[e] = 0.f;
  // saved activations, read unconditionally (clamped addresses) about one step ahead, each fetched again right after its last use
  float n_u[TW][4], n_c[TW][4], n_r[TW][4], n_hp[TW][4];
  auto fetch_uc = [&](int t) {
    const int tc = max(t, 0);
#pragma unroll
    for (int tt = 0; tt < TW; ++tt) {
      const int j = min(tw + SNW * tt, NT - 1) * 16 + lc;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = rowb[r] + tc;
        n_u[tt][r] = sd.gates[row * 3 * H + H + j];
        n_c[tt][r] = sd.gates[row * 3 * H + 2 * H + j];
      }
    }
  };
  auto fetch_r = [&](int t) {
    const int tc = max(t, 0);
#pragma unroll
    for (int tt = 0; tt < TW; ++tt) {
      const int j = min(tw + SNW * tt, NT - 1) * 16 + lc;
#pragma unroll
      for (int r = 0; r < 4; ++r) n_r[tt][r] = sd.gates[(rowb[r] + tc) * 3 * H + j];
    }
  };
  auto fetch_hp = [&](int t) {
    const int tp = max(t - 1, 0);          // (h_prev of t = 0 is never used)
#pragma unroll
    for (int tt = 0; tt < TW; ++tt) {
      const int j = min(tw + SNW * tt, NT - 1) * 16 + lc;
#pragma unroll
      for (int r = 0; r < 4; ++r) n_hp[tt][r] = sd.out[(rowb[r] + tp) * sd.ldo + j];
    }
  };
  fetch_uc(T - 1); fetch_r(T - 1); fetch_hp(T - 1);
  __syncthreads();

  for (int s = T - 1; s >= -1; --s) {
    const int t = layer ? s : s + 1;                  // this layer's step
    const bool on = layer ? s >= 0 : s <= T - 2;      // (wave-uniform)
    float c_hp[TW][4];                                // h_{t-1}, 0 past the length and at t = 0
    if (on) {
#pragma unroll
      for (int tt = 0; tt < TW; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) c_hp[tt][r] = (t < len[r] && t > 0) ? n_hp[tt][r] : 0.f;
      __builtin_amdgcn_sched_barrier(0);
      fetch_hp(t - 1);
      // phase 1 (elementwise): dpu, dpc ; dh <- dh_tot * u      (selects, no branches)
#pragma unroll
      for (int tt = 0; tt < TW; ++tt) {
        const int tile = tw + SNW * tt;
        if (tile >= NT) continue;
        const int j = tile * 16 + lc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = lq * 4 + r;
          const bool live = t < len[r];
          const float u = n_u[tt][r], c = n_c[tt][r];      // (a dead step's results are discarded by `live`)
          const float dold = dh[i * LD + j];
          // dL/d out[t]: layer 1's comes from layer 2's step t (zero past the length); nothing but the final state reads layer 2's
          const float d = layer ? dold : dold + d1[i * LD + j];
          // cell.h's gru_du / gru_dc / gru_dpu / gru_dpc, spelled out: through the helpers the compiler allocates the H = 32
          // kernel's address registers differently, and it is kept byte for byte as it was measured
          const float du = d * (c_hp[tt][r] - c), dc = d * (1.0f - u);
          const float v_dpu = live ? du * u * (1.0f - u) : 0.f;
          const float v_dpc = live ? dc * (1.0f - c * c) : 0.f;
          dh[i * LD + j] = live ? d * u : dold;
          const int64_t row = rowb[r] + t;
          sd.hprev[row * H + j] = c_hp[tt][r];
          sd.dxproj[row * 3 * H + H + j] = v_dpu;
          sd.dxproj[row * 3 * H + 2 * H + j] = v_dpc;
          dpc[i * LD + j] = v_dpc;
          dpg[i * LD2 + H + j] = v_dpu;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      fetch_uc(t - 1);
    }
    __syncthreads();
    if (on) {
      // phase 2: d(rh) = dpc . Wc_h^T ; dpr = d(rh)*h_prev*r(1-r) ; dh += d(rh)*r
      f32x4 acc[TW];
#pragma unroll
      for (int tt = 0; tt < TW; ++tt) acc[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      st_chain<H, TW, KS>(dpc, LD, wct, 0, acc, lc, lq);
#pragma unroll
      for (int tt = 0; tt < TW; ++tt) {
        const int tile = tw + SNW * tt;
        if (tile >= NT) continue;
        const int j = tile * 16 + lc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = lq * 4 + r;
          const bool live = t < len[r];
          const float rr = live ? n_r[tt][r] : 0.f, hp = c_hp[tt][r];   // both 0 past the length
          const float drh = acc[tt][r];
          const float v_dpr = gru_dpr(drh, hp, rr, live);
          dh[i * LD + j] += live ? drh * rr : 0.f;
          const int64_t row = rowb[r] + t;
          sd.dxproj[row * 3 * H + j] = v_dpr;
          sd.rh[row * H + j] = rr * hp;
          dpg[i * LD2 + j] = v_dpr;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      fetch_r(t - 1);
    }
    __syncthreads();
    if (on) {
      // phase 3: dh += [dpr | dpu] . Wg_h^T ; layer 2: dx = [dpr | dpu] . Wg_x^T + dpc . Wc_x^T -> layer 1's dout of this step
      f32x4 acc[TW];
#pragma unroll
      for (int tt = 0; tt < TW; ++tt) acc[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (layer == 0) {
        st_chain<2 * H, TW, 2 * KS>(dpg, LD2, wgt, 0, acc, lc, lq);
      } else {
        f32x4 ax[TW], ac[TW];
#pragma unroll
        for (int tt = 0; tt < TW; ++tt) { ax[tt] = (f32x4){0.f, 0.f, 0.f, 0.f}; ac[tt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
        // (three independent chains: their MFMAs interleave)
        constexpr int KQ = 2 * KS;
        float4 av4[KQ / 4], cv4[KS / 4];
#pragma unroll
        for (int q = 0; q < KQ / 4; ++q) av4[q] = *reinterpret_cast<const float4*>(&dpg[lc * LD2 + lq * KQ + 4 * q]);
#pragma unroll
        for (int q = 0; q < KS / 4; ++q) cv4[q] = *reinterpret_cast<const float4*>(&dpc[lc * LD + lq * KS + 4 * q]);
#pragma unroll
        for (int ks = 0; ks < KQ; ++ks) {
          const float av = st_elem(av4[ks >> 2], ks & 3);
#pragma unroll
          for (int tt = 0; tt < TW; ++tt) {
            acc[tt] = ST_MFMA(av, wgt[tt][ks], acc[tt]);
            ax[tt] = ST_MFMA(av, wxg[tt][ks], ax[tt]);
          }
          if (ks < KS) {
            const float cv = st_elem(cv4[ks >> 2], ks & 3);
#pragma unroll
            for (int tt = 0; tt < TW; ++tt) ac[tt] = ST_MFMA(cv, wxc[tt][ks], ac[tt]);
          }
        }
#pragma unroll
        for (int tt = 0; tt < TW; ++tt) {
          const int tile = tw + SNW * tt;
          if (tile >= NT) continue;
          const int j = tile * 16 + lc;
#pragma unroll
          for (int r = 0; r < 4; ++r) d1[(lq * 4 + r) * LD + j] = ax[tt][r] + ac[tt][r];
        }
      }
#pragma unroll
      for (int tt = 0; tt < TW; ++tt) {
        const int tile = tw + SNW * tt;
        if (tile >= NT) continue;
        const int j = tile * 16 + lc;
#pragma unroll
        for (int r = 0; r < 4; ++r) dh[(lq * 4 + r) * LD + j] += acc[tt][r];
      }
    }
    __syncthreads();
  }
}

}  // namespace

bool score_gru_stack_ok(int H) { return H == 16 || H == 32 || H == 64; }

int score_gru_stack_fwd(GruStackArgs& a, hipStream_t s) {
  if (!score_gru_stack_ok(a.H) || a.B <= 0 || a.T <= 0) return SCORE_E_SHAPE;
  if (!a.l[0].xproj || !a.l[0].Wg || !a.l[0].Wc || !a.Wg2 || !a.Wc2 || !a.bg2 || !a.bc2 || !a.length || !a.l[0].out ||
      !a.l[0].gates || !a.l[1].out || !a.l[1].gates)
    return SCORE_E_BADARG;
  dim3 grid((a.B + SRB - 1) / SRB);
#define LF(Hv) hipLaunchKernelGGL((gru_stack_fwd_kernel<Hv>), grid, dim3(128 * SNW), 0, s, a)
  if (a.H == 16) LF(16);
  else if (a.H == 32) LF(32);
  else LF(64);
#undef LF
  SCORE_CHECK_LAUNCH();
  return 0;
}

int score_gru_stack_bwd(GruStackArgs& a, hipStream_t s) {
  if (!score_gru_stack_ok(a.H) || a.B <= 0 || a.T <= 0) return SCORE_E_SHAPE;
  for (int l = 0; l < 2; ++l)
    if (!a.l[l].out || !a.l[l].gates || !a.l[l].dxproj || !a.l[l].rh || !a.l[l].hprev) return SCORE_E_BADARG;
  if (!a.l[0].Wg || !a.l[0].Wc || !a.Wg2 || !a.Wc2 || !a.length || !a.l[1].dfinal) return SCORE_E_BADARG;
  a.l[0].dfinal = nullptr;        // (nothing reads layer 1's final state)
  dim3 grid((a.B + SRB - 1) / SRB);
#define LB(Hv) hipLaunchKernelGGL((gru_stack_bwd_kernel<Hv>), grid, dim3(128 * SNW), 0, s, a)
  if (a.H == 16) LB(16);
  else if (a.H == 32) LB(32);
  else LB(64);
#undef LB
  SCORE_CHECK_LAUNCH();
  return 0;
}
