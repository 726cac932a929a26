// What the fused head kernels share (head_fused.hip: build_fc_net and the temporal attention; deems.hip: DEEMS's two towers):
// the MFMA tile loop over an LDS-resident A operand, and the body of build_fc_net's backward kernel.
#pragma once
#include "common.h"
#include "kernels.h"

typedef float hf_f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int HF_ROWS = 16;     // samples per workgroup
constexpr int HF_NW = 8;        // waves per workgroup
constexpr int HF_CH = 16;       // MFMA steps per prefetched chunk of B operands

// acc[t] (16 x 16, rows lq*4+r, column lc) += xs[16][Kp] . W[K][ldw] columns [n0[t], n0[t]+16) for NT tiles at once.
// xs: LDS, row stride LD, zero beyond K up to Kp (Kp % 16 == 0, so KQ = Kp/4 is a multiple of 4).
// (The weight operand read from a transposed copy, one 16-B load per lane and four steps, measured slower -- 0.056 vs
// 0.051 ms for the stage: 16 lanes then touch 16 different rows per load instead of one 64-B run.)
template <int NT>
__device__ __forceinline__ void hf_tiles(hf_f32x4 (&acc)[NT], const float* __restrict__ xs, int LD, int Kp, int K,
                                         const float* __restrict__ W, int ldw, const int (&n0)[NT], int N, int lc, int lq) {
  const int KQ = Kp >> 2;
  const int kbase = lq * KQ;
  int col[NT];
  bool cok[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    cok[t] = n0[t] >= 0 && n0[t] + lc < N;
    col[t] = cok[t] ? n0[t] + lc : 0;
  }
  // B operands of two chunks in registers: chunk c+1 is requested before chunk c's MFMAs are issued
  float b0[NT][HF_CH], b1[NT][HF_CH];
  auto fetch = [&](float (&bb)[NT][HF_CH], int s0) {
#pragma unroll
    for (int i = 0; i < HF_CH; ++i) {
      const int k = kbase + s0 + i;
      const int kc = k < K ? k : K - 1;                 // clamped, unconditional loads; masked below
#pragma unroll
      for (int t = 0; t < NT; ++t) bb[t][i] = W[(int64_t)kc * ldw + col[t]];
    }
  };
  const float* xrow = xs + lc * LD + kbase;
  auto compute = [&](const float (&bb)[NT][HF_CH], int s0) {
    float4 av[HF_CH / 4];
#pragma unroll
    for (int q = 0; q < HF_CH / 4; ++q) {
      const int s = s0 + 4 * q;
      av[q] = s < KQ ? *reinterpret_cast<const float4*>(xrow + s) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < HF_CH; ++i) {
      const int k = kbase + s0 + i;
      const bool kok = (s0 + i < KQ) && k < K;
      const float a = (i & 3) == 0 ? av[i >> 2].x : (i & 3) == 1 ? av[i >> 2].y : (i & 3) == 2 ? av[i >> 2].z : av[i >> 2].w;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float b = (kok && cok[t]) ? bb[t][i] : 0.f;
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kok ? a : 0.f, b, acc[t], 0, 0, 0);
      }
    }
  };
  fetch(b0, 0);
  for (int s0 = 0; s0 < KQ; s0 += 2 * HF_CH) {
    fetch(b1, s0 + HF_CH);          // (addresses past the quarter are clamped and their products masked)
    compute(b0, s0);
    fetch(b0, s0 + 2 * HF_CH);
    if (s0 + HF_CH < KQ) compute(b1, s0 + HF_CH);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// build_fc_net backward (head_fused.hip describes it): the body of head_bwd_fused_kernel, for row tile blockIdx.x and share
// `by` of `ny` of d bn1's column tiles
constexpr int HB_K2Q = 20;      // fc2: K = FC2 = 80 -> k-steps per lane quarter
constexpr int HB_K1Q = 52;      // fc1: K = FC1 = 200 -> padded to 208

struct HeadBwdArgs {
  int B, Dh;
  int ld;       // row stride of x, dbn, dhead and tmp (Dh, or a wider row that holds this head's Dh columns: deems.hip)
  const float* dz2; const float* W2; const float* f1; float keep;
  const float* W1; const float* x; const float* gamma; float rs;
  float* dz1; float* dbn; float* dhead; float* tmp;
};

__device__ __forceinline__ void head_bwd_body(const HeadBwdArgs& a, const int by, const int ny) {
  constexpr int N1 = 4 * HB_K2Q * 0 + 200, N2 = 80, KP1 = 4 * HB_K1Q;     // FC1, FC2, FC1 padded
  constexpr int LD2 = N2 + 4, LD1 = KP1 + 4;
  __shared__ __attribute__((aligned(16))) float z2s[HF_ROWS * LD2];          // dz2 rows
  __shared__ __attribute__((aligned(16))) float z1s[HF_ROWS * LD1];          // dz1 rows, zero beyond FC1
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lc = lane & 15, lq = lane >> 4;
  const int b0 = blockIdx.x * HF_ROWS;
  for (int e = tid; e < HF_ROWS * (N2 / 4); e += 64 * HF_NW) {
    const int i = e / (N2 / 4), c = (e - i * (N2 / 4)) * 4;
    const int row = b0 + i < a.B ? b0 + i : a.B - 1;
    float4 v = ld4(a.dz2 + (int64_t)row * N2 + c);
    if (b0 + i >= a.B) v = make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(z2s + i * LD2 + c) = v;
  }
  for (int e = tid; e < HF_ROWS * (LD1 - N1); e += 64 * HF_NW) {
    const int i = e / (LD1 - N1), c = e - i * (LD1 - N1);
    z1s[i * LD1 + N1 + c] = 0.f;
  }
  // fc2 backward: tiles wave and wave + 8 of the 13; B[k][n] = W2[n][k]
  float b2[2][HB_K2Q];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int n = (wave + HF_NW * t) * 16 + lc;
    const float msk = n < N1 ? 1.0f : 0.0f;
    const float* wrow = a.W2 + (int64_t)(n < N1 ? n : N1 - 1) * N2 + lq * HB_K2Q;
#pragma unroll
    for (int s4 = 0; s4 < HB_K2Q; s4 += 4) {
      const float4 w = ld4(wrow + s4);
      b2[t][s4 + 0] = w.x * msk; b2[t][s4 + 1] = w.y * msk; b2[t][s4 + 2] = w.z * msk; b2[t][s4 + 3] = w.w * msk;
    }
  }
  __syncthreads();
  {
    float4 av[HB_K2Q / 4];
#pragma unroll
    for (int s4 = 0; s4 < HB_K2Q / 4; ++s4) av[s4] = *reinterpret_cast<const float4*>(z2s + lc * LD2 + lq * HB_K2Q + 4 * s4);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int n0 = (wave + HF_NW * t) * 16;
      if (n0 >= N1) continue;
      hf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s4 = 0; s4 < HB_K2Q / 4; ++s4) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s4].x, b2[t][4 * s4 + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s4].y, b2[t][4 * s4 + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s4].z, b2[t][4 * s4 + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s4].w, b2[t][4 * s4 + 3], acc, 0, 0, 0);
      }
      const int col = n0 + lc;
      if (col < N1) {
        // (the four mask values first, from clamped rows: a load behind `row < B` sits in its own exec-mask branch with a
        //  vmcnt(0) wait -- four dependent round trips per tile)
        float y[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] = a.f1[(int64_t)min(b0 + lq * 4 + r, a.B - 1) * N1 + col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = lq * 4 + r, row = b0 + i;
          const float q = acc[r] / a.keep;
          const float v = (row < a.B && y[r] > 0.f) ? q : 0.f;      // relu (+ dropout) of fc1, as the GEMM epilogue had it
          if (row < a.B && by == 0) a.dz1[(int64_t)row * N1 + col] = v;
          z1s[i * LD1 + col] = v;
        }
      }
    }
  }
  __syncthreads();
  // fc1 backward + bn1 backward: tiles wave, wave + 8, ... of ceil(Dh / 16); B[k][n] = W1[n][k], streamed one tile ahead
  // (ny workgroups share a row tile's column tiles -- each has computed dz1 for itself: at 1024 samples the 64 row
  //  tiles alone left three quarters of the chip idle for 27 us of the launch stream; four shares: the same sums, 15 us)
  const int nt_all = (a.Dh + 15) >> 4;
  const int per = (nt_all + ny - 1) / ny;
  const int t0 = by * per, nt = min(nt_all, t0 + per);
  float4 av[HB_K1Q / 4];
#pragma unroll
  for (int s4 = 0; s4 < HB_K1Q / 4; ++s4) av[s4] = *reinterpret_cast<const float4*>(z1s + lc * LD1 + lq * HB_K1Q + 4 * s4);
  float4 bw[2][HB_K1Q / 4];
  auto fetch = [&](float4 (&dst)[HB_K1Q / 4], int tile) {
    const int n = tile * 16 + lc;
    const float* wrow = a.W1 + (int64_t)(n < a.Dh ? n : a.Dh - 1) * N1 + lq * HB_K1Q;
#pragma unroll
    for (int s4 = 0; s4 < HB_K1Q / 4; ++s4) {
      // (the last quarter's k range runs past FC1 = 200 into the next row: those products meet the zero padding of z1s)
      const int k = lq * HB_K1Q + 4 * s4;
      dst[s4] = ld4(k + 3 < N1 ? wrow + 4 * s4 : a.W1);
    }
  };
  if (t0 + wave < nt) fetch(bw[0], t0 + wave);
  int cur = 0;
  for (int tile = t0 + wave; tile < nt; tile += HF_NW, cur ^= 1) {
    if (tile + HF_NW < nt) {
      if (cur == 0) fetch(bw[1], tile + HF_NW); else fetch(bw[0], tile + HF_NW);
    }
    hf_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int col = tile * 16 + lc;
    const float cm = col < a.Dh ? 1.0f : 0.0f;
#pragma unroll
    for (int s4 = 0; s4 < HB_K1Q / 4; ++s4) {
      const float4 w = cur == 0 ? bw[0][s4] : bw[1][s4];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s4].x, w.x * cm, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s4].y, w.y * cm, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s4].z, w.z * cm, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s4].w, w.w * cm, acc, 0, 0, 0);
    }
    {
      const int cc = col < a.Dh ? col : a.Dh - 1;
      const float gs = a.gamma[cc] * a.rs;
      float xv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) xv[r] = a.x[(int64_t)min(b0 + lq * 4 + r, a.B - 1) * a.ld + cc];     // clamped, unconditional
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = b0 + lq * 4 + r;
        if (row < a.B && col < a.Dh) {
          const int64_t e = (int64_t)row * a.ld + col;
          const float dy = acc[r];
          a.dbn[e] = dy;
          a.dhead[e] = dy * gs;
          a.tmp[e] = dy * (xv[r] * a.rs);
        }
      }
    }
  }
}

}  // namespace
