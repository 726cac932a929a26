// The two one-filter convolutions of the Caser point baseline (point_models/point_model.py:147-160) over the gathered user
// history X [B, T, C] (C = item_fnum * eb_dim; rows of stride ldx in the gather's output), forward and backward:
//   hwin[b, p] = sum_{i < 50, c < C} X[b, p + i, c] Wh[i, c] + bh,  p = 0 .. T - 50      (conv2d: [50, C], VALID)
//   h[b]       = max_p hwin[b, p]                                                        (the max-pool over every position)
//   v[b, c]    = sum_t X[b, t, c] Wv[t] + bv                                             (conv2d_1: [T, 1])
//   v2[b, c]   = v[b, c] wd + bd                                                         (dense on a trailing axis of size 1)
// and the head input row [h, 0, 0, 0 | v2]: h padded to one 16-byte group (engine.hip make_dims), the pads written on every pass.
//
// Forward: a workgroup of 256 threads per sample, as R = 256 / CW row groups of CW lanes, CW the power of two that covers C
// (4 .. 256; wider C loops over column blocks).  Lane l of row group r owns the elements (t, c) with t = r (mod R), c = l (mod
// CW): one sweep over X[b] gives its share of v[c] and of up to CASER_PW window sums, held in registers; v is summed over the
// row groups in row-group order, the window sums over the 256 threads by a fixed tree.  T <= 57 (the reference runs T = 50:
// one window) is ONE sweep, X[b] read once; a longer history takes one more sweep per eight windows over the 57 rows those
// windows cover.  Backward: d X is pointwise (caser_dx_kernel); the six variables' gradients are sums over the batch, taken by
// caser_params_kernel in a fixed order -- per output a fixed split of the samples over eight partial sums, then those in order;
// no atomics -- so a run repeats bit for bit.
#include <math.h>
#include "common.h"
#include "kernels.h"

#define CASER_NT 256
#define CASER_PW 8        // window sums per sweep
#define CASER_L SCORE_CASER_L
#define CASER_HPAD SCORE_CASER_HPAD

// s_red[j * 256 + tid], j < nj: summed over tid into s_red[j * 256] by a fixed tree (every thread of the workgroup calls this)
__device__ __forceinline__ void caser_tree_sum(float* s_red, int nj, int tid) {
  __syncthreads();
  for (int st = CASER_NT / 2; st > 0; st >>= 1) {
    if (tid < st)
      for (int j = 0; j < nj; ++j) s_red[j * CASER_NT + tid] += s_red[j * CASER_NT + tid + st];
    __syncthreads();
  }
}

__global__ __launch_bounds__(CASER_NT) void caser_fwd_kernel(const CaserArgs a, int CW) {
  __shared__ float s_red[CASER_PW * CASER_NT];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = a.T, C = a.C, NW = T - CASER_L + 1;
  const int R = CASER_NT / CW, r = tid / CW, l = tid - r * CW;
  const float* __restrict__ X = a.X + (int64_t)b * T * a.ldx;
  const float* __restrict__ Wh = a.Wh;
  const float* __restrict__ Wv = a.Wv;
  float* head = a.head + (int64_t)b * a.ldh;
  float best = 0.f;
  int arg = 0;
  for (int p0 = 0; p0 < NW; p0 += CASER_PW) {
    const int nj = min(CASER_PW, NW - p0);
    // the rows this sweep's windows read; the first sweep takes every row (v needs them all, and its windows' rows are among them)
    const int lo = p0, hi = p0 == 0 ? T : min(T, p0 + CASER_PW - 1 + CASER_L);
    float acc[CASER_PW];
#pragma unroll
    for (int j = 0; j < CASER_PW; ++j) acc[j] = 0.f;
    for (int c0 = 0; c0 < C; c0 += CW) {
      const int c = c0 + l;
      float vacc = 0.f;
      if (c < C) {
        for (int t = lo + r; t < hi; t += R) {
          const float x = X[(int64_t)t * a.ldx + c];
          if (p0 == 0) vacc = fmaf(x, Wv[t], vacc);
#pragma unroll
          for (int j = 0; j < CASER_PW; ++j) {
            const int i = t - p0 - j;       // row of the filter that window p0 + j puts on row t
            if (j < nj && i >= 0 && i < CASER_L) acc[j] = fmaf(x, Wh[i * C + c], acc[j]);
          }
        }
      }
      if (p0 == 0) {      // v[c] and v2[c]: the row groups' shares, in row-group order
        s_red[tid] = vacc;
        __syncthreads();
        if (r == 0 && c < C) {
          float v = 0.f;
          for (int q = 0; q < R; ++q) v += s_red[q * CW + l];
          v += a.bv[0];
          a.v[(int64_t)b * C + c] = v;
          head[CASER_HPAD + c] = fmaf(v, a.wd[0], a.bd[0]);
        }
        __syncthreads();
      }
    }
#pragma unroll
    for (int j = 0; j < CASER_PW; ++j) s_red[j * CASER_NT + tid] = acc[j];
    caser_tree_sum(s_red, nj, tid);
    if (tid == 0) {
      for (int j = 0; j < nj; ++j) {
        const float hw = s_red[j * CASER_NT] + a.bh[0];
        a.hwin[(int64_t)b * NW + p0 + j] = hw;
        // the maximum and its position; on a tie the FIRST position keeps it (strictly greater only): the backward pass sends
        // h's gradient to that window alone, as TF's max-pool gradient does
        if (p0 + j == 0 || hw > best) { best = hw; arg = p0 + j; }
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    head[0] = best;
    head[1] = 0.f; head[2] = 0.f; head[3] = 0.f;      // the pad columns: every pass (the workspace is reused under other layouts)
    a.arg[b] = arg;
  }
}

// the position the forward pass chose, kept inside [0, T - 50] whatever the workspace holds
__device__ __forceinline__ int caser_arg(const CaserArgs& a, int b) {
  const int p = a.arg[b];
  return min(max(p, 0), a.T - CASER_L);
}

// d X[b, t, c] = dv2[b, c] wd Wv[t] + (0 <= t - arg[b] < 50 ? dh[b] Wh[t - arg[b], c] : 0), four columns per thread; the
// columns past C of the ldx-wide row (the part of the gather's output that this model does not read) get zeros
__global__ __launch_bounds__(CASER_NT) void caser_dx_kernel(const CaserArgs a) {
  const int ld4 = a.ldx >> 2;
  const int64_t e = (int64_t)blockIdx.x * CASER_NT + threadIdx.x;
  if (e >= (int64_t)a.B * a.T * ld4) return;
  const int64_t row = e / ld4;
  const int c = (int)(e - row * ld4) << 2;
  const int b = (int)(row / a.T), t = (int)(row - (int64_t)b * a.T);
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < a.C) {
    const float* dh_row = a.dhead + (int64_t)b * a.ldh;
    const float4 dv2 = *reinterpret_cast<const float4*>(dh_row + CASER_HPAD + c);
    const float s = a.wd[0] * a.Wv[t];
    o = make_float4(dv2.x * s, dv2.y * s, dv2.z * s, dv2.w * s);
    const int i = t - caser_arg(a, b);
    if (i >= 0 && i < CASER_L) {
      const float dh = dh_row[0];
      const float4 w = *reinterpret_cast<const float4*>(a.Wh + (int64_t)i * a.C + c);
      o.x = fmaf(dh, w.x, o.x); o.y = fmaf(dh, w.y, o.y); o.z = fmaf(dh, w.z, o.z); o.w = fmaf(dh, w.w, o.w);
    }
  }
  *reinterpret_cast<float4*>(a.dX + row * a.ldx + c) = o;
}

// The variables' gradients.  Workgroups [0, nwh): 32 elements of d Wh[i, c] = sum_b dh[b] X[b, arg[b] + i, c] each, thread
// (q, lane) summing the samples b = q (mod 8) in rising order, then the eight shares in order q.  Workgroups [nwh, nwh + T):
// d Wv[t] = wd sum_{b, c} dv2[b, c] X[b, t, c], thread tid summing the elements tid (mod 256) of the [B, C] plane in rising
// order, then the fixed tree.  The last workgroup: d bd = sum dv2, d wd = sum dv2 v, d bv = wd sum dv2, d bh = sum_b dh.
__global__ __launch_bounds__(CASER_NT) void caser_params_kernel(const CaserArgs a, int nwh) {
  __shared__ float s_red[3 * CASER_NT];
  const int tid = threadIdx.x, blk = blockIdx.x;
  const int B = a.B, T = a.T, C = a.C;
  if (blk < nwh) {
    const int q = tid >> 5, o = blk * 32 + (tid & 31);
    float acc = 0.f;
    if (o < CASER_L * C) {
      const int i = o / C, c = o - i * C;
      for (int b = q; b < B; b += 8)
        acc = fmaf(a.dhead[(int64_t)b * a.ldh], a.X[((int64_t)b * T + caser_arg(a, b) + i) * a.ldx + c], acc);
    }
    s_red[tid] = acc;
    __syncthreads();
    if (tid < 32 && o < CASER_L * C) {
      float g = 0.f;
      for (int k = 0; k < 8; ++k) g += s_red[k * 32 + tid];
      a.gWh[o] = g;
    }
    return;
  }
  const int64_t n = (int64_t)B * C;
  if (blk < nwh + T) {
    const int t = blk - nwh;
    float acc = 0.f;
    for (int64_t e = tid; e < n; e += CASER_NT) {
      const int b = (int)(e / C), c = (int)(e - (int64_t)b * C);
      acc = fmaf(a.dhead[(int64_t)b * a.ldh + CASER_HPAD + c], a.X[((int64_t)b * T + t) * a.ldx + c], acc);
    }
    s_red[tid] = acc;
    caser_tree_sum(s_red, 1, tid);
    if (tid == 0) a.gWv[t] = a.wd[0] * s_red[0];
    return;
  }
  float s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int64_t e = tid; e < n; e += CASER_NT) {
    const int b = (int)(e / C), c = (int)(e - (int64_t)b * C);
    const float g = a.dhead[(int64_t)b * a.ldh + CASER_HPAD + c];
    s1 += g;
    s2 = fmaf(g, a.v[e], s2);
  }
  for (int b = tid; b < B; b += CASER_NT) s3 += a.dhead[(int64_t)b * a.ldh];
  s_red[tid] = s1; s_red[CASER_NT + tid] = s2; s_red[2 * CASER_NT + tid] = s3;
  caser_tree_sum(s_red, 3, tid);
  if (tid == 0) {
    a.gbd[0] = s_red[0];
    a.gwd[0] = s_red[CASER_NT];
    a.gbv[0] = a.wd[0] * s_red[0];
    a.gbh[0] = s_red[2 * CASER_NT];
  }
}

static bool caser_shape_ok(const CaserArgs& a) {
  return a.B > 0 && a.T >= CASER_L && a.C > 0 && (a.C & 3) == 0 && a.ldx >= a.C && (a.ldx & 3) == 0 &&
         a.ldh >= CASER_HPAD + a.C && (a.ldh & 3) == 0;
}

int score_caser_fwd(const CaserArgs& a, hipStream_t s) {
  if (!caser_shape_ok(a)) return SCORE_E_SHAPE;
  int CW = 4;
  while (CW < a.C && CW < CASER_NT) CW <<= 1;
  hipLaunchKernelGGL(caser_fwd_kernel, dim3(a.B), dim3(CASER_NT), 0, s, a, CW);
  SCORE_CHECK_LAUNCH();
  return 0;
}

int score_caser_bwd(const CaserArgs& a, hipStream_t s, hipStream_t sp) {
  if (!caser_shape_ok(a)) return SCORE_E_SHAPE;
  const int nwh = (CASER_L * a.C + 31) / 32;
  hipLaunchKernelGGL(caser_params_kernel, dim3(nwh + a.T + 1), dim3(CASER_NT), 0, sp, a, nwh);
  SCORE_CHECK_LAUNCH();
  const int64_t n4 = (int64_t)a.B * a.T * (a.ldx >> 2);
  hipLaunchKernelGGL(caser_dx_kernel, dim3((unsigned)cdiv64(n4, CASER_NT)), dim3(CASER_NT), 0, s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}
