// The DELF point baseline (point_models/point_model.py:200-249) between the gather and the row scatter: per side a masked,
// target-conditioned attention over the gathered history X [B, T, C] (rows of stride ldx),
//   key_t = tanh(X_t W + b),  s_t = [t < len] <q, key_t> + [t >= len] (-2^32 + 1),  a = softmax_t(s),  rep = sum_t a_t X_t
// (side 0: X = user_seq rows, q = target_item, W = dense; side 1: X = item_seq rows, q = target_user, W = dense_1), then the four
// fusion MLPs over [tu|ti], [ru|ri], [tu|ri], [ti|ru] (relu(relu(. A_k + a_k) B_k + b_k), 10 and 4 wide), their sum f, the
// logit f w + c, y = sigmoid, and the log-loss terms of the sample.
//
// Forward: ONE launch, a workgroup of 256 threads per sample.  The threads form R = 256 / CW row groups of CW lanes, CW the
// power of two that covers C (4 .. 128).  Keys: DELF_TT history rows per thread, a chunk of R * DELF_TT rows staged in LDS
// (4 KB whatever T and C are: no assumption that a sample's X fits), W read from L2 row by row (coalesced over the lanes), the
// dot product with q summed over a row group by a fixed butterfly.  The scores go through the attention-weight array itself
// (global, [B, T]: any T), the softmax subtracts the row maximum, and every sum over T or over the lanes runs in a fixed order.
// Rows at or past the length are never read for the keys; with length <= 0 every score is the pad value, a = 1 / T, and rep is
// the mean over all T rows (tf.sequence_mask + softmax do exactly that).
// Backward: ONE launch of the same shape: the fusion MLPs' and the attention's input gradients, dX rows (every one of the ldx
// columns: zeros past C and for masked rows), the target rows' gradients into dhead, and the pre-activation gradients dpre
// [B * T, C] per side plus the fusion layers' (dact) -- what the engine's queued X^T dY products and column sums turn into
// the 22 variables' gradients (split-K in a fixed order, no atomics).
#include <math.h>
#include "common.h"
#include "kernels.h"
#include "cell.h"

#define DELF_NT 256
#define DELF_TT 4                      // history rows per thread in the key / input-gradient products
#define DELF_CMAX SCORE_DELF_CMAX
#define DELF_ACT SCORE_DELF_ACT
#define DELF_PAD (-4294967295.0f)      // (1 - mask) * (-2 ** 32 + 1) as TF's float32 holds it: -2^32

// block-wide sum / max of one value per thread by a fixed tree; every thread calls it and gets the result
__device__ __forceinline__ float delf_block_sum(float v, float* s_red, int tid) {
  __syncthreads();
  s_red[tid] = v;
  __syncthreads();
  for (int st = DELF_NT / 2; st > 0; st >>= 1) {
    if (tid < st) s_red[tid] += s_red[tid + st];
    __syncthreads();
  }
  return s_red[0];
}
__device__ __forceinline__ float delf_block_max(float v, float* s_red, int tid) {
  __syncthreads();
  s_red[tid] = v;
  __syncthreads();
  for (int st = DELF_NT / 2; st > 0; st >>= 1) {
    if (tid < st) s_red[tid] = fmaxf(s_red[tid], s_red[tid + st]);
    __syncthreads();
  }
  return s_red[0];
}

// rows whose keys exist (t < len, at most T) and rows that carry attention weight (all T when every position is masked)
__device__ __forceinline__ int delf_live(int len, int T) { return len <= 0 ? 0 : min(len, T); }
__device__ __forceinline__ int delf_weighted(int len, int T) { return len <= 0 ? T : min(len, T); }

// the two halves of fusion input k: 0 [tu|ti], 1 [ru|ri], 2 [tu|ri], 3 [ti|ru]; s_in: tu, ti, ru, ri at DELF_CMAX apart
__device__ __forceinline__ void delf_inter(int k, int Cu, int Ci, int* first, int* second, int* n1, int* n2) {
  const int f = k == 1 ? 2 : (k == 3 ? 1 : 0), s = k == 0 ? 1 : (k == 3 ? 2 : 3);
  *first = f; *second = s;
  *n1 = (f == 0 || f == 3) ? Cu : Ci;
  *n2 = (s == 0 || s == 3) ? Cu : Ci;
}
// one of four pointers of the argument block by a lane's own index (selects, not an indexed copy of the block)
__device__ __forceinline__ const float* delf_sel(const float* const (&p)[4], int k) {
  return k == 0 ? p[0] : (k == 1 ? p[1] : (k == 2 ? p[2] : p[3]));
}

__global__ __launch_bounds__(DELF_NT) void delf_fwd_kernel(const DelfArgs a) {
  __shared__ float s_x[DELF_NT * DELF_TT];
  __shared__ float s_red[DELF_NT];
  __shared__ float s_in[4 * DELF_CMAX];
  __shared__ float s_h[4 * 6 * 10 + 40 + 16];
  const int b = blockIdx.x, tid = threadIdx.x, T = a.T;
  // target rows: tu, ti
  for (int i = tid; i < a.Cu + a.Ci; i += DELF_NT) {
    if (i < a.Cu) s_in[i] = a.tu[(int64_t)b * a.ldq + i];
    else s_in[DELF_CMAX + i - a.Cu] = a.ti[(int64_t)b * a.ldq + i - a.Cu];
  }
  __syncthreads();
  for (int sd = 0; sd < 2; ++sd) {
    const DelfSide& S = a.s[sd];
    const int C = S.C;
    int CW = 4;
    while (CW < C) CW <<= 1;
    const int R = DELF_NT / CW, r = tid / CW, l = tid - r * CW, RC = R * DELF_TT;
    const float* __restrict__ X = S.X + (int64_t)b * T * S.ldx;
    const float* __restrict__ W = S.W;
    float* __restrict__ key = S.key + (int64_t)b * T * C;
    float* __restrict__ att = S.att + (int64_t)b * T;
    const float* q = s_in + (sd == 0 ? DELF_CMAX : 0);        // side 0: target_item, side 1: target_user
    const int len = S.len[b];
    const int TL = delf_live(len, T), TW = delf_weighted(len, T);
    const float ql = l < C ? q[l] : 0.f, bl = l < C ? S.b[l] : 0.f;
    // ---- keys and scores of the live rows
    for (int t0 = 0; t0 < TL; t0 += RC) {
      for (int i = tid; i < RC * C; i += DELF_NT) {
        const int row = i / C, c = i - row * C;
        s_x[i] = t0 + row < TL ? X[(int64_t)(t0 + row) * S.ldx + c] : 0.f;
      }
      __syncthreads();
      float acc[DELF_TT];
#pragma unroll
      for (int j = 0; j < DELF_TT; ++j) acc[j] = bl;
      if (l < C) {
        const float* xr = s_x + r * DELF_TT * C;
        for (int k = 0; k < C; ++k) {
          const float w = W[(int64_t)k * C + l];
#pragma unroll
          for (int j = 0; j < DELF_TT; ++j) acc[j] = fmaf(xr[j * C + k], w, acc[j]);
        }
      }
      float p[DELF_TT];
#pragma unroll
      for (int j = 0; j < DELF_TT; ++j) {
        const int t = t0 + r * DELF_TT + j;
        const float kv = tanhf(acc[j]);
        if (l < C && t < TL) key[(int64_t)t * C + l] = kv;
        p[j] = group_sum(l < C ? ql * kv : 0.f, min(CW, SCORE_WAVE));
      }
      if (CW > SCORE_WAVE) {       // a row group of two waves: their sums through LDS, lower wave first
        __syncthreads();
        if ((tid & (SCORE_WAVE - 1)) == 0)
#pragma unroll
          for (int j = 0; j < DELF_TT; ++j) s_red[(tid >> 6) * DELF_TT + j] = p[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < DELF_TT; ++j) p[j] = s_red[(2 * r) * DELF_TT + j] + s_red[(2 * r + 1) * DELF_TT + j];
      }
      if (l == 0)
#pragma unroll
        for (int j = 0; j < DELF_TT; ++j) {
          const int t = t0 + r * DELF_TT + j;
          if (t < TL) att[t] = p[j];
        }
      __syncthreads();
    }
    for (int t = TL + tid; t < T; t += DELF_NT) att[t] = DELF_PAD;
    __syncthreads();
    // ---- softmax over all T positions (row maximum subtracted)
    float mx = -INFINITY;
    for (int t = tid; t < T; t += DELF_NT) mx = fmaxf(mx, att[t]);
    mx = delf_block_max(mx, s_red, tid);
    float sum = 0.f;
    for (int t = tid; t < T; t += DELF_NT) {
      const float e = expf(att[t] - mx);
      att[t] = e;
      sum += e;
    }
    sum = delf_block_sum(sum, s_red, tid);
    for (int t = tid; t < T; t += DELF_NT) att[t] = att[t] / sum;
    __syncthreads();
    // ---- rep = sum_t a_t X_t: a row group's share in rising t, then the groups in order
    float part = 0.f;
    if (l < C)
      for (int t = r; t < TW; t += R) part = fmaf(att[t], X[(int64_t)t * S.ldx + l], part);
    s_x[tid] = part;
    __syncthreads();
    if (r == 0 && l < C) {
      float v = 0.f;
      for (int g = 0; g < R; ++g) v += s_x[g * CW + l];
      S.rep[(int64_t)b * C + l] = v;
      s_in[(sd == 0 ? 2 : 3) * DELF_CMAX + l] = v;
    }
    __syncthreads();
  }
  // ---- fusion MLPs: wave k takes input k; lane = part * 10 + unit, six parts over the input columns
  {
    const int k = tid >> 6, lane = tid & 63, part = lane / 10, j = lane - part * 10;
    int fi, se, n1, n2;
    delf_inter(k, a.Cu, a.Ci, &fi, &se, &n1, &n2);
    if (part < 6) {
      const float* A = delf_sel(a.A, k);
      const float* x1 = s_in + fi * DELF_CMAX;
      const float* x2 = s_in + se * DELF_CMAX;
      float acc = 0.f;
      for (int i = part; i < n1 + n2; i += 6) acc = fmaf(i < n1 ? x1[i] : x2[i - n1], A[i * 10 + j], acc);
      s_h[(k * 6 + part) * 10 + j] = acc;
    }
  }
  __syncthreads();
  float* s_h1 = s_h + 240;
  float* s_h2 = s_h + 280;
  float* act = a.act + (int64_t)b * DELF_ACT;
  if (tid < 40) {
    const int k = tid / 10, j = tid - k * 10;
    float v = 0.f;
    for (int p = 0; p < 6; ++p) v += s_h[(k * 6 + p) * 10 + j];
    v = fmaxf(v + delf_sel(a.a1, k)[j], 0.f);
    s_h1[tid] = v;
    act[tid] = v;
  }
  __syncthreads();
  if (tid < 16) {
    const int k = tid >> 2, o = tid & 3;
    float v = 0.f;
    const float* Bk = delf_sel(a.Bm, k);
    for (int j = 0; j < 10; ++j) v = fmaf(s_h1[k * 10 + j], Bk[j * 4 + o], v);
    v = fmaxf(v + delf_sel(a.b2, k)[o], 0.f);
    s_h2[tid] = v;
    act[40 + tid] = v;
  }
  __syncthreads();
  if (tid == 0) {
    float z = 0.f;
    for (int o = 0; o < 4; ++o) {
      const float f = ((s_h2[o] + s_h2[4 + o]) + s_h2[8 + o]) + s_h2[12 + o];
      act[56 + o] = f;
      z = fmaf(f, a.w[o], z);
    }
    z += a.c[0];
    const float pr = sigmoidf_(z);
    const float lab = (float)a.label[b];
    a.logit[b] = z;
    a.y[b] = pr;
    a.lossb[b] = logloss_term(pr, lab);
    a.dlogit[b] = logloss_dlogit(pr, lab, a.Bglobal);
  }
}

// d inter_k[i] = sum_j dpre1[k][j] A_k[i, j]
__device__ __forceinline__ float delf_dinter(const DelfArgs& a, const float* s_d1, int k, int i) {
  const float* A = a.A[k] + i * 10;
  float v = 0.f;
#pragma unroll
  for (int j = 0; j < 10; ++j) v = fmaf(s_d1[k * 10 + j], A[j], v);
  return v;
}

__global__ __launch_bounds__(DELF_NT) void delf_bwd_kernel(const DelfArgs a) {
  __shared__ float s_x[DELF_NT * DELF_TT];
  __shared__ float s_red[DELF_NT];
  __shared__ float s_q[2 * DELF_CMAX];         // tu, ti
  __shared__ float s_dt[2 * DELF_CMAX];        // d tu, d ti
  __shared__ float s_dr[2 * DELF_CMAX];        // d ru (side 0's dout), d ri (side 1's)
  __shared__ float s_d[40 + 16];
  const int b = blockIdx.x, tid = threadIdx.x, T = a.T, Cu = a.Cu, Ci = a.Ci;
  const float* act = a.act + (int64_t)b * DELF_ACT;
  float* dact = a.dact + (int64_t)b * DELF_ACT;
  float* s_d1 = s_d;
  float* s_d2 = s_d + 40;
  for (int i = tid; i < Cu + Ci; i += DELF_NT) {
    if (i < Cu) s_q[i] = a.tu[(int64_t)b * a.ldq + i];
    else s_q[DELF_CMAX + i - Cu] = a.ti[(int64_t)b * a.ldq + i - Cu];
  }
  // ---- the logit, f and the fusion MLPs
  const float g = a.dlogit[b];
  if (tid < 16) {
    const float v = act[40 + tid] > 0.f ? g * a.w[tid & 3] : 0.f;
    s_d2[tid] = v;
    dact[40 + tid] = v;
  }
  __syncthreads();
  if (tid < 40) {
    const int k = tid / 10, j = tid - k * 10;
    float v = 0.f;
    const float* Bk = delf_sel(a.Bm, k);
#pragma unroll
    for (int o = 0; o < 4; ++o) v = fmaf(s_d2[k * 4 + o], Bk[j * 4 + o], v);
    v = act[tid] > 0.f ? v : 0.f;
    s_d1[tid] = v;
    dact[tid] = v;
  }
  __syncthreads();
  if (tid < DELF_CMAX) {
    const int c = tid;
    if (c < Cu) {
      s_dt[c] = delf_dinter(a, s_d1, 0, c) + delf_dinter(a, s_d1, 2, c);                               // tu: [tu|ti], [tu|ri]
      s_dr[DELF_CMAX + c] = delf_dinter(a, s_d1, 1, Ci + c) + delf_dinter(a, s_d1, 2, Cu + c);         // ri: [ru|ri], [tu|ri]
    }
    if (c < Ci) {
      s_dt[DELF_CMAX + c] = delf_dinter(a, s_d1, 0, Cu + c) + delf_dinter(a, s_d1, 3, c);              // ti: [tu|ti], [ti|ru]
      s_dr[c] = delf_dinter(a, s_d1, 1, c) + delf_dinter(a, s_d1, 3, Ci + c);                          // ru: [ru|ri], [ti|ru]
    }
  }
  __syncthreads();
  for (int sd = 0; sd < 2; ++sd) {
    const DelfSide& S = a.s[sd];
    const int C = S.C;
    int CW = 4;
    while (CW < C) CW <<= 1;
    const int R = DELF_NT / CW, r = tid / CW, l = tid - r * CW, RC = R * DELF_TT;
    const float* __restrict__ X = S.X + (int64_t)b * T * S.ldx;
    const float* __restrict__ W = S.W;
    const float* __restrict__ key = S.key + (int64_t)b * T * C;
    const float* __restrict__ att = S.att + (int64_t)b * T;
    float* __restrict__ ds = S.ds + (int64_t)b * T;
    float* __restrict__ dX = S.dX + (int64_t)b * T * S.ldx;
    float* __restrict__ dpre = S.dpre + (int64_t)b * T * C;
    const float* q = s_q + (sd == 0 ? DELF_CMAX : 0);
    float* dq = s_dt + (sd == 0 ? DELF_CMAX : 0);
    const float* dout = s_dr + sd * DELF_CMAX;
    const int len = S.len[b];
    const int TL = delf_live(len, T), TW = delf_weighted(len, T);
    // ---- d a_t = <dout, X_t>, then the softmax: d s_t = a_t (d a_t - sum_t' a_t' d a_t'); a thread per position
    float u = 0.f;
    for (int t = tid; t < TW; t += DELF_NT) {
      const float* x = X + (int64_t)t * S.ldx;
      float v = 0.f;
      for (int c = 0; c < C; c += 4) {
        const float4 xv = ld4(x + c);
        v = fmaf(dout[c], xv.x, v); v = fmaf(dout[c + 1], xv.y, v); v = fmaf(dout[c + 2], xv.z, v); v = fmaf(dout[c + 3], xv.w, v);
      }
      ds[t] = v;
      u = fmaf(att[t], v, u);
    }
    const float sdot = delf_block_sum(u, s_red, tid);
    for (int t = tid; t < TW; t += DELF_NT) ds[t] = att[t] * (ds[t] - sdot);
    __syncthreads();
    // ---- d q = sum_{t live} d s_t key_t: a row group's share in rising t, then the groups in order
    float part = 0.f;
    if (l < C)
      for (int t = r; t < TL; t += R) part = fmaf(ds[t], key[(int64_t)t * C + l], part);
    s_x[tid] = part;
    __syncthreads();
    if (r == 0 && l < C) {
      float v = 0.f;
      for (int gq = 0; gq < R; ++gq) v += s_x[gq * CW + l];
      dq[l] += v;
    }
    __syncthreads();
    // ---- d pre_t = d s_t q (1 - key_t^2) for the live rows (zero rows past them), and d X_t = a_t dout + d pre_t W^T
    for (int t0 = 0; t0 < T; t0 += RC) {
      for (int i = tid; i < RC * C; i += DELF_NT) {
        const int row = i / C, c = i - row * C, t = t0 + row;
        float v = 0.f;
        if (t < TL) {
          const float kv = key[(int64_t)t * C + c];
          v = ds[t] * q[c] * (1.0f - kv * kv);
        }
        s_x[i] = v;
        if (t < T) dpre[(int64_t)t * C + c] = v;
      }
      __syncthreads();
      if (l < C) {
        float acc[DELF_TT];
#pragma unroll
        for (int j = 0; j < DELF_TT; ++j) acc[j] = 0.f;
        if (t0 < TL) {
          const float* pr = s_x + r * DELF_TT * C;
          const float* wr = W + (int64_t)l * C;
          for (int c = 0; c < C; c += 4) {
            const float4 w = ld4(wr + c);
#pragma unroll
            for (int j = 0; j < DELF_TT; ++j) {
              const float* p = pr + j * C + c;
              acc[j] = fmaf(p[0], w.x, acc[j]); acc[j] = fmaf(p[1], w.y, acc[j]);
              acc[j] = fmaf(p[2], w.z, acc[j]); acc[j] = fmaf(p[3], w.w, acc[j]);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < DELF_TT; ++j) {
          const int t = t0 + r * DELF_TT + j;
          if (t < T) dX[(int64_t)t * S.ldx + l] = t < TW ? fmaf(att[t], dout[l], acc[j]) : 0.f;
        }
      }
      __syncthreads();
    }
    // the columns of the gather's rows that this model does not read
    const int extra = S.ldx - C;
    for (int i = tid; i < T * extra; i += DELF_NT) {
      const int t = i / extra, c = C + i - t * extra;
      dX[(int64_t)t * S.ldx + c] = 0.f;
    }
  }
  __syncthreads();
  float* dh = a.dhead + (int64_t)b * a.ldh;
  for (int i = tid; i < Cu + Ci; i += DELF_NT) {
    if (i < Cu) dh[a.off_tu + i] = s_dt[i];
    else dh[a.off_ti + i - Cu] = s_dt[DELF_CMAX + i - Cu];
  }
}

static bool delf_shape_ok(const DelfArgs& a) {
  if (a.B <= 0 || a.T <= 0 || a.Bglobal <= 0 || a.Cu <= 0 || a.Ci <= 0 || a.Cu > DELF_CMAX || a.Ci > DELF_CMAX) return false;
  if ((a.Cu & 3) || (a.Ci & 3) || a.s[0].C != a.Ci || a.s[1].C != a.Cu) return false;
  for (int sd = 0; sd < 2; ++sd)
    if (a.s[sd].ldx < a.s[sd].C || (a.s[sd].ldx & 3)) return false;
  return a.ldh >= a.Cu + a.Ci && a.ldq >= a.Cu + a.Ci;
}

int score_delf_fwd(const DelfArgs& a, hipStream_t s) {
  if (!delf_shape_ok(a)) return SCORE_E_SHAPE;
  hipLaunchKernelGGL(delf_fwd_kernel, dim3(a.B), dim3(DELF_NT), 0, s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}

int score_delf_bwd(const DelfArgs& a, hipStream_t s) {
  if (!delf_shape_ok(a)) return SCORE_E_SHAPE;
  hipLaunchKernelGGL(delf_bwd_kernel, dim3(a.B), dim3(DELF_NT), 0, s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}
