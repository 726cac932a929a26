// The SASRec point baseline (point_models/point_model.py:313-469 on PointBaseModel :9-63) between the gather and the row scatter.
// Per sample, with X [T, C] the gathered history rows (C = Fi * D), two heads of width C / 2:
//   N = (X - mean) / sqrt(var + 1e-8) per row, Qin = gamma N + beta                       (normalize, :441-469)
//   Q = Qin Wq + bq, K = X Wk + bk, V = X Wv + bv                                         (multihead_attention, :362-439)
//   S_h = Q_h K_h^T / sqrt(C / 2); S_h[., u] = -2^32 + 1 where sum_c X[u, c] == 0; P_h = softmax over all T keys
//   W_h = dropout(P_h * [sum_c Qin[t, c] != 0]);  Y = concat_h(W_h V_h) + Qin
//   rep_t = Y_t [t < length], final = sum_t rep_t                                         (:318-331)
//   head rows: [rep_t | Y_t | target_user] for t = 1 .. T - 1, and [final | target_item | target_user]
// and, behind the shared head's two products (the engine's GEMMs), fc3 + sigmoid + the three log-loss means (:338-345).
//
// Attention forward: ONE launch, a workgroup of 256 threads per sample, X staged once in LDS (row stride C + 1: the score and
// A V loops walk rows at a fixed column).  Every sum runs in a fixed order -- a row's mean / variance / mask sums and a
// softmax row by one thread in rising index, a product's k loop in rising k -- so two runs give the same bits.
// Attention backward: ONE launch of the same shape, from the head-input gradient to dX (every one of the ldx columns written),
// the three pre-projection gradients dQ / dK / dV (rows of the queued weight-gradient products), the per-sample partials of the
// gamma / beta gradients and the target rows' gradients in dhead.  No atomics anywhere.
// The masks carry no gradient; a masked key's score is a constant, so no gradient passes through it.
#include <math.h>
#include "common.h"
#include "kernels.h"
#include "cell.h"

#define SAS_NT 256
#define SAS_TR 8                  // rows per register block of the C x C products
#define SAS_FC1 200
#define SAS_FC2 80
#define SAS_PAD_SCORE (-4294967295.0f)      // -2^32 + 1 (fp32: -2^32)
// one hash stream per use of tf.nn.dropout: the attention weights, then (application, layer) of the shared head
#define SAS_SEED_ATT 0x8A5CD789635D2DFFull
__device__ __forceinline__ uint64_t sas_head_stream(uint64_t seed, int app, int layer) {
  return seed ^ (0x5DEECE66Dull * (uint64_t)(2 * app + layer + 1));
}

__host__ __device__ static inline int64_t sas_lds_floats(int T, int C) {
  return 4 * (int64_t)T * (C + 1) + 2 * (int64_t)T * T + 4 * (int64_t)T;
}
bool score_sasrec_fits(int T, int C) {
  return T >= 3 && C >= 4 && (C & 3) == 0 && C <= SCORE_SASREC_CMAX && sas_lds_floats(T, C) * 4 <= 160 * 1024;
}

// rows of the sample that are live: tf.sequence_mask(length, T)
__device__ __forceinline__ int sas_live(int len, int T) { return len <= 0 ? 0 : min(len, T); }

// out[t, j] (+)= sum_k in[t, k] Wm(k, j) (+ bias[j]) for t < T, j < C; Wm(k, j) = TRANS ? W[j * C + k] : W[k * C + j].  in / out
// are LDS matrices of row stride ld; gout (optional): a [T, C] copy of the result in global memory.  A work item is one output
// column of SAS_TR rows; k rises, so the order of every sum is fixed.
template <bool TRANS, bool ACC>
__device__ __forceinline__ void sas_proj(const float* in, const float* __restrict__ W, const float* __restrict__ bias, float* out,
                                         float* __restrict__ gout, int ld, int T, int C, int tid) {
  const int nrb = (T + SAS_TR - 1) / SAS_TR;
  for (int item = tid; item < nrb * C; item += SAS_NT) {
    const int rb = item / C, j = item - rb * C, t0 = rb * SAS_TR;
    const float* row[SAS_TR];
    float acc[SAS_TR];
#pragma unroll
    for (int r = 0; r < SAS_TR; ++r) { row[r] = in + min(t0 + r, T - 1) * ld; acc[r] = 0.f; }
    if (TRANS) {
      const float* __restrict__ w = W + (int64_t)j * C;
      for (int k = 0; k < C; k += 4) {
        const float4 w4 = ld4(w + k);
#pragma unroll
        for (int r = 0; r < SAS_TR; ++r) {
          acc[r] = fmaf(row[r][k], w4.x, acc[r]); acc[r] = fmaf(row[r][k + 1], w4.y, acc[r]);
          acc[r] = fmaf(row[r][k + 2], w4.z, acc[r]); acc[r] = fmaf(row[r][k + 3], w4.w, acc[r]);
        }
      }
    } else {
      for (int k = 0; k < C; ++k) {
        const float w = W[(int64_t)k * C + j];
#pragma unroll
        for (int r = 0; r < SAS_TR; ++r) acc[r] = fmaf(row[r][k], w, acc[r]);
      }
    }
    const float bj = bias ? bias[j] : 0.f;
#pragma unroll
    for (int r = 0; r < SAS_TR; ++r)
      if (t0 + r < T) {
        float v = acc[r] + bj;
        if (ACC) v += out[(t0 + r) * ld + j];
        out[(t0 + r) * ld + j] = v;
        if (gout) gout[(int64_t)(t0 + r) * C + j] = v;
      }
  }
}

// a [T, C] matrix of global memory (row stride lds_) into an LDS matrix of row stride ld
__device__ __forceinline__ void sas_load(float* dst, int ld, const float* __restrict__ src, int lds_, int T, int C, int tid) {
  for (int i = tid; i < T * C; i += SAS_NT) {
    const int t = i / C, c = i - t * C;
    dst[t * ld + c] = src[(int64_t)t * lds_ + c];
  }
}

__global__ __launch_bounds__(SAS_NT) void sasrec_attn_fwd_kernel(const SasrecArgs a) {
  extern __shared__ float sm[];
  const int b = blockIdx.x, tid = threadIdx.x, T = a.T, C = a.C, CP = C + 1, dh = C >> 1, B = a.B;
  float* b0 = sm;                       // X, then Q, then Y
  float* b1 = b0 + T * CP;              // Qin
  float* b2 = b1 + T * CP;              // N, then K
  float* b3 = b2 + T * CP;              // V
  float* sc = b3 + T * CP;              // [2, T, T] scores, then weights
  float* km = sc + 2 * T * T;           // [T] key mask
  float* qm = km + T;                   // [T] query mask
  const int64_t row0 = (int64_t)b * T;
  sas_load(b0, CP, a.X + row0 * a.ldx, a.ldx, T, C, tid);
  __syncthreads();
  // ---- layer norm and the two masks: a row per thread, every sum in rising c
  for (int t = tid; t < T; t += SAS_NT) {
    const float* x = b0 + t * CP;
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += x[c];
    const float mean = s / (float)C;
    float v = 0.f;
    for (int c = 0; c < C; ++c) { const float d = x[c] - mean; v = fmaf(d, d, v); }
    const float sdev = sqrtf(v / (float)C + 1e-8f);
    float qs = 0.f;
    for (int c = 0; c < C; ++c) {
      const float n = (x[c] - mean) / sdev;
      const float q = fmaf(a.gamma[c], n, a.beta[c]);
      b2[t * CP + c] = n; b1[t * CP + c] = q;
      qs += q;
    }
    km[t] = s != 0.f ? 1.f : 0.f;
    qm[t] = qs != 0.f ? 1.f : 0.f;
    a.rstd[row0 + t] = 1.0f / sdev;
    a.km[row0 + t] = km[t];
  }
  __syncthreads();
  for (int i = tid; i < T * C; i += SAS_NT) {
    const int t = i / C, c = i - t * C;
    a.nrm[(row0 + t) * C + c] = b2[t * CP + c];
    a.qin[(row0 + t) * C + c] = b1[t * CP + c];
  }
  __syncthreads();
  // ---- the three projections: K and V from the raw X, Q from Qin
  sas_proj<false, false>(b0, a.Wk, a.bk, b2, a.k + row0 * C, CP, T, C, tid);
  sas_proj<false, false>(b0, a.Wv, a.bv, b3, a.v + row0 * C, CP, T, C, tid);
  __syncthreads();
  sas_proj<false, false>(b1, a.Wq, a.bq, b0, a.q + row0 * C, CP, T, C, tid);
  __syncthreads();
  // ---- both heads' scaled scores under the key mask
  const float sq = sqrtf((float)dh);
  for (int i = tid; i < 2 * T * T; i += SAS_NT) {
    const int h = i / (T * T), r = i - h * T * T, t = r / T, u = r - t * T;
    const float* q = b0 + t * CP + h * dh;
    const float* k = b2 + u * CP + h * dh;
    float s = 0.f;
    for (int c = 0; c < dh; ++c) s = fmaf(q[c], k[c], s);
    sc[i] = km[u] != 0.f ? s / sq : SAS_PAD_SCORE;
  }
  __syncthreads();
  // ---- softmax over all T keys: a row per thread
  for (int r = tid; r < 2 * T; r += SAS_NT) {
    float* p = sc + r * T;
    float m = p[0];
    for (int u = 1; u < T; ++u) m = fmaxf(m, p[u]);
    float s = 0.f;
    for (int u = 0; u < T; ++u) { const float e = expf(p[u] - m); p[u] = e; s += e; }
    for (int u = 0; u < T; ++u) p[u] = p[u] / s;
  }
  __syncthreads();
  // ---- query mask and dropout; P and the final weights are kept for the backward pass
  const bool drop = a.keep < 1.f;
  const uint64_t seed = (a.seed_dev ? *a.seed_dev : a.seed) ^ SAS_SEED_ATT;
  for (int i = tid; i < 2 * T * T; i += SAS_NT) {
    const int h = i / (T * T), r = i - h * T * T, t = r / T;
    const float p = sc[i];
    float w = p * qm[t];
    if (drop) {
      const uint64_t e = ((uint64_t)h * B + b) * (uint64_t)(T * T) + r;      // [2, B, T, T]: head h of sample b at row h B + b
      const bool on = a.mask_a ? a.mask_a[e] != 0 : hash_uniform(seed, e) < a.keep;
      w = on ? w / a.keep : 0.f;
    }
    a.p[(int64_t)b * 2 * T * T + i] = p;
    a.att[(int64_t)b * 2 * T * T + i] = w;
    sc[i] = w;
  }
  __syncthreads();
  // ---- Y = concat_h(W_h V_h) + Qin
  for (int i = tid; i < T * C; i += SAS_NT) {
    const int t = i / C, c = i - t * C, h = c >= dh ? 1 : 0;
    const float* w = sc + (h * T + t) * T;
    float s = 0.f;
    for (int u = 0; u < T; ++u) s = fmaf(w[u], b3[u * CP + c], s);
    const float y = s + b1[t * CP + c];
    b0[t * CP + c] = y;
    a.yseq[(row0 + t) * C + c] = y;
  }
  __syncthreads();
  // ---- rep, final and the head-input rows
  const int L = sas_live(a.length[b], T), Dh = a.Dh, Cu = a.Cu;
  const int64_t P = (int64_t)B * (T - 1);
  const float* tu = a.tu + (int64_t)b * a.ldq;
  const float* ti = a.ti + (int64_t)b * a.ldq;
  float* hfin = a.hin + (P + b) * Dh;
  for (int c = tid; c < C; c += SAS_NT) {
    float f = 0.f;
    for (int t = 0; t < L; ++t) f += b0[t * CP + c];
    a.fin[(int64_t)b * C + c] = f;
    hfin[c] = f;
    hfin[C + c] = ti[c];
  }
  for (int c = tid; c < Cu; c += SAS_NT) hfin[2 * C + c] = tu[c];
  float* hpos = a.hin + (int64_t)b * (T - 1) * Dh;
  for (int i = tid; i < (T - 1) * Dh; i += SAS_NT) {
    const int tt = i / Dh, col = i - tt * Dh, t = tt + 1;
    float v;
    if (col < C) v = t < L ? b0[t * CP + col] : 0.f;
    else if (col < 2 * C) v = b0[t * CP + col - C];
    else v = tu[col - 2 * C];
    hpos[i] = v;
  }
}

__global__ __launch_bounds__(SAS_NT) void sasrec_attn_bwd_kernel(const SasrecArgs a) {
  extern __shared__ float sm[];
  const int b = blockIdx.x, tid = threadIdx.x, T = a.T, C = a.C, CP = C + 1, dh = C >> 1, B = a.B, Dh = a.Dh, Cu = a.Cu;
  float* b0 = sm;                       // dY, then dQin
  float* b1 = b0 + T * CP;              // V, then K, then dK, then N
  float* b2 = b1 + T * CP;              // dV
  float* b3 = b2 + T * CP;              // Q, then dQ, then dK Wk^T + dV Wv^T
  float* sc = b3 + T * CP;              // [2, T, T] d weights, then d scores
  float* km = sc + 2 * T * T;           // [T]
  float* ra = km + T;                   // [T] mean_c(gamma dQin)
  float* rb = ra + T;                   // [T] mean_c(gamma dQin N)
  const int64_t row0 = (int64_t)b * T;
  const int L = sas_live(a.length[b], T);
  const int64_t P = (int64_t)B * (T - 1);
  const float* gpos = a.dhin + (int64_t)b * (T - 1) * Dh;      // rows t = 1 .. T - 1
  const float* gfin = a.dhin + (P + b) * Dh;
  // ---- dY from the head-input gradient: [d rep_t | d Y_t | .] of the positive rows, d final of the final row
  for (int i = tid; i < T * C; i += SAS_NT) {
    const int t = i / C, c = i - t * C;
    float v = 0.f, vr = 0.f;
    if (t >= 1) {      // (position 0 has no head row)
      const float* g = gpos + (int64_t)(t - 1) * Dh;
      v = g[C + c]; vr = g[c];
    }
    if (t < L) v += vr + gfin[c];
    b0[t * CP + c] = v;
  }
  sas_load(b1, CP, a.v + row0 * C, C, T, C, tid);
  for (int t = tid; t < T; t += SAS_NT) km[t] = a.km[row0 + t];
  // ---- the target rows: target_user enters every head row, target_item the final row
  {
    float* dh_ = a.dhead + (int64_t)b * a.ldh;
    for (int c = tid; c < Cu; c += SAS_NT) {
      float s = gfin[2 * C + c];
      for (int tt = 0; tt < T - 1; ++tt) s += gpos[(int64_t)tt * Dh + 2 * C + c];
      dh_[a.off_tu + c] = s;
    }
    for (int c = tid; c < C; c += SAS_NT) dh_[a.off_ti + c] = gfin[C + c];
  }
  __syncthreads();
  // ---- d weights = dY_h V_h^T and dV = W^T dY
  const float* attb = a.att + (int64_t)b * 2 * T * T;
  const float* pb = a.p + (int64_t)b * 2 * T * T;
  for (int i = tid; i < 2 * T * T; i += SAS_NT) {
    const int h = i / (T * T), r = i - h * T * T, t = r / T, u = r - t * T;
    const float* g = b0 + t * CP + h * dh;
    const float* v = b1 + u * CP + h * dh;
    float s = 0.f;
    for (int c = 0; c < dh; ++c) s = fmaf(g[c], v[c], s);
    sc[i] = s;
  }
  for (int i = tid; i < T * C; i += SAS_NT) {
    const int u = i / C, c = i - u * C, h = c >= dh ? 1 : 0;
    const float* w = attb + (int64_t)h * T * T + u;
    float s = 0.f;
    for (int t = 0; t < T; ++t) s = fmaf(w[(int64_t)t * T], b0[t * CP + c], s);
    b2[u * CP + c] = s;
    a.dv[(row0 + u) * C + c] = s;
  }
  __syncthreads();
  // ---- through dropout and the query mask (a weight that is zero passes nothing), the softmax and the scale; a masked key's
  // score is a constant
  const float ik = 1.0f / a.keep, sq = sqrtf((float)dh);
  for (int r = tid; r < 2 * T; r += SAS_NT) {
    float* g = sc + r * T;
    const float* p = pb + (int64_t)r * T;
    const float* w = attb + (int64_t)r * T;
    float s = 0.f;
    for (int u = 0; u < T; ++u) {
      const float dp = w[u] != 0.f ? g[u] * ik : 0.f;
      g[u] = dp;
      s = fmaf(dp, p[u], s);
    }
    for (int u = 0; u < T; ++u) g[u] = km[u] != 0.f ? p[u] * (g[u] - s) / sq : 0.f;
  }
  __syncthreads();
  sas_load(b1, CP, a.k + row0 * C, C, T, C, tid);
  sas_load(b3, CP, a.q + row0 * C, C, T, C, tid);
  __syncthreads();
  // ---- dQ = dS K, dK = dS^T Q: to global memory (the rows of the queued weight-gradient products), read back below
  for (int i = tid; i < T * C; i += SAS_NT) {
    const int t = i / C, c = i - t * C, h = c >= dh ? 1 : 0;
    const float* g = sc + (h * T + t) * T;
    float s = 0.f;
    for (int u = 0; u < T; ++u) s = fmaf(g[u], b1[u * CP + c], s);
    a.dq[(row0 + t) * C + c] = s;
    const float* gt = sc + h * T * T + t;      // (t as the key index u here)
    float s2 = 0.f;
    for (int tq = 0; tq < T; ++tq) s2 = fmaf(gt[tq * T], b3[tq * CP + c], s2);
    a.dk[(row0 + t) * C + c] = s2;
  }
  __threadfence_block();
  __syncthreads();
  sas_load(b3, CP, a.dq + row0 * C, C, T, C, tid);
  sas_load(b1, CP, a.dk + row0 * C, C, T, C, tid);
  __syncthreads();
  // ---- dQin = dY + dQ Wq^T (in place); the raw X's share of dX = dK Wk^T + dV Wv^T
  sas_proj<true, true>(b3, a.Wq, nullptr, b0, nullptr, CP, T, C, tid);
  __syncthreads();
  sas_proj<true, false>(b1, a.Wk, nullptr, b3, nullptr, CP, T, C, tid);
  __syncthreads();
  sas_proj<true, true>(b2, a.Wv, nullptr, b3, nullptr, CP, T, C, tid);
  sas_load(b1, CP, a.nrm + row0 * C, C, T, C, tid);      // (b1's dK was last read before the barrier above)
  __syncthreads();
  // ---- layer norm backward: dX = (g dQin - mean(g dQin) - N mean(g dQin N)) / sqrt(var + eps)
  for (int t = tid; t < T; t += SAS_NT) {
    float s1 = 0.f, s2 = 0.f;
    for (int c = 0; c < C; ++c) {
      const float gd = a.gamma[c] * b0[t * CP + c];
      s1 += gd;
      s2 = fmaf(gd, b1[t * CP + c], s2);
    }
    ra[t] = s1 / (float)C; rb[t] = s2 / (float)C;
  }
  __syncthreads();
  float* dX = a.dX + row0 * a.ldx;
  for (int i = tid; i < T * C; i += SAS_NT) {
    const int t = i / C, c = i - t * C;
    const float n = b1[t * CP + c];
    const float gd = a.gamma[c] * b0[t * CP + c];
    dX[(int64_t)t * a.ldx + c] = fmaf(a.rstd[row0 + t], gd - ra[t] - n * rb[t], b3[t * CP + c]);
  }
  {      // the columns of the gather's rows that this model does not read
    const int extra = a.ldx - C;
    for (int i = tid; i < T * extra; i += SAS_NT) {
      const int t = i / extra, c = C + i - t * extra;
      dX[(int64_t)t * a.ldx + c] = 0.f;
    }
  }
  // ---- gamma's and beta's gradients of this sample: rising t
  for (int c = tid; c < C; c += SAS_NT) {
    float sg = 0.f, sb = 0.f;
    for (int t = 0; t < T; ++t) {
      const float g = b0[t * CP + c];
      sg = fmaf(g, b1[t * CP + c], sg);
      sb += g;
    }
    a.dgamma[(int64_t)b * C + c] = sg;
    a.dbeta[(int64_t)b * C + c] = sb;
  }
}

// ---------------------------------------------------------------- the shared head around the engine's two GEMMs
// Rows of the head's activations from fc1's output on: positive rows (b-major, t = 1 .. T - 1), negative rows (t = 2 .. T - 1),
// final rows.  fc1's pre-activations z1 exist once, for the positive and the final rows [B (T - 1) + B, 200]: a negative row is
// the positive row of the same (b, t) under dropout masks of its own.  share != 0 (keep_prob = 1: no dropout anywhere): there
// are no negative rows at all, their loss term and gradient ride on the positive rows t >= 2.
struct SasRows { int64_t P, Nn, R; };
__host__ __device__ static inline SasRows sas_rows(int B, int T, int share) {
  SasRows r;
  r.P = (int64_t)B * (T - 1); r.Nn = share ? 0 : (int64_t)B * (T - 2); r.R = r.P + r.Nn + B;
  return r;
}
// row r of the expanded layout -> its row of z1 (positive and final rows only) and its application (0 pos, 1 neg, 2 final)
__device__ __forceinline__ int64_t sas_src_row(const SasRows& n, int T, int64_t r, int* app, int64_t* local) {
  if (r < n.P) { *app = 0; *local = r; return r; }
  if (r < n.P + n.Nn) {
    const int64_t i = r - n.P, bb = i / (T - 2);
    *app = 1; *local = i;
    return bb * (T - 1) + (i - bb * (T - 2)) + 1;
  }
  *app = 2; *local = r - n.P - n.Nn;
  return n.P + *local;
}

// f1[r, j] = dropout(relu(z1[src(r), j]))
__global__ __launch_bounds__(256) void sasrec_fan_kernel(const SasrecArgs a) {
  const SasRows n = sas_rows(a.B, a.T, a.share);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n.R * SAS_FC1) return;
  const int64_t r = i / SAS_FC1;
  const int j = (int)(i - r * SAS_FC1);
  int app; int64_t local;
  const int64_t src = sas_src_row(n, a.T, r, &app, &local);
  float v = fmaxf(a.z1[src * SAS_FC1 + j], 0.f);
  if (a.keep < 1.f) {
    const uint64_t seed = a.seed_dev ? *a.seed_dev : a.seed;
    const bool on = a.mask0 ? a.mask0[i] != 0 : hash_uniform(sas_head_stream(seed, app, 0), (uint64_t)(local * SAS_FC1 + j)) < a.keep;
    v = on ? v / a.keep : 0.f;
  }
  a.f1[i] = v;
}

// dz1[s, j] = sum over the rows r of the expanded layout with src(r) = s of dz1e[r, j]
__global__ __launch_bounds__(256) void sasrec_fold_kernel(const SasrecArgs a) {
  const SasRows n = sas_rows(a.B, a.T, a.share);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (n.P + a.B) * SAS_FC1) return;
  const int64_t s = i / SAS_FC1;
  const int j = (int)(i - s * SAS_FC1);
  float v;
  if (s < n.P) {
    v = a.dz1e[i];
    const int64_t bb = s / (a.T - 1);
    const int t = (int)(s - bb * (a.T - 1)) + 1;
    if (n.Nn && t >= 2) v += a.dz1e[(n.P + bb * (a.T - 2) + (t - 2)) * SAS_FC1 + j];
  } else {
    v = a.dz1e[(s + n.Nn) * SAS_FC1 + j];
  }
  a.dz1[i] = v;
}

// fc2's relu and dropout, fc3, the sigmoid, the three log-loss means and the gradient at the logits and at fc2's pre-activations:
// a workgroup per sample, a wave per row of the sample, the rows' loss terms added in rising row order
__global__ __launch_bounds__(SAS_NT) void sasrec_out_kernel(const SasrecArgs a) {
  __shared__ float s_term[4 * 256];      // per row of the sample (2 T - 2 <= 1024 checked by the launcher)
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, T = a.T;
  const SasRows n = sas_rows(a.B, T, a.share);
  const int npos = T - 1, nneg = a.share ? 0 : T - 2, nrow = npos + nneg + 1;
  const bool drop = a.keep < 1.f;
  const uint64_t seed = a.seed_dev ? *a.seed_dev : a.seed;
  const float w0 = a.W3[lane], w1 = lane + 64 < SAS_FC2 ? a.W3[lane + 64] : 0.f, b3 = a.b3[0];
  const float ipos = 1.0f / (float)npos, ineg = 1.0f / (float)(T - 2), ibg = 1.0f / (float)a.Bglobal;
  for (int k = wave; k < nrow; k += SAS_NT / 64) {
    int app; int64_t r, local;
    if (k < npos) { app = 0; local = (int64_t)b * npos + k; r = local; }
    else if (k < npos + nneg) { app = 1; local = (int64_t)b * nneg + (k - npos); r = n.P + local; }
    else { app = 2; local = b; r = n.P + n.Nn + b; }
    const float* z = a.z2 + r * SAS_FC2;
    float f[2];
    float part = 0.f;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int j = lane + 64 * e;
      f[e] = 0.f;
      if (j < SAS_FC2) {
        float v = fmaxf(z[j], 0.f);
        if (drop) {
          const bool on = a.mask1 ? a.mask1[r * SAS_FC2 + j] != 0
                                  : hash_uniform(sas_head_stream(seed, app, 1), (uint64_t)(local * SAS_FC2 + j)) < a.keep;
          v = on ? v / a.keep : 0.f;
        }
        f[e] = v;
        a.f2[r * SAS_FC2 + j] = v;
        part = fmaf(v, e ? w1 : w0, part);
      }
    }
    const float zl = wave_sum(part) + b3;
    // (1 - y as sigmoid(-z): exact where 1.0f - y has lost its digits)
    const float pr = sigmoidf_(zl), qr = sigmoidf_(-zl);
    float term, dl;
    if (app == 2) {
      const float lab = (float)a.label[b];
      term = -lab * logf(pr + SCORE_LOGLOSS_EPS) - (1.0f - lab) * logf(qr + SCORE_LOGLOSS_EPS);
      dl = (-lab / (pr + SCORE_LOGLOSS_EPS) + (1.0f - lab) / (qr + SCORE_LOGLOSS_EPS)) * ibg * pr * qr;
      if (lane == 0) { a.logit[b] = zl; a.ypred[b] = pr; }
    } else {
      const bool pos = app == 0, neg = app == 1 || (a.share && k >= 1);      // (shared: the positive row t = k + 1 >= 2 is a negative row too)
      term = 0.f; dl = 0.f;
      if (pos) { term += -logf(pr + SCORE_LOGLOSS_EPS) * ipos; dl += -1.0f / (pr + SCORE_LOGLOSS_EPS) * ipos; }
      if (neg) { term += -logf(qr + SCORE_LOGLOSS_EPS) * ineg; dl += 1.0f / (qr + SCORE_LOGLOSS_EPS) * ineg; }
      dl = dl * ibg * pr * qr;
    }
    if (lane == 0) { s_term[k] = term; a.rlogit[r] = zl; a.dlogit[r] = dl; }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int j = lane + 64 * e;
      if (j < SAS_FC2) a.dz2[r * SAS_FC2 + j] = f[e] > 0.f ? dl * (e ? w1 : w0) / a.keep : 0.f;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int k = 0; k < nrow; ++k) s += s_term[k];
    a.lossb[b] = s;
  }
}

static bool sasrec_shape_ok(const SasrecArgs& a) {
  if (a.B <= 0 || a.Bglobal <= 0 || !score_sasrec_fits(a.T, a.C)) return false;
  if (a.Cu <= 0 || a.Dh != 2 * a.C + a.Cu || a.ldx < a.C || a.ldq < a.C + a.Cu) return false;
  if (2 * a.T - 2 > 1024) return false;
  if (!(a.keep > 0.f) || a.keep > 1.f || (a.share != 0) != (a.keep >= 1.f)) return false;
  return a.off_ti >= 0 && a.off_tu >= 0 && a.off_ti + a.C <= a.ldh && a.off_tu + a.Cu <= a.ldh;
}

// (160 KiB of LDS per workgroup: set once per thread, device and kernel, before the first launch that needs more than the default)
#define SAS_MAX_DEVICES 16
static int sasrec_lds(const void* fn, size_t bytes, bool* set) {
  if (bytes <= 48 * 1024) return 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return SCORE_E_BADARG;
  const bool known = dev >= 0 && dev < SAS_MAX_DEVICES;
  if (known && set[dev]) return 0;
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) return (int)e;
  if (known) set[dev] = true;
  return 0;
}

int score_sasrec_attn_fwd(const SasrecArgs& a, hipStream_t s) {
  if (!sasrec_shape_ok(a)) return SCORE_E_SHAPE;
  const size_t lds = (size_t)sas_lds_floats(a.T, a.C) * sizeof(float);
  static thread_local bool attr_set[SAS_MAX_DEVICES] = {};
  SCORE_TRY(sasrec_lds(reinterpret_cast<const void*>(sasrec_attn_fwd_kernel), lds, attr_set));
  hipLaunchKernelGGL(sasrec_attn_fwd_kernel, dim3(a.B), dim3(SAS_NT), lds, s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}

int score_sasrec_attn_bwd(const SasrecArgs& a, hipStream_t s) {
  if (!sasrec_shape_ok(a)) return SCORE_E_SHAPE;
  const size_t lds = (size_t)sas_lds_floats(a.T, a.C) * sizeof(float);
  static thread_local bool attr_set[SAS_MAX_DEVICES] = {};
  SCORE_TRY(sasrec_lds(reinterpret_cast<const void*>(sasrec_attn_bwd_kernel), lds, attr_set));
  hipLaunchKernelGGL(sasrec_attn_bwd_kernel, dim3(a.B), dim3(SAS_NT), lds, s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}

int score_sasrec_fan(const SasrecArgs& a, hipStream_t s) {
  if (!sasrec_shape_ok(a)) return SCORE_E_SHAPE;
  const SasRows n = sas_rows(a.B, a.T, a.share);
  hipLaunchKernelGGL(sasrec_fan_kernel, dim3((unsigned)cdiv64(n.R * SAS_FC1, 256)), dim3(256), 0, s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}

int score_sasrec_fold(const SasrecArgs& a, hipStream_t s) {
  if (!sasrec_shape_ok(a)) return SCORE_E_SHAPE;
  const SasRows n = sas_rows(a.B, a.T, a.share);
  hipLaunchKernelGGL(sasrec_fold_kernel, dim3((unsigned)cdiv64((n.P + a.B) * SAS_FC1, 256)), dim3(256), 0, s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}

int score_sasrec_out(const SasrecArgs& a, hipStream_t s) {
  if (!sasrec_shape_ok(a)) return SCORE_E_SHAPE;
  hipLaunchKernelGGL(sasrec_out_kernel, dim3(a.B), dim3(SAS_NT), 0, s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}
