// The SVD++ point baseline (point_models/point_model.py:167-198) between the gather and the row scatter.  Per sample, with one
// scalar weight per feature field (wu_i, wi_j) and X_t the gathered history row [Fi * D]:
//   p_u = sum_i wu_i tu[i],  p_i = sum_j wi_j ti[j],  s_t = [t < len] sum_j wi_j X_t[j]   (each [D]),
//   nb = sum_t s_t,  c_d = sum_t |s_t,d|,  n = max_d c_d   (tf.norm(s, 1, (1, 2)): the matrix 1-norm),  q = nb / sqrt(n),
//   z = <p_i, p_u + q>,  y = sigmoid(z), and the log-loss terms of the sample.
// A sample with n = 0 (length <= 0, or every live row the dummy row) gets q = 0 / 0 and a NaN prediction, as in TF.
//
// Forward: ONE launch, a workgroup of 256 threads per sample.  The threads form G = 256 / D row groups of D lanes: lane d of
// group g takes column d of the rows t = g, g + G, ...  -- at D = 16 a wave covers four whole rows of 256 B --, sums its rows in
// rising t, and the groups are added in rising g; the sums over D run on one wave's fixed butterfly.  Saved for the backward
// pass: p_u, p_i, nb, share_d = [c_d == n] / ties, n and ties; s_t is not stored.
// Backward: ONE launch of the same shape.  s_t is recomputed from X by the same expression (the same bits, so sign(s) and the
// forward pass's c_d agree), d s_t,d = [t < len] (dnb_d + dc_d sign(s_t,d)), dX_t[j] = wi_j d s_t (every one of the ldx columns
// written, an exact 0 past the length), the target rows' gradients into dhead, and per sample the Fu + Fi weight-gradient
// partials, reduced over the workgroup by a fixed tree: the batch sum is the engine's queued column sum.  No atomics anywhere.
#include <math.h>
#include "common.h"
#include "kernels.h"
#include "cell.h"

#define SVDPP_NT 256
#define SVDPP_DMAX SCORE_SVDPP_DMAX
#define SVDPP_FMAX SCORE_SVDPP_FMAX

// rows of the sample that are live: tf.sequence_mask(length, T)
__device__ __forceinline__ int svdpp_live(int len, int T) { return len <= 0 ? 0 : min(len, T); }
// s_t,d of one row: x points at column d of the row's first field.  The ONE expression both passes evaluate
__device__ __forceinline__ float svdpp_row(const float* __restrict__ x, const float (&wi)[SVDPP_FMAX], int Fi, int D) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < SVDPP_FMAX; ++j)
    if (j < Fi) s = fmaf(wi[j], x[j * D], s);
  return s;
}
// sum over the D <= 128 entries of v (LDS) on one wave: lane l takes v[l] + v[l + 64], then the fixed butterfly
__device__ __forceinline__ float svdpp_wave_dsum(const float* v, int lane, int D) {
  const float a = lane < D ? v[lane] : 0.f, b = lane + SCORE_WAVE < D ? v[lane + SCORE_WAVE] : 0.f;
  return wave_sum(a + b);
}

__global__ __launch_bounds__(SVDPP_NT) void svdpp_fwd_kernel(const SvdppArgs a) {
  __shared__ float s_nb[SVDPP_NT], s_c[SVDPP_NT];
  __shared__ float s_v[5 * SVDPP_DMAX];      // p_u, p_i, nb, c, p_i (p_u + q)
  __shared__ float s_w[2 * SVDPP_FMAX];
  const int b = blockIdx.x, tid = threadIdx.x, D = a.D, Fu = a.Fu, Fi = a.Fi, T = a.T;
  const int G = SVDPP_NT / D, g = tid / D, d = tid - g * D;
  if (tid < Fu) s_w[tid] = a.wu[4 * tid];
  else if (tid < Fu + Fi) s_w[tid] = a.wi[4 * (tid - Fu)];
  __syncthreads();
  float wi[SVDPP_FMAX];
#pragma unroll
  for (int j = 0; j < SVDPP_FMAX; ++j) wi[j] = j < Fi ? s_w[Fu + j] : 0.f;
  const int L = svdpp_live(a.length[b], T);
  float nb = 0.f, c = 0.f;
  if (g < G) {
    const float* __restrict__ X = a.X + (int64_t)b * T * a.ldx + d;
    for (int t = g; t < L; t += G) {
      const float s = svdpp_row(X + (int64_t)t * a.ldx, wi, Fi, D);
      nb += s;
      c += fabsf(s);
    }
  }
  s_nb[tid] = nb; s_c[tid] = c;
  __syncthreads();
  if (tid < D) {
    float vn = 0.f, vc = 0.f;
    for (int k = 0; k < G; ++k) { vn += s_nb[k * D + tid]; vc += s_c[k * D + tid]; }
    const float* tu = a.tu + (int64_t)b * a.ldq + tid;
    const float* ti = a.ti + (int64_t)b * a.ldq + tid;
    float pu = 0.f, pi = 0.f;
    for (int i = 0; i < Fu; ++i) pu = fmaf(s_w[i], tu[i * D], pu);
    for (int j = 0; j < Fi; ++j) pi = fmaf(s_w[Fu + j], ti[j * D], pi);
    s_v[tid] = pu; s_v[SVDPP_DMAX + tid] = pi; s_v[2 * SVDPP_DMAX + tid] = vn; s_v[3 * SVDPP_DMAX + tid] = vc;
  }
  __syncthreads();
  if (tid < SCORE_WAVE) {      // one wave: the matrix 1-norm, its ties, q and the dot product
    const int lane = tid;
    const float* cs = s_v + 3 * SVDPP_DMAX;
    const float c0 = lane < D ? cs[lane] : 0.f, c1 = lane + SCORE_WAVE < D ? cs[lane + SCORE_WAVE] : 0.f;      // (c_d >= 0)
    const float n = wave_max(fmaxf(c0, c1));
    const float ties = wave_sum((lane < D && c0 == n ? 1.f : 0.f) + (lane + SCORE_WAVE < D && c1 == n ? 1.f : 0.f));
    const float rn = sqrtf(n);
    float* act = a.act + (int64_t)b * score_svdpp_act_floats(D);
    for (int e = lane; e < D; e += SCORE_WAVE) {
      const float pu = s_v[e], pi = s_v[SVDPP_DMAX + e], vn = s_v[2 * SVDPP_DMAX + e];
      s_v[4 * SVDPP_DMAX + e] = pi * (pu + vn / rn);
      act[e] = pu; act[D + e] = pi; act[2 * D + e] = vn; act[3 * D + e] = cs[e] == n ? 1.0f / ties : 0.f;
    }
    const float z = svdpp_wave_dsum(s_v + 4 * SVDPP_DMAX, lane, D);      // (a wave's own LDS writes are visible to it in order)
    if (lane == 0) {
      act[4 * D] = n; act[4 * D + 1] = ties; act[4 * D + 2] = 0.f; act[4 * D + 3] = 0.f;
      // tf.losses.log_loss's terms with 1 - y taken as sigmoid(-z): the logits of this model reach +-20 at TF's own initial values
      // (no head in front of the sigmoid), where 1.0f - y has no correct digit left while sigmoid(-z) has them all
      const float pr = sigmoidf_(z), qr = sigmoidf_(-z);
      const float lab = (float)a.label[b];
      a.logit[b] = z;
      a.y[b] = pr;
      a.lossb[b] = -lab * logf(pr + SCORE_LOGLOSS_EPS) - (1.0f - lab) * logf(qr + SCORE_LOGLOSS_EPS);
      a.dlogit[b] = (-lab / (pr + SCORE_LOGLOSS_EPS) + (1.0f - lab) / (qr + SCORE_LOGLOSS_EPS)) / (float)a.Bglobal * pr * qr;
    }
  }
}

__global__ __launch_bounds__(SVDPP_NT) void svdpp_bwd_kernel(const SvdppArgs a) {
  __shared__ float s_v[5 * SVDPP_DMAX];      // dnb, dc, dp_i, dp_u, dq nb
  __shared__ float s_w[2 * SVDPP_FMAX];
  __shared__ float s_red[(SVDPP_NT / SCORE_WAVE) * 2 * SVDPP_FMAX];
  const int b = blockIdx.x, tid = threadIdx.x, D = a.D, Fu = a.Fu, Fi = a.Fi, T = a.T;
  const int G = SVDPP_NT / D, g = tid / D, d = tid - g * D;
  if (tid < Fu) s_w[tid] = a.wu[4 * tid];
  else if (tid < Fu + Fi) s_w[tid] = a.wi[4 * (tid - Fu)];
  const float* act = a.act + (int64_t)b * score_svdpp_act_floats(D);
  if (tid < SCORE_WAVE) {      // one wave: dp_i, dp_u, dnb and, through <dq, nb>, dn and dc
    const int lane = tid;
    const float dz = a.dlogit[b], n = act[4 * D], rn = sqrtf(n);
    for (int e = lane; e < D; e += SCORE_WAVE) {
      const float pu = act[e], pi = act[D + e], vn = act[2 * D + e];
      const float dq = dz * pi;
      s_v[e] = dq / rn;                                        // dnb
      s_v[2 * SVDPP_DMAX + e] = dz * (pu + vn / rn);           // dp_i
      s_v[3 * SVDPP_DMAX + e] = dq;                            // dp_u (= dq)
      s_v[4 * SVDPP_DMAX + e] = dq * vn;
    }
    const float dot = svdpp_wave_dsum(s_v + 4 * SVDPP_DMAX, lane, D);
    const float dn = -0.5f * dot / (n * rn);
    for (int e = lane; e < D; e += SCORE_WAVE) s_v[SVDPP_DMAX + e] = dn * act[3 * D + e];      // dc
  }
  __syncthreads();
  float wi[SVDPP_FMAX], acc[2 * SVDPP_FMAX];
#pragma unroll
  for (int j = 0; j < SVDPP_FMAX; ++j) wi[j] = j < Fi ? s_w[Fu + j] : 0.f;
#pragma unroll
  for (int j = 0; j < 2 * SVDPP_FMAX; ++j) acc[j] = 0.f;
  const int L = svdpp_live(a.length[b], T);
  if (g < G) {
    const float dnb = s_v[d], dc = s_v[SVDPP_DMAX + d];
    const float* __restrict__ X = a.X + (int64_t)b * T * a.ldx + d;
    float* __restrict__ dX = a.dX + (int64_t)b * T * a.ldx + d;
    for (int t = g; t < T; t += G) {
      const float* x = X + (int64_t)t * a.ldx;
      float* dx = dX + (int64_t)t * a.ldx;
      if (t < L) {
        const float s = svdpp_row(x, wi, Fi, D);
        const float sg = s > 0.f ? 1.f : (s < 0.f ? -1.f : 0.f);
        const float ds = fmaf(dc, sg, dnb);
#pragma unroll
        for (int j = 0; j < SVDPP_FMAX; ++j)
          if (j < Fi) {
            dx[j * D] = wi[j] * ds;
            acc[SVDPP_FMAX + j] = fmaf(ds, x[j * D], acc[SVDPP_FMAX + j]);
          }
      } else {
#pragma unroll
        for (int j = 0; j < SVDPP_FMAX; ++j)
          if (j < Fi) dx[j * D] = 0.f;
      }
    }
  }
  // the columns of the gather's rows that this model does not read
  {
    const int C = Fi * D, extra = a.ldx - C;
    float* dXb = a.dX + (int64_t)b * T * a.ldx;
    for (int i = tid; i < T * extra; i += SVDPP_NT) {
      const int t = i / extra, c = C + i - t * extra;
      dXb[(int64_t)t * a.ldx + c] = 0.f;
    }
  }
  // the target rows: d target_item[j] = wi_j dp_i, d target_user[i] = wu_i dp_u, and their share of the weight gradients
  if (tid < D) {
    const float dpi = s_v[2 * SVDPP_DMAX + tid], dpu = s_v[3 * SVDPP_DMAX + tid];
    const float* tu = a.tu + (int64_t)b * a.ldq + tid;
    const float* ti = a.ti + (int64_t)b * a.ldq + tid;
    float* dh = a.dhead + (int64_t)b * a.ldh + tid;
#pragma unroll
    for (int j = 0; j < SVDPP_FMAX; ++j) {
      if (j < Fi) {
        dh[a.off_ti + j * D] = wi[j] * dpi;
        acc[SVDPP_FMAX + j] = fmaf(dpi, ti[j * D], acc[SVDPP_FMAX + j]);
      }
      if (j < Fu) {
        dh[a.off_tu + j * D] = s_w[j] * dpu;
        acc[j] = dpu * tu[j * D];
      }
    }
  }
  // the 2 x FMAX partials over the workgroup: each wave's butterfly, then the waves in order
  group_sum_n(acc, SCORE_WAVE);
  const int wave = tid >> 6, lane = tid & (SCORE_WAVE - 1);
  if (lane == 0)
#pragma unroll
    for (int j = 0; j < 2 * SVDPP_FMAX; ++j) s_red[wave * 2 * SVDPP_FMAX + j] = acc[j];
  __syncthreads();
  if (tid < Fu + Fi) {
    const int k = tid < Fu ? tid : SVDPP_FMAX + tid - Fu;
    float v = 0.f;
    for (int wv = 0; wv < SVDPP_NT / SCORE_WAVE; ++wv) v += s_red[wv * 2 * SVDPP_FMAX + k];
    a.dwpart[(int64_t)b * (Fu + Fi) + tid] = v;
  }
}

static bool svdpp_shape_ok(const SvdppArgs& a) {
  if (a.B <= 0 || a.T <= 0 || a.Bglobal <= 0 || a.D <= 0 || (a.D & 3) || a.D > SVDPP_DMAX) return false;
  if (a.Fu <= 0 || a.Fi <= 0 || a.Fu > SVDPP_FMAX || a.Fi > SVDPP_FMAX) return false;
  if (a.ldx < a.Fi * a.D || a.ldq < (a.Fu + a.Fi) * a.D || a.ldh < (a.Fu + a.Fi) * a.D) return false;
  return a.off_ti >= 0 && a.off_tu >= 0 && a.off_ti + a.Fi * a.D <= a.ldh && a.off_tu + a.Fu * a.D <= a.ldh;
}

int score_svdpp_fwd(const SvdppArgs& a, hipStream_t s) {
  if (!svdpp_shape_ok(a)) return SCORE_E_SHAPE;
  hipLaunchKernelGGL(svdpp_fwd_kernel, dim3(a.B), dim3(SVDPP_NT), 0, s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}

int score_svdpp_bwd(const SvdppArgs& a, hipStream_t s) {
  if (!svdpp_shape_ok(a)) return SCORE_E_SHAPE;
  hipLaunchKernelGGL(svdpp_bwd_kernel, dim3(a.B), dim3(SVDPP_NT), 0, s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}
