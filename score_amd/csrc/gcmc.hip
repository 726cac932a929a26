// The bilinear two-way softmax head of the GCMC slice baseline (slice_model.py:199-201) and its backward pass:
//   p = h_i . W4, n = h_i . W5 (dense_4 / dense_5, [H, H], no bias), a = <p, h_u>, c = <n, h_u>,
//   y = exp(a) / (exp(a) + exp(c))            (the literal fp32 form: where an exp overflows, IEEE gives what TF gives)
// plus the per-sample log-loss term (build_logloss, :77-86) and g = dL/dy * y (1 - y) / B_global, the gradient of a (that of
// c is -g).  The backward pass:  dh_u = g p - g n,  dh_i = (g h_u) W4^T - (g h_u) W5^T, and the rows +-g h_u that the dense
// gradients dW4 = h_i^T (g h_u), dW5 = -h_i^T (g h_u) are computed from (the engine queues those products, K = B).
//
// Both kernels: 256 threads, H <= 256.  The threads form G = 256 / H groups of H lanes, lane k of a group owning column k;
// group q handles the samples q, q + G, ..., q + 7G of the workgroup's slice of SB = 8G samples, whose rows sit in LDS.  W4 and
// W5 (512 KB at H = 256) are read from L2: the forward pass reads them row by row (a row across the lanes of a group), the
// backward pass row j by lane j.  Every sum runs in a fixed order: the results are the same bits on every run.
#include "common.h"
#include "kernels.h"
#include "cell.h"

#define GCMC_NT 256
#define GCMC_PER 8        // samples per thread

__global__ __launch_bounds__(GCMC_NT) void gcmc_head_fwd_kernel(int B, int H, const float* __restrict__ hu,
                                                                const float* __restrict__ hi, const float* __restrict__ W4,
                                                                const float* __restrict__ W5, const int32_t* __restrict__ label,
                                                                float* __restrict__ y, float* __restrict__ lossb,
                                                                float* __restrict__ p_out, float* __restrict__ n_out,
                                                                float* __restrict__ g_out, float inv_bglobal) {
  __shared__ float s_hi[GCMC_PER * GCMC_NT], s_pu[GCMC_PER * GCMC_NT], s_nu[GCMC_PER * GCMC_NT];
  const int G = GCMC_NT / H, SB = GCMC_PER * G;
  const int b0 = blockIdx.x * SB;
  const int nb = min(SB, B - b0);
  const int tid = threadIdx.x;
  for (int i = tid; i < SB * H; i += GCMC_NT) {
    const int s = i / H;
    s_hi[i] = s < nb ? hi[(int64_t)(b0 + s) * H + (i - s * H)] : 0.f;
  }
  __syncthreads();
  const int q = tid / H, k = tid - q * H;
  if (q < G) {
    float p[GCMC_PER], n[GCMC_PER];
#pragma unroll
    for (int r = 0; r < GCMC_PER; ++r) { p[r] = 0.f; n[r] = 0.f; }
    for (int j = 0; j < H; ++j) {
      const float w4 = W4[(int64_t)j * H + k], w5 = W5[(int64_t)j * H + k];
#pragma unroll
      for (int r = 0; r < GCMC_PER; ++r) {
        const float h = s_hi[(q + r * G) * H + j];
        p[r] = fmaf(h, w4, p[r]);
        n[r] = fmaf(h, w5, n[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < GCMC_PER; ++r) {
      const int s = q + r * G;
      float u = 0.f;
      if (s < nb) {
        const int64_t o = (int64_t)(b0 + s) * H + k;
        u = hu[o];
        p_out[o] = p[r];
        n_out[o] = n[r];
      }
      s_pu[s * H + k] = p[r] * u;
      s_nu[s * H + k] = n[r] * u;
    }
  }
  __syncthreads();
  // a and c: one wave per sample, lanes over k in order, then a fixed butterfly
  const int wave = tid >> 6, lane = tid & 63;
  for (int s = wave; s < nb; s += GCMC_NT / 64) {
    float a = 0.f, c = 0.f;
    for (int kk = lane; kk < H; kk += 64) { a += s_pu[s * H + kk]; c += s_nu[s * H + kk]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); c += __shfl_xor(c, o, 64); }
    if (lane == 0) {
      const int b = b0 + s;
      const float ea = expf(a), ec = expf(c);
      const float pr = ea / (ea + ec);
      const float lab = (float)label[b];
      const float eps = 1e-7f;
      y[b] = pr;
      lossb[b] = logloss_term(pr, lab);
      const float dp = (-lab / (pr + eps) + (1.0f - lab) / (1.0f - pr + eps)) * inv_bglobal;
      g_out[b] = dp * pr * (1.0f - pr);
    }
  }
}

__global__ __launch_bounds__(GCMC_NT) void gcmc_head_bwd_kernel(int B, int H, const float* __restrict__ hu,
                                                                const float* __restrict__ W4, const float* __restrict__ W5,
                                                                const float* __restrict__ p_in, const float* __restrict__ n_in,
                                                                const float* __restrict__ g_in, float* __restrict__ dhu,
                                                                float* __restrict__ dhi, float* __restrict__ gpos,
                                                                float* __restrict__ gneg) {
  __shared__ float s_gu[GCMC_PER * GCMC_NT];
  const int G = GCMC_NT / H, SB = GCMC_PER * G;
  const int b0 = blockIdx.x * SB;
  const int nb = min(SB, B - b0);
  const int tid = threadIdx.x;
  for (int i = tid; i < SB * H; i += GCMC_NT) {
    const int s = i / H, k = i - s * H;
    float gu = 0.f;
    if (s < nb) {
      const int64_t o = (int64_t)(b0 + s) * H + k;
      const float g = g_in[b0 + s];
      gu = g * hu[o];
      dhu[o] = g * p_in[o] - g * n_in[o];
      gpos[o] = gu;
      gneg[o] = -gu;
    }
    s_gu[i] = gu;
  }
  __syncthreads();
  const int q = tid / H, j = tid - q * H;
  if (q >= G) return;
  float acc[GCMC_PER];
#pragma unroll
  for (int r = 0; r < GCMC_PER; ++r) acc[r] = 0.f;
  const float* w4 = W4 + (int64_t)j * H;
  const float* w5 = W5 + (int64_t)j * H;
  if ((H & 3) == 0) {
    for (int k = 0; k < H; k += 4) {
      const float4 a = ld4(w4 + k), b = ld4(w5 + k);
      const float d[4] = {a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w};
#pragma unroll
      for (int r = 0; r < GCMC_PER; ++r) {
        const float* gu = s_gu + (q + r * G) * H + k;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r] = fmaf(gu[e], d[e], acc[r]);
      }
    }
  } else {
    for (int k = 0; k < H; ++k) {
      const float d = w4[k] - w5[k];
#pragma unroll
      for (int r = 0; r < GCMC_PER; ++r) acc[r] = fmaf(s_gu[(q + r * G) * H + k], d, acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < GCMC_PER; ++r) {
    const int s = q + r * G;
    if (s < nb) dhi[(int64_t)(b0 + s) * H + j] = acc[r];
  }
}

static inline int gcmc_blocks(int B, int H) { return (B + GCMC_PER * (GCMC_NT / H) - 1) / (GCMC_PER * (GCMC_NT / H)); }

int score_launch_gcmc_head_fwd(int B, int H, const float* hu, const float* hi, const float* W4, const float* W5,
                               const int32_t* label, float* y, float* lossb, float* p, float* n, float* g, int Bglobal,
                               hipStream_t s) {
  if (B <= 0 || H <= 0 || H > GCMC_NT || Bglobal <= 0) return SCORE_E_SHAPE;
  hipLaunchKernelGGL(gcmc_head_fwd_kernel, dim3(gcmc_blocks(B, H)), dim3(GCMC_NT), 0, s, B, H, hu, hi, W4, W5, label, y, lossb,
                     p, n, g, 1.0f / (float)Bglobal);
  SCORE_CHECK_LAUNCH();
  return 0;
}

int score_launch_gcmc_head_bwd(int B, int H, const float* hu, const float* W4, const float* W5, const float* p, const float* n,
                               const float* g, float* dhu, float* dhi, float* gpos, float* gneg, hipStream_t s) {
  if (B <= 0 || H <= 0 || H > GCMC_NT) return SCORE_E_SHAPE;
  hipLaunchKernelGGL(gcmc_head_bwd_kernel, dim3(gcmc_blocks(B, H)), dim3(GCMC_NT), 0, s, B, H, hu, W4, W5, p, n, g, dhu, dhi,
                     gpos, gneg);
  SCORE_CHECK_LAUNCH();
  return 0;
}
