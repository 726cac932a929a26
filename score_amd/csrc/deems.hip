// The DEEMS point baseline's two-tower head (point_models/point_model.py:281-311): two build_fc_net towers -- bn (inference form)
// -> fc 200 relu dropout -> fc 80 relu dropout -> fc 1 -> sigmoid -- over [h_u | target_user] and [h_i | target_item], each with
// variables and dropout masks of its own, meeting in y_pred = (y_u + y_i) / 2, the log-loss of y_pred and the consistency term
// 0.05 (y_i - y_u)^2 that the reference reports with the loss but does not train on (:299-300: train_step is built first).
//
// The two head inputs are column ranges of ONE row [h_u | target_user | h_i | target_item] of `ld` floats (so the target-row
// kernels and dhead work as for every other model type); a tower reads and writes its range with the row stride.
//
// Forward, ONE launch (deems_head_fwd_kernel): a workgroup of 8 waves owns 16 samples, waves 0-3 run the user tower and waves 4-7
// the item tower side by side -- each the chain of head_fwd_fused_kernel (head_fused.hip) on v_mfma_f32_16x16x4_f32 from LDS with
// the weights streamed from L2 --, the two logits meet in LDS, and the kernel leaves everything the backward pass starts from.
// At the reference's B = 200 there are 13 workgroups: what counts is the dependent chain of one, and the towers' chains overlap.
// Backward, ONE launch: the body of head_bwd_fused_kernel per (row tile, tower).  No atomics; every sum in a fixed order.
#include "common.h"
#include "kernels.h"
#include "cell.h"
#include "head_tiles.h"

namespace {

constexpr int DM_NW = 4;                        // waves per tower
constexpr int DM_NTH = 64 * DM_NW;              // threads per tower
constexpr int DM_N1 = 200, DM_N2 = 80;          // build_fc_net's widths
constexpr int DM_LD1 = ((DM_N1 + 15) & ~15) + 4, DM_LD2 = ((DM_N2 + 15) & ~15) + 4;
constexpr int DM_HDR = 64;                      // floats in front of the towers' tiles: the logits [2][16], their gradients [2][16]

__host__ __device__ inline int dm_ld0(int Dh) { return ((Dh + 15) & ~15) + 4; }
__host__ __device__ inline int dm_tower_floats(int Dh) { return HF_ROWS * (dm_ld0(Dh) + DM_LD1 + DM_LD2); }

// A sample's outputs from its two logits: y_u, y_i, y_pred; the loss term, scaled so that the mean over Bglobal that the loss
// reduction takes (head.hip loss_final_kernel) yields mean(log-loss) + SUM(consistency); and dL/d logit of each tower for
// L = the log-loss alone (eps as logloss_term; the consistency term has no gradient in the reference)
struct DeemsOut { float yu, yi, y, lossb, dlu, dli; };
__device__ __forceinline__ DeemsOut deems_combine(float zu, float zi, float lab, int Bglobal) {
  DeemsOut o;
  o.yu = sigmoidf_(zu); o.yi = sigmoidf_(zi);
  o.y = 0.5f * (o.yu + o.yi);
  const float d = o.yi - o.yu;
  o.lossb = logloss_term(o.y, lab) + 0.05f * (d * d) * (float)Bglobal;
  const float dy = (-lab / (o.y + SCORE_LOGLOSS_EPS) + (1.0f - lab) / (1.0f - o.y + SCORE_LOGLOSS_EPS)) / (float)Bglobal;
  o.dlu = dy * 0.5f * (o.yu * (1.0f - o.yu));
  o.dli = dy * 0.5f * (o.yi * (1.0f - o.yi));
  return o;
}
__device__ __forceinline__ void deems_store(const DeemsArgs& a, int row, const float zu, const float zi, const DeemsOut& o) {
  a.t[0].logit[row] = zu; a.t[1].logit[row] = zi;
  a.t[0].y[row] = o.yu; a.t[1].y[row] = o.yi;
  a.y_pred[row] = o.y; a.lossb[row] = o.lossb;
  a.t[0].dlogit[row] = o.dlu; a.t[1].dlogit[row] = o.dli;
}

__global__ __launch_bounds__(2 * DM_NTH) void deems_head_fwd_kernel(const DeemsArgs a) {
  extern __shared__ float sm[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tw = __builtin_amdgcn_readfirstlane(wave / DM_NW);       // the tower of this wave
  const int wv = wave - tw * DM_NW, ttid = tid - tw * DM_NTH;
  const int lc = lane & 15, lq = lane >> 4;
  const int b0 = blockIdx.x * HF_ROWS;
  const DeemsTower& t = a.t[tw];
  const int Dh = t.Dh, H = a.H, N1 = DM_N1, N2 = DM_N2;
  const int Kp0 = (Dh + 15) & ~15, LD0 = Kp0 + 4;
  constexpr int Kp1 = (DM_N1 + 15) & ~15, LD1 = DM_LD1, Kp2 = (DM_N2 + 15) & ~15, LD2 = DM_LD2;
  (void)Kp2;
  float* zs = sm;                          // [2][16] logits
  float* dls = sm + 2 * HF_ROWS;           // [2][16] dL/d logit
  float* xs = sm + DM_HDR + (tw ? dm_tower_floats(a.t[0].Dh) : 0);      // [16][LD0] bn output
  float* f1s = xs + HF_ROWS * LD0;         // [16][LD1]
  float* f2s = f1s + HF_ROWS * LD1;        // [16][LD2]
  // the item tower draws from a stream of its own
  const uint64_t sbase = (a.seed_dev ? *a.seed_dev : a.seed0) ^ (tw ? SCORE_DEEMS_ITEM_SEED : 0ull);
  const uint64_t seed0 = sbase, seed1 = sbase ^ 0x5DEECE66Dull;
  const int drop = a.keep < 1.f ? 1 : 0;

  for (int e = ttid; e < HF_ROWS * (LD0 + LD1 + LD2); e += DM_NTH) xs[e] = 0.f;      // (the zero padding of every layer's K)
  __syncthreads();
  // bn: y = x * (gamma * rs) + beta.  The first H columns of x are the recurrence's final state, stored into the row on the way
  {
    const int n4 = Dh >> 2, total = HF_ROWS * n4;
    for (int e = ttid; e < total; e += DM_NTH) {
      const int i = e / n4, j = (e - i * n4) * 4;
      const int row = min(b0 + i, a.B - 1);
      float* xrow = a.x + (int64_t)row * a.ld + t.col + j;
      const bool from_h = t.h != nullptr && j < H;
      const float4 xv = ld4(from_h ? t.h + (int64_t)row * H + j : xrow);
      const float4 gv = ld4(t.gamma + j), bv = ld4(t.beta + j);
      float4 v;
      v.x = xv.x * (gv.x * a.rs) + bv.x; v.y = xv.y * (gv.y * a.rs) + bv.y;
      v.z = xv.z * (gv.z * a.rs) + bv.z; v.w = xv.w * (gv.w * a.rs) + bv.w;
      if (b0 + i < a.B) {
        if (from_h) st4(xrow, xv);
        st4(a.bn + (int64_t)row * a.ld + t.col + j, v);
        *reinterpret_cast<float4*>(xs + i * LD0 + j) = v;
      }
    }
  }
  __syncthreads();

  // fc1: 13 tiles of 16 columns, tiles wv, wv + 4, wv + 8, wv + 12 of this tower's four waves in one pass
  {
    constexpr int nt1 = (DM_N1 + 15) >> 4;
    hf_f32x4 acc[4];
    int n0[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      acc[q] = (hf_f32x4){0.f, 0.f, 0.f, 0.f};
      const int tile = wv + DM_NW * q;
      n0[q] = tile < nt1 ? tile * 16 : -1;
    }
    hf_tiles<4>(acc, xs, LD0, Kp0, Dh, t.W1, N1, n0, N1, lc, lq);
    float bias1[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) bias1[q] = t.b1[min(max(n0[q] + lc, 0), N1 - 1)];      // clamped, unconditional
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int col = n0[q] + lc;
      if (n0[q] < 0 || col >= N1) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = lq * 4 + r, row = b0 + i;
        const float v = relu_dropout(acc[q][r], bias1[q], drop, a.keep, t.mask0, seed0, min(row, a.B - 1), col, N1);
        f1s[i * LD1 + col] = v;
        if (row < a.B) t.f1[(int64_t)row * N1 + col] = v;
      }
    }
  }
  __syncthreads();

  // fc2: 5 tiles, wv and wv + 4
  {
    constexpr int nt2 = (DM_N2 + 15) >> 4;
    hf_f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const int n0[2] = {wv * 16, wv + DM_NW < nt2 ? (wv + DM_NW) * 16 : -1};
    hf_tiles<2>(acc, f1s, LD1, Kp1, N1, t.W2, N2, n0, N2, lc, lq);
    float bias2[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) bias2[q] = t.b2[min(max(n0[q] + lc, 0), N2 - 1)];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int col = n0[q] + lc;
      if (n0[q] < 0 || col >= N2) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = lq * 4 + r, row = b0 + i;
        const float v = relu_dropout(acc[q][r], bias2[q], drop, a.keep, t.mask1, seed1, min(row, a.B - 1), col, N2);
        f2s[i * LD2 + col] = v;
        if (row < a.B) t.f2[(int64_t)row * N2 + col] = v;
      }
    }
  }
  __syncthreads();

  // fc3: four lanes per sample, fixed-order partial sums; the two towers' logits meet in LDS
  if (wv == 0) {
    const int i = lane >> 2, part = lane & 3;
    float s = 0.f;
    for (int n = part; n < N2; n += 4) s = fmaf(f2s[i * LD2 + n], t.W3[n], s);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if (part == 0) zs[tw * HF_ROWS + i] = s + t.b3[0];
  }
  __syncthreads();
  if (tid < HF_ROWS) {
    const int row = b0 + tid;
    float dlu = 0.f, dli = 0.f;
    if (row < a.B) {
      const float zu = zs[tid], zi = zs[HF_ROWS + tid];
      const DeemsOut o = deems_combine(zu, zi, (float)a.label[row], a.Bglobal);
      deems_store(a, row, zu, zi, o);
      dlu = o.dlu; dli = o.dli;
    }
    dls[tid] = dlu; dls[HF_ROWS + tid] = dli;
  }
  __syncthreads();
  // dz2[b][n] = [f2 > 0] * dlogit[b] * w3[n] / keep: what each tower's backward starts from
  for (int e = ttid; e < HF_ROWS * N2; e += DM_NTH) {
    const int i = e / N2, n = e - i * N2, row = b0 + i;
    const float q = dls[tw * HF_ROWS + i] * t.W3[n] / a.keep;
    if (row < a.B) t.dz2[(int64_t)row * N2 + n] = f2s[i * LD2 + n] > 0.f ? q : 0.f;
  }
}

// the layer-by-layer form's pieces: both towers' bn in one launch over the whole rows, its backward, and the combine
__global__ void deems_bn_fwd_kernel(const DeemsArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)a.B * a.ld) return;
  const int64_t row = i / a.ld;
  const int c = (int)(i - row * a.ld);
  const DeemsTower& t = a.t[c >= a.t[1].col ? 1 : 0];
  const int j = c - t.col;
  float xv = a.x[i];
  if (t.h != nullptr && j < a.H) { xv = t.h[row * a.H + j]; a.x[i] = xv; }
  a.bn[i] = xv * (t.gamma[j] * a.rs) + t.beta[j];
}
// dhead = dbn * gamma * rs ; tmp = dbn * x * rs  (d gamma = colsum(tmp), d beta = colsum(dbn))
__global__ void deems_bn_bwd_kernel(const DeemsArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)a.B * a.ld) return;
  const int c = (int)(i % a.ld);
  const DeemsTower& t = a.t[c >= a.t[1].col ? 1 : 0];
  const float d = a.dbn[i];
  a.dhead[i] = d * (t.gamma[c - t.col] * a.rs);
  a.tmp[i] = d * (a.x[i] * a.rs);
}
__global__ void deems_out_kernel(const DeemsArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  const float zu = a.t[0].logit[b], zi = a.t[1].logit[b];
  deems_store(a, b, zu, zi, deems_combine(zu, zi, (float)a.label[b], a.Bglobal));
}

struct DeemsBwdArgs { HeadBwdArgs t[2]; };
__global__ __launch_bounds__(64 * HF_NW) void deems_head_bwd_kernel(const DeemsBwdArgs a) {
  head_bwd_body(a.t[blockIdx.y], 0, 1);
}

// rows of `ld` floats holding both towers' column ranges, every range and the state width a multiple of four floats
bool deems_shape_ok(const DeemsArgs& a) {
  if (a.B <= 0 || a.H <= 0 || (a.H & 3) || (a.ld & 3)) return false;
  for (int k = 0; k < 2; ++k)
    if (a.t[k].Dh <= 0 || (a.t[k].Dh & 3) || (a.t[k].col & 3) || a.t[k].col < 0 || a.t[k].col + a.t[k].Dh > a.ld || a.t[k].Dh < a.H)
      return false;
  return a.t[0].col + a.t[0].Dh <= a.t[1].col;
}

}  // namespace

bool score_deems_head_fwd_fits(int Dh_user, int Dh_item) {
  return Dh_user > 0 && Dh_item > 0 &&
         (size_t)(DM_HDR + dm_tower_floats(Dh_user) + dm_tower_floats(Dh_item)) * sizeof(float) <= 150 * 1024;
}

// Returns SCORE_E_SHAPE when the towers do not fit the kernel's LDS (the caller then runs the layer-by-layer form).
int score_deems_head_fwd(const DeemsArgs& a, hipStream_t s) {
  if (!deems_shape_ok(a)) return SCORE_E_BADARG;
  if (!score_deems_head_fwd_fits(a.t[0].Dh, a.t[1].Dh)) return SCORE_E_SHAPE;
  const size_t lds = (size_t)(DM_HDR + dm_tower_floats(a.t[0].Dh) + dm_tower_floats(a.t[1].Dh)) * sizeof(float);
  static thread_local bool attr_set = false;
  if (!attr_set && lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(deems_head_fwd_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  hipLaunchKernelGGL(deems_head_fwd_kernel, dim3((a.B + HF_ROWS - 1) / HF_ROWS), dim3(2 * DM_NTH), lds, s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}

int score_deems_bn_fwd(const DeemsArgs& a, hipStream_t s) {
  if (!deems_shape_ok(a) || a.t[0].col != 0 || a.t[1].col + a.t[1].Dh != a.ld || a.t[0].Dh != a.t[1].col) return SCORE_E_BADARG;
  hipLaunchKernelGGL(deems_bn_fwd_kernel, dim3((unsigned)cdiv64((int64_t)a.B * a.ld, 256)), dim3(256), 0, s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}
int score_deems_bn_bwd(const DeemsArgs& a, hipStream_t s) {
  if (!deems_shape_ok(a) || a.t[0].col != 0 || a.t[1].col + a.t[1].Dh != a.ld || a.t[0].Dh != a.t[1].col) return SCORE_E_BADARG;
  hipLaunchKernelGGL(deems_bn_bwd_kernel, dim3((unsigned)cdiv64((int64_t)a.B * a.ld, 256)), dim3(256), 0, s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}
int score_deems_out(const DeemsArgs& a, hipStream_t s) {
  if (a.B <= 0) return SCORE_E_BADARG;
  hipLaunchKernelGGL(deems_out_kernel, dim3((a.B + 63) / 64), dim3(64), 0, s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}
// both towers' dz1, d bn, d head input and the d gamma terms from their dz2 (what head_bwd_fused_kernel does for one head)
int score_deems_head_bwd(const DeemsArgs& a, hipStream_t s) {
  if (!deems_shape_ok(a)) return SCORE_E_BADARG;
  DeemsBwdArgs b;
  for (int k = 0; k < 2; ++k) {
    const DeemsTower& t = a.t[k];
    HeadBwdArgs& h = b.t[k];
    h.B = a.B; h.Dh = t.Dh; h.ld = a.ld; h.dz2 = t.dz2; h.W2 = t.W2; h.f1 = t.f1; h.keep = a.keep; h.W1 = t.W1;
    h.x = a.x + t.col; h.gamma = t.gamma; h.rs = a.rs; h.dz1 = t.dz1; h.dbn = a.dbn + t.col; h.dhead = a.dhead + t.col;
    h.tmp = a.tmp + t.col;
  }
  hipLaunchKernelGGL(deems_head_bwd_kernel, dim3((a.B + HF_ROWS - 1) / HF_ROWS, 2), dim3(64 * HF_NW), 0, s, b);
  SCORE_CHECK_LAUNCH();
  return 0;
}
