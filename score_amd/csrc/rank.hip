// The point baselines' head over target LINES (score_rank_forward, include/score_hip.h): L lines of C candidate items that share
// one user history.  bn1 is a per-column affine and fc1 is linear, so fc1's pre-activation of sample (l, c) splits by the columns
// of the head input:
//   z1[l, c] = (b1 + bn1(x_line[l]) . W1[line rows])  +  bn1(target_item[l, c]) . W1[item rows]
// The first term needs the line alone: rank_line_kernel computes it ONCE per line, a workgroup per line.  The second is the
// fused head's tile (head_fused.hip) with K = Di instead of Dhead: rank_tile_kernel, a workgroup of 8 waves per (line, 16
// candidates), gathers the candidates' table rows straight into LDS through bn1's affine and runs fc1 (item rows only), fc2, fc3
// and the sigmoid back to back on v_mfma_f32_16x16x4_f32 (exact fp32 products), the weights streamed from L2 (hf_tiles).
//
// Why the line part is a launch of its own and not a prologue of the tile kernel: as a prologue every one of a line's
// ceil(C / 16) tiles would stream W1's line rows again -- as many bytes as the candidate part streams, or more (H + Du against Di
// rows) -- and would do so in front of its first MFMA, on the critical path of every workgroup.  As a launch it is L small
// workgroups behind the history encoder, and a tile reads its line's 200 sums with one load per output column.
//
// No atomics in any sum (the id report is an idempotent OR), every sum in a fixed order: results are reproducible run to run.
// All LDS is dynamic and every carve offset a multiple of 16 bytes.
#include "common.h"
#include "kernels.h"
#include "cell.h"
#include "head_tiles.h"      // hf_tiles and the tile constants

namespace {

constexpr int RL_NW = 4;        // waves of a line workgroup: each sums every fourth row of W1

__device__ __forceinline__ float4 rank_line_rows(const float* __restrict__ xs, const float* __restrict__ W1, int N1, int j0, int j1,
                                                 int c4, float4 acc) {
#pragma unroll 4
  for (int j = j0; j < j1; j += RL_NW) acc = fma4(xs[j], ld4(W1 + (int64_t)j * N1 + c4 * 4), acc);
  return acc;
}

// zline[l, n] = b1[n] + sum over the line's columns j (all but [off_ti, off_ti + Di)) of bn1(head[l, j]) W1[j, n].
// Wave w takes the rows j = w, w + 4, ... of either column range in ascending order, a lane four output columns (one 16-byte
// load per row); the four partial sums meet in LDS as (p0 + p1) + (p2 + p3)
__global__ __launch_bounds__(64 * RL_NW) void rank_line_kernel(const RankArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int Dh = a.Dh, N1 = a.N1, N1p = (N1 + 3) & ~3;
  float* xs = sm;                              // [Dh4]  bn1 of the line's row
  float* part = xs + ((Dh + 3) & ~3);          // [RL_NW][N1p]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l = blockIdx.x;
  for (int j = tid; j < Dh; j += 64 * RL_NW) xs[j] = a.head[(int64_t)l * Dh + j] * (a.gamma[j] * a.rs) + a.beta[j];
  __syncthreads();
  const int n4 = N1 >> 2;
  const int c4 = lane < n4 ? lane : n4 - 1;      // clamped, unconditional loads
  const int hi0 = a.off_ti + a.Di;
  // (the first row of either range that is this wave's: j = w mod 4)
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  acc = rank_line_rows(xs, a.W1, N1, wave, a.off_ti, c4, acc);
  acc = rank_line_rows(xs, a.W1, N1, hi0 + ((wave - hi0) & (RL_NW - 1)), Dh, c4, acc);
  if (lane < n4) *reinterpret_cast<float4*>(part + wave * N1p + lane * 4) = acc;
  __syncthreads();
  for (int n = tid; n < N1; n += 64 * RL_NW)
    a.zline[(int64_t)l * N1 + n] = a.b1[n] + ((part[n] + part[N1p + n]) + (part[2 * N1p + n] + part[3 * N1p + n]));
}

// one line's tile of HF_ROWS candidates: blockIdx.x = l * ntile + t
__global__ __launch_bounds__(64 * HF_NW) void rank_tile_kernel(const RankArgs a, const int ntile) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int Di = a.Di, N1 = a.N1, N2 = a.N2;
  const int Kp0 = (Di + 15) & ~15, LD0 = Kp0 + 4;
  const int Kp1 = (N1 + 15) & ~15, LD1 = Kp1 + 4;
  const int Kp2 = (N2 + 15) & ~15, LD2 = Kp2 + 4;
  float* xs = sm;                          // [16][LD0]  bn1 of the candidates' item columns
  float* f1s = xs + HF_ROWS * LD0;         // [16][LD1]
  float* f2s = f1s + HF_ROWS * LD1;        // [16][LD2]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lc = lane & 15, lq = lane >> 4;
  const int l = (int)blockIdx.x / ntile, c0 = ((int)blockIdx.x - l * ntile) * HF_ROWS;
  const int C = a.C;

  for (int e = tid; e < HF_ROWS * (LD0 + LD1 + LD2); e += 64 * HF_NW) sm[e] = 0.f;      // rows past C and the layers' K padding
  __syncthreads();
  // the tile's Fi table rows per candidate -> bn1's affine of the item columns -> LDS.  Candidates past C stay zero; their
  // addresses are the line's last candidate's (nothing is read past the line)
  {
    const int n4 = Di >> 2, D4 = a.D >> 2, Fi = Di / a.D;
    const int32_t* ids = a.cand + (int64_t)l * C * Fi;
    for (int e = tid; e < HF_ROWS * n4; e += 64 * HF_NW) {
      const int i = e / n4, j4 = e - i * n4;
      const int f = j4 / D4, cc = j4 - f * D4;
      const int c = c0 + i;
      const bool ok = c < C;
      uint32_t row = (uint32_t)ids[(int64_t)(ok ? c : C - 1) * Fi + f];
      if (row >= a.n_rows) {        // outside the table: the dummy row, reported (bit 5 = target_item)
        row = 0;
        if (a.id_status && ok && cc == 0) atomicOr(a.id_status, 1 << 5);
      }
      const float4 xv = ld4(a.table + ((int64_t)row * D4 + cc) * 4);
      const float4 gv = ld4(a.gamma + a.off_ti + j4 * 4);
      const float4 bv = ld4(a.beta + a.off_ti + j4 * 4);
      if (ok) {
        float4 v;
        v.x = xv.x * (gv.x * a.rs) + bv.x; v.y = xv.y * (gv.y * a.rs) + bv.y;
        v.z = xv.z * (gv.z * a.rs) + bv.z; v.w = xv.w * (gv.w * a.rs) + bv.w;
        *reinterpret_cast<float4*>(xs + i * LD0 + j4 * 4) = v;
      }
    }
  }
  __syncthreads();

  // fc1 over the item rows of W1, on top of the line's part: tiles of 16 columns, two per wave and pass
  const float* W1i = a.W1 + (int64_t)a.off_ti * N1;
  const float* zl = a.zline + (int64_t)l * N1;
  const int nt1 = (N1 + 15) >> 4;
  for (int tb = 0; tb < nt1; tb += 2 * HF_NW) {
    hf_f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const int t0 = tb + wave, t1 = tb + HF_NW + wave;
    const int n0[2] = {t0 < nt1 ? t0 * 16 : -1, t1 < nt1 ? t1 * 16 : -1};
    if (n0[0] >= 0) hf_tiles<2>(acc, xs, LD0, Kp0, Di, W1i, N1, n0, N1, lc, lq);
    float z1[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) z1[t] = zl[min(max(n0[t] + lc, 0), N1 - 1)];     // clamped, unconditional (no load behind a branch)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int col = n0[t] + lc;
      if (n0[t] < 0 || col >= N1) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) f1s[(lq * 4 + r) * LD1 + col] = fmaxf(acc[t][r] + z1[t], 0.f);
    }
  }
  __syncthreads();

  // fc2
  const int nt2 = (N2 + 15) >> 4;
  for (int tb = 0; tb < nt2; tb += HF_NW) {
    hf_f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
    const int t0 = tb + wave;
    const int n0[1] = {t0 < nt2 ? t0 * 16 : -1};
    if (n0[0] >= 0) hf_tiles<1>(acc, f1s, LD1, Kp1, N1, a.W2, N2, n0, N2, lc, lq);
    const int col = n0[0] + lc;
    const float bias2 = a.b2[min(max(col, 0), N2 - 1)];
    if (n0[0] >= 0 && col < N2) {
#pragma unroll
      for (int r = 0; r < 4; ++r) f2s[(lq * 4 + r) * LD2 + col] = fmaxf(acc[0][r] + bias2, 0.f);
    }
  }
  __syncthreads();

  // fc3 + sigmoid + the sample's log-loss term: four lanes per candidate, fixed-order partial sums (as the fused head)
  if (wave == 0) {
    const int i = lane >> 2, part = lane & 3;
    float s = 0.f;
    for (int n = part; n < N2; n += 4) s = fmaf(f2s[i * LD2 + n], a.W3[n], s);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    const int c = c0 + i;
    if (part == 0 && c < C) {
      const int64_t b = (int64_t)l * C + c;
      const float p = sigmoidf_(s + a.b3[0]);
      a.y[b] = p;
      a.lossb[b] = logloss_term(p, (float)a.label[b]);
    }
  }
}

inline size_t rank_tile_lds(int Di, int N1, int N2) {
  const int LD0 = ((Di + 15) & ~15) + 4, LD1 = ((N1 + 15) & ~15) + 4, LD2 = ((N2 + 15) & ~15) + 4;
  return (size_t)HF_ROWS * (LD0 + LD1 + LD2) * sizeof(float);
}
inline size_t rank_line_lds(int Dh, int N1) { return ((size_t)((Dh + 3) & ~3) + (size_t)RL_NW * ((N1 + 3) & ~3)) * sizeof(float); }

}  // namespace

bool score_rank_head_fits(int L, int C, int Dh, int off_ti, int Di, int D, int N1, int N2) {
  if (L <= 0 || C <= 0 || D <= 0 || (D & 3) || Di <= 0 || Di % D || off_ti < 0 || (off_ti & 3) || off_ti + Di > Dh) return false;
  if (N1 <= 0 || (N1 & 3) || N1 > 4 * 64 || N2 <= 0) return false;             // (a line wave's lanes cover N1 / 4 column groups)
  if ((int64_t)L * ((C + HF_ROWS - 1) / HF_ROWS) >= (1LL << 31) || (int64_t)L * C >= (1LL << 31)) return false;
  return rank_tile_lds(Di, N1, N2) <= 150 * 1024 && rank_line_lds(Dh, N1) <= 48 * 1024;
}

// The line kernel alone: zline [L, N1] for a caller that pairs the lines with something else than C candidates each (catalog.hip)
int score_rank_line(const RankArgs& a, hipStream_t s) {
  if (!score_rank_head_fits(a.L, 1, a.Dh, a.off_ti, a.Di, a.D, a.N1, a.N2)) return SCORE_E_SHAPE;
  hipLaunchKernelGGL(rank_line_kernel, dim3(a.L), dim3(64 * RL_NW), rank_line_lds(a.Dh, a.N1), s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}

// Returns SCORE_E_SHAPE for a shape the two kernels do not cover (score_rank_head_fits)
int score_rank_head(const RankArgs& a, hipStream_t s) {
  if (!score_rank_head_fits(a.L, a.C, a.Dh, a.off_ti, a.Di, a.D, a.N1, a.N2)) return SCORE_E_SHAPE;
  const size_t lds = rank_tile_lds(a.Di, a.N1, a.N2);
  static thread_local bool attr_set = false;
  if (!attr_set && lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(rank_tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       150 * 1024);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  hipLaunchKernelGGL(rank_line_kernel, dim3(a.L), dim3(64 * RL_NW), rank_line_lds(a.Dh, a.N1), s, a);
  SCORE_CHECK_LAUNCH();
  const int ntile = (a.C + HF_ROWS - 1) / HF_ROWS;
  hipLaunchKernelGGL(rank_tile_kernel, dim3((unsigned)(a.L * ntile)), dim3(64 * HF_NW), lds, s, a, ntile);
  SCORE_CHECK_LAUNCH();
  return 0;
}
