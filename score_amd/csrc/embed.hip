// Embedding-table kernels: row gather, fused gather + co-attention forward/backward,
// target-row gather/backward.  HBM-bound: every lane moves 16 B per load, all K
// neighbour rows of a unit are issued before the first use.
//
// Mapping ("slot" = one float4 of the F*D-wide concatenated feature vector of a
// neighbour, score.py:51-66 reshape): a GROUP of GS lanes (power of two, <= 64)
// owns one (b,t) unit; lane gl owns slots gl, gl+GS, ... (SPL of them) and walks
// the K neighbours in registers, so sums over K are sequential per lane (bitwise
// reproducible) and only the K relateness scores cross lanes.
#include <string.h>
#include "common.h"
#include "kernels.h"

// ------------------------------------------------------------------ plain gather (score.py:51-66)
__global__ void gather_rows_kernel(const float* __restrict__ table, int D4, const int32_t* __restrict__ idx,
                                   int64_t n_chunks, float* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n_chunks; i += stride) {
    int64_t r = i / D4;
    int c = (int)(i - r * D4);
    int64_t row = idx[r];
    st4(out + i * 4, ld4(table + (row * D4 + c) * 4));
  }
}

extern "C" int score_gather_fwd(const float* table, int64_t n_rows, int32_t D, const int32_t* idx,
                                int64_t n_idx, float* out, void* stream) {
  if (!table || !idx || !out || n_rows <= 0 || n_idx < 0) return SCORE_E_BADARG;
  if (D <= 0 || (D & 3)) return SCORE_E_SHAPE;
  if (n_idx == 0) return 0;
  int64_t n_chunks = n_idx * (D / 4);
  int blocks = (int)(cdiv64(n_chunks, 256) < 4096 ? cdiv64(n_chunks, 256) : 4096);
  hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, table, D / 4, idx,
                     n_chunks, out);
  SCORE_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ fused gather + co-attention
// One launch serves both co_attention calls of the model (score.py:196-197): blocks
// [0, first_block[1]) work on call 0, the rest on call 1, each with its own geometry.
static inline void coattn_geom(int D, int F, int* GS, int* SPL, int* nslots) {
  *nslots = F * (D / 4);
  int gs = 1;
  while (gs < *nslots && gs < 64) gs <<= 1;
  *GS = gs;
  *SPL = (*nslots + gs - 1) / gs;
}

template <int KMAX, int SPL>
__global__ __launch_bounds__(256) void coattn_fwd_kernel(const CoattnArgs a) {
  const int ci = (int)blockIdx.x >= a.c[1].first_block ? 1 : 0;
  const CoattnCall& cc = a.c[ci];
  const int GS = cc.GS, nslots = cc.nslots, F = cc.F, K = a.K, D4 = a.D4;
  const int lane = threadIdx.x & 63;
  const int wave = (((int)blockIdx.x - cc.first_block) * (int)blockDim.x + (int)threadIdx.x) >> 6;
  const int upw = 64 / GS;
  const int gl = lane & (GS - 1);
  const int unit = wave * upw + lane / GS;
  const bool unit_ok = unit < a.n_units;
  const int u = unit_ok ? unit : 0;  // clamp: inactive groups still take part in shuffles
  const int Dx = nslots * 4;
  const int D = D4 * 4;
  const float* __restrict__ table = a.table;
  const float* __restrict__ W = cc.W;
  const int mode = a.mode;

  bool ok[SPL];
  int f[SPL], coff[SPL];
  float4 w1[SPL], w2[SPL];
#pragma unroll
  for (int j = 0; j < SPL; ++j) {
    int s = gl + j * GS;
    ok[j] = unit_ok && s < nslots;
    int sc = s < nslots ? s : 0;
    f[j] = sc / D4;
    coff[j] = (sc - f[j] * D4) * 4;
    if (mode == 0) {
      w1[j] = ld4(W + Dx + sc * 4);
      w2[j] = ld4(W + 2 * Dx + sc * 4);
    } else {
      w1[j] = w2[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }

  // unit u = b * T + t over the ACTIVE time slices; the index tensors keep their [B, Tidx, K, F] strides
  const int b_idx = u / a.T;
  const int64_t ui = (int64_t)b_idx * a.Tidx + (u - b_idx * a.T);
  const int32_t* __restrict__ i1 = cc.idx1 + ui * K * F;
  const int32_t* __restrict__ i2 = cc.idx2 + ui * K * F;
  // Every load of the unit is unconditional and goes out before anything is consumed: first the 2K row ids,
  // then the 2K rows (16 B per lane each).  Inactive lanes / slots and k >= K read a valid clamped address and
  // are zeroed by a select afterwards: with the loads under `if (k < K)` / `if (ok)` branches the compiler
  // emitted one region per k that waited (vmcnt(0)) for its own two rows before the next k's ids were even
  // requested -- 2K dependent round trips per wave instead of two (0.134 -> 0.097 ms at cfg-3).
  float4 v1[SPL][KMAX];
  float4 sum2[SPL];
  float part[KMAX];
  int32_t ra[SPL][KMAX], rb[SPL][KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int kc = k < K ? k : K - 1;
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
      ra[j][k] = i1[kc * F + f[j]];
      rb[j][k] = i2[kc * F + f[j]];
    }
  }
  // ids outside the table: read as the dummy row, reported once per lane that saw one (clamped positions repeat real
  // ids of the tensor, so nothing is reported that the feed does not hold)
  const uint32_t NR = a.n_rows;
  bool bad1 = false, bad2 = false;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
      const bool b1 = (uint32_t)ra[j][k] >= NR, b2 = (uint32_t)rb[j][k] >= NR;
      bad1 |= b1; bad2 |= b2;
      ra[j][k] = b1 ? 0 : ra[j][k];
      rb[j][k] = b2 ? 0 : rb[j][k];
    }
  if (a.id_status && (bad1 || bad2)) atomicOr(a.id_status, (bad1 ? 1 << cc.bit1 : 0) | (bad2 ? 1 << cc.bit2 : 0));
  float4 yv[SPL][KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
      v1[j][k] = ld4(table + (int64_t)ra[j][k] * D + coff[j]);
      yv[j][k] = ld4(table + (int64_t)rb[j][k] * D + coff[j]);
    }
#pragma unroll
  for (int j = 0; j < SPL; ++j) sum2[j] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    part[k] = 0.f;
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
      const bool live = ok[j] && k < K;
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 x = live ? v1[j][k] : z;
      const float4 y = live ? yv[j][k] : z;
      v1[j][k] = x;
      sum2[j] = add4(sum2[j], y);
      part[k] += dot4(x, w1[j]) + dot4(y, w2[j]);
    }
  }

  if (mode == 1) {  // RCA: reduce_sum over K (score.py:266-269)
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
      if (!ok[j]) continue;
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) o = add4(o, v1[j][k]);
      st4(cc.out1 + (int64_t)u * cc.ld1 + (gl + j * GS) * 4, o);
      st4(cc.out2 + (int64_t)u * cc.ld2 + (gl + j * GS) * 4, sum2[j]);
    }
    return;
  }

  // c = w_t . target + bias (constant over t and i), then r_i = relu(part_i + c)
  float cpart = 0.f;
  if (cc.tidx) {
    // (round 6: straight from the table by the target's ids -- the copy that target_fwd_kernel gathers for the head and the query
    //  branch is the same bits, and reading it put that launch and a stream boundary in front of this kernel, the first of the
    //  step's chain; an id outside the table is the dummy row here as there, and reported there)
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
      uint32_t tr = (uint32_t)cc.tidx[(int64_t)b_idx * F + f[j]];
      tr = tr >= NR ? 0u : tr;
      const float4 tv = ld4(table + (int64_t)tr * D + coff[j]);
      if (ok[j]) cpart += dot4(tv, ld4(W + (gl + j * GS) * 4));
    }
  } else {
#pragma unroll
    for (int j = 0; j < SPL; ++j)
      if (ok[j]) cpart += dot4(ld4(cc.tgt + (int64_t)b_idx * cc.ldt + (gl + j * GS) * 4), ld4(W + (gl + j * GS) * 4));
  }
  float red[KMAX + 1];          // the K partial scores and the target term: reduced across the group together
#pragma unroll
  for (int k = 0; k < KMAX; ++k) red[k] = (k < K) ? part[k] : 0.f;
  red[KMAX] = cpart;
  group_sum_n<KMAX + 1>(red, GS);
  const float c = red[KMAX] + cc.bias[0];
  float r[KMAX];
  float rmax = 0.f, rsum = 0.f;  // relu output >= 0
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    r[k] = 0.f;
    if (k < K) {
      r[k] = fmaxf(red[k] + c, 0.f);
      rmax = fmaxf(rmax, r[k]);
      rsum += r[k];
    }
  }
  float p[KMAX];
  float den = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    p[k] = (k < K) ? expf(r[k] - rmax) : 0.f;
    den += p[k];
  }
  const float inv_den = 1.0f / den;
#pragma unroll
  for (int j = 0; j < SPL; ++j) {
    if (!ok[j]) continue;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) o = fma4(p[k] * inv_den, v1[j][k], o);
    st4(cc.out1 + (int64_t)u * cc.ld1 + (gl + j * GS) * 4, o);
    const float fk = (float)K;
    st4(cc.out2 + (int64_t)u * cc.ld2 + (gl + j * GS) * 4,
        make_float4(sum2[j].x / fk, sum2[j].y / fk, sum2[j].z / fk, sum2[j].w / fk));
  }
  // atten_info = [K*r_0..K*r_{K-1}, sum_i r_i (K times)]  (score.py:165-166)
  if (unit_ok) {
    for (int i = gl; i < 2 * K; i += GS) {
      float val = rsum;
      float rv = 0.f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (i == k) rv = r[k];
      if (i < K) {
        val = (float)K * rv;
        cc.rsave[(int64_t)u * K + i] = rv;
      }
      cc.info[(int64_t)u * cc.ldi + i] = val;
    }
  }
}

// ------------------------------------------------------------------ backward
// Per unit (collapsed form):
//   dr_i  = K*ga_i + sum_j ga_{K+j} + p_i (dp_i - sum_k p_k dp_k),  dp_i = g1 . seq1_i
//   dz_i  = dr_i * [r_i > 0]
//   dseq1_i = p_i g1 + dz_i w1,   dseq2_i = g2/K + dz_i w2
//   dw1 += sum_i dz_i seq1_i,  dw2 += sum_i dz_i seq2_i,  dzsum = sum_i dz_i
__device__ __forceinline__ void atomic_add4(float* d, float4 v) {
  atomicAdd(d, v.x); atomicAdd(d + 1, v.y); atomicAdd(d + 2, v.z); atomicAdd(d + 3, v.w);
}

// Nothing that uses `row` is placed in front of the load of `last`, the last row of its batch (an empty statement the
// compiler cannot move a use across: a scheduling barrier alone left the uses where instruction selection had put
// them, in front of it).  Loads return in order, so one wait for `last` is the wait for the whole batch.
__device__ __forceinline__ void rows_in_flight(float4& row, const float4& last) {
  asm volatile("" : "+v"(row.x), "+v"(row.y), "+v"(row.z), "+v"(row.w) : "v"(last.w));
}

// Per-unit metadata of the backward, ONE ELEMENT PER LANE (the instances with NM > 0).  A unit's K*F ids of each index
// tensor and its 3K saved scalars (K relu'd scores from rsave, then the 2K score gradients of ginfo) are lists whose
// addresses depend on nothing but the unit's number, and every lane of a feature needs the same few of them.  Instead of
// 2K id registers and 3K scalar registers in every lane, the GS lanes of the unit's group load each list contiguously:
//  * ids: register i of lane gl holds element i * kpr * F + gl, i.e. the ids of the kpr = 2^ksh neighbours
//    [i * kpr, (i + 1) * kpr) (kpr * F <= GS; lanes past kpr * F and elements past K * F repeat the last element).  The
//    register a neighbour k lives in, k >> ksh, is the same in every lane: a select between registers and ONE
//    ds_bpermute inside the group give lane gl the id of (k, its feature) when it uses it;
//  * scalars: register i of lane gl holds element i * GS + gl; element e is broadcast from lane e % GS.
// Ids outside the table become row 0 once, on the lane that loaded them.  NM registers per list: coattn_meta_regs()
// says what a geometry needs, and score_coattn_bwd_multi takes the NM = 0 instance (every lane reads its own ids and
// scalars, nothing a unit ahead) where that is more than the instance holds.

static inline int coattn_ksh(int GS, int F) {      // log2 of the neighbours per id register; -1: a feature set does not fit a group
  if (F > GS) return -1;
  int sh = 0;
  while ((2 << sh) * F <= GS) ++sh;
  return sh;
}
static inline int coattn_meta_regs(int GS, int F, int K) {      // registers per list (0: not in this form)
  const int ksh = coattn_ksh(GS, F);
  if (ksh < 0) return 0;
  const int ids = (K + (1 << ksh) - 1) >> ksh, sc = (3 * K + GS - 1) / GS;
  return ids > sc ? ids : sc;
}

// One list: up to four registers, NAMED (r0 .. r3; an instance touches the first NM).  As an array read through selects
// on the register number the compiler kept the list in scratch memory and indexed it there.
template <typename T> struct MetaList { T r0, r1, r2, r3; };
struct UnitMeta { MetaList<int32_t> a, b; MetaList<float> s; };      // ids of idx1, ids of idx2, saved scalars
template <int I, typename T> __device__ __forceinline__ T& meta_at(MetaList<T>& l) {
  if constexpr (I == 0) return l.r0;
  else if constexpr (I == 1) return l.r1;
  else if constexpr (I == 2) return l.r2;
  else return l.r3;
}
// register `reg` (the same in every lane, < NM) of a list
template <int NM, typename T>
__device__ __forceinline__ T meta_reg(const MetaList<T>& l, int reg) {
  static_assert(NM >= 1 && NM <= 4, "a list is at most four registers");
  T v = l.r0;
  if constexpr (NM > 1) { const T x = l.r1; v = reg == 1 ? x : v; }
  if constexpr (NM > 2) { const T x = l.r2; v = reg == 2 ? x : v; }
  if constexpr (NM > 3) { const T x = l.r3; v = reg == 3 ? x : v; }
  return v;
}

// every load unconditional, to a clamped, valid position
template <int I>
__device__ __forceinline__ void unit_meta_load1(UnitMeta& m, const int32_t* __restrict__ i1, const int32_t* __restrict__ i2,
                                                const float* __restrict__ rs, const float* __restrict__ gi, int K, int KF,
                                                int GS, int per, int gc, int gl) {
  const int e = I * per + gc, es = I * GS + gl;
  const int ei = e < KF ? e : KF - 1;
  const int esc = es < 3 * K ? es : 3 * K - 1;
  meta_at<I>(m.a) = i1[ei];
  meta_at<I>(m.b) = i2[ei];
  meta_at<I>(m.s) = *(esc < K ? rs + esc : gi + (esc - K));
}
template <int I>
__device__ __forceinline__ void unit_meta_clamp1(UnitMeta& m, uint32_t n_rows) {      // (the forward reported them: score_state_t.id_status)
  const int32_t x = meta_at<I>(m.a), y = meta_at<I>(m.b);
  meta_at<I>(m.a) = (uint32_t)x < n_rows ? x : 0;
  meta_at<I>(m.b) = (uint32_t)y < n_rows ? y : 0;
}
template <int NM>
__device__ __forceinline__ void unit_meta_load(UnitMeta& m, const CoattnArgs& a, const CoattnCall& cc, int u, int gl) {
  const int K = a.K, KF = a.K * cc.F, GS = cc.GS, per = cc.F << cc.ksh;
  const int ub = u / a.T;
  const int64_t ui = (int64_t)ub * a.Tidx + (u - ub * a.T);   // [B, Tidx, K, F] strides of the index tensors
  const int32_t* __restrict__ i1 = cc.idx1 + ui * KF;
  const int32_t* __restrict__ i2 = cc.idx2 + ui * KF;
  const float* __restrict__ rs = cc.rsave + (int64_t)u * K;
  const float* __restrict__ gi = cc.ginfo + (int64_t)u * cc.ldi;
  const int gc = gl < per ? gl : per - 1;
  unit_meta_load1<0>(m, i1, i2, rs, gi, K, KF, GS, per, gc, gl);
  if constexpr (NM > 1) unit_meta_load1<1>(m, i1, i2, rs, gi, K, KF, GS, per, gc, gl);
  if constexpr (NM > 2) unit_meta_load1<2>(m, i1, i2, rs, gi, K, KF, GS, per, gc, gl);
  if constexpr (NM > 3) unit_meta_load1<3>(m, i1, i2, rs, gi, K, KF, GS, per, gc, gl);
  unit_meta_clamp1<0>(m, a.n_rows);
  if constexpr (NM > 1) unit_meta_clamp1<1>(m, a.n_rows);
  if constexpr (NM > 2) unit_meta_clamp1<2>(m, a.n_rows);
  if constexpr (NM > 3) unit_meta_clamp1<3>(m, a.n_rows);
}

// The source lanes and register numbers of a unit's elements are the same for every unit.  Hoisted out of the unit loop
// they are 10 to 30 registers that live through all of it -- the compiler spilled them and read them back one at a
// time -- so each use site works from copies of its inputs that the compiler cannot look through (an empty volatile
// statement: nothing is emitted), and the two or three integer operations per element stay where the element is used.
#define META_RECOMPUTE(vgpr, sgpr0, sgpr1) asm volatile("" : "+v"(vgpr), "+s"(sgpr0), "+s"(sgpr1))

// the ids of (k, feature fj) of one index tensor for k < KMAX (k >= K repeats K - 1)
template <int KMAX, int NM>
__device__ __forceinline__ void unit_ids(int32_t (&out)[KMAX], const MetaList<int32_t>& l, int K, int F, int ksh, int fj, int gbase) {
  META_RECOMPUTE(gbase, K, F);
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int kc = k < K ? k : K - 1;
    const int reg = kc >> ksh;
    out[k] = __builtin_amdgcn_ds_bpermute((gbase + (kc - (reg << ksh)) * F + fj) << 2, meta_reg<NM>(l, reg));
  }
}

// element e (the same in every lane) of the unit's list of saved scalars
template <int NM>
__device__ __forceinline__ float unit_scalar(const MetaList<float>& l, int e, int gbase, int GS, int gsh) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute((gbase + (e & (GS - 1))) << 2, __float_as_int(meta_reg<NM>(l, e >> gsh))));
}

template <int KMAX, int SPL, bool ATOMIC, int NM>
__global__ __launch_bounds__(256, (KMAX <= 10 && SPL == 1) ? 4 : 1) void coattn_bwd_kernel_t(const CoattnArgs a) {
  extern __shared__ float lds[];  // [4 waves][upw][2*Dx]
  const int ci = (int)blockIdx.x >= a.c[1].first_block ? 1 : 0;
  const CoattnCall& cc = a.c[ci];
  const int GS = cc.GS, nslots = cc.nslots, F = cc.F, K = a.K, D4 = a.D4, n_units = a.n_units;
  const int mode = a.mode;
  const bool all_rows = a.all_rows != 0, ahead = a.meta_ahead != 0;
  const int lane = threadIdx.x & 63;
  const int wib = threadIdx.x >> 6;
  const int upw = 64 / GS;
  const int gl = lane & (GS - 1);
  const int grp = lane / GS;
  const int gbase = lane - gl;      // first lane of this lane's group
  const int gsh = __builtin_ctz(GS), ksh = cc.ksh;
  const int Dx = nslots * 4;
  const int D = D4 * 4;
  const int my_blocks = (ci == 0 ? min(a.c[1].first_block, (int)gridDim.x) : (int)gridDim.x) - cc.first_block;
  const int waves_total = my_blocks * 4;
  const int blk = (int)blockIdx.x - cc.first_block;
  const int wave0 = blk * 4 + wib;
  const float* __restrict__ table = a.table;
  float* __restrict__ gtable = a.gtable;
  const float* __restrict__ W = cc.W;

  bool sok[SPL];
  int f[SPL], coff[SPL];
  float4 w1[SPL], w2[SPL], dw1[SPL], dw2[SPL];
#pragma unroll
  for (int j = 0; j < SPL; ++j) {
    int s = gl + j * GS;
    sok[j] = s < nslots;
    int sc = sok[j] ? s : 0;
    f[j] = sc / D4;
    coff[j] = (sc - f[j] * D4) * 4;
    w1[j] = w2[j] = dw1[j] = dw2[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mode == 0) {
      w1[j] = ld4(W + Dx + sc * 4);
      w2[j] = ld4(W + 2 * Dx + sc * 4);
    }
  }

  const int n_iter = (n_units + waves_total * upw - 1) / (waves_total * upw);
  UnitMeta cur;      // the current unit's id lists and saved scalars, one element per lane
  if constexpr (NM > 0) {
    if (ahead) {      // the first unit's metadata (a group past the last unit reads unit 0's, like everything else)
      const int unit = wave0 * upw + grp;
      unit_meta_load<NM>(cur, a, cc, unit < n_units ? unit : 0, gl);
    }
  }
  for (int it = 0; it < n_iter; ++it) {
    const int unit = (it * waves_total + wave0) * upw + grp;
    const bool unit_ok = unit < n_units;
    const int u = unit_ok ? unit : 0;
    const int ub = u / a.T;
    const int64_t ui = (int64_t)ub * a.Tidx + (u - ub * a.T);   // [B, Tidx, K, F] strides of the index tensors
    const int32_t* __restrict__ i1 = cc.idx1 + ui * K * F;
    const int32_t* __restrict__ i2 = cc.idx2 + ui * K * F;
    float4 g1[SPL], g2[SPL];
    bool ok[SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j) ok[j] = unit_ok && sok[j];
    if (NM == 0 || mode == 1) {
#pragma unroll
      for (int j = 0; j < SPL; ++j) {
        g1[j] = g2[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok[j]) {
          g1[j] = ld4(cc.g1 + (int64_t)u * cc.ld1 + (gl + j * GS) * 4);
          g2[j] = ld4(cc.g2 + (int64_t)u * cc.ld2 + (gl + j * GS) * 4);
        }
      }
    }
    if (mode == 1) {  // RCA: d(sum_k row_k) = g for every k
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
          if (!ok[j] || k >= K) continue;
          if (!ATOMIC) continue;  // pull mode: every row gradient is g itself, nothing to prepare
          int64_t r1 = i1[k * F + f[j]], r2 = i2[k * F + f[j]];
          r1 = (uint64_t)r1 < a.n_rows ? r1 : 0;
          r2 = (uint64_t)r2 < a.n_rows ? r2 : 0;
          if (r1 != 0) atomic_add4(gtable + r1 * D + coff[j], g1[j]);
          if (r2 != 0) atomic_add4(gtable + r2 * D + coff[j], g2[j]);
        }
      }
      continue;
    }

    // pass 1: seq1 rows -> dp_k = g1 . seq1_k.
    // Every load is unconditional (clamped addresses, zeroed by selects afterwards): under `if (k < K && ok)` every k
    // was a region of its own that waited for its id and then for its row.  The scheduling barriers and rows_in_flight
    // behind the rows keep the requests together in the code the compiler emits: held to 128 VGPRs, it put every load
    // next to its use (profiles/coattn_bwd_active_rows.md), and it would sink the next unit's requests to the bottom of
    // the loop, where nothing hides them.
    // NM > 0: the unit's ids and saved scalars (`cur`, one element per lane: UnitMeta) are requested at the top of its
    // iteration, a round trip of their own; g1 / g2 go out in front of pass 1's rows and ride on their wait; then one
    // round trip per pass: four per unit, where the NM = 0 form makes seven in the emitted code (two for the ids, the
    // saved scalars' own, g1 / g2 in front of everything) and spills (profiles/coattn_bwd_prefetch.md).
    // CoattnArgs.meta_ahead (debug_flags bit 16): the metadata is requested ONE UNIT AHEAD instead, right behind the
    // pass-1 rows of the unit before -- a wave knows its next unit's number an iteration early, and its loads return
    // in issue order, so they arrive with the wait for that unit's pass 2: three round trips per unit.  The first
    // unit's come from a prologue in front of the loop; the request behind a wave's last unit goes to a clamped, valid
    // unit (unit 0) and is dropped.  Not the default: 12 us of the kernel's 93 at cfg-3 are the one-element-per-lane
    // form's, the unit ahead added 0.7 us more and 0.3 % of step rate, inside the run-to-run spread.
    // NM = 0: all 2K row ids of every lane, then the K seq1 rows; the saved scalars between pass 1 and pass 2.
    // Same arithmetic in the same order in both.
    int32_t r1[SPL][KMAX], rb2[SPL][KMAX];
    float dp[KMAX];
    UnitMeta nxt;
    if constexpr (NM > 0) {
      if (!ahead) unit_meta_load<NM>(cur, a, cc, u, gl);
#pragma unroll
      for (int j = 0; j < SPL; ++j) {
        const int sc = sok[j] ? gl + j * GS : 0;
        g1[j] = ld4(cc.g1 + (int64_t)u * cc.ld1 + sc * 4);
        g2[j] = ld4(cc.g2 + (int64_t)u * cc.ld2 + sc * 4);
      }
    } else {
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        const int kc = k < K ? k : K - 1;
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
          r1[j][k] = i1[kc * F + f[j]];
          rb2[j][k] = i2[kc * F + f[j]];
        }
      }
      __builtin_amdgcn_sched_barrier(0);      // every id is requested before the first one is used
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
          r1[j][k] = (uint32_t)r1[j][k] < a.n_rows ? r1[j][k] : 0;      // (the forward reported it: score_state_t.id_status)
          rb2[j][k] = (uint32_t)rb2[j][k] < a.n_rows ? rb2[j][k] : 0;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k) dp[k] = 0.f;
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
      if constexpr (NM > 0) unit_ids<KMAX, NM>(r1[j], cur.a, K, F, ksh, f[j], gbase);
      float4 v1[KMAX];
#pragma unroll
      for (int k = 0; k < KMAX; ++k) v1[k] = ld4(table + (int64_t)r1[j][k] * D + coff[j]);
      if constexpr (NM > 0) {
        if (j == 0) {
          if (ahead) {
            const int64_t unit_n = ((int64_t)(it + 1) * waves_total + wave0) * upw + grp;
            unit_meta_load<NM>(nxt, a, cc, unit_n < n_units ? (int)unit_n : 0, gl);
          }
          __builtin_amdgcn_sched_barrier(0);      // all of it is requested before the first row is used
        }
      }
#pragma unroll
      for (int k = 0; k < KMAX; ++k) rows_in_flight(v1[k], v1[KMAX - 1]);
      if constexpr (NM > 0) {
        g1[j].x = ok[j] ? g1[j].x : 0.f; g1[j].y = ok[j] ? g1[j].y : 0.f;
        g1[j].z = ok[j] ? g1[j].z : 0.f; g1[j].w = ok[j] ? g1[j].w : 0.f;
        g2[j].x = ok[j] ? g2[j].x : 0.f; g2[j].y = ok[j] ? g2[j].y : 0.f;
        g2[j].z = ok[j] ? g2[j].z : 0.f; g2[j].w = ok[j] ? g2[j].w : 0.f;
        // (g2 is not used before pass 3: without this its load was moved down there, a round trip of its own)
        asm volatile("" : "+v"(g2[j].x), "+v"(g2[j].y), "+v"(g2[j].z), "+v"(g2[j].w));
      }
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        const bool live = ok[j] && k < K;
        v1[k].x = live ? v1[k].x : 0.f; v1[k].y = live ? v1[k].y : 0.f;
        v1[k].z = live ? v1[k].z : 0.f; v1[k].w = live ? v1[k].w : 0.f;
        if constexpr (NM == 0) {
          r1[j][k] = live ? r1[j][k] : 0;
          rb2[j][k] = live ? rb2[j][k] : 0;
        }
        dp[k] += dot4(v1[k], g1[j]);
      }
    }
    // softmax from the saved relu'd scores
    float r[KMAX], p[KMAX], gik[KMAX];
    float rmax = 0.f, gsum = 0.f;
    int gb_s = gbase, K_s = K, GS_s = GS;
    if constexpr (NM > 0) META_RECOMPUTE(gb_s, K_s, GS_s);
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {      // (k >= K repeats K - 1; NM = 0: clamped, unconditional loads, see above)
      const int kc = k < K ? k : K - 1;
      float rv, g2v;
      if constexpr (NM > 0) {
        const int kcs = k < K_s ? k : K_s - 1;
        rv = unit_scalar<NM>(cur.s, kcs, gb_s, GS_s, gsh);
        gik[k] = unit_scalar<NM>(cur.s, K_s + kcs, gb_s, GS_s, gsh);
        g2v = unit_scalar<NM>(cur.s, 2 * K_s + kcs, gb_s, GS_s, gsh);
      } else {
        rv = cc.rsave[(int64_t)u * K + kc];
        g2v = cc.ginfo[(int64_t)u * cc.ldi + K + kc];
        gik[k] = cc.ginfo[(int64_t)u * cc.ldi + kc];
      }
      r[k] = (k < K) ? rv : 0.f;
      rmax = fmaxf(rmax, r[k]);
      gsum += (k < K) ? g2v : 0.f;
    }
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      p[k] = (k < K) ? expf(r[k] - rmax) : 0.f;
      den += p[k];
    }
    const float inv_den = 1.0f / den;
    float pdp = 0.f;
    group_sum_n<KMAX>(dp, GS);       // dp_k = g1 . seq1_k: the K dot products reduced across the group together
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      p[k] *= inv_den;
      dp[k] = (k < K) ? dp[k] : 0.f;
      pdp += p[k] * dp[k];
    }
    float dz[KMAX];
    float dzs = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      dz[k] = 0.f;
      if (k < K) {
        float dr = (float)K * gik[k] + gsum + p[k] * (dp[k] - pdp);
        dz[k] = r[k] > 0.f ? dr : 0.f;
        dzs += dz[k];
      }
    }
    if (unit_ok && gl == 0) cc.dzsum[u] = dzs;
    if (!ATOMIC && unit_ok) {  // the scalars the pull-form scatter multiplies G and w with
      for (int i = gl; i < K; i += GS) {
        float pv = 0.f, dv = 0.f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if (i == k) { pv = p[k]; dv = dz[k]; }
        cc.pcoef[(int64_t)u * K + i] = pv;
        cc.dzcoef[(int64_t)u * K + i] = dv;
      }
    }
    const float invK = 1.0f / (float)K;
    // Passes 2 and 3: dw1 += dz_k seq1_k over the seq1 rows, then dw2 += dz_k seq2_k over the seq2 rows, K rows in
    // flight together each.  Every term carries dz_k = [r_k > 0] dr_k, so only the rows of the k whose relu was
    // ACTIVE (r_k > 0 in rsave) are requested: an inactive k adds fma(0, row, acc) = acc whatever its row holds, and
    // its load goes to row 0, the all-zero row, like every masked use (a select on the row id per lane, no branch:
    // see the forward kernel's loads) -- one hot line instead of a gathered row.  A third of all (unit, k) are
    // inactive on the cfg-3 batches: the kernel fetches 12 % less, in the same time (it is bound by its dependent
    // round trips, not by bytes: profiles/coattn_bwd_active_rows.md).
    // Pass 1 keeps all K rows: dp_k enters sum_k p_k dp_k for every k.  The atomic scatter's target row
    // and its != 0 test keep the real id (an inactive k still adds p_k g1 / g2/K to its row): only the load moves.
    // The only value that can differ: a table that already holds Inf/NaN in a row of an inactive k no longer poisons dw1/dw2.
    // (CoattnArgs.all_rows, debug_flags bit 15: every row as before, the A/B.)
    // The seq1 rows are READ AGAIN (cache hits: this wave fetched them a moment ago) instead of being held in
    // 40 VGPRs across the reductions and the softmax: 24 -> 10 spilled registers at 4 waves/SIMD, 0.262 -> 0.241 ms
    bool act[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) act[k] = all_rows || (k < K && r[k] > 0.f);
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
      float4 xr[KMAX];
      if constexpr (NM > 0) {      // (from the unit's list again: a shuffle, not K registers held since pass 1)
        unit_ids<KMAX, NM>(r1[j], cur.a, K, F, ksh, f[j], gbase);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) r1[j][k] = (ok[j] && k < K) ? r1[j][k] : 0;
      }
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        const int32_t lr = act[k] ? r1[j][k] : 0;      // the row LOADED; r1 stays the row the gradient goes to
        xr[k] = ld4(table + (int64_t)lr * D + coff[j]);
      }
      if constexpr (NM > 0) {      // (one round trip: the first row was requested, waited for and used in front of the other K - 1)
#pragma unroll
        for (int k = 0; k < KMAX; ++k) rows_in_flight(xr[k], xr[KMAX - 1]);
      }
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        dw1[j] = fma4(dz[k], xr[k], dw1[j]);
        if (ATOMIC && r1[j][k] != 0) {
          float4 d1 = fma4(dz[k], w1[j],
                           make_float4(p[k] * g1[j].x, p[k] * g1[j].y, p[k] * g1[j].z, p[k] * g1[j].w));
          atomic_add4(gtable + (int64_t)r1[j][k] * D + coff[j], d1);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
      const float4 g2k = make_float4(g2[j].x * invK, g2[j].y * invK, g2[j].z * invK, g2[j].w * invK);
      float4 y[KMAX];
      if constexpr (NM > 0) {
        unit_ids<KMAX, NM>(rb2[j], cur.b, K, F, ksh, f[j], gbase);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) rb2[j][k] = (ok[j] && k < K) ? rb2[j][k] : 0;
      }
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        const int32_t lr = act[k] ? rb2[j][k] : 0;
        y[k] = ld4(table + (int64_t)lr * D + coff[j]);
      }
      if constexpr (NM > 0) {
#pragma unroll
        for (int k = 0; k < KMAX; ++k) rows_in_flight(y[k], y[KMAX - 1]);
      }
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        dw2[j] = fma4(dz[k], y[k], dw2[j]);
        if (ATOMIC && rb2[j][k] != 0) atomic_add4(gtable + (int64_t)rb2[j][k] * D + coff[j], fma4(dz[k], w2[j], g2k));
      }
    }
    if constexpr (NM > 0) {
      if (ahead) cur = nxt;
    }
  }
  if (mode == 1) return;
  // block-level reduction of (dw1, dw2) -> slab[block][2*Dx], fixed order
  float* mine = lds + ((wib * upw + grp) * 2) * Dx;
#pragma unroll
  for (int j = 0; j < SPL; ++j) {
    if (!sok[j]) continue;
    st4(mine + (gl + j * GS) * 4, dw1[j]);
    st4(mine + Dx + (gl + j * GS) * 4, dw2[j]);
  }
  __syncthreads();
  const int nsrc = 4 * upw;
  for (int e = threadIdx.x; e < 2 * Dx; e += blockDim.x) {
    float s = 0.f;
    for (int q = 0; q < nsrc; ++q) s += lds[q * 2 * Dx + e];
    cc.slab[(int64_t)blk * 2 * Dx + e] = s;
  }
}

// ------------------------------------------------------------------ forward, several units per wave
// The forward in the form of the backward's NM > 0 instances (mode 0, one slot per lane, K <= 10): a group works through
// a CHUNK of up to CoattnArgs.CH consecutive time slices of ONE sample instead of one unit.
//  * What does not depend on the slice is loaded once per chunk, together with the first unit's ids: w1 / w2, the lane's
//    partial of the target term (cpart: target ids -> table row, or cc.tgt) and its slice of w_t.
//  * A unit's K*F ids of each index tensor are held one element per lane (MetaList, as in the backward) and handed out
//    by ds_bpermute where the row address is formed: 2 NM registers, not 2 KMAX.  Ids outside the table become row 0 on
//    the lane that loaded them, where they are also noted for id_status (one atomicOr per chunk).
//  * The ids of the chunk's next unit are requested right behind the 2K rows of the current one and arrive with them;
//    behind the chunk's last unit the request goes to unit 0 and is dropped.
// So a unit costs one dependent round trip (its rows), a chunk two more in front (ids + constants, then the target row).
// A unit's stores are issued in front of the next unit's row requests: loads and stores leave vmcnt in issue order, so the
// wait for those rows (vmcnt = the id requests behind them) asks nothing of the stores that the rows' own latency has
// not long covered.  Arithmetic, its order and the stores are those of coattn_fwd_kernel: bit-identical outputs.
template <int I>
__device__ __forceinline__ void unit_ids_load1(MetaList<int32_t>& la, MetaList<int32_t>& lb, const int32_t* __restrict__ i1,
                                               const int32_t* __restrict__ i2, int KF, int per, int gc) {
  const int e = I * per + gc;
  const int ei = e < KF ? e : KF - 1;
  meta_at<I>(la) = i1[ei];
  meta_at<I>(lb) = i2[ei];
}
// the id lists alone of the unit whose index-tensor position is ui (every load unconditional, to a clamped, valid position)
template <int NM>
__device__ __forceinline__ void unit_ids_load(MetaList<int32_t>& la, MetaList<int32_t>& lb, const CoattnArgs& a, const CoattnCall& cc,
                                              int64_t ui, int gl) {
  const int KF = a.K * cc.F, per = cc.F << cc.ksh;
  const int32_t* __restrict__ i1 = cc.idx1 + ui * KF;
  const int32_t* __restrict__ i2 = cc.idx2 + ui * KF;
  const int gc = gl < per ? gl : per - 1;
  unit_ids_load1<0>(la, lb, i1, i2, KF, per, gc);
  if constexpr (NM > 1) unit_ids_load1<1>(la, lb, i1, i2, KF, per, gc);
  if constexpr (NM > 2) unit_ids_load1<2>(la, lb, i1, i2, KF, per, gc);
  if constexpr (NM > 3) unit_ids_load1<3>(la, lb, i1, i2, KF, per, gc);
}
template <int I>
__device__ __forceinline__ void unit_ids_clamp1(MetaList<int32_t>& la, MetaList<int32_t>& lb, uint32_t n_rows, bool& bad1, bool& bad2) {
  const int32_t x = meta_at<I>(la), y = meta_at<I>(lb);
  const bool b1 = (uint32_t)x >= n_rows, b2 = (uint32_t)y >= n_rows;
  bad1 |= b1; bad2 |= b2;
  meta_at<I>(la) = b1 ? 0 : x;
  meta_at<I>(lb) = b2 ? 0 : y;
}
template <int NM>
__device__ __forceinline__ void unit_ids_clamp(MetaList<int32_t>& la, MetaList<int32_t>& lb, uint32_t n_rows, bool& bad1, bool& bad2) {
  unit_ids_clamp1<0>(la, lb, n_rows, bad1, bad2);
  if constexpr (NM > 1) unit_ids_clamp1<1>(la, lb, n_rows, bad1, bad2);
  if constexpr (NM > 2) unit_ids_clamp1<2>(la, lb, n_rows, bad1, bad2);
  if constexpr (NM > 3) unit_ids_clamp1<3>(la, lb, n_rows, bad1, bad2);
}

template <int KMAX, int NM>
__global__ __launch_bounds__(256, 4) void coattn_fwd_kernel_units(const CoattnArgs a) {
  const int ci = (int)blockIdx.x >= a.c[1].first_block ? 1 : 0;
  const CoattnCall& cc = a.c[ci];
  const int GS = cc.GS, nslots = cc.nslots, F = cc.F, K = a.K, D4 = a.D4, ksh = cc.ksh;
  const int lane = threadIdx.x & 63;
  const int wave = (((int)blockIdx.x - cc.first_block) * (int)blockDim.x + (int)threadIdx.x) >> 6;
  const int upw = 64 / GS;
  const int gl = lane & (GS - 1);
  const int gbase = lane - gl;      // first lane of this lane's group
  const int chunk = wave * upw + lane / GS;
  const bool chunk_ok = chunk < a.n_chunks;
  const int c = chunk_ok ? chunk : 0;  // clamp: inactive groups still take part in shuffles
  const int b_idx = c / a.cps;
  const int t0 = (c - b_idx * a.cps) * a.CH;
  const int nt = chunk_ok ? min(a.CH, a.T - t0) : 0;      // the last chunk of a sample is short
  // unit i of the chunk is (b_idx, t0 + i) over the ACTIVE time slices; the index tensors keep their [B, Tidx, K, F] strides
  const int Dx = nslots * 4;
  const int D = D4 * 4;
  const float* __restrict__ table = a.table;
  const float* __restrict__ W = cc.W;
  const uint32_t NR = a.n_rows;

  const bool sok = gl < nslots;
  const int sc = sok ? gl : 0;
  const int f = sc / D4;
  const int coff = (sc - f * D4) * 4;

  // once per chunk, all of it requested before anything is used: w1 / w2 / w_t, the target, the first unit's ids
  MetaList<int32_t> ca, cb, na, nb;      // the current and the next unit's id lists
  const float4 w1 = ld4(W + Dx + sc * 4);
  const float4 w2 = ld4(W + 2 * Dx + sc * 4);
  const float4 wt = ld4(W + sc * 4);
  float4 tv;
  uint32_t tr = 0;
  if (cc.tidx) tr = (uint32_t)cc.tidx[(int64_t)b_idx * F + f];
  else tv = ld4(cc.tgt + (int64_t)b_idx * cc.ldt + sc * 4);
  unit_ids_load<NM>(ca, cb, a, cc, (int64_t)b_idx * a.Tidx + t0, gl);
  const float bias = cc.bias[0];
  __builtin_amdgcn_sched_barrier(0);
  if (cc.tidx) {      // (an id outside the table is the dummy row here; target_fwd_kernel reports it)
    tr = tr >= NR ? 0u : tr;
    tv = ld4(table + (int64_t)tr * D + coff);
  }
  // c = w_t . target + bias (constant over t and i): the lane's partial, reduced with every unit's scores
  float cpart = 0.f;
  if (chunk_ok && sok) cpart += dot4(tv, wt);

  bool bad1 = false, bad2 = false;
  unit_ids_clamp<NM>(ca, cb, NR, bad1, bad2);
  for (int i = 0; i < a.CH; ++i) {
    const bool unit_ok = i < nt;
    if (!__any(unit_ok)) break;      // (the groups of a wave own chunks of their own: the longest decides)
    const bool ok = unit_ok && sok;
    // Every address of the unit is formed here, from copies of the sample and slice numbers that the compiler cannot look
    // through: hoisted out of the loop, the per-lane 64-bit pointers of the four outputs and the two id lists are 12
    // registers and more that live through all of it, and were spilled (44 registers, the rows' addresses with them).
    int bq = b_idx, tq = t0 + i, gq = gl, fq = f, cq = coff;
    asm volatile("" : "+v"(bq), "+v"(tq), "+v"(gq), "+v"(fq), "+v"(cq));
    const int u = bq * a.T + tq;
    const int64_t uin = i + 1 < nt ? (int64_t)bq * a.Tidx + tq + 1 : 0;
    // the 2K rows (16 B per lane each), then the next unit's ids; nothing is consumed before all of it is requested.
    // Inactive lanes / units and k >= K read a valid clamped address and are zeroed by a select afterwards.
    int32_t ra[KMAX], rb[KMAX];
    unit_ids<KMAX, NM>(ra, ca, K, F, ksh, fq, gbase);
    unit_ids<KMAX, NM>(rb, cb, K, F, ksh, fq, gbase);
    float4 v1[KMAX], yv[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      v1[k] = ld4(table + (int64_t)ra[k] * D + cq);
      yv[k] = ld4(table + (int64_t)rb[k] * D + cq);
    }
    unit_ids_load<NM>(na, nb, a, cc, uin, gq);
    __builtin_amdgcn_sched_barrier(0);
    // (w1 / w2 as the loop holds them: the compiler kept a second, pairwise copy of both for packed arithmetic through the
    //  whole loop, eight more registers while the rows are in flight)
    float4 w1q = w1, w2q = w2;
    asm volatile("" : "+v"(w1q.x), "+v"(w1q.y), "+v"(w1q.z), "+v"(w1q.w), "+v"(w2q.x), "+v"(w2q.y), "+v"(w2q.z), "+v"(w2q.w));
    // coattn_fwd_kernel zeroes the rows of dead lanes and of k >= K by selects, eight per neighbour.  The same bits with one:
    // a dead lane's score partial is what the arithmetic makes of zero rows (zpart: 0 unless w1 / w2 are not finite), it
    // stores nothing else; k >= K enters neither the scores nor out1 (both test k < K), and out2's sum skips it (adding
    // +0 never changes a sum that started at +0).
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    float zpart = 0.f;
    zpart += dot4(z, w1q) + dot4(z, w2q);
    float4 sum2 = z;
    float part[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      part[k] = 0.f;
      if (k < K) sum2 = add4(sum2, yv[k]);
      part[k] += dot4(v1[k], w1q) + dot4(yv[k], w2q);
      part[k] = ok ? part[k] : zpart;
    }
    float red[KMAX + 1];          // the K partial scores and the target term: reduced across the group together
#pragma unroll
    for (int k = 0; k < KMAX; ++k) red[k] = (k < K) ? part[k] : 0.f;
    red[KMAX] = cpart;
    group_sum_n<KMAX + 1>(red, GS);
    const float cst = red[KMAX] + bias;
    // The next unit's ids are taken up HERE, in front of this unit's stores: they were requested right behind the rows and
    // have long arrived.  Taken up at the top of the next iteration, the wait for them stood behind the stores and, the
    // atten_info loop storing a number of times the compiler cannot count, drained them: vmcnt(0), a round trip per unit.
    unit_ids_clamp<NM>(na, nb, NR, bad1, bad2);
    // (an empty statement that needs the clamped ids: without it the clamp, and the wait with it, sank behind the stores)
    asm volatile("" : "+v"(na.r0), "+v"(nb.r0));
    if constexpr (NM > 1) asm volatile("" : "+v"(na.r1), "+v"(nb.r1));
    static_assert(NM <= 2, "instances: one or two registers per id list");
    __builtin_amdgcn_sched_barrier(0);
    float r[KMAX];
    float rmax = 0.f, rsum = 0.f;  // relu output >= 0
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      r[k] = 0.f;
      if (k < K) {
        r[k] = fmaxf(red[k] + cst, 0.f);
        rmax = fmaxf(rmax, r[k]);
        rsum += r[k];
      }
    }
    // atten_info = [K*r_0..K*r_{K-1}, sum_i r_i (K times)]  (score.py:165-166)
    if (unit_ok) {
      for (int e = gq; e < 2 * K; e += GS) {
        float val = rsum;
        float rv = 0.f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if (e == k) rv = r[k];
        if (e < K) {
          val = (float)K * rv;
          cc.rsave[(int64_t)u * K + e] = rv;
        }
        cc.info[(int64_t)u * cc.ldi + e] = val;
      }
    }
    float p[KMAX];
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      p[k] = (k < K) ? expf(r[k] - rmax) : 0.f;
      den += p[k];
    }
    const float inv_den = 1.0f / den;
    if (ok) {
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) o = fma4(p[k] * inv_den, v1[k], o);
      st4(cc.out1 + (int64_t)u * cc.ld1 + gq * 4, o);
      const float fk = (float)K;
      st4(cc.out2 + (int64_t)u * cc.ld2 + gq * 4, make_float4(sum2.x / fk, sum2.y / fk, sum2.z / fk, sum2.w / fk));
    }
    ca = na; cb = nb;
  }
  if (a.id_status && (bad1 || bad2)) atomicOr(a.id_status, (bad1 ? 1 << cc.bit1 : 0) | (bad2 ? 1 << cc.bit2 : 0));
}

// score_coattn_last_forms (include/score_hip.h): the instance the latest forward / backward launch of this process took --
// process-global words written on the host by whatever names the instance (the launch templates from their own parameters,
// COATTN_DISPATCH in the branch it takes), like score_pull_last_form
static int g_coattn_last_forms[2] = {-1, -1};
static int g_coattn_dispatched[2];      // KMAX, SPL of the instance COATTN_DISPATCH took
extern "C" int score_coattn_last_forms(int32_t backward) { return g_coattn_last_forms[backward ? 1 : 0]; }
static void coattn_note_fwd(int units, int kmax, int spl_or_nm, int ch) {
  g_coattn_last_forms[0] = units | kmax << 1 | spl_or_nm << 8 | (ch > 0xFFFF ? 0xFFFF : ch) << 12;
}
static void coattn_note_bwd(int kmax, int spl, int nm, int atomic, int mode) {
  g_coattn_last_forms[1] = kmax << 1 | spl << 8 | nm << 12 | (atomic ? 1 : 0) << 16 | (mode & 3) << 20;
}
#define COATTN_TOOK(KM, SP) g_coattn_dispatched[0] = KM; g_coattn_dispatched[1] = SP;
#define COATTN_DISPATCH(KERNEL, EXTRA, SPLV, KV, ...)                                                   \
  do {                                                                                                  \
    if (SPLV == 1) {                                                                                    \
      if (KV <= 4) { COATTN_TOOK(4, 1) hipLaunchKernelGGL((KERNEL<4, 1 EXTRA>), __VA_ARGS__); }         \
      else if (KV <= 10) { COATTN_TOOK(10, 1) hipLaunchKernelGGL((KERNEL<10, 1 EXTRA>), __VA_ARGS__); } \
      else if (KV <= 20) { COATTN_TOOK(20, 1) hipLaunchKernelGGL((KERNEL<20, 1 EXTRA>), __VA_ARGS__); } \
      else { COATTN_TOOK(32, 1) hipLaunchKernelGGL((KERNEL<32, 1 EXTRA>), __VA_ARGS__); }               \
    } else if (SPLV == 2) {                                                                             \
      if (KV <= 4) { COATTN_TOOK(4, 2) hipLaunchKernelGGL((KERNEL<4, 2 EXTRA>), __VA_ARGS__); }         \
      else if (KV <= 10) { COATTN_TOOK(10, 2) hipLaunchKernelGGL((KERNEL<10, 2 EXTRA>), __VA_ARGS__); } \
      else if (KV <= 20) { COATTN_TOOK(20, 2) hipLaunchKernelGGL((KERNEL<20, 2 EXTRA>), __VA_ARGS__); } \
      else { COATTN_TOOK(32, 2) hipLaunchKernelGGL((KERNEL<32, 2 EXTRA>), __VA_ARGS__); }               \
    } else {                                                                                            \
      if (KV <= 10) { COATTN_TOOK(10, 4) hipLaunchKernelGGL((KERNEL<10, 4 EXTRA>), __VA_ARGS__); }      \
      else { COATTN_TOOK(20, 4) hipLaunchKernelGGL((KERNEL<20, 4 EXTRA>), __VA_ARGS__); }               \
    }                                                                                                   \
  } while (0)
#define COMMA_TRUE0 , true, 0
#define COMMA_FALSE0 , false, 0
// The backward's instances that hold a unit's metadata one element per lane (SPL <= 2), by the registers per list:
// one where a whole list fits the group (cfg-3: 40 ids and 30 scalars in 64 lanes), two or four otherwise; K <= 10 only.
// Returns false where no instance holds `need` registers: the caller takes the NM = 0 instance.
template <int KMAX, int SPL, bool ATOMIC, int NM>
static void coattn_bwd_launch(int total, size_t lds_bytes, hipStream_t s, const CoattnArgs& a) {
  coattn_note_bwd(KMAX, SPL, NM, ATOMIC, a.mode);
  hipLaunchKernelGGL((coattn_bwd_kernel_t<KMAX, SPL, ATOMIC, NM>), dim3(total), dim3(256), lds_bytes, s, a);
}
template <int SPL, bool ATOMIC>
static bool coattn_bwd_ahead(int need, int total, size_t lds_bytes, hipStream_t s, const CoattnArgs& a) {
  const int K = a.K;
  if (need < 1 || need > 4) return false;
  if (K <= 4) {
    if (need > 2) return false;
    if (need == 1) coattn_bwd_launch<4, SPL, ATOMIC, 1>(total, lds_bytes, s, a);
    else coattn_bwd_launch<4, SPL, ATOMIC, 2>(total, lds_bytes, s, a);
  } else if (K <= 10) {
    if (need == 1) coattn_bwd_launch<10, SPL, ATOMIC, 1>(total, lds_bytes, s, a);
    else if (need == 2) coattn_bwd_launch<10, SPL, ATOMIC, 2>(total, lds_bytes, s, a);
    else coattn_bwd_launch<10, SPL, ATOMIC, 4>(total, lds_bytes, s, a);
  } else {
    // K > 10: the 256-register instances neither spill nor wait on scratch in the NM = 0 form, and at cfg-5 (K = 20,
    // 3.2 ms of row requests per launch) the shuffles cost more than the waits they save: 3.17 -> 3.50 ms measured
    return false;
  }
  return true;
}

static int coattn_check(const void* table, int64_t n_rows, int D, int F, int K, int B, int T) {
  if (!table || n_rows <= 0 || B <= 0 || T <= 0) return SCORE_E_BADARG;
  if (D <= 0 || (D & 3) || D > 256 || F <= 0 || K <= 0 || K > 32) return SCORE_E_SHAPE;
  if (F * (D / 4) > 256) return SCORE_E_SHAPE;
  if (F * (D / 4) > 128 && K > 20) return SCORE_E_SHAPE;
  return 0;
}

// The forward's several-units-per-wave form (coattn_fwd_kernel_units): registers per id list of a call (ids only: the
// backward's lists also hold 3K scalars), 0 where a feature set does not fit a group
static inline int coattn_fwd_id_regs(int GS, int F, int K) {
  const int ksh = coattn_ksh(GS, F);
  return ksh < 0 ? 0 : (K + (1 << ksh) - 1) >> ksh;
}
// Registers per list of the instance that serves every call of a launch; 0: coattn_fwd_kernel (mode != 0, K > 10, more
// than one slot per lane, lists longer than an instance holds).  Instances: one or two registers at K <= 4, one at
// K <= 10 -- with two or four, the KMAX = 10 kernel no longer fits 128 registers (8 and 13 spilled: the lists are 2 x 2
// per register, and the selects between them hold more), and a spilled loop is what this form is there to avoid.
static int coattn_fwd_units_regs(int D, int K, int mode, int ncalls, const int* F) {
  if (mode != 0 || K > 10) return 0;
  int need = 1;
  for (int c = 0; c < ncalls; ++c) {
    int GS, SPL, nslots;
    coattn_geom(D, F[c], &GS, &SPL, &nslots);
    const int n = coattn_fwd_id_regs(GS, F[c], K);
    if (SPL != 1 || n == 0 || n > (K <= 4 ? 2 : 1)) return 0;
    need = n > need ? n : need;
  }
  return need;
}
// Time slices per chunk, from the shape alone.  A wave makes two round trips per chunk (ids and constants, then the
// target row) and one per unit, so longer chunks mean fewer trips per unit -- and fewer waves, each with more to do
// behind the others.  COATTN_FWD_SLOTS waves are resident at once (256 CUs x 4 SIMDs x 4 waves of <= 128 VGPRs).  Two
// slices where that still leaves two full rounds of them, one slice otherwise: a launch that cannot fill the machine
// twice is over soonest with every unit in flight at once.  Measured at cfg-3 (B = 1024, 18 slices, 2 calls; the kernel
// in the step, then alone on the low-duplication probe; coattn_fwd_kernel: 94.2 and 172.0 us): 1 slice 85.9 / 169.7 us,
// 2: 78.3 / 171.4, 3: 80.2 / 174.6, 4: 80.1 / 174.6, 6: 79.0 and 81.7 / 179.7 and 180.8, 9: 86.9 / 187.0 -- past two,
// nothing more comes off the step's kernel, and the memory-bound probe loses a little with every slice added
// (profiles/coattn_fwd_units.md section 4).
static const int COATTN_FWD_SLOTS = 4096;
int score_coattn_fwd_chunk_rule(int D, int K, int B, int T, int ncalls, const int* F) {
  if (coattn_fwd_units_regs(D, K, 0, ncalls, F) == 0) return 0;
  int64_t waves = 0;      // with two slices per chunk
  for (int c = 0; c < ncalls; ++c) {
    int GS, SPL, nslots;
    coattn_geom(D, F[c], &GS, &SPL, &nslots);
    waves += cdiv64((int64_t)B * ((T + 1) / 2), 64 / GS);
  }
  return waves >= 2 * COATTN_FWD_SLOTS ? 2 : 1;
}
template <int KMAX, int NM>
static void coattn_fwd_units_launch(int total, hipStream_t s, const CoattnArgs& a) {
  coattn_note_fwd(1, KMAX, NM, a.CH);
  hipLaunchKernelGGL((coattn_fwd_kernel_units<KMAX, NM>), dim3(total), dim3(256), 0, s, a);
}

// Launch 1 or 2 calls (ncalls) of the forward in a single grid.
int score_coattn_fwd_multi(CoattnArgs& a, int ncalls, int D, int B, hipStream_t s) {
  int spl = 1, total = 0;
  a.D4 = D / 4;
  a.n_units = B * a.T;
  if (a.Tidx <= 0) a.Tidx = a.T;
  if (a.n_rows == 0) a.n_rows = 0x80000000u;      // (no row count given: int32 ids >= 0 pass)
  // several units per wave wherever an instance holds the id lists of every call (a.CH > 0 on entry: that chunk length
  // instead of the rule's, for measurements)
  const int Fs[2] = {a.c[0].F, a.c[ncalls > 1 ? 1 : 0].F};
  const int nm = a.fwd_one_unit ? 0 : coattn_fwd_units_regs(D, a.K, a.mode, ncalls, Fs);
  if (nm > 0) {
    if (a.CH <= 0) a.CH = score_coattn_fwd_chunk_rule(D, a.K, B, a.T, ncalls, Fs);
    a.cps = (a.T + a.CH - 1) / a.CH;
    a.n_chunks = B * a.cps;
    for (int c = 0; c < 2; ++c) {
      if (c >= ncalls) { a.c[c] = a.c[0]; a.c[c].first_block = 0x7fffffff; continue; }
      int SPLc;
      coattn_geom(D, a.c[c].F, &a.c[c].GS, &SPLc, &a.c[c].nslots);
      a.c[c].ksh = coattn_ksh(a.c[c].GS, a.c[c].F);
      a.c[c].first_block = total;
      total += (int)cdiv64(cdiv64(a.n_chunks, 64 / a.c[c].GS), 4);
    }
    if (a.K <= 4) {
      if (nm == 1) coattn_fwd_units_launch<4, 1>(total, s, a);
      else coattn_fwd_units_launch<4, 2>(total, s, a);
    } else {
      coattn_fwd_units_launch<10, 1>(total, s, a);
    }
    SCORE_CHECK_LAUNCH();
    return 0;
  }
  for (int c = 0; c < 2; ++c) {
    if (c >= ncalls) { a.c[c] = a.c[0]; a.c[c].first_block = 0x7fffffff; continue; }
    int SPLc;
    coattn_geom(D, a.c[c].F, &a.c[c].GS, &SPLc, &a.c[c].nslots);
    if (SPLc > spl) spl = SPLc;
    a.c[c].first_block = total;
    total += (int)cdiv64(cdiv64(a.n_units, 64 / a.c[c].GS), 4);
  }
  if (spl == 3) spl = 4;
  COATTN_DISPATCH(coattn_fwd_kernel, , spl, a.K, dim3(total), dim3(256), 0, s, a);
  coattn_note_fwd(0, g_coattn_dispatched[0], g_coattn_dispatched[1], 0);
  SCORE_CHECK_LAUNCH();
  return 0;
}

// Backward of 1 or 2 calls in a single grid + the per-call slab reductions into dW[c] (+=).
int score_coattn_bwd_multi(CoattnArgs& a, int ncalls, int D, int B, float* const dW[2], float* scratch,
                           int64_t scratch_floats, int atomic_scatter, ColsumJobs* cq, hipStream_t s) {
  int spl = 1, total = 0, nblk[2] = {0, 0};
  size_t lds_bytes = 0;
  int64_t used = 0;
  a.D4 = D / 4;
  a.n_units = B * a.T;
  if (a.Tidx <= 0) a.Tidx = a.T;
  if (a.n_rows == 0) a.n_rows = 0x80000000u;
  for (int c = 0; c < 2; ++c) {
    if (c >= ncalls) { a.c[c] = a.c[0]; a.c[c].first_block = 0x7fffffff; continue; }
    int SPLc;
    coattn_geom(D, a.c[c].F, &a.c[c].GS, &SPLc, &a.c[c].nslots);
    if (SPLc > spl) spl = SPLc;
    int upw = 64 / a.c[c].GS, Dx = a.c[c].nslots * 4;
    int blocks = (int)cdiv64(cdiv64(a.n_units, upw), 4);
    if (blocks > 512) blocks = 512;
    nblk[c] = blocks;
    a.c[c].first_block = total;
    total += blocks;
    a.c[c].slab = scratch + used;
    used += (int64_t)blocks * 2 * Dx;
    size_t l = (size_t)4 * upw * 2 * Dx * sizeof(float);
    if (l > lds_bytes) lds_bytes = l;
  }
  if (a.mode == 0 && used > scratch_floats) return SCORE_E_WORKSPACE;
  if (spl == 3) spl = 4;
  // one element per lane and a unit ahead where the lists of both calls fit an instance's registers
  int need = (a.mode == 0 && spl <= 2) ? 1 : 0;
  for (int c = 0; c < ncalls && need > 0; ++c) {
    const int n = coattn_meta_regs(a.c[c].GS, a.c[c].F, a.K);
    need = n == 0 ? 0 : n > need ? n : need;
  }
  for (int c = 0; c < 2; ++c) a.c[c].ksh = need > 0 ? coattn_ksh(a.c[c].GS, a.c[c].F) : 0;
  bool ahead;
  if (spl == 1) ahead = atomic_scatter ? coattn_bwd_ahead<1, true>(need, total, lds_bytes, s, a) : coattn_bwd_ahead<1, false>(need, total, lds_bytes, s, a);
  else if (spl == 2) ahead = atomic_scatter ? coattn_bwd_ahead<2, true>(need, total, lds_bytes, s, a) : coattn_bwd_ahead<2, false>(need, total, lds_bytes, s, a);
  else ahead = false;
  if (!ahead) {
    if (atomic_scatter) COATTN_DISPATCH(coattn_bwd_kernel_t, COMMA_TRUE0, spl, a.K, dim3(total), dim3(256), lds_bytes, s, a);
    else COATTN_DISPATCH(coattn_bwd_kernel_t, COMMA_FALSE0, spl, a.K, dim3(total), dim3(256), lds_bytes, s, a);
    coattn_note_bwd(g_coattn_dispatched[0], g_coattn_dispatched[1], 0, atomic_scatter, a.mode);
  }
  SCORE_CHECK_LAUNCH();
  if (a.mode == 0) {
    for (int c = 0; c < ncalls; ++c) {
      int Dx = a.c[c].nslots * 4;
      if (cq) SCORE_TRY(colsum_queue_add(cq, a.c[c].slab, nblk[c], 2 * Dx, 2 * Dx, dW[c] + Dx, 1));
      else SCORE_TRY(score_launch_colsum(a.c[c].slab, nblk[c], 2 * Dx, 2 * Dx, dW[c] + Dx, 1, scratch + used,
                                         scratch_floats - used, s));
    }
  }
  return 0;
}

extern "C" int score_coattn_fwd_chunk(int32_t D, int32_t K, int32_t B, int32_t T, int32_t F0, int32_t F1) {
  if (D <= 0 || (D & 3) || K <= 0 || B <= 0 || T <= 0 || F0 <= 0 || F1 < 0) return SCORE_E_BADARG;
  const int F[2] = {F0, F1};
  return score_coattn_fwd_chunk_rule(D, K, B, T, F1 > 0 ? 2 : 1, F);
}

// ABI wrappers: one call; `tgt` is [B, F*D] contiguous
extern "C" int score_coattn_fwd(const float* table, int64_t n_rows, int32_t D, int32_t F, int32_t K,
                                int32_t B, int32_t T, const int32_t* idx1, const int32_t* idx2,
                                const float* tgt, const float* W, const float* bias, float* out1,
                                int32_t ld1, float* out2, int32_t ld2, float* info, int32_t ldi,
                                float* rsave, int32_t mode, void* stream) {
  SCORE_TRY(coattn_check(table, n_rows, D, F, K, B, T));
  if (!idx1 || !idx2 || !out1 || !out2) return SCORE_E_BADARG;
  if (mode == 0 && (!tgt || !W || !bias || !info || !rsave)) return SCORE_E_BADARG;
  if ((ld1 & 3) || (ld2 & 3)) return SCORE_E_SHAPE;
  CoattnArgs a;
  memset(&a, 0, sizeof(a));
  a.table = table; a.K = K; a.T = T; a.mode = mode; a.n_rows = (uint32_t)(n_rows < 0x80000000ll ? n_rows : 0x80000000ll);
  CoattnCall& c = a.c[0];
  c.idx1 = idx1; c.idx2 = idx2; c.tgt = tgt; c.ldt = F * D; c.W = W; c.bias = bias;
  c.out1 = out1; c.ld1 = ld1; c.out2 = out2; c.ld2 = ld2; c.info = info; c.ldi = ldi; c.rsave = rsave; c.F = F;
  return score_coattn_fwd_multi(a, 1, D, B, (hipStream_t)stream);
}

extern "C" int score_coattn_bwd(const float* table, float* grad_table, int64_t n_rows, int32_t D, int32_t F,
                                int32_t K, int32_t B, int32_t T, const int32_t* idx1, const int32_t* idx2,
                                const float* W, const float* rsave, const float* g1, int32_t ld1,
                                const float* g2, int32_t ld2, const float* ginfo, int32_t ldi, float* dzsum,
                                float* dW, float* scratch, int64_t scratch_floats, int32_t mode, void* stream) {
  SCORE_TRY(coattn_check(table, n_rows, D, F, K, B, T));
  if (!grad_table || !idx1 || !idx2 || !g1 || !g2) return SCORE_E_BADARG;
  if (mode == 0 && (!W || !rsave || !ginfo || !dzsum || !dW || !scratch)) return SCORE_E_BADARG;
  if ((ld1 & 3) || (ld2 & 3)) return SCORE_E_SHAPE;
  CoattnArgs a;
  memset(&a, 0, sizeof(a));
  a.table = table; a.gtable = grad_table; a.K = K; a.T = T; a.mode = mode;
  a.n_rows = (uint32_t)(n_rows < 0x80000000ll ? n_rows : 0x80000000ll);
  CoattnCall& c = a.c[0];
  c.idx1 = idx1; c.idx2 = idx2; c.W = W; c.rsave = const_cast<float*>(rsave); c.g1 = g1; c.ld1 = ld1; c.g2 = g2; c.ld2 = ld2;
  c.ginfo = ginfo; c.ldi = ldi; c.dzsum = dzsum; c.F = F;
  float* dWs[2] = {dW, nullptr};
  return score_coattn_bwd_multi(a, 1, D, B, dWs, scratch, scratch_floats, 1, nullptr, (hipStream_t)stream);
}

// ------------------------------------------------------------------ target rows (score.py:62-66, 210, 217)
__global__ void target_fwd_kernel(const float* __restrict__ table, int D4, int Fu, int Fi, int B,
                                  const int32_t* __restrict__ tu, const int32_t* __restrict__ ti,
                                  float* __restrict__ query, int ldq, float* __restrict__ head, int ldh,
                                  int off_ti, int off_tu, uint32_t n_rows, int32_t* __restrict__ id_status) {
  const int cu = Fu * D4, ci = Fi * D4;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * (cu + ci)) return;
  int b = (int)(i / (cu + ci));
  int s = (int)(i - (int64_t)b * (cu + ci));
  if (s < cu) {  // target_user slot
    int fidx = s / D4, c = s - fidx * D4;
    uint32_t row = (uint32_t)tu[b * Fu + fidx];
    if (row >= n_rows) {        // outside the table: the dummy row, reported (bit 4 = target_user)
      row = 0;
      if (id_status && c == 0) atomicOr(id_status, 1 << 4);
    }
    float4 v = ld4(table + ((int64_t)row * D4 + c) * 4);
    if (query) st4(query + (int64_t)b * ldq + s * 4, v);
    st4(head + (int64_t)b * ldh + off_tu + s * 4, v);
  } else {
    int s2 = s - cu;
    int fidx = s2 / D4, c = s2 - fidx * D4;
    uint32_t row = (uint32_t)ti[b * Fi + fidx];
    if (row >= n_rows) {        // (bit 5 = target_item)
      row = 0;
      if (id_status && c == 0) atomicOr(id_status, 1 << 5);
    }
    float4 v = ld4(table + ((int64_t)row * D4 + c) * 4);
    if (query) st4(query + (int64_t)b * ldq + cu * 4 + s2 * 4, v);
    st4(head + (int64_t)b * ldh + off_ti + s2 * 4, v);
  }
}

int score_launch_target_fwd(const float* table, int D, int Fu, int Fi, int B, const int32_t* tu,
                            const int32_t* ti, float* query, int ldq, float* head, int ldh, int off_ti,
                            int off_tu, hipStream_t s, int64_t n_rows, int32_t* id_status) {
  int64_t n = (int64_t)B * (Fu + Fi) * (D / 4);
  const uint32_t nr = (n_rows <= 0 || n_rows > 0x80000000ll) ? 0x80000000u : (uint32_t)n_rows;
  hipLaunchKernelGGL(target_fwd_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, s, table, D / 4, Fu, Fi, B,
                     tu, ti, query, ldq, head, ldh, off_ti, off_tu, nr, id_status);
  SCORE_CHECK_LAUNCH();
  return 0;
}

// d target rows = dquery + dhead + S * w_t ; scatter-add into the table gradient.
// S[c][b] = sum_t dzsum_c[b*T+t] (c = 0: co-attention 1, whose target is the item; c = 1: the user) is summed here by
// every thread that needs it, in t order (the few rows of dzsum a block reads sit in L1), and stored once per (c, b)
// for the weight / bias gradients queued behind this launch -- it was a launch of its own in front of this one, two
// 5-us kernels on the critical path between the co-attention backward and the row scatter.
__global__ void target_bwd_kernel(float* __restrict__ gtable, int D4, int Fu, int Fi, int B, int T,
                                  const int32_t* __restrict__ tu, const int32_t* __restrict__ ti,
                                  const float* __restrict__ dquery, int ldq, const float* __restrict__ dhead,
                                  int ldh, int off_ti, int off_tu, const float* __restrict__ W1,
                                  const float* __restrict__ W2, const float* __restrict__ dz1,
                                  const float* __restrict__ dz2, float* __restrict__ S,
                                  float* __restrict__ dtgt, uint32_t n_rows) {
  const int cu = Fu * D4, ci = Fi * D4;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * (cu + ci)) return;
  int b = (int)(i / (cu + ci));
  int s = (int)(i - (int64_t)b * (cu + ci));
  float4 g;
  int64_t row;
  int c;
  const bool user = s < cu;
  float Sb = 0.f;
  if (S) {       // (co-attention models only)
    const float* src = user ? dz2 : dz1;
    if (src)
      for (int t = 0; t < T; ++t) Sb += src[(int64_t)b * T + t];
    if (s == 0) S[B + b] = Sb;
    if (s == cu) S[b] = Sb;
  }
  if (user) {
    int fidx = s / D4;
    c = s - fidx * D4;
    row = tu[b * Fu + fidx];
    g = ld4(dhead + (int64_t)b * ldh + off_tu + s * 4);
    if (dquery) g = add4(g, ld4(dquery + (int64_t)b * ldq + s * 4));
    if (W2) g = fma4(Sb, ld4(W2 + s * 4), g);  // co-attention 2 targets the user (score.py:197)
  } else {
    int s2 = s - cu;
    int fidx = s2 / D4;
    c = s2 - fidx * D4;
    row = ti[b * Fi + fidx];
    g = ld4(dhead + (int64_t)b * ldh + off_ti + s2 * 4);
    if (dquery) g = add4(g, ld4(dquery + (int64_t)b * ldq + cu * 4 + s2 * 4));
    if (W1) g = fma4(Sb, ld4(W1 + s2 * 4), g);     // co-attention 1 targets the item (score.py:196)
  }
  if (dtgt) {  // pull mode: hand the [B, Du+Di] row gradients to the sorted scatter
    st4(dtgt + (int64_t)b * (cu + ci) * 4 + s * 4, g);
  } else if (row != 0 && (uint64_t)row < n_rows) {      // (an id outside the table was read as the dummy row)
    atomic_add4(gtable + (row * D4 + c) * 4, g);
  }
}

int score_launch_target_bwd(float* grad_table, int D, int Fu, int Fi, int B, int T, const int32_t* tu,
                            const int32_t* ti, const float* dquery, int ldq, const float* dhead, int ldh,
                            int off_ti, int off_tu, const float* query, const float* W1, const float* W2,
                            const float* dzsum1, const float* dzsum2, float* S, float* dW1, float* dB1,
                            float* dW2, float* dB2, float* dtgt_out, float* scratch, int64_t scratch_floats,
                            ColsumJobs* cq, GemmQueue* gq, hipStream_t s, int64_t n_rows) {
  const bool coattn = W1 != nullptr;
  int64_t n = (int64_t)B * (Fu + Fi) * (D / 4);
  hipLaunchKernelGGL(target_bwd_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, s, grad_table, D / 4, Fu,
                     Fi, B, T, tu, ti, dquery, ldq, dhead, ldh, off_ti, off_tu, W1, W2, dzsum1, dzsum2,
                     coattn ? S : nullptr, dtgt_out,
                     (n_rows <= 0 || n_rows > 0x80000000ll) ? 0x80000000u : (uint32_t)n_rows);
  SCORE_CHECK_LAUNCH();
  if (coattn) {
    // dW_t = tgt^T S (call 0 targets the item: query cols Du.., call 1 the user: cols 0..), dbias = sum_b S
    const int Du = Fu * D, Di = Fi * D;
    if (cq) {   // one output column each: row-weighted column sums with the pass's other column sums (query and S stay
                // untouched until they run) -- as queued GEMM jobs they alone kept a launch of the f32 GEMM kernel in the end-of-pass
                // flush at cfg-3
      SCORE_TRY(colsum_queue_add(cq, query + Du, B, Di, ldq, dW1, 0, S));
      SCORE_TRY(colsum_queue_add(cq, query, B, Du, ldq, dW2, 0, S + B));
    } else if (gq) {
      SCORE_TRY(gemm_queue_add(gq, Di, 1, B, query + Du, ldq, S, 1, dW1, 1));
      SCORE_TRY(gemm_queue_add(gq, Du, 1, B, query, ldq, S + B, 1, dW2, 1));
    } else {
      SCORE_TRY(score_gemm(2, Di, 1, B, query + Du, ldq, S, 1, dW1, 1, nullptr, 0, 1.f, nullptr, 0, scratch,
                           scratch_floats, s));
      SCORE_TRY(score_gemm(2, Du, 1, B, query, ldq, S + B, 1, dW2, 1, nullptr, 0, 1.f, nullptr, 0, scratch,
                           scratch_floats, s));
    }
    if (cq) {
      SCORE_TRY(colsum_queue_add(cq, S, B, 1, 1, dB1, 0));
      SCORE_TRY(colsum_queue_add(cq, S + B, B, 1, 1, dB2, 0));
    } else {
      SCORE_TRY(score_launch_colsum(S, B, 1, 1, dB1, 0, scratch, scratch_floats, s));
      SCORE_TRY(score_launch_colsum(S + B, B, 1, 1, dB2, 0, scratch, scratch_floats, s));
    }
  }
  return 0;
}
