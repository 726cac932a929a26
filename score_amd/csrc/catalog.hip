// Top-K over a whole item catalogue for the point baselines with a line-form head (GRU4Rec, Caser): score_catalog_build /
// score_catalog_topk (include/score_hip.h).  rank.hip splits fc1's pre-activation of a (line, candidate) pair by the columns of
// the head input; with the WHOLE catalogue as the candidate set the candidate half no longer depends on the call at all:
//   z1[l, n] = zline[l] + zcat[n],   zcat[n] = bn1(item_n) . W1[item rows]       (no bias: fc1's bias is in zline, once)
// catalog_zcat_kernel computes zcat [N, 200] once per catalogue and weight state: the first stage of rank_tile_kernel without a
// line.  catalog_score_kernel, a workgroup per (line, chunk of the catalogue), then has per pair relu(zline + zcat[n]), fc2
// (200 x 80), fc3 and a comparison against the K-th best so far; catalog_merge_kernel, a workgroup per line, reduces the
// chunks' lists.  score_catalog_topk_in scores, per line, only a list of catalogue indices: the same kernel body instantiated
// with CAND, which walks list positions and gathers its rows through the list (see catalog_score_kernel).
//
// The order.  Pairs are ordered by descending fc3 logit, ties by ascending catalogue index, NaN behind every number: a TOTAL
// order, held as one 64-bit key per pair -- (the logit's bits made monotone, NaN -> 0) << 32 | ~index -- whose unsigned
// comparison IS the order (ct_key).  Key 0 is the empty slot (index -1, logit -inf): below every pair.  Since the order is total
// the K best of a line do not depend on how the catalogue is cut into steps and chunks.
//
// Row sums.  Every row of every step goes through the same instruction sequence (the MFMA's own sum over its four k, the same
// 52 steps, the same four-lane fc3 sum), so equal inputs give equal bits wherever the row lies.
//
// No atomics but the idempotent OR of the id report; no workgroup waits on another.  All LDS is dynamic, every carve offset a
// multiple of 16 bytes.
#include "common.h"
#include "kernels.h"
#include "head_tiles.h"      // hf_tiles, HB_K1Q
#include "devprep.h"         // dp_lower_bound

namespace {

typedef unsigned long long ct_u64;

constexpr int CT_N1 = 200, CT_N2 = 80;        // fc1 / fc2 outputs (the head's fixed widths)
constexpr int CT_KQ = HB_K1Q;                 // fc2's k-steps per lane quarter: K = 200 padded to 208
constexpr int CT_LD1 = 4 * CT_KQ + 4;         // LDS row stride of relu(z1): 212 floats
constexpr int CT_LD2 = CT_N2 + 4;             // ... of relu(z2): 84
constexpr int CT_ROWS = 32;                   // pairs per step: two MFMA row tiles, i.e. two independent accumulator chains per wave
constexpr int CT_MW = CT_N2 / 16;             // matrix waves: one per column tile of fc2 (5)
constexpr int CT_NW = CT_MW + 1;              // + the selection wave
constexpr int CT_EXCL = 512;                  // exclusion entries of a chunk staged in LDS (more: searched in global memory)
constexpr int CT_Q4 = CT_ROWS * (CT_N1 / 4) / (64 * CT_MW);      // 16-byte groups of a step's zcat rows per matrix-wave thread (5)
static_assert(CT_ROWS * (CT_N1 / 4) == CT_Q4 * 64 * CT_MW, "a step's zcat rows split evenly over the matrix waves");
static_assert(SCORE_CATALOG_KMAX == 128, "a lane of the selection wave holds two list entries");

__device__ __forceinline__ ct_u64 ct_key(float v, int n) {
  uint32_t b = __float_as_uint(v);
  if (v == 0.f) b = 0u;                                                          // (-0 orders as +0)
  const uint32_t u = (v != v) ? 0u : ((b & 0x80000000u) ? ~b : (b | 0x80000000u));
  return ((ct_u64)u << 32) | (uint32_t)~(uint32_t)n;
}
__device__ __forceinline__ int ct_key_index(ct_u64 key) { return (int)~(uint32_t)key; }
__device__ __forceinline__ float ct_key_logit(ct_u64 key) {
  const uint32_t u = (uint32_t)(key >> 32);
  if (key == 0ull) return __uint_as_float(0xFF800000u);                          // the empty slot: -inf
  if (u == 0u) return __uint_as_float(0x7FC00000u);                              // NaN
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// The K best keys so far, descending, in the registers of ONE wave: rank j in e0 of lane j (j < 64) or e1 of lane j - 64.
// x (wave-uniform) goes where the first smaller entry is; everything behind moves one rank down (rank 127 falls out).
__device__ __forceinline__ void ct_insert(ct_u64& e0, ct_u64& e1, ct_u64 x, int lane) {
  const ct_u64 last0 = __shfl(e0, 63, 64);
  ct_u64 p0 = __shfl_up(e0, 1, 64), p1 = __shfl_up(e1, 1, 64);
  if (lane == 0) { p0 = ~0ull; p1 = last0; }
  e0 = e0 > x ? e0 : (p0 > x ? x : p0);
  e1 = e1 > x ? e1 : (p1 > x ? x : p1);
}
__device__ __forceinline__ ct_u64 ct_kth(ct_u64 e0, ct_u64 e1, int k) {
  return __shfl(k > 64 ? e1 : e0, (k - 1) & 63, 64);
}

// zcat[n, :] for the tile of HF_ROWS catalogue items blockIdx.x: the Fi table rows -> bn1's affine of the item columns -> LDS,
// one hf_tiles product against W1's item rows; no bias, no relu
__global__ __launch_bounds__(64 * HF_NW) void catalog_zcat_kernel(const CatalogArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int Di = a.Di, N1 = a.N1, N = a.N;
  const int Kp0 = (Di + 15) & ~15, LD0 = Kp0 + 4;
  float* xs = sm;                          // [16][LD0]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lc = lane & 15, lq = lane >> 4;
  const int r0 = (int)blockIdx.x * HF_ROWS;
  for (int e = tid; e < HF_ROWS * LD0; e += 64 * HF_NW) xs[e] = 0.f;       // rows past N and the K padding
  __syncthreads();
  {
    const int n4 = Di >> 2, D4 = a.D >> 2, Fi = Di / a.D;
    for (int e = tid; e < HF_ROWS * n4; e += 64 * HF_NW) {
      const int i = e / n4, j4 = e - i * n4;
      const int f = j4 / D4, cc = j4 - f * D4;
      const int n = r0 + i;
      const bool ok = n < N;
      uint32_t row = (uint32_t)a.item_rows[(int64_t)(ok ? n : N - 1) * Fi + f];
      if (row >= a.n_rows) {        // outside the table: the dummy row, reported (bit 5 = the item's tensor)
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
  const float* W1i = a.W1 + (int64_t)a.off_ti * N1;
  const int nt1 = (N1 + 15) >> 4;
  for (int tb = 0; tb < nt1; tb += 2 * HF_NW) {
    hf_f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const int t0 = tb + wave, t1 = tb + HF_NW + wave;
    const int n0[2] = {t0 < nt1 ? t0 * 16 : -1, t1 < nt1 ? t1 * 16 : -1};
    if (n0[0] >= 0) hf_tiles<2>(acc, xs, LD0, Kp0, Di, W1i, N1, n0, N1, lc, lq);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int col = n0[t] + lc;
      if (n0[t] < 0 || col >= N1) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = r0 + lq * 4 + r;
        if (n < N) a.zcat[(int64_t)n * N1 + col] = acc[t][r];
      }
    }
  }
}

inline size_t catalog_zcat_lds(int Di) { return (size_t)HF_ROWS * (((Di + 15) & ~15) + 4) * sizeof(float); }

// LDS of the scoring kernel, in floats: relu(z1) and relu(z2) of a step, two buffers each; the line's zline; the staged exclusions;
// behind them, in the candidate form only, CT_CSLOTS steps' catalogue indices
constexpr int CT_CSLOTS = 4;                  // a step's indices live from two steps ahead of its rows to the selection a step behind
constexpr int CT_SM_F1 = 0, CT_SM_F2 = CT_SM_F1 + 2 * CT_ROWS * CT_LD1, CT_SM_ZL = CT_SM_F2 + 2 * CT_ROWS * CT_LD2,
              CT_SM_EX = CT_SM_ZL + CT_N1, CT_SM_FLOATS = CT_SM_EX + CT_EXCL, CT_SM_CI = CT_SM_FLOATS,
              CT_SM_FLOATS_IN = CT_SM_CI + CT_CSLOTS * CT_ROWS;
static_assert(CT_SM_F2 % 4 == 0 && CT_SM_ZL % 4 == 0 && CT_SM_EX % 4 == 0 && CT_SM_CI % 4 == 0, "16-byte carve offsets");
static_assert(2 * CT_SM_FLOATS * 4 <= 160 * 1024 && 2 * CT_SM_FLOATS_IN * 4 <= 160 * 1024, "two workgroups per compute unit");
// the counting form (RANKS) adds, behind either carve, one flag per row of a step: the row is in the line's exclusions
constexpr int CT_SM_RK = CT_ROWS;
static_assert(CT_SM_FLOATS % 4 == 0 && CT_SM_FLOATS_IN % 4 == 0, "16-byte carve offsets");
static_assert(2 * (CT_SM_FLOATS + CT_SM_RK) * 4 <= 160 * 1024 && 2 * (CT_SM_FLOATS_IN + CT_SM_RK) * 4 <= 160 * 1024,
              "two workgroups per compute unit, counting form");
static_assert(SCORE_CATALOG_TMAX == CT_ROWS, "a line's targets are one step of rows");
static_assert(SCORE_CATALOG_RPART >= 2 * SCORE_CATALOG_TMAX + 1, "32 counts, 32 flags, the live count");

// Workgroup blockIdx.x = l * nchunk + ch: line l against the catalogue items [ch * chunk, min(N, (ch + 1) * chunk)), CT_ROWS a
// step.  Waves 0 .. 4 hold fc2 as MFMA B fragments in registers, one column tile each (52 values a lane: W2 is read ONCE per
// workgroup), and run a step's two row tiles as two independent accumulator chains; the next step's zcat rows are requested
// before the MFMAs issue and go into the other relu(z1) buffer behind them.  Wave 5 holds fc3 and the K best keys in
// registers and works one step behind the matrix waves, on the other relu(z2) buffer: fc3 as rank_tile_kernel sums it (four
// lanes a pair, fixed order), then only the pairs whose key beats the current K-th -- rare after the first steps -- are looked
// up in the line's exclusions and inserted.  One barrier per step.
//
// CAND, the candidate form (score_catalog_topk_in): [c0, c1) are POSITIONS of line l's list cand_idx[cand_off[l] ..
// cand_off[l + 1]) -- the last chunk's workgroup walks to the list's end, however long -- and a step's rows are
// zcat[cand_idx[pos]]; the key carries that catalogue index, so the merge and the outputs are those of the whole form.  The
// dependent index load stays off the step: while step t runs, the selection wave puts the 32 indices of step t + 2 into slot
// (t + 2) % CT_CSLOTS of an LDS array (four slots: the selection reads step t - 1's while fetch reads step t + 1's), ordered by
// the step's one barrier; only the first two steps' indices are read straight from global memory.  An index outside [0, N)
// reads row 0, gets no key and NaN in cand_logits.  A workgroup whose range is empty writes k empty keys and returns.
//
// RANKS, the counting form (score_catalog_ranks / score_catalog_ranks_in): "how many pairs of the line stand ahead of target
// j", for up to 32 targets a line, in place of the K best.  The targets' own logits come from a PROLOGUE step in every
// workgroup -- the loop starts at t = -1 with the rows zcat[tgt_idx[..]] in buffer 1, the same MFMA steps and the same
// four-lane fc3 sum as any row, so their bits are the pair's own (row sums, above) -- and their keys stay in lanes 0 .. 31 of
// the selection wave.  (The other route, a score_catalog_topk_in launch over the target lists, was not taken: it brings W2 in
// again for every line and adds two launches, where the prologue is one step among at least eight and needs no array.)
// Behind it the selection wave takes every live pair of a step: the exclusion test (whole form, staged: the step's excluded
// rows as 32 flags in LDS, set from a cursor that walks the ascending staged list -- no search, no global load; otherwise the
// search select does), then per target popc(ballot(key > target's key)) into lane j's counter, the live count, and a note
// when a pair IS the target (1: counted, 2: excluded).  The chunk's partials go to rpart; catalog_ranks_reduce_kernel adds
// them.  Chunk 0's workgroup writes tgt_logit, and for that runs its prologue even where a candidate list is empty.
// (RANKS asks for three waves a SIMD, i.e. at most 168 registers: without the bound the allocator takes 182 and the second
// workgroup of a compute unit no longer fits; 0 sets nothing, so the top-K instantiations compile as they did.)
template <bool CAND, bool RANKS = false>
__global__ __launch_bounds__(64 * CT_NW) __attribute__((amdgpu_waves_per_eu(RANKS ? 3 : 0))) void catalog_score_kernel(const CatalogArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* f1s = sm + CT_SM_F1;
  float* f2s = sm + CT_SM_F2;
  float* zl = sm + CT_SM_ZL;
  uint32_t* exs = reinterpret_cast<uint32_t*>(sm + CT_SM_EX);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lc = lane & 15, lq = lane >> 4;
  const int N = a.N, k = a.k;
  const int l = (int)blockIdx.x / a.nchunk, ch = (int)blockIdx.x - l * a.nchunk;
  int c0_, c1_;
  const int32_t* cand = nullptr;              // line l's list (CAND)
  int* cis = nullptr;                         // [CT_CSLOTS][CT_ROWS] catalogue indices of the steps in flight (CAND)
  // RANKS: the line's targets tgt_idx[tlo .. tlo + nt), the first max_targets of them; a longer line is reported (bit 1)
  int64_t tlo = 0;
  int nt = 0;
  int32_t* rp = nullptr;                      // this workgroup's partials
  int* xfl = nullptr;                         // [CT_ROWS] the step's rows that are excluded (whole form, staged)
  if constexpr (RANKS) {
    tlo = a.tgt_off[l];
    const int64_t c = a.tgt_off[l + 1] - tlo;
    nt = (int)(c < (int64_t)a.max_targets ? (c > 0 ? c : 0) : a.max_targets);
    if (c > (int64_t)a.max_targets && a.id_status && tid == 0 && ch == 0) atomicOr(a.id_status, 1 << 1);
    rp = a.rpart + ((int64_t)l * a.nchunk + ch) * SCORE_CATALOG_RPART;
    xfl = reinterpret_cast<int*>(sm + (CAND ? CT_SM_FLOATS_IN : CT_SM_FLOATS));
  }
  if constexpr (CAND) {
    const int64_t lo = a.cand_off[l], cnt64 = a.cand_off[l + 1] - lo;
    const int cnt = (int)(cnt64 < (int64_t)0x7FFFFF00 ? (cnt64 > 0 ? cnt64 : 0) : 0x7FFFFF00);
    cand = a.cand_idx + lo;
    cis = reinterpret_cast<int*>(sm + CT_SM_CI);
    c0_ = (int)min((int64_t)ch * a.chunk, (int64_t)cnt);
    c1_ = ch == a.nchunk - 1 ? cnt : (int)min((int64_t)c0_ + a.chunk, (int64_t)cnt);
    if (c1_ <= c0_) {                          // (workgroup-uniform, in front of the first barrier)
      if constexpr (RANKS) {                   // nothing counted; chunk 0 goes on, through the prologue alone (nstep = 0)
        if (ch != 0) {
          if (tid < SCORE_CATALOG_RPART) rp[tid] = 0;
          return;
        }
        c1_ = c0_;
      } else {
        ct_u64* out = a.part + ((int64_t)l * a.nchunk + ch) * k;
        if (tid < k) out[tid] = 0ull;
        return;
      }
    }
  } else {
    c0_ = ch * a.chunk; c1_ = min(N, c0_ + a.chunk);
  }
  const int c0 = c0_, c1 = c1_;
  const int nstep = (c1 - c0 + CT_ROWS - 1) / CT_ROWS;

  for (int e = tid; e < CT_N1; e += 64 * CT_NW) zl[e] = a.zline[(int64_t)l * CT_N1 + e];
  for (int e = tid; e < 2 * CT_ROWS * (CT_LD1 - CT_N1); e += 64 * CT_NW) {       // fc2's K padding, both buffers
    const int i = e / (CT_LD1 - CT_N1), c = e - i * (CT_LD1 - CT_N1);
    f1s[i * CT_LD1 + CT_N1 + c] = 0.f;
  }
  // the line's exclusions that fall into this chunk: [xa, xb) of excl_idx
  int64_t xa = 0, xb = 0;
  if (a.excl_off && (!RANKS || c1 > c0)) {     // (RANKS: chunk 0 of an empty list has no candidate to take a bound from)
    const int64_t lo = a.excl_off[l], hi = a.excl_off[l + 1];
    const uint32_t* ex = reinterpret_cast<const uint32_t*>(a.excl_idx) + lo;
    if constexpr (CAND) {            // between the range's first and last candidate, by value (each clamped into the catalogue)
      const int v0 = min(max(cand[c0], 0), N), v1 = min(max(cand[c1 - 1], -1), N - 1) + 1;
      xa = lo + dp_lower_bound(ex, hi - lo, (uint32_t)v0);
      xb = lo + dp_lower_bound(ex, hi - lo, (uint32_t)v1);
      if (xb < xa) xb = xa;
    } else {
      xa = lo + dp_lower_bound(ex, hi - lo, (uint32_t)c0);
      xb = lo + dp_lower_bound(ex, hi - lo, (uint32_t)c1);
    }
  }
  const int xn = (int)(xb - xa < (int64_t)0x7FFFFFFF ? xb - xa : 0x7FFFFFFF);
  const bool staged = xn <= CT_EXCL;
  if (staged)
    for (int e = tid; e < xn; e += 64 * CT_NW) exs[e] = (uint32_t)a.excl_idx[xa + e];

  // resident weights
  float bw[CT_KQ];
  float w3[CT_N2 / 4];
  float bias2 = 0.f, bias3 = 0.f;
  if (wave < CT_MW) {
    const int col = wave * 16 + lc;
#pragma unroll
    for (int s = 0; s < CT_KQ; ++s) {
      const int kk = lq * CT_KQ + s;
      const float w = a.W2[(int64_t)(kk < CT_N1 ? kk : CT_N1 - 1) * CT_N2 + col];        // clamped, unconditional
      bw[s] = kk < CT_N1 ? w : 0.f;
    }
    bias2 = a.b2[col];
  } else {
#pragma unroll
    for (int q = 0; q < CT_N2 / 4; ++q) w3[q] = a.W3[(lane & 3) + 4 * q];
    bias3 = a.b3[0];
  }

  // a step's zcat rows: CT_Q4 16-byte groups per matrix-wave thread; rows past the chunk's end read its last row
  float4 pre[CT_Q4];
  // (CAND: the row of the list position's catalogue index, from the step's LDS slot -- step 0's from the list itself)
  auto fetch = [&](int step, bool first) {
#pragma unroll
    for (int j = 0; j < CT_Q4; ++j) {
      const int e = tid + 64 * CT_MW * j;
      const int i = e / (CT_N1 / 4), c4 = e - i * (CT_N1 / 4);
      int n;
      if constexpr (CAND) {
        n = first ? cand[min(c0 + i, c1 - 1)] : cis[(step & (CT_CSLOTS - 1)) * CT_ROWS + i];
        n = (uint32_t)n < (uint32_t)N ? n : 0;
      } else {
        n = min(c0 + step * CT_ROWS + i, c1 - 1);
      }
      pre[j] = ld4(a.zcat + (int64_t)n * CT_N1 + c4 * 4);
    }
  };
  auto store = [&](int buf) {
    float* o = f1s + buf * (CT_ROWS * CT_LD1);
#pragma unroll
    for (int j = 0; j < CT_Q4; ++j) {
      const int e = tid + 64 * CT_MW * j;
      const int i = e / (CT_N1 / 4), c4 = e - i * (CT_N1 / 4);
      const float4 z = *reinterpret_cast<const float4*>(zl + c4 * 4);
      float4 v;
      v.x = fmaxf(pre[j].x + z.x, 0.f); v.y = fmaxf(pre[j].y + z.y, 0.f);
      v.z = fmaxf(pre[j].z + z.z, 0.f); v.w = fmaxf(pre[j].w + z.w, 0.f);
      *reinterpret_cast<float4*>(o + i * CT_LD1 + c4 * 4) = v;
    }
  };

  // RANKS, the prologue's rows: zcat[tgt_idx[tlo + i]], row 0 for a target outside the catalogue and behind the last target
  auto fetch_targets = [&]() {
#pragma unroll
    for (int j = 0; j < CT_Q4; ++j) {
      const int e = tid + 64 * CT_MW * j;
      const int i = e / (CT_N1 / 4), c4 = e - i * (CT_N1 / 4);
      int n = i < nt ? a.tgt_idx[tlo + i] : 0;
      n = (uint32_t)n < (uint32_t)N ? n : 0;
      pre[j] = ld4(a.zcat + (int64_t)n * CT_N1 + c4 * 4);
    }
  };

  ct_u64 e0 = 0ull, e1 = 0ull, thr = 0ull;       // the selection wave's list and its K-th key (0: fewer than K so far)
  const uint32_t* ex = staged ? exs : reinterpret_cast<const uint32_t*>(a.excl_idx) + xa;
  auto select = [&](const float* f2, int base, const int* ci) {
#pragma unroll
    for (int p = 0; p < CT_ROWS / 16; ++p) {
      const int i = lane >> 2, part = lane & 3;
      const float* row = f2 + (p * 16 + i) * CT_LD2 + part;
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < CT_N2 / 4; ++q) s = fmaf(row[4 * q], w3[q], s);
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      const float logit = s + bias3;
      int n = base + p * 16 + i;
      bool mine = part == 0 && n < c1;
      if constexpr (CAND) {          // n: a list position; the key takes its catalogue index, none outside the catalogue
        const int at = n;
        n = ci[p * 16 + i];
        const bool inside = (uint32_t)n < (uint32_t)N;
        if (mine && a.all_logits) a.all_logits[(cand - a.cand_idx) + at] = inside ? logit : __uint_as_float(0x7FC00000u);
        mine = mine && inside;
      } else {
        if (mine && a.all_logits) a.all_logits[(int64_t)l * N + n] = logit;
      }
      const ct_u64 key = mine ? ct_key(logit, n) : 0ull;
      ct_u64 m = __ballot(key > thr);
      while (m) {
        const int b = __ffsll((long long)m) - 1;
        m &= m - 1;
        const ct_u64 x = __shfl(key, b, 64);
        if (x <= thr) continue;                  // (the K-th rose since the ballot)
        const uint32_t idx = (uint32_t)ct_key_index(x);
        const int64_t pos = dp_lower_bound(ex, xn, idx);
        if (pos < xn && ex[pos] == idx) continue;
        ct_insert(e0, e1, x, lane);
        thr = ct_kth(e0, e1, k);
      }
    }
  };

  // RANKS.  Lane j < nt of the selection wave: target j's catalogue index, its key (all ones while unknown and for a target
  // outside the catalogue: nothing is ahead of it), the pairs ahead of it so far, its hit flags; every lane: the pairs counted
  int tn = -1, cnt = 0, hit = 0, nlive = 0, xc = 0;       // xc: the staged exclusions in front of the step (whole form)
  ct_u64 tkey = ~0ull;
  // the prologue's fc3: select's sum over the 32 target rows, row j's logit to lane j
  auto targets = [&](const float* f2) {
    float lg[CT_ROWS / 16];
#pragma unroll
    for (int p = 0; p < CT_ROWS / 16; ++p) {
      const int i = lane >> 2, part = lane & 3;
      const float* row = f2 + (p * 16 + i) * CT_LD2 + part;
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < CT_N2 / 4; ++q) s = fmaf(row[4 * q], w3[q], s);
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      lg[p] = s + bias3;
    }
    const float v0 = __shfl(lg[0], 4 * (lane & 15), 64), v1 = __shfl(lg[1], 4 * (lane & 15), 64);
    const float logit = (lane & 16) ? v1 : v0;
    const bool inside = lane < nt && (uint32_t)tn < (uint32_t)N;
    if (inside) tkey = ct_key(logit, tn);
    if (ch == 0 && lane < nt) a.tgt_logit[tlo + lane] = inside ? logit : __uint_as_float(0x7FC00000u);
  };
  auto count = [&](const float* f2, int base, const int* ci) {
    if constexpr (!CAND) {
      if (staged) {                // the step's rows [base, base + 32) that are excluded: exs[xc ..) up to the first index behind them
        if (lane < CT_ROWS) xfl[lane] = 0;
        for (;;) {
          const int e = xc + lane;
          const uint32_t v = e < xn ? exs[e] : 0xFFFFFFFFu;
          if ((uint32_t)(v - (uint32_t)base) < (uint32_t)CT_ROWS) xfl[v - (uint32_t)base] = 1;
          const ct_u64 m = __ballot(e < xn && v < (uint32_t)(base + CT_ROWS));
          xc += __popcll(m);
          if (m != ~0ull) break;                 // (64 in a row only where an index repeats)
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // one wave: the flags are read by other lanes than set them
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
    }
#pragma unroll
    for (int p = 0; p < CT_ROWS / 16; ++p) {
      const int i = lane >> 2, part = lane & 3;
      const float* row = f2 + (p * 16 + i) * CT_LD2 + part;
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < CT_N2 / 4; ++q) s = fmaf(row[4 * q], w3[q], s);
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      const float logit = s + bias3;
      int n = base + p * 16 + i;
      bool mine = part == 0 && n < c1;
      if constexpr (CAND) {
        n = ci[p * 16 + i];
        mine = mine && (uint32_t)n < (uint32_t)N;
      }
      bool out = false;            // the pair is in the line's exclusions
      if (mine) {
        if (!CAND && staged) {
          out = xfl[p * 16 + i] != 0;
        } else {
          const int64_t pos = dp_lower_bound(ex, xn, (uint32_t)n);
          out = pos < xn && ex[pos] == (uint32_t)n;
        }
      }
      const ct_u64 key = (mine && !out) ? ct_key(logit, n) : 0ull;
      nlive += __popcll(__ballot(mine && !out));
      for (int j = 0; j < nt; ++j) {
        const ct_u64 tk = __shfl(tkey, j, 64);
        const int tj = __shfl(tn, j, 64);
        const ct_u64 ahead = __ballot(key > tk);
        const ct_u64 met = __ballot(mine && n == tj), met_out = __ballot(mine && out && n == tj);
        if (lane == j) {
          cnt += __popcll(ahead);
          if (met) hit |= met_out ? 2 : 1;
        }
      }
    }
    if constexpr (!CAND) {
      if (staged) __builtin_amdgcn_wave_barrier();       // (the flags are cleared for the next step behind this step's reads)
    }
  };
  (void)targets; (void)count; (void)fetch_targets; (void)select;
  (void)cnt; (void)hit; (void)nlive; (void)xc; (void)tkey; (void)xfl; (void)rp;

  if constexpr (CAND) {            // the first two steps' indices (the selection wave: a lane each)
    if (wave == CT_MW) cis[lane] = (!RANKS || c1 > c0) ? cand[min(c0 + lane, c1 - 1)] : 0;
  }
  if constexpr (RANKS) {
    if (wave == CT_MW && lane < nt) tn = a.tgt_idx[tlo + lane];
    if (wave < CT_MW) fetch_targets();
  } else {
    if (wave < CT_MW) fetch(0, true);
  }
  __syncthreads();                 // zl, the padding and the exclusions are in LDS
  if (wave < CT_MW) store(RANKS ? 1 : 0);
  __syncthreads();
  for (int t = RANKS ? -1 : 0; t <= nstep; ++t) {
    if (wave < CT_MW) {
      if (t < nstep) {
        if (t + 1 < nstep) fetch(t + 1, false);
        hf_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        const float* x0 = f1s + (t & 1) * (CT_ROWS * CT_LD1) + lc * CT_LD1 + lq * CT_KQ;
        const float* x1 = x0 + 16 * CT_LD1;
#pragma unroll
        for (int s4 = 0; s4 < CT_KQ / 4; ++s4) {
          const float4 a0 = *reinterpret_cast<const float4*>(x0 + 4 * s4);
          const float4 a1 = *reinterpret_cast<const float4*>(x1 + 4 * s4);
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, bw[4 * s4 + 0], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, bw[4 * s4 + 0], acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, bw[4 * s4 + 1], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, bw[4 * s4 + 1], acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, bw[4 * s4 + 2], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, bw[4 * s4 + 2], acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, bw[4 * s4 + 3], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, bw[4 * s4 + 3], acc1, 0, 0, 0);
        }
        float* o = f2s + (t & 1) * (CT_ROWS * CT_LD2) + wave * 16 + lc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          o[(lq * 4 + r) * CT_LD2] = fmaxf(acc0[r] + bias2, 0.f);
          o[(16 + lq * 4 + r) * CT_LD2] = fmaxf(acc1[r] + bias2, 0.f);
        }
        if (t + 1 < nstep) store((t + 1) & 1);
      }
    } else if constexpr (CAND) {   // step t + 2's indices: requested in front of the selection, into their slot behind it
      int ahead = 0;
      const bool get = lane < CT_ROWS && t + 2 < nstep;
      if (get) ahead = cand[min(c0 + (t + 2) * CT_ROWS + lane, c1 - 1)];
      if constexpr (RANKS) {
        if (t >= 1)
          count(f2s + ((t - 1) & 1) * (CT_ROWS * CT_LD2), c0 + (t - 1) * CT_ROWS, cis + ((t - 1) & (CT_CSLOTS - 1)) * CT_ROWS);
        else if (t == 0)
          targets(f2s + CT_ROWS * CT_LD2);
      } else {
      if (t >= 1)
        select(f2s + ((t - 1) & 1) * (CT_ROWS * CT_LD2), c0 + (t - 1) * CT_ROWS, cis + ((t - 1) & (CT_CSLOTS - 1)) * CT_ROWS);
      }
      if (get) cis[((t + 2) & (CT_CSLOTS - 1)) * CT_ROWS + lane] = ahead;
    } else if constexpr (RANKS) {
      if (t >= 1)
        count(f2s + ((t - 1) & 1) * (CT_ROWS * CT_LD2), c0 + (t - 1) * CT_ROWS, nullptr);
      else if (t == 0)
        targets(f2s + CT_ROWS * CT_LD2);
    } else if (t >= 1) {
      select(f2s + ((t - 1) & 1) * (CT_ROWS * CT_LD2), c0 + (t - 1) * CT_ROWS, nullptr);
    }
    __syncthreads();
  }
  if constexpr (RANKS) {           // the chunk's partials: counts, flags, the pairs counted
    if (wave == CT_MW) {
      if (lane < CT_ROWS) { rp[lane] = cnt; rp[CT_ROWS + lane] = hit; }
      if (lane == 0) rp[2 * CT_ROWS] = nlive;
    }
  } else {
  if (wave == CT_MW) {             // the chunk's list, descending, empty slots (key 0) behind
    ct_u64* out = a.part + ((int64_t)l * a.nchunk + ch) * k;
    if (lane < k) out[lane] = e0;
    if (lane + 64 < k) out[lane + 64] = e1;
  }
  }
}

// The counting form's reduce, a wave per line: the chunks' partials added in chunk order (integers: any order gives the same),
// then per target ahead and state, per line n_scored.  A target outside [0, N): ahead -1, state -1; one behind the first
// max_targets of its line: the same, and NaN for its logit (chunk 0 wrote the others').
__global__ __launch_bounds__(64) void catalog_ranks_reduce_kernel(const CatalogArgs a) {
  const int lane = threadIdx.x, l = blockIdx.x;
  const int64_t tlo = a.tgt_off[l], c = a.tgt_off[l + 1] - tlo;
  const int nt = (int)(c < (int64_t)a.max_targets ? (c > 0 ? c : 0) : a.max_targets);
  const int32_t* p = a.rpart + (int64_t)l * a.nchunk * SCORE_CATALOG_RPART;
  int cnt = 0, hit = 0, live = 0;
  for (int ch = 0; ch < a.nchunk; ++ch) {
    const int32_t* q = p + (int64_t)ch * SCORE_CATALOG_RPART;
    if (lane < CT_ROWS) { cnt += q[lane]; hit |= q[CT_ROWS + lane]; }
    if (lane == 0) live += q[2 * CT_ROWS];
  }
  if (lane < nt) {
    const bool inside = (uint32_t)a.tgt_idx[tlo + lane] < (uint32_t)a.N;
    a.ahead[tlo + lane] = inside ? cnt : -1;
    a.state[tlo + lane] = !inside ? -1 : (hit & 2) ? 2 : (hit & 1);
  }
  for (int64_t e = nt + lane; e < c; e += 64) {
    a.ahead[tlo + e] = -1;
    a.state[tlo + e] = -1;
    a.tgt_logit[tlo + e] = __uint_as_float(0x7FC00000u);
  }
  if (lane == 0) a.n_scored[l] = live;
}

// One wave per line: the nchunk lists through the same insertion.  A list is descending, so behind the first 64 of its keys
// that all miss the current K-th nothing of it can enter.
__global__ __launch_bounds__(64) void catalog_merge_kernel(const CatalogArgs a) {
  const int lane = threadIdx.x, l = blockIdx.x, k = a.k;
  const ct_u64* p = a.part + (int64_t)l * a.nchunk * k;
  ct_u64 e0 = 0ull, e1 = 0ull, thr = 0ull;
  for (int ch = 0; ch < a.nchunk; ++ch) {
    for (int j0 = 0; j0 < k; j0 += 64) {
      const int j = j0 + lane;
      const ct_u64 key = p[(int64_t)ch * k + (j < k ? j : k - 1)];
      ct_u64 m = __ballot(j < k && key > thr);
      if (!m) break;
      while (m) {
        const int b = __ffsll((long long)m) - 1;
        m &= m - 1;
        const ct_u64 x = __shfl(key, b, 64);
        if (x <= thr) continue;
        ct_insert(e0, e1, x, lane);
        thr = ct_kth(e0, e1, k);
      }
    }
  }
  if (lane < k) {
    a.top_idx[(int64_t)l * k + lane] = ct_key_index(e0);
    a.top_logit[(int64_t)l * k + lane] = ct_key_logit(e0);
  }
  if (lane + 64 < k) {
    a.top_idx[(int64_t)l * k + lane + 64] = ct_key_index(e1);
    a.top_logit[(int64_t)l * k + lane + 64] = ct_key_logit(e1);
  }
}

}  // namespace

// The cut of a catalogue of N items into chunks for L lines (score_catalog_plan): ONE resident round -- at most 512 workgroups,
// two on each of the 256 compute units, so a line gets floor(512 / L) chunks -- and never fewer than 256 items a chunk, so that
// the 64 KB of fc2 a workgroup brings in are spread over eight steps at least.  A multiple of CT_ROWS.  Measured against targets
// of 512 (rounded up: 600 workgroups at 100 lines), 1024, 2048 and 4096 workgroups: DESIGN 7q.  k takes no part in the rule at
// present.
void score_catalog_chunks(int L, int N, int k, int* chunk, int* nchunk) {
  (void)k;
  const int64_t want = (L > 0 && L < 512) ? 512 / L : 1;
  int64_t c = align_up64(cdiv64(N > 0 ? N : 1, want), CT_ROWS);
  if (c < 256) c = 256;
  *chunk = (int)c;
  *nchunk = (int)cdiv64(N > 0 ? N : 1, c);
}

int score_catalog_zcat(const CatalogArgs& a, hipStream_t s) {
  if (a.N <= 0 || a.N1 != CT_N1 || a.Di <= 0 || a.D <= 0 || (a.D & 3) || a.Di % a.D || (a.off_ti & 3)) return SCORE_E_SHAPE;
  const size_t lds = catalog_zcat_lds(a.Di);
  if (lds > 150 * 1024) return SCORE_E_SHAPE;
  static thread_local bool attr_set = false;
  if (!attr_set && lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(catalog_zcat_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       150 * 1024);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  hipLaunchKernelGGL(catalog_zcat_kernel, dim3((unsigned)((a.N + HF_ROWS - 1) / HF_ROWS)), dim3(64 * HF_NW), lds, s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}


// Every sweep of the catalogue, in its four forms: CAND, the lines' candidate lists in the whole catalogue's place (the plan is
// that of a catalogue of a.max_count items, chunk / nchunk cut list positions, a.all_logits is cand_logits, aligned with cand_idx);
// RANKS, the counting form (score_catalog_ranks*) in the selecting one's place.  The form's checks, the cut against the span the
// plan was made for, the scoring kernel on a workgroup per (line, chunk), then a wave per line over the chunks' lists or partials.
namespace {
template <bool CAND, bool RANKS>
int catalog_sweep_launch(const CatalogArgs& a, hipStream_t s) {
  const int span = CAND ? a.max_count : a.N;
  if (a.L <= 0 || a.N <= 0 || a.N1 != CT_N1 || span <= 0) return SCORE_E_SHAPE;
  if (!RANKS && (a.k < 1 || a.k > SCORE_CATALOG_KMAX)) return SCORE_E_SHAPE;
  if (RANKS && (!a.tgt_off || !a.tgt_idx || !a.rpart || !a.ahead || !a.tgt_logit || !a.state || !a.n_scored)) return SCORE_E_BADARG;
  if (RANKS && (a.max_targets < 1 || a.max_targets > SCORE_CATALOG_TMAX)) return SCORE_E_BADARG;
  if (CAND && (!a.cand_off || !a.cand_idx)) return SCORE_E_BADARG;
  if (a.chunk <= 0 || a.chunk % CT_ROWS || (int64_t)a.nchunk * a.chunk < span || (int64_t)(a.nchunk - 1) * a.chunk >= span ||
      (int64_t)a.L * a.nchunk >= (1LL << 31))
    return SCORE_E_SHAPE;
  const size_t lds = (size_t)((CAND ? CT_SM_FLOATS_IN : CT_SM_FLOATS) + (RANKS ? CT_SM_RK : 0)) * sizeof(float);
  static thread_local bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(catalog_score_kernel<CAND, RANKS>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  hipLaunchKernelGGL((catalog_score_kernel<CAND, RANKS>), dim3((unsigned)(a.L * a.nchunk)), dim3(64 * CT_NW), lds, s, a);
  SCORE_CHECK_LAUNCH();
  if (RANKS) hipLaunchKernelGGL(catalog_ranks_reduce_kernel, dim3((unsigned)a.L), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(catalog_merge_kernel, dim3((unsigned)a.L), dim3(64), 0, s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}
}  // namespace

int score_catalog_sweep(const CatalogArgs& a, bool cand, bool ranks, hipStream_t s) {
  if (ranks) return cand ? catalog_sweep_launch<true, true>(a, s) : catalog_sweep_launch<false, true>(a, s);
  return cand ? catalog_sweep_launch<true, false>(a, s) : catalog_sweep_launch<false, false>(a, s);
}
