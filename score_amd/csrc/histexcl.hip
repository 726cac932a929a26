// History exclusions as the catalogue's scoring kernels take them (score_catalog_lines_t.excl_*), straight from a
// PointLogStore's user histories: score_catalog_history_exclusions (include/score_hip.h).  Line l's list is the set of catalogue
// indices j whose id cat_ids[j] occurs anywhere in user user_ids[l]'s whole segment of user_hist_seq, without keep_ids[l]:
// strictly ascending, no repeats, exact offsets -- what harness._history_exclusions + ItemCatalog.exclusions build with two dozen
// torch launches, a global sort and a host wait.
//
// A bitmap per (line, range of HX_RANGE catalogue indices) in LDS: a workgroup walks the user's segment HX_THREADS entries a
// stride -- any length --, finds each id in its range of the sorted id column by binary search and ORs the index's bit in; the
// list is then read off the bitmap in index order.  The OR is the only atomic, and its order cannot show: a bit is set or not.
// Three steps, no workgroup waits on another, no host wait:
//   count   bitmap -> its popcount                                   counts[l * n_ranges + r]
//   scan    devprep's reduce-then-scan over the L * n_ranges counts  prefix (int64)
//   fill    the bitmap again -> the set bits' indices at prefix[l * n_ranges + r] + their rank, by a popcount prefix over the
//           bitmap's words; excl_off[l] = prefix[l * n_ranges]
// The bitmap is built twice instead of being kept: L * N / 8 bytes of workspace (12.5 MB at 100 lines of 10^6 items) would cost
// more than the second walk of histories a few thousand events long.  What bounds it: a history costs n_ranges walks of it (a
// range whose id span the entry misses costs two comparisons), so time grows with events * N / 32768 per line; nothing is
// assumed to fit -- a segment of any length and a catalogue of any N < 2^31 take more strides and more ranges.
#include "common.h"
#include "devprep.h"

#define HX_THREADS 256

namespace {

constexpr int HX_WORDS = 1024;                     // a workgroup's bitmap: 4 KiB of LDS
constexpr int HX_RANGE = 32 * HX_WORDS;            // catalogue indices a workgroup covers
constexpr int HX_PER = HX_WORDS / HX_THREADS;      // consecutive bitmap words a thread reads off
static_assert(HX_PER * HX_THREADS == HX_WORDS, "the bitmap's words split evenly over the threads");

struct HistExcl {
  const int64_t* off; const int32_t* seq; int64_t n_users;
  const int32_t* user_ids; const int32_t* keep_ids; const int32_t* cat_ids;
  int32_t L, N, n_ranges;
  int32_t* counts; const int64_t* prefix;
  int64_t* excl_off; int32_t* excl_idx; int64_t capacity; int32_t* status;
};

// first position of the ascending (signed) ids that is >= c
__device__ __forceinline__ int hx_lower_bound(const int32_t* __restrict__ ids, int n, int32_t c) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (ids[mid] < c) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// bits[0 .. HX_WORDS) <- the catalogue indices c0 + b of line l's list that fall into range r (bit b & 31 of word b >> 5);
// returns with the bitmap complete for every thread
__device__ __forceinline__ void hx_bitmap(uint32_t* bits, const HistExcl& a, int l, int r) {
  const int tid = (int)threadIdx.x;
  for (int w = tid; w < HX_WORDS; w += HX_THREADS) bits[w] = 0u;
  __syncthreads();
  const int64_t u = (int64_t)a.user_ids[l] - 1;
  if (u >= 0 && u < a.n_users) {                   // (workgroup-uniform)
    const int c0 = r * HX_RANGE;
    const int cn = a.N - c0 < HX_RANGE ? a.N - c0 : HX_RANGE;
    const int32_t* ids = a.cat_ids + c0;
    const int32_t first = ids[0], last = ids[cn - 1];
    const bool has_keep = a.keep_ids != nullptr;
    const int32_t keep = has_keep ? a.keep_ids[l] : 0;
    const int64_t b = a.off[u], e = a.off[u + 1];
    for (int64_t i = b + tid; i < e; i += HX_THREADS) {
      const int32_t id = a.seq[i];
      if (id < first || id > last || (has_keep && id == keep)) continue;
      const int pos = hx_lower_bound(ids, cn, id);
      if (pos < cn && ids[pos] == id) atomicOr(&bits[pos >> 5], 1u << (pos & 31));
    }
  }
  __syncthreads();
}

// workgroup blockIdx.x = l * n_ranges + r
__global__ __launch_bounds__(HX_THREADS) void hist_excl_count_kernel(const HistExcl a) {
  __shared__ uint32_t bits[HX_WORDS];
  __shared__ int64_t sc[HX_THREADS];
  const int tid = (int)threadIdx.x;
  const int l = (int)blockIdx.x / a.n_ranges, r = (int)blockIdx.x - l * a.n_ranges;
  hx_bitmap(bits, a, l, r);
  int64_t c = 0;
#pragma unroll
  for (int j = 0; j < HX_PER; ++j) c += __popc(bits[tid * HX_PER + j]);
  const int64_t incl = gb_block_incl_scan<HX_THREADS>(c, sc, tid);
  if (tid == HX_THREADS - 1) a.counts[blockIdx.x] = (int32_t)incl;
}

__global__ __launch_bounds__(HX_THREADS) void hist_excl_fill_kernel(const HistExcl a) {
  __shared__ uint32_t bits[HX_WORDS];
  __shared__ int64_t sc[HX_THREADS];
  const int tid = (int)threadIdx.x;
  const int l = (int)blockIdx.x / a.n_ranges, r = (int)blockIdx.x - l * a.n_ranges;
  hx_bitmap(bits, a, l, r);
  uint32_t w[HX_PER];
  int64_t c = 0;
#pragma unroll
  for (int j = 0; j < HX_PER; ++j) {
    w[j] = bits[tid * HX_PER + j];
    c += __popc(w[j]);
  }
  int64_t at = a.prefix[blockIdx.x] + gb_block_incl_scan<HX_THREADS>(c, sc, tid) - c;
  const int base = r * HX_RANGE + tid * HX_PER * 32;
#pragma unroll
  for (int j = 0; j < HX_PER; ++j) {
    uint32_t m = w[j];
    while (m) {
      const int b = __ffs((int)m) - 1;
      m &= m - 1;
      if (at < a.capacity) a.excl_idx[at] = base + j * 32 + b;
      ++at;
    }
  }
  if (r == 0 && tid == 0) {
    a.excl_off[l] = a.prefix[blockIdx.x];
    if (l == 0) {                                  // (one thread of the grid: the total and the overflow report)
      const int64_t total = a.prefix[(int64_t)a.L * a.n_ranges];
      a.excl_off[a.L] = total;
      if (total > a.capacity) *a.status = *a.status | 1;
    }
  }
}

struct Temp { int32_t* counts; int64_t* prefix; int64_t* bsum; int64_t total_bytes; };

Temp excl_carve(void* temp, int64_t n) {
  Temp t;
  Carver c(temp);
  c.scan(t.counts, t.prefix, t.bsum, n);
  t.total_bytes = c.off;
  return t;
}

}  // namespace

extern "C" int score_catalog_history_exclusions_plan(int32_t L, int32_t N, int64_t max_events, int32_t* range, int32_t* n_ranges,
                                                     int32_t* threads, int64_t* temp_bytes) {
  if (L <= 0 || N <= 0 || max_events < 0) return SCORE_E_BADARG;
  const int64_t nr = cdiv64(N, HX_RANGE);
  if ((int64_t)L * nr >= ((int64_t)1 << 31)) return SCORE_E_SHAPE;
  if (range) *range = HX_RANGE;
  if (n_ranges) *n_ranges = (int32_t)nr;
  if (threads) *threads = HX_THREADS;
  if (temp_bytes) *temp_bytes = excl_carve(nullptr, (int64_t)L * nr).total_bytes;
  return 0;
}

extern "C" int score_catalog_history_exclusions(const score_point_log_store_t* st, const int32_t* user_ids, const int32_t* keep_ids,
                                                int32_t L, const int32_t* cat_ids, int32_t N, int64_t* excl_off, int32_t* excl_idx,
                                                int64_t capacity, int32_t* status, void* temp, int64_t temp_bytes, void* stream) {
  if (!st || !user_ids || !cat_ids || !excl_off || !excl_idx || !status || !temp) return SCORE_E_BADARG;
  if (st->struct_bytes != (int64_t)sizeof(score_point_log_store_t)) return SCORE_E_BADARG;
  if (L <= 0 || N <= 0 || capacity < 0) return SCORE_E_BADARG;
  if (!st->user_hist_off || !st->user_hist_seq || st->n_users <= 0) return SCORE_E_BADARG;
  int32_t nr = 0;
  int64_t need = 0;
  SCORE_TRY(score_catalog_history_exclusions_plan(L, N, 0, nullptr, &nr, nullptr, &need));
  if (temp_bytes < need) return SCORE_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = (int64_t)L * nr;
  const Temp t = excl_carve(temp, n);
  HistExcl a;
  a.off = st->user_hist_off; a.seq = st->user_hist_seq; a.n_users = st->n_users;
  a.user_ids = user_ids; a.keep_ids = keep_ids; a.cat_ids = cat_ids;
  a.L = L; a.N = N; a.n_ranges = nr;
  a.counts = t.counts; a.prefix = t.prefix;
  a.excl_off = excl_off; a.excl_idx = excl_idx; a.capacity = capacity; a.status = status;
  hipLaunchKernelGGL(hist_excl_count_kernel, dim3((unsigned)n), dim3(HX_THREADS), 0, s, a);
  SCORE_CHECK_LAUNCH();
  SCORE_TRY(gb_scan(t.counts, n, t.bsum, t.prefix, s));
  hipLaunchKernelGGL(hist_excl_fill_kernel, dim3((unsigned)n), dim3(HX_THREADS), 0, s, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}
