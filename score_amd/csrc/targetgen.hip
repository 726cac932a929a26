// The target lines every loader iterates over (gen_target.py:79-121; dataprep.gen_target_lines(draws="cell")), the popular-item
// list (gen_target.py:277-290) and sampling.py:31-37's 1-in-N down-sampling, on the device from the uploaded log.
//
// Draws: key(seed, tag, c, j) of cellkey.h with cell c = the line's user id.  tag 4: negative j without a pop list,
//   n_users + 1 + ((key * n_items) >> 32); tag 5: negative j from the pop list, pop[(key * n_pop) >> 32]; tag 6, j = 0: the
//   line stays iff (key * sample_factor) >> 32 == 0.  The products are 64-bit.
//
// score_target_build, count call:
//   keys     key = 0-based user of an event of slice pred_time, the sink n_users for every other event (and for an event whose
//            uid, iid or slice lies outside its range); value = its position in the log.  The same kernel marks the users with
//            an event in [start_time, pred_time): plain stores of the constant 1 into a zeroed array, so it does not matter
//            which store lands last.
//   sort     score_sort_pairs (sort.hip): stable, so the head of a user's run is its first event of the slice in log order.
//   flags    a head whose user is marked and passes the sample rule gets a line; the scan of the flags is its line index, and
//            the total goes back to the host (the call's one wait).
// fill call: a wave takes 64 sorted positions (a lane reads one flag), then the flagged ones in turn, the whole wave on one
//   line: word 0 the positive, word 1 + j negative j.  The words up to the first 16-byte boundary and behind the last go out
//   one per lane, those between four per lane.  A line of 1 + neg = 100 words is 400 bytes = 25 * 16, so every such line
//   starts on a boundary and takes the 16-byte stores alone; a width that is no multiple of 4 words (5, 7, 11, 101 in the
//   tests) puts line starts 0, 4, 8 and 12 bytes past one.
// score_target_build_lists (CCMR's user_neg_dict, gen_target.py:79-96): the same two calls with one more source per negative
//   word: negative j of user u is neg_items[neg_off[u - 1] + j] where j is below the user's list length, else the draw above at
//   the same j.  The fill kernel is the one above, compiled a second time with the list lookup in tg_word.
// Host waits: one per count call (the line count's read-back), none per fill; score_target_host_waits counts them.
// score_pop_items: per item the count of non-empty slices, a flag, the scan, a compaction in id order.
// No atomics, no workgroup waits on another: every array is a pure function of the input.
#include "common.h"
#include "cellkey.h"
#include "devprep.h"

namespace {

static_assert(SCAN_CHUNK == SCORE_TARGET_SCAN_TILE, "the header documents the scan's tile");
constexpr uint64_t TAG_NEG = 4, TAG_POP = 5, TAG_SAMPLE = 6;
constexpr int TG_MAX_PER_LINE = 4096;

__global__ __launch_bounds__(DP_THREADS) void tg_keys_kernel(const int32_t* __restrict__ uid, const int32_t* __restrict__ iid,
                                                            const int32_t* __restrict__ t_idx, int64_t n, int32_t U, int32_t I,
                                                            int32_t start_time, int32_t pred_time, uint32_t* __restrict__ keys,
                                                            uint32_t* __restrict__ vals, int32_t* __restrict__ hist) {
  DP_LOOP(i, n) {
    const int64_t u = (int64_t)uid[i] - 1, it = (int64_t)iid[i] - U - 1;
    const int32_t t = t_idx[i];
    const bool ok = u >= 0 && u < U && it >= 0 && it < I && t >= 0;
    keys[i] = (uint32_t)(ok && t == pred_time ? u : U);
    vals[i] = (uint32_t)i;
    if (ok && t >= start_time && t < pred_time) hist[u] = 1;
  }
}

// flag[p] = 1 where sorted position p is a head that gets a line, ev[p] = the log position of that event (else -1)
__global__ __launch_bounds__(DP_THREADS) void tg_flag_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                            const int32_t* __restrict__ hist, int64_t n, int32_t U,
                                                            int32_t sample_factor, uint64_t seed, int32_t* __restrict__ flag,
                                                            int32_t* __restrict__ ev) {
  DP_LOOP(p, n) {
    const uint32_t k = keys[p], v = vals[p];
    bool keep = k < (uint32_t)U && (p == 0 || keys[p - 1] != k) && (int64_t)v < n && hist[k] != 0;
    if (keep && sample_factor > 1)
      keep = (((uint64_t)gb_key(gb_cell_hash(seed, TAG_SAMPLE, (uint64_t)k + 1ull), 0) * (uint64_t)sample_factor) >> 32) == 0;
    flag[p] = keep ? 1 : 0;
    ev[p] = keep ? (int32_t)v : -1;
  }
}

struct Fill {
  const int32_t* uid; const int32_t* iid; const int32_t* ev; const int64_t* lidx; const int32_t* pop;
  const int64_t* noff; const int32_t* nitems;                      // the users' negative lists (score_target_build_lists)
  int32_t* line_user; int32_t* line_items;
  int64_t n, cap_lines, n_pop, n_neg;
  int32_t U, I, per;
  uint64_t seed;
};

// lbase / llen: where the user's list starts in nitems and how many of its entries the line takes (LISTS only)
template <bool LISTS>
__device__ __forceinline__ int32_t tg_word(const Fill& a, uint64_t h, int32_t pos, int32_t w, int64_t lbase, int32_t llen) {
  if (w == 0) return pos;
  if (LISTS && w - 1 < llen) return a.nitems[lbase + (w - 1)];
  const uint64_t k = gb_key(h, (uint64_t)(w - 1));
  return a.pop ? a.pop[(k * (uint64_t)a.n_pop) >> 32] : (int32_t)((int64_t)a.U + 1 + (int64_t)((k * (uint64_t)a.I) >> 32));
}

template <bool LISTS>
__global__ __launch_bounds__(DP_THREADS) void tg_fill_kernel(Fill a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * DP_THREADS + threadIdx.x) >> 6, nwaves = (int64_t)gridDim.x * (DP_THREADS / 64);
  for (int64_t base = wave * 64; base < a.n; base += nwaves * 64) {
    const int64_t p = base + lane;
    uint64_t live = __ballot(p < a.n && a.ev[p] >= 0);
    while (live) {                                                  // (wave-uniform)
      const int src = __ffsll((unsigned long long)live) - 1;
      live &= live - 1;
      const int64_t v = a.ev[base + src], l = a.lidx[base + src];
      if (v < 0 || v >= a.n || l < 0 || l >= a.cap_lines) continue;
      const int32_t u = a.uid[v], pos = a.iid[v];
      if (u < 1 || u > a.U) continue;                               // (never with the count call's own ev)
      const uint64_t h = gb_cell_hash(a.seed, a.pop ? TAG_POP : TAG_NEG, (uint64_t)u);
      int64_t lbase = 0;
      int32_t llen = 0;
      if (LISTS) {
        const int64_t b = a.noff[u - 1], e = a.noff[u];
        if (b >= 0 && e >= b && e <= a.n_neg) { lbase = b; llen = (int32_t)(e - b < (int64_t)a.per ? e - b : (int64_t)a.per); }
      }
      int32_t* row = a.line_items + l * a.per;
      if (lane == 0) a.line_user[l] = u;
      int32_t head = (int32_t)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) >> 2);
      head = head < a.per ? head : a.per;
      const int32_t nvec = (a.per - head) >> 2, tail = head + 4 * nvec;
      const auto word = [&](int32_t w) { return tg_word<LISTS>(a, h, pos, w, lbase, llen); };
      if (lane < head) row[lane] = word(lane);
      for (int32_t c = lane; c < nvec; c += 64) {
        const int32_t w = head + 4 * c;
        int4 x;
        x.x = word(w); x.y = word(w + 1); x.z = word(w + 2); x.w = word(w + 3);
        *reinterpret_cast<int4*>(row + w) = x;
      }
      if (tail + lane < a.per) row[tail + lane] = word(tail + lane);                    // (fewer than 4 words)
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- pop items
__global__ __launch_bounds__(DP_THREADS) void tg_pop_flag_kernel(const int64_t* __restrict__ off1, int32_t U, int32_t I, int32_t S,
                                                                int32_t pop_standard, int32_t max_iid, int32_t* __restrict__ flag) {
  DP_LOOP(i, I) {
    const int64_t* o = off1 + i * S;
    int32_t cnt = 0;
    int64_t prev = o[0];
    for (int32_t t = 1; t <= S; ++t) {
      const int64_t next = o[t];
      cnt += next > prev ? 1 : 0;
      prev = next;
    }
    flag[i] = (cnt >= pop_standard && (int64_t)U + 1 + i <= (int64_t)max_iid) ? 1 : 0;
  }
}

__global__ __launch_bounds__(DP_THREADS) void tg_pop_fill_kernel(const int32_t* __restrict__ flag, const int64_t* __restrict__ idx,
                                                                int32_t U, int32_t I, int32_t* __restrict__ pop, int64_t cap) {
  DP_LOOP(i, I) {
    if (!flag[i]) continue;
    const int64_t q = idx[i];
    if (q >= 0 && q < cap) pop[q] = (int32_t)((int64_t)U + 1 + i);
  }
}

// ------------------------------------------------------------------------------------------------------------------ host
struct Temp { SortBufs sort; int32_t* flag; int32_t* ev; int32_t* hist; int64_t* lidx; int64_t* bsum; int64_t total_bytes; };

Temp carve(void* temp, int64_t n, int64_t U) {
  Temp t;
  Carver c(temp);
  c.sort_pairs(t.sort, n);
  t.flag = c.words<int32_t>(n);
  t.ev = c.words<int32_t>(n);
  t.hist = c.words<int32_t>(U);
  t.lidx = c.prefix(n);
  t.bsum = c.block_sums(n);
  c.sort_temp(t.sort, n);
  t.total_bytes = c.off;
  return t;
}

struct PopTemp { int32_t* flag; int64_t* idx; int64_t* bsum; int64_t total_bytes; };

PopTemp pop_carve(void* temp, int64_t I) {
  PopTemp t;
  Carver c(temp);
  c.scan(t.flag, t.idx, t.bsum, I);
  t.total_bytes = c.off;
  return t;
}

std::atomic<int> g_host_waits{0};      // every wait for a stream in this file is a dp_read_words that counts here

}  // namespace

extern "C" int64_t score_target_build_temp_bytes(int64_t n_events, int32_t n_users) {
  if (n_events <= 0 || n_events >= (1ll << 31) || n_users <= 0) return -1;
  return carve(nullptr, n_events, n_users).total_bytes;
}

namespace {

// both entry points: noff == nullptr is score_target_build
int tg_build(const score_target_build_t* a, const int64_t* noff, const int32_t* nitems, int64_t n_neg, int32_t* line_user,
             int32_t* line_items, int64_t cap_lines, int64_t* n_lines, void* temp, int64_t temp_bytes, void* stream) {
  if (!a || a->struct_bytes != (int64_t)sizeof(score_target_build_t)) return SCORE_E_BADARG;
  if (!a->uid || !a->iid || !a->t_idx || !temp) return SCORE_E_BADARG;
  if (a->n_events <= 0 || a->n_users <= 0 || a->n_items <= 0 || a->neg_sample_num < 0 || a->sample_factor < 0 || a->n_pop < 0)
    return SCORE_E_BADARG;
  if (line_user ? (!line_items || cap_lines <= 0 || (a->pop_items && a->n_pop <= 0)) : !n_lines) return SCORE_E_BADARG;
  const int64_t lim = 1ll << 31;
  if (a->n_events >= lim || (int64_t)a->n_users + a->n_items >= lim || a->n_pop >= lim ||
      (int64_t)a->neg_sample_num + 1 > TG_MAX_PER_LINE)
    return SCORE_E_SHAPE;
  if (score_target_build_temp_bytes(a->n_events, a->n_users) > temp_bytes) return SCORE_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = a->n_events;
  const int32_t U = a->n_users;
  const Temp t = carve(temp, n, U);
  if (line_user) {
    Fill f;
    f.uid = a->uid; f.iid = a->iid; f.ev = t.ev; f.lidx = t.lidx; f.pop = a->pop_items;
    f.noff = noff; f.nitems = nitems; f.n_neg = n_neg;
    f.line_user = line_user; f.line_items = line_items;
    f.n = n; f.cap_lines = cap_lines; f.n_pop = a->n_pop;
    f.U = U; f.I = a->n_items; f.per = 1 + a->neg_sample_num;
    f.seed = a->seed;
    const int64_t groups = cdiv64(cdiv64(n, 64), DP_THREADS / 64);
    const dim3 grid((unsigned)(groups < 8192 ? groups : 8192));
    if (noff) hipLaunchKernelGGL(tg_fill_kernel<true>, grid, dim3(DP_THREADS), 0, s, f);
    else hipLaunchKernelGGL(tg_fill_kernel<false>, grid, dim3(DP_THREADS), 0, s, f);
    SCORE_CHECK_LAUNCH();
    return 0;
  }
  SortBufs b = t.sort;
  hipLaunchKernelGGL(dp_zero_kernel<int32_t>, dim3(dp_grid(U)), dim3(DP_THREADS), 0, s, t.hist, (int64_t)U);
  SCORE_CHECK_LAUNCH();
  hipLaunchKernelGGL(tg_keys_kernel, dim3(dp_grid(n)), dim3(DP_THREADS), 0, s, a->uid, a->iid, a->t_idx, n, U, a->n_items,
                     a->start_time, a->pred_time, b.k0, b.v0, t.hist);
  SCORE_CHECK_LAUNCH();
  SCORE_TRY(dp_sort(b, n, dp_bits_of((uint32_t)U), s));
  hipLaunchKernelGGL(tg_flag_kernel, dim3(dp_grid(n)), dim3(DP_THREADS), 0, s, b.k0, b.v0, t.hist, n, U, a->sample_factor, a->seed,
                     t.flag, t.ev);
  SCORE_CHECK_LAUNCH();
  SCORE_TRY(gb_scan(t.flag, n, t.bsum, t.lidx, s));
  return dp_read_words(t.lidx + n, n_lines, 1, s, &g_host_waits);
}

}  // namespace

extern "C" int score_target_host_waits(void) { return g_host_waits.load(std::memory_order_relaxed); }

extern "C" int score_target_build(const score_target_build_t* a, int32_t* line_user, int32_t* line_items, int64_t cap_lines,
                                  int64_t* n_lines, void* temp, int64_t temp_bytes, void* stream) {
  return tg_build(a, nullptr, nullptr, 0, line_user, line_items, cap_lines, n_lines, temp, temp_bytes, stream);
}

extern "C" int score_target_build_lists(const score_target_lists_t* a, int32_t* line_user, int32_t* line_items,
                                        int64_t cap_lines, int64_t* n_lines, void* temp, int64_t temp_bytes, void* stream) {
  if (!a || a->struct_bytes != (int64_t)sizeof(score_target_lists_t)) return SCORE_E_BADARG;
  if (!a->neg_off || a->n_neg < 0 || (a->n_neg > 0 && !a->neg_items)) return SCORE_E_BADARG;
  if (a->n_neg >= (1ll << 31)) return SCORE_E_SHAPE;
  return tg_build(&a->build, a->neg_off, a->neg_items, a->n_neg, line_user, line_items, cap_lines, n_lines, temp, temp_bytes,
                  stream);
}

extern "C" int64_t score_pop_items_temp_bytes(int32_t n_items) {
  if (n_items <= 0) return -1;
  return pop_carve(nullptr, n_items).total_bytes;
}

extern "C" int score_pop_items(const score_pop_items_t* a, int32_t* pop_items, int64_t cap_pop, int64_t* n_pop, void* temp,
                               int64_t temp_bytes, void* stream) {
  if (!a || a->struct_bytes != (int64_t)sizeof(score_pop_items_t)) return SCORE_E_BADARG;
  if (!a->item_off1 || !temp || a->n_users <= 0 || a->n_items <= 0 || a->time_slice_num <= 0) return SCORE_E_BADARG;
  if (pop_items ? cap_pop <= 0 : !n_pop) return SCORE_E_BADARG;
  const int64_t lim = 1ll << 31;
  if ((int64_t)a->n_items * a->time_slice_num >= lim || (int64_t)a->n_users + a->n_items >= lim) return SCORE_E_SHAPE;
  if (score_pop_items_temp_bytes(a->n_items) > temp_bytes) return SCORE_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t I = a->n_items;
  const PopTemp t = pop_carve(temp, I);
  if (pop_items) {
    hipLaunchKernelGGL(tg_pop_fill_kernel, dim3(dp_grid(I)), dim3(DP_THREADS), 0, s, t.flag, t.idx, a->n_users, a->n_items,
                       pop_items, cap_pop);
    SCORE_CHECK_LAUNCH();
    return 0;
  }
  hipLaunchKernelGGL(tg_pop_flag_kernel, dim3(dp_grid(I)), dim3(DP_THREADS), 0, s, a->item_off1, a->n_users, a->n_items,
                     a->time_slice_num, a->pop_standard, a->max_iid, t.flag);
  SCORE_CHECK_LAUNCH();
  SCORE_TRY(gb_scan(t.flag, I, t.bsum, t.idx, s));
  return dp_read_words(t.idx + I, n_pop, 1, s, &g_host_waits);
}
