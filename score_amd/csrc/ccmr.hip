// CCMR's first offline step on the device (feateng_ccmr.py:24-44,119-183; dataprep.remap_ccmr_log(build="device")) and the
// per-user lists of negatively rated items (user_neg_dict, :173-183; targets.UserNegLists.from_events(build="device")).
//
// score_ccmr_prep, one call, no host wait:
//   events   one thread per event: the date YYYYMMDD is checked against the civil calendar (leap years by the Gregorian rule,
//            years 1 .. 9999 as datetime.date takes them) and turned into its day number (date.toordinal()) by integer
//            arithmetic alone; slice = (day - start_day) / delta_days truncated TOWARDS ZERO (C++'s integer division, Python's
//            int() at :125); uid = raw + 1, iid = raw + 1 + n_users; keep_pos = rating is 4 or 5, keep_neg = any other rating.
//            A bad date or id stores the constant 1 into its status word and the event joins neither half.  A positive
//            event marks its item in a zeroed array (plain stores of one constant).
//   movies   key = raw item of a movie_info line (the sink n_items where it lies outside, with a status word), value = the
//            line's position; a feature outside its vocabulary sets a status word.  A stable score_sort_pairs: the head of an
//            item's run is its FIRST line (:167).
//   rows     one thread per item: a binary search for its run; row = [iid, did, aid, gid, nid] of the head line, a present
//            feature f of field k at 1 + f + n_users + n_items + sum(vocab[:k]), an empty one (-1) at the field's last id.  An
//            item without a line gets the four "none" ids; where such an item is marked the thread flags it, and the scan's
//            total of those flags is status word SCORE_CCMR_ST_MISSING.
// score_neg_lists_build, no host wait: a stable score_sort_pairs on (uid - 1, log position) over the negative events (a uid
//   outside 1 .. n_users behind the sink n_users), items gathered in that order (zero behind the last list), off[u] = the lower
//   bound of key u by binary search, u = 0 .. n_users.
// Host waits: none in this file.  remap_ccmr_log(build="device") waits three times in all: one download (the row table with the
// status words in front of it) and the two compactions of score_log_compact (score_log_host_waits counts those).
// No atomics, no workgroup waits on another: every array is a pure function of the input.
#include "common.h"
#include "devprep.h"

namespace {

// YYYYMMDD -> date.toordinal() (0001-01-01 is day 1), or -1 for what datetime.date refuses
__device__ __forceinline__ int32_t cc_ordinal(int32_t v) {
  if (v <= 0) return -1;
  int32_t y = v / 10000;
  const int32_t m = (v / 100) % 100, d = v % 100;
  if (y < 1 || y > 9999 || m < 1 || m > 12 || d < 1) return -1;
  const bool leap = (y % 4 == 0 && y % 100 != 0) || y % 400 == 0;
  const int32_t len = m == 2 ? (leap ? 29 : 28) : (m == 4 || m == 6 || m == 9 || m == 11) ? 30 : 31;
  if (d > len) return -1;
  y -= m <= 2 ? 1 : 0;                                              // the year starts with March: the leap day comes last
  const int32_t era = y / 400, yoe = y - era * 400;
  const int32_t doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
  const int32_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + doe - 305;                                  // (0000-03-01 is day -305 of this count)
}

struct Prep {
  const int32_t* user; const int32_t* item; const int32_t* rating; const int32_t* date;
  int32_t* uid; int32_t* iid; int32_t* t_idx; int32_t* day; int32_t* keep_pos; int32_t* keep_neg;
  int32_t* occurs; int32_t* status;
  int64_t n;
  int32_t U, I, start_day, delta_days;
};

__global__ __launch_bounds__(DP_THREADS) void cc_events_kernel(Prep a) {
  DP_LOOP(i, a.n) {
    const int32_t u = a.user[i], it = a.item[i], r = a.rating[i];
    const int32_t day = cc_ordinal(a.date[i]);
    const bool ok_u = u >= 0 && u < a.U, ok_i = it >= 0 && it < a.I, ok = ok_u && ok_i && day >= 0;
    if (day < 0) a.status[SCORE_CCMR_ST_DATE] = 1;
    if (!ok_u) a.status[SCORE_CCMR_ST_USER] = 1;
    if (!ok_i) a.status[SCORE_CCMR_ST_ITEM] = 1;
    const bool pos = ok && (r == 4 || r == 5);
    a.uid[i] = ok ? u + 1 : 0;
    a.iid[i] = ok ? it + 1 + a.U : 0;
    a.t_idx[i] = ok ? (day - a.start_day) / a.delta_days : -1;      // (towards zero)
    a.day[i] = ok ? day : 0;
    a.keep_pos[i] = pos ? 1 : 0;
    a.keep_neg[i] = ok && !pos ? 1 : 0;
    if (pos) a.occurs[it] = 1;
  }
}

struct Movies {
  const int32_t* col[5];
  int64_t m;
  int32_t U, I, vocab[4];
};

__global__ __launch_bounds__(DP_THREADS) void cc_movie_keys_kernel(Movies a, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                                  int32_t* __restrict__ status) {
  DP_LOOP(j, a.m) {
    const int32_t it = a.col[0][j];
    const bool ok = it >= 0 && it < a.I;
    if (!ok) status[SCORE_CCMR_ST_MOVIE_ITEM] = 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int32_t f = a.col[1 + k][j];
      if (f < -1 || f >= a.vocab[k] - 1) status[SCORE_CCMR_ST_FEATURE] = 1;       // (the last id of a field is its "none")
    }
    keys[j] = (uint32_t)(ok ? it : a.I);
    vals[j] = (uint32_t)j;
  }
}

__global__ __launch_bounds__(DP_THREADS) void cc_rows_kernel(Movies a, const uint32_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ vals, const int32_t* __restrict__ occurs,
                                                            int32_t* __restrict__ rows, int32_t* __restrict__ miss) {
  DP_LOOP(i, a.I) {
    const int64_t p = dp_lower_bound(keys, a.m, (uint32_t)i);
    int64_t line = -1;
    if (p < a.m && keys[p] == (uint32_t)i && (int64_t)vals[p] < a.m) line = vals[p];
    int64_t base = (int64_t)a.U + a.I;                              // the ids of field k are base + 1 .. base + vocab[k]
    int32_t* row = rows + i * 5;
    row[0] = (int32_t)(a.U + 1 + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int32_t f = line >= 0 ? a.col[1 + k][line] : -1;
      row[1 + k] = (int32_t)((f >= 0 && f < a.vocab[k] - 1) ? base + 1 + f : base + a.vocab[k]);
      base += a.vocab[k];
    }
    miss[i] = (line < 0 && occurs[i] != 0) ? 1 : 0;
  }
}

__global__ void cc_total_kernel(const int64_t* __restrict__ total, int32_t* __restrict__ status) {
  if (threadIdx.x == 0 && blockIdx.x == 0) status[SCORE_CCMR_ST_MISSING] = (int32_t)(*total < 0x7FFFFFFF ? *total : 0x7FFFFFFF);
}

// ------------------------------------------------------------------------------------------------------------- neg lists
__global__ __launch_bounds__(DP_THREADS) void cc_neg_keys_kernel(const int32_t* __restrict__ uid, int64_t n, int32_t U,
                                                                uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  DP_LOOP(i, n) {
    const int64_t u = (int64_t)uid[i] - 1;
    keys[i] = (uint32_t)(u >= 0 && u < U ? u : U);
    vals[i] = (uint32_t)i;
  }
}

__global__ __launch_bounds__(DP_THREADS) void cc_neg_lists_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                                 const int32_t* __restrict__ iid, int64_t n, int32_t U,
                                                                 int64_t* __restrict__ off, int32_t* __restrict__ items) {
  const int64_t total = n > (int64_t)U + 1 ? n : (int64_t)U + 1;
  DP_LOOP(i, total) {
    if (i < n) {
      const uint32_t k = keys[i], v = vals[i];
      items[i] = (k < (uint32_t)U && (int64_t)v < n) ? iid[v] : 0;
    }
    if (i <= U) off[i] = dp_lower_bound(keys, n, (uint32_t)i);
  }
}

// ------------------------------------------------------------------------------------------------------------------ host
struct PrepTemp { SortBufs sort; int32_t* occurs; int32_t* miss; int64_t* midx; int64_t* bsum; int64_t total_bytes; };

PrepTemp prep_carve(void* temp, int64_t m, int64_t I) {
  PrepTemp t;
  Carver c(temp);
  c.sort_pairs(t.sort, m > 0 ? m : 1);
  t.occurs = c.words<int32_t>(I);
  c.scan(t.miss, t.midx, t.bsum, I);
  c.sort_temp(t.sort, m);
  t.total_bytes = c.off;
  return t;
}

struct NegTemp { SortBufs sort; int64_t total_bytes; };

NegTemp neg_carve(void* temp, int64_t n) {
  NegTemp t;
  Carver c(temp);
  c.sort_pairs(t.sort, n > 0 ? n : 1);
  c.sort_temp(t.sort, n);
  t.total_bytes = c.off;
  return t;
}

}  // namespace

extern "C" int64_t score_ccmr_prep_temp_bytes(int64_t n_movies, int32_t n_items) {
  if (n_movies < 0 || n_movies >= (1ll << 31) || n_items <= 0) return -1;
  return prep_carve(nullptr, n_movies, n_items).total_bytes;
}

extern "C" int score_ccmr_prep(const score_ccmr_prep_t* a, void* temp, int64_t temp_bytes, void* stream) {
  if (!a || a->struct_bytes != (int64_t)sizeof(score_ccmr_prep_t)) return SCORE_E_BADARG;
  if (!temp || !a->user || !a->item || !a->rating || !a->date || !a->uid || !a->iid || !a->t_idx || !a->day || !a->keep_pos ||
      !a->keep_neg || !a->item_rows || !a->status)
    return SCORE_E_BADARG;
  if (a->n_events <= 0 || a->n_movies < 0 || a->n_users <= 0 || a->n_items <= 0 || a->delta_days <= 0 || a->start_day < 1)
    return SCORE_E_BADARG;
  int64_t size = 1 + (int64_t)a->n_users + a->n_items;
  for (int k = 0; k < 4; ++k) {
    if (a->vocab[k] < 1) return SCORE_E_BADARG;
    size += a->vocab[k];
  }
  for (int k = 0; k < 5; ++k)
    if (a->n_movies > 0 && !a->movie[k]) return SCORE_E_BADARG;
  const int64_t lim = 1ll << 31;
  if (a->n_events >= lim || a->n_movies >= lim || size >= lim) return SCORE_E_SHAPE;
  if (score_ccmr_prep_temp_bytes(a->n_movies, a->n_items) > temp_bytes) return SCORE_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = a->n_events, m = a->n_movies, I = a->n_items;
  const PrepTemp t = prep_carve(temp, m, I);
  hipLaunchKernelGGL(dp_zero_kernel<int32_t>, dim3(1), dim3(DP_THREADS), 0, s, a->status, (int64_t)SCORE_CCMR_STATUS_WORDS);
  SCORE_CHECK_LAUNCH();
  hipLaunchKernelGGL(dp_zero_kernel<int32_t>, dim3(dp_grid(I)), dim3(DP_THREADS), 0, s, t.occurs, I);
  SCORE_CHECK_LAUNCH();
  Prep e;
  e.user = a->user; e.item = a->item; e.rating = a->rating; e.date = a->date;
  e.uid = a->uid; e.iid = a->iid; e.t_idx = a->t_idx; e.day = a->day; e.keep_pos = a->keep_pos; e.keep_neg = a->keep_neg;
  e.occurs = t.occurs; e.status = a->status;
  e.n = n;
  e.U = a->n_users; e.I = a->n_items; e.start_day = a->start_day; e.delta_days = a->delta_days;
  hipLaunchKernelGGL(cc_events_kernel, dim3(dp_grid(n)), dim3(DP_THREADS), 0, s, e);
  SCORE_CHECK_LAUNCH();
  Movies mv;
  for (int k = 0; k < 5; ++k) mv.col[k] = a->movie[k];
  mv.m = m;
  mv.U = a->n_users; mv.I = a->n_items;
  for (int k = 0; k < 4; ++k) mv.vocab[k] = a->vocab[k];
  SortBufs b = t.sort;
  if (m > 0) {
    hipLaunchKernelGGL(cc_movie_keys_kernel, dim3(dp_grid(m)), dim3(DP_THREADS), 0, s, mv, b.k0, b.v0, a->status);
    SCORE_CHECK_LAUNCH();
    SCORE_TRY(dp_sort(b, m, dp_bits_of((uint32_t)I), s));
  }
  hipLaunchKernelGGL(cc_rows_kernel, dim3(dp_grid(I)), dim3(DP_THREADS), 0, s, mv, b.k0, b.v0, t.occurs, a->item_rows, t.miss);
  SCORE_CHECK_LAUNCH();
  SCORE_TRY(gb_scan(t.miss, I, t.bsum, t.midx, s));
  hipLaunchKernelGGL(cc_total_kernel, dim3(1), dim3(64), 0, s, t.midx + I, a->status);
  SCORE_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t score_neg_lists_temp_bytes(int64_t n_neg) {
  if (n_neg < 0 || n_neg >= (1ll << 31)) return -1;
  return neg_carve(nullptr, n_neg).total_bytes;
}

extern "C" int score_neg_lists_build(const int32_t* neg_uid, const int32_t* neg_iid, int64_t n_neg, int32_t n_users, int64_t* off,
                                     int32_t* items, void* temp, int64_t temp_bytes, void* stream) {
  if (!off || !temp || n_neg < 0 || n_users <= 0 || (n_neg > 0 && (!neg_uid || !neg_iid || !items))) return SCORE_E_BADARG;
  if (n_neg >= (1ll << 31) || n_users == 0x7FFFFFFF) return SCORE_E_SHAPE;
  if (score_neg_lists_temp_bytes(n_neg) > temp_bytes) return SCORE_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const NegTemp t = neg_carve(temp, n_neg);
  SortBufs b = t.sort;
  if (n_neg > 0) {
    hipLaunchKernelGGL(cc_neg_keys_kernel, dim3(dp_grid(n_neg)), dim3(DP_THREADS), 0, s, neg_uid, n_neg, n_users, b.k0, b.v0);
    SCORE_CHECK_LAUNCH();
    SCORE_TRY(dp_sort(b, n_neg, dp_bits_of((uint32_t)n_users), s));
  }
  const int64_t total = n_neg > (int64_t)n_users + 1 ? n_neg : (int64_t)n_users + 1;
  hipLaunchKernelGGL(cc_neg_lists_kernel, dim3(dp_grid(total)), dim3(DP_THREADS), 0, s, b.k0, b.v0, neg_iid, n_neg, n_users, off,
                     items);
  SCORE_CHECK_LAUNCH();
  return 0;
}
