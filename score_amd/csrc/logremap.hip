// The first link of the data path on the device: a raw behaviour log -> remapped ids, feature rows, time slices
// (feateng_tmall.py:30-133, feateng_taobao.py:16-88; dataprep.remap_tmall_log / remap_taobao_log(build="device")).
//
// score_log_remap: n_cols raw int32 columns, each one vocabulary, numbered one behind the other from 1 in column order and
//   inside a column in order of first appearance (dataprep._first_appearance).  Per column, count call:
//   keys     key = the value's 32-bit pattern (raw columns hold negatives; only the grouping matters), value = log position.
//            A pattern with a bit above key_bits sets the status word (a plain store of the constant 1) and is masked, so
//            the sort never sees it.
//   sort     score_sort_pairs: stable, so a run's head holds the value's first log position and its tail the last.
//   mark     head[p] in sorted order and is_first[vals[p]] = head[p] in log order: vals is a permutation, so every word of
//            is_first gets exactly one plain store and nothing has to be zeroed first.
//   rank     gb_scan over is_first: rank[first_pos]; its total is the vocabulary size.  A one-thread kernel adds it to the
//            running base (a device word: no host wait between columns) and notes it for the read-back.
//   runs     gb_scan over head: the run index of a sorted position; heads store run_first[run], tails run_last[run].
//   write    ids[pos] = base + rank[run_first[run]]; for a table's entity column the head also stores
//            ent_last[id - base] = run_last[run], which is what the fill call reads.
//   The call's one wait is the read-back of the n_cols counts and the status word.
// fill call: one thread per row e of a table: [id_e, id_f1[last], ...] with last = ent_last[e], in 16-byte stores where the
//   row is a multiple of four words on a 16-byte boundary.  No host wait, nothing at or past the cap.
// score_log_slices: element-wise, the Tmall 15-day slices from MMDD (floor division) or the epoch filter and slices.
// score_log_compact: keep flags -> gb_scan -> stable scatter of up to 8 columns and the kept positions.
// No atomics, no workgroup waits on another: every array is a pure function of the input.
#include "common.h"
#include "devprep.h"

namespace {

constexpr int LR_MAX_COLS = SCORE_LOG_REMAP_MAX_COLS, LR_MAX_TABLES = SCORE_LOG_REMAP_MAX_TABLES;
constexpr int LR_RES_WORDS = 32;              // int64: base[0 .. 8], counts at 9 .. 16, status at 17

__global__ void lr_init_kernel(int64_t* __restrict__ res) {
  if (threadIdx.x < LR_RES_WORDS) res[threadIdx.x] = threadIdx.x == 0 ? 1 : 0;      // base[0] = 1: 0 is the dummy node
}

__global__ __launch_bounds__(DP_THREADS) void lr_keys_kernel(const int32_t* __restrict__ col, int64_t n, int32_t key_bits,
                                                            uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                            int64_t* __restrict__ status) {
  const uint32_t mask = key_bits >= 32 ? 0xFFFFFFFFu : ((1u << key_bits) - 1u);
  DP_LOOP(i, n) {
    const uint32_t k = (uint32_t)col[i];
    if (k & ~mask) *status = 1;
    keys[i] = k & mask;
    vals[i] = (uint32_t)i;
  }
}

__global__ __launch_bounds__(DP_THREADS) void lr_mark_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                            int64_t n, int32_t* __restrict__ head, int32_t* __restrict__ is_first) {
  DP_LOOP(p, n) {
    const int32_t h = (p == 0 || keys[p - 1] != keys[p]) ? 1 : 0;
    const uint32_t v = vals[p];
    head[p] = h;
    if ((int64_t)v < n) is_first[v] = h;
  }
}

__global__ void lr_base_kernel(int64_t* __restrict__ res, const int64_t* __restrict__ total, int32_t c) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    res[1 + LR_MAX_COLS + c] = *total;
    res[c + 1] = res[c] + *total;
  }
}

__global__ __launch_bounds__(DP_THREADS) void lr_runs_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                            const int32_t* __restrict__ head, const int64_t* __restrict__ run,
                                                            int64_t n, int32_t* __restrict__ run_first,
                                                            int32_t* __restrict__ run_last) {
  DP_LOOP(p, n) {
    const int64_t r = run[p] + head[p] - 1;
    if (r < 0 || r >= n) continue;                                  // (never with this call's own scan)
    if (head[p]) run_first[r] = (int32_t)vals[p];
    if (p == n - 1 || keys[p + 1] != keys[p]) run_last[r] = (int32_t)vals[p];
  }
}

__global__ __launch_bounds__(DP_THREADS) void lr_write_kernel(const uint32_t* __restrict__ vals, const int32_t* __restrict__ head,
                                                             const int64_t* __restrict__ run, const int64_t* __restrict__ rank,
                                                             const int32_t* __restrict__ run_first,
                                                             const int32_t* __restrict__ run_last, const int64_t* __restrict__ base,
                                                             int64_t n, int32_t* __restrict__ ids, int32_t* __restrict__ ent_last0,
                                                             int32_t* __restrict__ ent_last1) {
  const int64_t b = *base;
  DP_LOOP(p, n) {
    const int64_t r = run[p] + head[p] - 1;
    const uint32_t v = vals[p];
    if (r < 0 || r >= n || (int64_t)v >= n) continue;
    const int64_t f = run_first[r];
    if (f < 0 || f >= n) continue;
    const int64_t e = rank[f];
    ids[v] = (int32_t)(b + e);
    if (head[p] && e >= 0 && e < n) {
      if (ent_last0) ent_last0[e] = run_last[r];
      if (ent_last1) ent_last1[e] = run_last[r];
    }
  }
}

struct RowFill {
  const int32_t* id[1 + SCORE_LOG_REMAP_MAX_FEATS];      // the entity's id column, then the feature columns' id columns
  const int32_t* ent_last; const int64_t* count;
  int32_t* rows;
  int64_t n, cap;
  int32_t width;
};

__global__ __launch_bounds__(DP_THREADS) void lr_rows_kernel(RowFill a) {
  int64_t m = *a.count;
  m = m < a.cap ? m : a.cap;
  const bool vec = (a.width & 3) == 0 && (reinterpret_cast<uintptr_t>(a.rows) & 15u) == 0;
  DP_LOOP(e, m) {
    const int64_t last = a.ent_last[e];
    if (last < 0 || last >= a.n) continue;
    int32_t w[1 + SCORE_LOG_REMAP_MAX_FEATS];
#pragma unroll
    for (int j = 0; j < 1 + SCORE_LOG_REMAP_MAX_FEATS; ++j) w[j] = j < a.width ? a.id[j][last] : 0;
    int32_t* row = a.rows + e * a.width;
    if (vec) {
      *reinterpret_cast<int4*>(row) = make_int4(w[0], w[1], w[2], w[3]);
      if (a.width == 8) *reinterpret_cast<int4*>(row + 4) = make_int4(w[4], w[5], w[6], w[7]);
    } else {
#pragma unroll
      for (int j = 0; j < 1 + SCORE_LOG_REMAP_MAX_FEATS; ++j)
        if (j < a.width) row[j] = w[j];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- slices
__global__ __launch_bounds__(DP_THREADS) void lr_slices_tmall_kernel(const int32_t* __restrict__ mmdd, int64_t n,
                                                                    int32_t* __restrict__ t_idx, int32_t* __restrict__ status) {
  DP_LOOP(i, n) {
    const int32_t v = mmdd[i];
    const int32_t m = v / 100, d = v - m * 100;
    // days before the month's first in 2015 (no leap day), and the month's length
    const int32_t before = m == 1 ? 0 : m == 2 ? 31 : m == 3 ? 59 : m == 4 ? 90 : m == 5 ? 120 : m == 6 ? 151 : m == 7 ? 181 :
                           m == 8 ? 212 : m == 9 ? 243 : m == 10 ? 273 : m == 11 ? 304 : 334;
    const int32_t len = m == 2 ? 28 : (m == 4 || m == 6 || m == 9 || m == 11) ? 30 : 31;
    if (v < 0 || m < 1 || m > 12 || d < 1 || d > len) {
      *status = 1;
      t_idx[i] = 0;
      continue;
    }
    const int32_t diff = before + d - 121;                          // days since 2015-05-01 (its day of the year is 121)
    int32_t q = diff / 15;
    if (diff - q * 15 < 0) --q;                                     // floor, as Python's //
    t_idx[i] = q;
  }
}

__global__ __launch_bounds__(DP_THREADS) void lr_slices_epoch_kernel(const int32_t* __restrict__ ts, const int32_t* __restrict__ flag,
                                                                    int64_t n, int32_t start_ts, int32_t end_ts, int32_t delta,
                                                                    int32_t* __restrict__ t_idx, int32_t* __restrict__ keep) {
  DP_LOOP(i, n) {
    const int32_t t = ts[i];
    const bool k = t >= start_ts && t <= end_ts && (!flag || flag[i] != 0);
    keep[i] = k ? 1 : 0;
    t_idx[i] = k ? (int32_t)(((int64_t)t - start_ts) / delta) : -1;
  }
}

// --------------------------------------------------------------------------------------------------------------- compact
struct Compact {
  const int32_t* in[LR_MAX_COLS]; int32_t* out[LR_MAX_COLS];
  const int32_t* flag; const int64_t* idx; int32_t* kept_pos;
  int64_t n, cap;
  int32_t n_cols;
};

__global__ __launch_bounds__(DP_THREADS) void lr_flag_kernel(const int32_t* __restrict__ keep, int64_t n, int32_t* __restrict__ flag) {
  DP_LOOP(i, n) flag[i] = keep[i] != 0 ? 1 : 0;
}

__global__ __launch_bounds__(DP_THREADS) void lr_compact_kernel(Compact a) {
  DP_LOOP(i, a.n) {
    if (!a.flag[i]) continue;
    const int64_t q = a.idx[i];
    if (q < 0 || q >= a.cap) continue;
#pragma unroll
    for (int c = 0; c < LR_MAX_COLS; ++c)
      if (c < a.n_cols) a.out[c][q] = a.in[c][i];
    if (a.kept_pos) a.kept_pos[q] = (int32_t)i;
  }
}

// ------------------------------------------------------------------------------------------------------------------ host
struct Temp {
  int64_t* res; SortBufs sort;
  int32_t* head; int32_t* is_first; int32_t* run_first; int32_t* run_last; int32_t* ent_last[LR_MAX_TABLES];
  int64_t* rank; int64_t* run; int64_t* bsum; int64_t total_bytes;
};

Temp carve(void* temp, int64_t n) {
  Temp t;
  Carver c(temp);
  t.res = c.take<int64_t>(LR_RES_WORDS, 1);
  c.sort_pairs(t.sort, n);
  t.head = c.words<int32_t>(n);
  t.is_first = c.words<int32_t>(n);
  t.run_first = c.words<int32_t>(n);
  t.run_last = c.words<int32_t>(n);
  for (int i = 0; i < LR_MAX_TABLES; ++i) t.ent_last[i] = c.words<int32_t>(n);
  t.rank = c.prefix(n);
  t.run = c.prefix(n);
  t.bsum = c.block_sums(n);
  c.sort_temp(t.sort, n);
  t.total_bytes = c.off;
  return t;
}

struct CompactTemp { int32_t* flag; int64_t* idx; int64_t* bsum; int64_t total_bytes; };

CompactTemp compact_carve(void* temp, int64_t n) {
  CompactTemp t;
  Carver c(temp);
  c.scan(t.flag, t.idx, t.bsum, n);
  t.total_bytes = c.off;
  return t;
}

std::atomic<int> g_host_waits{0};      // every wait for a stream in this file is a dp_read_words that counts here

}  // namespace

extern "C" int score_log_host_waits(void) { return g_host_waits.load(std::memory_order_relaxed); }

extern "C" int64_t score_log_remap_temp_bytes(int64_t n_events, int32_t n_cols) {
  if (n_events <= 0 || n_events >= (1ll << 31) || n_cols < 1 || n_cols > LR_MAX_COLS) return -1;
  return carve(nullptr, n_events).total_bytes;
}

extern "C" int score_log_remap(const score_log_remap_t* a, int32_t* const* rows, const int64_t* cap_rows, int64_t* counts,
                               void* temp, int64_t temp_bytes, void* stream) {
  if (!a || a->struct_bytes != (int64_t)sizeof(score_log_remap_t)) return SCORE_E_BADARG;
  if (!temp || a->n_events <= 0 || a->n_cols < 1 || a->n_cols > LR_MAX_COLS || a->key_bits < 1 || a->key_bits > 32 ||
      a->n_tables < 0 || a->n_tables > LR_MAX_TABLES)
    return SCORE_E_BADARG;
  for (int c = 0; c < a->n_cols; ++c)
    if (!a->cols[c] || !a->ids[c]) return SCORE_E_BADARG;
  for (int t = 0; t < a->n_tables; ++t) {
    const score_log_table_t& tb = a->tables[t];
    if (tb.entity < 0 || tb.entity >= a->n_cols || tb.n_feat < 0 || tb.n_feat > SCORE_LOG_REMAP_MAX_FEATS) return SCORE_E_BADARG;
    for (int j = 0; j < tb.n_feat; ++j)
      if (tb.feat[j] < 0 || tb.feat[j] >= a->n_cols) return SCORE_E_BADARG;
  }
  if (rows) {
    if (!cap_rows || a->n_tables < 1) return SCORE_E_BADARG;
    for (int t = 0; t < a->n_tables; ++t)
      if (!rows[t] || cap_rows[t] <= 0) return SCORE_E_BADARG;
  } else if (!counts) {
    return SCORE_E_BADARG;
  }
  if (a->n_events >= (1ll << 31)) return SCORE_E_SHAPE;
  if (score_log_remap_temp_bytes(a->n_events, a->n_cols) > temp_bytes) return SCORE_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = a->n_events;
  const Temp t = carve(temp, n);
  if (rows) {
    for (int k = 0; k < a->n_tables; ++k) {
      const score_log_table_t& tb = a->tables[k];
      RowFill f;
      for (int j = 0; j < 1 + SCORE_LOG_REMAP_MAX_FEATS; ++j) f.id[j] = a->ids[tb.entity];
      for (int j = 0; j < tb.n_feat; ++j) f.id[1 + j] = a->ids[tb.feat[j]];
      f.ent_last = t.ent_last[k]; f.count = t.res + 1 + LR_MAX_COLS + tb.entity;
      f.rows = rows[k];
      f.n = n; f.cap = cap_rows[k];
      f.width = 1 + tb.n_feat;
      hipLaunchKernelGGL(lr_rows_kernel, dim3(dp_grid(f.cap < n ? f.cap : n)), dim3(DP_THREADS), 0, s, f);
      SCORE_CHECK_LAUNCH();
    }
    return 0;
  }
  hipLaunchKernelGGL(lr_init_kernel, dim3(1), dim3(64), 0, s, t.res);
  SCORE_CHECK_LAUNCH();
  int64_t* status = t.res + 1 + 2 * LR_MAX_COLS;
  for (int c = 0; c < a->n_cols; ++c) {
    SortBufs b = t.sort;
    int32_t* el[LR_MAX_TABLES] = {nullptr, nullptr};
    for (int j = 0; j < a->n_tables; ++j)
      if (a->tables[j].entity == c) el[j] = t.ent_last[j];
    hipLaunchKernelGGL(lr_keys_kernel, dim3(dp_grid(n)), dim3(DP_THREADS), 0, s, a->cols[c], n, a->key_bits, b.k0, b.v0, status);
    SCORE_CHECK_LAUNCH();
    SCORE_TRY(dp_sort(b, n, a->key_bits, s));
    hipLaunchKernelGGL(lr_mark_kernel, dim3(dp_grid(n)), dim3(DP_THREADS), 0, s, b.k0, b.v0, n, t.head, t.is_first);
    SCORE_CHECK_LAUNCH();
    SCORE_TRY(gb_scan(t.is_first, n, t.bsum, t.rank, s));
    hipLaunchKernelGGL(lr_base_kernel, dim3(1), dim3(64), 0, s, t.res, t.rank + n, c);
    SCORE_CHECK_LAUNCH();
    SCORE_TRY(gb_scan(t.head, n, t.bsum, t.run, s));
    hipLaunchKernelGGL(lr_runs_kernel, dim3(dp_grid(n)), dim3(DP_THREADS), 0, s, b.k0, b.v0, t.head, t.run, n, t.run_first,
                       t.run_last);
    SCORE_CHECK_LAUNCH();
    hipLaunchKernelGGL(lr_write_kernel, dim3(dp_grid(n)), dim3(DP_THREADS), 0, s, b.v0, t.head, t.run, t.rank, t.run_first,
                       t.run_last, t.res + c, n, a->ids[c], el[0], el[1]);
    SCORE_CHECK_LAUNCH();
  }
  int64_t host[1 + LR_MAX_COLS];                                     // the counts and the status word behind them: one wait
  SCORE_TRY(dp_read_words(t.res + 1 + LR_MAX_COLS, host, 1 + LR_MAX_COLS, s, &g_host_waits));
  if (host[LR_MAX_COLS] != 0) return SCORE_E_BADARG;                 // a value wider than key_bits
  int64_t sum = 0;
  for (int c = 0; c < a->n_cols; ++c) sum += host[c];
  if (sum + 1 >= (1ll << 31)) return SCORE_E_SHAPE;
  for (int c = 0; c < a->n_cols; ++c) counts[c] = host[c];
  return 0;
}

extern "C" int score_log_slices(int32_t mode, const int32_t* time, const int32_t* flag, int64_t n_events, int32_t start_ts,
                                int32_t end_ts, int32_t delta, int32_t* t_idx, int32_t* keep, int32_t* status, void* stream) {
  if (!time || !t_idx || n_events <= 0) return SCORE_E_BADARG;
  if (n_events >= (1ll << 31)) return SCORE_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  if (mode == SCORE_LOG_SLICES_TMALL) {
    if (!status) return SCORE_E_BADARG;
    hipLaunchKernelGGL(lr_slices_tmall_kernel, dim3(dp_grid(n_events)), dim3(DP_THREADS), 0, s, time, n_events, t_idx, status);
  } else if (mode == SCORE_LOG_SLICES_EPOCH) {
    if (!keep || delta <= 0 || end_ts < start_ts) return SCORE_E_BADARG;
    hipLaunchKernelGGL(lr_slices_epoch_kernel, dim3(dp_grid(n_events)), dim3(DP_THREADS), 0, s, time, flag, n_events, start_ts,
                       end_ts, delta, t_idx, keep);
  } else {
    return SCORE_E_BADARG;
  }
  SCORE_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t score_log_compact_temp_bytes(int64_t n_events) {
  if (n_events <= 0 || n_events >= (1ll << 31)) return -1;
  return compact_carve(nullptr, n_events).total_bytes;
}

extern "C" int score_log_compact(const int32_t* const* cols_in, int32_t* const* cols_out, int32_t n_cols, const int32_t* keep,
                                 int64_t n_events, int32_t* kept_pos, int64_t cap, int64_t* n_kept, void* temp,
                                 int64_t temp_bytes, void* stream) {
  if (!cols_in || !cols_out || !keep || !n_kept || !temp || n_events <= 0 || n_cols < 1 || n_cols > LR_MAX_COLS || cap <= 0)
    return SCORE_E_BADARG;
  for (int c = 0; c < n_cols; ++c)
    if (!cols_in[c] || !cols_out[c]) return SCORE_E_BADARG;
  if (n_events >= (1ll << 31)) return SCORE_E_SHAPE;
  if (score_log_compact_temp_bytes(n_events) > temp_bytes) return SCORE_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = n_events;
  const CompactTemp t = compact_carve(temp, n);
  hipLaunchKernelGGL(lr_flag_kernel, dim3(dp_grid(n)), dim3(DP_THREADS), 0, s, keep, n, t.flag);
  SCORE_CHECK_LAUNCH();
  SCORE_TRY(gb_scan(t.flag, n, t.bsum, t.idx, s));
  int64_t total = 0;
  SCORE_TRY(dp_read_words(t.idx + n, &total, 1, s, &g_host_waits));
  *n_kept = total;
  if (total == 0) return 0;
  Compact k;
  for (int c = 0; c < LR_MAX_COLS; ++c) { k.in[c] = cols_in[c < n_cols ? c : 0]; k.out[c] = cols_out[c < n_cols ? c : 0]; }
  k.flag = t.flag; k.idx = t.idx; k.kept_pos = kept_pos;
  k.n = n; k.cap = cap; k.n_cols = n_cols;
  hipLaunchKernelGGL(lr_compact_kernel, dim3(dp_grid(n)), dim3(DP_THREADS), 0, s, k);
  SCORE_CHECK_LAUNCH();
  return 0;
}
