// Per-entity histories of the point baselines straight from the remapped interaction log: what the reference builds with
// gen_target.py:223-275 (gen_user_item_hist_dict_*: a dict of (other id, time) lists per entity, each sorted by time with
// Python's STABLE sorted) and trims in gen_history_point.py:22-65 (the last MAX_LEN ids), as one CSR per side in HBM.
//   events outside [start_time, pred_time) are dropped (:241-244);
//   a history is ordered by (time_key, position in the log): equal times keep log order (:257-259);
//   the kept history is its last hist_max_len ids (gen_history_point.py:31-32, 54-55).
// One call builds one side (users: ent = uid, other = iid; items: the roles exchanged) in three steps on `stream`:
//   fill     key = (entity << time_bits) | time_key, value = the event's position; events outside the window, or of an entity
//            outside [id_lo, id_lo + n_ent), get the key of a sink behind every entity;
//   sort     score_sort_pairs (sort.hip): a stable LSD sort, so equal keys stay in log order.  ONE sort where
//            bits(n_ent) + time_bits <= 32 (Tmall: 19 + 11 users, 21 + 11 items), else TWO: by time_key, then -- the keys
//            rewritten from the sorted positions -- by entity;
//   segments one kernel: a binary search per entity over the sorted keys gives off[e]; len[e] = min(count, hist_max_len);
//            seq[p] = other[value[p]] for every sorted position of the window.
// So seq holds the WHOLE window in (entity, time, log) order -- bounded by the log, not by samples --, entity e's history is
// seq[off[e] .. off[e + 1]) and its kept history the last len[e] ids of that.  Nothing here is atomic: the three arrays are a
// pure function of the input.
// Limits on n: the sort's, n < 2^31 (positions and destinations are 32-bit words; a tile's per-wave counters hold 1,024 at
// most whatever n).  The 54 M rows of the full Tmall log are 6,592 tiles: 864 MB of keys and values in two copies and 108 MB
// of histogram matrix in `temp`.
#include "common.h"
#include "devprep.h"

namespace {

struct HistFill {
  const int32_t* ent; const int32_t* time_key; const int32_t* t_idx;
  int64_t n;
  int32_t start_time, pred_time, id_lo, n_ent, time_bits;
};

// the entity of event i as 0 .. n_ent - 1, or n_ent (the sink)
__device__ __forceinline__ uint32_t ph_entity(const HistFill& a, int64_t i) {
  const int32_t t = a.t_idx[i];
  const int64_t e = (int64_t)a.ent[i] - a.id_lo;
  return (t >= a.start_time && t < a.pred_time && e >= 0 && e < a.n_ent) ? (uint32_t)e : (uint32_t)a.n_ent;
}

// mode 0: keys[i] = (entity << time_bits) | time_key, vals[i] = i      (the one-sort form)
// mode 1: keys[i] = time_key, vals[i] = i                               (first of two sorts)
// mode 2: keys[p] = entity of event vals[p]                             (second of two sorts: vals is sorted by time)
__global__ __launch_bounds__(DP_THREADS) void point_hist_fill_kernel(HistFill a, int mode, uint32_t* __restrict__ keys,
                                                                     uint32_t* __restrict__ vals) {
  const uint32_t tmask = a.time_bits >= 32 ? 0xFFFFFFFFu : ((1u << a.time_bits) - 1u);
  DP_LOOP(i, a.n) {
    if (mode == 2) {
      const uint32_t v = vals[i];
      keys[i] = (int64_t)v < a.n ? ph_entity(a, v) : (uint32_t)a.n_ent;
    } else {
      const uint32_t tk = (uint32_t)a.time_key[i] & tmask;
      const uint32_t e = ph_entity(a, i);
      keys[i] = mode == 1 ? tk : (e == (uint32_t)a.n_ent ? e << a.time_bits : (e << a.time_bits) | tk);
      vals[i] = (uint32_t)i;
    }
  }
}

__global__ __launch_bounds__(DP_THREADS) void point_hist_segments_kernel(const uint32_t* __restrict__ keys,
                                                                         const uint32_t* __restrict__ vals,
                                                                         const int32_t* __restrict__ other, int64_t n, int shift,
                                                                         int32_t n_ent, int32_t hist_max_len,
                                                                         int64_t* __restrict__ off, int32_t* __restrict__ seq,
                                                                         int32_t* __restrict__ len) {
  const int64_t total = n > (int64_t)n_ent + 1 ? n : (int64_t)n_ent + 1;
  DP_LOOP(i, total) {
    if (i < n) {
      const uint32_t v = vals[i];
      seq[i] = ((keys[i] >> shift) < (uint32_t)n_ent && (int64_t)v < n) ? other[v] : 0;
    }
    if (i <= n_ent) {
      const int64_t b = dp_lower_bound(keys, n, shift, (uint32_t)i);
      off[i] = b;
      if (i < n_ent) {
        const int64_t c = dp_lower_bound(keys, n, shift, (uint32_t)i + 1u) - b;
        len[i] = (int32_t)(c < hist_max_len ? c : hist_max_len);
      }
    }
  }
}

struct Temp { SortBufs sort; int64_t total_bytes; };

Temp carve(void* temp, int64_t n) {
  Temp t;
  Carver c(temp);
  c.sort_pairs(t.sort, n);
  c.sort_temp(t.sort, n);
  t.total_bytes = c.off;
  return t;
}

}  // namespace

extern "C" int64_t score_point_hist_temp_bytes(int64_t n_events) {
  if (n_events <= 0 || n_events >= (1ll << 31)) return -1;
  return carve(nullptr, n_events).total_bytes;
}

extern "C" int score_point_hist_build(const int32_t* ent, const int32_t* other, const int32_t* time_key, const int32_t* t_idx,
                                      int64_t n_events, int32_t start_time, int32_t pred_time, int32_t id_lo, int32_t n_ent,
                                      int32_t time_bits, int32_t hist_max_len, int64_t* off, int32_t* seq, int32_t* len,
                                      void* temp, int64_t temp_bytes, void* stream) {
  if (!ent || !other || !time_key || !t_idx || !off || !seq || !len || !temp) return SCORE_E_BADARG;
  if (n_events <= 0 || n_ent <= 0 || hist_max_len <= 0 || time_bits < 1 || time_bits > 31) return SCORE_E_BADARG;
  if (n_events >= (1ll << 31) || n_ent == 0x7FFFFFFF) return SCORE_E_SHAPE;
  if (score_point_hist_temp_bytes(n_events) > temp_bytes) return SCORE_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  SortBufs b = carve(temp, n_events).sort;
  HistFill a;
  a.ent = ent; a.time_key = time_key; a.t_idx = t_idx; a.n = n_events;
  a.start_time = start_time; a.pred_time = pred_time; a.id_lo = id_lo; a.n_ent = n_ent; a.time_bits = time_bits;
  const int ebits = dp_bits_of((uint32_t)n_ent);                  // (the sink is entity n_ent)
  const bool one_sort = ebits + time_bits <= 32;
  const unsigned grid = dp_grid(n_events);
  hipLaunchKernelGGL(point_hist_fill_kernel, dim3(grid), dim3(DP_THREADS), 0, s, a, one_sort ? 0 : 1, b.k0, b.v0);
  SCORE_CHECK_LAUNCH();
  SCORE_TRY(dp_sort(b, n_events, one_sort ? ebits + time_bits : time_bits, s));
  if (!one_sort) {
    hipLaunchKernelGGL(point_hist_fill_kernel, dim3(grid), dim3(DP_THREADS), 0, s, a, 2, b.k0, b.v0);
    SCORE_CHECK_LAUNCH();
    SCORE_TRY(dp_sort(b, n_events, ebits, s));
  }
  const int64_t total = n_events > (int64_t)n_ent + 1 ? n_events : (int64_t)n_ent + 1;
  hipLaunchKernelGGL(point_hist_segments_kernel, dim3(dp_grid(total)), dim3(DP_THREADS), 0, s, b.k0, b.v0, other, n_events,
                     one_sort ? time_bits : 0, n_ent, hist_max_len, off, seq, len);
  SCORE_CHECK_LAUNCH();
  return 0;
}
