// The temporal graph store (graph.py, TemporalGraph) straight from the remapped behaviour log, on the device: what
// graph_storage.py:93-246 builds per (entity, slice) cell -- a 1-hop list, a capped 2-hop list and the degree behind every 2-hop
// entry -- as one CSR per side in HBM, with the per-cell counter-based draws of TemporalGraph.from_log(draws="cell").
//
// The draw rule (uint64, wrapping; the finaliser of hash_uniform, common.h):
//   G = 0x9E3779B97F4A7C15;  mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31
//   key(seed, tag, c, j) = mix(mix(seed + G * ((tag << 40) + c + 1)) + G * (j + 1)) >> 32
//   tag 0 item shuffle, 1 item down-sample, 2 user shuffle, 3 user down-sample; c = e * S + t; j = position.
//   "The random order of n positions" = the positions sorted by (key, position).
//
// score_graph_build_1hop, both sides, per side:
//   keys     key = cell of the event (e * S + t), value = its position in the log; an event whose user, item or slice lies
//            outside its range gets the key of a sink behind every cell (n_ent * S);
//   sort     score_sort_pairs (sort.hip): stable, so a cell keeps log order; one, two or three radix passes by bits(n_ent * S);
//   segments a binary search per cell over the sorted keys gives off1; nbr1[p] = other id of the event at sorted position p.
// score_graph_build_2hop, one side, called twice:
//   with nbr2 == NULL   the side's over-long cells (more than max_1hop entries) are put in their random order: their entries,
//            compacted (a scan over the cells' lengths), are sorted by key and then stably by cell -- two score_sort_pairs over
//            the compacted entries only -- and written back in place.  Then a count kernel gives every cell's capped 2-hop
//            length and a scan gives off2; the total comes back to the host (the caller sizes nbr2 / deg2 by it).
//   with nbr2 != NULL   a fill kernel writes nbr2 and deg2: a wave per non-empty cell; a cell with more than max_2hop
//            candidates (at most max_1hop^2 <= 4096) keeps the first max_2hop of their random order, selected by rank over
//            (key, position) in LDS.
// The reference's pass order (graph_storage.py:147-189, 193-237) is the caller's: item count, item fill (it reads user lists
// still in log order), user count (it shuffles the user lists), user fill (it reads item lists as the item pass left them).
//
// The scan is reduce-then-scan (block sums, one workgroup over the block sums, a second pass): no workgroup waits on
// another.  Nothing here is atomic: every array is a pure function of (log, caps, seed).
#include "common.h"
#include "cellkey.h"
#include "devprep.h"

namespace {

constexpr int GB_MAX_CAND = 4096;                        // max_1hop^2 at most
constexpr int FILL_WAVES = 2;

struct Side {                       // one side's view of the build: its own lists and the other side's
  int64_t* off1; int32_t* nbr1;
  const int64_t* other_off1; const int32_t* other_nbr1;
  int64_t ncell, other_ncell;
  int32_t other_base, n_other, S, max_1hop, max_2hop;
  uint64_t seed, tag_shuffle, tag_sample;
};

// ---------------------------------------------------------------------------------------------------------------- 1-hop
__global__ __launch_bounds__(DP_THREADS) void gb_keys_kernel(const int32_t* __restrict__ uid, const int32_t* __restrict__ iid,
                                                            const int32_t* __restrict__ t_idx, int64_t n, int32_t U, int32_t I,
                                                            int32_t S, int item_side, uint32_t* __restrict__ keys,
                                                            uint32_t* __restrict__ vals) {
  const int64_t ncell = (int64_t)(item_side ? I : U) * S;
  DP_LOOP(i, n) {
    const int64_t u = (int64_t)uid[i] - 1, it = (int64_t)iid[i] - U - 1, t = t_idx[i];
    const bool ok = u >= 0 && u < U && it >= 0 && it < I && t >= 0 && t < S;
    keys[i] = (uint32_t)(ok ? (item_side ? it : u) * S + t : ncell);
    vals[i] = (uint32_t)i;
  }
}

__global__ __launch_bounds__(DP_THREADS) void gb_segments_kernel(const uint32_t* __restrict__ keys,
                                                                const uint32_t* __restrict__ vals,
                                                                const int32_t* __restrict__ other, int64_t n, int64_t ncell,
                                                                int64_t* __restrict__ off1, int32_t* __restrict__ nbr1,
                                                                uint32_t* __restrict__ cellkey) {
  const int64_t total = n > ncell + 1 ? n : ncell + 1;
  DP_LOOP(i, total) {
    if (i < n) {
      const uint32_t k = keys[i], v = vals[i];
      nbr1[i] = ((int64_t)k < ncell && (int64_t)v < n) ? other[v] : 0;
      cellkey[i] = k;
    }
    if (i <= ncell) off1[i] = dp_lower_bound(keys, n, (uint32_t)i);
  }
}

// --------------------------------------------------------------------------------------------------------------- shuffle
// len[c] = the cell's length if it is over-long, else 0
__global__ __launch_bounds__(DP_THREADS) void gb_over_len_kernel(const int64_t* __restrict__ off1, int64_t ncell,
                                                                int32_t max_1hop, int32_t* __restrict__ len) {
  DP_LOOP(c, ncell) {
    const int64_t l = off1[c + 1] - off1[c];
    len[c] = l > max_1hop ? (int32_t)l : 0;
  }
}

// the entries of the over-long cells, compacted in (cell, log) order: key = the draw of (cell, position), value = the entry's
// place in nbr1.  ooff: the scan of gb_over_len_kernel's lengths.
__global__ __launch_bounds__(DP_THREADS) void gb_compact_kernel(const uint32_t* __restrict__ cellkey,
                                                               const int64_t* __restrict__ off1,
                                                               const int64_t* __restrict__ ooff, int64_t n, int64_t ncell,
                                                               int32_t max_1hop, uint64_t seed, uint64_t tag,
                                                               uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  DP_LOOP(p, n) {
    const int64_t c = cellkey[p];
    if (c >= ncell) continue;
    const int64_t b = off1[c];
    if (off1[c + 1] - b <= max_1hop || p < b || p >= off1[c + 1]) continue;      // (p outside its cell: never with the keys
    const int64_t q = ooff[c] + (p - b);                                         //  score_graph_build_1hop left in temp)
    keys[q] = gb_key(gb_cell_hash(seed, tag, (uint64_t)c), (uint64_t)(p - b));
    vals[q] = (uint32_t)p;
  }
}

__global__ __launch_bounds__(DP_THREADS) void gb_rekey_kernel(const uint32_t* __restrict__ cellkey,
                                                             const uint32_t* __restrict__ vals, int64_t m, int64_t n,
                                                             int64_t ncell, uint32_t* __restrict__ keys) {
  DP_LOOP(i, m) {
    const int64_t v = vals[i];
    const uint32_t c = v < n ? cellkey[v] : (uint32_t)ncell;
    keys[i] = (int64_t)c < ncell ? c : (uint32_t)(ncell - 1);                     // (inside bits(ncell - 1), whatever temp held)
  }
}

__global__ __launch_bounds__(DP_THREADS) void gb_gather_kernel(const int32_t* __restrict__ nbr1,
                                                              const uint32_t* __restrict__ vals, int64_t m, int64_t n,
                                                              uint32_t* __restrict__ picked) {
  DP_LOOP(i, m) {
    const int64_t v = vals[i];
    picked[i] = v < n ? (uint32_t)nbr1[v] : 0u;
  }
}

// compacted slot i (now sorted by (cell, key, position)) goes back to entry i - ooff[cell] of its cell
__global__ __launch_bounds__(DP_THREADS) void gb_writeback_kernel(const uint32_t* __restrict__ cells,
                                                                 const uint32_t* __restrict__ picked,
                                                                 const int64_t* __restrict__ off1,
                                                                 const int64_t* __restrict__ ooff, int64_t m, int64_t ncell,
                                                                 int32_t* __restrict__ nbr1) {
  DP_LOOP(i, m) {
    const int64_t c = cells[i];
    if (c >= ncell) continue;
    const int64_t j = i - ooff[c];
    if (j < 0 || j >= off1[c + 1] - off1[c]) continue;
    nbr1[off1[c] + j] = (int32_t)picked[i];
  }
}

// ----------------------------------------------------------------------------------------------------------------- 2-hop
// neighbour x of a cell in slice t: the length d of x's cell, where it starts, and how many entries it contributes
__device__ __forceinline__ int32_t gb_contrib(const Side& a, int32_t x, int32_t t, int32_t& d, int32_t& start) {
  d = 0; start = 0;
  const int64_t oe = (int64_t)x - a.other_base;
  if (oe < 0 || oe >= a.n_other) return 0;
  const int64_t oc = oe * a.S + t;
  const int64_t o0 = a.other_off1[oc];
  d = (int32_t)(a.other_off1[oc + 1] - o0);
  start = (int32_t)o0;
  return d > 1 ? (d < a.max_1hop ? d : a.max_1hop) : 0;
}

__global__ __launch_bounds__(DP_THREADS) void gb_count_kernel(Side a, int32_t* __restrict__ len2) {
  DP_LOOP(c, a.ncell) {
    const int64_t b = a.off1[c], l = a.off1[c + 1] - b;
    const int32_t m = (int32_t)(l < a.max_1hop ? l : a.max_1hop), t = (int32_t)(c % a.S);
    int32_t cand = 0, d, st;
    for (int32_t i = 0; i < m; ++i) cand += gb_contrib(a, a.nbr1[b + i], t, d, st);
    len2[c] = cand < a.max_2hop ? cand : a.max_2hop;
  }
}

__device__ __forceinline__ void gb_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A wave takes 64 consecutive cells at a time (a lane reads one cell's length), then the non-empty ones in turn, the whole
// wave on one cell: lane i looks up neighbour i (max_1hop <= 64), a wave scan places the contributions.
__global__ __launch_bounds__(FILL_WAVES * 64) void gb_fill_kernel(Side a, const int64_t* __restrict__ off2,
                                                                 int32_t* __restrict__ nbr2, int32_t* __restrict__ deg2,
                                                                 int64_t cap2) {
  __shared__ uint32_t skey[FILL_WAVES][GB_MAX_CAND];
  __shared__ uint8_t ssrc[FILL_WAVES][GB_MAX_CAND];                // which neighbour a candidate came through
  __shared__ int32_t sstart[FILL_WAVES][64], sbase[FILL_WAVES][64], sdeg[FILL_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t nwaves = (int64_t)gridDim.x * FILL_WAVES;
  for (int64_t base = ((int64_t)blockIdx.x * FILL_WAVES + w) * 64; base < a.ncell; base += nwaves * 64) {
    const int64_t cl = base + lane;
    const bool some = cl < a.ncell && a.off1[cl + 1] > a.off1[cl];
    uint64_t live = __ballot(some);
    while (live) {                                                  // (wave-uniform)
      const int src = __ffsll((unsigned long long)live) - 1;
      live &= live - 1;
      const int64_t c = base + src;
      const int64_t b1 = a.off1[c], l = a.off1[c + 1] - b1;
      const int32_t m = (int32_t)(l < a.max_1hop ? l : a.max_1hop), t = (int32_t)(c % a.S);
      int32_t L = 0, d = 0, ob = 0;
      if (lane < m) L = gb_contrib(a, a.nbr1[b1 + lane], t, d, ob);
      int32_t incl = L;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int32_t y = __shfl_up(incl, off, SCORE_WAVE);
        if (lane >= off) incl += y;
      }
      const int32_t cand = __shfl(incl, 63, SCORE_WAVE), start = incl - L;
      if (cand == 0 || cand > GB_MAX_CAND) continue;
      const int64_t o2 = off2[c];
      const int32_t n_out = cand < a.max_2hop ? cand : a.max_2hop;
      if (o2 < 0 || o2 + n_out > cap2) continue;                    // (never with this build's own off2)
      if (cand <= a.max_2hop) {
        for (int i = 0; i < m; ++i) {
          const int32_t Li = __shfl(L, i, SCORE_WAVE), si = __shfl(start, i, SCORE_WAVE);
          const int32_t bi = __shfl(ob, i, SCORE_WAVE), di = __shfl(d, i, SCORE_WAVE);
          if (lane < Li) {
            nbr2[o2 + si + lane] = a.other_nbr1[(int64_t)bi + lane];
            deg2[o2 + si + lane] = di;
          }
        }
        continue;
      }
      // more candidates than max_2hop: the first max_2hop of their random order, by rank over (key, position)
      const uint64_t h = gb_cell_hash(a.seed, a.tag_sample, (uint64_t)c);
      sstart[w][lane] = start; sbase[w][lane] = ob; sdeg[w][lane] = d;
      for (int i = 0; i < m; ++i) {
        const int32_t Li = __shfl(L, i, SCORE_WAVE), si = __shfl(start, i, SCORE_WAVE);
        if (lane < Li) {
          skey[w][si + lane] = gb_key(h, (uint64_t)(si + lane));
          ssrc[w][si + lane] = (uint8_t)i;
        }
      }
      gb_wave_sync();
      for (int32_t j0 = 0; j0 < cand; j0 += 64) {
        const int32_t j = j0 + lane;
        const bool on = j < cand;
        const uint32_t kj = on ? skey[w][j] : 0u;
        int32_t rank = 0;
        for (int32_t i = 0; i < cand; ++i) {
          const uint32_t ki = skey[w][i];                           // (one address for the wave: a broadcast)
          rank += (ki < kj || (ki == kj && i < j)) ? 1 : 0;
        }
        if (on && rank < a.max_2hop) {
          const int i = ssrc[w][j];
          nbr2[o2 + rank] = a.other_nbr1[(int64_t)sbase[w][i] + (j - sstart[w][i])];
          deg2[o2 + rank] = sdeg[w][i];
        }
      }
      gb_wave_sync();                                               // (the next cell writes the same LDS)
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ host
struct Temp { uint32_t* cellkey[2]; SortBufs sort; int32_t* len; int64_t* bsum; int64_t total_bytes; };

Temp carve(void* temp, int64_t n, int64_t ncell_max) {
  Temp t;
  Carver c(temp);
  t.cellkey[0] = c.words<uint32_t>(n);
  t.cellkey[1] = c.words<uint32_t>(n);
  c.sort_pairs(t.sort, n);
  t.len = c.words<int32_t>(ncell_max);
  t.bsum = c.block_sums(ncell_max);
  c.sort_temp(t.sort, n);
  t.total_bytes = c.off;
  return t;
}

int check_args(const score_graph_build_t* g, const void* temp, int64_t temp_bytes) {
  if (!g || g->struct_bytes != (int64_t)sizeof(score_graph_build_t)) return SCORE_E_BADARG;
  if (!g->uid || !g->iid || !g->t_idx || !g->user_off1 || !g->user_nbr1 || !g->item_off1 || !g->item_nbr1 || !temp)
    return SCORE_E_BADARG;
  if (g->n_events <= 0 || g->n_users <= 0 || g->n_items <= 0 || g->time_slice_num <= 0 || g->max_1hop <= 0 || g->max_2hop <= 0)
    return SCORE_E_BADARG;
  const int64_t lim = 1ll << 31;
  if (g->n_events >= lim || (int64_t)g->n_users * g->time_slice_num >= lim || (int64_t)g->n_items * g->time_slice_num >= lim ||
      (int64_t)g->n_users + g->n_items >= lim || (int64_t)g->max_1hop * g->max_1hop > GB_MAX_CAND)
    return SCORE_E_SHAPE;
  if (score_graph_build_temp_bytes(g->n_events, g->n_users, g->n_items, g->time_slice_num) > temp_bytes) return SCORE_E_WORKSPACE;
  return 0;
}

int64_t ncell_max_of(const score_graph_build_t* g) {
  return (int64_t)(g->n_users > g->n_items ? g->n_users : g->n_items) * g->time_slice_num;
}

}  // namespace

extern "C" int64_t score_graph_build_temp_bytes(int64_t n_events, int32_t n_users, int32_t n_items, int32_t time_slice_num) {
  if (n_events <= 0 || n_events >= (1ll << 31) || n_users <= 0 || n_items <= 0 || time_slice_num <= 0) return -1;
  const int64_t ncell = (int64_t)(n_users > n_items ? n_users : n_items) * time_slice_num;
  if (ncell >= (1ll << 31)) return -1;
  return carve(nullptr, n_events, ncell).total_bytes;
}

extern "C" int score_graph_build_1hop(const score_graph_build_t* g, void* temp, int64_t temp_bytes, void* stream) {
  SCORE_TRY(check_args(g, temp, temp_bytes));
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = g->n_events;
  const Temp t = carve(temp, n, ncell_max_of(g));
  for (int side = 0; side < 2; ++side) {
    const int64_t ncell = (int64_t)(side ? g->n_items : g->n_users) * g->time_slice_num;
    SortBufs b = t.sort;
    hipLaunchKernelGGL(gb_keys_kernel, dim3(dp_grid(n)), dim3(DP_THREADS), 0, s, g->uid, g->iid, g->t_idx, n, g->n_users,
                       g->n_items, g->time_slice_num, side, b.k0, b.v0);
    SCORE_CHECK_LAUNCH();
    SCORE_TRY(dp_sort(b, n, dp_bits_of((uint32_t)ncell), s));
    hipLaunchKernelGGL(gb_segments_kernel, dim3(dp_grid(n > ncell + 1 ? n : ncell + 1)), dim3(DP_THREADS), 0, s, b.k0, b.v0,
                       side ? g->uid : g->iid, n, ncell, side ? g->item_off1 : g->user_off1,
                       side ? g->item_nbr1 : g->user_nbr1, t.cellkey[side]);
    SCORE_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int score_graph_build_2hop(const score_graph_build_t* g, int32_t item_side, int64_t* off2, int32_t* nbr2,
                                      int32_t* deg2, int64_t cap2, int64_t* total, void* temp, int64_t temp_bytes,
                                      void* stream) {
  SCORE_TRY(check_args(g, temp, temp_bytes));
  if (!off2 || (item_side != 0 && item_side != 1)) return SCORE_E_BADARG;
  if (nbr2 ? (!deg2 || cap2 <= 0) : !total) return SCORE_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = g->n_events;
  const int32_t S = g->time_slice_num;
  Side a;
  a.off1 = item_side ? g->item_off1 : g->user_off1;
  a.nbr1 = item_side ? g->item_nbr1 : g->user_nbr1;
  a.other_off1 = item_side ? g->user_off1 : g->item_off1;
  a.other_nbr1 = item_side ? g->user_nbr1 : g->item_nbr1;
  a.ncell = (int64_t)(item_side ? g->n_items : g->n_users) * S;
  a.n_other = item_side ? g->n_users : g->n_items;
  a.other_ncell = (int64_t)a.n_other * S;
  a.other_base = item_side ? 1 : g->n_users + 1;
  a.S = S; a.max_1hop = g->max_1hop; a.max_2hop = g->max_2hop;
  a.seed = g->seed; a.tag_shuffle = item_side ? 0 : 2; a.tag_sample = item_side ? 1 : 3;
  if (nbr2) {
    const int64_t groups = cdiv64(cdiv64(a.ncell, 64), FILL_WAVES);
    hipLaunchKernelGGL(gb_fill_kernel, dim3((unsigned)(groups < 8192 ? groups : 8192)), dim3(FILL_WAVES * 64), 0, s, a, off2,
                       nbr2, deg2, cap2);
    SCORE_CHECK_LAUNCH();
    return 0;
  }
  const Temp t = carve(temp, n, ncell_max_of(g));
  const uint32_t* cellkey = t.cellkey[item_side];
  // the over-long cells' entries, in their random order
  hipLaunchKernelGGL(gb_over_len_kernel, dim3(dp_grid(a.ncell)), dim3(DP_THREADS), 0, s, a.off1, a.ncell, a.max_1hop, t.len);
  SCORE_CHECK_LAUNCH();
  SCORE_TRY(gb_scan(t.len, a.ncell, t.bsum, off2, s));
  int64_t n_over = 0;
  SCORE_TRY(dp_read_words(off2 + a.ncell, &n_over, 1, s, nullptr));
  if (n_over < 0 || n_over > n) return SCORE_E_BADARG;
  if (n_over > 0) {
    SortBufs b = t.sort;
    hipLaunchKernelGGL(gb_compact_kernel, dim3(dp_grid(n)), dim3(DP_THREADS), 0, s, cellkey, a.off1, off2, n, a.ncell,
                       a.max_1hop, a.seed, a.tag_shuffle, b.k0, b.v0);
    SCORE_CHECK_LAUNCH();
    SCORE_TRY(dp_sort(b, n_over, 32, s));
    hipLaunchKernelGGL(gb_rekey_kernel, dim3(dp_grid(n_over)), dim3(DP_THREADS), 0, s, cellkey, b.v0, n_over, n, a.ncell, b.k0);
    SCORE_CHECK_LAUNCH();
    SCORE_TRY(dp_sort(b, n_over, dp_bits_of((uint32_t)(a.ncell - 1)), s));
    hipLaunchKernelGGL(gb_gather_kernel, dim3(dp_grid(n_over)), dim3(DP_THREADS), 0, s, a.nbr1, b.v0, n_over, n, b.k1);
    SCORE_CHECK_LAUNCH();
    hipLaunchKernelGGL(gb_writeback_kernel, dim3(dp_grid(n_over)), dim3(DP_THREADS), 0, s, b.k0, b.k1, a.off1, off2, n_over,
                       a.ncell, a.nbr1);
    SCORE_CHECK_LAUNCH();
  }
  // the capped 2-hop lengths and their scan
  hipLaunchKernelGGL(gb_count_kernel, dim3(dp_grid(a.ncell)), dim3(DP_THREADS), 0, s, a, t.len);
  SCORE_CHECK_LAUNCH();
  SCORE_TRY(gb_scan(t.len, a.ncell, t.bsum, off2, s));
  return dp_read_words(off2 + a.ncell, total, 1, s, nullptr);
}
