// Device-side batch assembly for the point baselines: replaces the per-line Python of the reference's point loaders
// (point_models/data_loader.py: DataLoaderUserSeq :15-87, DataLoaderDualSeq :89-185) -- two or three readline()s, a split,
// a dict lookup per id and an np.stack per batch -- with ONE launch over a sequence store that was parsed once
// (score_amd/pointdata.py, PointSeqStore) and lives in HBM.
//   a history holds the last max_len ids of its line as ROWS of the feature-row table; shorter than T, it is padded by
//   repeating its last id (:52-56);
//   the reported length is the untruncated one (:60);
//   all 1 + neg samples of a line share the line's user history, user row and length (:58-66): the history's T x Fi words are
//   resolved once per line into LDS and stored per_line times;
//   the dual form's item-side histories are per sample (:150-160): resolved into LDS a chunk of samples at a time;
//   the tensors a point model does not use are written as zeros here, so no memset launch surrounds the kernel.
// The kernel is bound by its launch and by stores: every large span goes out as 16-byte stores from its first 16-byte
// boundary on, with dword stores for the at most three words in front of it and behind it.
#include "common.h"

#define PL_THREADS 256
#define PL_LDS_WORDS 8192      // 32 KiB: one user history (T * Fi words) or a chunk of item histories (T * Fu words each)

struct PointAssemble {
  const int64_t* user_off; const int32_t* user_seq; const int32_t* user_len;
  const int64_t* item_off; const int32_t* item_seq; const int32_t* item_len;
  const int32_t* target_user; const int32_t* target_item;
  const int32_t* user_rows; const int32_t* item_rows;
  int64_t n_user_rows, n_item_rows, first_line;
  int32_t* user_1hop; int32_t* user_2hop; int32_t* item_1hop; int32_t* item_2hop;
  int32_t* out_user; int32_t* out_item; int32_t* label; int32_t* length; int32_t* length2;     // length2 null: single form
  int per_line, T, Fu, Fi;
};

// n words at dst, by the whole workgroup: word o is src[o % period] (src in LDS), or 0 where src is null
__device__ __forceinline__ void pl_put_span(int32_t* __restrict__ dst, const int32_t* src, int n, int period) {
  const int tid = (int)threadIdx.x;
  int head = (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(dst) >> 2)) & 3u);      // words up to the 16-byte boundary
  if (head > n) head = n;
  const int nq = (n - head) >> 2;
  if (tid < head) dst[tid] = src ? src[tid % period] : 0;
  for (int q = tid; q < nq; q += PL_THREADS) {
    const int o = head + 4 * q;
    int4 v = make_int4(0, 0, 0, 0);
    if (src) {
      int e = o % period;
      v.x = src[e]; e = e + 1 == period ? 0 : e + 1;
      v.y = src[e]; e = e + 1 == period ? 0 : e + 1;
      v.z = src[e]; e = e + 1 == period ? 0 : e + 1;
      v.w = src[e];
    }
    *reinterpret_cast<int4*>(dst + o) = v;
  }
  const int o = head + 4 * nq + tid;
  if (o < n) dst[o] = src ? src[o % period] : 0;
}

// Where a history lies.  span(h, T, b, m): history h's window is seq[b .. b + m), m <= T ids (m = 0: none); row(x): the row
// of the feature table a stored word x names, or -1 for a row of zeros.
// The file form (PointSeqStore): history h is seq[off[h] .. off[h + 1]), already cut to the last max_len = T ids, and the words
// are rows, clamped into the table.
struct PlFileHist {
  const int64_t* off; const int32_t* seq; int64_t n_rows;
  __device__ __forceinline__ void span(int64_t h, int T, int64_t& b, int& m) const {
    b = off[h];
    m = (int)(off[h + 1] - b);
  }
  __device__ __forceinline__ int64_t row(int32_t x) const { return x < 0 ? 0 : (x >= n_rows ? n_rows - 1 : (int64_t)x); }
};
// The log form (PointLogStore, csrc/pointhist.hip): history h belongs to the entity ids[h]; entity e's kept history is the last
// len[e] ids of seq[off[e] .. off[e + 1]) and the window the last min(len[e], T) of those.  The words are ids of the OTHER
// side: row = id - row_lo; id 0 (the reference's stand-in history of an item without one) and anything outside the table is a
// row of zeros.  An entity outside [id_lo, id_lo + n_ent) has no history.
struct PlLogHist {
  const int32_t* ids; const int64_t* off; const int32_t* seq; const int32_t* len;
  int64_t id_lo, n_ent, row_lo, n_rows;
  __device__ __forceinline__ void span(int64_t h, int T, int64_t& b, int& m) const {
    const int64_t e = (int64_t)ids[h] - id_lo;
    b = 0; m = 0;
    if (e < 0 || e >= n_ent) return;
    const int32_t l = len[e];
    m = l < T ? l : T;
    if (m < 0) m = 0;
    b = off[e + 1] - m;
    if (b < off[e]) { b = off[e]; m = (int)(off[e + 1] - b); }
  }
  __device__ __forceinline__ int64_t row(int32_t x) const {
    const int64_t r = (int64_t)x - row_lo;
    return (r < 0 || r >= n_rows) ? -1 : r;
  }
};

// words [0, n_hist * T * F) of `lds`: history first_hist + s, position t, feature f -> feature f of the row of the history's
// id at min(t, m - 1) (m ids in the window: the pad repeats the last one).  An empty history gives 0.
template <class Hist>
__device__ __forceinline__ void pl_resolve(int32_t* lds, const Hist h, const int32_t* __restrict__ rows, int64_t first_hist,
                                           int n_hist, int T, int F) {
  const int per = T * F, n = n_hist * per;
  for (int w = (int)threadIdx.x; w < n; w += PL_THREADS) {
    const int s = w / per, r = w - s * per, t = r / F, f = r - t * F;
    int64_t b;
    int m;
    h.span(first_hist + s, T, b, m);
    int32_t v = 0;
    if (m > 0) {
      const int64_t row = h.row(h.seq[b + (t < m ? t : m - 1)]);
      if (row >= 0) v = rows[row * F + f];
    }
    lds[w] = v;
  }
}

// a line's item_1hop span in the dual form: the item-side histories resolved into LDS a chunk of samples at a time
template <class Hist>
__device__ __forceinline__ void pl_item_side(int32_t* lds, const Hist h, const int32_t* __restrict__ rows, int64_t first_hist,
                                             int per_line, int T, int F, int32_t* __restrict__ dst) {
  const int pi = T * F;
  const int chunk = PL_LDS_WORDS / pi;                   // samples whose histories fit in LDS together (>= 1: checked by the caller)
  for (int c0 = 0; c0 < per_line; c0 += chunk) {
    const int n = per_line - c0 < chunk ? per_line - c0 : chunk;
    if (c0) __syncthreads();                             // the chunk before has been read out
    pl_resolve(lds, h, rows, first_hist + c0, n, T, F);
    __syncthreads();
    pl_put_span(dst + (int64_t)c0 * pi, lds, n * pi, n * pi);
  }
}

// grid (n_lines, 3): part 0 = the user history, the targets, label and lengths of a line; part 1 = its item_1hop span;
// part 2 = its two 2-hop spans (zeros)
__global__ __launch_bounds__(PL_THREADS) void point_assemble_kernel(PointAssemble a) {
  __shared__ int32_t lds[PL_LDS_WORDS];
  const int tid = (int)threadIdx.x, part = (int)blockIdx.y, per_line = a.per_line;
  const int64_t gl = a.first_line + blockIdx.x;            // line of the store
  const int64_t s0 = (int64_t)blockIdx.x * per_line;       // its first sample in the batch
  const int pu = a.T * a.Fi, pi = a.T * a.Fu;              // words of a sample's user-side / item-side history
  if (part == 0) {
    pl_resolve(lds, PlFileHist{a.user_off, a.user_seq, a.n_item_rows}, a.item_rows, gl, 1, a.T, a.Fi);
    __syncthreads();
    pl_put_span(a.user_1hop + s0 * pu, lds, per_line * pu, pu);
    int64_t tu = a.target_user[gl];
    tu = tu < 0 ? 0 : (tu >= a.n_user_rows ? a.n_user_rows - 1 : tu);
    for (int e = tid; e < per_line * a.Fu; e += PL_THREADS) a.out_user[s0 * a.Fu + e] = a.user_rows[tu * a.Fu + e % a.Fu];
    for (int e = tid; e < per_line * a.Fi; e += PL_THREADS) {
      const int c = e / a.Fi, f = e - c * a.Fi;
      int64_t ti = a.target_item[gl * per_line + c];
      ti = ti < 0 ? 0 : (ti >= a.n_item_rows ? a.n_item_rows - 1 : ti);
      a.out_item[s0 * a.Fi + e] = a.item_rows[ti * a.Fi + f];
    }
    const int32_t len = a.user_len[gl];
    for (int c = tid; c < per_line; c += PL_THREADS) {
      a.label[s0 + c] = c == 0 ? 1 : 0;                    // a line's first item is the positive (:62-65)
      a.length[s0 + c] = len;
      if (a.length2) a.length2[s0 + c] = a.item_len[gl * per_line + c];
    }
  } else if (part == 1) {
    if (!a.length2) {
      pl_put_span(a.item_1hop + s0 * pi, nullptr, per_line * pi, 1);
    } else {
      pl_item_side(lds, PlFileHist{a.item_off, a.item_seq, a.n_user_rows}, a.user_rows, gl * per_line, per_line, a.T, a.Fu,
                   a.item_1hop + s0 * pi);
    }
  } else {
    pl_put_span(a.user_2hop + s0 * pi, nullptr, per_line * pi, 1);
    pl_put_span(a.item_2hop + s0 * pu, nullptr, per_line * pu, 1);
  }
}

extern "C" int score_point_batch_assemble(const score_point_store_t* st, int64_t first_line, int32_t n_lines, int32_t per_line,
                                          int32_t T, int32_t Fu, int32_t Fi, const score_batch_out_t* out, int32_t* length2,
                                          void* stream) {
  if (!st || !out || st->struct_bytes != (int64_t)sizeof(score_point_store_t)) return SCORE_E_BADARG;
  if (n_lines <= 0 || per_line <= 0 || T <= 0 || Fu <= 0 || Fi <= 0 || first_line < 0) return SCORE_E_BADARG;
  if (!st->user_off || !st->user_seq || !st->user_len || !st->target_user || !st->target_item || !st->user_rows ||
      !st->item_rows || st->n_user_rows <= 0 || st->n_item_rows <= 0)
    return SCORE_E_BADARG;
  if (length2 && (!st->item_off || !st->item_seq || !st->item_len)) return SCORE_E_BADARG;
  if (!out->user_1hop || !out->user_2hop || !out->item_1hop || !out->item_2hop || !out->target_user || !out->target_item ||
      !out->label || !out->length)
    return SCORE_E_BADARG;
  if (first_line + n_lines > st->n_lines || per_line != st->per_line || T != st->max_len) return SCORE_E_BADARG;
  const int64_t B = (int64_t)n_lines * per_line;
  if ((int64_t)T * Fi > PL_LDS_WORDS || (int64_t)T * Fu > PL_LDS_WORDS || B * T * (Fu > Fi ? Fu : Fi) >= ((int64_t)1 << 31))
    return SCORE_E_SHAPE;
  PointAssemble a;
  a.user_off = st->user_off; a.user_seq = st->user_seq; a.user_len = st->user_len;
  a.item_off = st->item_off; a.item_seq = st->item_seq; a.item_len = st->item_len;
  a.target_user = st->target_user; a.target_item = st->target_item;
  a.user_rows = st->user_rows; a.item_rows = st->item_rows;
  a.n_user_rows = st->n_user_rows; a.n_item_rows = st->n_item_rows; a.first_line = first_line;
  a.user_1hop = out->user_1hop; a.user_2hop = out->user_2hop; a.item_1hop = out->item_1hop; a.item_2hop = out->item_2hop;
  a.out_user = out->target_user; a.out_item = out->target_item; a.label = out->label; a.length = out->length;
  a.length2 = length2;
  a.per_line = per_line; a.T = T; a.Fu = Fu; a.Fi = Fi;
  hipLaunchKernelGGL(point_assemble_kernel, dim3((unsigned)n_lines, 3), dim3(PL_THREADS), 0, (hipStream_t)stream, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}

// ---- the same batches from per-entity histories (PointLogStore: built from the log by csrc/pointhist.hip) --------------------
// What differs from the file form: a history is found through the ENTITY's id (the line's user; a sample's item), the window
// is the last min(len, T) ids of the entity's kept segment, an id becomes a row by subtraction (users 1 .. U are rows
// 0 .. U - 1 of user_rows, items U + 1 .. U + I rows 0 .. I - 1 of item_rows), an item without history is the reference's
// one-element history [0] -- zeros, length 1 (gen_history_point.py:58-59) --, and the dual form's target_user is the last id of
// the kept history of the line's LAST item as written (data_loader.py:141-143's rebinding), 0 where it has none.
struct PointAssembleLog {
  const int64_t* user_off; const int32_t* user_seq; const int32_t* user_len;
  const int64_t* item_off; const int32_t* item_seq; const int32_t* item_len;
  const int32_t* line_user; const int32_t* line_items; const int32_t* line_last_item;
  const int32_t* user_rows; const int32_t* item_rows;
  int64_t n_users, n_items, first_line;
  int32_t* user_1hop; int32_t* user_2hop; int32_t* item_1hop; int32_t* item_2hop;
  int32_t* out_user; int32_t* out_item; int32_t* label; int32_t* length; int32_t* length2;     // length2 null: single form
  int per_line, T, Fu, Fi;
};

// grid (n_lines, 3), the parts of point_assemble_kernel
__global__ __launch_bounds__(PL_THREADS) void point_assemble_log_kernel(PointAssembleLog a) {
  __shared__ int32_t lds[PL_LDS_WORDS];
  const int tid = (int)threadIdx.x, part = (int)blockIdx.y, per_line = a.per_line;
  const int64_t gl = a.first_line + blockIdx.x;            // line of the store
  const int64_t s0 = (int64_t)blockIdx.x * per_line;       // its first sample in the batch
  const int pu = a.T * a.Fi, pi = a.T * a.Fu;              // words of a sample's user-side / item-side history
  const int64_t U = a.n_users, I = a.n_items;
  // (users' histories hold item ids, items' histories user ids)
  const PlLogHist hu{a.line_user, a.user_off, a.user_seq, a.user_len, 1, U, U + 1, I};
  const PlLogHist hi{a.line_items, a.item_off, a.item_seq, a.item_len, U + 1, I, 1, U};
  if (part == 0) {
    pl_resolve(lds, hu, a.item_rows, gl, 1, a.T, a.Fi);
    __syncthreads();
    pl_put_span(a.user_1hop + s0 * pu, lds, per_line * pu, pu);
    int64_t tu = (int64_t)a.line_user[gl] - 1;             // row of user_rows, or outside: zeros
    if (a.length2) {
      const int64_t e = (int64_t)a.line_last_item[gl] - (U + 1);
      tu = -1;
      if (e >= 0 && e < I && a.item_len[e] > 0 && a.item_off[e + 1] > a.item_off[e]) tu = (int64_t)a.item_seq[a.item_off[e + 1] - 1] - 1;
    }
    const bool tu_ok = tu >= 0 && tu < U;
    for (int e = tid; e < per_line * a.Fu; e += PL_THREADS) a.out_user[s0 * a.Fu + e] = tu_ok ? a.user_rows[tu * a.Fu + e % a.Fu] : 0;
    for (int e = tid; e < per_line * a.Fi; e += PL_THREADS) {
      const int c = e / a.Fi, f = e - c * a.Fi;
      const int64_t ti = (int64_t)a.line_items[gl * per_line + c] - (U + 1);
      a.out_item[s0 * a.Fi + e] = (ti >= 0 && ti < I) ? a.item_rows[ti * a.Fi + f] : 0;
    }
    const int64_t eu = (int64_t)a.line_user[gl] - 1;
    const int32_t len = (eu >= 0 && eu < U) ? a.user_len[eu] : 0;
    for (int c = tid; c < per_line; c += PL_THREADS) {
      a.label[s0 + c] = c == 0 ? 1 : 0;
      a.length[s0 + c] = len;
      if (a.length2) {
        const int64_t ei = (int64_t)a.line_items[gl * per_line + c] - (U + 1);
        const int32_t l = (ei >= 0 && ei < I) ? a.item_len[ei] : 0;
        a.length2[s0 + c] = l > 0 ? l : 1;                 // (no history: the one-element history [0])
      }
    }
  } else if (part == 1) {
    if (!a.length2) pl_put_span(a.item_1hop + s0 * pi, nullptr, per_line * pi, 1);
    else pl_item_side(lds, hi, a.user_rows, gl * per_line, per_line, a.T, a.Fu, a.item_1hop + s0 * pi);
  } else {
    pl_put_span(a.user_2hop + s0 * pi, nullptr, per_line * pi, 1);
    pl_put_span(a.item_2hop + s0 * pu, nullptr, per_line * pu, 1);
  }
}

extern "C" int score_point_batch_assemble_log(const score_point_log_store_t* st, int64_t first_line, int32_t n_lines,
                                              int32_t per_line, int32_t T, int32_t Fu, int32_t Fi, const score_batch_out_t* out,
                                              int32_t* length2, void* stream) {
  if (!st || !out || st->struct_bytes != (int64_t)sizeof(score_point_log_store_t)) return SCORE_E_BADARG;
  if (n_lines <= 0 || per_line <= 0 || T <= 0 || Fu <= 0 || Fi <= 0 || first_line < 0) return SCORE_E_BADARG;
  if (!st->user_hist_off || !st->user_hist_seq || !st->user_hist_len || !st->line_user || !st->line_items || !st->user_rows ||
      !st->item_rows || st->n_users <= 0 || st->n_items <= 0)
    return SCORE_E_BADARG;
  if (length2 && (!st->item_hist_off || !st->item_hist_seq || !st->item_hist_len || !st->line_last_item)) return SCORE_E_BADARG;
  if (!out->user_1hop || !out->user_2hop || !out->item_1hop || !out->item_2hop || !out->target_user || !out->target_item ||
      !out->label || !out->length)
    return SCORE_E_BADARG;
  if (first_line + n_lines > st->n_lines || per_line != st->per_line) return SCORE_E_BADARG;
  const int64_t B = (int64_t)n_lines * per_line;
  if ((int64_t)T * Fi > PL_LDS_WORDS || (int64_t)T * Fu > PL_LDS_WORDS || B * T * (Fu > Fi ? Fu : Fi) >= ((int64_t)1 << 31))
    return SCORE_E_SHAPE;
  PointAssembleLog a;
  a.user_off = st->user_hist_off; a.user_seq = st->user_hist_seq; a.user_len = st->user_hist_len;
  a.item_off = st->item_hist_off; a.item_seq = st->item_hist_seq; a.item_len = st->item_hist_len;
  a.line_user = st->line_user; a.line_items = st->line_items; a.line_last_item = st->line_last_item;
  a.user_rows = st->user_rows; a.item_rows = st->item_rows;
  a.n_users = st->n_users; a.n_items = st->n_items; a.first_line = first_line;
  a.user_1hop = out->user_1hop; a.user_2hop = out->user_2hop; a.item_1hop = out->item_1hop; a.item_2hop = out->item_2hop;
  a.out_user = out->target_user; a.out_item = out->target_item; a.label = out->label; a.length = out->length;
  a.length2 = length2;
  a.per_line = per_line; a.T = T; a.Fu = Fu; a.Fi = Fi;
  hipLaunchKernelGGL(point_assemble_log_kernel, dim3((unsigned)n_lines, 3), dim3(PL_THREADS), 0, (hipStream_t)stream, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}

// ---- lines for arbitrary users (PointLogStore.user_lines) -----------------------------------------------------------------------
// What part 0 of point_assemble_log_kernel writes for the FIRST sample of a single-form line whose line_user is user_ids[l], and
// nothing else: no expanded batch, no zeroed 2-hop spans.  A workgroup per line; known[l] = the id lies in 1 .. n_users.  Plain
// stores only.
struct PointUserLines {
  const int64_t* user_off; const int32_t* user_seq; const int32_t* user_len;
  const int32_t* user_ids; const int32_t* user_rows; const int32_t* item_rows;
  int64_t n_users, n_items;
  int32_t* out_seq; int32_t* length; int32_t* out_user; int32_t* known;
  int T, Fu, Fi;
};

__global__ __launch_bounds__(PL_THREADS) void point_user_lines_kernel(PointUserLines a) {
  __shared__ int32_t lds[PL_LDS_WORDS];
  const int tid = (int)threadIdx.x;
  const int64_t l = blockIdx.x;
  const int pu = a.T * a.Fi;
  const int64_t U = a.n_users, I = a.n_items;
  const PlLogHist hu{a.user_ids, a.user_off, a.user_seq, a.user_len, 1, U, U + 1, I};
  pl_resolve(lds, hu, a.item_rows, l, 1, a.T, a.Fi);
  __syncthreads();
  pl_put_span(a.out_seq + l * pu, lds, pu, pu);
  const int64_t eu = (int64_t)a.user_ids[l] - 1;
  const bool ok = eu >= 0 && eu < U;
  for (int f = tid; f < a.Fu; f += PL_THREADS) a.out_user[l * a.Fu + f] = ok ? a.user_rows[eu * a.Fu + f] : 0;
  if (tid == 0) {
    a.length[l] = ok ? a.user_len[eu] : 0;
    a.known[l] = ok ? 1 : 0;
  }
}

extern "C" int score_point_user_lines(const score_point_log_store_t* st, const int32_t* user_ids, int32_t L, int32_t T, int32_t Fu,
                                      int32_t Fi, int32_t* user_seq, int32_t* length, int32_t* target_user, int32_t* known,
                                      void* stream) {
  if (!st || !user_ids || !user_seq || !length || !target_user || !known) return SCORE_E_BADARG;
  if (st->struct_bytes != (int64_t)sizeof(score_point_log_store_t)) return SCORE_E_BADARG;
  if (L <= 0 || T <= 0 || Fu <= 0 || Fi <= 0) return SCORE_E_BADARG;
  if (!st->user_hist_off || !st->user_hist_seq || !st->user_hist_len || !st->user_rows || !st->item_rows || st->n_users <= 0 ||
      st->n_items <= 0)
    return SCORE_E_BADARG;
  if ((int64_t)T * Fi > PL_LDS_WORDS || (int64_t)L * T * Fi >= ((int64_t)1 << 31) || (int64_t)L * Fu >= ((int64_t)1 << 31))
    return SCORE_E_SHAPE;
  PointUserLines a;
  a.user_off = st->user_hist_off; a.user_seq = st->user_hist_seq; a.user_len = st->user_hist_len;
  a.user_ids = user_ids; a.user_rows = st->user_rows; a.item_rows = st->item_rows;
  a.n_users = st->n_users; a.n_items = st->n_items;
  a.out_seq = user_seq; a.length = length; a.out_user = target_user; a.known = known;
  a.T = T; a.Fu = Fu; a.Fi = Fi;
  hipLaunchKernelGGL(point_user_lines_kernel, dim3((unsigned)L), dim3(PL_THREADS), 0, (hipStream_t)stream, a);
  SCORE_CHECK_LAUNCH();
  return 0;
}
