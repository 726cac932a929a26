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

// words [0, n_hist * T * F) of `lds`: history first_hist + s, position t, feature f -> feature f of the row of the history's
// id at min(t, m - 1) (m kept ids: the pad repeats the last one).  Rows are clamped into the table; an empty history gives 0.
__device__ __forceinline__ void pl_resolve(int32_t* lds, const int64_t* __restrict__ off, const int32_t* __restrict__ seq,
                                           const int32_t* __restrict__ rows, int64_t n_rows, int64_t first_hist, int n_hist,
                                           int T, int F) {
  const int per = T * F, n = n_hist * per;
  for (int w = (int)threadIdx.x; w < n; w += PL_THREADS) {
    const int s = w / per, r = w - s * per, t = r / F, f = r - t * F;
    const int64_t b = off[first_hist + s];
    const int m = (int)(off[first_hist + s + 1] - b);
    int32_t v = 0;
    if (m > 0) {
      int64_t row = seq[b + (t < m ? t : m - 1)];
      row = row < 0 ? 0 : (row >= n_rows ? n_rows - 1 : row);
      v = rows[row * F + f];
    }
    lds[w] = v;
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
    pl_resolve(lds, a.user_off, a.user_seq, a.item_rows, a.n_item_rows, gl, 1, a.T, a.Fi);
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
      const int chunk = PL_LDS_WORDS / pi;                 // samples whose histories fit in LDS together (>= 1: checked by the caller)
      for (int c0 = 0; c0 < per_line; c0 += chunk) {
        const int n = per_line - c0 < chunk ? per_line - c0 : chunk;
        if (c0) __syncthreads();                           // the chunk before has been read out
        pl_resolve(lds, a.item_off, a.item_seq, a.user_rows, a.n_user_rows, gl * per_line + c0, n, a.T, a.Fu);
        __syncthreads();
        pl_put_span(a.item_1hop + (s0 + c0) * pi, lds, n * pi, n * pi);
      }
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
