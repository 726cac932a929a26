// Internal (non-ABI) launchers shared between the translation units of libscore_hip.
#pragma once
#include "common.h"

// gemm.hip / gemm_bf16x3.hip
// One launch can carry several GEMM problems of the same operand layout and tile shape (the independent
// weight-gradient products of a backward pass): a workgroup finds its problem from the running block count.
// Every problem's block range starts at a multiple of 8, so (index inside the problem) % 8 still names the
// XCD group of common.h's tile order; the padding blocks exit at once.
#define GEMM_GROUP_MAX 16
struct GemmProb {
  const float* A; const float* B; float* C; float* slab;   // slab: split-K partials [gz][M][N] (null: write C)
  const float* bias;                                       // this problem's own bias (null: the launch's)
  int M, N, K, lda, ldb, ldc, k_chunk, gx, gy, nblocks;    // nblocks = gx*gy*gz; the launch gives it align8(nblocks)
};
struct GemmGroup { int n; int total_blocks; GemmProb p[GEMM_GROUP_MAX]; };
// score_gemm's flag bits (include/score_hip.h) as every GEMM kernel and the engine spell them; GF_X3F: bf16x3 forced (A/B);
// flags >> 16: the bias row group
enum { GF_BIAS = 1, GF_RELU = 2, GF_ACC = 4, GF_DROP = 8, GF_X3 = 16, GF_X3F = 32, GF_RELUGRAD = 64 };
// bias element of (row, col): one bias row, or one per group of g = flags >> 16 output rows
__device__ __forceinline__ int64_t bias_index(int flags, int row, int col, int N) {
  const int g = flags >> 16;
  return g ? (int64_t)(row / g) * N + col : col;
}
// what the f32 and the bf16x3 kernels do to an output element before they store it
__device__ __forceinline__ float gemm_epilogue(float v, int row, int col, int N, const float* bias, int flags,
                                               float keep, const uint8_t* mask, uint64_t seed) {
  if (flags & GF_BIAS) v += bias[bias_index(flags, row, col, N)];
  if (flags & GF_RELU) v = fmaxf(v, 0.f);
  if (flags & GF_DROP) {
    uint64_t e = (uint64_t)row * (uint64_t)N + (uint64_t)col;
    bool on = mask ? (mask[e] != 0) : (hash_uniform(seed, e) < keep);
    v = on ? v / keep : 0.f;  // tf.nn.dropout: x / keep_prob * binary mask
  }
  if (flags & GF_RELUGRAD) {   // backward of relu (+dropout): `mask` carries the layer's fp32 output Y [M,N]
    const float y = reinterpret_cast<const float*>(mask)[(int64_t)row * N + col];
    v = y > 0.f ? v / keep : 0.f;
  }
  return v;
}
int score_launch_gemm_bf16x3(int trans, int wm, const GemmGroup& g, const float* bias, int flags, float keep,
                             const uint8_t* mask, uint64_t seed, hipStream_t s);
// deferred weight-gradient products C = A^T . B (layout 2) of a backward pass: queued while the pass runs
// (their operands must stay untouched until the flush), then issued as one grouped launch per kernel family
// plus one launch that reduces every split-K slab.
struct GemmQueueJob { const float* A; const float* B; float* C; int M, N, K, lda, ldb, ldc; };
struct GemmQueue { int n; GemmQueueJob j[2 * GEMM_GROUP_MAX]; };
int gemm_queue_add(GemmQueue* q, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C,
                   int ldc);
// every split-K slab set of a flushed queue: C = sum_z slab[z]  (slab order); blocks = workgroups of 256 its reduce needs
struct ReduceJob { const float* slab; float* C; int ns, M, N, ldc, first_block, pad; };
struct ReduceGroup { int n; int blocks; ReduceJob j[2 * GEMM_GROUP_MAX]; };
// defer == nullptr: the slab reduce follows the products on `s`.  defer given: the products only; *defer describes the reduce
// the caller still owes (score_launch_finish, behind the products)
// with_colsums (+ cs_part): the queued column sums' FIRST stage runs in the same launch as the f32 products (*colsums_done = 1 if
// it did: score_launch_finish(..., stage1_done) then starts at the second stage)
struct ColsumJobs;
int gemm_queue_flush(GemmQueue* q, int x3, float* slab, int64_t slab_floats, hipStream_t s, ReduceGroup* defer = nullptr,
                     const ColsumJobs* with_colsums = nullptr, float* cs_part = nullptr, int64_t cs_part_floats = 0,
                     int* colsums_done = nullptr);
#define COLSUM_MAX_JOBS 24
#define COLSUM_MAX_PARTS 128
struct ColsumJob { const float* X; float* out; const float* scale; int M, N, ld, acc, cols, rpb, nparts; int64_t part_off; };
struct ColsumJobs { ColsumJob job[COLSUM_MAX_JOBS]; int n; int64_t part_used; };
// deferred column sums: queue jobs during a pass, run them all in two launches at its end.
// The queued X matrices must stay untouched until the flush.
// scale (optional, [M]): out[n] = sum_m scale[m] * X[m][n] -- a product X^T s with one output column, without a GEMM launch
int colsum_queue_add(ColsumJobs* q, const float* X, int M, int N, int ld, float* out, int acc, const float* scale = nullptr);
int colsum_queue_flush(ColsumJobs* q, float* part, int64_t part_floats, hipStream_t s);
// the end of a backward pass in TWO launches instead of four: the queued column sums' first stage, then ONE launch that is
// the deferred split-K slab reduce of gemm_queue_flush (rg, may be empty) AND the column sums' second stage -- the two are
// independent of each other, each workgroup does what its index says.  Same arithmetic, same order as the separate launches.
// w1: the folded first attention layer's gradient computed by the same launch from the dweff / dwq products' slabs
// (instead of score_launch_attn_w1_grad behind it); stage1_done: see gemm_queue_flush
struct W1Fold { int Dk, NA; const float* dweff; const float* dwq; float* gW1; const float* slab_e; const float* slab_q; int ns_e, ns_q; };
int score_launch_finish(const ReduceGroup* rg, ColsumJobs* q, float* part, int64_t part_floats, hipStream_t s, int stage1_done = 0,
                        const W1Fold* w1 = nullptr);
int score_launch_colsum(const float* X, int M, int N, int ld, float* out, int accumulate,
                        float* scratch, int64_t scratch_floats, hipStream_t s);
// embed.hip
struct CoattnCall {
  const int32_t* idx1; const int32_t* idx2;
  const float* tgt; int ldt;
  const int32_t* tidx;                        // forward, optional: the target's ids [B, F] -- the target rows are then read from
                                              // the table (the same bits as a gathered copy in tgt, which is not read)
  const float* W; const float* bias;
  float* out1; int ld1; float* out2; int ld2;
  float* info; int ldi; float* rsave;
  const float* g1; const float* g2; const float* ginfo;
  float* dzsum; float* slab;
  float* pcoef; float* dzcoef;                // backward, pull mode: softmax p_i and dz_i per (unit, i)
  int F, GS, nslots, first_block;
  int ksh;                                    // backward (set by the launcher): log2 of the neighbours per id register (embed.hip)
  int bit1, bit2;                             // bits of *CoattnArgs.id_status that name idx1 / idx2 (position in the feed tuple)
};
struct CoattnArgs {
  CoattnCall c[2];
  const float* table; float* gtable;
  int D4, K, T, n_units, mode;
  int Tidx;                                   // time stride of the index tensors ([B, Tidx, K, F]); 0 = T.  T = slices computed
  // ids outside [0, n_rows) (tf.nn.embedding_lookup raises there, score.py:51-66) are read as the dummy row 0 and
  // reported: bit1 / bit2 of the call OR-ed into *id_status (optional device word, score_state_t.id_status)
  uint32_t n_rows; int32_t* id_status;
  int all_rows;                               // backward, A/B (debug_flags bit 15): the rows of relu-inactive k are loaded too
  int meta_ahead;                             // backward, A/B (debug_flags bit 16): a unit's ids and saved scalars are requested one
                                              // unit ahead, not at the top of its own iteration
  int fwd_one_unit;                           // forward, A/B (debug_flags bit 17): coattn_fwd_kernel, one unit per wave, wherever
                                              // the launcher would take coattn_fwd_kernel_units
  int CH, cps, n_chunks;                      // forward (set by the launcher): time slices per chunk of coattn_fwd_kernel_units,
                                              // chunks per sample = ceil(T / CH), chunks per call = B * cps
};
int score_coattn_fwd_chunk_rule(int D, int K, int B, int T, int ncalls, const int* F);   // CH of a shape; 0: the one-unit kernel
int score_coattn_fwd_multi(CoattnArgs& a, int ncalls, int D, int B, hipStream_t s);
int score_coattn_bwd_multi(CoattnArgs& a, int ncalls, int D, int B, float* const dW[2], float* scratch,
                           int64_t scratch_floats, int atomic_scatter, ColsumJobs* cq, hipStream_t s);
int score_launch_target_fwd(const float* table, int D, int Fu, int Fi, int B, const int32_t* tu,
                            const int32_t* ti, float* query, int ldq, float* head, int ldh,
                            int off_ti, int off_tu, hipStream_t s, int64_t n_rows = 0, int32_t* id_status = nullptr);
int score_launch_target_bwd(float* grad_table, int D, int Fu, int Fi, int B, int T, const int32_t* tu,
                            const int32_t* ti, const float* dquery, int ldq, const float* dhead, int ldh,
                            int off_ti, int off_tu, const float* query, const float* W1, const float* W2,
                            const float* dzsum1, const float* dzsum2, float* S /*[2][B]*/,
                            float* dW1, float* dB1, float* dW2, float* dB2, float* dtgt_out, float* scratch,
                            int64_t scratch_floats, ColsumJobs* cq, struct GemmQueue* gq, hipStream_t s,
                            int64_t n_rows = 0);
// head.hip
int score_launch_attn_build_inp(int B, int T, int H, int NI, const float* q, const float* ur, const float* ir,
                                const float* info, float* inp, hipStream_t s);
int score_launch_attn_pool_fwd(int B, int T, int H, int NA, const float* a2, const float* w5, const float* b5,
                               const int32_t* length, const float* ur, const float* ir, float* score, float* head,
                               int ldh, int off_u, int off_i, hipStream_t s);
int score_launch_attn_tail_fwd(int B, int T, int H, int N1, int N2, const float* a1, const float* W4, const float* b4,
                               const float* w5, const float* b5, const int32_t* length, const float* ur, const float* ir,
                               float* a2, float* score, float* head, int ldh, int off_u, int off_i, hipStream_t s);
int score_launch_attn_pool_bwd(int B, int T, int H, int NA, const float* a2, const float* w5,
                               const int32_t* length, const float* ur, const float* ir, const float* score,
                               const float* dhead, int ldh, int off_u, int off_i, float* ds, float* da2,
                               hipStream_t s, int N1 = 0, const float* W4 = nullptr, const float* a1 = nullptr,
                               float* da1 = nullptr);
int score_launch_attn_inp_bwd(int B, int T, int H, int NI, const float* dinp, const float* q, const float* ur,
                              const float* ir, const float* info, const float* score, const float* dhead, int ldh,
                              int off_u, int off_i, const float* dqd, float* dur, float* dir, float* dinfo, float* dq,
                              hipStream_t s);
int score_launch_attn_inp_bwd_fused(int B, int T, int H, int NI, int N1, const float* da1, const float* Weff, const float* q,
                                    const float* ur, const float* ir, const float* info, const float* score,
                                    const float* dhead, int ldh, int off_u, int off_i, float* dur, float* dir, float* dinfo,
                                    float* dq, hipStream_t s, int N2 = 0, const float* a2 = nullptr, const float* a1 = nullptr,
                                    const float* w5 = nullptr, const float* W4 = nullptr, const int32_t* length = nullptr,
                                    float* ds = nullptr, float* da2 = nullptr, float* da1_out = nullptr);
bool score_attn_inp_bwd_fused_fits(int B, int T, int H, int NI, int N1, int N2, int ldh, int off_u, int off_i, bool pool);
#define SCORE_WEFF_COPIES 8       /* replicas of the folded attention weight (head.hip: attn_fold_w1_body) */
int score_launch_attn_dzsum(int B, int T, int NA, const float* dz, float* dzsum, hipStream_t s);
int score_launch_attn_w1_grad(int Dk, int NA, const float* dweff, const float* dwq, float* gW1, hipStream_t s);
int score_launch_bn_fwd(int B, int Dh, const float* x, const float* gamma, const float* beta, float rs, float* y,
                        hipStream_t s);
int score_launch_bn_bwd(int B, int Dh, const float* x, const float* gamma, float rs, const float* dy, float* dx,
                        float* dgamma, float* dbeta, float* tmp, float* scratch, int64_t scratch_floats,
                        ColsumJobs* cq, hipStream_t s);
// the per-step transforms of the weights in one launch: [Wx_gates | Wx_cand] copies, the folded first attention layer
// (W1 = null: none), the L2 partial sums
int score_launch_weight_prep(const float* gk0, const float* ck0, const float* gb0, const float* cb0, const float* gk1,
                             const float* ck1, const float* gb1, const float* cb1, int I0, int I1, int Imax, int H, float* cat,
                             int Dk, int NA, const float* W1, float* weff, float* wq, int copies, int64_t copy_stride,
                             const float* wreg, int64_t n_reg, float* part, hipStream_t s);
int score_launch_head_out(int B, int NF, const float* f2, const float* w3, const float* b3, const int32_t* label,
                          float* logit, float* y, float* lossb, float* dlogit, float* loss, float lambda,
                          const float* part, int Bglobal, hipStream_t s, const int32_t* id_status = nullptr);
int score_launch_loss_final(int B, const float* lossb, float* loss, float lambda, const float* part, int Bglobal,
                            hipStream_t s, const int32_t* id_status = nullptr);
// head_fused.hip: bn1 + fc1 + fc2 + fc3 + sigmoid + loss terms in one launch (SCORE_E_SHAPE: shape not covered)
int score_launch_head_fwd_fused(int B, int Dh, int N1, int N2, const float* x, const float* gamma, const float* beta,
                                float rs, const float* W1, const float* b1, const float* W2, const float* b2,
                                const float* W3, const float* b3, float keep, const uint8_t* mask0, const uint8_t* mask1,
                                uint64_t seed0, uint64_t seed1, const int32_t* label, float* bn, float* f1, float* f2,
                                float* logit, float* y, float* lossb, float* dlogit, int Bglobal, hipStream_t s,
                                const uint64_t* seed_dev = nullptr, float* dz2 = nullptr, int single_launch = 0);
bool score_head_fwd_fused_fits(int B, int Dh, int N1, int N2);
void score_head_forms_begin(int backward);      // score_forward (0) / score_backward (1) starts: clears its half of score_head_last_forms
int score_launch_head_bwd_fused(int B, int Dh, int N1, int N2, const float* dz2, const float* W2, const float* f1, float keep,
                                const float* W1, const float* x, const float* gamma, float rs, float* dz1, float* dbn,
                                float* dhead, float* tmp, hipStream_t s);
// head_fused.hip: attention input rows + dense_3 (folded) + dense_4 + dense_5 + masked softmax + pooling in one launch
int score_launch_attn_fwd_fused(int B, int T, int H, int NI, int N1, int N2, const float* q, const float* ur,
                                const float* ir, const float* info, const float* Weff, const float* qz, const float* W4,
                                const float* b4, const float* w5, const float* b5, const int32_t* length, float* inp,
                                float* a1, float* a2, float* score, float* head, int ldh, int off_u, int off_i,
                                hipStream_t s, int weff_copies = 1, int64_t weff_copy_stride = 0);
int score_launch_outer_relu_bwd(int B, int NF, const float* dlogit, const float* w, const float* f, float keep,
                                float* dz, hipStream_t s);
int score_launch_copy2d(int64_t rows, int cols, const float* src, int lds_, float* dst, int ldd, hipStream_t s);

// scatter.hip: occurrence sort ("index plan") and the pull-form gradient scatter
struct PlanFillArgs {
  const int32_t* idx[6];   // user_1hop, item_2hop, user_2hop, item_1hop, target_user, target_item
  int64_t off[7];          // prefix offsets of the six tensors in the occurrence space
  int F[6];
  int K, G, shift;         // G > 1: key = (row % G) << shift | row / G
  int T, TA;               // index tensors are [B, T, K, F]; only slices t < TA are enumerated (bt = b * TA + t)
  uint32_t n_rows;         // ids >= n_rows (feature_size) become the dummy row 0 and are reported in *id_status
  int32_t* id_status;      // optional device word (score_state_t.id_status)
};
struct PullArgs {
  const float* G[6]; int ldg[6]; int gcol[6];     // activation-gradient matrix per segment
  const float* cA[6]; const float* cB[6];         // per-(unit,k) scalars (null: constA / none)
  const float* Wv[6];                             // co-attention weight slice multiplied by cB
  float constA[6];
  const uint32_t* uid;     // null: a run's destination is its row id; else the run's unique position
  int D, K, LPRp;
  int zero_is_dummy;       // key 0 is the masked dummy row (score.py:44-47): no gradient
  uint8_t* flags;          // optional per-destination-row state byte: 2 = written this step
  // what the one-occurrence-per-lane form (pull_kernel_lanes) needs to bound its 32-bit offsets and to stage Wv: the
  // features and the G rows (bt values) of each segment.  All zero (a caller that does not know): the present kernel.
  int nf[6]; int64_t rows[6];
  int force_old;           // debug_flags bit 18: the present kernel whatever the geometry
};
struct PlanRemapArgs { int32_t* out[6]; int F[6]; int K; int T, TA; };
int score_launch_plan_unique(const PlanRemapArgs& ra, const uint32_t* keys, const uint32_t* vals, int64_t n,
                             uint32_t* flags_scratch, uint32_t* uid, uint32_t* unique_keys, int32_t* unique_rows,
                             int32_t* meta, int G, int shift, void* temp, size_t temp_bytes, hipStream_t s);
int score_scan_temp_bytes(int64_t n, size_t* bytes);
int score_plan_temp_bytes(int64_t n, int end_bit, size_t* bytes);
int score_launch_plan(const PlanFillArgs& a, int key_bits, uint32_t* keys_in, uint32_t* vals_in, uint32_t* keys_out,
                      uint32_t* vals_out, void* temp, size_t temp_bytes, hipStream_t s, int which = 0);
// sort.hip: the stable radix sort of the plan (small batches) and its scratch
int score_launch_plan_own(const PlanFillArgs& a, int key_bits, uint32_t* keys_in, uint32_t* vals_in, uint32_t* keys_out,
                          uint32_t* vals_out, void* temp, size_t temp_bytes, hipStream_t s);
size_t score_sort_temp_bytes(int64_t n);
int score_pull_window(int64_t n);
// Which pull kernel a launch takes.  pull_kernel_lanes<MODE, LPR, TU> (an occurrence's key, descriptor, coefficients and
// offsets on ONE lane of its group, handed out by DPP; 32-bit offsets from one base; Wv in LDS) when ALL of: the
// contribution form is 1 or 2 (not the owner-side row sum); D is 16, 32 or 64 (a group of D/4 lanes fills whole DPP
// banks of one 16-lane row); the caller gave nf[] / rows[] for all six segments; every byte the occurrences can reach
// in G / cA / cB lies below 4 GiB from the lowest of those pointers (score_pull_form); PullArgs.force_old is 0.
// Otherwise pull_kernel<MODE>.  Both forms give the same bits.
int score_launch_pull(PullArgs& a, const uint32_t* keys, const uint32_t* vals, int64_t n, float* out,
                      float* partials, int64_t partial_floats, hipStream_t s);

// gru.hip: both GRUs of the model in one launch
struct GruSide {
  const float* xproj;            // [B*T, 3H]  hoisted x.Wx + b
  const float* Wg; int ldwg;     // h-rows of gates/kernel     [H, 2H]
  const float* Wc; int ldwc;     // h-rows of candidate/kernel [H, H]
  float* out; int ldo;           // [B*T, H] h_t (0 past the length)
  float* gates;                  // [B*T, 3H] saved (r, u, c)
  float* final_state;            // [B, H] or null
  // backward
  const float* dout; int lddo;   // dL/d out
  const float* dfinal;           // dL/d final state or null
  float* dxproj;                 // [B*T, 3H] pre-activation grads
  float* rh;                     // [B*T, H] r * h_{t-1}
  float* hprev;                  // [B*T, H] h_{t-1}  (+ 3*H*H scratch floats at its end for the fallback)
  float* bias_slab;              // optional [workgroups of this side][3H]: column sums of the dxproj rows a workgroup wrote
                                 // (the bias gradients' partial sums; only kernels that report GruArgs.bias_slab_rows fill it)
  const int32_t* length;         // optional [B]: this side's own sequence lengths (null: GruArgs.length).  Honoured by the register
                                 // kernels of gru.hip only (score_gru_reg_route); every other recurrence takes GruArgs.length
};
struct GruArgs {
  GruSide s[2];
  const int32_t* length;
  int B, T, H;
  int nw8;      // H = 128: 8 waves per workgroup (2 per SIMD) instead of 4
  // hidden sizes without a register-resident kernel: H = 256 streams its weights from L2 (gru_stream.hip; scratch
  // = score_gru_stream_tmp_floats); others run the recurrence step by step (two grouped GEMMs + two pointwise
  // launches per time slice; scratch 10 * B * H floats), x3 = bf16x3 allowed there.  stepwise != 0 forces that path (A/B)
  float* tmp; int64_t tmp_floats; int x3; int stepwise;
  int x3_rec;   // H = 128: the recurrence itself on the bf16 matrix cores, fp32-accurate (gru_x3.hip)
  int bias_slab_rows;   // out (backward): rows of GruSide.bias_slab written per side, 0 if the kernel that ran does not
};
// nprob same-shape GEMMs C_i = op(A_i) op(B_i) in one launch (the two sides of a recurrence step); flags: 4 = C += .
int score_gemm_same_shape(int trans, int nprob, int M, int N, int K, const float* const* A, int lda,
                          const float* const* B, int ldb, float* const* C, int ldc, int flags, int x3, float* scratch,
                          int64_t scratch_floats, hipStream_t s, const float* const* bias = nullptr);   // flags: 1 = + bias[i][N]
// gemm_panel.hip: bf16x3 products C = A . Bt^T (+ bias) with a whole-N output panel per workgroup (the GRU input projections
// and their input gradients at cfg-3's sizes): A is read once, the weights come as fragment images written once per step
struct PanelGroup { const float* A; const float* img; float* C; const float* bias; };
bool score_gemm_panel_ok(int ngroups, int M, int N, int K, int lda, int ldc, int* mt_out);      // false: use the tiled kernels
int64_t score_gemm_panel_image_floats(int N, int K);                                          // 0: shape not covered
// images of nimg weight matrices of one shape; Bt(n, k) = trans ? B[k * ldb + n] : B[n * ldb + k]
int score_gemm_panel_prep(int nimg, const float* const* B, int ldb, int trans, int N, int K, float* const* img, hipStream_t s);
int score_gemm_panel(int ngroups, const PanelGroup* g, int M, int N, int K, int lda, int ldc, hipStream_t s);
// gru_stream.hip: H = 256 (weights streamed from L2 in MFMA fragment order; tmp holds the fragment copies)
bool score_gru_stream_ok(int H);
int64_t score_gru_stream_tmp_floats(int H, int nsides);
int score_gru_fwd_stream(GruArgs& a, int nsides, hipStream_t s);
int score_gru_bwd_stream(GruArgs& a, int nsides, hipStream_t s);
// gru_x3.hip: H = 128 recurrences as bf16x3 products (weights resident in registers as split planes)
bool score_gru_x3_ok(int H, int nw8);
int score_gru_fwd_x3(GruArgs& a, int nsides, hipStream_t s);
int score_gru_bwd_x3(GruArgs& a, int nsides, hipStream_t s);
int score_gru_fwd_multi(GruArgs& a, int nsides, hipStream_t s);
int score_gru_bwd_multi(GruArgs& a, int nsides, hipStream_t s);
// do score_gru_*_multi run these arguments on the register kernels of gru.hip (H in {16, 32, 64, 128} and not the bf16x3 route)?
// Only then does a side's own GruSide.length count
bool score_gru_reg_route(const GruArgs& a, int nsides);
// gcmc.hip: the GCMC slice baseline's bilinear two-way softmax head (slice_model.py:199-201), H <= 256.  Forward: y, the
// per-sample log-loss term, and p = h_i W4, n = h_i W5, g = dL/da saved for the backward; backward: dh_u, dh_i and the rows
// gpos = g h_u, gneg = -g h_u of the dense gradients dW4 = h_i^T gpos, dW5 = h_i^T gneg
int score_launch_gcmc_head_fwd(int B, int H, const float* hu, const float* hi, const float* W4, const float* W5,
                               const int32_t* label, float* y, float* lossb, float* p, float* n, float* g, int Bglobal,
                               hipStream_t s);
int score_launch_gcmc_head_bwd(int B, int H, const float* hu, const float* W4, const float* W5, const float* p, const float* n,
                               const float* g, float* dhu, float* dhi, float* gpos, float* gneg, hipStream_t s);
// gru_stack.hip: GRU4Rec's two GRUs stacked in depth (point_model.py:129-132) as ONE persistent kernel each way, H in
// {16, 32, 64}.  l[0] = layer 1 as for score_gru_*_multi (xproj hoisted; Wg / Wc the h rows of its kernels), l[1] = layer 2's
// saved regions only: its input is layer 1's state, handed over in LDS one step later, against the WHOLE kernels Wg2 [2H, 2H] /
// Wc2 [2H, H] (TF's [x, h] row order) and the biases bg2 [2H] / bc2 [H] -- no projection buffer, no GEMM, no launch boundary.
// Backward: l[1].dfinal = dL/d layer 2's final state; layer 2's input gradient reaches layer 1 through LDS; both layers'
// dxproj / rh / hprev rows are written as score_gru_bwd_multi writes them.
struct GruStackArgs {
  GruSide l[2];
  const float* Wg2; const float* Wc2; const float* bg2; const float* bc2;
  const int32_t* length;
  int B, T, H;
};
bool score_gru_stack_ok(int H);
int score_gru_stack_fwd(GruStackArgs& a, hipStream_t s);
int score_gru_stack_bwd(GruStackArgs& a, hipStream_t s);
// caser.hip: the Caser point baseline's two one-filter convolutions (point_model.py:147-160) over X [B, T, C] (rows of stride
// ldx).  Forward, one launch: hwin[b, p] = sum_{i < 50, c} X[b, p + i, c] Wh[i, c] + bh, h = max_p hwin (arg: its first position),
// v[b, c] = sum_t X[b, t, c] Wv[t] + bv, v2 = v wd + bd; head row b (stride ldh) <- [h, 0, 0, 0 | v2].  Backward, two launches:
// dX (every one of its ldx columns: zeros past C) on `s`; the six variables' gradients, summed over the batch in a fixed order,
// on `sp` -- they read dhead, X, arg and v only, so the two may run side by side.
#define SCORE_CASER_L 50          /* conv2d's kernel height: the reference's constant, not max_time_len */
#define SCORE_CASER_HPAD 4        /* h's place in the head input, padded to one 16-byte group */
struct CaserArgs {
  int B, T, C, ldx, ldh;
  const float* X; const float* Wh; const float* bh; const float* Wv; const float* bv; const float* wd; const float* bd;
  float* head; float* hwin; int32_t* arg; float* v;
  const float* dhead; float* dX;
  float* gWh; float* gbh; float* gWv; float* gbv; float* gwd; float* gbd;
};
int score_caser_fwd(const CaserArgs& a, hipStream_t s);
int score_caser_bwd(const CaserArgs& a, hipStream_t s, hipStream_t sp);
// rank.hip: the bn1 / fc1 / fc2 / fc3 head of the point baselines over L target lines of C candidates (score_rank_forward).
// head: the lines' head input rows [L, Dh] -- every column but the item's [off_ti, off_ti + Di) is the line's own.  Two launches:
// zline[l, :N1] = b1 + bn1(head[l]) . W1 over the line's columns (a workgroup per line), then a workgroup per (line, 16
// candidates): the candidates' table rows -> bn1 -> LDS, relu(zline[l] + x . W1[item rows]), fc2, fc3, sigmoid;
// y / lossb [L * C] at l * C + c.  Ids >= n_rows are read as row 0 and reported as bit 5 of *id_status.
struct RankArgs {
  int L, C, Dh, off_ti, Di, D, N1, N2;
  const float* head; const float* table; const int32_t* cand; const int32_t* label;
  const float* gamma; const float* beta; float rs;
  const float* W1; const float* b1; const float* W2; const float* b2; const float* W3; const float* b3;
  float* zline; float* y; float* lossb;
  uint32_t n_rows; int32_t* id_status;
};
bool score_rank_head_fits(int L, int C, int Dh, int off_ti, int Di, int D, int N1, int N2);
int score_rank_head(const RankArgs& a, hipStream_t s);
int score_rank_line(const RankArgs& a, hipStream_t s);       // the line kernel alone (zline; a.C is not read): the catalogue pass
// catalog.hip: top-K over a whole item catalogue (score_catalog_build / score_catalog_topk).  fc1's pre-activation of the pair
// (line l, catalogue item n) is zline[l] + zcat[n]; zcat [N, 200] = bn1(item_n) . W1[item rows] is a per-catalogue constant.
// score_catalog_zcat fills it (a workgroup per 16 items; ids >= n_rows read as row 0, bit 5 of *id_status).
// score_catalog_sweep, selecting: a workgroup per (line, chunk of the catalogue) holds fc2 / fc3 resident, walks its chunk and keeps its k
// best pairs -- ordered by (logit descending, index ascending; NaN behind every number) as 64-bit keys, see catalog.hip -- in
// part [L, nchunk, k]; then a workgroup per line merges the nchunk lists into top_idx / top_logit [L, k] (-1 / -inf padding).
// excl_off / excl_idx (optional): per line, ascending catalogue indices that are never selected.  all_logits (optional) [L, N].
// Fixed head widths: fc1 = 200, fc2 = 80 outputs.
struct CatalogArgs {
  int L, N, k, chunk, nchunk;
  int Di, D, off_ti, N1;                 // the item columns [off_ti, off_ti + Di) of the head input; N1 = 200
  const float* table; const int32_t* item_rows;
  const float* gamma; const float* beta; float rs;
  const float* W1; const float* W2; const float* b2; const float* W3; const float* b3;
  float* zcat; const float* zline;
  const int64_t* excl_off; const int32_t* excl_idx;
  unsigned long long* part;
  int32_t* top_idx; float* top_logit; float* all_logits;
  uint32_t n_rows; int32_t* id_status;
  // the candidate form (score_catalog_sweep, cand): per line the catalogue indices cand_idx[cand_off[l] .. cand_off[l + 1]),
  // strictly ascending; chunk / nchunk cut max_count list POSITIONS, all_logits is aligned with cand_idx
  const int64_t* cand_off; const int32_t* cand_idx; int max_count;
  // the counting form (score_catalog_sweep, ranks; score_catalog_ranks*): per line the targets
  // tgt_idx[tgt_off[l] .. tgt_off[l + 1]), the first max_targets of them counted; rpart [L, nchunk, SCORE_CATALOG_RPART] the
  // chunks' integer partials; ahead / tgt_logit / state aligned with tgt_idx, n_scored [L].  (Behind every field the top-K
  // kernels read, so that their argument offsets stay where they were.)
  const int64_t* tgt_off; const int32_t* tgt_idx; int max_targets;
  int32_t* rpart; int32_t* ahead; float* tgt_logit; int32_t* state; int32_t* n_scored;
};
// a chunk's partials of the counting form, int32: 32 counts of pairs ahead, 32 hit flags (1: the target was met and counted,
// 2: met and excluded), the number of pairs counted; padded to a multiple of 16 bytes
constexpr int SCORE_CATALOG_RPART = 68;
void score_catalog_chunks(int L, int N, int k, int* chunk, int* nchunk);
int score_catalog_zcat(const CatalogArgs& a, hipStream_t s);
// the sweep and its second launch.  cand: the lines' candidate lists (plan of a.max_count), else the whole catalogue (plan of a.N);
// ranks: the counting form, else the selecting one
int score_catalog_sweep(const CatalogArgs& a, bool cand, bool ranks, hipStream_t s);
// delf.hip: the DELF point baseline (point_model.py:200-249) between the gather and the scatter.  Per side (0: user_seq rows
// against target_item through dense; 1: item_seq rows against target_user through dense_1) X [B * T, C] with row stride ldx,
// the saved keys [B * T, C] (live rows only), attention weights att [B, T], rep [B, C]; backward: ds [B, T] (gradient at the
// scores), dX (every one of the ldx columns written) and dpre [B * T, C] (gradient at tanh's argument; zero rows past the
// length).  act [B, SCORE_DELF_ACT] = [h1 of the four fusion MLPs (40) | h2 (16) | f (4) | pad], dact the same layout with the
// gradients at the pre-activations (f's slots unused).  tu / ti: the gathered target rows (row stride ldq); dhead (stride ldh)
// receives d target_item at off_ti and d target_user at off_tu.  One launch each way, a workgroup per sample.
#define SCORE_DELF_CMAX 128       /* widest Fu * D / Fi * D the kernels cover */
#define SCORE_DELF_ACT 64
struct DelfSide {
  const float* X; const float* W; const float* b; const int32_t* len;
  float* key; float* att; float* rep; float* ds; float* dX; float* dpre;
  int C, ldx;
};
struct DelfArgs {
  DelfSide s[2];
  const float* tu; const float* ti;
  const float* A[4]; const float* a1[4]; const float* Bm[4]; const float* b2[4]; const float* w; const float* c;
  const int32_t* label;
  float* act; float* dact; float* logit; float* y; float* lossb; float* dlogit; float* dhead;
  int B, T, Cu, Ci, ldq, ldh, off_ti, off_tu, Bglobal;
};
int score_delf_fwd(const DelfArgs& a, hipStream_t s);
int score_delf_bwd(const DelfArgs& a, hipStream_t s);
// deems.hip: the DEEMS point baseline's two build_fc_net towers (point_model.py:292-311).  x [B, ld] holds both head inputs as
// column ranges of one row, [h_u | target_user | h_i | target_item]: tower k owns columns [col, col + Dh), the first H of them the
// final state of its recurrence (h: where the recurrence left it, [B, H]; the forward kernels store it into x on the way; null: x
// holds it already).  bn, dbn, dhead and tmp (bn's d gamma terms) are laid out as x; f1 / f2 / dz1 / dz2 / logit / y / dlogit are
// per tower.  mask0 [B, 200] / mask1 [B, 80]: this tower's explicit dropout masks or null (then from seed0, or *seed_dev; the item
// tower's stream is the user tower's seed ^ SCORE_DEEMS_ITEM_SEED).  lossb: log-loss term + 0.05 (y_i - y_u)^2 * Bglobal, so that
// the mean the loss reduction takes gives mean(log-loss) + SUM(consistency); dlogit: of the log-loss alone.
#define SCORE_DEEMS_ITEM_SEED 0xD1B54A32D192ED03ull
struct DeemsTower {
  const float* h;
  const float* gamma; const float* beta;
  const float* W1; const float* b1; const float* W2; const float* b2; const float* W3; const float* b3;
  const uint8_t* mask0; const uint8_t* mask1;
  float* f1; float* f2; float* dz2; float* dz1; float* logit; float* y; float* dlogit;
  int Dh, col;
};
struct DeemsArgs {
  DeemsTower t[2];       // 0: user tower, 1: item tower
  int B, H, ld, Bglobal;
  float* x; float* bn; float* dbn; float* dhead; float* tmp;
  float rs, keep; uint64_t seed0; const uint64_t* seed_dev;
  const int32_t* label; float* y_pred; float* lossb;
};
bool score_deems_head_fwd_fits(int Dh_user, int Dh_item);
int score_deems_head_fwd(const DeemsArgs& a, hipStream_t s);      // everything in one launch; SCORE_E_SHAPE: does not fit
int score_deems_bn_fwd(const DeemsArgs& a, hipStream_t s);        // the layer-by-layer form: both towers' bn ...
int score_deems_out(const DeemsArgs& a, hipStream_t s);           // ... and, from the two logits, y / lossb / dlogit
int score_deems_head_bwd(const DeemsArgs& a, hipStream_t s);      // both towers' head backward in one launch (from dz2)
int score_deems_bn_bwd(const DeemsArgs& a, hipStream_t s);        // the layer-by-layer form's bn backward, both towers
// svdpp.hip: the SVD++ point baseline (point_models/point_model.py:167-198) between the gather and the scatter.  X [B * T, ldx]:
// the gathered user_seq rows, Fi * D columns read; tu / ti: the gathered target rows (row stride ldq); wu / wi: the scalar
// weights, one per 4-float cell (wu[4 i], wi[4 j]).  act [B, 4 D + 4] = [p_u | p_i | nb | share | n, ties, 0, 0] is what the
// forward kernel saves (share_d = [c_d == n] / ties); s_t is recomputed from X in the backward kernel, which writes dX (every one
// of the ldx columns; an exact 0 past the length), d target_item / d target_user into dhead (row stride ldh) and the per-sample
// weight-gradient partials dwpart [B, Fu + Fi] (user weights first).  One launch each way, a workgroup per sample.
#define SCORE_SVDPP_DMAX 128      /* widest eb_dim the kernels cover */
#define SCORE_SVDPP_FMAX 8        /* most feature fields per side (the index plan's limit too) */
struct SvdppArgs {
  const float* X; const float* tu; const float* ti; const float* wu; const float* wi;
  const int32_t* length; const int32_t* label;
  float* act; float* logit; float* y; float* lossb; float* dlogit;
  float* dX; float* dhead; float* dwpart;
  int B, T, D, Fu, Fi, ldx, ldq, ldh, off_ti, off_tu, Bglobal;
};
__host__ __device__ static inline int64_t score_svdpp_act_floats(int D) { return 4 * (int64_t)D + 4; }
int score_svdpp_fwd(const SvdppArgs& a, hipStream_t s);
int score_svdpp_bwd(const SvdppArgs& a, hipStream_t s);
// sasrec.hip: the SASRec point baseline (point_models/point_model.py:313-469) between the gather and the scatter.  X [B * T, ldx]:
// the gathered user_seq rows, C = Fi * D columns read; tu / ti: the gathered target rows (row stride ldq).  The attention's
// forward kernel saves, per (b, t) row, N (nrm), 1 / sqrt(var + eps) (rstd), the key mask (km), Qin, Q, K, V and Y (yseq)
// [B * T, C], per sample the softmax P and the final weights att = dropout(P * query mask) [B, 2, T, T] and final [B, C], and
// writes the head-input rows hin [B (T - 1) + B, Dh = 2 C + Cu]: [rep_t | Y_t | tu] for t = 1 .. T - 1 (b-major), then
// [final | ti | tu].  The shared head runs fc1 ONCE over those rows (z1, the engine's GEMM); from there on the rows are
// positive (b-major, t = 1 .. T - 1), negative (t = 2 .. T - 1), final -- R of them: f1 = dropout(relu(z1)) fanned out
// (score_sasrec_fan), z2 (GEMM), then f2, the logits, y, the loss terms, dlogit and dz2 (score_sasrec_out).  share != 0
// (keep_prob = 1): no negative rows, their terms ride on the positive rows t >= 2.  Backward: dz1e [R, 200] (GEMM) folded back
// onto the rows of z1 (score_sasrec_fold), dhin (GEMM), then score_sasrec_attn_bwd: dQ / dK / dV [B * T, C], dX (every one of the
// ldx columns), per-sample dgamma / dbeta [B, C], d target_item / d target_user into dhead (row stride ldh).
// mask0 [R, 200] / mask1 [R, 80] / mask_a [2, B, T, T]: explicit dropout masks or null (then from seed, or *seed_dev).
#define SCORE_SASREC_CMAX 128     /* widest Fi * D the kernels cover */
struct SasrecArgs {
  const float* X; const float* tu; const float* ti;
  const float* beta; const float* gamma; const float* Wq; const float* bq; const float* Wk; const float* bk; const float* Wv; const float* bv;
  const float* W3; const float* b3;
  const int32_t* length; const int32_t* label;
  const uint8_t* mask0; const uint8_t* mask1; const uint8_t* mask_a;
  float keep; uint64_t seed; const uint64_t* seed_dev;
  float* nrm; float* rstd; float* km; float* qin; float* q; float* k; float* v; float* yseq; float* p; float* att; float* fin; float* hin;
  float* z1; float* f1; float* z2; float* f2; float* rlogit; float* dlogit; float* dz2; float* dz1e; float* dz1; float* dhin;
  float* logit; float* ypred; float* lossb;
  float* dq; float* dk; float* dv; float* dX; float* dhead; float* dgamma; float* dbeta;
  int B, T, C, Cu, Dh, ldx, ldq, ldh, off_ti, off_tu, Bglobal, share;
};
bool score_sasrec_fits(int T, int C);                             // T >= 3, C <= SCORE_SASREC_CMAX, a sample's buffers inside 160 KiB of LDS
int score_sasrec_attn_fwd(const SasrecArgs& a, hipStream_t s);
int score_sasrec_fan(const SasrecArgs& a, hipStream_t s);
int score_sasrec_out(const SasrecArgs& a, hipStream_t s);
int score_sasrec_fold(const SasrecArgs& a, hipStream_t s);
int score_sasrec_attn_bwd(const SasrecArgs& a, hipStream_t s);
