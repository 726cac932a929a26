/*
 * score_hip.h -- C-ABI of libscore_hip.so: the MI355X (gfx950) implementation of
 * the SCoRe forward/backward hot path (reference: qinjr/SCoRe code/score/score.py).
 *
 * The reference is pure Python on TensorFlow 1.x and has no FFI of its own
 * ("Native components: NONE"); what a reference maintainer
 * binds instead of `sess.run(...)` is this header (INTEGRATION.md shows the
 * ctypes stub).  Each entry point cites the reference lines it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch tensors in
 *     this repo); the library never allocates, frees or retains device memory;
 *   - sizes are int64_t / int32_t, `stream` is a hipStream_t passed as void*;
 *   - return value: 0 = ok, >0 = hipError_t, <0 = SCORE_E_* argument error;
 *   - state between calls: none, except the side stream + three events that score_forward/backward fork
 *     independent work onto.  They live in a score_context_t the caller creates, passes in
 *     score_state_t.context and destroys; calls with DIFFERENT contexts are re-entrant across streams and
 *     host threads.  A NULL context selects one process-wide default context per device (created on
 *     first use under a mutex, released by score_context_destroy(NULL)): calls sharing it must not
 *     overlap in time.  The library reads no environment variable (A/B switches: score_state_t.debug_flags);
 *   - all arithmetic is fp32, all indices int32 (score.py:21-30 placeholders);
 *   - table row 0 is the dummy node and must be all-zero in `table`
 *     (score.py:44-47 emb_mtx * mask): kernels rely on it and never update it.
 */
#ifndef SCORE_HIP_H
#define SCORE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCORE_E_BADARG   (-1)  /* null pointer / non-positive size               */
#define SCORE_E_SHAPE    (-2)  /* shape outside what the kernels are built for   */
#define SCORE_E_WORKSPACE (-3) /* workspace too small                            */
#define SCORE_E_INDEX    (-4)  /* a feature id outside [0, feature_size) was fed (score_id_status) */

/* Per-caller resources of the whole-path entry points (one non-blocking HIP stream + three events on the
 * current device).  Replaces nothing in the reference: it is what `tf.Session` owns there (train_score.py:188). */
typedef void* score_context_t;
int score_context_create(score_context_t* ctx);
/* ctx == NULL: release the process-wide default contexts.  Synchronises the context's stream first. */
int score_context_destroy(score_context_t ctx);
/* Events for stream-to-stream ordering ONLY (round 6): hipEventDisableTiming | hipEventDisableSystemFence -- recording one does
 * not write back / invalidate the caches at system scope, which an event made for the host's eyes does on every record (a dozen
 * records per training step sit between dependent kernels of the launch stream).  What they order is device work on device
 * memory; a host thread that wants to READ results behind such an event must use an ordinary event (or synchronise the stream).
 * The context's own fork / join events are of this kind.  score_event_record / score_stream_wait_event take any hipEvent_t.
 * Replaces nothing in the reference. */
int score_event_create(void** event);
int score_event_destroy(void* event);
int score_event_record(void* event, void* stream);
int score_stream_wait_event(void* stream, void* event);
int score_event_query(void* event);          /* 0 = reached, 1 = not yet, else an error */
int score_event_synchronize(void* event);

/* The scalars of a training step that change from step to step, kept in DEVICE memory so that a captured step
 * (hipGraph: small shapes are launch-bound, ~60 launches of a few microseconds each) can be replayed with new
 * values: ApplyAdam's alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t) (score.py:96-99) and the seed of the
 * step's dropout masks (score.py:71,73).  The caller rewrites them (one 16-byte copy) before every step. */
typedef struct {
  float    adam_alpha;
  uint32_t reserved;
  uint64_t drop_seed;
} score_step_scalars_t;

/* model_type values (train_score.py:170-179 selects the class by name) */
enum { SCORE_MODEL_SCORE = 0, SCORE_MODEL_RIA = 1, SCORE_MODEL_RCA = 2,
       SCORE_MODEL_SCORE_USER = 3, SCORE_MODEL_SCORE_ITEM = 4,
       SCORE_MODEL_RRN = 5 /* slice_models/slice_model.py:155-174: summed 1-hop sets -> GRUs -> head */,
       /* slice_models/slice_model.py:177-203: summed 1-hop sets -> two relu denses per side -> GRUs -> bilinear two-way
        * softmax of the final states.  Its arithmetic reads user_1hop and item_1hop only; the other four index tensors are
        * still read and checked for ids outside the table (their rows get a zero gradient), as for RRN. */
       SCORE_MODEL_GCMC = 6,
       /* point_models/point_model.py:9-138 (GRU4Rec): the flat user history through two GRUs stacked in depth (gru1 -> gru2,
        * :129-132), layer 2's final state + the target rows -> the same bn1 / fc head, log-loss and L2 filter.  obj_per_time_slice
        * must be 1.  The batch rides in score_batch_t: user_1hop = user_seq seen as [B,T,1,Fi], length = user_seq_length (values
        * above T behave as T), target_user / target_item / label as they are.  user_2hop, item_1hop and item_2hop do not exist in
        * this model: the caller passes zero-filled tensors of their shapes (row 0 is the masked row: no arithmetic, no gradient);
        * they are still enumerated by the index plan.  Workspace pairs (score_workspace_field: gru_out, gates, xproj, dxproj, rh,
        * hprev): index 0 = layer 1, 1 = layer 2.  At H in {16, 32, 64} the two recurrences run as ONE kernel each way
        * (csrc/gru_stack.hip: layer 2 one step behind layer 1, its input handed over in LDS); other H, and debug_flags bit 13,
        * run them one layer per launch with the projection GEMM between them. */
       SCORE_MODEL_GRU4REC = 7,
       /* point_models/point_model.py:140-164 (Caser): two one-filter convolutions over the flat user history X [T, C],
        * C = item_fnum * eb_dim -- the horizontal one ([50, C], VALID, max over the T - 49 positions: one scalar h per sample; 50
        * is the reference's constant, so max_time_len >= 50) and the vertical one ([T, 1]: v [C]) followed by a dense on a
        * trailing axis of size 1 (one scalar weight and bias: v2 = v wd + bd) -- then [h | v2 | target_item | target_user]
        * through the same bn1 / fc head, log-loss and L2 filter.  hidden_size is accepted and ignored, obj_per_time_slice must
        * be 1, and the batch rides in score_batch_t as for SCORE_MODEL_GRU4REC, except that length is NOT read (the reference's
        * graph does not use user_seq_length: every one of the T positions is computed and gets gradient; active_slices is
        * ignored too).  The head input is held padded to a multiple of four floats, [h, 0, 0, 0 | v2 | target_item |
        * target_user]: bn1/gamma, bn1/beta and fc1/kernel have 4 + 2 Di + Du rows in score_param_layout, rows 1..3 being pad
        * rows that the caller initialises to zero and that training then leaves at zero (zero gradient, zero L2 term, zero
        * Adam update); the variables TF has are the rows 0, 4, 5, ...  conv2d/kernel is [50, C], conv2d_1/kernel [T, 1],
        * dense/kernel [1, 1].  Workspace fields (score_workspace_field): caser_hwin [B, T - 49] the window sums + bias,
        * caser_arg [B] (int32) the first position of the maximum, caser_v [B, C] v before the scalar dense.  Kernels:
        * csrc/caser.hip. */
       SCORE_MODEL_CASER = 8,
       /* point_models/point_model.py:200-249 (DELF) on PointBaseModel (:9-63): two histories -- user_seq [B, T, Fi] (the items of
        * the target user) and item_seq [B, T, Fu] (the users of the target item), each with its own length -- through a masked,
        * target-conditioned attention: key_t = tanh(X_t W + b) (dense [Ci, Ci] on user_seq, dense_1 [Cu, Cu] on item_seq; Ci =
        * item_fnum * eb_dim, Cu = user_fnum * eb_dim), s_t = <q, key_t> for t < length and -2^32 + 1 past it, a = softmax_t(s),
        * rep = sum_t a_t X_t (the value is X, not the key); q = target_item for user_seq (-> ru) and target_user for item_seq
        * (-> ri).  Then four fusion MLPs relu(relu(. A + a) B + b), 10 and 4 wide, over [tu|ti], [ru|ri], [tu|ri], [ti|ru]
        * (dense_2 .. dense_9), their sum f, y = sigmoid(f w + c) (dense_10), log-loss, and the L2 filter over all eleven kernels.
        * No bn1 / fc head, no dropout (keep_prob has no effect), hidden_size accepted and ignored, obj_per_time_slice must be 1,
        * Ci and Cu <= 128 (SCORE_E_SHAPE beyond).  The batch: user_1hop = user_seq as [B, T, 1, Fi], item_1hop = item_seq as
        * [B, T, 1, Fu], user_2hop / item_2hop zeros, length = user_seq_length, length2 = item_seq_length; a length >= T means all
        * T positions, a length <= 0 masks every position (then a = 1 / T over all T: tf.sequence_mask + softmax).  active_slices =
        * A promises BOTH lengths <= A (and no length <= 0, whose sample reads all T rows).  Workspace fields
        * (score_workspace_field, each a per-side pair): delf_key [B*T, C] tanh keys (live rows), delf_att [B, T] attention weights,
        * delf_rep [B, C] ru / ri, delf_ds [B, T] and delf_dpre [B*T, C] the gradients at the scores and at tanh's argument;
        * delf_act / delf_dact [B, 64]: [h1 (4 x 10) | h2 (4 x 4) | f (4) | pad] and the pre-activation gradients.  Kernels:
        * csrc/delf.hip, one launch each way. */
       SCORE_MODEL_DELF = 9,
       /* point_models/point_model.py:281-311 (DEEMS) on DELF (:200-249) on PointBaseModel (:9-63): h_u = the final state of gru1
        * over user_seq under user_seq_length, h_i = that of gru2 over item_seq under item_seq_length (GRUCell(hidden_size),
        * dynamic_rnn: the state frozen past the length, a length >= T all T positions, a length <= 0 a zero final state), then two
        * build_fc_net towers (bn in inference form, fc 200 relu dropout, fc 80 relu dropout, fc 1, sigmoid) with variables and
        * dropout masks of their own: y_u on [h_u | target_user], y_i on [h_i | target_item]; y_pred = (y_u + y_i) / 2.  The
        * reference builds train_step from log_loss(label, y_pred) + reg_lambda * l2 and only then adds 0.05 * SUM_b (y_i - y_u)^2
        * to self.loss (:299-300): loss[0] / loss[1] INCLUDE that term (a sum over the batch, not a mean), the gradients do NOT.
        * DELF's constructor runs first, so its 22 variables exist: they are laid out, initialised, regularised (their kernels
        * add to the L2 term and get reg_lambda * W through score_adam; their biases never change) and never read by a launch --
        * the DELF kernels do not run.  score_param_layout: 46 entries in TF's creation order -- dense .. dense_10, gru1 / gru2,
        * batch_normalization/{gamma, beta}, dense_11 .. dense_13 (user tower), batch_normalization_1/{gamma, beta}, dense_14 ..
        * dense_16 (item tower).  obj_per_time_slice must be 1, hidden_size a multiple of 4.  The batch rides as for
        * SCORE_MODEL_DELF (user_1hop = user_seq, item_1hop = item_seq, length, length2); active_slices = A promises both lengths
        * <= A, and -- unlike DELF -- a length <= 0 does not ask for all T slices: that sample's recurrence never runs.
        * score_forward's drop_mask0 / drop_mask1 cover both towers, the user tower first: [2, B, 200] and [2, B, 80]; from a seed
        * the item tower draws from a stream of its own (the user tower's seeds ^ a constant).  The head input is ONE row
        * [h_u | target_user | h_i | target_item] (score_workspace_t.head_inp, 2 H + Du + Di wide); workspace fields
        * (score_workspace_field): gru_final = h_u | h_i, deems_y = y_u | y_i [B] each, deems_logit, deems_dlogit likewise,
        * deems_f1 / deems_f2 / deems_dz1 / deems_dz2 the towers' layer outputs and their gradients.  At H in {16, 32, 64, 128}
        * (128: with gemm_mode 0 or debug_flags bit 2) both recurrences run as ONE launch each way, each side under its own lengths;
        * other H, and debug_flags bit 13, run one launch per side.  Both towers and the loss terms are ONE launch each way
        * (csrc/deems.hip); debug_flags bit 6 runs them layer by layer. */
       SCORE_MODEL_DEEMS = 10,
       /* point_models/point_model.py:167-198 (SVDpp) on PointBaseModel (:9-63): the matrix-factorisation baseline.  One scalar
        * weight per feature field; per sample p_u = sum_i wu_i E(target_user[i]), p_i = sum_j wi_j E(target_item[j]),
        * s_t = [t < length] sum_j wi_j E(user_seq[t][j]) (tf.sequence_mask: a length >= T means all T positions), nb = sum_t s_t,
        * n = tf.norm(s, 1, (1, 2)) -- the MATRIX 1-norm: max over the D columns of sum_t |s_t,d| --, q = nb / sqrt(n),
        * y_pred = sigmoid(<p_i, p_u + q>), tf.losses.log_loss + reg_lambda * sum w^2 / 2 over the scalars (emb_mtx is not
        * regularised).  No bn, no fc head, no dropout (keep_prob has no effect); hidden_size is accepted and ignored.  The
        * gradient of the maximum is shared equally among the columns that attain it (reduce_max), sign(0) = 0.  A sample whose
        * length is <= 0 or whose live history rows are all id 0 has n = 0 and nb = 0: q = 0 / 0, so its y_pred and the batch
        * loss are NaN, as in TF (the reference's loader yields no such sample); nothing special-cases it.
        * score_param_layout: Fu + Fi entries in TF's creation order, user_feat_w_0 .. user_feat_w_{Fu-1}, item_feat_w_0 ..
        * item_feat_w_{Fi-1}, each rows = 1, cols = 0, regularised, init 4.  Offsets stay multiples of 4: every scalar owns a
        * 4-float cell of the regularised region whose three pad floats are zero from initialisation on and a fixed point of
        * training (zero gradient, zero L2 term, zero Adam update).  obj_per_time_slice must be 1, eb_dim <= 128 (a pass
        * also needs user_fnum, item_fnum <= 8, the index plan's limit for every type).  The batch rides as for SCORE_MODEL_GRU4REC (user_1hop = user_seq as [B, T, 1, Fi], length =
        * user_seq_length, read; the other index tensors zeros; length2 NULL); active_slices = A promises every length <= A, and a
        * length <= 0 does not ask for all T slices.  Workspace field (score_workspace_field): svdpp_act [B, 4 D + 4] =
        * [p_u | p_i | nb | share | n, ties, 0, 0], share_d = [c_d == n] / ties with c_d = sum_t |s_t,d| and ties the number of
        * maximal columns.  Kernels: csrc/svdpp.hip, one launch each way; the batch sums of the weight gradients through the
        * queued column sums, every sum in a fixed order. */
       SCORE_MODEL_SVDPP = 11,
       /* point_models/point_model.py:313-469 (SASRec) on PointBaseModel (:9-63): one block of two-head self-attention over the flat
        * history.  C = Fi * D, X [B, T, C] the gathered user_seq.  Per row N = (X - mean) / sqrt(var + 1e-8) (population variance
        * over C), Qin = gamma N + beta; Q = Qin Wq + bq, K = X Wk + bk, V = X Wv + bv (K and V from the RAW X); per head (width
        * C / 2) S = Q_h K_h^T / sqrt(C / 2), a key u with sum_c X[u, c] == 0 gets the score -2^32 + 1, softmax over ALL T keys (no
        * causal mask, lengths not used: every key masked gives uniform weights 1 / T), the weights times the query mask
        * [sum_c Qin[t, c] != 0], tf.nn.dropout on them ([2 B, T, T], head h of sample b at row h B + b), Y = concat_h(A_h V_h) + Qin.
        * rep_t = Y_t [t < length] (a length >= T: all positions), final = sum_t rep_t.  The shared head prediction_layer/fc1..fc3
        * (200 relu, dropout, 80 relu, dropout, 1 sigmoid; NO batch norm; input width 2 C + Cu) is applied three times with
        * independent dropout: to the positive rows [rep_t | Y_t | target_user], t = 1 .. T - 1, to the "negative" rows, the same
        * expression for t = 2 .. T - 1, and to [final | target_item | target_user], which gives y_pred [B].  loss = mean over
        * B (T - 1) of -log(p_pos + 1e-7) + mean over B (T - 2) of -log(1 - p_neg + 1e-7) + log_loss(label, y_pred) + reg_lambda *
        * sum l2_loss over the eight variables whose names hold neither "bias" nor "emb" -- BOTH layer-norm variables among them
        * (gamma's ones contribute reg_lambda * C / 2 from the start); padded positions count in both means.  The masks carry no
        * gradient.  At keep_prob = 1 the negative predictions equal the positive ones for t >= 2 and are computed once.
        * max_time_len >= 3, Fi * D <= 128 and 4 T (C + 1) + 2 T^2 + 4 T floats within 160 KiB (SCORE_E_SHAPE beyond);
        * obj_per_time_slice must be 1; hidden_size is accepted and ignored.  All T positions are always computed: active_slices
        * has no effect, length is read for rep / final only; length2 NULL.  The batch rides as for SCORE_MODEL_GRU4REC.
        * THE QUERY MASK AT TF'S INITIAL VALUES: with gamma = 1 and beta = 0, sum_c Qin of a live row is the rounding residue of
        * a sum that is exactly 0 in real arithmetic; TF's own mask there is an accident of its fp32 summation order.  The
        * kernels compute the formula as written, in fp32, in rising c; this one case is not pinned to any restatement.
        * score_param_layout: 14 entries in TF's creation order -- ln/Variable (beta, zeros), ln/Variable_1 (gamma, ones), both
        * regularised; multihead_attention/dense, dense_1, dense_2 (kernel [C, C] + bias); prediction_layer/fc1, fc2, fc3.
        * Dropout: score_forward's drop_mask0 [R, 200] / drop_mask1 [R, 80] with R = B (T - 1) + B (T - 2) + B rows ordered positive
        * (b-major, t = 1 .. T - 1), negative (t = 2 .. T - 1), final; score_state_t.drop_mask2 [2, B, T, T] for the attention
        * weights; without masks from the counter hash of drop_seed (or of score_step_scalars_t.drop_seed), one stream per use.
        * Workspace fields (score_workspace_field): sasrec_y [B, T, C], sasrec_final [B, C], sasrec_p / sasrec_att [B, 2, T, T]
        * (softmax / final weights), sasrec_qin [B, T, C], sasrec_hin (the head-input rows), sasrec_logit [R].
        * Kernels: csrc/sasrec.hip -- the attention in one launch each way, a workgroup per sample; the head's products are the
        * library's GEMMs; every sum in a fixed order, no atomics. */
       SCORE_MODEL_SASREC = 12 };

/* Constructor arguments of SCOREBASE.__init__ (score.py:12-13). */
typedef struct {
  int64_t feature_size;        /* N: rows of emb_mtx                              */
  int32_t eb_dim;              /* D: multiple of 4, <= 256                        */
  int32_t hidden_size;         /* H                                               */
  int32_t max_time_len;        /* T                                               */
  int32_t obj_per_time_slice;  /* K <= 32 (SCORE_MODEL_GRU4REC / _CASER / _DELF / _DEEMS / _SVDPP / _SASREC: 1) */
  int32_t user_fnum;           /* Fu                                              */
  int32_t item_fnum;           /* Fi                                              */
  int32_t model_type;          /* SCORE_MODEL_*                                   */
} score_config_t;

/* One dense variable inside the flat parameter buffer (TF variable names,
 * score.py graph-construction order). */
typedef struct {
  char    name[64];
  int64_t offset;              /* in floats, into the flat buffer                 */
  int32_t rows, cols;          /* cols == 0 for vectors                           */
  int32_t regularised;         /* build_l2norm name filter, score.py:91-94        */
  int32_t init;                /* 0 zeros, 1 ones, 2 glorot-uniform, 3 glorot-uniform with TF's convolution fans: fan_in = fan_out = rows * cols,
                                  4 truncated normal(0, 1): values beyond +-2 redrawn (tf.truncated_normal_initializer) */
} score_param_entry_t;

/* Layout of the flat dense-parameter buffer: regularised tensors first
 * ([0, n_reg) floats), then biases.  Returns the number of entries (or <0). */
int score_param_layout(const score_config_t* cfg, score_param_entry_t* out, int32_t max_entries,
                       int64_t* n_floats, int64_t* n_reg_floats);

/* The batch handed to SCOREBASE.train/eval (score.py:101-133, graph_loader.py:383),
 * already on the device as row-major int32. */
typedef struct {
  const int32_t* user_1hop;    /* [B,T,K,Fi] */
  const int32_t* user_2hop;    /* [B,T,K,Fu] */
  const int32_t* item_1hop;    /* [B,T,K,Fu] */
  const int32_t* item_2hop;    /* [B,T,K,Fi] */
  const int32_t* target_user;  /* [B,Fu]     */
  const int32_t* target_item;  /* [B,Fi]     */
  const int32_t* label;        /* [B]        */
  const int32_t* length;       /* [B]        */
  int32_t B;
  int32_t active_slices;       /* 0 (or >= T) = all T time slices.  0 < A < T: the caller promises
                                  length[b] <= A for every sample, and only slices t < A are gathered,
                                  planned and computed; every [B*T, .] activation of the pass is then
                                  laid out [B*A, .].  Slices t >= length[b] reach nothing in the
                                  reference either: dynamic_rnn(sequence_length) zeroes their outputs
                                  (score.py:205-208) and the temporal attention masks them to an exact 0
                                  weight (:182-185), so loss, predictions and every gradient are
                                  unchanged; samples with length[b] > A are treated as length A.
                                  The index tensors keep their [B,T,K,F] strides.                   */
  const int32_t* length2;      /* [B] SCORE_MODEL_DELF / _DEEMS only: item_seq_length, the mask of item_1hop's T positions (length is
                                  user_seq_length, the mask of user_1hop's).  NULL for every other model type: none reads it. */
} score_batch_t;

/* Named float offsets into the workspace (for tests / introspection). */
typedef struct {
  int64_t total_bytes;
  int64_t xside;      /* [2][B*T][Di+Du]  user_side, item_side (score.py:200-201) */
  int64_t atten_info; /* [B*T][4K]        [info_item | info_user] (score.py:198)          */
  int64_t rsave;      /* [2][B*T][K]      relu'd relateness r_i per co-attention  */
  int64_t query;      /* [B][Du+Di]       [target_user, target_item] (:210)       */
  int64_t head_inp;   /* [B][Dhead]       (:217)                                  */
  int64_t att_score;  /* [B][T]           (:213)                                  */
  int64_t logit;      /* [B]                                                      */
  int64_t y_pred;     /* [B]              (:76)                                   */
  int64_t loss;       /* [4]: loss, log_loss, l2, unused                          */
  int64_t gru_out;    /* [2][B*T][H]      user_side_rep_t, item_side_rep_t        */
  int64_t gru_final;  /* [2][B][H]        final states (RIA, score.py:244-247)    */
  /* index plan (score_index_plan) */
  int64_t n_occurrences;    /* R*B row uses in the batch (SURVEY 8d's R per sample)          */
  int64_t plan_meta;        /* int32 [2+G]: [0] = U unique rows (incl. row 0), [1+o] = first
                               unique position owned by shard o (o = 0..G)                   */
  int64_t plan_unique_rows; /* int32 [U]: local row index (row / G) of every unique row,
                               grouped by owner shard (row % G), ascending                   */
  int64_t plan_remap[6];    /* int32 copies of user_1hop, item_2hop, user_2hop, item_1hop,
                               target_user, target_item holding unique positions            */
} score_workspace_t;

int score_workspace_layout(const score_config_t* cfg, int32_t B, score_workspace_t* out);
/* Float offset of an INTERNAL workspace region by name ("gates", "a1", "dxproj", "dtgt", ...: csrc/engine.hip lists them) for
 * tests and tools that compare two forms of a pass region by region; *second (optional) gets the offset of the second
 * side / call of a paired region, -1 if the region is single.  Host-only; SCORE_E_BADARG for an unknown name.  Replaces
 * nothing in the reference (what `sess.run([tensor])` on an intermediate would be, score.py:188-224). */
int score_workspace_field(const score_config_t* cfg, int32_t B, const char* name, int64_t* offset, int64_t* second);

/* ---- per-op entry points (each is also a stage of score_forward/backward) ---- */

/* Measurement helper (bench.py's `roofline.peak_measured`, SURVEY.md 8d "the measured stream-copy ceiling as a second
 * denominator"): dst[i] = src[i] for n_floats floats (a multiple of 4; both 16-byte aligned) as a plain float4 grid-stride
 * copy -- the HBM bandwidth a trivially coalesced kernel reaches on this box (n_floats * 8 bytes move per call). */
int score_stream_copy(float* dst, const float* src, int64_t n_floats, void* stream);

/* tf.truncated_normal_initializer (defaults: mean 0, stddev 1, resampled outside 2 sigma; score.py:44) for a
 * row shard of emb_mtx: local row i holds global row i * row_stride + row_first (row_stride = number of shards,
 * row_first = this shard's rank; 1 / 0 for the whole table).  Every element is a pure function of
 * (seed, global row, column) -- the inverse-CDF of a counter-based uniform -- so any sharding of the same seed
 * yields the same table, and no rank ever materialises rows it does not own.  Global row 0 (the masked dummy
 * row, score.py:45-47) and local rows past n_global_rows are written as zeros. */
int score_table_init(float* table, int64_t n_local_rows, int32_t D, int64_t row_stride, int64_t row_first,
                     int64_t n_global_rows, uint64_t seed, void* stream);

/* tf.nn.embedding_lookup + reshape (score.py:51-66): out[r, :] = table[idx[r], :].
 * Bit-exact copy. n_idx rows of D floats. */
int score_gather_fwd(const float* table, int64_t n_rows, int32_t D, const int32_t* idx,
                     int64_t n_idx, float* out, void* stream);

/* Fused gather + co_attention (score.py:147-167 in its exact collapsed form,
 * SURVEY.md 8a A4) for ONE call: seq1/seq2 index tensors [BT,K,F], target rows
 * gathered to tgt [B, F*D].  Writes seq1_result to out1 (row stride ld1),
 * seq2_result to out2 (ld2), atten_info [BT,2K] into info (ldi) and r [BT,K]
 * into rsave.  W = dense kernel [3*F*D], bias = [1].  mode 0 = co-attention,
 * mode 1 = RCA's reduce_sum over K (score.py:266-269; W/bias/info/rsave unused). */
int score_coattn_fwd(const float* table, int64_t n_rows, int32_t D, int32_t F, int32_t K,
                     int32_t B, int32_t T, const int32_t* idx1, const int32_t* idx2,
                     const float* tgt, const float* W, const float* bias,
                     float* out1, int32_t ld1, float* out2, int32_t ld2,
                     float* info, int32_t ldi, float* rsave, int32_t mode, void* stream);

/* The time slices per chunk that the forward above (F1 = 0) or score_forward's launch of both co-attention calls
 * (feature counts F0, F1) takes for B samples of T computed slices: mode 0 with K <= 10, one float4 per lane and id
 * lists that fit an instance run csrc/embed.hip coattn_fwd_kernel_units, where a wave works through a chunk of
 * consecutive slices of one sample.  0 = the shape runs coattn_fwd_kernel (one unit per wave); < 0 = bad argument.
 * A function of the shape alone, never of a timing. */
int score_coattn_fwd_chunk(int32_t D, int32_t K, int32_t B, int32_t T, int32_t F0, int32_t F1);

/* Backward of the above.  g1/g2/ginfo are the gradients of out1/out2/info with
 * the same strides.  Scatter-adds row gradients into grad_table [n_rows, D]
 * (row 0 skipped: mask, score.py:47), writes dzsum [BT] (sum_i dz_i, feeds the
 * target-row / w_t / bias gradients) and accumulates dW[Dx..3Dx) into
 * partial slabs reduced by the library into dW (+=). */
int score_coattn_bwd(const float* table, float* grad_table, int64_t n_rows, int32_t D, int32_t F,
                     int32_t K, int32_t B, int32_t T, const int32_t* idx1, const int32_t* idx2,
                     const float* W, const float* rsave,
                     const float* g1, int32_t ld1, const float* g2, int32_t ld2,
                     const float* ginfo, int32_t ldi, float* dzsum, float* dW,
                     float* scratch, int64_t scratch_floats, int32_t mode, void* stream);

/* C[M,N] = epi(op(A) . op(B)) in exact fp32 (v_mfma_f32_32x32x2_f32).
 * trans: 0 = A[M,K] B[K,N];  1 = A[M,K] B[N,K]^T;  2 = A[K,M]^T B[K,N] (K is the
 * reduced dim).  flags: 1 add bias[N], 2 relu, 4 accumulate into C,
 * 8 dropout (tf.nn.dropout: x/keep * mask; mask from drop_mask bytes or, if null,
 * from a counter hash of drop_seed), 16 use the bf16x3 matrix-core product (fp32-accurate,
 * see score_state_t.gemm_mode) on the shapes where it measured faster, 32 use it whenever legal,
 * 64 relu backward fused: drop_mask then points at the layer's fp32 output Y [M,N] and the result is
 * C = [Y > 0] * (A.B) / keep_prob (not together with 8).
 * Bits 16-30: bias row group g (0 = the usual single bias row): bias is [ceil(M/g), N] and
 * output row r adds bias row r/g -- the per-sample term of the folded attention layer.
 * scratch is used for split-K. */
int score_gemm(int32_t trans, int32_t M, int32_t N, int32_t K,
               const float* A, int32_t lda, const float* Bm, int32_t ldb,
               float* C, int32_t ldc, const float* bias, int32_t flags,
               float keep_prob, const uint8_t* drop_mask, uint64_t drop_seed,
               float* scratch, int64_t scratch_floats, void* stream);

/* The same-shape products of `ngroups` (<= 4) independent problems C_i[M,N] = A_i[M,K] . op(B_i) (+ bias_i[N]) in ONE launch
 * on the bf16 matrix cores, fp32-accurate (bf16x3), with a whole-N output panel per workgroup: the form the GRU input
 * projections of the two sides (score.py:205-208) and their input gradients take at cfg-3's sizes (csrc/gemm_panel.hip).
 * trans_b: 0 = B_i[K,N], 1 = B_i[N,K] (C = A . B^T).  `images` is scratch for the weights' MFMA-fragment images,
 * ngroups * K/32 * 8*ceil(N/128) * 768 floats.  Shapes it does not cover (N % 16, N <= 256 or > 512, K % 32, ld % 4, too few
 * rows to fill the chip) return SCORE_E_SHAPE: use score_gemm. */
int score_gemm_panel_products(int32_t trans_b, int32_t ngroups, int32_t M, int32_t N, int32_t K,
                              const float* const* A, int32_t lda, const float* const* Bm, int32_t ldb,
                              float* const* C, int32_t ldc, const float* const* bias,
                              float* images, int64_t image_floats, void* stream);
/* The two halves of score_gemm_panel_products: the images of the weights (once per set of weights), and the products
 * from prepared images (as the engine runs them: the images are written once per step, beside the gather). */
int score_gemm_panel_images(int32_t trans_b, int32_t ngroups, int32_t N, int32_t K, const float* const* Bm, int32_t ldb,
                            float* images, int64_t image_floats, void* stream);
int score_gemm_panel_run(int32_t ngroups, int32_t M, int32_t N, int32_t K, const float* const* A, int32_t lda,
                         float* const* C, int32_t ldc, const float* const* bias, const float* images,
                         int64_t image_floats, void* stream);

/* tf.nn.dynamic_rnn(GRUCell(H), sequence_length) recurrence (score.py:205-208)
 * given the hoisted input projection xproj [B*T,3H] = x.[Wx_gates|Wx_cand]+bias.
 * Wg/Wc point at the h-rows of gates/kernel [H,2H] and candidate/kernel [H,H].
 * out [B*T, ldo] gets h_t (0 for t>=len), gates_save [B*T,3H] gets (r,u,c),
 * final [B,H] the carried state. */
int score_gru_fwd(int32_t B, int32_t T, int32_t H, const float* xproj, const float* Wg, int32_t ldwg,
                  const float* Wc, int32_t ldwc, const int32_t* length,
                  float* out, int32_t ldo, float* gates_save, float* final_state, void* stream);

/* Backward recurrence: dout [B*T, lddo] (+ dfinal [B,H] or null) ->
 * dxproj [B*T,3H] (pre-activation grads dr,du,dc), rh [B*T,H] = r*h_{t-1} and
 * hprev [B*T,H] = h_{t-1}; `hprev` must have room for B*T*H + 3*H*H floats (its tail
 * is scratch for the transposed recurrent weights). */
int score_gru_bwd(int32_t B, int32_t T, int32_t H, const float* Wg, int32_t ldwg, const float* Wc,
                  int32_t ldwc, const int32_t* length, const float* out, int32_t ldo,
                  const float* gates_save, const float* dout, int32_t lddo, const float* dfinal,
                  float* dxproj, float* rh, float* hprev, void* stream);

/* Guard of the optimizer entry points.  tf.nn.embedding_lookup raises inside sess.run for an id outside the table and
 * NO variable is updated by that call (score.py:51-66, 101-116).  The kernels that read the ids report such a batch in
 * the device word score_state_t.id_status; an optimizer call that is handed the same word reads it when it EXECUTES
 * (one uniform load) and, if it is non-zero, leaves the variable and both Adam slots untouched.  `skipped` (optional
 * device counter) gets +1 from each suppressed call it is passed to: the caller hands it to ONE call per step (the dense
 * variables') and learns how many steps to take off its own step count / beta powers when it sees the word.  The word
 * is sticky: every later guarded call is suppressed too until the caller clears it.  NULL guard / NULL id_status =
 * unguarded (a row shard's optimizer: the sharded path rejects such a batch on the host before the step starts). */
typedef struct {
  const int32_t* id_status;
  int32_t* skipped;
} score_guard_t;

/* tf.train.AdamOptimizer ApplyAdam (score.py:96-99), dense over n floats:
 * g' = g + l2*p (first n_reg floats); m += (g'-m)(1-b1); v += (g'^2-v)(1-b2);
 * p -= m*alpha/(sqrt(v)+eps).  alpha = lr*sqrt(1-b2^t)/(1-b1^t) from the host. */
int score_adam(float* p, float* m, float* v, const float* g, int64_t n, int64_t n_reg,
               float l2, float alpha, float beta1, float beta2, float eps, const score_guard_t* guard, void* stream);

/* score_adam / score_adam_rows with alpha read from device memory (sc->adam_alpha) at execution time. */
int score_adam_dev(float* p, float* m, float* v, const float* g, int64_t n, int64_t n_reg, float l2,
                   const score_step_scalars_t* sc, float beta1, float beta2, float eps, const score_guard_t* guard,
                   void* stream);
int score_adam_rows_dev(float* p, float* m, float* v, const float* g, int64_t n_rows, int32_t D, uint8_t* row_flags,
                        const score_step_scalars_t* sc, float beta1, float beta2, float eps, const score_guard_t* guard,
                        void* stream);

/* The same update over the [n_rows, D] embedding table, driven by a per-row state byte so the
 * dense sweep only moves the rows dense ApplyAdam actually changes (bit-identical result):
 *   0  m = v = 0 and no gradient this step  -> ApplyAdam is the identity: nothing is read
 *   1  m or v nonzero, no gradient this step -> g = 0 (moments decay, p moves); g is not read
 *   2  gradient written this step (score_backward / score_segment_sum_rows set it) -> full
 *      update from g, then the state becomes 1
 *   (3 exists only inside score_adam_catchup_ids: a live row the batch is about to read, see below)
 * g rows in state 0/1 are never read, so grad_table needs no zero fill between steps.
 * A suppressed call (guard) leaves the state bytes as they are: the caller clamps the 2s back to 1. */
int score_adam_rows(float* p, float* m, float* v, const float* g, int64_t n_rows, int32_t D,
                    uint8_t* row_flags, float alpha, float beta1, float beta2, float eps, const score_guard_t* guard,
                    void* stream);
/* score_adam_rows on the table and score_adam on the flat dense variables [n] (first n_reg regularised with l2) in ONE launch:
 * disjoint memory, the same arithmetic per element as the two calls.  guard: ONE counted call (the dense half counts a suppressed
 * step, neither half applies anything while the word is set). */
int score_adam_rows_and_dense(float* p, float* m, float* v, const float* g, int64_t n_rows, int32_t D, uint8_t* row_flags,
                              float* wp, float* wm, float* wv, const float* wg, int64_t n, int64_t n_reg, float l2, float alpha,
                              float beta1, float beta2, float eps, const score_guard_t* guard, void* stream);

/* ---- time-tiled ApplyAdam over the table ----------------------------------------------------------------------
 * Dense ApplyAdam moves every live row every step, but the update of a row WITHOUT a gradient (m *= b1, v *= b2,
 * p -= alpha_t m/(sqrt(v)+eps)) reads nothing except the row and the step's alpha.  These entry points apply such
 * updates late, in step order, the first time a row is needed: the same fp32 operations in the same order as the
 * sweep of score_adam_rows, so the table, m and v are bit-identical to it at every point where they are observed
 * -- while a row's HBM traffic drops from once per step to once per use.  Nothing is skipped: every (row, step)
 * update is executed exactly once.
 *   row_step[r]   optimizer steps already applied to row r (meaningful for rows in state 1 / 2)
 *   alpha_ring    SCORE_ADAM_RING + 1 floats: alpha of step s at [s % SCORE_ADAM_RING] (score_adam_touched writes
 *                 it), and one sticky error word at [SCORE_ADAM_RING], nonzero if a row ever lagged more steps than
 *                 the ring remembers (the caller's window sweep must keep every live row within
 *                 SCORE_ADAM_RING - 2 steps)
 * Protocol of step n (1-based), single table (no row sharding):
 *   score_adam_catchup_ids(ids of the batch, upto = n-1)      before score_forward
 *   score_adam_catchup_rows(slice n % window, upto = n-1)     any time after that call has finished and before
 *                                                            the next step's catchup_ids; may run on another
 *                                                            stream beside forward/backward/score_adam_touched
 *   score_forward, score_backward (scatter_mode 0: rows with a gradient end in state 2)
 *   score_adam_touched(step = n, alpha_n)                     state-2 rows: ApplyAdam from g, state 1, row_step n
 * and score_adam_catchup_rows(0, n_rows, upto = n) before anything else reads p, m or v. */
#define SCORE_ADAM_RING 64
typedef struct {
  float* p; float* m; float* v;   /* [n_rows, D] variable and its two Adam slots           */
  const float* g;                 /* [n_rows, D] row gradients (rows in state 2 are valid) */
  int64_t n_rows;
  int32_t D;
  int32_t reserved;
  uint8_t* row_flags;             /* [n_rows] state bytes of score_adam_rows               */
  uint32_t* row_step;             /* [n_rows]                                              */
  float* alpha_ring;              /* [SCORE_ADAM_RING + 1]                                 */
  float beta1, beta2, eps;
  int32_t reserved2;
  const int32_t* id_status;       /* optional guard word (score_guard_t.id_status).  While it is non-zero:
                                     score_adam_touched applies nothing -- its rows go back to state 1 with
                                     row_step = step - 1 (they were current up to there), alpha_ring is not written --
                                     and the catch-up entry points replay nothing (the steps they would replay may be
                                     ones that were suppressed): the table, m and v stay as the last applied step left them */
  const int32_t* skipped_steps;   /* optional DEVICE counter (score_guard_t.skipped of the same caller): steps suppressed so
                                     far, i.e. by how much the `step` arguments run ahead of what was really applied   */
} score_adam_table_t;
int score_adam_touched(const score_adam_table_t* t, uint32_t step, float alpha, void* stream);
/* score_adam_touched(t, step, alpha) and score_adam(p, m, v, g, n, n_reg, l2, alpha, t->beta1, t->beta2, t->eps, guard) --
 * the step's whole ApplyAdam, table rows with a gradient and the flat dense variables -- in ONE launch: the two touch disjoint
 * memory and were two dependent launches at the end of every step (the reference's own batch sizes are bound by the host's
 * launch calls).  The guard is t->id_status; `skipped` (optional) counts the step when it is suppressed.  Same arithmetic in
 * the same order per element as the two calls: the same bits. */
int score_adam_touched_and_dense(const score_adam_table_t* t, uint32_t step, float alpha, float* p, float* m, float* v,
                                 const float* g, int64_t n, int64_t n_reg, float l2, int32_t* skipped, void* stream);
/* A backward pass whose gradient nobody applies: every state-2 row back to state 1.  A row that was live keeps its
 * row_step (the batch's rows were brought up to `upto` before that pass); a row that was in state 0 -- m = v = 0: its owed
 * updates are identities and any count is right for it -- gets row_step = upto, which keeps it inside the ring. */
int score_adam_unmark(const score_adam_table_t* t, uint32_t upto, void* stream);
/* every value of ids[0..n_ids) that names a live row (values outside [0, n_rows) are ignored, so a whole flat batch
 * buffer may be passed): replay the zero-gradient steps row_step+1 .. upto of that row */
int score_adam_catchup_ids(const score_adam_table_t* t, const int32_t* ids, int64_t n_ids, uint32_t upto, void* stream);
/* The NEXT batch's rows, one step early.  Between score_backward's row scatter of step `step` (its stage boundary 4: every
 * row that gets this step's gradient is in state 2 by then) and the next step's score_forward, on any stream: every id that
 * names a live row NOT in state 2 is replayed through `step` itself -- its gradient in this step is zero, so its update
 * needs nothing but alpha (= the alpha score_adam_touched(step) is called with; written to the ring here too).  Rows in
 * state 2 are left to score_adam_touched.  Afterwards every row the next batch reads is current up to `step`, and the
 * next step needs no score_adam_catchup_ids: its 0.07 ms (cfg-3) run beside this step's weight-gradient products instead
 * of in front of the next forward.  Must not overlap score_adam_catchup_rows on another stream (same rows). */
int score_adam_catchup_ids_through(const score_adam_table_t* t, const int32_t* ids, int64_t n_ids, uint32_t step, float alpha,
                                   void* stream);
/* the same for every state-1 row of [row_begin, row_end) */
int score_adam_catchup_rows(const score_adam_table_t* t, int64_t row_begin, int64_t row_end, uint32_t upto, void* stream);

/* ---- whole-path entry points --------------------------------------------- */

typedef struct {
  const float* table;   /* [n_table_rows, D] effective table (row 0 == 0)         */
  int64_t n_table_rows;
  const float* w;       /* flat dense parameters                                  */
  float* workspace;     /* score_workspace_layout(...).total_bytes                */
  int64_t workspace_bytes;
  int32_t scatter_mode; /* embedding-gradient scatter: 0 = sorted occurrences + per-row pull
                           (no float atomics, bitwise reproducible; needs score_index_plan
                           with 1 shard), 1 = global_atomic_add_f32 into grad_table,
                           2 = pull into the unique-row order of a sharded plan (grad_table
                           is the [U, D] gradient of the gathered mini-table)            */
  int32_t global_batch; /* samples the loss mean runs over (data parallel); 0 = batch->B  */
  int32_t gemm_mode;    /* dense layers: 0 = v_mfma_f32_32x32x2_f32 (bitwise an fp32 fmaf chain),
                           1 = "bf16x3": every fp32 operand split exactly into three bf16 and
                           six v_mfma_f32_32x32x16_bf16 per k-step -- fp32 accuracy (dropped
                           terms < 2^-24 relative) at 2.7x the matrix-core rate              */
  int32_t debug_flags;  /* A/B switches (0 in production): bit 0 = run the H = 256 recurrence step by step (grouped GEMMs +
                           pointwise launches per time slice) instead of the persistent streaming kernel; bit 1 = the
                           head's forward in one launch at every batch size; bit 2 = the H = 128 recurrences on the
                           f32-input MFMA kernels instead of the bf16x3 form; bit 3 = the GRU input projections (and
                           their input gradients) on the tiled bf16x3 kernel instead of the whole-N panel form
                           (csrc/gemm_panel.hip); bit 4 = the input gradients in the panel form at every size; bit 6 =
                           build_fc_net layer by layer instead of the fused head kernels; bit 7 = the temporal attention
                           layer by layer instead of its fused kernels (the paths shapes outside the fused kernels'
                           instantiated widths take anyway); bit 5 = the index plan sorts with the library's radix sort at
                           every size, bit 8 = with csrc/sort.hip's at every size (default: by the number of occurrences;
                           both are stable, the plan is the same bits); bit 9 (512) = never take the per-sample
                           whole-model kernels (csrc/persample.h: at H = 32, B <= 512, K <= 10, <= 48 computed slices
                           SCORE / SCORE_USER / SCORE_ITEM run each pass as ONE kernel, a workgroup per sample), bit 10
                           (1024) = take them for the forward pass only, bit 11 (2048) = for the backward pass only;
                           bit 12 (4096) = NO second stream: everything score_forward / score_backward would fork onto
                           the context's side stream runs on `stream`, in launch order (same results bit for bit; what
                           a suspected stream race is compared against -- score_amd.model inlines its own streams too);
                           bit 14 (16384) = unused, ignored; bit 13 (8192) =
                           (SCORE_MODEL_GRU4REC) the two stacked recurrences one layer per launch with the projection GEMM between
                           them (the composed form: what H outside {16, 32, 64} runs anyway) instead of csrc/gru_stack.hip;
                           (SCORE_MODEL_DEEMS) its two recurrences one launch per side instead of one grouped launch;
                           bit 15 (32768) = the co-attention backward loads the seq1 / seq2 rows of EVERY neighbour for the
                           w1 / w2 gradients, instead of only those whose relu'd score is > 0 (an inactive one contributes
                           dz = 0 times its row: the same bits on a finite table; csrc/embed.hip);
                           bit 16 (65536) = the co-attention backward requests a unit's ids and saved scalars one unit ahead,
                           behind the pass-1 rows of the unit before, instead of at the top of the unit's own iteration
                           (same registers, same arithmetic, same bits; K <= 10 only; measured inside the noise at cfg-3);
                           bit 17 (131072) = the fused gather + co-attention forward runs one unit per wave
                           (coattn_fwd_kernel) where it would work through a chunk of slices per wave
                           (coattn_fwd_kernel_units, see score_coattn_fwd_chunk): same bits, the A/B arm;
                           bit 18 (262144) = the embedding-gradient scatter runs pull_kernel where score_pull_form would
                           choose pull_kernel_lanes (one occurrence per lane; csrc/scatter.hip): same bits, the A/B arm;
                           bits 20 .. 23 = no switch but a number, for measurements: a chunk length 1 .. 15 to take in
                           place of score_coattn_fwd_chunk's (0 = the rule).
                           The ONLY switches of the launch sequence: the library reads no environment variable       */
  uint8_t* row_flags;   /* optional [n_table_rows] row state of the dense table optimizer (see
                           score_adam_rows): score_backward (scatter_mode 0) marks every row it
                           writes into grad_table with 2 and leaves all other rows of grad_table
                           untouched, so grad_table needs no zero fill.  NULL = off: the caller
                           zero-fills grad_table and uses score_adam.                            */
  void* gather_done_event; /* optional hipEvent_t: score_forward records it right after the fused gather +
                           co-attention launch, so a caller can start the index plan of the same batch on
                           another stream behind the HBM-bound gather instead of beside it             */
  void* plan_done_event;   /* optional hipEvent_t (recorded by the caller after score_index_plan on its own
                           stream): score_backward waits for it just before the row scatter, the first
                           consumer of the plan -- not at its start                                   */
  const score_step_scalars_t* step_scalars; /* optional DEVICE pointer: score_forward then takes the dropout seed from it
                           (its by-value drop_seed argument is ignored; shapes the fused head kernel does not cover
                           return SCORE_E_SHAPE when keep_prob < 1), so the launch sequence holds no per-step value */
  score_context_t context; /* side stream + events of this caller (score_context_create); NULL = the
                           process-wide default context of the current device                         */
  int32_t* id_status;   /* optional DEVICE word, zero-initialised by the caller, sticky: tf.nn.embedding_lookup on the
                           CPU raises for an id outside [0, feature_size) (score.py:51-66).  Here every kernel that turns an
                           id into an address reads such an id as the dummy row 0 instead (never an out-of-bounds access,
                           with or without this word), and the kernels that see the ids as fed -- the fused gather and
                           the target-row gather of score_forward, the occurrence fill of score_index_plan -- OR bit i
                           into the word, i = position of the tensor in the feed tuple (0 user_1hop, 1 user_2hop,
                           2 item_1hop, 3 item_2hop, 4 target_user, 5 target_item; graph_loader.py:383).  No extra launch,
                           no read-back: score_forward's loss reduction reads the word and, if it is set, writes NaN
                           to loss[0] / loss[1] and the bits to loss[3], so whoever reads the loss learns of it;
                           score_id_status() is the synchronous query.  Ids of time slices >= active_slices are never
                           dereferenced and not checked.                                                         */
  void* grads_done_event; /* optional hipEvent_t (score_backward): everything that FINISHES grad_w -- the slab reduce, the folded
                           attention layer's gradient, the column sums -- runs on the context's side stream, and this event is
                           recorded behind it.  Where the finishers are forked:
                             - the layer-by-layer pass under scatter_mode 0 (or 1) with weight-gradient products queued: behind
                               target_bwd_kernel, the last launch that feeds them, in FRONT of the row scatter, which runs
                               beside them (and beside the products) on `stream`;
                             - otherwise -- scatter_mode 2, the row-sharded pass, or a pass with no queued products: behind the
                               end-of-pass products, which follow the row scatter on `stream`;
                             - the per-sample whole-model pass: with the products, behind the backward kernel, in front of the
                               row scatter.
                           grad_table is complete on `stream` when score_backward returns; grad_w only once the event has fired.
                           The event says NOTHING about the row scatter, and the scatter reads the co-attention weights: the dense
                           variables may only be updated (and grad_w read) behind the event AND behind `stream`'s own launches of
                           the pass -- on `stream`, after making it wait for the event, or on another stream that waits for the
                           event and for stage boundary 4.  NULL: everything on `stream`. */
  void* loss_done_event;  /* optional hipEvent_t (score_forward): the loss reduction (one workgroup: loss[0..3] from the per-sample
                           terms and the L2 partial sums) then runs on the context's side stream behind the head, and this event is
                           recorded behind it -- the head's successor on `stream` (score_backward's first launch) no longer queues
                           behind a one-block kernel.  loss[] is final once the event has fired; on `stream` it is final behind
                           score_backward of the same step (which joins the side stream), not behind score_forward alone.  NULL:
                           on `stream`, as before (evaluation: nothing follows the forward pass).
                           (The per-sample whole-model forward kernel reduces the loss itself -- its last workgroup to finish
                           does it, round 5 -- so there the event is simply recorded on `stream` behind that kernel.)      */
  float* loss_host;       /* optional: four floats of PINNED HOST memory mapped into the device (hipHostMalloc): the per-sample
                           forward kernel also stores loss[0..3] there (system scope), so a caller that returns the loss every
                           step (score.py:101-116) reads it after waiting for an event recorded behind score_forward -- no copy,
                           no extra stream.  Ignored by the layer-by-layer pass (score_persample_form tells which runs).   */
  float* plan_workspace;  /* optional (score_backward, scatter_mode 0): the batch's index plan lies in THIS buffer -- another
                           workspace of the same layout, where score_index_plan wrote it -- instead of in `workspace`: a caller
                           that alternates two buffers for the plans can sort the next batch's plan while this step's scatter
                           still reads its own (everything else of the step stays in `workspace`).  NULL: in `workspace`.       */
  const uint8_t* drop_mask2; /* optional (score_forward, SCORE_MODEL_SASREC with keep_prob < 1): explicit dropout mask of the
                           attention weights, device [2, B, T, T] of 0 / 1 (head h of sample b at row h B + b); NULL: from the seed.
                           (The slot of two reserved 32-bit words: 8 bytes, 8-byte aligned -- size and every offset as before.) */
} score_state_t;

/* Synchronous query of a score_state_t.id_status word: copies it to *bits (optional), waits for `stream`, clears the
 * word when `clear` != 0, and returns SCORE_E_INDEX if any bit was set (0 otherwise): the status TF's
 * InvalidArgumentError "indices[...] is not in [0, N)" corresponds to (score.py:51-66). */
int score_id_status(int32_t* id_status, int32_t* bits, int32_t clear, void* stream);

/* Which kernel form the two sides' GRU input projections (score.py:205-208; *x_form) and their input gradients
 * (*dx_form) take in score_forward / score_backward for a batch of B samples with `active_slices` computed time slices
 * (0 = all T) under st->gemm_mode / st->debug_flags: 0 = the tiled kernels (gemm_bf16x3.hip / gemm.hip), n > 0 = the
 * whole-N panel form (gemm_panel.hip) with each side's output columns as n panel groups (2 = column halves: H = 256).
 * Host-only query, nothing is launched: what the parity tests assert before they compare the two forms. */
int score_gemm_forms(const score_config_t* cfg, const score_state_t* st, int32_t B, int32_t active_slices,
                     int32_t* x_form, int32_t* dx_form);

/* 1 if score_forward / score_backward run a batch of B samples with `active_slices` computed time slices (0 = all T) as the
 * per-sample whole-model kernels (csrc/persample.h) under st->scatter_mode / st->debug_flags, 0 if layer by layer.  Host-only:
 * callers use it to place their own side-stream work (score_amd/model.py), tests to assert the form they compare. */
int score_persample_form(const score_config_t* cfg, const score_state_t* st, int32_t B, int32_t active_slices);

/* Index plan of a batch (depends on the indices only; run it before score_backward, on
 * any stream ordered before it).  Radix-sorts all R*B row uses by (owner shard, row).
 * n_shards > 1 (table row-sharded, owner = row % n_shards) or dedup == 1 additionally
 * de-duplicates them: unique rows grouped by owner -> what to request from each shard --
 * and writes the six index tensors remapped to unique positions, so the same kernels run
 * on the gathered [U, D] mini-table.  dedup is 0 or 1 (SCORE_E_BADARG otherwise).
 * Replaces nothing in the reference (it has no multi-device code);
 * it is the index-routing step BASELINE.json's north_star asks for. */
int score_index_plan(const score_config_t* cfg, const score_state_t* st, const score_batch_t* batch,
                     int32_t n_shards, int32_t dedup, void* stream);

/* The small-batch sort behind score_index_plan as an op of its own (csrc/sort.hip): a STABLE least-significant-digit radix
 * sort of n (key, value) pairs of 32-bit words by the low key_bits bits of the key (all higher bits must be zero), 11 - 12 bits
 * per pass (key_bits 21: two passes; 32: three), six launches for two passes whatever n.  keys / vals and keys_alt / vals_alt
 * are the two buffers the passes alternate between; *result_in_alt says where the sorted pairs are (1: the alt buffers -- an
 * odd number of passes --, 0: keys / vals); the other pair holds an intermediate pass.  temp: score_sort_pairs_temp_bytes(n). */
int score_sort_pairs(uint32_t* keys, uint32_t* vals, uint32_t* keys_alt, uint32_t* vals_alt, int64_t n, int32_t key_bits,
                     void* temp, int64_t temp_bytes, int32_t* result_in_alt, void* stream);
int64_t score_sort_pairs_temp_bytes(int64_t n);

/* out[rows[j], :] = sum over slots j with equal rows[j] of src[j, :] (slot order; rows never
 * named keep their value).  The shard owner uses it to combine the row gradients received
 * from every rank.  row_flags (optional, [n_out_rows]): every row written is marked 2 for
 * score_adam_rows.  scratch: score_segment_sum_scratch_bytes(n, D) -- the answer carries 64 bytes of slack, the call itself
 * returns SCORE_E_WORKSPACE (nothing launched) from 65 bytes below it.  Row 0 is a row like any other here, n_out_rows = 1
 * included.  D: a multiple of 4 up to 256 (score_pull_geometry has the refusals); n below 2^29; n = 0 does nothing. */
int score_segment_sum_rows(const int32_t* rows, const float* src, int64_t n, int32_t D, int64_t n_out_rows,
                           float* out, uint8_t* row_flags, void* scratch, int64_t scratch_bytes, void* stream);
int64_t score_segment_sum_scratch_bytes(int64_t n, int32_t D);

/* Which kernel the embedding-gradient scatter of score_backward takes (host only, no GPU needed).  1 = pull_kernel_lanes,
 * the form with one occurrence's metadata per lane, 32-bit offsets from one base pointer and the co-attention weight
 * slices in LDS; 0 = pull_kernel.  The lanes form needs: mode 1 (constant coefficients: RCA / RRN) or 2 (co-attention
 * coefficients) -- not 0, the owner-side row sum; D in {16, 32, 64}; and span_bytes, the distance from the lowest
 * activation-gradient / coefficient pointer of the launch to the end of the highest, in (0, 4 GiB].  debug_flags bit 18
 * overrides it.  Both kernels give the same bits.  score_pull_last_form: what this process's latest scatter launch took
 * (-1 before the first). */
int score_pull_form(int32_t D, int32_t mode, int64_t span_bytes);
int score_pull_last_form(void);

/* The launch geometry of the row scatter (pull kernel + fix-up launch) over n occurrences at row width D, as the launcher
 * computes it (host only, no GPU needed; the launcher and this query share one function):
 *   *window            occurrences per window: 8 below 2^18 occurrences, 16 from 2^18, 32 from 2^19, 64 from 2^20
 *   *lanes_per_row     lanes of a group, four floats each: the power of two at or above D/4 (D = 12: 4 lanes, 3 used)
 *   *groups_per_block  256 / lanes_per_row: windows per workgroup, and the groups a long chain is split over
 *   *long_chain        a run that continues through more than this many windows after its first is summed by the whole
 *                      workgroup in the fix-up launch (chunk = ceil(L / groups_per_block) windows per group, eight loads per
 *                      trip), a shorter one by the group of its first window
 * SCORE_E_BADARG: a null pointer, n < 0, D <= 0 or D not a multiple of 4.  SCORE_E_SHAPE: D above 256 (more than 64 lanes).
 * score_segment_sum_rows refuses those widths the same way: D % 4 != 0 with SCORE_E_BADARG before anything is launched; D
 * above 256 with SCORE_E_SHAPE from the launcher, after the sort of the row ids inside scratch -- `out` and `row_flags` are
 * untouched in both cases.  (score_rows_accumulate / _multi refuse D above 256 with SCORE_E_BADARG.) */
int score_pull_geometry(int64_t n, int32_t D, int32_t* window, int32_t* lanes_per_row, int32_t* groups_per_block,
                        int32_t* long_chain);

/* Which forms the head and the temporal attention of the launch-stream pass took in this process's latest score_forward (bits
 * 0 .. 15) and latest score_backward (bits 16 .. 19 and 2 .. 4); -1 before the first of either.  Written on the host by the
 * launchers, read-only, like score_pull_last_form (with a captured graph: the forms of the capture).  A pass clears its fields
 * when it starts, so 0 in a field also stands for a stage the pass does not have or did not reach (the per-sample kernels,
 * a model type without attention / without build_fc_net's head).
 *   bits  0 ..  1  head forward     0 layer by layer, 1 head_fwd_fused_kernel in one launch, 2 in two launches
 *   bits  2 ..  4  head backward    0 layer by layer, else ny of head_bwd_fused_kernel's grid (1, 2, 4)
 *   bits  5 ..  7  attention fwd    0 separate launches, else S of attn_fwd_fused_kernel (samples per workgroup: 1, 2, 4)
 *   bits  8 .. 15  attention fwd    KQ of the attn_fwd_fused_kernel instance (36, 44, 52, 84, 148; 0 with separate launches)
 *   bits 16 .. 18  attention bwd    0 separate launches, else S of attn_inp_bwd_fused_kernel
 *   bit  19        attention bwd    1 the pooling / softmax / dense_5 / dense_4 backward ran inside attn_inp_bwd_fused_kernel
 *   bit  20        a score_forward has run        bit 21   a score_backward has run */
int score_head_last_forms(void);

/* What the latest product of this process launched (host only; -1 before the first): score_gemm, and the grouped launches the
 * engine makes for same-shape products.  Written on the host where the launch is decided, read-only, like score_pull_last_form.
 *   bits  0 ..  1  family     1 gemm_f32_kernel (exact fp32 on the f32 matrix instruction), 2 gemm_bf16x3_kernel
 *   bits  2 ..  3  WM         wave tile height in 32-row units (f32: block = 64 WM rows; bf16x3: wm, block = 64 wm rows)
 *   bits  4 ..  5  WN         f32: wave tile width in 32-column units (block = 64 WN columns); bf16x3: 0 (always 128 columns)
 *   bits  6 ..  7  trans      the operand layout of the kernel instance (0 NN, 1 NT, 2 TN)
 *   bit   8        grouped    1 several same-shape problems in one launch (never split)
 *   bits 12 .. 27  K slabs    workgroup layers along K actually launched; 1 = K not split, more = splitk_reduce_kernel follows
 *                             and applies the epilogue */
int score_gemm_last_form(void);

/* What the latest recurrence launch of this process was (host only; -1 before the first): score_gru_fwd / score_gru_bwd and
 * the engine's two-sided launches.  Written on the host where the launch is decided, read-only.
 *   bits  0 ..  2  family     1 bf16x3 recurrence (H = 128), 2 register-resident weights (H = 16, 32, 64; 128 with the bf16x3
 *                             form off), 3 streamed weights (H = 256 inside the engine), 4 step by step (grouped products and
 *                             pointwise launches per slice), 5 state in LDS (every other H through score_gru_fwd / _bwd)
 *   bits  4 ..  7  waves      waves per workgroup of that launch (register form: 4; 2 for the H = 32 backward from T = 20 on)
 *   bit   8        direction  0 forward, 1 backward */
int score_gru_last_form(void);

/* Which instance of the fused gather + co-attention kernels (csrc/embed.hip) this process's latest forward launch
 * (backward = 0) and latest backward launch (backward != 0) took: score_coattn_fwd / score_coattn_bwd and the one-grid
 * launches score_forward / score_backward make for the model's two calls.  Host only; each direction's word is written
 * where its launch is decided, read-only, and is -1 before the first launch of that direction (a refused call writes nothing).
 * Forward word:
 *   bit   0        kernel     0 coattn_fwd_kernel (one unit per group), 1 coattn_fwd_kernel_units (a chunk of slices per group)
 *   bits  1 ..  6  KMAX       neighbours the instance unrolls (4, 10, 20, 32)
 *   bits  8 .. 10  SPL / NM   one-unit kernel: float4 slots per lane (1, 2, 4); units kernel: registers per id list (1, 2)
 *   bits 12 .. 27  CH         time slices per chunk of the units kernel; 0 with the one-unit kernel
 * Backward word (coattn_bwd_kernel_t<KMAX, SPL, ATOMIC, NM>):
 *   bits  1 ..  6  KMAX       4, 10, 20, 32
 *   bits  8 .. 10  SPL        float4 slots per lane: the larger of the launch's calls (1, 2, 4; three slots run as 4)
 *   bits 12 .. 14  NM         registers per metadata list, one element per lane (1, 2, 4); 0: every lane reads its own ids
 *   bit  16        ATOMIC     1 the kernel adds the row gradients itself (score_coattn_bwd always), 0 the pull-form scatter follows
 *   bits 20 .. 21  mode       0 co-attention, 1 sum over the neighbours (RCA) */
int score_coattn_last_forms(int32_t backward);

/* The owner's usual way to combine the row gradients it receives: one call per source rank, in rank
 * order, each with that rank's rows (unique inside a call -- they come from score_index_plan's
 * de-duplication) and gradients.  The first writer of a row this step stores, later ones add:
 * out[rows[i], :] (+)= src[i, :], reproducible without a sort or an atomic.  row_flags (required):
 * rows already in state 2 are added to, every row touched ends in state 2 (score_adam_rows). */
int score_rows_accumulate(const int32_t* rows, const float* src, int64_t n, int32_t D, int64_t n_out_rows,
                          float* out, uint8_t* row_flags, void* stream);
/* All source ranks in ONE launch: rows / src hold the sources' lists back to back, source p at [offsets[p], offsets[p+1])
 * (offsets: HOST array of n_sources + 1 entries, offsets[0] = 0; n_sources <= 64), every list unique and ascending (what
 * score_index_plan's unique-row lists are).  The result is bit for bit that of n_sources score_rows_accumulate calls in
 * source order: the slot of the lowest source that names a row adds the later sources' rows in source order (binary search
 * per list) and stores once -- to a row an earlier call left in state 2 it adds what is there FIRST, ((out + g_p0) + g_p1) ...,
 * as the per-source calls do.  D: a multiple of 4 up to 256, else SCORE_E_BADARG (both ops). */
int score_rows_accumulate_multi(const int32_t* rows, const float* src, const int64_t* offsets, int32_t n_sources, int32_t D,
                                int64_t n_out_rows, float* out, uint8_t* row_flags, void* stream);

/* Forward of SCORE / RIA / RCA / SCORE_USER / SCORE_ITEM (score.py:188-369) +
 * build_fc_net / build_logloss / build_l2norm (:68-94).  keep_prob 1.0 = eval
 * (score.py:129), 0.8 = train (:113).  Results land in the workspace
 * (y_pred, loss, ...). drop_mask0/1: optional explicit [B,200]/[B,80] byte masks (SCORE_MODEL_DEEMS: [2,B,200]/[2,B,80]).
 * stage_events: null, or 5 hipEvent_t handles (each may be null) recorded on `stream`
 * at the stage boundaries: [0] before the fused gather+co-attention launch, [1] after
 * it, [2] after the GRUs, [3] after the temporal attention, [4] after head + loss. */
int score_forward(const score_config_t* cfg, const score_state_t* st, const score_batch_t* batch,
                  float reg_lambda, float keep_prob, const uint8_t* drop_mask0,
                  const uint8_t* drop_mask1, uint64_t drop_seed, void* const* stage_events,
                  void* stream);

/* Backward of the same graph: grad_w [n_floats] (overwritten; WITHOUT the L2
 * term, which score_adam adds) and grad_table [n_table_rows, D] (scatter_mode 1: zeroed by
 * the caller, accumulated into; modes 0/2: the rows of the batch are overwritten, see
 * score_state_t.row_flags).  Must follow score_forward on the same workspace/batch (and, to reuse its fork of the context's side
 * stream, on the same stream and context: otherwise the pass records one event more at its start).
 * stage_events: null, or SIX handles: [0] start, [1] after the head, [2] after the temporal
 * attention, [3] after the GRUs, [4] after the co-attention/embedding scatter, [5] after the
 * weight-gradient products (all X^T dY of the pass, as grouped launches: where they ran on the side stream beside the scatter,
 * behind `stream`'s wait for them; the finishers of grad_w are a separate matter, see score_state_t.grads_done_event).
 * grad_w between the two calls: score_backward's zero fill / first writers of grad_w run on the context's side stream, forked
 * where score_forward of the same step began -- i.e. they may execute any time after score_forward was CALLED.  Nothing may
 * read or write grad_w on `stream` (or anywhere else) between score_forward and the completion of score_backward of the same
 * step; the previous step's readers (the optimizer) must be on `stream` before score_forward, or joined into it.            */
int score_backward(const score_config_t* cfg, const score_state_t* st, const score_batch_t* batch,
                   float keep_prob, float* grad_w, float* grad_table, void* const* stage_events,
                   void* stream);

/* ---- line-form ranking pass of the point baselines (csrc/rank.hip) ---------------------------------------------------------
 * A target line is one user and C = 1 + neg_sample_num candidate items.  The reference's loader writes the SAME user_seq,
 * user_seq_length and target_user for all C samples of a line (point_models/data_loader.py:48-85: only target_item differs) and
 * its evaluation loop (train_time_point_models.py:127-154) runs PointBaseModel.eval (point_model.py:101-112) on the expanded
 * batch of B = L * C samples: C identical recurrences (or convolutions) per line.  Here the history encoder runs ONCE per line,
 * at batch size L, and one head launch scores the L * C candidates.
 *
 * SCORE_MODEL_GRU4REC and SCORE_MODEL_CASER only (SCORE_E_SHAPE for every other model type): the two point baselines whose
 * sequence part depends on the user alone and that share the bn1 / fc1 / fc2 / fc3 head (point_model.py:44-52).  bn1 is a
 * per-column affine and fc1 is linear, so fc1's pre-activation splits by the columns of the head input:
 *     z1[l, c] = (fc1/bias + bn1(x_line[l]) . W1[line rows])  +  bn1(target_item[l, c]) . W1[item rows]
 * with x_line = [h | target_user] (Caser: [h, 0, 0, 0 | v2 | target_user]).  The first term is computed once per line, the second
 * per candidate, straight from the table rows.  The results are those of score_forward at keep_prob = 1 on the expanded batch,
 * up to the order of fc1's sum: y_pred [L * C] in the loader's order (sample l * C + c), and loss[0..3] as the workspace's
 * loss region -- loss = log_loss + reg_lambda * l2, log_loss (the mean over the L * C samples, or over
 * score_state_t.global_batch where that is set), l2, and the id status bits.
 *
 * Ids outside [0, feature_size) follow the library's rule: read as row 0, their feed-tuple bit OR-ed into
 * score_state_t.id_status -- 0 for user_seq, 4 for target_user, 5 for cand_items -- and the loss turns NaN.
 * Needs D % 4 == 0 as everywhere, hidden_size % 4 == 0 (GRU4Rec: the item columns of bn1 are read 16 bytes at a time) and
 * L * ceil(C / 16) < 2^31 (SCORE_E_SHAPE beyond).  score_state_t.workspace must hold score_rank_workspace_bytes(cfg, L, C) bytes
 * (SCORE_E_WORKSPACE): the workspace of score_workspace_layout at B = L, and behind it the lines' z1 part [L, 200], the
 * per-sample loss terms [L * C] and a block of zero ids (the index tensors a point model does not have).  Nothing in
 * score_state_t but table, w, workspace, context, id_status, global_batch, gemm_mode, debug_flags and loss_done_event is read. */
typedef struct {
  const int32_t* user_seq;     /* [L, T, Fi]                                                                              */
  const int32_t* length;       /* [L]   user_seq_length (SCORE_MODEL_CASER: required, not read, as in score_forward)       */
  const int32_t* target_user;  /* [L, Fu]                                                                                 */
  const int32_t* cand_items;   /* [L, C, Fi]  a line's candidates, as target_item of the expanded batch lies in memory     */
  const int32_t* label;        /* [L * C]                                                                                 */
  int32_t L, C;
  int32_t active_slices;       /* as score_batch_t.active_slices, for the L histories                                     */
} score_rank_batch_t;

/* *bytes = size of the workspace score_rank_forward needs for L lines of C candidates.  Host only.  SCORE_E_SHAPE for a model
 * type other than GRU4Rec / Caser, SCORE_E_BADARG for L <= 0, C <= 0 or a null pointer. */
int score_rank_workspace_bytes(const score_config_t* cfg, int32_t L, int32_t C, int64_t* bytes);
int score_rank_forward(const score_config_t* cfg, const score_state_t* st, const score_rank_batch_t* rb,
                       float reg_lambda, float* y_pred /* [L*C] */, float* loss /* [4] as workspace.loss */, void* stream);

/* ---- top-K over a whole item catalogue (csrc/catalog.hip) -------------------------------------------------------------------
 * "Which k items of the catalogue does the model put first for this user": the line-form split above with the WHOLE catalogue
 * as every line's candidate set.  The candidate half of fc1's pre-activation then depends on nothing but the catalogue and the
 * weights:
 *     z1[l, n] = zline[l] + zcat[n],     zcat[n] = bn1(item_n) . W1[item rows]
 * score_catalog_build fills zcat [N, 200] (caller-owned) from the table, bn1 and fc1; it is valid until the table or the dense
 * variables change.  score_catalog_topk runs the history encoder at B = L, zline, and then per (line, chunk of the catalogue)
 * one workgroup that holds fc2 / fc3 resident, walks its chunk and keeps its k best; a workgroup per line merges the chunks.
 * SCORE_MODEL_GRU4REC and SCORE_MODEL_CASER only, under the shape conditions of score_rank_forward (SCORE_E_SHAPE otherwise);
 * N <= 2^30.
 *
 * Order: descending fc3 logit (the argument of y_pred's sigmoid: it orders as y_pred does and still separates candidates where
 * the fp32 sigmoid saturates), ties to the lower catalogue index, a NaN logit behind every number.  This is a total order: the
 * result does not depend on the cut into chunks.  An index listed in the line's exclusions is never selected; a line with fewer
 * than k selectable items is filled with index -1 and logit -inf.  1 <= k <= SCORE_CATALOG_KMAX (SCORE_E_BADARG beyond).
 * all_logits (optional) receives every pair's logit at l * N + n, excluded items included.
 * Ids outside the table: read as row 0 and reported in score_state_t.id_status, bit 5 for item_rows (score_catalog_build), bits
 * 0 and 4 for user_seq and target_user.  Every refusal -- a null pointer, L, N <= 0 (SCORE_E_BADARG), model type and shape
 * (SCORE_E_SHAPE), a workspace below score_catalog_plan's workspace_bytes (SCORE_E_WORKSPACE) -- comes before any launch.
 * The workspace: score_workspace_layout at B = L, and behind it zline [L, 200], a block of zero ids and the chunks' lists. */
#define SCORE_CATALOG_KMAX 128
typedef struct {
  const int32_t* item_rows;    /* [N, Fi] device: an item's table rows, as target_item of a sample                            */
  int32_t N;
  float* zcat;                 /* [N, 200] device, caller-owned: written by score_catalog_build, read by score_catalog_topk   */
} score_catalog_t;
typedef struct {
  const int32_t* user_seq;     /* [L, T, Fi]  as score_rank_batch_t                                                           */
  const int32_t* length;       /* [L]                                                                                         */
  const int32_t* target_user;  /* [L, Fu]                                                                                     */
  int32_t L, active_slices;
  const int64_t* excl_off;     /* [L + 1] device offsets into excl_idx, or null: no exclusions                                */
  const int32_t* excl_idx;     /* catalogue indices in [0, N), ascending within a line                                        */
} score_catalog_lines_t;
int score_catalog_build(const score_config_t* cfg, const score_state_t* st, const score_catalog_t* cat, void* stream);
/* The cut of the catalogue, host only and a function of (L, N, k) alone: a scoring workgroup walks `chunk` items (a positive
 * multiple of 16 -- of 32, the step of the scoring kernel), the catalogue falls into nchunk = ceil(N / chunk) chunks.  The rule:
 * chunk = max(256, ceil(N / max(1, floor(512 / L))) rounded up to 32) -- one resident round of at most 512 workgroups where the
 * catalogue is large enough, never fewer than 256 items each; k takes no part in it at present.  *workspace_bytes: what
 * score_state_t.workspace must hold for score_catalog_topk. */
int score_catalog_plan(const score_config_t* cfg, int32_t L, int32_t N, int32_t k, int32_t* chunk, int32_t* nchunk,
                       int64_t* workspace_bytes);
int score_catalog_topk(const score_config_t* cfg, const score_state_t* st, const score_catalog_t* cat,
                       const score_catalog_lines_t* lines, int32_t k, int32_t* top_idx /* [L, k] */, float* top_logit /* [L, k] */,
                       float* all_logits /* [L, N] or null */, void* stream);
/* sizeof / late-field offsets of the two structures above and SCORE_CATALOG_KMAX, for a binding's layout check (as
 * score_abi_struct_sizes): returns the number of values written (6), SCORE_E_BADARG for a null pointer or n too small. */
int score_catalog_struct_sizes(int64_t* out, int32_t n);

/* ---- ... within per-line candidate lists --------------------------------------------------------------------------------------
 * "Which k of THESE items": every line brings a list of catalogue indices -- a category, the items in stock, what a retrieval
 * stage handed over, the 1 + 99 candidates of the sampled evaluation protocol -- and score_catalog_topk_in scores only those
 * pairs, against the same zcat, and returns the k best of them: the order, the -1 / -inf padding, the exclusions (an excluded
 * candidate is never returned) and the bits of a pair's logit are those of score_catalog_topk, wherever the item stands in a list.
 * The list contract: catalogue indices in [0, N), STRICTLY ASCENDING within a line -- no repeats.  A list that breaks it may
 * return an item twice and may miss exclusions; an index outside [0, N) is never selected, reads nothing outside zcat and gets
 * NaN in cand_logits.  Lines may have any length, 0 included (such a line is all padding).
 * max_count sizes the plan -- score_catalog_plan's rule with the longest list in N's place: a scoring workgroup walks `chunk`
 * list positions, and the last of a line's nchunk workgroups walks to the end of the list however long it is, so an understated
 * max_count costs time, never results.  cand_logits (optional) receives every listed pair's logit at its place in cand_idx,
 * excluded candidates included.  Refusals, all before any launch: a null pointer, max_count <= 0, k outside
 * [1, SCORE_CATALOG_KMAX] (SCORE_E_BADARG), a model type other than GRU4Rec / Caser (SCORE_E_SHAPE), a workspace below
 * score_catalog_cands_plan's workspace_bytes (SCORE_E_WORKSPACE). */
typedef struct {
  const int64_t* cand_off;     /* [L + 1] device offsets into cand_idx                                                        */
  const int32_t* cand_idx;     /* catalogue indices in [0, N), strictly ascending within a line; non-null                     */
  int32_t max_count;           /* the plan's size: >= 1; normally the longest line's count                                    */
} score_catalog_cands_t;
int score_catalog_cands_plan(const score_config_t* cfg, int32_t L, int32_t max_count, int32_t k, int32_t* chunk, int32_t* nchunk,
                             int64_t* workspace_bytes);
int score_catalog_topk_in(const score_config_t* cfg, const score_state_t* st, const score_catalog_t* cat,
                          const score_catalog_lines_t* lines, const score_catalog_cands_t* cands, int32_t k,
                          int32_t* top_idx /* [L, k] */, float* top_logit /* [L, k] */,
                          float* cand_logits /* [cand_off[L]] aligned with cand_idx, or null */, void* stream);
/* sizeof(score_catalog_cands_t) and the offsets of its three fields: returns the number of values written (4), SCORE_E_BADARG
 * for a null pointer or n too small. */
int score_catalog_cands_struct_sizes(int64_t* out, int32_t n);

/* ---- ... the exact rank of given items (the counting form) ---------------------------------------------------------------------
 * "Where does item t stand for this user": per line up to SCORE_CATALOG_TMAX target catalogue indices, and for each the number
 * of scored items AHEAD of it.  The same sweep as score_catalog_topk / score_catalog_topk_in with a counter in place of the
 * k-best list: no list, no merge, no [L, N] array.
 * Definitions, for line l, target index t, S_l the scored items -- the whole catalogue (score_catalog_ranks), or the line's
 * candidate list restricted to [0, N) (score_catalog_ranks_in) -- and E_l the line's exclusions (lines->excl_*, unchanged):
 *   ahead      number of n in S_l \ E_l that stand in front of t in score_catalog_topk's order: fc3 logit descending, ties to the
 *              lower catalogue index, NaN behind every number, -0 as +0.  t never counts against itself.  This is the 0-based
 *              place t has, or would have, in an unbounded top-k list of the line, whether or not t is excluded or listed.
 *   tgt_logit  the fc3 logit of the pair (l, t): the bits score_catalog_topk's all_logits holds for it.
 *   state      1: t is in S_l \ E_l.   2: t is in S_l and excluded.   0: t is inside [0, N) but not in S_l (candidate form only;
 *              ahead is still counted against the list).   -1: t is outside [0, N): ahead -1, tgt_logit NaN, nothing scored
 *              for it.
 *   n_scored   [L]: |S_l \ E_l| (a candidate listed twice counts twice; the list contract forbids it).
 * Targets are a CSR pair as the exclusions are: tgt_idx[tgt_off[l] .. tgt_off[l + 1]), in any order, repeats allowed, a line may
 * have none; ahead / tgt_logit / state are aligned with tgt_idx.  At most max_targets per line, 1 <= max_targets <=
 * SCORE_CATALOG_TMAX.  A line with more is a caller error the call survives: its first max_targets are counted, the others get
 * ahead -1, state -1 and NaN, and bit 1 of score_state_t.id_status is set (user_2hop's bit, which no line-form call sets
 * otherwise: its 2-hop ids are a block of zeros).
 * The target logits come from one extra step in every scoring workgroup (the targets' zcat rows through the same fc2 / fc3
 * sums), the counts from integer partials per chunk that a workgroup per line adds: a pure function of the inputs, the same
 * bits every run.  span sizes the plan as N (score_catalog_ranks) or max_count (score_catalog_ranks_in) does: chunk and nchunk
 * are score_catalog_plan's.  Refusals, all before any launch: a null pointer, max_targets outside [1, SCORE_CATALOG_TMAX], L,
 * N, max_count <= 0 (SCORE_E_BADARG), a model type other than GRU4Rec / Caser (SCORE_E_SHAPE), a workspace below
 * score_catalog_ranks_plan's workspace_bytes (SCORE_E_WORKSPACE).  The workspace: score_workspace_layout at B = L, behind it
 * zline [L, 200], a block of zero ids and the chunks' integer partials. */
#define SCORE_CATALOG_TMAX 32
typedef struct {
  const int64_t* tgt_off;      /* [L + 1] device offsets into tgt_idx                                                         */
  const int32_t* tgt_idx;      /* catalogue indices, any order, repeats allowed; outside [0, N): state -1; non-null           */
  int32_t max_targets;         /* 1 .. SCORE_CATALOG_TMAX: no line has more                                                   */
} score_catalog_targets_t;
int score_catalog_ranks_plan(const score_config_t* cfg, int32_t L, int32_t span /* N or max_count */, int32_t* chunk,
                             int32_t* nchunk, int64_t* workspace_bytes);
int score_catalog_ranks(const score_config_t* cfg, const score_state_t* st, const score_catalog_t* cat,
                        const score_catalog_lines_t* lines, const score_catalog_targets_t* targets,
                        int32_t* ahead /* [tgt_off[L]] */, float* tgt_logit /* [tgt_off[L]] */, int32_t* state /* [tgt_off[L]] */,
                        int32_t* n_scored /* [L] */, void* stream);
int score_catalog_ranks_in(const score_config_t* cfg, const score_state_t* st, const score_catalog_t* cat,
                           const score_catalog_lines_t* lines, const score_catalog_cands_t* cands,
                           const score_catalog_targets_t* targets, int32_t* ahead, float* tgt_logit, int32_t* state,
                           int32_t* n_scored, void* stream);
/* sizeof(score_catalog_targets_t), the offsets of its three fields and SCORE_CATALOG_TMAX: returns the number of values written
 * (5), SCORE_E_BADARG for a null pointer or n too small. */
int score_catalog_ranks_struct_sizes(int64_t* out, int32_t n);

/* ---- ... with the users' histories excluded, built on the device (csrc/histexcl.hip) -----------------------------------------
 * score_catalog_lines_t.excl_off / excl_idx for L users of a score_point_log_store_t (declared below): line l's list is the set
 * of catalogue indices j with cat_ids[j] anywhere in user user_ids[l]'s WHOLE segment user_hist_seq[off[u - 1] .. off[u]) -- not
 * only the kept or windowed part -- and cat_ids[j] != keep_ids[l] (keep_ids NULL: nothing is kept back).  Written strictly
 * ascending and without repeats into excl_idx[excl_off[l] .. excl_off[l + 1]); excl_off [L + 1] is exact.  A user id outside
 * 1 .. n_users and a user without events have empty lists.  cat_ids [N]: the catalogue's id column, strictly ascending (signed).
 * Only user_hist_off / user_hist_seq / n_users of the store are read.
 * A pure function of its inputs: a bitmap per (line, range of the catalogue) in LDS, set by binary search per history entry
 * (an idempotent OR, the only atomic), read off in index order; offsets by a count, a reduce-then-scan and a fill.  No host wait,
 * no workgroup waits on another.  If the total exceeds `capacity` (entries of excl_idx) nothing is written at or past it and bit 0
 * of *status is set (other bits and an exact fit leave *status alone: the caller clears it); excl_off stays exact.
 * score_catalog_history_exclusions_plan, host only: *range = catalogue indices a workgroup covers, *n_ranges = ceil(N / range),
 * *threads = history entries a workgroup takes a stride (a segment of any length is walked), *temp_bytes = the workspace;
 * max_events (the longest segment, >= 0) takes no part in the rule at present.  Any of the four pointers may be NULL.
 * Refusals, all before any launch: a null pointer, struct_bytes, L, N <= 0, capacity < 0 (SCORE_E_BADARG); L * n_ranges >= 2^31
 * (SCORE_E_SHAPE); temp_bytes below the plan's (SCORE_E_WORKSPACE). */
/* (score_catalog_history_exclusions itself is declared behind the store's struct, below) */
int score_catalog_history_exclusions_plan(int32_t L, int32_t N, int64_t max_events, int32_t* range, int32_t* n_ranges,
                                          int32_t* threads, int64_t* temp_bytes);

/* ---- one training step in one call (csrc/step.hip) -----------------------------------------------------------------------
 * The steady-state step of model.train (score.py:101-116) for a caller that runs the time-tiled table optimizer with the
 * look-ahead (score_adam_catchup_ids_through) and sorts the next batch's index plan a step ahead: exactly
 *   wait(ev_ahead), wait(ev_sweep)                                   [stream]   if wait_ahead / wait_sweep
 *   score_forward(..., loss_host, loss_done_event = ev_loss if loss_host)                   [stream]
 *   score_backward(plan_done_event = ev_plan, grads_done_event = ev_grads, stage event 4 = ev_b4)   [stream]
 *   wait(ev_grads); score_adam_touched_and_dense(step, alpha, l2 = reg_lambda)              [stream]
 *   wait(ev_b4); score_adam_catchup_ids_through(next ids, step, alpha); record(ev_ahead);
 *                score_index_plan(next batch -> next_workspace); record(ev_plan)            [side_stream]   if next_batch
 *                score_adam_catchup_rows(slice); record(ev_sweep)                           [side_stream]   if slice_hi > slice_lo
 *   (in this order of CALLS; on the device the side stream's work runs beside the optimizer launch)
 * -- the same entry points with the same arguments a caller would use one by one (the events are the caller's, re-used from
 * call to call: every wait above is issued before the same call re-records its event).  PRECONDITIONS the caller guarantees:
 * the batch's rows are up to date through step - 1 (the previous call named this batch as next_batch, or the caller ran
 * score_adam_catchup_ids), ev_plan is recorded behind THIS batch's index plan in st->workspace, no row is in state 2.
 * What it saves is host time between the calls (the reference's own batch sizes are bound by it), nothing on the device. */
typedef struct {
  const score_adam_table_t* table;                       /* the embedding table's optimizer state (g = grad_table of the passes) */
  float* w; float* w_m; float* w_v; float* w_g;          /* flat dense variables, their Adam slots and gradient [n_w]           */
  int64_t n_w, n_reg;
  int32_t* skipped;                                      /* optional score_guard_t.skipped                                      */
  float reg_lambda, keep_prob, alpha;
  uint32_t step;                                         /* the optimizer step being applied (1-based)                          */
  uint64_t drop_seed;
  int64_t slice_lo, slice_hi; uint32_t slice_upto;       /* the window slice of this step (score_adam_catchup_rows)             */
  int32_t wait_ahead, wait_sweep;
  const score_batch_t* next_batch; const int32_t* next_ids; int64_t n_next_ids;      /* optional: the batch the NEXT call trains on */
  float* next_workspace; int64_t next_workspace_bytes;
  float* loss_host;                                      /* optional, see score_state_t.loss_host                               */
  void* side_stream;
  void* ev_ahead; void* ev_sweep; void* ev_plan; void* ev_stage2 /* unused */; void* ev_b4; void* ev_grads; void* ev_loss;   /* hipEvent_t */
  void* ev_plan_next;     /* optional hipEvent_t.  Given (and next_workspace a DIFFERENT workspace than st->workspace: the caller
                             alternates two): the next batch's index plan is queued FIRST on the side stream, with no wait, and
                             this event recorded behind it -- the sort runs beside this step's passes.  NULL: one workspace, the
                             plan behind this step's scatter, ev_plan re-recorded (the sequence above).                         */
  void* const* fwd_stage_events;   /* optional: score_forward's stage_events (five hipEvent_t or NULL each) -- a caller timing the pass */
  void* plan_stream;      /* optional: a third stream for that early plan (it waits for ev_b4's previous record first); NULL: the
                             side stream -- the look-ahead catch-up then queues behind the sort.                                */
} score_train_step_t;
int score_train_step(const score_config_t* cfg, const score_state_t* st, const score_batch_t* batch, const score_train_step_t* p,
                     void* stream);

/* sizeof of every struct above in the header's order (score_step_scalars_t, score_config_t, score_param_entry_t, score_batch_t,
 * score_workspace_t, score_guard_t, score_adam_table_t, score_state_t, score_train_step_t, score_graph_t, score_batch_out_t), then
 * offsetof(score_state_t, plan_workspace), offsetof(score_train_step_t, plan_stream), offsetof(score_adam_table_t, skipped_steps):
 * a binding in another language checks its own structures against these before its first call.  Returns how many values it
 * wrote (out needs room for at least that many: SCORE_E_BADARG otherwise).  Host only. */
int score_abi_struct_sizes(int64_t* out, int32_t n);

/* ---- "next" row f1: batch assembly on the device -------------------------------------- */

/* In-memory temporal bipartite graph (replaces the MongoDB documents {uid|iid,'1hop','2hop'} of
 * graph_storage.py:78-246).  CSR over (entity, time slice): the neighbours of 0-based entity e in
 * slice t are nbr[off[e*S + t] .. off[e*S + t + 1]).  Ids follow feateng_tmall.py:72-101: users
 * 1..U, items U+1..U+I.  user_rows [U, Fu] / item_rows [I, Fi] hold [id, side features...]. */
typedef struct {
  const int64_t* user_off1; const int32_t* user_nbr1;   /* user -> items it interacted with   */
  const int64_t* user_off2; const int32_t* user_nbr2;   /* user -> co-interacting users        */
  const int64_t* item_off1; const int32_t* item_nbr1;   /* item -> users                       */
  const int64_t* item_off2; const int32_t* item_nbr2;   /* item -> co-interacted items         */
  const int32_t* user_rows; const int32_t* item_rows;
  int32_t n_users, n_items, time_slice_num, user_fnum, item_fnum;
  /* GraphHandler mode (graph_loader.py:243-247, set per data set at train_score.py:295-301): 0 = 'rs', 2-hop neighbours
   * drawn uniformly (:192); 1 = 'is', drawn with probability softmax_j(1 / (degree_j - 1)) (:118-120), degree_j being
   * the slice degree of the 1-hop neighbour that 2-hop entry j was reached through (the 'degrees' lists of
   * graph_storage.py:172-176).  user_deg2 / item_deg2 are aligned with user_nbr2 / item_nbr2 (mode 1 only). */
  int32_t sample_mode;
  const int32_t* user_deg2; const int32_t* item_deg2;
} score_graph_t;

typedef struct {   /* the 8-tuple of graph_loader.py:383, device int32, B = n_lines * (1 + neg) */
  int32_t* user_1hop; int32_t* user_2hop; int32_t* item_1hop; int32_t* item_2hop;
  int32_t* target_user; int32_t* target_item; int32_t* label; int32_t* length;
} score_batch_out_t;

/* GraphHandler.gen_{user,item}_history + GraphLoader.worker (graph_loader.py:169-277, 340-383, mode
 * 'rs'): uids [n_lines], iids [n_lines*(1+neg)] (positive first).  1-hop lists are truncated /
 * cyclically padded exactly as the reference does; 2-hop lists are sampled K times with replacement
 * (uniformly, or degree-weighted in mode 'is': score_graph_t.sample_mode) from a counter-based generator
 * (`seed`), so draws differ from NumPy's but have its distribution. */
int score_batch_assemble(const score_graph_t* g, const int32_t* uids, const int32_t* iids,
                         int32_t n_lines, int32_t neg_sample_num, int32_t T, int32_t K,
                         int32_t start_time, int32_t pred_time, uint64_t seed,
                         const score_batch_out_t* out, void* stream);

/* ---- point baselines: batch assembly from a device-resident sequence store ------------------- */

/* The files of point_models/data_loader.py parsed once (score_amd/pointdata.py, PointSeqStore), device int32 / int64.
 * Line l of the target file: its user history is user_seq[user_off[l] .. user_off[l + 1]) -- the LAST max_len ids of the line,
 * at least one, each the ROW of that item in item_rows -- and user_len[l] its untruncated length.  The dual form (DataLoaderDualSeq)
 * adds one history per sample: item_seq[item_off[l * per_line + c] ..) rows of user_rows, item_len[l * per_line + c]; NULL in
 * the single form.  target_user [n_lines] / target_item [n_lines * per_line] are rows of user_rows [n_user_rows, Fu] /
 * item_rows [n_item_rows, Fi], which hold [id, side features...].  struct_bytes = sizeof(score_point_store_t): the call
 * refuses any other value (this struct's own size check; score_abi_struct_sizes does not list it). */
typedef struct {
  int64_t struct_bytes;
  const int64_t* user_off; const int32_t* user_seq; const int32_t* user_len;
  const int64_t* item_off; const int32_t* item_seq; const int32_t* item_len;
  const int32_t* target_user; const int32_t* target_item;
  const int32_t* user_rows; const int32_t* item_rows;
  int64_t n_lines, n_user_rows, n_item_rows;
  int32_t per_line, max_len;
} score_point_store_t;

/* One batch of DataLoaderUserSeq / DataLoaderDualSeq (data_loader.py:15-87, 89-185) in ONE launch: target lines
 * [first_line, first_line + n_lines) of the store, B = n_lines * per_line samples, into the flat batch layout.
 * user_1hop = user_seq as [B, T, 1, Fi] (a history shorter than T is padded by repeating its last id), length = the untruncated
 * user length, target_user / target_item, label = 1 for a line's first sample and 0 for the others.  length2 != NULL: the dual
 * form -- item_1hop = item_seq as [B, T, 1, Fu] and length2 = item_seq_length (the store must hold the item side).  Every
 * tensor the point model does not use (user_2hop, item_2hop, and item_1hop in the single form) is written as zeros by the
 * same launch.  T * Fi and T * Fu may not exceed 8192 words (SCORE_E_SHAPE); T must equal the store's max_len, per_line
 * its per_line. */
int score_point_batch_assemble(const score_point_store_t* store, int64_t first_line, int32_t n_lines, int32_t per_line,
                               int32_t T, int32_t Fu, int32_t Fi, const score_batch_out_t* out, int32_t* length2,
                               void* stream);

/* ---- point baselines: per-entity histories from the interaction log, and batches from them ---- */

/* One side's histories straight from the remapped log (gen_target.py:223-275 gen_user_item_hist_dict_*, then
 * gen_history_point.py:22-65's cut to the last MAX_LEN ids), device arrays.  ent / other / time_key / t_idx [n_events]: the
 * entity whose history an event joins (users: uid), the id it contributes (iid), a non-negative key below 2^time_bits that
 * orders events as the reference's time_int does, and the slice index; events with start_time <= t_idx < pred_time and
 * id_lo <= ent < id_lo + n_ent count.  Entity e = ent - id_lo: its history, ordered by (time_key, position in the log) as
 * Python's stable sorted orders it, is seq[off[e] .. off[e + 1]); len[e] = min(its count, hist_max_len), and the KEPT
 * history is the last len[e] ids of it.  off int64 [n_ent + 1], seq int32 [n_events] (off[n_ent] words are used, the rest
 * is zero), len int32 [n_ent].  A stable sort (score_sort_pairs: once where bits(n_ent) + time_bits <= 32, else by time and
 * then by entity) and one kernel of binary searches; no atomics, so the output is a pure function of the input.
 * n_events < 2^31 (SCORE_E_SHAPE); temp: score_point_hist_temp_bytes(n_events) (SCORE_E_WORKSPACE). */
int score_point_hist_build(const int32_t* ent, const int32_t* other, const int32_t* time_key, const int32_t* t_idx,
                           int64_t n_events, int32_t start_time, int32_t pred_time, int32_t id_lo, int32_t n_ent,
                           int32_t time_bits, int32_t hist_max_len, int64_t* off, int32_t* seq, int32_t* len,
                           void* temp, int64_t temp_bytes, void* stream);
int64_t score_point_hist_temp_bytes(int64_t n_events);

/* Both sides' histories and the target lines (score_amd/pointdata.py, PointLogStore), device int32 / int64.  Users are the
 * ids 1 .. n_users (row id - 1 of user_rows [n_users, Fu]), items n_users + 1 .. n_users + n_items (row id - 1 - n_users of
 * item_rows [n_items, Fi]).  line_user [n_lines], line_items [n_lines * per_line] (a line's positive, then its negatives),
 * line_last_item [n_lines] (the line's last item AS WRITTEN, which may lie behind the first per_line).  The item side and
 * line_last_item may be NULL in the single form.  struct_bytes = sizeof(score_point_log_store_t): the call refuses any other
 * value (this struct's own size check; score_abi_struct_sizes does not list it). */
typedef struct {
  int64_t struct_bytes;
  const int64_t* user_hist_off; const int32_t* user_hist_seq; const int32_t* user_hist_len;
  const int64_t* item_hist_off; const int32_t* item_hist_seq; const int32_t* item_hist_len;
  const int32_t* line_user; const int32_t* line_items; const int32_t* line_last_item;
  const int32_t* user_rows; const int32_t* item_rows;
  int64_t n_lines, n_users, n_items;
  int32_t per_line, hist_max_len;
} score_point_log_store_t;

/* score_point_batch_assemble from a score_point_log_store_t: the same launch shape, the same output, the same error codes and
 * shape limits.  A sample's history is found through its entity's id and is the last min(len, T) ids of the kept history,
 * padded by repeating the last; length = len of the line's user; the dual form's length2 = len of the sample's item, 1 for an
 * item without history, whose sequence is zeros (the reference's one-element history [0]); id 0 anywhere is a row of zeros
 * (the reference needs a key '0' in its feature dictionary for that).  target_user is the line's user in the single form; in
 * the dual form it is the last id of the kept history of line_last_item (DataLoaderDualSeq's rebinding), zeros where that
 * item has none.  T is free: one store serves every T with T * Fi, T * Fu <= 8192. */
int score_point_batch_assemble_log(const score_point_log_store_t* store, int64_t first_line, int32_t n_lines, int32_t per_line,
                                   int32_t T, int32_t Fu, int32_t Fi, const score_batch_out_t* out, int32_t* length2,
                                   void* stream);

/* Lines for arbitrary users, one launch that writes these four tensors and nothing else: for line l with user u = user_ids[l]
 * exactly what score_point_batch_assemble_log writes for the first sample of a single-form line whose line_user is u -- the last
 * min(user_hist_len[u - 1], T) ids of the kept history as rows of item_rows, padded by repeating the last; length =
 * user_hist_len[u - 1]; target_user = user_rows[u - 1] -- and known[l] = 1.  A user of 1 .. n_users without events is a cold
 * user: zeros, length 0, known 1.  An id outside 1 .. n_users: zeros, length 0, known 0.  The same user may occur several times.
 * Plain stores, no atomics.  The user side and the two row tables are required; line_user, line_items, line_last_item and the
 * item side may be NULL.  Refusals, all before the launch: a null pointer, struct_bytes, L, T, Fu, Fi <= 0 (SCORE_E_BADARG);
 * T * Fi > 8192, L * T * Fi >= 2^31 (SCORE_E_SHAPE). */
int score_point_user_lines(const score_point_log_store_t* store, const int32_t* user_ids, int32_t L, int32_t T, int32_t Fu,
                           int32_t Fi, int32_t* user_seq /* [L, T, Fi] */, int32_t* length /* [L] */,
                           int32_t* target_user /* [L, Fu] */, int32_t* known /* [L] */, void* stream);

/* The L users' history exclusions for score_catalog_topk / score_catalog_topk_in (csrc/histexcl.hip; the contract stands with
 * score_catalog_history_exclusions_plan, above). */
int score_catalog_history_exclusions(const score_point_log_store_t* store, const int32_t* user_ids,
                                     const int32_t* keep_ids /* [L] or NULL */, int32_t L,
                                     const int32_t* cat_ids /* [N], strictly ascending */, int32_t N,
                                     int64_t* excl_off /* [L + 1] */, int32_t* excl_idx, int64_t capacity, int32_t* status,
                                     void* temp, int64_t temp_bytes, void* stream);

/* ---- the temporal graph store from the behaviour log, on the device (csrc/graphbuild.hip) ---- */

/* What TemporalGraph.from_log(draws="cell") builds (graph_storage.py:93-246 with per-cell counter-based draws), as device
 * arrays.  uid / iid / t_idx int32 [n_events]: the remapped log (users 1 .. n_users, items n_users + 1 .. n_users + n_items,
 * slices 0 .. time_slice_num - 1); an event with ANY of the three outside its range joins no cell on either side.  Cell
 * c = e * time_slice_num + t of 0-based entity e.  user_off1 int64 [n_users * S + 1], item_off1 int64 [n_items * S + 1],
 * user_nbr1 / item_nbr1 int32 [n_events] (off1[last] words are used, the rest is zero).
 * The draw rule: G = 0x9E3779B97F4A7C15, mix = the finaliser of splitmix64,
 *   key(seed, tag, c, j) = mix(mix(seed + G * ((tag << 40) + c + 1)) + G * (j + 1)) >> 32,
 * tag 0 item shuffle, 1 item down-sample, 2 user shuffle, 3 user down-sample; the random order of n positions is the
 * positions sorted by (key, position).  struct_bytes = sizeof(score_graph_build_t): the calls refuse any other value.
 * Limits: n_events, n_users * S, n_items * S, n_users + n_items < 2^31 and max_1hop^2 <= 4096 (SCORE_E_SHAPE beyond); temp:
 * score_graph_build_temp_bytes (SCORE_E_WORKSPACE, before any launch).  One workspace serves all calls of a build, and has to:
 * the sorted cell keys of score_graph_build_1hop stay in it for the 2-hop calls. */
typedef struct {
  int64_t struct_bytes;
  const int32_t* uid; const int32_t* iid; const int32_t* t_idx;
  int64_t n_events;
  int32_t n_users, n_items, time_slice_num, max_1hop, max_2hop, reserved;
  uint64_t seed;
  int64_t* user_off1; int32_t* user_nbr1; int64_t* item_off1; int32_t* item_nbr1;
} score_graph_build_t;

int64_t score_graph_build_temp_bytes(int64_t n_events, int32_t n_users, int32_t n_items, int32_t time_slice_num);

/* Both sides' 1-hop CSRs in log order: a stable score_sort_pairs by cell and a binary search per cell.  No host wait. */
int score_graph_build_1hop(const score_graph_build_t* g, void* temp, int64_t temp_bytes, void* stream);

/* One side's 2-hop and degree lists (item_side: 1 items, 0 users), in two calls.
 *   nbr2 == NULL: the side's cells with more than max_1hop entries are put in their random order in place (two
 *     score_sort_pairs over their entries only), every cell's capped 2-hop length is counted and scanned into off2
 *     int64 [n_ent * S + 1], and *total (host) receives off2's last word.  Waits for the stream twice.
 *   nbr2 != NULL: nbr2 / deg2 int32 [cap2 >= total] are filled from off2; nothing is written past cap2.  No host wait.
 * A cell walks the first min(len, max_1hop) entries x of its stored list; x's cell of the same slice, of full length d > 1,
 * contributes its first min(d, max_1hop) stored entries and d once per entry; more than max_2hop candidates keep the first
 * max_2hop of their random order.  The reference's pass order is the caller's: items (both calls), then users -- the item
 * fill reads user lists still in log order, the user fill reads item lists as the item pass left them. */
int score_graph_build_2hop(const score_graph_build_t* g, int32_t item_side, int64_t* off2, int32_t* nbr2, int32_t* deg2,
                           int64_t cap2, int64_t* total, void* temp, int64_t temp_bytes, void* stream);

/* ---- the target lines from the behaviour log, on the device (csrc/targetgen.hip) ---- */

/* What dataprep.gen_target_lines(draws="cell") yields (gen_target.py:79-121, with sampling.py:31-37's down-sampling folded
 * in), as device arrays.  uid / iid / t_idx int32 [n_events]: the remapped log; an event whose uid lies outside 1 .. n_users,
 * whose iid outside n_users + 1 .. n_users + n_items or whose slice is negative is dropped.  User u gets a line iff it has an
 * event in slice pred_time and one in [start_time, pred_time) and, where sample_factor > 1,
 * (key(seed, 6, u, 0) * sample_factor) >> 32 == 0 (sample_factor 0 or 1: no down-sampling).  Lines come in ascending user id:
 * line_user int32 [n_lines], line_items int32 [n_lines, 1 + neg_sample_num] = the user's first item of slice pred_time in log
 * order, then negative j = n_users + 1 + ((key(seed, 4, u, j) * n_items) >> 32), or, with a pop list (pop_items != NULL,
 * device int32 [n_pop], n_pop > 0 wherever a line is filled), pop_items[(key(seed, 5, u, j) * n_pop) >> 32]; key is the
 * graph build's, its cell the user id, the products 64-bit.  struct_bytes = sizeof(score_target_build_t): the calls refuse any
 * other value.  Limits: n_events, n_users + n_items < 2^31 and 1 + neg_sample_num <= 4096 (SCORE_E_SHAPE beyond); temp:
 * score_target_build_temp_bytes (SCORE_E_WORKSPACE); both before any launch.  One workspace serves both calls of a build.
 * Tile sizes (a test puts event counts at their edges): the prefix sum works on SCORE_TARGET_SCAN_TILE words per workgroup,
 * score_sort_pairs on SCORE_TARGET_SORT_TILE pairs. */
#define SCORE_TARGET_SCAN_TILE 4096
#define SCORE_TARGET_SORT_TILE 8192
typedef struct {
  int64_t struct_bytes;
  const int32_t* uid; const int32_t* iid; const int32_t* t_idx;
  int64_t n_events;
  int32_t n_users, n_items, start_time, pred_time, neg_sample_num, sample_factor;
  uint64_t seed;
  const int32_t* pop_items; int64_t n_pop;
} score_target_build_t;

int64_t score_target_build_temp_bytes(int64_t n_events, int32_t n_users);

/* In two calls.
 *   line_user == NULL: the events of slice pred_time are sorted by user (a stable score_sort_pairs on (uid, log position), every
 *     other event behind a sink key, so a run's head is the user's first event of the slice), users with history are marked
 *     by plain stores of one constant, the heads that get a line are flagged and scanned to their line index, and *n_lines
 *     (host) receives the count.  Waits for the stream once.
 *   line_user != NULL: one kernel evaluates the keys and fills line_user / line_items of lines 0 .. min(n_lines, cap_lines) - 1
 *     from what the first call left in temp, 16 bytes per store where a line's words allow it; nothing is written at or past
 *     line cap_lines.  No host wait.
 * No atomics, no workgroup waits on another: the output is a pure function of the input. */
int score_target_build(const score_target_build_t* a, int32_t* line_user, int32_t* line_items, int64_t cap_lines,
                       int64_t* n_lines, void* temp, int64_t temp_bytes, void* stream);

/* How often score_target_build and score_target_build_lists have waited for a stream in this process so far (host only): one
 * per count call, none per fill. */
int score_target_host_waits(void);

/* CCMR's target rule (gen_target.py:79-96; dataprep.gen_target_lines(draws="cell", neg_lists=...)): score_target_build with the
 * users' own negatively rated items in front of the draws.  neg_off int64 [n_users + 1] and neg_items int32 [n_neg] are a CSR
 * over uid = 1 .. n_users (score_neg_lists_build): negative j of user u is neg_items[neg_off[u - 1] + j] where
 * j < neg_off[u] - neg_off[u - 1], otherwise the draw score_target_build makes at position j (the same key, tag and j, so with
 * empty lists the output is score_target_build's word for word, and under one seed a user's padding is the same for every
 * pred_time).  Eligibility, the positive and the line order come from `build` alone.  struct_bytes =
 * sizeof(score_target_lists_t) and build.struct_bytes = sizeof(score_target_build_t): the calls refuse any other value.  The
 * same two calls (count: one stream wait; fill: none, 16-byte stores where a line's words allow, nothing at or past
 * cap_lines), limits and workspace (score_target_build_temp_bytes) as score_target_build; n_neg < 2^31 (SCORE_E_SHAPE).  A list
 * whose bounds do not lie in 0 .. n_neg in ascending order is taken as empty. */
typedef struct {
  int64_t struct_bytes;
  score_target_build_t build;
  const int64_t* neg_off; const int32_t* neg_items; int64_t n_neg;
} score_target_lists_t;

int score_target_build_lists(const score_target_lists_t* a, int32_t* line_user, int32_t* line_items, int64_t cap_lines,
                             int64_t* n_lines, void* temp, int64_t temp_bytes, void* stream);

/* user_neg_dict (feateng_ccmr.py:173-183; targets.UserNegLists) from the negative events neg_uid / neg_iid int32 [n_neg] in log
 * order: off int64 [n_users + 1], items int32 [n_neg]; the items of uid u are items[off[u - 1] .. off[u]) in log order,
 * duplicates kept.  An event whose uid lies outside 1 .. n_users joins no list: off[n_users] words of items are used, the rest
 * is zero.  A stable score_sort_pairs on (uid, log position), a gather and a binary search per user; no host wait; n_neg = 0
 * is allowed (off is all zero).  temp: score_neg_lists_temp_bytes(n_neg) (SCORE_E_WORKSPACE, before any launch). */
int64_t score_neg_lists_temp_bytes(int64_t n_neg);
int score_neg_lists_build(const int32_t* neg_uid, const int32_t* neg_iid, int64_t n_neg, int32_t n_users, int64_t* off,
                          int32_t* items, void* temp, int64_t temp_bytes, void* stream);

/* The popular-item list (gen_target.py:277-290, dataprep.gen_pop_items): the ids n_users + 1 + i, ascending, of the items i
 * with at least pop_standard non-empty slices in item_off1 int64 [n_items * time_slice_num + 1] (a graph's item side) and
 * id <= max_iid.  struct_bytes = sizeof(score_pop_items_t).  Two calls like score_target_build: pop_items == NULL counts
 * (flags, a scan, *n_pop on the host: one stream wait), pop_items != NULL compacts in id order into int32 [cap_pop], writing
 * nothing at or past cap_pop.  n_items * time_slice_num, n_users + n_items < 2^31 (SCORE_E_SHAPE); temp:
 * score_pop_items_temp_bytes (SCORE_E_WORKSPACE). */
typedef struct {
  int64_t struct_bytes;
  const int64_t* item_off1;
  int32_t n_users, n_items, time_slice_num, pop_standard, max_iid, reserved;
} score_pop_items_t;

int64_t score_pop_items_temp_bytes(int32_t n_items);
int score_pop_items(const score_pop_items_t* a, int32_t* pop_items, int64_t cap_pop, int64_t* n_pop, void* temp,
                    int64_t temp_bytes, void* stream);

/* ---- the raw log's remap on the device (csrc/logremap.hip) --------------------------------------- */
/* feateng_tmall.py:30-133 / feateng_taobao.py:16-88 (dataprep.remap_tmall_log / remap_taobao_log): n_cols <= 8 raw int32 columns
 * of n_events events, each one vocabulary.  The vocabularies are numbered one behind the other from 1 in column order, the
 * values of a column in order of FIRST APPEARANCE in the log: ids[c][pos] = base_c + rank of the value's first log position
 * among the column's distinct values, base_0 = 1, base_{c+1} = base_c + counts[c].  Per column a stable score_sort_pairs on
 * (the value's 32-bit pattern, log position), two prefix sums and plain stores; the bases ride in a device word, so the whole
 * remap waits for the stream ONCE, for the counts.  key_bits (1 .. 32): every column's patterns must fit it (a negative value
 * needs 32); one that does not is found on the device and the count call returns SCORE_E_BADARG after its wait.
 * Up to two feature-row tables: a table names an entity column and up to seven feature columns, and row id_e - base_e is
 * [id_e, id_f1[last], id_f2[last], ...] with `last` the entity's LAST log position ("later rows overwrite earlier ones": the
 * dict assignments of feateng_tmall.py:130-131 and feateng_taobao.py:81).
 * struct_bytes = sizeof(score_log_remap_t): the calls refuse any other value.  Limits: n_events < 2^31, 1 + the sum of the
 * counts < 2^31 (SCORE_E_SHAPE; the latter after the count call's wait); temp: score_log_remap_temp_bytes (SCORE_E_WORKSPACE,
 * before any launch).  One workspace serves both calls. */
#define SCORE_LOG_REMAP_MAX_COLS 8
#define SCORE_LOG_REMAP_MAX_TABLES 2
#define SCORE_LOG_REMAP_MAX_FEATS 7
typedef struct {
  int32_t entity, n_feat;                      /* column indices; the row is 1 + n_feat words wide */
  int32_t feat[SCORE_LOG_REMAP_MAX_FEATS];
  int32_t reserved;
} score_log_table_t;

typedef struct {
  int64_t struct_bytes;
  const int32_t* cols[SCORE_LOG_REMAP_MAX_COLS];   /* DEVICE int32 [n_events] each: the raw columns          */
  int32_t* ids[SCORE_LOG_REMAP_MAX_COLS];          /* DEVICE int32 [n_events] each: the remapped columns     */
  int64_t n_events;
  int32_t n_cols, key_bits, n_tables, reserved;
  score_log_table_t tables[SCORE_LOG_REMAP_MAX_TABLES];
} score_log_remap_t;

int64_t score_log_remap_temp_bytes(int64_t n_events, int32_t n_cols);

/* In two calls.
 *   rows == NULL: writes ids[c] for every column and counts[0 .. n_cols) (HOST int64), and leaves every table entity's last
 *     log position per row in temp.  Waits for the stream once.
 *   rows != NULL: HOST array of n_tables DEVICE pointers, rows[t] int32 [cap_rows[t], 1 + n_feat]; fills them from what the
 *     first call left in temp and the ids it wrote (which must still be there), 16 bytes per store where a row is a multiple
 *     of four words; nothing is written at or past row cap_rows[t].  No host wait.
 * No atomics, no workgroup waits on another: the output is a pure function of the input. */
int score_log_remap(const score_log_remap_t* a, int32_t* const* rows, const int64_t* cap_rows, int64_t* counts, void* temp,
                    int64_t temp_bytes, void* stream);

/* The time slices of a raw log, element-wise; no host wait.
 *   SCORE_LOG_SLICES_TMALL (feateng_tmall.py:10-11,53-56): time = MMDD as an integer; t_idx = floor((day of 2015 - day of
 *     05-01) / 15), negative before May 1 (floor, as Python's //).  A month outside 1 .. 12 or a day outside the month (2015 has
 *     no February 29) sets *status (DEVICE int32, zeroed by the caller, sticky) to 1.  flag / keep / start_ts .. delta unused.
 *   SCORE_LOG_SLICES_EPOCH (feateng_taobao.py:27-32): keep[i] = start_ts <= time[i] <= end_ts (both inclusive) and, where flag
 *     is given, flag[i] != 0; t_idx = (time - start_ts) / delta for kept events, -1 for the others.  delta > 0. */
#define SCORE_LOG_SLICES_TMALL 0
#define SCORE_LOG_SLICES_EPOCH 1
int score_log_slices(int32_t mode, const int32_t* time, const int32_t* flag, int64_t n_events, int32_t start_ts, int32_t end_ts,
                     int32_t delta, int32_t* t_idx, int32_t* keep, int32_t* status, void* stream);

/* Stable compaction of n_cols <= 8 columns by keep flags (any non-zero word keeps): cols_in / cols_out are HOST arrays of DEVICE
 * pointers, cols_out[c] int32 [cap]; kept_pos (optional) int32 [cap] receives the kept events' log positions.  A prefix sum,
 * *n_kept (HOST) after one stream wait, then one scatter -- not launched when nothing is kept; nothing is written at or past cap.
 * temp: score_log_compact_temp_bytes(n_events). */
int64_t score_log_compact_temp_bytes(int64_t n_events);
/* How often score_log_remap and score_log_compact have waited for a stream in this process so far (host only): a test takes
 * the difference around a call -- one per count call and per compaction, none per fill. */
int score_log_host_waits(void);
int score_log_compact(const int32_t* const* cols_in, int32_t* const* cols_out, int32_t n_cols, const int32_t* keep,
                      int64_t n_events, int32_t* kept_pos, int64_t cap, int64_t* n_kept, void* temp, int64_t temp_bytes,
                      void* stream);

/* ---- CCMR's rating log on the device (csrc/ccmr.hip) ------------------------------------------------ */
/* feateng_ccmr.py:24-44,119-171 (dataprep.remap_ccmr_log) in one call without a host wait.  user / item / rating / date int32
 * [n_events]: the raw log, date = YYYYMMDD as an integer.  Per event: uid = user + 1, iid = item + 1 + n_users, day =
 * the date's day number (datetime.date.toordinal(): 0001-01-01 is 1; integer civil-date arithmetic, no table), t_idx =
 * (day - start_day) / delta_days truncated TOWARDS ZERO (a date 1 .. delta_days - 1 days before the start lies in slice 0),
 * keep_pos = 1 iff rating is 4 or 5, keep_neg = 1 for every other rating.  A date datetime.date refuses (year outside 1 .. 9999,
 * month, day of the month, February 29 outside a leap year), a user outside [0, n_users) or an item outside [0, n_items) sets
 * its status word to 1; that event gets zeros, slice -1 and neither flag.
 * movie[0 .. 4] int32 [n_movies]: raw item, first director, actor, genre, nation of a movie_info line, -1 = empty.  item_rows
 * int32 [n_items, 5] = [iid, did, aid, gid, nid] from the item's FIRST line (feateng_ccmr.py:167): a present feature f of
 * field k is 1 + f + n_users + n_items + vocab[0] + .. + vocab[k - 1], an empty one the field's last id n_users + n_items +
 * vocab[0] + .. + vocab[k]; vocab counts that "none" entry, so f must lie in [0, vocab[k] - 1).  An item without a line gets the
 * four "none" ids.  status int32 [SCORE_CCMR_STATUS_WORDS] (DEVICE, zeroed by the call): SCORE_CCMR_ST_MISSING receives the
 * number of items that occur among the positive events and have no line, the other words 0 or 1.
 * struct_bytes = sizeof(score_ccmr_prep_t).  Limits: n_events, n_movies, 1 + n_users + n_items + the vocabularies < 2^31
 * (SCORE_E_SHAPE); temp: score_ccmr_prep_temp_bytes (SCORE_E_WORKSPACE); both before any launch.  n_movies = 0 is allowed. */
#define SCORE_CCMR_STATUS_WORDS 8
#define SCORE_CCMR_ST_DATE 0
#define SCORE_CCMR_ST_USER 1
#define SCORE_CCMR_ST_ITEM 2
#define SCORE_CCMR_ST_MOVIE_ITEM 3
#define SCORE_CCMR_ST_FEATURE 4
#define SCORE_CCMR_ST_MISSING 5
typedef struct {
  int64_t struct_bytes;
  const int32_t* user; const int32_t* item; const int32_t* rating; const int32_t* date;
  const int32_t* movie[5];
  int64_t n_events, n_movies;
  int32_t n_users, n_items, vocab[4], start_day, delta_days;
  int32_t* uid; int32_t* iid; int32_t* t_idx; int32_t* day; int32_t* keep_pos; int32_t* keep_neg;
  int32_t* item_rows; int32_t* status;
} score_ccmr_prep_t;

int64_t score_ccmr_prep_temp_bytes(int64_t n_movies, int32_t n_items);
int score_ccmr_prep(const score_ccmr_prep_t* a, void* temp, int64_t temp_bytes, void* stream);

/* ---- "next" row f4: ranking metrics of an evaluation pass on the device ----------------------- */

/* get_ranking_quality (train_score.py:104-142) without the host round trip of the predictions:
 * pred / ids are [n_lines, per_line] (one positive in column 0 + the sampled negatives, the layout
 * model.eval's outputs arrive in, train_score.py:153-157).  The rank of a line is the position, in
 * descending-score order with np.argsort(...)[::-1]'s tie order, of the first entry whose id equals
 * the positive's.  out6 (device) = means over the lines of NDCG@5, NDCG@10, HR@1, HR@5, HR@10, MRR;
 * ranks (optional, device int32 [n_lines]) receives the 0-based ranks.  scratch: 6 * n_lines floats. */
int score_ranking_quality(const float* pred, const int32_t* ids, int64_t n_lines, int32_t per_line,
                          float* out6, int32_t* ranks, float* scratch, int64_t scratch_floats, void* stream);

/* sklearn.metrics.roc_auc_score / log_loss of an evaluation pass (train_score.py:159-160) on the device:
 * pred float32 [n] in (0,1), label int32 [n] in {0,1}.  AUC is the Mann-Whitney statistic with average
 * ranks for tied scores (what the trapezoidal ROC area equals); log-loss clips to [eps, 1-eps] with
 * eps = 2^-52 and accumulates in double.  out2 (device doubles) = {auc, logloss}; auc is NaN when only
 * one class is present.  scratch: score_auc_scratch_bytes(n). */
int score_auc_logloss(const float* pred, const int32_t* label, int64_t n, double* out2, void* scratch,
                      int64_t scratch_bytes, void* stream);
int64_t score_auc_scratch_bytes(int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_HIP_H */
