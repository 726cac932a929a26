// Whole-path orchestration: parameter/workspace layout and the forward / backward
// launch sequences of SCORE and its ablations (score.py:188-369) and of the slice baselines RRN and GCMC
// (slice_model.py:155-203) and of the point baselines GRU4Rec, Caser, SVD++, DELF, DEEMS and SASRec (point_model.py:123-469) on
// one stream.  Host code only; every kernel lives in embed/gemm/gru/gru_stack/head/gcmc/caser/delf/deems/svdpp/sasrec/rank.hip.
#include <string.h>
#include <stdlib.h>
#include <stdio.h>
#include <math.h>
#include <mutex>
#include <new>
#include "common.h"
#include "kernels.h"
#include "persample.h"

namespace {

const int FC1 = 200, FC2 = 80, AT1 = 80, AT2 = 40;
const int CASER_L = SCORE_CASER_L, CASER_HPAD = SCORE_CASER_HPAD;       // kernels.h
const int MAX_ENTRIES = 48;       // dense variables of a model type at most (DEEMS: 46)

// What decides a pass's launch sequence.  FAM_SLICE: SCORE, RIA, RCA, SCORE_USER, SCORE_ITEM and RRN, which differ by attn, coattn
// and Is[] only; every other model type is a family of its own
enum Family { FAM_SLICE, FAM_GCMC, FAM_G4R, FAM_CASER, FAM_DELF, FAM_DEEMS, FAM_SVDPP, FAM_SASREC };

struct Dims {
  int64_t N;
  int D, H, T, K, Fu, Fi, mt;
  int Du, Di, I, Dq, NI, Dk, Dhead, nstate;
  int Is[2];       // GRU input width per side (user, item): I, except RRN / GCMC (their 1-hop sums only)
  bool coattn, attn;
  // the family and what follows from it (set in make_dims only).
  // FAM_G4R: "side" 0 is layer 1 (input: the gathered user_seq rows, Di wide), "side" 1 layer 2 (input: layer 1's outputs, H wide)
  // FAM_CASER: no recurrence at all (H = 0 here, whatever the config says); C = Di columns of xside[0] are its X
  // FAM_DELF: no recurrence and no bn1 / fc head (H = 0 here); X of side 0 = Di columns of xside[0], of side 1 = Du columns of xside[1]
  // FAM_DEEMS: side 0 = gru1 over the user_seq rows (Di columns of xside[0], lengths score_batch_t.length), side 1 = gru2 over the
  //   item_seq rows (Du columns of xside[1], lengths length2); two fc heads of its own on the column ranges [h_u | target_user]
  //   and [h_i | target_item] of ONE head_inp row; DELF's 22 variables laid out and regularised, never read by a launch
  // FAM_SVDPP: no recurrence, no head (H = 0 here); X = Di columns of xside[0]; Fu + Fi scalar variables (svdpp.hip)
  // FAM_SASREC: no recurrence, no bn1 (H = 0 here); X = Di columns of xside[0]; a head of its own applied to 2 T - 2 rows per sample,
  //   in workspace regions of its own (sasrec.hip); Dhead = Di + Du holds the target rows only
  Family family;
  int n_gru;             // recurrences with variables, workspace and launches: 2, or 0 (Caser, DELF, SVD++, SASRec)
  bool fc_head;          // bn1 and fc1-3 behind head_inp (not GCMC, DELF, SVD++; DEEMS has two heads of its own, deems_tower; SASRec: prediction_layer, no bn1)
  bool sums_1hop;        // the gather leaves plain 1-hop sums: no co-attention, no attention, Is[] = {Di, Du} (RRN and every later type)
  bool reads_targets;    // the model reads the target rows (not GCMC: their gradient is zero)
  int Ic;          // row capacity of a side's block of the concatenated [Wx_gates | Wx_cand] copy: I (GRU4Rec: max(I, H))
  int off_u, off_i, off_ti, off_tu;  // columns of head_inp
};

int make_dims(const score_config_t* c, Dims* d) {
  if (!c) return SCORE_E_BADARG;
  d->N = c->feature_size; d->D = c->eb_dim; d->H = c->hidden_size; d->T = c->max_time_len;
  d->K = c->obj_per_time_slice; d->Fu = c->user_fnum; d->Fi = c->item_fnum; d->mt = c->model_type;
  if (d->N <= 0 || d->D <= 0 || (d->D & 3) || d->D > 256 || d->H <= 0 || d->T <= 0 || d->K <= 0 || d->K > 32 ||
      d->Fu <= 0 || d->Fi <= 0 || d->mt < 0 || d->mt > SCORE_MODEL_SASREC)
    return SCORE_E_SHAPE;
  d->Du = d->Fu * d->D; d->Di = d->Fi * d->D; d->I = d->Di + d->Du; d->Dq = d->Du + d->Di;
  const bool gcmc = d->mt == SCORE_MODEL_GCMC, g4r = d->mt == SCORE_MODEL_GRU4REC, caser = d->mt == SCORE_MODEL_CASER,
             delf = d->mt == SCORE_MODEL_DELF, deems = d->mt == SCORE_MODEL_DEEMS, svdpp = d->mt == SCORE_MODEL_SVDPP,
             sasrec = d->mt == SCORE_MODEL_SASREC;
  d->family = gcmc ? FAM_GCMC : g4r ? FAM_G4R : caser ? FAM_CASER : delf ? FAM_DELF : deems ? FAM_DEEMS : svdpp ? FAM_SVDPP :
              sasrec ? FAM_SASREC : FAM_SLICE;
  d->n_gru = (caser || delf || svdpp || sasrec) ? 0 : 2;
  d->fc_head = !gcmc && !delf && !deems && !svdpp && !sasrec;
  d->reads_targets = !gcmc;
  if ((g4r || caser || delf || deems || svdpp || sasrec) && d->K != 1) return SCORE_E_SHAPE;      // (user_seq rides as a [B, T, 1, Fi] set)
  if (sasrec) {
    // (max_time_len >= 3: the negative rows t = 2 .. T - 1; Fi * D <= 128 and a sample's buffers inside one workgroup's LDS)
    if (!score_sasrec_fits(d->T, d->Di)) return SCORE_E_SHAPE;
    d->H = 0;                                                 // hidden_size: accepted and ignored, as for Caser and DELF
  }
  if (svdpp) {
    if (d->D > SCORE_SVDPP_DMAX || d->Fu + d->Fi > MAX_ENTRIES) return SCORE_E_SHAPE;      // (the widths svdpp.hip covers; a variable per field)
    d->H = 0;                                                 // hidden_size: accepted and ignored, as for Caser and DELF
  }
  if (deems && (d->H & 3)) return SCORE_E_SHAPE;                // (the towers' column ranges of head_inp start at 16-byte groups)
  if (delf) {
    if (d->Di > SCORE_DELF_CMAX || d->Du > SCORE_DELF_CMAX) return SCORE_E_SHAPE;      // (the widths delf.hip covers)
    d->H = 0;                                                 // hidden_size: accepted and ignored, as for Caser
  }
  if (caser) {
    if (d->T < CASER_L) return SCORE_E_SHAPE;                 // (conv2d's VALID window, point_model.py:147: TF refuses the graph)
    d->H = 0;                                                 // hidden_size: accepted and ignored -- no GRU variable, workspace or launch
  }
  // (GCMC starts from RRN's two 1-hop sums, slice_model.py:184-187; GRU4Rec's user_seq rows are RRN's "sum" over a one-element set)
  d->sums_1hop = d->mt == SCORE_MODEL_RRN || d->family != FAM_SLICE;
  d->coattn = d->mt != SCORE_MODEL_RCA && !d->sums_1hop;
  d->attn = d->mt != SCORE_MODEL_RIA && !d->sums_1hop;
  d->NI = (d->mt == SCORE_MODEL_RCA || d->mt == SCORE_MODEL_RIA || d->sums_1hop) ? 0 : 4 * d->K;
  // RRN (slice_model.py:159-160): user side = sum_k user_1hop (item features), item side = sum_k item_1hop
  d->Is[0] = d->sums_1hop ? d->Di : d->I;
  d->Is[1] = g4r ? d->H : d->sums_1hop ? d->Du : d->I;
  d->Ic = g4r && d->H > d->I ? d->H : d->I;
  if (gcmc && d->H > 256) return SCORE_E_SHAPE;            // (its head kernels, gcmc.hip)
  d->Dk = d->attn ? 2 * d->H + d->NI : 0;
  d->nstate = d->n_gru == 0 ? 0 : (d->mt == SCORE_MODEL_SCORE_USER || d->mt == SCORE_MODEL_SCORE_ITEM || g4r) ? 1 : 2;
  d->Dhead = d->nstate * d->H + d->Di + d->Du;
  d->off_u = d->mt == SCORE_MODEL_SCORE_ITEM ? -1 : 0;       // (GRU4Rec: layer 2's final state sits where SCORE_USER's state does)
  d->off_i = d->mt == SCORE_MODEL_SCORE_USER ? -1 : (d->mt == SCORE_MODEL_SCORE_ITEM ? 0 : d->H);
  d->off_ti = d->nstate * d->H;       // [..., target_item, target_user]  (score.py:217)
  if (caser) {
    // [h, 0, 0, 0 | v2 (Di) | target_item | target_user]: TF's 1 + 2 Di + Du columns with h padded to four floats, so that the
    // target kernels' 16-byte accesses at off_ti / off_tu and the head kernels' vector path (Dhead % 4 == 0) hold
    d->Dhead = CASER_HPAD + 2 * d->Di + d->Du;
    d->off_u = d->off_i = -1;
    d->off_ti = CASER_HPAD + d->Di;
  }
  d->off_tu = d->off_ti + d->Di;
  if (deems) {
    // [h_u | target_user | h_i | target_item]: each tower's input is a column range (deems_tower)
    d->off_u = 0; d->off_tu = d->H; d->off_i = d->H + d->Du; d->off_ti = 2 * d->H + d->Du;
  }
  return 0;
}

// the GRUs' input rows of side sd and their stride: the [B*T, I] gather output, or GCMC's Z = relu(relu(S Wa) Wc) [B*T, Dx]
// (GRU4Rec's layer 2 reads layer 1's outputs [B*T, H])
static inline int x_ld(const Dims& d, int sd) {
  return d.family == FAM_GCMC ? d.Is[sd] : (d.family == FAM_G4R && sd == 1) ? d.H : d.I;
}

// time slices actually computed for a batch (score_batch_t.active_slices): every [B*T, .] activation of the
// pass is laid out [B * TA, .]; the workspace regions keep their full-T sizes and offsets
// (Caser reads no length, SASRec attends over all T positions: all of them, whatever the batch says)
static inline int active_T(const Dims& d, const score_batch_t* bt) {
  const int a = (d.family == FAM_CASER || d.family == FAM_SASREC) ? 0 : bt->active_slices;
  return (a > 0 && a < d.T) ? a : d.T;
}

// ---------------------------------------------------------------- dense parameter layout
struct PEntry { const char* name; int rows, cols, reg, init; };

struct Params {  // float offsets into the flat buffer
  int64_t ca_w[2], ca_b[2];
  int64_t gk[2], gb[2], ck[2], cb[2];  // gates/candidate kernel/bias per GRU (0 user side, 1 item side)
  int64_t at_w[4], at_b[4];
  int64_t bn_g, bn_b, fc_w[3], fc_b[3];
  int64_t gm_a[2], gm_c[2], gm_4, gm_5;  // GCMC: per side dense (Wa) and dense_2 / dense_3 (Wc); the head's dense_4, dense_5
  int64_t cs_wh, cs_bh, cs_wv, cs_bv, cs_wd, cs_bd;  // Caser: conv2d (horizontal), conv2d_1 (vertical), dense (the scalar one)
  int64_t dl_w[11], dl_b[11];           // DELF: dense .. dense_10, kernels and biases (DEEMS: the same variables, dormant)
  int64_t sv_w;                         // SVD++: user_feat_w_0's 4-float cell; user_feat_w_i at + 4 i, item_feat_w_j at + 4 (Fu + j)
  int64_t sa_beta, sa_gamma, sa_w[3], sa_b[3];      // SASRec: ln/Variable, ln/Variable_1, multihead_attention/dense .. dense_2 (Q, K, V);
                                        // prediction_layer/fc1 .. fc3 are fc_w / fc_b
  int64_t bn_g2, bn_b2, fc_w2[3], fc_b2[3];     // DEEMS: the item tower (batch_normalization_1, dense_14 .. dense_16); the user tower
                                        // (batch_normalization, dense_11 .. dense_13) is bn_g / bn_b / fc_w / fc_b
  int64_t n_floats, n_reg;
};

int build_layout_raw(const Dims& d, score_param_entry_t* out, int max_entries, Params* P) {
  // TF creation order (score.py:188-224): co_attention denses, GRU cells, attention denses, bn1, fc1-3
  char names[MAX_ENTRIES][64];
  int rows[MAX_ENTRIES], cols[MAX_ENTRIES], reg[MAX_ENTRIES], init[MAX_ENTRIES];
  int n = 0, nd = 0;
  memset(P, 0, sizeof(*P));      // (a variable the model type does not have: offset 0, never read)
  const bool gcmc = d.family == FAM_GCMC, caser = d.family == FAM_CASER, deems = d.family == FAM_DEEMS;
  const bool delf = d.family == FAM_DELF || deems;      // (DEEMS.__init__ runs DELF's first: its variables exist, point_model.py:283)
  auto add = [&](const char* nm, int r, int c, int rg, int in) {
    snprintf(names[n], 64, "%s", nm);
    rows[n] = r; cols[n] = c; reg[n] = rg; init[n] = in; ++n;
  };
  auto dense = [&](int i, int o) {
    char b[64];
    if (nd == 0) snprintf(b, 64, "dense"); else snprintf(b, 64, "dense_%d", nd);
    ++nd;
    char k[64], bb[64];
    snprintf(k, 64, "%s/kernel", b); snprintf(bb, 64, "%s/bias", b);
    add(k, i, o, 1, 2); add(bb, o, 0, 0, 0);
  };
  if (d.coattn) { dense(3 * d.Di, 1); dense(3 * d.Du, 1); }
  // GCMC (slice_model.py:182-201): dense .. dense_3 (per-side relu denses, no bias), gru1 / gru2, dense_4 / dense_5 (the head)
  const int Dx[2] = {d.Di, d.Du};
  if (gcmc) {
    add("dense/kernel", Dx[0], Dx[0], 1, 2); add("dense_1/kernel", Dx[1], Dx[1], 1, 2);
    add("dense_2/kernel", Dx[0], Dx[0], 1, 2); add("dense_3/kernel", Dx[1], Dx[1], 1, 2);
  }
  const char* sides[2] = {"gru_user_side", "gru_item_side"};
  if (gcmc || d.family == FAM_G4R || deems) { sides[0] = "gru1"; sides[1] = "gru2"; }     // (GRU4Rec, point_model.py:129-132: the two stacked layers; DEEMS :287-290)
  // Caser (point_model.py:147-157): conv2d [50, C, 1, 1], conv2d_1 [T, 1, 1, 1] (init 3: glorot with TF's convolution fans,
  // fan_in = fan_out = rows * cols), dense [1, 1]
  if (caser) {
    add("conv2d/kernel", CASER_L, d.Di, 1, 3); add("conv2d/bias", 1, 0, 0, 0);
    add("conv2d_1/kernel", d.T, 1, 1, 3); add("conv2d_1/bias", 1, 0, 0, 0);
    dense(1, 1);
  }
  // SVD++ (point_model.py:171-187): one scalar per feature field, shape [], truncated normal (init 4), all regularised -- each
  // in a 4-float cell of the regularised region (the 16-byte alignment below), consecutive: the pad floats stay zero
  if (d.family == FAM_SVDPP) {
    char b[64];
    for (int i = 0; i < d.Fu; ++i) { snprintf(b, 64, "user_feat_w_%d", i); add(b, 1, 0, 1, 4); }
    for (int j = 0; j < d.Fi; ++j) { snprintf(b, 64, "item_feat_w_%d", j); add(b, 1, 0, 1, 4); }
  }
  // SASRec (point_model.py:441-469, 362-439, 353-360): the layer norm's beta and gamma -- plain tf.Variable's whose names hold
  // neither "bias" nor "emb": BOTH regularised --, the three projections, the shared head without a batch norm
  if (d.family == FAM_SASREC) {
    add("ln/Variable", d.Di, 0, 1, 0); add("ln/Variable_1", d.Di, 0, 1, 1);
    const char* pr[3] = {"multihead_attention/dense", "multihead_attention/dense_1", "multihead_attention/dense_2"};
    for (int k = 0; k < 3; ++k) {
      char b[64];
      snprintf(b, 64, "%s/kernel", pr[k]); add(b, d.Di, d.Di, 1, 2);
      snprintf(b, 64, "%s/bias", pr[k]); add(b, d.Di, 0, 0, 0);
    }
    const int Dh = 2 * d.Di + d.Du;
    add("prediction_layer/fc1/kernel", Dh, FC1, 1, 2); add("prediction_layer/fc1/bias", FC1, 0, 0, 0);
    add("prediction_layer/fc2/kernel", FC1, FC2, 1, 2); add("prediction_layer/fc2/bias", FC2, 0, 0, 0);
    add("prediction_layer/fc3/kernel", FC2, 1, 1, 2); add("prediction_layer/fc3/bias", 1, 0, 0, 0);
  }
  // DELF (point_model.py:216-232, 235-249): the two attention denses, four fusion MLPs (10, 4), the output unit
  if (delf) {
    dense(d.Di, d.Di); dense(d.Du, d.Du);
    const int in[4] = {d.Du + d.Di, d.Di + d.Du, 2 * d.Du, 2 * d.Di};      // [tu|ti], [ru|ri], [tu|ri], [ti|ru]
    for (int k = 0; k < 4; ++k) { dense(in[k], 10); dense(10, 4); }
    dense(4, 1);
  }
  for (int s = 0; s < d.n_gru; ++s) {
    char b[64];
    snprintf(b, 64, "%s/gru_cell/gates/kernel", sides[s]); add(b, d.Is[s] + d.H, 2 * d.H, 1, 2);
    snprintf(b, 64, "%s/gru_cell/gates/bias", sides[s]); add(b, 2 * d.H, 0, 0, 1);
    snprintf(b, 64, "%s/gru_cell/candidate/kernel", sides[s]); add(b, d.Is[s] + d.H, d.H, 1, 2);
    snprintf(b, 64, "%s/gru_cell/candidate/bias", sides[s]); add(b, d.H, 0, 0, 0);
  }
  if (d.attn) { dense(d.Dq, d.Dk); dense(4 * d.Dk, AT1); dense(AT1, AT2); dense(AT2, 1); }
  if (gcmc) { add("dense_4/kernel", d.H, d.H, 1, 2); add("dense_5/kernel", d.H, d.H, 1, 2); }
  if (d.fc_head) {
    add("bn1/gamma", d.Dhead, 0, 1, 1);
    add("bn1/beta", d.Dhead, 0, 1, 0);
    add("fc1/kernel", d.Dhead, FC1, 1, 2); add("fc1/bias", FC1, 0, 0, 0);
    add("fc2/kernel", FC1, FC2, 1, 2); add("fc2/bias", FC2, 0, 0, 0);
    add("fc3/kernel", FC2, 1, 1, 2); add("fc3/bias", 1, 0, 0, 0);
  }
  // DEEMS (point_model.py:295-296, 302-311): build_fc_net twice without names -- batch_normalization, dense_11 .. dense_13 on
  // [h_u | target_user], batch_normalization_1, dense_14 .. dense_16 on [h_i | target_item]
  if (deems) {
    const int Dt[2] = {d.H + d.Du, d.H + d.Di};
    for (int k = 0; k < 2; ++k) {
      add(k ? "batch_normalization_1/gamma" : "batch_normalization/gamma", Dt[k], 0, 1, 1);
      add(k ? "batch_normalization_1/beta" : "batch_normalization/beta", Dt[k], 0, 1, 0);
      dense(Dt[k], FC1); dense(FC1, FC2); dense(FC2, 1);
    }
  }
  // offsets: regularised tensors first, then the rest; every tensor 16-B aligned.  The
  // regularised region is padded with zeros that stay zero (zero grad, zero l2 term).
  int64_t off[MAX_ENTRIES];
  int64_t cur = 0;
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = 0; i < n; ++i) {
      if ((reg[i] != 0) != (pass == 0)) continue;
      off[i] = cur;
      int64_t sz = (int64_t)rows[i] * (cols[i] ? cols[i] : 1);
      cur = align_up64(cur + sz, 4);
    }
    if (pass == 0) P->n_reg = cur;
  }
  P->n_floats = cur;
  if (out) {
    if (n > max_entries) return SCORE_E_BADARG;
    for (int i = 0; i < n; ++i) {
      memset(&out[i], 0, sizeof(out[i]));
      snprintf(out[i].name, 64, "%s", names[i]);
      out[i].offset = off[i]; out[i].rows = rows[i]; out[i].cols = cols[i];
      out[i].regularised = reg[i]; out[i].init = init[i];
    }
  }
  int i = 0;      // (in creation order, as above)
  if (d.coattn) { for (int c = 0; c < 2; ++c) { P->ca_w[c] = off[i++]; P->ca_b[c] = off[i++]; } }
  if (gcmc) { P->gm_a[0] = off[i++]; P->gm_a[1] = off[i++]; P->gm_c[0] = off[i++]; P->gm_c[1] = off[i++]; }
  if (caser) { P->cs_wh = off[i++]; P->cs_bh = off[i++]; P->cs_wv = off[i++]; P->cs_bv = off[i++]; P->cs_wd = off[i++]; P->cs_bd = off[i++]; }
  if (d.family == FAM_SVDPP) { P->sv_w = off[i]; i += d.Fu + d.Fi; }
  if (d.family == FAM_SASREC) {
    P->sa_beta = off[i++]; P->sa_gamma = off[i++];
    for (int k = 0; k < 3; ++k) { P->sa_w[k] = off[i++]; P->sa_b[k] = off[i++]; }
    for (int f = 0; f < 3; ++f) { P->fc_w[f] = off[i++]; P->fc_b[f] = off[i++]; }
  }
  if (delf) { for (int k = 0; k < 11; ++k) { P->dl_w[k] = off[i++]; P->dl_b[k] = off[i++]; } }
  for (int s = 0; s < d.n_gru; ++s) { P->gk[s] = off[i++]; P->gb[s] = off[i++]; P->ck[s] = off[i++]; P->cb[s] = off[i++]; }
  if (d.attn) { for (int a = 0; a < 4; ++a) { P->at_w[a] = off[i++]; P->at_b[a] = off[i++]; } }
  if (gcmc) { P->gm_4 = off[i++]; P->gm_5 = off[i++]; }
  if (d.fc_head) {
    P->bn_g = off[i++]; P->bn_b = off[i++];
    for (int f = 0; f < 3; ++f) { P->fc_w[f] = off[i++]; P->fc_b[f] = off[i++]; }
  }
  if (deems) {
    P->bn_g = off[i++]; P->bn_b = off[i++];
    for (int f = 0; f < 3; ++f) { P->fc_w[f] = off[i++]; P->fc_b[f] = off[i++]; }
    P->bn_g2 = off[i++]; P->bn_b2 = off[i++];
    for (int f = 0; f < 3; ++f) { P->fc_w2[f] = off[i++]; P->fc_b2[f] = off[i++]; }
  }
  return n;
}

// Every entry point derives the parameter and workspace layouts from the config: a few dozen snprintf's and a page of
// arithmetic per call, six times per training step -- ~30 us of a host-bound 200-us step at the reference's own shapes.  The last
// result per thread is kept (a step alternates between one config and one batch size).
struct LayoutKey { int64_t N; int D, H, T, K, Fu, Fi, mt, B; };
static inline LayoutKey layout_key(const Dims& d, int B) {
  LayoutKey k;
  memset(&k, 0, sizeof(k));            // (padding bytes too: the keys are compared with memcmp)
  k.N = d.N; k.D = d.D; k.H = d.H; k.T = d.T; k.K = d.K; k.Fu = d.Fu; k.Fi = d.Fi; k.mt = d.mt; k.B = B;
  return k;
}
static inline bool same_key(const LayoutKey& a, const LayoutKey& b) { return memcmp(&a, &b, sizeof(a)) == 0; }
int build_layout(const Dims& d, score_param_entry_t* out, int max_entries, Params* P) {
  struct Memo { bool ok; LayoutKey k; Params P; int n; score_param_entry_t ent[MAX_ENTRIES]; };
  static thread_local Memo memo = {};
  LayoutKey k = layout_key(d, 0);
  if (!memo.ok || !same_key(memo.k, k)) {
    memset(&memo.k, 0, sizeof(memo.k));
    memo.n = build_layout_raw(d, memo.ent, MAX_ENTRIES, &memo.P);
    memo.k = k; memo.ok = memo.n >= 0;
    if (memo.n < 0) return memo.n;
  }
  *P = memo.P;
  if (out) {
    if (memo.n > max_entries) return SCORE_E_BADARG;
    memcpy(out, memo.ent, sizeof(score_param_entry_t) * memo.n);
  }
  return memo.n;
}

// ---------------------------------------------------------------- workspace layout (float offsets)
struct WS {
  int64_t xside[2], info, rsave[2], query, head_inp, att_score, logit, y_pred, loss;
  int64_t gru_out[2], gru_final[2], xproj[2], gates[2];
  int64_t q, ainp, a1, a2, bn, f1, f2, lossb, dlogit, part;
  int64_t weff, wq, qz, adzsum, dweff, dwq, dqd;   // folded first attention layer (head.hip)
  int64_t dwslab, dwslab_floats, dgstage, scratch2, gru_tmp, gru_tmp_floats;          // deferred weight-gradient products (gemm.hip), bn1 dgamma staging
  // backward
  int64_t dz2, dz1, dbn, dhead, ds, da2, da1, dainp, dgru[2], dinfo, dq, dquery, dfinal[2];
  int64_t dxproj[2], rh[2], hprev[2], dxside[2], dzsum[2], S, scratch;
  int64_t pcoef[2], dzcoef[2], dtgt, keys_in, keys_out, vals_in, vals_out, sort_temp, partials;
  int64_t n_occ, sort_temp_bytes, partial_floats;
  int64_t uid, unique_rows, meta, remap[6];
  int64_t ca_slab, ca_slab_floats, cs_part, cs_part_floats, wxcat;
  int64_t pimg_x[2], pimg_d[2];      // weight fragment images of the panel GEMMs (gemm_panel.hip): projection, input gradient
  int64_t psimg;                     // weight images of the per-sample whole-model kernels (persample.h)
  // GCMC only (-1 otherwise): per side A = relu(S Wa), Z = relu(A Wc) and the gradients at their pre-activations, [B*T, Dx];
  // the head's p = h_i W4 | n = h_i W5 [2][B, H], g = dL/da [B], and gpos = g h_u | gneg = -g h_u [2][B, H]
  int64_t gcmc_a[2], gcmc_z[2], gcmc_dz[2], gcmc_da[2], gcmc_pn, gcmc_g, gcmc_gu;
  // Caser only (-1 otherwise): the window sums [B, T - 49], the first position of their maximum [B] (int32), v before the scalar
  // dense [B, C]
  int64_t caser_hwin, caser_arg, caser_v;
  // DELF only (-1 otherwise), per side: tanh keys [B*T, C], attention weights [B, T], attention outputs [B, C], the gradient at
  // the scores [B, T] and at the keys' pre-activations [B*T, C]; the fusion layers' activations and their gradients [B, 64]
  int64_t delf_key[2], delf_att[2], delf_rep[2], delf_ds[2], delf_dpre[2], delf_act, delf_dact;
  // DEEMS only (-1 otherwise): the item tower's f1 / f2 / dz1 / dz2 (the user tower's are the head's own regions; bn, dbn, dhead and
  // dgstage hold both towers' column ranges), and per tower [2][B] the logits, y_u | y_i, dL/d logit
  int64_t deems_f1, deems_f2, deems_dz1, deems_dz2, deems_logit, deems_y, deems_dlogit;
  // SVD++ only (-1 otherwise): what the forward kernel saves [B, 4 D + 4] (kernels.h: SvdppArgs.act) and the per-sample partials of
  // the weight gradients [B, Fu + Fi]
  int64_t svdpp_act, svdpp_dw;
  // SASRec only (-1 otherwise; kernels.h: SasrecArgs).  Per (b, t) row: N, Qin, Q, K, V, Y and dQ, dK, dV [B*T, C], 1 / sqrt(var +
  // eps) and the key mask [B*T]; per sample the softmax and the final attention weights [B, 2, T, T], final [B, C] and the
  // gamma / beta partials [B, C]; the head: its input rows and their gradient [B (T-1) + B, 2 C + Cu], z1 / dz1 [.., 200], and over
  // the R = B (T-1) + B (T-2) + B rows of the three applications f1 / dz1e [R, 200], z2 / f2 / dz2 [R, 80], logit / dlogit [R]
  int64_t sas_nrm, sas_qin, sas_q, sas_k, sas_v, sas_y, sas_dq, sas_dk, sas_dv, sas_rstd, sas_km, sas_p, sas_att, sas_fin,
      sas_dgamma, sas_dbeta, sas_hin, sas_dhin, sas_z1, sas_dz1, sas_f1, sas_dz1e, sas_z2, sas_f2, sas_dz2, sas_logit, sas_dlogit;
  int64_t scratch_floats, total;
};

// the projections' 3H output columns as one panel (3H <= 512) or as two column halves, each a panel group of its own
// (H = 256: 768 columns; A is then read twice); 0: no panel form
static int panel_x_splits(int H) { return 3 * H <= 512 ? 1 : ((3 * H) % 32 == 0 && 3 * H <= 1024 ? 2 : 0); }
// ... and the input gradients' I output columns likewise (cfg-5, Tmall-shaped: 896)
static int panel_d_splits(int I) { return I <= 512 ? 1 : (I % 32 == 0 && I <= 1024 ? 2 : 0); }

// the per-sample whole-model kernels (persample.h: SCORE / SCORE_USER / SCORE_ITEM at H = 32) read their weights as images
static int64_t ps_image_region_floats(const Dims& d) {
  if (d.H != 32 || !d.coattn || !d.attn) return 0;
  PsShape s;
  memset(&s, 0, sizeof(s));
  s.H = d.H; s.I = d.I; s.Dk = d.Dk; s.Dhead = d.Dhead;
  PsImages im;
  ps_plan_images(s, &im);
  return im.total;
}

// distance between the replicas of the folded first attention layer's weight (head.hip)
static inline int64_t weff_copy_stride(const Dims& d) { return align_up64(2 * (int64_t)d.Dk * AT1 + 48, 4); }
// hands out the workspace's regions front to back, each 16-B aligned (an empty one still takes four floats)
struct Taker {
  int64_t cur;
  int64_t operator()(int64_t n) { int64_t o = cur; cur = align_up64(cur + (n > 0 ? n : 4), 4); return o; }
};
// the regions only one family has: at the end, so that the other model types' layouts stay what they were
void ws_family_regions(const Dims& d, int B, Taker& take, WS* w) {
  const int64_t BT = (int64_t)B * d.T;
  if (d.family == FAM_GCMC) {
    const int Dx[2] = {d.Di, d.Du};
    for (int s = 0; s < 2; ++s) {
      w->gcmc_a[s] = take(BT * Dx[s]); w->gcmc_z[s] = take(BT * Dx[s]);
      w->gcmc_dz[s] = take(BT * Dx[s]); w->gcmc_da[s] = take(BT * Dx[s]);
    }
    w->gcmc_pn = take(2 * (int64_t)B * d.H); w->gcmc_g = take(B); w->gcmc_gu = take(2 * (int64_t)B * d.H);
  } else {
    for (int s = 0; s < 2; ++s) w->gcmc_a[s] = w->gcmc_z[s] = w->gcmc_dz[s] = w->gcmc_da[s] = -1;
    w->gcmc_pn = w->gcmc_g = w->gcmc_gu = -1;
  }
  if (d.family == FAM_CASER) {
    w->caser_hwin = take((int64_t)B * (d.T - CASER_L + 1)); w->caser_arg = take(B); w->caser_v = take((int64_t)B * d.Di);
  } else {
    w->caser_hwin = w->caser_arg = w->caser_v = -1;
  }
  if (d.family == FAM_DELF) {
    const int Cx[2] = {d.Di, d.Du};
    for (int s = 0; s < 2; ++s) {
      w->delf_key[s] = take(BT * Cx[s]); w->delf_att[s] = take(BT); w->delf_rep[s] = take((int64_t)B * Cx[s]);
      w->delf_ds[s] = take(BT); w->delf_dpre[s] = take(BT * Cx[s]);
    }
    w->delf_act = take((int64_t)B * SCORE_DELF_ACT); w->delf_dact = take((int64_t)B * SCORE_DELF_ACT);
  } else {
    for (int s = 0; s < 2; ++s) w->delf_key[s] = w->delf_att[s] = w->delf_rep[s] = w->delf_ds[s] = w->delf_dpre[s] = -1;
    w->delf_act = w->delf_dact = -1;
  }
  if (d.family == FAM_DEEMS) {
    w->deems_f1 = take((int64_t)B * FC1); w->deems_f2 = take((int64_t)B * FC2);
    w->deems_dz1 = take((int64_t)B * FC1); w->deems_dz2 = take((int64_t)B * FC2);
    w->deems_logit = take(2 * (int64_t)B); w->deems_y = take(2 * (int64_t)B); w->deems_dlogit = take(2 * (int64_t)B);
  } else {
    w->deems_f1 = w->deems_f2 = w->deems_dz1 = w->deems_dz2 = w->deems_logit = w->deems_y = w->deems_dlogit = -1;
  }
  if (d.family == FAM_SVDPP) {
    w->svdpp_act = take((int64_t)B * score_svdpp_act_floats(d.D)); w->svdpp_dw = take((int64_t)B * (d.Fu + d.Fi));
  } else {
    w->svdpp_act = w->svdpp_dw = -1;
  }
  if (d.family == FAM_SASREC) {
    const int64_t C = d.Di, rows1 = BT, R = BT + (int64_t)B * (d.T - 2), TT2 = 2 * (int64_t)B * d.T * d.T;      // (rows1 = B (T-1) + B)
    w->sas_nrm = take(BT * C); w->sas_qin = take(BT * C); w->sas_q = take(BT * C); w->sas_k = take(BT * C); w->sas_v = take(BT * C);
    w->sas_y = take(BT * C); w->sas_dq = take(BT * C); w->sas_dk = take(BT * C); w->sas_dv = take(BT * C);
    w->sas_rstd = take(BT); w->sas_km = take(BT); w->sas_p = take(TT2); w->sas_att = take(TT2);
    w->sas_fin = take((int64_t)B * C); w->sas_dgamma = take((int64_t)B * C); w->sas_dbeta = take((int64_t)B * C);
    w->sas_hin = take(rows1 * (2 * C + d.Du)); w->sas_dhin = take(rows1 * (2 * C + d.Du));
    w->sas_z1 = take(rows1 * FC1); w->sas_dz1 = take(rows1 * FC1); w->sas_f1 = take(R * FC1); w->sas_dz1e = take(R * FC1);
    w->sas_z2 = take(R * FC2); w->sas_f2 = take(R * FC2); w->sas_dz2 = take(R * FC2); w->sas_logit = take(R); w->sas_dlogit = take(R);
  } else {
    w->sas_nrm = w->sas_qin = w->sas_q = w->sas_k = w->sas_v = w->sas_y = w->sas_dq = w->sas_dk = w->sas_dv = w->sas_rstd = w->sas_km =
        w->sas_p = w->sas_att = w->sas_fin = w->sas_dgamma = w->sas_dbeta = w->sas_hin = w->sas_dhin = w->sas_z1 = w->sas_dz1 = w->sas_f1 =
            w->sas_dz1e = w->sas_z2 = w->sas_f2 = w->sas_dz2 = w->sas_logit = w->sas_dlogit = -1;
  }
}

void build_ws_raw(const Dims& d, int B, WS* w) {
  Taker take = {0};
  const int64_t BT = (int64_t)B * d.T;
  for (int s = 0; s < 2; ++s) w->xside[s] = take(BT * d.I);
  w->info = take(BT * 4 * d.K);
  for (int c = 0; c < 2; ++c) w->rsave[c] = take(BT * d.K);
  w->query = take((int64_t)B * d.Dq);
  w->head_inp = take((int64_t)B * d.Dhead);
  w->att_score = take(BT);
  w->logit = take(B); w->y_pred = take(B); w->loss = take(4);
  for (int s = 0; s < 2; ++s) w->gru_out[s] = take(BT * d.H);
  for (int s = 0; s < 2; ++s) w->gru_final[s] = take((int64_t)B * d.H);
  for (int s = 0; s < 2; ++s) w->xproj[s] = take(BT * 3 * d.H);
  for (int s = 0; s < 2; ++s) w->gates[s] = take(BT * 3 * d.H);
  w->q = take((int64_t)B * d.Dk);
  w->ainp = take(BT * 2 * d.Dk);
  w->weff = take(SCORE_WEFF_COPIES * weff_copy_stride(d)); w->wq = take((int64_t)d.Dk * AT1); w->qz = take((int64_t)B * AT1);
  w->a1 = take(BT * AT1); w->a2 = take(BT * AT2);
  w->bn = take((int64_t)B * d.Dhead);
  w->f1 = take((int64_t)B * FC1); w->f2 = take((int64_t)B * FC2);
  w->lossb = take(B); w->dlogit = take(B); w->part = take(256 + 4);      // (+ one word: the per-sample forward kernel's count of finished workgroups)
  w->dz2 = take((int64_t)B * FC2); w->dz1 = take((int64_t)B * FC1);
  w->dbn = take((int64_t)B * d.Dhead); w->dhead = take((int64_t)B * d.Dhead);
  w->ds = take(BT); w->da2 = take(BT * AT2); w->da1 = take(BT * AT1);
  w->dainp = take(BT * 2 * d.Dk);
  w->adzsum = take((int64_t)B * AT1); w->dweff = take(2 * (int64_t)d.Dk * AT1); w->dwq = take((int64_t)d.Dk * AT1);
  w->dqd = take((int64_t)B * d.Dk);
  for (int s = 0; s < 2; ++s) w->dgru[s] = take(BT * d.H);
  w->dinfo = take(BT * 4 * d.K);
  w->dq = take((int64_t)B * d.Dk); w->dquery = take((int64_t)B * d.Dq);
  for (int s = 0; s < 2; ++s) w->dfinal[s] = take((int64_t)B * d.H);
  for (int s = 0; s < 2; ++s) {
    w->dxproj[s] = take(BT * 3 * d.H);
    w->rh[s] = take(BT * d.H);
    w->hprev[s] = take(BT * d.H + 3 * (int64_t)d.H * d.H);
  }
  for (int s = 0; s < 2; ++s) w->dxside[s] = take(BT * d.I);
  for (int c = 0; c < 2; ++c) w->dzsum[c] = take(BT);
  w->S = take(2 * (int64_t)B);
  w->scratch_floats = 4 << 20;
  w->scratch = take(w->scratch_floats);
  w->ca_slab_floats = 2 * 512 * 2 * (int64_t)(d.Di > d.Du ? d.Di : d.Du);
  w->ca_slab = take(w->ca_slab_floats);
  w->cs_part_floats = 1 << 21;
  w->cs_part = take(w->cs_part_floats);
  w->wxcat = take(2 * (int64_t)(d.Ic + 1) * 3 * d.H);
  for (int sd = 0; sd < 2; ++sd) {
    const int ns = d.n_gru ? panel_x_splits(d.H) : 0;      // (Caser: no recurrence, no projection)
    w->pimg_x[sd] = take(ns ? ns * score_gemm_panel_image_floats(3 * d.H / ns, d.Is[sd]) : 0);
    const int nd = d.n_gru ? panel_d_splits(d.Is[sd]) : 0;
    w->pimg_d[sd] = take(nd ? nd * score_gemm_panel_image_floats(d.Is[sd] / nd, 3 * d.H) : 0);
  }
  w->psimg = take(ps_image_region_floats(d));
  w->dgstage = take((int64_t)B * d.Dhead);
  w->scratch2 = take(w->scratch_floats);           // split-K scratch of the side stream's products
  // scratch of the recurrences without a register-resident kernel: MFMA-fragment weight copies (H = 256) or the
  // step-by-step form's state
  w->gru_tmp_floats = 10 * (int64_t)B * d.H;
  if (w->gru_tmp_floats < 12 * (int64_t)d.H * d.H) w->gru_tmp_floats = 12 * (int64_t)d.H * d.H;
  w->gru_tmp = take(w->gru_tmp_floats);
  {
    // split-K partials of every queued weight-gradient product: ~24 slabs of each dense variable
    Params Pl;
    build_layout(d, nullptr, 0, &Pl);
    w->dwslab_floats = 48 * Pl.n_floats;
    w->dwslab = take(w->dwslab_floats);
  }
  // sorted pull-form scatter (scatter.hip)
  for (int c = 0; c < 2; ++c) { w->pcoef[c] = take(BT * d.K); w->dzcoef[c] = take(BT * d.K); }
  w->dtgt = take((int64_t)B * d.Dq);
  w->n_occ = (int64_t)B * (2 * (int64_t)d.T * d.K * (d.Fu + d.Fi) + d.Fu + d.Fi);
  const int64_t np = w->n_occ + 1;   // + sentinel occurrence of row 0
  w->keys_in = take(np); w->keys_out = take(np);
  w->vals_in = take(np); w->vals_out = take(np);
  w->uid = take(np); w->unique_rows = take(np); w->meta = take(80);
  {
    const int64_t nn[6] = {BT * d.K * d.Fi, BT * d.K * d.Fi, BT * d.K * d.Fu, BT * d.K * d.Fu, (int64_t)B * d.Fu,
                           (int64_t)B * d.Fi};
    for (int g = 0; g < 6; ++g) w->remap[g] = take(nn[g]);
  }
  size_t tb = 0, tb2 = 0;
  score_plan_temp_bytes(np, 32, &tb);
  score_scan_temp_bytes(np, &tb2);
  if (tb2 > tb) tb = tb2;
  if (score_sort_temp_bytes(np) > tb) tb = score_sort_temp_bytes(np);       // (sort.hip's histogram matrix)
  w->sort_temp_bytes = (int64_t)tb;
  w->sort_temp = take((int64_t)(tb + 3) / 4 + 4);
  {
    // fewer active slices shrink the occurrence list, and a shorter list may use a narrower window:
    // below 2^20 occurrences there are never more than 2^15 windows
    int64_t nw = cdiv64(np, score_pull_window(np));
    if (nw < (1 << 15) + 1) nw = (1 << 15) + 1;
    w->partial_floats = 2 * nw * d.D + 8 + 2 * nw;
  }
  w->partials = take(w->partial_floats);
  ws_family_regions(d, B, take, w);
  w->total = take.cur;
}

void build_ws(const Dims& d, int B, WS* w) {
  struct Memo { bool ok; LayoutKey k; WS w; };
  static thread_local Memo memo = {};
  LayoutKey k = layout_key(d, B);
  if (!memo.ok || !same_key(memo.k, k)) {
    memset(&memo.k, 0, sizeof(memo.k));
    build_ws_raw(d, B, &memo.w);
    memo.k = k; memo.ok = true;
  }
  *w = memo.w;
}

// A second stream for work that is independent of the long narrow kernels of the path: the GRU recurrences
// occupy 128 workgroups (16 samples each at B = 1024), half the chip; the attention query branch (forward) and
// the weight gradients already known (backward) run beside them.  The stream and its three events belong to a
// score_context_t (score_context_create / score_context_destroy, include/score_hip.h) that the caller passes in
// score_state_t.context; forked from / joined back into the caller's stream with events.  A caller that passes no
// context shares ONE process-wide default context per device (created on first use, released by
// score_context_destroy(NULL)): the only state the library keeps between calls.
struct SideStream { hipStream_t st; hipEvent_t fork, join, wx; int device; hipStream_t fwd_on; };
#define HIPTRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return (int)e_; } while (0)
// events that order device work only (include/score_hip.h score_event_create)
#define SCORE_DEVICE_EVENT_FLAGS (hipEventDisableTiming | hipEventDisableSystemFence)
extern "C" int score_event_create(void** event) {
  if (!event) return SCORE_E_BADARG;
  hipEvent_t e;
  HIPTRY(hipEventCreateWithFlags(&e, SCORE_DEVICE_EVENT_FLAGS));
  *event = (void*)e;
  return 0;
}
extern "C" int score_event_destroy(void* event) {
  if (!event) return SCORE_E_BADARG;
  HIPTRY(hipEventDestroy((hipEvent_t)event));
  return 0;
}
extern "C" int score_event_record(void* event, void* stream) {
  if (!event) return SCORE_E_BADARG;
  HIPTRY(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
  return 0;
}
extern "C" int score_stream_wait_event(void* stream, void* event) {
  if (!event) return SCORE_E_BADARG;
  HIPTRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0));
  return 0;
}
extern "C" int score_event_query(void* event) {
  if (!event) return SCORE_E_BADARG;
  const hipError_t e = hipEventQuery((hipEvent_t)event);
  return e == hipSuccess ? 0 : e == hipErrorNotReady ? 1 : (int)e;
}
extern "C" int score_event_synchronize(void* event) {
  if (!event) return SCORE_E_BADARG;
  HIPTRY(hipEventSynchronize((hipEvent_t)event));
  return 0;
}
static int side_stream_create(SideStream* sd) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return SCORE_E_BADARG;
  hipStream_t st; hipEvent_t a, b, c;
  hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  if (e != hipSuccess) return (int)e;
  if ((e = hipEventCreateWithFlags(&a, SCORE_DEVICE_EVENT_FLAGS)) != hipSuccess) { hipStreamDestroy(st); return (int)e; }
  if ((e = hipEventCreateWithFlags(&b, SCORE_DEVICE_EVENT_FLAGS)) != hipSuccess) { hipEventDestroy(a); hipStreamDestroy(st); return (int)e; }
  if ((e = hipEventCreateWithFlags(&c, SCORE_DEVICE_EVENT_FLAGS)) != hipSuccess) { hipEventDestroy(a); hipEventDestroy(b); hipStreamDestroy(st); return (int)e; }
  sd->st = st; sd->fork = a; sd->join = b; sd->wx = c; sd->device = dev; sd->fwd_on = nullptr;
  return 0;
}
static void side_stream_release(SideStream* sd) {
  if (!sd->st) return;
  hipStreamSynchronize(sd->st);
  hipEventDestroy(sd->fork); hipEventDestroy(sd->join); hipEventDestroy(sd->wx);
  hipStreamDestroy(sd->st);
  sd->st = nullptr;
}
#define SCORE_MAX_DEVICES 16
static SideStream g_default_ctx[SCORE_MAX_DEVICES];
static std::mutex g_default_mu;
static int side_stream(const score_state_t* st, SideStream** out) {
  if (st && st->context) { *out = reinterpret_cast<SideStream*>(st->context); return 0; }
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= SCORE_MAX_DEVICES) return SCORE_E_BADARG;
  std::lock_guard<std::mutex> lock(g_default_mu);
  SideStream& sd = g_default_ctx[dev];
  if (!sd.st) SCORE_TRY(side_stream_create(&sd));
  *out = &sd;
  return 0;
}
// A/B switches of the launch sequence: score_state_t.debug_flags only (round 4: the environment switches of rounds 1 - 3 --
// SCORE_WGRAD_SIDE / _EARLY, SCORE_PANEL_DX, SCORE_GEMM_TILED, SCORE_GRU_STEPWISE, SCORE_GRU_BIAS_COLSUM, SCORE_HEAD_UNFUSED,
// SCORE_ATTN_*_UNFUSED -- were decided A/Bs or duplicates of a flag bit, and a process-wide switch read once cannot be
// flipped by the test that wants to compare the two paths).  include/score_hip.h describes the bits; flags_of is the one
// place that reads them.
enum {
  DF_GRU_STEPWISE = 1, DF_HEAD_FUSED_ANY_B = 2, DF_GRU_F32_REC = 4, DF_NO_PANEL = 8, DF_PANEL_DX = 16, DF_SORT_LIB = 32,
  DF_HEAD_UNFUSED = 64, DF_ATTN_UNFUSED = 128, DF_SORT_OWN = 256, DF_NO_PS = 512, DF_PS_FWD_ONLY = 1024, DF_PS_BWD_ONLY = 2048,
  DF_ONE_STREAM = 4096, DF_G4R_COMPOSED = 8192, DF_COATTN_ALL_ROWS = 32768,
  DF_COATTN_META_AHEAD = 65536, DF_COATTN_FWD_ONE_UNIT = 131072, DF_PULL_OLD_FORM = 262144
};
// (bits 20 .. 23 are no switch but a number: the chunk length of the co-attention forward, 0 = the launcher's rule)
static inline int coattn_fwd_ch_of(const score_state_t* st) { return (st->debug_flags >> 20) & 15; }
// (DF_G4R_COMPOSED / Flags.g4r_composed, bit 13, reads "one recurrence per launch": GRU4Rec's composed form, and DEEMS's two
//  recurrences as one launch per side instead of one grouped launch)
struct Flags {
  bool gru_stepwise, head_fused_any_b, gru_f32_rec, no_panel, panel_dx, sort_lib, head_unfused, attn_unfused, sort_own, no_ps,
      ps_fwd_only, ps_bwd_only, one_stream, g4r_composed, coattn_all_rows, coattn_meta_ahead, coattn_fwd_one_unit, pull_old_form;
};
static inline Flags flags_of(const score_state_t* st) {
  auto on = [st](int bit) { return (st->debug_flags & bit) != 0; };
  Flags o;
  o.gru_stepwise = on(DF_GRU_STEPWISE); o.head_fused_any_b = on(DF_HEAD_FUSED_ANY_B); o.gru_f32_rec = on(DF_GRU_F32_REC);
  o.no_panel = on(DF_NO_PANEL); o.panel_dx = on(DF_PANEL_DX); o.sort_lib = on(DF_SORT_LIB); o.sort_own = on(DF_SORT_OWN);
  o.head_unfused = on(DF_HEAD_UNFUSED); o.attn_unfused = on(DF_ATTN_UNFUSED); o.no_ps = on(DF_NO_PS);
  o.ps_fwd_only = on(DF_PS_FWD_ONLY); o.ps_bwd_only = on(DF_PS_BWD_ONLY); o.one_stream = on(DF_ONE_STREAM);
  o.g4r_composed = on(DF_G4R_COMPOSED); o.coattn_all_rows = on(DF_COATTN_ALL_ROWS);
  o.coattn_meta_ahead = on(DF_COATTN_META_AHEAD); o.coattn_fwd_one_unit = on(DF_COATTN_FWD_ONE_UNIT);
  o.pull_old_form = on(DF_PULL_OLD_FORM);
  return o;
}
// Flags.one_stream (debug_flags bit 12): no second stream at all -- everything the passes would fork runs on the caller's
// stream, in launch order (the context's events are still recorded and waited for: on one stream those are no-ops).  What a
// suspected stream race is compared against.
static int side_stream(const score_state_t* st, hipStream_t s, SideStream** out) {
  SideStream* real = nullptr;
  SCORE_TRY(side_stream(st, &real));
  if (!st || !flags_of(st).one_stream) { *out = real; return 0; }
  static thread_local SideStream inl;
  const hipStream_t was = inl.fwd_on;
  inl = *real; inl.st = s; inl.fwd_on = was;
  *out = &inl;
  return 0;
}
// the side stream behind everything `s` holds so far
static inline int fork_side(SideStream* side, hipStream_t s) {
  HIPTRY(hipEventRecord(side->fork, s));
  HIPTRY(hipStreamWaitEvent(side->st, side->fork, 0));
  return 0;
}

#define G(call) SCORE_TRY(call)
// every GEMM of the path goes through here: ORs in the caller's product mode (score_state_t.gemm_mode)
static inline int gemm_mode_call(int x3, int tr, int M, int N, int K, const float* A, int lda, const float* B,
                                 int ldb, float* C, int ldc, const float* bias, int flags, float keep,
                                 const uint8_t* mask, uint64_t seed, float* scratch, int64_t scratch_floats,
                                 void* s) {
  return score_gemm(tr, M, N, K, A, lda, B, ldb, C, ldc, bias, flags | x3, keep, mask, seed, scratch, scratch_floats,
                    s);
}
// optional stage boundary events (hipEvent_t handles) recorded on the launch stream
#define EV(i) \
  do { if (stage_events && stage_events[i]) HIPTRY(hipEventRecord((hipEvent_t)stage_events[i], s)); } while (0)

// ---------------------------------------------------------------- what a pass and its helpers share
// ids at or past this row count are out of range (the kernels compare 32-bit ids)
static inline uint32_t clamp_rows(int64_t n) { return (uint32_t)(n < 0x80000000ll ? n : 0x80000000ll); }
static inline int global_batch(const score_state_t* st, int B) { return st->global_batch > 0 ? st->global_batch : B; }

struct Pass {
  Dims d; Params P; WS w; Flags fl;
  const score_state_t* st; const score_batch_t* bt;
  int B, T, BT, H;           // T: the time slices computed (active_T)
  int x3, Bg;                // GF_X3 under score_state_t.gemm_mode 1; the batch the loss is averaged over
  uint32_t n_rows;           // score_state_t.n_table_rows, clamped
  int64_t weff_stride;
  float rs;                  // bn1 at inference statistics: 1 / sqrt(1 + eps)
  float* ws; const float* W; float* scratch;
  hipStream_t s;             // the launch stream
};
// c->d comes from make_dims; st / bt have passed the entry point's argument checks
static int pass_fill(Pass* c, const score_state_t* st, const score_batch_t* bt, void* stream) {
  const Dims& d = c->d;
  build_layout(d, nullptr, 0, &c->P);
  c->st = st; c->bt = bt; c->fl = flags_of(st);
  c->B = bt->B; c->T = active_T(d, bt); c->H = d.H; c->BT = c->B * c->T;
  build_ws(d, c->B, &c->w);
  if (c->w.total * 4 > st->workspace_bytes) return SCORE_E_WORKSPACE;
  c->x3 = st->gemm_mode == 1 ? GF_X3 : 0; c->Bg = global_batch(st, c->B); c->n_rows = clamp_rows(st->n_table_rows);
  c->weff_stride = weff_copy_stride(d); c->rs = (float)(1.0 / sqrt(1.0 + 1e-3));
  c->ws = st->workspace; c->W = st->w; c->scratch = c->ws + c->w.scratch;
  c->s = (hipStream_t)stream;
  return 0;
}
// side sd's block of the concatenated [Wx_gates | Wx_cand ; b_gates | b_cand] copy (score_launch_weight_prep)
static inline const float* wxcat(const Pass& c, int sd) { return c.ws + c.w.wxcat + (int64_t)sd * (c.d.Ic + 1) * 3 * c.H; }
// what the step derives from the weights alone, in ONE launch: the [Wx_gates | Wx_cand] copies for the hoisted GRU input
// projections, the folded first attention layer (dense_3 on [q, k, q-k, q*k], head.hip) and the L2 norm's partial sums
// (three launches before round 4: the reference's own batch sizes are bound by the host's launch calls)
static int weight_prep(const Pass& c, hipStream_t on) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w; const float* W = c.W;
  return score_launch_weight_prep(W + P.gk[0], W + P.ck[0], W + P.gb[0], W + P.cb[0], W + P.gk[1], W + P.ck[1], W + P.gb[1],
                                  W + P.cb[1], d.Is[0], d.Is[1], d.Ic, d.H, c.ws + w.wxcat, d.Dk, AT1,
                                  d.attn ? W + P.at_w[1] : nullptr, c.ws + w.weff, c.ws + w.wq, SCORE_WEFF_COPIES, c.weff_stride, W,
                                  P.n_reg, c.ws + w.part, on);
}

// the GRUs' input rows of side sd, as the backward pass's queued weight gradients read them: the gather's output, GCMC's Z, or
// (GRU4Rec's layer 2) layer 1's outputs; x_ld is their stride
static inline const float* gru_x_rows(const Pass& c, int sd) {
  return c.ws + (c.d.family == FAM_GCMC ? c.w.gcmc_z[sd] : (c.d.family == FAM_G4R && sd == 1) ? c.w.gru_out[0] : c.w.xside[sd]);
}

// ---------------------------------------------------------------- the recurrences' argument blocks
static void gru_header(const Pass& c, GruArgs* ga) {
  memset(ga, 0, sizeof(*ga));
  ga->B = c.B; ga->T = c.T; ga->H = c.H; ga->length = c.bt->length;
  ga->nw8 = 1;     // H = 128: two waves per SIMD hide the LDS/epilogue latency (measured -0.08 ms/step)
  ga->tmp = c.ws + c.w.gru_tmp; ga->tmp_floats = c.w.gru_tmp_floats;
  ga->x3 = c.x3 != 0; ga->x3_rec = ga->x3 && !c.fl.gru_f32_rec; ga->stepwise = c.fl.gru_stepwise;
}
// a side's h rows of its kernels, its saved outputs and gates: what both directions read
static void gru_side(const Pass& c, int sd, GruSide* g) {
  const int H = c.H;
  g->Wg = c.W + c.P.gk[sd] + (int64_t)c.d.Is[sd] * 2 * H; g->ldwg = 2 * H;
  g->Wc = c.W + c.P.ck[sd] + (int64_t)c.d.Is[sd] * H; g->ldwc = H;
  g->out = c.ws + c.w.gru_out[sd]; g->ldo = H; g->gates = c.ws + c.w.gates[sd];
}
// the rows a backward recurrence leaves for the queued weight-gradient products
static void gru_side_saved(const Pass& c, int sd, GruSide* g) {
  g->dxproj = c.ws + c.w.dxproj[sd]; g->rh = c.ws + c.w.rh[sd]; g->hprev = c.ws + c.w.hprev[sd];
}
// per-workgroup column sums of dxproj (the recurrence's bias gradients), where the kernel that runs provides them; one row per
// 16 samples at most: far inside the scratch that only the other recurrence kernels use (null: no room)
static float* gru_bias_slab(const Pass& c, int sd) {
  const int64_t stride = (int64_t)(c.B / 16 + 1) * 3 * c.H;
  return 2 * stride <= c.w.gru_tmp_floats ? c.ws + c.w.gru_tmp + sd * stride : nullptr;
}
// a one-layer-per-launch backward recurrence's side: dL/d out, dL/d final state (or null) and everything it writes
static void gru_side_bwd(const Pass& c, int sd, const float* dfinal, GruSide* g) {
  g->dout = c.ws + c.w.dgru[sd]; g->lddo = c.H; g->dfinal = dfinal;
  gru_side_saved(c, sd, g);
  g->bias_slab = gru_bias_slab(c, sd);
}

// ---------------------------------------------------------------- GRU4Rec's two stacked recurrences (point_model.py:129-132)
// The stacked kernel (gru_stack.hip: both layers in one launch, layer 2 one step behind layer 1) or, with Flags.g4r_composed
// and at every H it does not cover, the COMPOSED form: layer 1's recurrence, the GEMM that projects its outputs, layer 2's
// recurrence -- the kernels of the other model types, one layer per launch -- and the mirror image backward.
static bool g4r_stacked(const Dims& d, const Flags& fl) {
  return !fl.g4r_composed && !fl.gru_stepwise && score_gru_stack_ok(d.H);
}
// one layer's GruSide in either form and direction (no dout, no bias slab: the stacked kernel takes neither); layer 2 alone
// has a final state
static void g4r_side(const Pass& c, int l, GruSide* g) {
  gru_side(c, l, g);
  g->xproj = c.ws + c.w.xproj[l]; g->final_state = l ? c.ws + c.w.gru_final[1] : nullptr;
  gru_side_saved(c, l, g);
}
static void g4r_stack_args(const Pass& c, GruStackArgs* a) {
  memset(a, 0, sizeof(*a));
  a->B = c.B; a->T = c.T; a->H = c.H; a->length = c.bt->length;
  for (int l = 0; l < 2; ++l) g4r_side(c, l, &a->l[l]);
  a->Wg2 = c.W + c.P.gk[1]; a->Wc2 = c.W + c.P.ck[1]; a->bg2 = c.W + c.P.gb[1]; a->bc2 = c.W + c.P.cb[1];
}
static int g4r_grus_fwd(const Pass& c) {
  const Dims& d = c.d; const WS& w = c.w; float* ws = c.ws; hipStream_t s = c.s;
  const int H = c.H, BT = c.BT;
  // layer 1's hoisted projection of the gathered rows: x . [Wx_gates | Wx_cand] + [b_gates | b_cand]
  G(gemm_mode_call(c.x3, 0, BT, 3 * H, d.Di, ws + w.xside[0], d.I, wxcat(c, 0), 3 * H, ws + w.xproj[0], 3 * H,
                   wxcat(c, 0) + (int64_t)d.Di * 3 * H, GF_BIAS, 1.f, nullptr, 0, c.scratch, w.scratch_floats, s));
  if (g4r_stacked(d, c.fl)) {
    GruStackArgs a;
    g4r_stack_args(c, &a);
    return score_gru_stack_fwd(a, s);
  }
  for (int l = 0; l < 2; ++l) {
    if (l == 1)     // layer 2's input rows are layer 1's outputs (zero past the length)
      G(gemm_mode_call(c.x3, 0, BT, 3 * H, H, ws + w.gru_out[0], H, wxcat(c, 1), 3 * H, ws + w.xproj[1], 3 * H,
                       wxcat(c, 1) + (int64_t)H * 3 * H, GF_BIAS, 1.f, nullptr, 0, c.scratch, w.scratch_floats, s));
    GruArgs ga;
    gru_header(c, &ga);
    g4r_side(c, l, &ga.s[0]);
    G(score_gru_fwd_multi(ga, 1, s));
  }
  return 0;
}
// dfinal2: dL/d layer 2's final state [B, H].  Leaves both layers' dxproj / rh / hprev rows for the queued weight-gradient
// products; *bias_rows as GruArgs.bias_slab_rows
static int g4r_grus_bwd(const Pass& c, const float* dfinal2, int* bias_rows) {
  const WS& w = c.w; const int H = c.H;
  *bias_rows = 0;
  if (g4r_stacked(c.d, c.fl)) {
    GruStackArgs a;
    g4r_stack_args(c, &a);
    a.l[1].dfinal = dfinal2;
    return score_gru_stack_bwd(a, c.s);
  }
  for (int l = 1; l >= 0; --l) {
    GruArgs ga;
    gru_header(c, &ga);
    g4r_side(c, l, &ga.s[0]);
    gru_side_bwd(c, l, l ? dfinal2 : nullptr, &ga.s[0]);       // (dgru[1]: zeros, only the final state is read)
    G(score_gru_bwd_multi(ga, 1, c.s));
    *bias_rows = ga.bias_slab_rows;
    if (l == 1)     // layer 2's input gradient is layer 1's dout: [dgates | dcand] . [Wx_gates | Wx_cand]^T
      G(gemm_mode_call(c.x3, 1, c.BT, H, 3 * H, c.ws + w.dxproj[1], 3 * H, wxcat(c, 1), 3 * H, c.ws + w.dgru[0], H, nullptr, 0, 1.f,
                       nullptr, 0, c.scratch, w.scratch_floats, c.s));
  }
  return 0;
}

// ---------------------------------------------------------------- Caser's two convolutions (point_model.py:147-160, caser.hip)
// X = the gathered user_seq rows: columns [0, Di) of xside[0]; the backward pass writes every column of dxside[0] (zeros past Di)
static void caser_args(const Pass& c, float* gw, CaserArgs* a) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w; float* ws = c.ws; const float* W = c.W;
  memset(a, 0, sizeof(*a));
  a->B = c.B; a->T = d.T; a->C = d.Di; a->ldx = d.I; a->ldh = d.Dhead;
  a->X = ws + w.xside[0]; a->Wh = W + P.cs_wh; a->bh = W + P.cs_bh; a->Wv = W + P.cs_wv; a->bv = W + P.cs_bv;
  a->wd = W + P.cs_wd; a->bd = W + P.cs_bd;
  a->head = ws + w.head_inp; a->hwin = ws + w.caser_hwin; a->arg = reinterpret_cast<int32_t*>(ws + w.caser_arg); a->v = ws + w.caser_v;
  a->dhead = ws + w.dhead; a->dX = ws + w.dxside[0];
  if (gw) {
    a->gWh = gw + P.cs_wh; a->gbh = gw + P.cs_bh; a->gWv = gw + P.cs_wv; a->gbv = gw + P.cs_bv; a->gwd = gw + P.cs_wd; a->gbd = gw + P.cs_bd;
  }
}

// ---------------------------------------------------------------- DELF (point_model.py:200-249, delf.hip)
// Side 0: X = the gathered user_seq rows (columns [0, Di) of xside[0]) against target_item through dense; side 1: the item_seq
// rows (columns [0, Du) of xside[1]) against target_user through dense_1, masked by score_batch_t.length2.  The backward kernel
// writes every column of both dxside and the target rows' gradients into dhead ([d target_item | d target_user])
static void delf_args(const Pass& c, DelfArgs* a) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w; float* ws = c.ws; const float* W = c.W;
  memset(a, 0, sizeof(*a));
  a->B = c.B; a->T = c.T; a->Cu = d.Du; a->Ci = d.Di; a->ldq = d.Dq; a->ldh = d.Dhead; a->off_ti = d.off_ti; a->off_tu = d.off_tu;
  a->Bglobal = c.Bg;
  const int Cx[2] = {d.Di, d.Du};
  const int32_t* len[2] = {c.bt->length, c.bt->length2};
  for (int s = 0; s < 2; ++s) {
    DelfSide& S = a->s[s];
    S.X = ws + w.xside[s]; S.ldx = d.I; S.C = Cx[s]; S.W = W + P.dl_w[s]; S.b = W + P.dl_b[s]; S.len = len[s];
    S.key = ws + w.delf_key[s]; S.att = ws + w.delf_att[s]; S.rep = ws + w.delf_rep[s]; S.ds = ws + w.delf_ds[s];
    S.dX = ws + w.dxside[s]; S.dpre = ws + w.delf_dpre[s];
  }
  a->tu = ws + w.query; a->ti = ws + w.query + d.Du;       // [target_user | target_item] (score_launch_target_fwd)
  for (int k = 0; k < 4; ++k) {
    a->A[k] = W + P.dl_w[2 + 2 * k]; a->a1[k] = W + P.dl_b[2 + 2 * k];
    a->Bm[k] = W + P.dl_w[3 + 2 * k]; a->b2[k] = W + P.dl_b[3 + 2 * k];
  }
  a->w = W + P.dl_w[10]; a->c = W + P.dl_b[10];
  a->label = c.bt->label;
  a->act = ws + w.delf_act; a->dact = ws + w.delf_dact; a->logit = ws + w.logit; a->y = ws + w.y_pred; a->lossb = ws + w.lossb;
  a->dlogit = ws + w.dlogit; a->dhead = ws + w.dhead;
}
// ---------------------------------------------------------------- SVD++ (point_model.py:167-198, svdpp.hip)
// X = the gathered user_seq rows (columns [0, Di) of xside[0]) under score_batch_t.length; the backward kernel writes every column
// of dxside[0], the target rows' gradients into dhead ([d target_item | d target_user]) and the weight gradients' per-sample partials
static void svdpp_args(const Pass& c, SvdppArgs* a) {
  const Dims& d = c.d; const WS& w = c.w; float* ws = c.ws;
  memset(a, 0, sizeof(*a));
  a->B = c.B; a->T = c.T; a->D = d.D; a->Fu = d.Fu; a->Fi = d.Fi; a->ldx = d.I; a->ldq = d.Dq; a->ldh = d.Dhead;
  a->off_ti = d.off_ti; a->off_tu = d.off_tu; a->Bglobal = c.Bg;
  a->X = ws + w.xside[0]; a->tu = ws + w.query; a->ti = ws + w.query + d.Du;       // [target_user | target_item] (score_launch_target_fwd)
  a->wu = c.W + c.P.sv_w; a->wi = c.W + c.P.sv_w + 4 * (int64_t)d.Fu;
  a->length = c.bt->length; a->label = c.bt->label;
  a->act = ws + w.svdpp_act; a->logit = ws + w.logit; a->y = ws + w.y_pred; a->lossb = ws + w.lossb; a->dlogit = ws + w.dlogit;
  a->dX = ws + w.dxside[0]; a->dhead = ws + w.dhead; a->dwpart = ws + w.svdpp_dw;
}
// ---------------------------------------------------------------- SASRec (point_model.py:313-469, sasrec.hip)
// X = the gathered user_seq rows (columns [0, Di) of xside[0]), all T positions; score_batch_t.length masks rep / final only.  The
// head's rows live in regions of their own (R per batch, not B); the backward kernel writes every column of dxside[0] and the target
// rows' gradients into dhead ([d target_item | d target_user]).  share: keep_prob = 1, the negative rows ride on the positive ones
static void sasrec_args(const Pass& c, float keep_prob, const uint8_t* mask0, const uint8_t* mask1, uint64_t seed, SasrecArgs* a) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w; float* ws = c.ws; const float* W = c.W;
  memset(a, 0, sizeof(*a));
  a->B = c.B; a->T = d.T; a->C = d.Di; a->Cu = d.Du; a->Dh = 2 * d.Di + d.Du; a->ldx = d.I; a->ldq = d.Dq; a->ldh = d.Dhead;
  a->off_ti = d.off_ti; a->off_tu = d.off_tu; a->Bglobal = c.Bg; a->share = keep_prob >= 1.f ? 1 : 0;
  a->X = ws + w.xside[0]; a->tu = ws + w.query; a->ti = ws + w.query + d.Du;       // [target_user | target_item] (score_launch_target_fwd)
  a->beta = W + P.sa_beta; a->gamma = W + P.sa_gamma;
  a->Wq = W + P.sa_w[0]; a->bq = W + P.sa_b[0]; a->Wk = W + P.sa_w[1]; a->bk = W + P.sa_b[1]; a->Wv = W + P.sa_w[2]; a->bv = W + P.sa_b[2];
  a->W3 = W + P.fc_w[2]; a->b3 = W + P.fc_b[2];
  a->length = c.bt->length; a->label = c.bt->label;
  a->mask0 = mask0; a->mask1 = mask1; a->mask_a = c.st->drop_mask2;
  a->keep = keep_prob; a->seed = seed; a->seed_dev = c.st->step_scalars ? &c.st->step_scalars->drop_seed : nullptr;
  a->nrm = ws + w.sas_nrm; a->rstd = ws + w.sas_rstd; a->km = ws + w.sas_km; a->qin = ws + w.sas_qin; a->q = ws + w.sas_q;
  a->k = ws + w.sas_k; a->v = ws + w.sas_v; a->yseq = ws + w.sas_y; a->p = ws + w.sas_p; a->att = ws + w.sas_att; a->fin = ws + w.sas_fin;
  a->hin = ws + w.sas_hin; a->z1 = ws + w.sas_z1; a->f1 = ws + w.sas_f1; a->z2 = ws + w.sas_z2; a->f2 = ws + w.sas_f2;
  a->rlogit = ws + w.sas_logit; a->dlogit = ws + w.sas_dlogit; a->dz2 = ws + w.sas_dz2; a->dz1e = ws + w.sas_dz1e; a->dz1 = ws + w.sas_dz1;
  a->dhin = ws + w.sas_dhin; a->logit = ws + w.logit; a->ypred = ws + w.y_pred; a->lossb = ws + w.lossb;
  a->dq = ws + w.sas_dq; a->dk = ws + w.sas_dk; a->dv = ws + w.sas_dv; a->dX = ws + w.dxside[0]; a->dhead = ws + w.dhead;
  a->dgamma = ws + w.sas_dgamma; a->dbeta = ws + w.sas_dbeta;
}
// rows of fc1's GEMM (positive + final) and of everything behind it (+ the negative rows, unless shared)
static inline int sasrec_rows1(const Pass& c) { return c.B * c.d.T; }
static inline int sasrec_rows(const Pass& c, const SasrecArgs& a) { return c.B * c.d.T + (a.share ? 0 : c.B * (c.d.T - 2)); }
// ---------------------------------------------------------------- DEEMS (point_model.py:281-311, deems.hip)
// The two recurrences: side 0 = gru1 over the user_seq rows under score_batch_t.length, side 1 = gru2 over the item_seq rows under
// length2.  On the register kernels of gru.hip both run as ONE grouped launch each way, each side reading its own lengths
// (GruSide.length); every other route, and Flags.g4r_composed ("one recurrence per launch"), runs one call per side with that
// side's lengths in GruArgs.length -- the same kernels on the same rows either way.
static const int32_t* deems_length(const Pass& c, int sd) { return sd ? c.bt->length2 : c.bt->length; }
// both sides' arguments as the grouped launch takes them (bwd: with what the backward recurrence reads and writes)
static void deems_gru_args(const Pass& c, GruArgs* ga, const float* const* dfinal) {
  gru_header(c, ga);
  for (int sd = 0; sd < 2; ++sd) {
    GruSide& g = ga->s[sd];
    gru_side(c, sd, &g);
    g.xproj = c.ws + c.w.xproj[sd]; g.final_state = c.ws + c.w.gru_final[sd]; g.length = deems_length(c, sd);
    if (dfinal) gru_side_bwd(c, sd, dfinal[sd], &g);
  }
}
static bool deems_grouped(const Pass& c, const GruArgs& ga) { return !c.fl.g4r_composed && score_gru_reg_route(ga, 2); }
// side sd alone, its lengths the call's
static void deems_one_side(const Pass& c, const GruArgs& both, int sd, GruArgs* one) {
  gru_header(c, one);
  one->s[0] = both.s[sd]; one->s[0].length = nullptr;
  one->length = deems_length(c, sd);
}
static int deems_grus_fwd(const Pass& c) {
  const Dims& d = c.d; const WS& w = c.w; float* ws = c.ws; const int H = c.H;
  for (int sd = 0; sd < 2; ++sd) {     // x . [Wx_gates | Wx_cand] + [b_gates | b_cand]: one GEMM per side (Is[0] != Is[1])
    const float* cat = wxcat(c, sd);
    G(gemm_mode_call(c.x3, 0, c.BT, 3 * H, d.Is[sd], ws + w.xside[sd], d.I, cat, 3 * H, ws + w.xproj[sd], 3 * H,
                     cat + (int64_t)d.Is[sd] * 3 * H, GF_BIAS, 1.f, nullptr, 0, c.scratch, w.scratch_floats, c.s));
  }
  GruArgs ga;
  deems_gru_args(c, &ga, nullptr);
  if (deems_grouped(c, ga)) return score_gru_fwd_multi(ga, 2, c.s);
  for (int sd = 0; sd < 2; ++sd) {
    GruArgs one;
    deems_one_side(c, ga, sd, &one);
    G(score_gru_fwd_multi(one, 1, c.s));
  }
  return 0;
}
static int deems_grus_bwd(const Pass& c, const float* const* dfinal, int* bias_rows) {
  GruArgs ga;
  deems_gru_args(c, &ga, dfinal);
  if (deems_grouped(c, ga)) {
    G(score_gru_bwd_multi(ga, 2, c.s));
    *bias_rows = ga.bias_slab_rows;
    return 0;
  }
  for (int sd = 0; sd < 2; ++sd) {
    GruArgs one;
    deems_one_side(c, ga, sd, &one);
    G(score_gru_bwd_multi(one, 1, c.s));
    *bias_rows = one.bias_slab_rows;
  }
  return 0;
}
// tower k's variables and buffers: 0 = the user tower on columns [0, H + Du) of a head_inp row, 1 = the item tower on the rest
struct DeemsVars { int64_t bn_g, bn_b; const int64_t* fc_w; const int64_t* fc_b; };
static DeemsVars deems_vars(const Params& P, int k) {
  return k ? DeemsVars{P.bn_g2, P.bn_b2, P.fc_w2, P.fc_b2} : DeemsVars{P.bn_g, P.bn_b, P.fc_w, P.fc_b};
}
static void deems_args(const Pass& c, float keep_prob, const uint8_t* mask0, const uint8_t* mask1, uint64_t seed, DeemsArgs* a) {
  const Dims& d = c.d; const WS& w = c.w; float* ws = c.ws; const float* W = c.W; const int B = c.B;
  memset(a, 0, sizeof(*a));
  a->B = B; a->H = c.H; a->ld = d.Dhead; a->Bglobal = c.Bg;
  a->x = ws + w.head_inp; a->bn = ws + w.bn; a->dbn = ws + w.dbn; a->dhead = ws + w.dhead; a->tmp = ws + w.dgstage;
  a->rs = c.rs; a->keep = keep_prob; a->seed0 = seed;
  a->seed_dev = c.st->step_scalars ? &c.st->step_scalars->drop_seed : nullptr;
  a->label = c.bt->label; a->y_pred = ws + w.y_pred; a->lossb = ws + w.lossb;
  const int64_t f1[2] = {w.f1, w.deems_f1}, f2[2] = {w.f2, w.deems_f2}, dz1[2] = {w.dz1, w.deems_dz1}, dz2[2] = {w.dz2, w.deems_dz2};
  for (int k = 0; k < 2; ++k) {
    DeemsTower& t = a->t[k];
    const DeemsVars v = deems_vars(c.P, k);
    t.h = ws + w.gru_final[k];
    t.gamma = W + v.bn_g; t.beta = W + v.bn_b;
    t.W1 = W + v.fc_w[0]; t.b1 = W + v.fc_b[0]; t.W2 = W + v.fc_w[1]; t.b2 = W + v.fc_b[1]; t.W3 = W + v.fc_w[2]; t.b3 = W + v.fc_b[2];
    // score_forward's masks cover both towers, the user tower first: [2, B, 200] and [2, B, 80]
    t.mask0 = mask0 ? mask0 + (int64_t)k * B * FC1 : nullptr; t.mask1 = mask1 ? mask1 + (int64_t)k * B * FC2 : nullptr;
    t.f1 = ws + f1[k]; t.f2 = ws + f2[k]; t.dz1 = ws + dz1[k]; t.dz2 = ws + dz2[k];
    t.logit = ws + w.deems_logit + (int64_t)k * B; t.y = ws + w.deems_y + (int64_t)k * B; t.dlogit = ws + w.deems_dlogit + (int64_t)k * B;
    t.Dh = c.H + (k ? d.Di : d.Du); t.col = k ? d.off_i : d.off_u;
  }
}
// does score_forward's fused head run (and leave dz2)?
static bool deems_head_fused(const Pass& c) {
  return !c.fl.head_unfused && score_deems_head_fwd_fits(c.H + c.d.Du, c.H + c.d.Di);
}

// ---------------------------------------------------------------- the two co-attention calls
// 1: (user_1hop, item_2hop, target_item) ; 2: (user_2hop, item_1hop, target_user)  (score.py:196-197)
// user_side = [user_1hop_seq | user_2hop_seq], item_side = [item_1hop_seq | item_2hop_seq]   (:200-201)
// What the forward and the backward pass share; col1 / col2 / info_col[i]: where call i's two outputs start in a row of
// the user side, of the item side and of atten_info -- each pass points its own regions there
struct CoattnCols { int col1[2], col2[2], info_col[2]; };
static void coattn_args(const Pass& c, CoattnArgs* ca, CoattnCols* k) {
  const Dims& d = c.d;
  memset(ca, 0, sizeof(*ca));
  ca->table = c.st->table; ca->K = d.K; ca->T = c.T; ca->Tidx = d.T; ca->mode = d.coattn ? 0 : 1; ca->n_rows = c.n_rows;
  const int32_t* idx1[2] = {c.bt->user_1hop, c.bt->user_2hop};
  const int32_t* idx2[2] = {c.bt->item_2hop, c.bt->item_1hop};
  for (int i = 0; i < 2; ++i) {
    CoattnCall& cc = ca->c[i];
    cc.idx1 = idx1[i]; cc.idx2 = idx2[i]; cc.W = d.coattn ? c.W + c.P.ca_w[i] : nullptr; cc.rsave = c.ws + c.w.rsave[i];
    cc.ld1 = d.I; cc.ld2 = d.I; cc.ldi = 4 * d.K; cc.F = i ? d.Fu : d.Fi;
    k->col1[i] = i ? d.Di : 0; k->col2[i] = i ? 0 : d.Du; k->info_col[i] = i * 2 * d.K;
  }
}

// ---------------------------------------------------------------- panel GEMM groups (gemm_panel.hip)
// The two sides' GRU input projections (which = 0: [BT, Is] . cat -> 3H columns) or their input gradients (which = 1:
// [BT, 3H] . cat^T -> Is columns), each side's output columns as `ns` column halves: group g is side g / ns, half g % ns.
// src: the block of the concatenated copy a group's image is made of (trans: as score_gemm_panel_prep takes it)
struct PanelGroups { int n, Nh, K, trans, lda, ldc; const float* src[4]; float* img[4]; PanelGroup pg[4]; };
static void panel_groups(const Pass& c, int which, const float* const* A, float* const* C, PanelGroups* p) {
  const Dims& d = c.d; const int H = c.H;
  const int ns = which == 0 ? panel_x_splits(H) : panel_d_splits(d.Is[0]);
  p->n = 2 * ns; p->Nh = (which == 0 ? 3 * H : d.Is[0]) / ns; p->K = which == 0 ? d.Is[0] : 3 * H; p->trans = which == 0;
  p->lda = which == 0 ? x_ld(d, 0) : 3 * H; p->ldc = which == 0 ? 3 * H : d.I;
  const int64_t per = score_gemm_panel_image_floats(p->Nh, p->K);
  for (int g = 0; g < p->n; ++g) {
    const int side = g / ns, half = g % ns;
    const float* cat = wxcat(c, side);
    p->src[g] = which == 0 ? cat + half * p->Nh : cat + (int64_t)half * p->Nh * 3 * H;
    p->img[g] = c.ws + (which == 0 ? c.w.pimg_x : c.w.pimg_d)[side] + half * per;
    PanelGroup& pg = p->pg[g];
    pg.A = A ? A[side] : nullptr; pg.img = p->img[g]; pg.C = C ? C[side] + half * p->Nh : nullptr;
    pg.bias = which == 0 ? cat + (int64_t)d.Is[side] * 3 * H + half * p->Nh : nullptr;    // (each side's own bias row)
  }
}
// the weights as fragment images
static int panel_prep(const Pass& c, int which, hipStream_t on) {
  PanelGroups p;
  panel_groups(c, which, nullptr, nullptr, &p);
  return score_gemm_panel_prep(p.n, p.src, 3 * c.H, p.trans, p.Nh, p.K, p.img, on);
}
static int panel_launch(const Pass& c, int which, const float* const* A, float* const* C) {
  PanelGroups p;
  panel_groups(c, which, A, C, &p);
  return score_gemm_panel(p.n, p.pg, c.BT, p.Nh, p.K, p.lda, p.ldc, c.s);
}

// ---------------------------------------------------------------- the loss reduction behind a head
// One workgroup, no reader inside the step: with score_state_t.loss_done_event it runs on the side stream, so the backward
// pass's first launch follows the head directly
// n per-sample terms at lossb, averaged over Bg samples, into loss[0..3] (the ranking pass: its own terms and the caller's loss)
static int loss_tail_at(const Pass& c, SideStream* sd, float reg_lambda, int n, const float* lossb, float* loss, int Bg) {
  hipStream_t ls = c.s;
  if (c.st->loss_done_event) { G(fork_side(sd, c.s)); ls = sd->st; }
  G(score_launch_loss_final(n, lossb, loss, reg_lambda, c.ws + c.w.part, Bg, ls, c.st->id_status));
  if (c.st->loss_done_event) HIPTRY(hipEventRecord((hipEvent_t)c.st->loss_done_event, ls));
  return 0;
}
static int loss_tail(const Pass& c, SideStream* sd, float reg_lambda) {
  return loss_tail_at(c, sd, reg_lambda, c.B, c.ws + c.w.lossb, c.ws + c.w.loss, c.Bg);
}

// ---------------------------------------------------------------- embedding rows (score.py:51-66): the sorted pull-form scatter
// plan: the workspace that holds this batch's sorted occurrences (score_index_plan wrote them there): the pass's own, or
// score_state_t.plan_workspace -- the plan sorted into ANOTHER workspace of the same layout, a step ahead.  Everything else,
// the unique positions of scatter_mode 2 among it, is read from the pass's own workspace.
static int row_scatter(const Pass& c, float* plan, float* grad_table) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w; float* ws = c.ws; const float* W = c.W;
  PullArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.D = d.D; pa.K = d.K; pa.zero_is_dummy = 1;
  pa.flags = c.st->scatter_mode == 0 ? c.st->row_flags : nullptr;
  pa.uid = c.st->scatter_mode == 2 ? reinterpret_cast<const uint32_t*>(ws + w.uid) : nullptr;
  pa.force_old = c.fl.pull_old_form ? 1 : 0;               // (debug_flags bit 18: pull_kernel, A/B against pull_kernel_lanes)
  const int nf[6] = {d.Fi, d.Fi, d.Fu, d.Fu, d.Fu, d.Fi};  // features of the six index tensors, as score_index_plan enumerates them
  for (int g = 0; g < 6; ++g) { pa.nf[g] = nf[g]; pa.rows[g] = g < 4 ? (int64_t)c.B * c.T : (int64_t)c.B; }
  const float invK = 1.0f / (float)d.K;
  const float* Gm[6] = {ws + w.dxside[0], ws + w.dxside[1], ws + w.dxside[0], ws + w.dxside[1], ws + w.dtgt, ws + w.dtgt};
  const int ldg[6] = {d.I, d.I, d.I, d.I, d.Dq, d.Dq};
  const int gcol[6] = {0, d.Du, d.Di, 0, 0, d.Du};
  for (int g = 0; g < 6; ++g) { pa.G[g] = Gm[g]; pa.ldg[g] = ldg[g]; pa.gcol[g] = gcol[g]; pa.constA[g] = 1.0f; }
  if (d.coattn) {
    pa.cA[0] = ws + w.pcoef[0]; pa.cA[2] = ws + w.pcoef[1];
    pa.constA[1] = invK; pa.constA[3] = invK;
    pa.cB[0] = pa.cB[1] = ws + w.dzcoef[0]; pa.cB[2] = pa.cB[3] = ws + w.dzcoef[1];
    pa.Wv[0] = W + P.ca_w[0] + d.Di; pa.Wv[1] = W + P.ca_w[0] + 2 * d.Di;
    pa.Wv[2] = W + P.ca_w[1] + d.Du; pa.Wv[3] = W + P.ca_w[1] + 2 * d.Du;
  }
  const int64_t n_occ = (int64_t)c.B * (2 * (int64_t)c.T * d.K * (d.Fu + d.Fi) + d.Fu + d.Fi);   // what score_index_plan enumerated
  return score_launch_pull(pa, reinterpret_cast<uint32_t*>(plan + w.keys_out), reinterpret_cast<uint32_t*>(plan + w.vals_out),
                           n_occ + 1, grad_table, ws + w.partials, w.partial_floats, c.s);
}

// ---------------------------------------------------------------- the queued weight gradients and column sums of a backward pass
// Weight gradients C = X^T dY and bias gradients (column sums) have no consumer inside a pass: queued, issued together.  BOTH
// forms of the backward pass queue through these functions, in this order -- head, attention denses, query projection, the
// recurrence sides: the order within gq and within cq decides the grouping of the launches and the split-K slab of each
// product, and with them the bits.  Queueing is host bookkeeping; what is queued must be final when its queue is flushed.
struct GradQueues { GemmQueue gq; ColsumJobs cq; };
static inline void queues_init(GradQueues* q) { q->gq.n = 0; q->cq.n = 0; q->cq.part_used = 0; }
// build_fc_net (score.py:68-81).  bn1_sums: bn1's d gamma / d beta as column sums of what a fused kernel wrote (the
// layer-by-layer pass's score_launch_bn_bwd queues its own, at this place in cq)
static int queue_head(const Pass& c, GradQueues* q, float* gw, bool bn1_sums) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w; float* ws = c.ws; const int B = c.B;
  // fc3: dW = f2^T dlogit, db = sum dlogit
  G(gemm_queue_add(&q->gq, FC2, 1, B, ws + w.f2, FC2, ws + w.dlogit, 1, gw + P.fc_w[2], 1));
  G(colsum_queue_add(&q->cq, ws + w.dlogit, B, 1, 1, gw + P.fc_b[2], 0));
  // fc2
  G(gemm_queue_add(&q->gq, FC1, FC2, B, ws + w.f1, FC1, ws + w.dz2, FC2, gw + P.fc_w[1], FC2));
  G(colsum_queue_add(&q->cq, ws + w.dz2, B, FC2, FC2, gw + P.fc_b[1], 0));
  // fc1 + bn1
  G(gemm_queue_add(&q->gq, d.Dhead, FC1, B, ws + w.bn, d.Dhead, ws + w.dz1, FC1, gw + P.fc_w[0], FC1));
  G(colsum_queue_add(&q->cq, ws + w.dz1, B, FC1, FC1, gw + P.fc_b[0], 0));
  if (bn1_sums) {
    G(colsum_queue_add(&q->cq, ws + w.dgstage, B, d.Dhead, d.Dhead, gw + P.bn_g, 0));
    G(colsum_queue_add(&q->cq, ws + w.dbn, B, d.Dhead, d.Dhead, gw + P.bn_b, 0));
  }
  return 0;
}
// ... of one of DEEMS's towers: the same products and column sums on that tower's buffers and variables (bn's sums always from
// what the head's backward wrote: dgstage and dbn hold both towers' column ranges)
static int queue_head_tower(const Pass& c, GradQueues* q, float* gw, const DeemsArgs& a, int k) {
  const DeemsTower& t = a.t[k]; const DeemsVars v = deems_vars(c.P, k); const int B = c.B, ld = a.ld;
  G(gemm_queue_add(&q->gq, FC2, 1, B, t.f2, FC2, t.dlogit, 1, gw + v.fc_w[2], 1));
  G(colsum_queue_add(&q->cq, t.dlogit, B, 1, 1, gw + v.fc_b[2], 0));
  G(gemm_queue_add(&q->gq, FC1, FC2, B, t.f1, FC1, t.dz2, FC2, gw + v.fc_w[1], FC2));
  G(colsum_queue_add(&q->cq, t.dz2, B, FC2, FC2, gw + v.fc_b[1], 0));
  G(gemm_queue_add(&q->gq, t.Dh, FC1, B, a.bn + t.col, ld, t.dz1, FC1, gw + v.fc_w[0], FC1));
  G(colsum_queue_add(&q->cq, t.dz1, B, FC1, FC1, gw + v.fc_b[0], 0));
  G(colsum_queue_add(&q->cq, a.tmp + t.col, B, t.Dh, ld, gw + v.bn_g, 0));
  G(colsum_queue_add(&q->cq, a.dbn + t.col, B, t.Dh, ld, gw + v.bn_b, 0));
  return 0;
}
// the temporal attention's denses (score.py:169-186)
static int queue_attn(const Pass& c, GradQueues* q, float* gw) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w; float* ws = c.ws; const int B = c.B, BT = c.BT;
  // dense_5 (40 -> 1): dW = a2^T ds ; db = sum ds
  G(gemm_queue_add(&q->gq, AT2, 1, BT, ws + w.a2, AT2, ws + w.ds, 1, gw + P.at_w[3], 1));
  G(colsum_queue_add(&q->cq, ws + w.ds, BT, 1, 1, gw + P.at_b[3], 0));
  // dense_4 (80 -> 40); da2 is already relu-masked
  G(gemm_queue_add(&q->gq, AT1, AT2, BT, ws + w.a1, AT1, ws + w.da2, AT2, gw + P.at_w[2], AT2));
  G(colsum_queue_add(&q->cq, ws + w.da2, BT, AT2, AT2, gw + P.at_b[2], 0));
  // dense_3 (4Dk -> 80), folded: weight gradient from [k, q*k]^T da1 and q^T sum_t da1 (adzsum); gw + P.at_w[1] is assembled
  // from dweff / dwq after the queue is flushed
  G(gemm_queue_add(&q->gq, 2 * d.Dk, AT1, BT, ws + w.ainp, 2 * d.Dk, ws + w.da1, AT1, ws + w.dweff, AT1));
  G(colsum_queue_add(&q->cq, ws + w.da1, BT, AT1, AT1, gw + P.at_b[1], 0));
  G(gemm_queue_add(&q->gq, d.Dk, AT1, B, ws + w.q, d.Dk, ws + w.adzsum, AT1, ws + w.dwq, AT1));
  return 0;
}
// dense_2, the query projection
static int queue_query(const Pass& c, GradQueues* q, float* gw) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w;
  G(gemm_queue_add(&q->gq, d.Dq, d.Dk, c.B, c.ws + w.query, d.Dq, c.ws + w.dq, d.Dk, gw + P.at_w[0], d.Dk));
  G(colsum_queue_add(&q->cq, c.ws + w.dq, c.B, d.Dk, d.Dk, gw + P.at_b[0], 0));
  return 0;
}
// One recurrence's kernels and biases.  The kernels are [x ; h] row blocks (TF GRUCell), x rows first: the x rows of the two
// kernels straight into their gradients (same A panel, the column tiles of [dgates | dcand]), then the h rows.  The input rows
// are x_ld(d, sd) wide with Is[sd] columns read; the per-sample pass runs only model types where both are d.I and the rows
// are the gather's.  bias_rows > 0: the recurrence left per-workgroup column sums of dxproj (gru_bias_slab): a few dozen rows
// instead of B*T
static int queue_gru_side(const Pass& c, GradQueues* q, float* gw, int sd, int bias_rows) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w; float* ws = c.ws;
  const int H = c.H, BT = c.BT, Is = d.Is[sd], ld = x_ld(d, sd);
  float* dxp = ws + w.dxproj[sd];
  const float* xin = gru_x_rows(c, sd);
  G(gemm_queue_add(&q->gq, Is, 2 * H, BT, xin, ld, dxp, 3 * H, gw + P.gk[sd], 2 * H));
  G(gemm_queue_add(&q->gq, Is, H, BT, xin, ld, dxp + 2 * H, 3 * H, gw + P.ck[sd], H));
  G(gemm_queue_add(&q->gq, H, 2 * H, BT, ws + w.hprev[sd], H, dxp, 3 * H, gw + P.gk[sd] + (int64_t)Is * 2 * H, 2 * H));
  G(gemm_queue_add(&q->gq, H, H, BT, ws + w.rh[sd], H, dxp + 2 * H, 3 * H, gw + P.ck[sd] + (int64_t)Is * H, H));
  const float* rows = bias_rows > 0 ? gru_bias_slab(c, sd) : dxp;
  const int nrows = bias_rows > 0 ? bias_rows : BT;
  G(colsum_queue_add(&q->cq, rows, nrows, 2 * H, 3 * H, gw + P.gb[sd], 0));
  G(colsum_queue_add(&q->cq, rows + 2 * H, nrows, H, 3 * H, gw + P.cb[sd], 0));
  return 0;
}

// the 22 variables' gradients as queued X^T dY products and column sums of what the backward kernel left: dense / dense_1
// over the B * T rows of a side (masked rows: zero dpre), the fusion kernels over the B samples -- a kernel's rows in the two
// blocks its input is concatenated from
static int queue_delf(const Pass& c, GradQueues* q, float* gw) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w; float* ws = c.ws; const int B = c.B, BT = c.BT;
  const int Cx[2] = {d.Di, d.Du};
  for (int s = 0; s < 2; ++s) {
    G(gemm_queue_add(&q->gq, Cx[s], Cx[s], BT, ws + w.xside[s], d.I, ws + w.delf_dpre[s], Cx[s], gw + P.dl_w[s], Cx[s]));
    G(colsum_queue_add(&q->cq, ws + w.delf_dpre[s], BT, Cx[s], Cx[s], gw + P.dl_b[s], 0));
  }
  const float* tu = ws + w.query; const float* ti = ws + w.query + d.Du;
  const float* ru = ws + w.delf_rep[0]; const float* ri = ws + w.delf_rep[1];
  const float* act = ws + w.delf_act; const float* dact = ws + w.delf_dact;
  const int LA = SCORE_DELF_ACT;
  // fusion input k = [first | second]: 0 [tu|ti], 1 [ru|ri], 2 [tu|ri], 3 [ti|ru]
  const float* first[4] = {tu, ru, tu, ti}; const int ld1[4] = {d.Dq, d.Di, d.Dq, d.Dq}; const int n1[4] = {d.Du, d.Di, d.Du, d.Di};
  const float* second[4] = {ti, ri, ri, ru}; const int ld2[4] = {d.Dq, d.Du, d.Du, d.Di}; const int n2[4] = {d.Di, d.Du, d.Du, d.Di};
  for (int k = 0; k < 4; ++k) {
    float* gA = gw + P.dl_w[2 + 2 * k];
    G(gemm_queue_add(&q->gq, n1[k], 10, B, first[k], ld1[k], dact + 10 * k, LA, gA, 10));
    G(gemm_queue_add(&q->gq, n2[k], 10, B, second[k], ld2[k], dact + 10 * k, LA, gA + (int64_t)n1[k] * 10, 10));
    G(colsum_queue_add(&q->cq, dact + 10 * k, B, 10, LA, gw + P.dl_b[2 + 2 * k], 0));
    G(gemm_queue_add(&q->gq, 10, 4, B, act + 10 * k, LA, dact + 40 + 4 * k, LA, gw + P.dl_w[3 + 2 * k], 4));
    G(colsum_queue_add(&q->cq, dact + 40 + 4 * k, B, 4, LA, gw + P.dl_b[3 + 2 * k], 0));
  }
  G(gemm_queue_add(&q->gq, 4, 1, B, act + 56, LA, ws + w.dlogit, 1, gw + P.dl_w[10], 1));
  G(colsum_queue_add(&q->cq, ws + w.dlogit, B, 1, 1, gw + P.dl_b[10], 0));
  return 0;
}

// SVD++'s Fu + Fi scalars: each the batch sum of its column of the per-sample partials, into its own 4-float cell
static int queue_svdpp(const Pass& c, GradQueues* q, float* gw) {
  const int nv = c.d.Fu + c.d.Fi;
  for (int k = 0; k < nv; ++k)
    G(colsum_queue_add(&q->cq, c.ws + c.w.svdpp_dw + k, c.B, 1, nv, gw + c.P.sv_w + 4 * (int64_t)k, 0));
  return 0;
}

// SASRec's 14 variables: the head's kernels over the rows of its three applications (fc1: over the rows of z1, its folded
// gradient), the three projections over the B * T rows (Q from Qin, K and V from the raw X), gamma and beta from the per-sample
// partials
static int queue_sasrec(const Pass& c, GradQueues* q, float* gw, const SasrecArgs& a) {
  const Dims& d = c.d; const Params& P = c.P; const int B = c.B, BT = B * d.T, C = d.Di;
  const int R1 = sasrec_rows1(c), R = sasrec_rows(c, a);
  G(gemm_queue_add(&q->gq, FC2, 1, R, a.f2, FC2, a.dlogit, 1, gw + P.fc_w[2], 1));
  G(colsum_queue_add(&q->cq, a.dlogit, R, 1, 1, gw + P.fc_b[2], 0));
  G(gemm_queue_add(&q->gq, FC1, FC2, R, a.f1, FC1, a.dz2, FC2, gw + P.fc_w[1], FC2));
  G(colsum_queue_add(&q->cq, a.dz2, R, FC2, FC2, gw + P.fc_b[1], 0));
  G(gemm_queue_add(&q->gq, a.Dh, FC1, R1, a.hin, a.Dh, a.dz1, FC1, gw + P.fc_w[0], FC1));
  G(colsum_queue_add(&q->cq, a.dz1, R1, FC1, FC1, gw + P.fc_b[0], 0));
  const float* in[3] = {a.qin, a.X, a.X}; const int ldi[3] = {C, d.I, d.I};
  const float* dy[3] = {a.dq, a.dk, a.dv};
  for (int k = 0; k < 3; ++k) {
    G(gemm_queue_add(&q->gq, C, C, BT, in[k], ldi[k], dy[k], C, gw + P.sa_w[k], C));
    G(colsum_queue_add(&q->cq, dy[k], BT, C, C, gw + P.sa_b[k], 0));
  }
  G(colsum_queue_add(&q->cq, a.dgamma, B, C, C, gw + P.sa_gamma, 0));
  G(colsum_queue_add(&q->cq, a.dbeta, B, C, C, gw + P.sa_beta, 0));
  return 0;
}

}  // namespace

extern "C" int score_context_create(void** ctx) {
  if (!ctx) return SCORE_E_BADARG;
  SideStream* sd = new (std::nothrow) SideStream();
  if (!sd) return SCORE_E_BADARG;
  memset(sd, 0, sizeof(*sd));
  int rc = side_stream_create(sd);
  if (rc != 0) { delete sd; return rc; }
  *ctx = sd;
  return 0;
}

extern "C" int score_context_destroy(void* ctx) {
  if (ctx) {
    SideStream* sd = reinterpret_cast<SideStream*>(ctx);
    side_stream_release(sd);
    delete sd;
    return 0;
  }
  std::lock_guard<std::mutex> lock(g_default_mu);
  for (int i = 0; i < SCORE_MAX_DEVICES; ++i) side_stream_release(&g_default_ctx[i]);
  return 0;
}

extern "C" int score_id_status(int32_t* id_status, int32_t* bits, int32_t clear, void* stream) {
  if (!id_status) return SCORE_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  int32_t host = 0;
  HIPTRY(hipMemcpyAsync(&host, id_status, sizeof(host), hipMemcpyDeviceToHost, s));
  HIPTRY(hipStreamSynchronize(s));
  if (host && clear) {
    HIPTRY(hipMemsetAsync(id_status, 0, sizeof(host), s));
    HIPTRY(hipStreamSynchronize(s));
  }
  if (bits) *bits = host;
  return host ? SCORE_E_INDEX : 0;
}

extern "C" int score_param_layout(const score_config_t* cfg, score_param_entry_t* out, int32_t max_entries,
                                  int64_t* n_floats, int64_t* n_reg_floats) {
  Dims d;
  SCORE_TRY(make_dims(cfg, &d));
  Params P;
  int n = build_layout(d, out, max_entries, &P);
  if (n < 0) return n;
  if (n_floats) *n_floats = P.n_floats;
  if (n_reg_floats) *n_reg_floats = P.n_reg;
  return n;
}

extern "C" int score_workspace_layout(const score_config_t* cfg, int32_t B, score_workspace_t* out) {
  Dims d;
  SCORE_TRY(make_dims(cfg, &d));
  if (B <= 0 || !out) return SCORE_E_BADARG;
  WS w;
  build_ws(d, B, &w);
  out->total_bytes = w.total * 4;
  out->xside = w.xside[0]; out->atten_info = w.info; out->rsave = w.rsave[0]; out->query = w.query;
  out->head_inp = w.head_inp; out->att_score = w.att_score; out->logit = w.logit; out->y_pred = w.y_pred;
  out->loss = w.loss; out->gru_out = w.gru_out[0]; out->gru_final = w.gru_final[0];
  out->plan_meta = w.meta; out->plan_unique_rows = w.unique_rows; out->n_occurrences = w.n_occ;
  for (int g = 0; g < 6; ++g) out->plan_remap[g] = w.remap[g];
  return 0;
}

// float offset of an internal workspace region by name (tests / tools compare the forms of a pass region by region);
// per-side / per-call regions: the first one (the second follows at the same distance as in score_workspace_t's pairs)
extern "C" int score_workspace_field(const score_config_t* cfg, int32_t B, const char* name, int64_t* offset, int64_t* second) {
  Dims d;
  SCORE_TRY(make_dims(cfg, &d));
  if (B <= 0 || !name || !offset) return SCORE_E_BADARG;
  WS w;
  build_ws(d, B, &w);
  struct { const char* n; int64_t a, b; } tab[] = {
      {"xside", w.xside[0], w.xside[1]}, {"info", w.info, -1}, {"rsave", w.rsave[0], w.rsave[1]}, {"query", w.query, -1},
      {"head_inp", w.head_inp, -1}, {"att_score", w.att_score, -1}, {"logit", w.logit, -1}, {"y_pred", w.y_pred, -1},
      {"gru_out", w.gru_out[0], w.gru_out[1]}, {"gru_final", w.gru_final[0], w.gru_final[1]}, {"xproj", w.xproj[0], w.xproj[1]},
      {"gates", w.gates[0], w.gates[1]}, {"q", w.q, -1}, {"ainp", w.ainp, -1}, {"a1", w.a1, -1}, {"a2", w.a2, -1},
      {"bn", w.bn, -1}, {"f1", w.f1, -1}, {"f2", w.f2, -1}, {"lossb", w.lossb, -1}, {"dlogit", w.dlogit, -1},
      {"dz2", w.dz2, -1}, {"dz1", w.dz1, -1}, {"dbn", w.dbn, -1}, {"dhead", w.dhead, -1}, {"dgstage", w.dgstage, -1},
      {"ds", w.ds, -1}, {"da2", w.da2, -1}, {"da1", w.da1, -1}, {"adzsum", w.adzsum, -1}, {"dq", w.dq, -1},
      {"dquery", w.dquery, -1}, {"dgru", w.dgru[0], w.dgru[1]}, {"dinfo", w.dinfo, -1}, {"dxproj", w.dxproj[0], w.dxproj[1]},
      {"rh", w.rh[0], w.rh[1]}, {"hprev", w.hprev[0], w.hprev[1]}, {"dxside", w.dxside[0], w.dxside[1]},
      {"dzsum", w.dzsum[0], w.dzsum[1]}, {"pcoef", w.pcoef[0], w.pcoef[1]}, {"dzcoef", w.dzcoef[0], w.dzcoef[1]},
      {"dtgt", w.dtgt, -1}, {"S", w.S, -1}, {"ca_slab", w.ca_slab, -1}, {"psimg", w.psimg, -1},
      {"gcmc_a", w.gcmc_a[0], w.gcmc_a[1]}, {"gcmc_z", w.gcmc_z[0], w.gcmc_z[1]}, {"gcmc_dz", w.gcmc_dz[0], w.gcmc_dz[1]},
      {"gcmc_da", w.gcmc_da[0], w.gcmc_da[1]}, {"gcmc_pn", w.gcmc_pn, w.gcmc_pn + (int64_t)B * d.H}, {"gcmc_g", w.gcmc_g, -1},
      {"gcmc_gu", w.gcmc_gu, w.gcmc_gu + (int64_t)B * d.H}, {"caser_hwin", w.caser_hwin, -1}, {"caser_arg", w.caser_arg, -1},
      {"caser_v", w.caser_v, -1}, {"delf_key", w.delf_key[0], w.delf_key[1]}, {"delf_att", w.delf_att[0], w.delf_att[1]},
      {"delf_rep", w.delf_rep[0], w.delf_rep[1]}, {"delf_ds", w.delf_ds[0], w.delf_ds[1]},
      {"delf_dpre", w.delf_dpre[0], w.delf_dpre[1]}, {"delf_act", w.delf_act, -1}, {"delf_dact", w.delf_dact, -1},
      {"deems_f1", w.deems_f1 < 0 ? -1 : w.f1, w.deems_f1}, {"deems_f2", w.deems_f2 < 0 ? -1 : w.f2, w.deems_f2},
      {"deems_dz1", w.deems_dz1 < 0 ? -1 : w.dz1, w.deems_dz1}, {"deems_dz2", w.deems_dz2 < 0 ? -1 : w.dz2, w.deems_dz2},
      {"deems_logit", w.deems_logit, w.deems_logit + B}, {"deems_y", w.deems_y, w.deems_y + B},
      {"deems_dlogit", w.deems_dlogit, w.deems_dlogit + B}, {"svdpp_act", w.svdpp_act, -1}, {"svdpp_dw", w.svdpp_dw, -1},
      {"sasrec_y", w.sas_y, -1}, {"sasrec_final", w.sas_fin, -1}, {"sasrec_att", w.sas_att, -1}, {"sasrec_p", w.sas_p, -1},
      {"sasrec_qin", w.sas_qin, -1}, {"sasrec_hin", w.sas_hin, -1}, {"sasrec_logit", w.sas_logit, -1}};
  for (auto& e : tab)
    if (strcmp(e.n, name) == 0) {
      if (e.a < 0) return SCORE_E_BADARG;       // (a region of another model type)
      *offset = e.a;
      if (second) *second = e.b;
      return 0;
    }
  return SCORE_E_BADARG;
}

extern "C" int score_index_plan(const score_config_t* cfg, const score_state_t* st, const score_batch_t* bt,
                                int32_t n_shards, int32_t dedup, void* stream) {
  Dims d;
  SCORE_TRY(make_dims(cfg, &d));
  if (!st || !bt || !st->workspace || bt->B <= 0 || n_shards < 1 || n_shards > 64 || (dedup != 0 && dedup != 1)) return SCORE_E_BADARG;
  const int TA = active_T(d, bt);
  const int B = bt->B, BT = B * TA;
  WS w;
  build_ws(d, B, &w);
  if (w.total * 4 > st->workspace_bytes) return SCORE_E_WORKSPACE;
  if (BT > (1 << 21) || d.Fu > 8 || d.Fi > 8) return SCORE_E_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  float* ws = st->workspace;
  const Flags fl = flags_of(st);
  PlanFillArgs pf;
  memset(&pf, 0, sizeof(pf));
  const int32_t* idx[6] = {bt->user_1hop, bt->item_2hop, bt->user_2hop, bt->item_1hop, bt->target_user,
                           bt->target_item};
  const int Fs[6] = {d.Fi, d.Fi, d.Fu, d.Fu, d.Fu, d.Fi};
  int64_t off = 0;
  for (int g = 0; g < 6; ++g) {
    if (!idx[g]) return SCORE_E_BADARG;
    pf.idx[g] = idx[g]; pf.F[g] = Fs[g]; pf.off[g] = off;
    off += (g < 4 ? (int64_t)BT * d.K : (int64_t)B) * Fs[g];
  }
  pf.off[6] = off; pf.K = d.K; pf.G = n_shards; pf.T = d.T; pf.TA = TA;
  pf.n_rows = clamp_rows(d.N); pf.id_status = st->id_status;
  // key = row (1 shard) or (owner = row % G) << shift | (row / G)
  const int64_t rows_local = cdiv64(d.N, n_shards);
  int shift = 1;
  while (shift < 31 && ((int64_t)1 << shift) < rows_local) ++shift;
  int obits = 0;
  while ((1 << obits) < n_shards) ++obits;
  if (shift + obits > 32) return SCORE_E_SHAPE;
  pf.shift = n_shards > 1 ? shift : 0;
  const int key_bits = n_shards > 1 ? shift + obits : shift;
  uint32_t* keys_in = reinterpret_cast<uint32_t*>(ws + w.keys_in);
  uint32_t* vals_in = reinterpret_cast<uint32_t*>(ws + w.vals_in);
  uint32_t* keys_out = reinterpret_cast<uint32_t*>(ws + w.keys_out);
  uint32_t* vals_out = reinterpret_cast<uint32_t*>(ws + w.vals_out);
  G(score_launch_plan(pf, key_bits, keys_in, vals_in, keys_out, vals_out, ws + w.sort_temp,
                      (size_t)w.sort_temp_bytes, s, fl.sort_lib ? 1 : fl.sort_own ? 2 : 0));
  if (n_shards > 1 || dedup) {
    PlanRemapArgs ra;
    memset(&ra, 0, sizeof(ra));
    for (int g = 0; g < 6; ++g) { ra.out[g] = reinterpret_cast<int32_t*>(ws + w.remap[g]); ra.F[g] = Fs[g]; }
    ra.K = d.K; ra.T = d.T; ra.TA = TA;
    // keys_in / vals_in are dead after the sort: reuse them for the head flags and the unique keys
    G(score_launch_plan_unique(ra, keys_out, vals_out, off + 1, keys_in, reinterpret_cast<uint32_t*>(ws + w.uid),
                               vals_in, reinterpret_cast<int32_t*>(ws + w.unique_rows),
                               reinterpret_cast<int32_t*>(ws + w.meta), n_shards, shift, ws + w.sort_temp,
                               (size_t)w.sort_temp_bytes, s));
  }
  return 0;
}

// do the two sides' GRU input projections (which = 0) / their input gradients (which = 1) take the panel form?  Same
// answer in the forward pass (which writes the weight images) and in the backward pass (which uses them).
// The input gradients: from 64 K rows per side (cfg-5), or with Flags.panel_dx.  The kernel itself is 30 % faster there
// too (71 vs 101 us at cfg-3), but a panel workgroup owns its CU (8 waves x 256 registers), and the backward pass has
// ~350 us of other streams' work to place -- the side stream's query branch and early weight gradients, the optimizer's
// window slice -- which the tiled kernel lets run beside it and a one-round panel kernel pushes into the co-attention
// backward and the scatter (cfg-3: 0.254 -> 0.329 ms), or, with the recurrences' weight gradients moved in front of those
// (round 3's SCORE_WGRAD_EARLY), into them (1.287 -> 1.285 ms/step; projections only: 1.273; round 4: with the head's and the
// attention's products folded into the end-of-pass launch, or the side stream joined before the co-attention backward, the
// same: profiles/r04_probes.md).  At cfg-5's sizes the other
// streams' work is small beside these products: 20.3 -> 19.8 ms/step with both.
static bool panel_gemms(const Dims& d, const score_state_t* st, int BT, int which) {
  const Flags fl = flags_of(st);
  const bool two_sided = d.family == FAM_SLICE || d.family == FAM_GCMC;      // (the families of fwd_grus_two_sided)
  if (st->gemm_mode != 1 || fl.no_panel || d.Is[0] != d.Is[1] || !two_sided) return false;
  if (which == 1 && d.family == FAM_GCMC) return false;      // (GCMC's input gradients take Z's relu mask in the epilogue: the tiled kernels)
  const int ns = panel_x_splits(d.H), nd = panel_d_splits(d.Is[0]);
  return which == 0 ? ns > 0 && score_gemm_panel_ok(2 * ns, BT, 3 * d.H / ns, d.Is[0], x_ld(d, 0), 3 * d.H, nullptr)
                    : (fl.panel_dx || (int64_t)BT >= 65536) && nd > 0 &&
                          score_gemm_panel_ok(2 * nd, BT, d.Is[0] / nd, 3 * d.H, 3 * d.H, d.I, nullptr);
}

extern "C" int score_gemm_forms(const score_config_t* cfg, const score_state_t* st, int32_t B, int32_t active_slices,
                                int32_t* x_form, int32_t* dx_form) {
  Dims d;
  SCORE_TRY(make_dims(cfg, &d));
  if (!st || B <= 0 || active_slices < 0) return SCORE_E_BADARG;
  const int T = (active_slices > 0 && active_slices < d.T) ? active_slices : d.T;
  const int64_t BT = (int64_t)B * T;
  if (BT > (1ll << 30)) return SCORE_E_SHAPE;
  if (x_form) *x_form = panel_gemms(d, st, (int)BT, 0) ? panel_x_splits(d.H) : 0;
  if (dx_form) *dx_form = panel_gemms(d, st, (int)BT, 1) ? panel_d_splits(d.Is[0]) : 0;
  return 0;
}

// ---------------------------------------------------------------- per-sample whole-model path (persample.h)
// The reference's own shapes (train_score.py:15-16, 285-372: D = 16, H = 32, B = 100 / 200) are bound by launch latency,
// not by bytes or flops: score_forward / score_backward then run ONE kernel each (a workgroup per sample) plus the
// weight-gradient products and the row scatter.  Flags.no_ps: never; ps_fwd_only: the forward pass only; ps_bwd_only: the
// backward pass only (A/B and parity tests compare the forms).
namespace {
struct PsPlan { PsShape s; PsImages im; };

bool ps_path(const Dims& d, const score_state_t* st, const score_batch_t* bt, int TA, PsPlan* pp) {
  if (flags_of(st).no_ps || st->scatter_mode == 1) return false;
  if (!d.coattn || !d.attn) return false;                     // SCORE, SCORE_USER, SCORE_ITEM
  if (ps_plan_shape(bt->B, TA, d.T, d.K, d.D, d.Fu, d.Fi, d.H, d.NI, d.Dk, d.Dhead, d.off_u, d.off_i, d.off_ti, d.off_tu,
                    global_batch(st, bt->B), &pp->s) != 0)
    return false;
  ps_plan_images(pp->s, &pp->im);
  return true;
}

// the step's weight images and the L2 partial sums: one launch
int ps_prep(const Pass& c, const PsPlan& pp) {
  const Dims& d = c.d; const Params& P = c.P; const float* W = c.W;
  float* img = c.ws + c.w.psimg;
  const int H = d.H, I = d.I, Dk = d.Dk, Dh = d.Dhead;
  PsPrepArgs pa;
  memset(&pa, 0, sizeof(pa));
  int n = 0;
  auto job = [&](const float* Wp, const float* W2, int64_t off, int K, int N, int ld, int kind, int trans, int aux) {
    PsImgJob& j = pa.job[n++];
    j.W = Wp; j.W2 = W2; j.img = img + off; j.K = K; j.N = N; j.ld = ld; j.kind = kind; j.trans = trans; j.aux = aux;
  };
  for (int sd = 0; sd < 2; ++sd) job(W + P.gk[sd], W + P.ck[sd], pp.im.wx[sd], I, 3 * H, 0, PS_SRC_WXCAT, 0, H);
  job(W + P.at_w[0], nullptr, pp.im.q2, I, Dk, Dk, PS_SRC_PLAIN, 0, 0);
  job(W + P.at_w[1], nullptr, pp.im.wq, Dk, AT1, AT1, PS_SRC_WQ, 0, Dk);
  job(W + P.at_w[1], nullptr, pp.im.weff, 2 * Dk, AT1, AT1, PS_SRC_WEFF, 0, Dk);
  job(W + P.at_w[2], nullptr, pp.im.w4, AT1, AT2, AT2, PS_SRC_PLAIN, 0, 0);
  job(W + P.fc_w[0], nullptr, pp.im.fc1, Dh, FC1, FC1, PS_SRC_PLAIN, 0, 0);
  job(W + P.fc_w[1], nullptr, pp.im.fc2, FC1, FC2, FC2, PS_SRC_PLAIN, 0, 0);
  job(W + P.fc_w[1], nullptr, pp.im.fc2t, FC2, FC1, FC2, PS_SRC_PLAIN, 1, 0);
  job(W + P.fc_w[0], nullptr, pp.im.fc1t, FC1, Dh, FC1, PS_SRC_PLAIN, 1, 0);
  job(W + P.at_w[2], nullptr, pp.im.w4t, AT2, AT1, AT2, PS_SRC_PLAIN, 1, 0);
  job(W + P.at_w[1], nullptr, pp.im.wefft, AT1, 2 * Dk, AT1, PS_SRC_WEFF, 1, Dk);
  job(W + P.at_w[1], nullptr, pp.im.wqt, AT1, Dk, AT1, PS_SRC_WQ, 1, Dk);
  job(W + P.at_w[0], nullptr, pp.im.q2t, Dk, I, Dk, PS_SRC_PLAIN, 1, 0);
  for (int sd = 0; sd < 2; ++sd) job(W + P.gk[sd], W + P.ck[sd], pp.im.wxt[sd], 3 * H, I, 0, PS_SRC_WXCAT, 1, H);
  pa.njobs = n;
  pa.wreg = W; pa.n_reg = P.n_reg; pa.part = c.ws + c.w.part;
  return score_launch_ps_prep(pa, c.s);
}

int forward_ps(const Pass& c, const PsPlan& pp, float reg_lambda, float keep_prob, const uint8_t* mask0, const uint8_t* mask1,
               uint64_t seed, void* const* stage_events) {
  const Params& P = c.P; const WS& w = c.w; const score_state_t* st = c.st; const score_batch_t* bt = c.bt;
  float* ws = c.ws; hipStream_t s = c.s;
  G(ps_prep(c, pp));
  // (the layer-by-layer backward pass that follows reads the concatenated / folded copies)
  if (c.fl.ps_fwd_only) G(weight_prep(c, s));
  EV(0);
  PsFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.s = pp.s; a.im = pp.im; a.img = ws + w.psimg;
  a.idx1[0] = bt->user_1hop; a.idx2[0] = bt->item_2hop; a.idx1[1] = bt->user_2hop; a.idx2[1] = bt->item_1hop;
  a.tu = bt->target_user; a.ti = bt->target_item; a.label = bt->label; a.length = bt->length;
  a.table = st->table; a.n_rows = c.n_rows; a.id_status = st->id_status; a.W = st->w;
  for (int i = 0; i < 2; ++i) {
    a.ca_w[i] = P.ca_w[i]; a.ca_b[i] = P.ca_b[i]; a.gk[i] = P.gk[i]; a.gb[i] = P.gb[i]; a.ck[i] = P.ck[i]; a.cb[i] = P.cb[i];
    a.xside[i] = ws + w.xside[i]; a.rsave[i] = ws + w.rsave[i]; a.gates[i] = ws + w.gates[i]; a.gru_out[i] = ws + w.gru_out[i];
    a.gru_final[i] = ws + w.gru_final[i];
  }
  for (int i = 0; i < 4; ++i) a.at_b[i] = P.at_b[i];
  a.at_w5 = P.at_w[3]; a.bn_g = P.bn_g; a.bn_b = P.bn_b;
  for (int i = 0; i < 3; ++i) a.fc_b[i] = P.fc_b[i];
  a.fc_w3 = P.fc_w[2];
  a.query = ws + w.query; a.head_inp = ws + w.head_inp; a.info = ws + w.info; a.q = ws + w.q; a.ainp = ws + w.ainp;
  a.a1 = ws + w.a1; a.a2 = ws + w.a2; a.att_score = ws + w.att_score; a.bn = ws + w.bn; a.f1 = ws + w.f1; a.f2 = ws + w.f2;
  a.logit = ws + w.logit; a.y = ws + w.y_pred; a.lossb = ws + w.lossb; a.dlogit = ws + w.dlogit; a.dz2 = ws + w.dz2;
  a.keep = keep_prob; a.rs = c.rs; a.drop = keep_prob < 1.f ? 1 : 0;
  a.mask0 = mask0; a.mask1 = mask1; a.seed0 = seed; a.seed1 = seed ^ 0x5DEECE66Dull;
  a.seed_dev = st->step_scalars ? &st->step_scalars->drop_seed : nullptr;
  a.loss = ws + w.loss; a.loss_host = st->loss_host; a.part = ws + w.part;
  a.done = reinterpret_cast<unsigned int*>(ws + w.part) + 256;
  a.lambda = reg_lambda; a.inv_bglobal = 1.0f / (float)c.Bg;
  G(score_launch_ps_fwd(a, s));
  if (st->gather_done_event) HIPTRY(hipEventRecord((hipEvent_t)st->gather_done_event, s));
  EV(1); EV(2); EV(3);
  // (the loss: reduced by the kernel's last workgroup -- until round 5 a one-workgroup launch on the side stream)
  if (st->loss_done_event) HIPTRY(hipEventRecord((hipEvent_t)st->loss_done_event, s));
  EV(4);
  return 0;
}

int backward_ps(const Pass& c, const PsPlan& pp, float keep_prob, float* gw, float* grad_table, void* const* stage_events) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w; const score_state_t* st = c.st; const score_batch_t* bt = c.bt;
  float* ws = c.ws; const int B = c.B; hipStream_t s = c.s;
  SideStream* side = nullptr;
  G(side_stream(st, s, &side));
  side->fwd_on = nullptr;
  // With score_state_t.grads_done_event everything that FINISHES grad_w -- the weight-gradient products, the column sums, the
  // slab reduce -- runs on the context's side stream behind the backward kernel, beside the row scatter on `stream`: at these
  // shapes every dependent launch costs the chain ~5 us whatever it computes, so the chain holds the scatter only
  const bool fin_side = st->grads_done_event != nullptr;
  hipStream_t fs = fin_side ? side->st : s;
  // (no memset of grad_w: every float of it is overwritten by this pass -- each variable of SCORE / SCORE_USER / SCORE_ITEM gets a
  //  gradient, every product and column sum stores rather than accumulates -- except the alignment padding between the tensors,
  //  which the backward kernel's first workgroup clears)
  if (c.fl.ps_bwd_only) G(ps_prep(c, pp));      // (after a layer-by-layer forward pass: no images yet)
  EV(0);
  PsBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.s = pp.s; a.im = pp.im; a.img = ws + w.psimg;
  a.idx1[0] = bt->user_1hop; a.idx2[0] = bt->item_2hop; a.idx1[1] = bt->user_2hop; a.idx2[1] = bt->item_1hop;
  a.length = bt->length; a.table = st->table; a.n_rows = c.n_rows; a.W = c.W;
  for (int i = 0; i < 2; ++i) {
    a.ca_w[i] = P.ca_w[i]; a.gk[i] = P.gk[i]; a.ck[i] = P.ck[i];
    a.rsave[i] = ws + w.rsave[i]; a.gates[i] = ws + w.gates[i]; a.gru_out[i] = ws + w.gru_out[i];
    a.dxproj[i] = ws + w.dxproj[i]; a.rh[i] = ws + w.rh[i]; a.hprev[i] = ws + w.hprev[i]; a.dxside[i] = ws + w.dxside[i];
    a.pcoef[i] = ws + w.pcoef[i]; a.dzcoef[i] = ws + w.dzcoef[i];
  }
  a.at_w5 = P.at_w[3]; a.bn_g = P.bn_g;
  a.query = ws + w.query; a.head_inp = ws + w.head_inp; a.info = ws + w.info; a.q = ws + w.q; a.ainp = ws + w.ainp;
  a.a1 = ws + w.a1; a.a2 = ws + w.a2; a.att_score = ws + w.att_score; a.f1 = ws + w.f1; a.dz2 = ws + w.dz2;
  a.dz1 = ws + w.dz1; a.dbn = ws + w.dbn; a.dgstage = ws + w.dgstage; a.ds = ws + w.ds; a.da2 = ws + w.da2; a.da1 = ws + w.da1;
  a.adzsum = ws + w.adzsum; a.dq = ws + w.dq; a.dtgt = ws + w.dtgt; a.S = ws + w.S;
  a.caslab[0] = ws + w.ca_slab; a.caslab[1] = ws + w.ca_slab + (int64_t)B * 2 * d.Di;
  a.keep = keep_prob; a.rs = c.rs;
  {
    score_param_entry_t ent[MAX_ENTRIES];
    Params Pl;
    const int ne = build_layout(d, ent, MAX_ENTRIES, &Pl);
    if (ne < 0) return ne;
    a.gw = gw; a.npad = 0;
    for (int i = 0; i < ne; ++i) {
      const int64_t end = ent[i].offset + (int64_t)ent[i].rows * (ent[i].cols ? ent[i].cols : 1);
      const int64_t stop = align_up64(end, 4);
      if (stop > end) {
        if (a.npad >= PS_MAX_PADS) return SCORE_E_SHAPE;
        a.pad_off[a.npad] = (int)end; a.pad_len[a.npad] = (int)(stop - end); ++a.npad;
      }
    }
  }
  if ((int64_t)B * 2 * (d.Di + d.Du) > w.ca_slab_floats) return SCORE_E_WORKSPACE;
  G(score_launch_ps_bwd(a, s));
  if (fin_side) {
    HIPTRY(hipEventRecord(side->wx, s));
    HIPTRY(hipStreamWaitEvent(fs, side->wx, 0));
  }
  EV(1); EV(2); EV(3);

  // every weight gradient X^T dY and column sum of the pass, from what the kernel left in the workspace (bn1's sums as behind
  // a fused head; the recurrences' bias gradients from the full dxproj rows: the kernel writes no bias slab)
  GradQueues q;
  queues_init(&q);
  ColsumJobs& cq = q.cq;
  G(queue_head(c, &q, gw, true));
  G(queue_attn(c, &q, gw));
  G(queue_query(c, &q, gw));
  for (int sd = 0; sd < 2; ++sd) G(queue_gru_side(c, &q, gw, sd, 0));
  // the co-attention denses: [w_t | w_1 | w_2] -- w_t from the target rows weighted by S, w_1 | w_2 from the per-sample slabs
  G(colsum_queue_add(&cq, a.caslab[0], B, 2 * d.Di, 2 * d.Di, gw + P.ca_w[0] + d.Di, 0));
  G(colsum_queue_add(&cq, a.caslab[1], B, 2 * d.Du, 2 * d.Du, gw + P.ca_w[1] + d.Du, 0));
  G(colsum_queue_add(&cq, ws + w.query + d.Du, B, d.Di, d.Dq, gw + P.ca_w[0], 0, ws + w.S));
  G(colsum_queue_add(&cq, ws + w.query, B, d.Du, d.Dq, gw + P.ca_w[1], 0, ws + w.S + B));
  G(colsum_queue_add(&cq, ws + w.S, B, 1, 1, gw + P.ca_b[0], 0));
  G(colsum_queue_add(&cq, ws + w.S + B, B, 1, 1, gw + P.ca_b[1], 0));

  // ---- the weight-gradient products in one grouped flush, then the finishers (side stream with grads_done_event)
  {
    // (round 5: TWO launches -- products + column sums' first stage, then slab reduce + second stage + the folded attention
    //  layer's gradient -- where there were four in a row: they stand between the backward kernel and the dense ApplyAdam)
    ReduceGroup rg;
    int cs_done = 0;
    // (all products on the f32 kernel here: at the CCMR shape -- 7,600 (b, t) rows -- the bf16x3 family would take four of them as a
    //  launch of its own IN FRONT of this one, on the chain to the dense ApplyAdam: 0.3582 vs 0.3566 ms, two alternating pairs)
    G(gemm_queue_flush(&q.gq, 0, ws + w.dwslab, w.dwslab_floats, fs, &rg, &cq, ws + w.cs_part, w.cs_part_floats, &cs_done));
    W1Fold wf;
    memset(&wf, 0, sizeof(wf));
    wf.Dk = d.Dk; wf.NA = AT1; wf.dweff = ws + w.dweff; wf.dwq = ws + w.dwq; wf.gW1 = gw + P.at_w[1];
    G(score_launch_finish(&rg, &cq, ws + w.cs_part, w.cs_part_floats, fs, cs_done, &wf));
    if (fin_side) HIPTRY(hipEventRecord((hipEvent_t)st->grads_done_event, fs));
  }
  // ---- embedding rows.  The plan: in score_state_t.plan_workspace whenever the caller names one.  No scatter-mode test here:
  // this pass never runs under scatter_mode 1 (ps_path), the header defines the field for mode 0 only, and the project's own
  // callers set it there only (score_amd/model.py; step.hip passes none).  The test of the layer-by-layer pass would matter
  // for a sharded (mode 2) caller that sorts into a second buffer: the unique positions would then have to come from that
  // buffer too (row_scatter reads them from the pass's own workspace).
  if (st->plan_done_event) HIPTRY(hipStreamWaitEvent(s, (hipEvent_t)st->plan_done_event, 0));
  G(row_scatter(c, st->plan_workspace ? st->plan_workspace : ws, grad_table));
  EV(4);
  EV(5);
  // (the forward pass put its loss reduction on the side stream: loss[] is final on `stream` behind this pass -- it ran beside
  //  the backward kernel, the wait costs nothing)
  if (st->loss_done_event) HIPTRY(hipStreamWaitEvent(s, (hipEvent_t)st->loss_done_event, 0));
  return 0;
}
}  // namespace

extern "C" int score_persample_form(const score_config_t* cfg, const score_state_t* st, int32_t B, int32_t active_slices) {
  Dims d;
  SCORE_TRY(make_dims(cfg, &d));
  if (!st || B <= 0 || active_slices < 0) return SCORE_E_BADARG;
  score_batch_t bt;
  memset(&bt, 0, sizeof(bt));
  bt.B = B; bt.active_slices = active_slices;
  PsPlan pp;
  return ps_path(d, st, &bt, active_T(d, &bt), &pp) ? 1 : 0;
}

// ---------------------------------------------------------------- the layer-by-layer forward pass
// fwd_open, the same for every model type, then ONE function per family (fwd_slice .. fwd_delf): the family's launches
// between EV(1) and EV(4), in order, with its waits for the side stream's `wx` and `join` where it needs them.
namespace {
// score_forward's arguments behind the batch, and what fwd_open leaves for the stages after it
struct FwdState {
  float reg_lambda, keep_prob; const uint8_t *mask0, *mask1; uint64_t seed; void* const* stage_events;
  SideStream* sd;      // the side stream, forked behind the launch stream, `wx` and `join` recorded on it
  bool panel_x;        // the projections take the panel form (panel_gemms)
};

// Side stream: the target rows, the L2 norm of the weights (needs no batch), then the attention's query branch (target rows and
// weights only) -- beside the gather and the GRUs.  Launch stream: the gather.  Ends with EV(1).
int fwd_open(const Pass& c, FwdState* f) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w; const score_state_t* st = c.st; const score_batch_t* bt = c.bt;
  float* ws = c.ws; const float* W = c.W; const int B = c.B, x3 = c.x3; hipStream_t s = c.s;
  void* const* stage_events = f->stage_events;
  SideStream* sd = nullptr;
  G(side_stream(st, s, &sd));
  f->sd = sd;
  G(fork_side(sd, s));
  sd->fwd_on = s;       // (score_backward on this stream next finds the side stream already behind everything before this pass)
  // target rows -> query [tu | ti] and head_inp [.., ti, tu]      (score.py:62-66, 210, 217).  On the side stream since round 6:
  // its readers on `stream` -- the attention, the head -- are behind the side stream's join anyway, and the fused gather, which
  // was the third, reads the target rows from the table itself (CoattnCall.tidx): the step's chain starts with the gather
  // (four interleaved pairs at cfg-3: 886.5 k vs 881.3 k samples/s)
  G(score_launch_target_fwd(st->table, d.D, d.Fu, d.Fi, B, bt->target_user, bt->target_item, ws + w.query, d.Dq,
                            ws + w.head_inp, d.Dhead, d.off_ti, d.off_tu, sd->st, st->n_table_rows, st->id_status));
  G(weight_prep(c, sd->st));       // (off the main stream)
  // the panel form of the projections and of their input gradients (gemm_panel.hip) takes the weights as fragment images:
  // written here, once per step, behind the concatenated copies (the backward pass reuses them as it reuses the copies)
  f->panel_x = panel_gemms(d, st, c.BT, 0);
  if (f->panel_x) G(panel_prep(c, 0, sd->st));
  if (panel_gemms(d, st, c.BT, 1)) G(panel_prep(c, 1, sd->st));
  HIPTRY(hipEventRecord(sd->wx, sd->st));
  if (d.attn) {
    float* scratch2 = ws + w.scratch2;
    G(gemm_mode_call(x3, 0, B, d.Dk, d.Dq, ws + w.query, d.Dq, W + P.at_w[0], d.Dk, ws + w.q, d.Dk, W + P.at_b[0], GF_BIAS,
                     1.f, nullptr, 0, scratch2, w.scratch_floats, sd->st));
    // dense_3 on [q, k, q-k, q*k], folded (head.hip; Weff / Wq come from the weight-prep launch above):
    // a1 = relu([k, q*k] . Weff + (q . Wq + b)[sample])
    G(gemm_mode_call(x3, 0, B, AT1, d.Dk, ws + w.q, d.Dk, ws + w.wq, AT1, ws + w.qz, AT1, W + P.at_b[1], GF_BIAS, 1.f,
                     nullptr, 0, scratch2, w.scratch_floats, sd->st));
  }
  HIPTRY(hipEventRecord(sd->join, sd->st));
  EV(0);
  {
    CoattnArgs ca;
    CoattnCols k;
    coattn_args(c, &ca, &k);
    ca.id_status = st->id_status;
    ca.c[0].bit1 = 0; ca.c[0].bit2 = 3; ca.c[1].bit1 = 1; ca.c[1].bit2 = 2;      // positions in the feed tuple (graph_loader.py:383)
    const int32_t* tidx[2] = {bt->target_item, bt->target_user};
    for (int i = 0; i < 2; ++i) {
      CoattnCall& cc = ca.c[i];
      cc.tgt = ws + w.query + (i ? 0 : d.Du); cc.ldt = d.Dq; cc.tidx = tidx[i];
      cc.bias = d.coattn ? W + P.ca_b[i] : nullptr;
      cc.out1 = ws + w.xside[0] + k.col1[i]; cc.out2 = ws + w.xside[1] + k.col2[i]; cc.info = ws + w.info + k.info_col[i];
    }
    ca.fwd_one_unit = c.fl.coattn_fwd_one_unit ? 1 : 0;      // (debug_flags bit 17: one unit per wave, A/B)
    ca.CH = coattn_fwd_ch_of(st);                            // (bits 20 .. 23: a chunk length to measure; 0 = the rule)
    G(score_coattn_fwd_multi(ca, 2, d.D, B, s));
  }
  if (st->gather_done_event) HIPTRY(hipEventRecord((hipEvent_t)st->gather_done_event, s));
  EV(1);
  return 0;
}

// GRUs (:205-208) of the slice models and GCMC: hoisted x-projection of the rows xin[side], then the persistent recurrence
int fwd_grus_two_sided(const Pass& c, const FwdState& f, const float* const* xin) {
  const Dims& d = c.d; const WS& w = c.w; float* ws = c.ws; const int H = c.H, BT = c.BT, x3 = c.x3; hipStream_t s = c.s;
  GruArgs ga;
  gru_header(c, &ga);
  float* xp[2] = {ws + w.xproj[0], ws + w.xproj[1]};
  if (d.Is[0] == d.Is[1]) {    // both sides' projections in ONE grouped launch (each with its own bias row)
    if (f.panel_x) {
      G(panel_launch(c, 0, xin, xp));
    } else {
      const float* Bx[2] = {wxcat(c, 0), wxcat(c, 1)};
      const float* bx[2] = {Bx[0] + (int64_t)d.Is[0] * 3 * H, Bx[1] + (int64_t)d.Is[1] * 3 * H};
      G(score_gemm_same_shape(0, 2, BT, 3 * H, d.Is[0], xin, x_ld(d, 0), Bx, 3 * H, xp, 3 * H, GF_BIAS, x3 != 0, c.scratch,
                              w.scratch_floats, s, bx));
    }
  }
  for (int sd = 0; sd < 2; ++sd) {
    // x . [Wx_gates | Wx_cand] + [b_gates | b_cand]: one GEMM per side on the concatenated copy
    const float* cat = wxcat(c, sd);
    if (d.Is[0] != d.Is[1])
      G(gemm_mode_call(x3, 0, BT, 3 * H, d.Is[sd], xin[sd], x_ld(d, sd), cat, 3 * H, xp[sd], 3 * H, cat + (int64_t)d.Is[sd] * 3 * H,
                       GF_BIAS, 1.f, nullptr, 0, c.scratch, w.scratch_floats, s));
    gru_side(c, sd, &ga.s[sd]);
    ga.s[sd].xproj = xp[sd]; ga.s[sd].final_state = ws + w.gru_final[sd];
  }
  return score_gru_fwd_multi(ga, 2, s);
}

// temporal attention (:169-186, 210-215); q, Weff/Wq and qz come from the side stream
int fwd_attention(const Pass& c, const FwdState& f) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w; const score_batch_t* bt = c.bt;
  float* ws = c.ws; const float* W = c.W; const int B = c.B, T = c.T, H = c.H, BT = c.BT, x3 = c.x3; hipStream_t s = c.s;
  HIPTRY(hipStreamWaitEvent(s, f.sd->join, 0));
  // all of it in one launch (head_fused.hip) where the shape allows ...
  int frc = c.fl.attn_unfused ? SCORE_E_SHAPE
                : score_launch_attn_fwd_fused(B, T, H, d.NI, AT1, AT2, ws + w.q, ws + w.gru_out[0], ws + w.gru_out[1],
                                              ws + w.info, ws + w.weff, ws + w.qz, W + P.at_w[2], W + P.at_b[2],
                                              W + P.at_w[3], W + P.at_b[3], bt->length, ws + w.ainp, ws + w.a1, ws + w.a2,
                                              ws + w.att_score, ws + w.head_inp, d.Dhead, d.off_u, d.off_i, s,
                                              SCORE_WEFF_COPIES, c.weff_stride);
  if (frc != SCORE_E_SHAPE) return frc;
  // (... else the separate launches)
  G(score_launch_attn_build_inp(B, T, H, d.NI, ws + w.q, ws + w.gru_out[0], ws + w.gru_out[1], ws + w.info,
                                ws + w.ainp, s));
  G(gemm_mode_call(x3, 0, BT, AT1, 2 * d.Dk, ws + w.ainp, 2 * d.Dk, ws + w.weff, AT1, ws + w.a1, AT1, ws + w.qz,
                   GF_BIAS | GF_RELU | (T << 16), 1.f, nullptr, 0, c.scratch, w.scratch_floats, s));
  // dense_4, dense_5, mask, softmax over T and the pooling: one launch, a block per sample (head.hip)
  int trc = c.fl.attn_unfused ? SCORE_E_SHAPE
                : score_launch_attn_tail_fwd(B, T, H, AT1, AT2, ws + w.a1, W + P.at_w[2], W + P.at_b[2], W + P.at_w[3],
                                             W + P.at_b[3], bt->length, ws + w.gru_out[0], ws + w.gru_out[1], ws + w.a2,
                                             ws + w.att_score, ws + w.head_inp, d.Dhead, d.off_u, d.off_i, s);
  if (trc != SCORE_E_SHAPE) return trc;
  G(gemm_mode_call(x3, 0, BT, AT2, AT1, ws + w.a1, AT1, W + P.at_w[2], AT2, ws + w.a2, AT2, W + P.at_b[2],
                   GF_BIAS | GF_RELU, 1.f, nullptr, 0, c.scratch, w.scratch_floats, s));
  return score_launch_attn_pool_fwd(B, T, H, AT2, ws + w.a2, W + P.at_w[3], W + P.at_b[3], bt->length,
                                    ws + w.gru_out[0], ws + w.gru_out[1], ws + w.att_score, ws + w.head_inp, d.Dhead,
                                    d.off_u, d.off_i, s);
}

// build_fc_net (:68-76) on head_inp, the loss and its reduction
int fwd_fc_head(const Pass& c, const FwdState& f) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w; const score_state_t* st = c.st; const score_batch_t* bt = c.bt;
  float* ws = c.ws; const float* W = c.W; const int B = c.B, x3 = c.x3; hipStream_t s = c.s;
  const float keep_prob = f.keep_prob;
  const int dflag = keep_prob < 1.f ? GF_DROP : 0;
  // the whole head in one launch (head_fused.hip); shapes it does not cover take the layer-by-layer path
  int hrc = c.fl.head_unfused ? SCORE_E_SHAPE
                : score_launch_head_fwd_fused(B, d.Dhead, FC1, FC2, ws + w.head_inp, W + P.bn_g, W + P.bn_b, c.rs, W + P.fc_w[0],
                                              W + P.fc_b[0], W + P.fc_w[1], W + P.fc_b[1], W + P.fc_w[2], W + P.fc_b[2],
                                              keep_prob, f.mask0, f.mask1, f.seed, f.seed ^ 0x5DEECE66Dull,
                                              bt->label, ws + w.bn, ws + w.f1, ws + w.f2, ws + w.logit, ws + w.y_pred,
                                              ws + w.lossb, ws + w.dlogit, c.Bg, s,
                                              st->step_scalars ? &st->step_scalars->drop_seed : nullptr, ws + w.dz2,
                                              c.fl.head_fused_any_b ? 1 : 0);
  if (hrc == 0) return loss_tail(c, f.sd, f.reg_lambda);       // (dz2 came with the head)
  if (hrc != SCORE_E_SHAPE) return hrc;
  if (st->step_scalars && keep_prob < 1.f) return SCORE_E_SHAPE;   // the layer-by-layer path takes its seed by value
  G(score_launch_bn_fwd(B, d.Dhead, ws + w.head_inp, W + P.bn_g, W + P.bn_b, c.rs, ws + w.bn, s));
  G(gemm_mode_call(x3, 0, B, FC1, d.Dhead, ws + w.bn, d.Dhead, W + P.fc_w[0], FC1, ws + w.f1, FC1, W + P.fc_b[0],
                   GF_BIAS | GF_RELU | dflag, keep_prob, f.mask0, f.seed, c.scratch, w.scratch_floats, s));
  G(gemm_mode_call(x3, 0, B, FC2, FC1, ws + w.f1, FC1, W + P.fc_w[1], FC2, ws + w.f2, FC2, W + P.fc_b[1],
                   GF_BIAS | GF_RELU | dflag, keep_prob, f.mask1, f.seed ^ 0x5DEECE66Dull, c.scratch, w.scratch_floats, s));
  // fc3, sigmoid, log-loss, l2 (:74-94)
  G(score_launch_head_out(B, FC2, ws + w.f2, W + P.fc_w[2], W + P.fc_b[2], bt->label, ws + w.logit, ws + w.y_pred,
                          ws + w.lossb, ws + w.dlogit, ws + w.loss, f.reg_lambda, ws + w.part, c.Bg, s, st->id_status));
  if (st->loss_done_event) HIPTRY(hipEventRecord((hipEvent_t)st->loss_done_event, s));
  return 0;
}

// SCORE and its ablations, RRN: GRUs, then the attention (SCORE, RCA, SCORE_USER, SCORE_ITEM) or the final states, the fc head
int fwd_slice(const Pass& c, const FwdState& f) {
  const Dims& d = c.d; const WS& w = c.w; float* ws = c.ws; const int B = c.B, H = c.H; hipStream_t s = c.s;
  void* const* stage_events = f.stage_events;
  HIPTRY(hipStreamWaitEvent(s, f.sd->wx, 0));
  const float* xin[2] = {ws + w.xside[0], ws + w.xside[1]};
  G(fwd_grus_two_sided(c, f, xin));
  EV(2);
  if (d.attn) {
    G(fwd_attention(c, f));
  } else {
    // RIA: final GRU states feed the head (:244-249)
    G(score_launch_copy2d(B, H, ws + w.gru_final[0], H, ws + w.head_inp, d.Dhead, s));
    G(score_launch_copy2d(B, H, ws + w.gru_final[1], H, ws + w.head_inp + H, d.Dhead, s));
  }
  EV(3);
  if (!d.attn) HIPTRY(hipStreamWaitEvent(s, f.sd->join, 0));     // (with attention the join was waited for there)
  G(fwd_fc_head(c, f));
  EV(4);
  return 0;
}

int fwd_gcmc(const Pass& c, const FwdState& f) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w;
  float* ws = c.ws; const float* W = c.W; const int B = c.B, H = c.H, BT = c.BT; hipStream_t s = c.s;
  void* const* stage_events = f.stage_events;
  // GCMC (slice_model.py:182-190): per side A = relu(S Wa), Z = relu(A Wc), S the 1-hop sum the gather left in xside.  TF applies
  // Wa to every neighbour and sums; summing first is the same by linearity, with K times fewer flops
  for (int sd = 0; sd < 2; ++sd) {
    const int Dx = d.Is[sd];
    G(gemm_mode_call(c.x3, 0, BT, Dx, Dx, ws + w.xside[sd], d.I, W + P.gm_a[sd], Dx, ws + w.gcmc_a[sd], Dx, nullptr, GF_RELU, 1.f,
                     nullptr, 0, c.scratch, w.scratch_floats, s));
    G(gemm_mode_call(c.x3, 0, BT, Dx, Dx, ws + w.gcmc_a[sd], Dx, W + P.gm_c[sd], Dx, ws + w.gcmc_z[sd], Dx, nullptr, GF_RELU, 1.f,
                     nullptr, 0, c.scratch, w.scratch_floats, s));
  }
  HIPTRY(hipStreamWaitEvent(s, f.sd->wx, 0));
  const float* xin[2] = {ws + w.gcmc_z[0], ws + w.gcmc_z[1]};
  G(fwd_grus_two_sided(c, f, xin));
  EV(2);
  EV(3);
  HIPTRY(hipStreamWaitEvent(s, f.sd->join, 0));
  // GCMC (:199-203): y = exp(a) / (exp(a) + exp(c)) of the final states, its log-loss term and dL/da (gcmc.hip); no dropout,
  // keep_prob has no effect
  G(score_launch_gcmc_head_fwd(B, H, ws + w.gru_final[0], ws + w.gru_final[1], W + P.gm_4, W + P.gm_5, c.bt->label, ws + w.y_pred,
                               ws + w.lossb, ws + w.gcmc_pn, ws + w.gcmc_pn + (int64_t)B * H, ws + w.gcmc_g, c.Bg, s));
  G(loss_tail(c, f.sd, f.reg_lambda));
  EV(4);
  return 0;
}

int fwd_g4r(const Pass& c, const FwdState& f) {
  hipStream_t s = c.s;
  void* const* stage_events = f.stage_events;
  HIPTRY(hipStreamWaitEvent(s, f.sd->wx, 0));
  G(g4r_grus_fwd(c));
  EV(2);
  // GRU4Rec (point_model.py:134): layer 2's final state feeds the head
  G(score_launch_copy2d(c.B, c.H, c.ws + c.w.gru_final[1], c.H, c.ws + c.w.head_inp, c.d.Dhead, s));
  EV(3);
  HIPTRY(hipStreamWaitEvent(s, f.sd->join, 0));
  G(fwd_fc_head(c, f));
  EV(4);
  return 0;
}

int fwd_caser(const Pass& c, const FwdState& f) {
  hipStream_t s = c.s;
  void* const* stage_events = f.stage_events;
  // Caser has no GRU: both convolutions, the max over the windows and the scalar dense in ONE launch, straight into head_inp
  CaserArgs a;
  caser_args(c, nullptr, &a);
  G(score_caser_fwd(a, s));
  EV(2);
  EV(3);
  HIPTRY(hipStreamWaitEvent(s, f.sd->join, 0));
  G(fwd_fc_head(c, f));
  EV(4);
  return 0;
}

int fwd_delf(const Pass& c, const FwdState& f) {
  hipStream_t s = c.s;
  void* const* stage_events = f.stage_events;
  // DELF: both attentions, the fusion MLPs, y and the loss terms in ONE launch behind the gather (the target rows come from
  // the side stream); no dropout, keep_prob has no effect
  HIPTRY(hipStreamWaitEvent(s, f.sd->join, 0));
  DelfArgs a;
  delf_args(c, &a);
  G(score_delf_fwd(a, s));
  EV(2);
  EV(3);
  G(loss_tail(c, f.sd, f.reg_lambda));
  EV(4);
  return 0;
}

int fwd_svdpp(const Pass& c, const FwdState& f) {
  hipStream_t s = c.s;
  void* const* stage_events = f.stage_events;
  // SVD++: the factor sums, the norm, y and the loss terms in ONE launch behind the gather (the target rows come from the side
  // stream); no dropout, keep_prob has no effect
  HIPTRY(hipStreamWaitEvent(s, f.sd->join, 0));
  SvdppArgs a;
  svdpp_args(c, &a);
  G(score_svdpp_fwd(a, s));
  EV(2);
  EV(3);
  G(loss_tail(c, f.sd, f.reg_lambda));
  EV(4);
  return 0;
}

int fwd_sasrec(const Pass& c, const FwdState& f) {
  const WS& w = c.w; hipStream_t s = c.s;
  void* const* stage_events = f.stage_events;
  // SASRec: layer norm, attention, rep / final and the head-input rows in ONE launch behind the gather (the target rows come from
  // the side stream)
  HIPTRY(hipStreamWaitEvent(s, f.sd->join, 0));
  SasrecArgs a;
  sasrec_args(c, f.keep_prob, f.mask0, f.mask1, f.seed, &a);
  G(score_sasrec_attn_fwd(a, s));
  EV(2);
  // the shared head: fc1's pre-activations ONCE over the positive and the final rows, fanned out into the three applications'
  // dropout groups; fc2 over all rows; fc3, the sigmoid, the three loss means and the gradients at the logits in one launch
  const int R1 = sasrec_rows1(c), R = sasrec_rows(c, a);
  G(gemm_mode_call(c.x3, 0, R1, FC1, a.Dh, a.hin, a.Dh, c.W + c.P.fc_w[0], FC1, a.z1, FC1, c.W + c.P.fc_b[0], GF_BIAS, 1.f, nullptr, 0,
                   c.scratch, w.scratch_floats, s));
  G(score_sasrec_fan(a, s));
  G(gemm_mode_call(c.x3, 0, R, FC2, FC1, a.f1, FC1, c.W + c.P.fc_w[1], FC2, a.z2, FC2, c.W + c.P.fc_b[1], GF_BIAS, 1.f, nullptr, 0,
                   c.scratch, w.scratch_floats, s));
  EV(3);
  G(score_sasrec_out(a, s));
  G(loss_tail(c, f.sd, f.reg_lambda));
  EV(4);
  return 0;
}

int fwd_deems(const Pass& c, const FwdState& f) {
  const WS& w = c.w; const int B = c.B; hipStream_t s = c.s;
  void* const* stage_events = f.stage_events;
  HIPTRY(hipStreamWaitEvent(s, f.sd->wx, 0));
  G(deems_grus_fwd(c));
  EV(2);
  EV(3);
  HIPTRY(hipStreamWaitEvent(s, f.sd->join, 0));       // (the target rows in head_inp come from the side stream)
  DeemsArgs a;
  deems_args(c, f.keep_prob, f.mask0, f.mask1, f.seed, &a);
  // both towers, y and the loss terms in ONE launch (deems.hip); the final states go into head_inp on the way
  int hrc = c.fl.head_unfused ? SCORE_E_SHAPE : score_deems_head_fwd(a, s);
  if (hrc != 0 && hrc != SCORE_E_SHAPE) return hrc;
  if (hrc == SCORE_E_SHAPE) {       // ... or layer by layer: bn of both towers, then each tower's three denses, then the combine
    if (c.st->step_scalars && f.keep_prob < 1.f) return SCORE_E_SHAPE;   // (this form takes its seed by value)
    const int dflag = f.keep_prob < 1.f ? GF_DROP : 0;
    G(score_deems_bn_fwd(a, s));
    for (int k = 0; k < 2; ++k) {
      const DeemsTower& t = a.t[k];
      const uint64_t seed = f.seed ^ (k ? SCORE_DEEMS_ITEM_SEED : 0ull);
      G(gemm_mode_call(c.x3, 0, B, FC1, t.Dh, a.bn + t.col, a.ld, t.W1, FC1, t.f1, FC1, t.b1, GF_BIAS | GF_RELU | dflag, f.keep_prob,
                       t.mask0, seed, c.scratch, w.scratch_floats, s));
      G(gemm_mode_call(c.x3, 0, B, FC2, FC1, t.f1, FC1, t.W2, FC2, t.f2, FC2, t.b2, GF_BIAS | GF_RELU | dflag, f.keep_prob, t.mask1,
                       seed ^ 0x5DEECE66Dull, c.scratch, w.scratch_floats, s));
      G(gemm_mode_call(c.x3, 0, B, 1, FC2, t.f2, FC2, t.W3, 1, t.logit, 1, t.b3, GF_BIAS, 1.f, nullptr, 0, c.scratch,
                       w.scratch_floats, s));
    }
    G(score_deems_out(a, s));
  }
  G(loss_tail(c, f.sd, f.reg_lambda));
  EV(4);
  return 0;
}
}  // namespace

extern "C" int score_forward(const score_config_t* cfg, const score_state_t* st, const score_batch_t* bt,
                             float reg_lambda, float keep_prob, const uint8_t* drop_mask0,
                             const uint8_t* drop_mask1, uint64_t drop_seed, void* const* stage_events,
                             void* stream) {
  Pass c;
  SCORE_TRY(make_dims(cfg, &c.d));
  if (!st || !bt || !st->table || !st->w || !st->workspace || bt->B <= 0) return SCORE_E_BADARG;
  if (!bt->user_1hop || !bt->user_2hop || !bt->item_1hop || !bt->item_2hop || !bt->target_user ||
      !bt->target_item || !bt->label || !bt->length)
    return SCORE_E_BADARG;
  if ((c.d.family == FAM_DELF || c.d.family == FAM_DEEMS) && !bt->length2) return SCORE_E_BADARG;        // (item_seq_length: the model types that read it)
  if (!(keep_prob > 0.f) || keep_prob > 1.f) return SCORE_E_BADARG;
  SCORE_TRY(pass_fill(&c, st, bt, stream));
  score_head_forms_begin(0);
  {
    PsPlan pp;       // the reference's own shapes: the whole pass as one kernel per sample (persample.h)
    if (!c.fl.ps_bwd_only && ps_path(c.d, st, bt, c.T, &pp))
      return forward_ps(c, pp, reg_lambda, keep_prob, drop_mask0, drop_mask1, drop_seed, stage_events);
  }
  FwdState f = {reg_lambda, keep_prob, drop_mask0, drop_mask1, drop_seed, stage_events, nullptr, false};
  SCORE_TRY(fwd_open(c, &f));
  switch (c.d.family) {
    case FAM_SLICE: return fwd_slice(c, f);
    case FAM_GCMC: return fwd_gcmc(c, f);
    case FAM_G4R: return fwd_g4r(c, f);
    case FAM_CASER: return fwd_caser(c, f);
    case FAM_DELF: return fwd_delf(c, f);
    case FAM_DEEMS: return fwd_deems(c, f);
    case FAM_SVDPP: return fwd_svdpp(c, f);
    case FAM_SASREC: return fwd_sasrec(c, f);
  }
  return SCORE_E_BADARG;
}

// ---------------------------------------------------------------- the line-form ranking pass (GRU4Rec, Caser; rank.hip)
// L target lines of C candidates (include/score_hip.h: score_rank_forward): fwd_open and the history encoder at B = L -- the
// launches score_forward makes for a batch of L samples, up to the head --, then the line-form head and the loss reduction over
// the L * C terms.
namespace {
// What every line-form pass keeps behind the workspace of a batch of L samples (build_ws at B = L, untouched): the lines' part of
// fc1's pre-activation [L, FC1], then `mid` floats of the pass's own (none at 0), then zero ids for the three index tensors a point
// model's batch does not have and for the target item of the B = L pass (int32 [L * T * max(Fu, Fi)]; the head input's item columns
// get row 0 there and are not read).  -> the Taker behind them, for what the pass carves next
struct LineWS { int64_t zline, mid, zero_ids, n_zero_ids; };
Taker carve_line_ws(const Dims& d, int L, int64_t mid, LineWS* r) {
  WS w;
  build_ws(d, L, &w);
  Taker take = {w.total};
  r->zline = take((int64_t)L * FC1);
  r->mid = mid > 0 ? take(mid) : 0;
  r->n_zero_ids = (int64_t)L * d.T * (d.Fu > d.Fi ? d.Fu : d.Fi);
  r->zero_ids = take(r->n_zero_ids);
  return take;
}
// the ranking pass: mid = the per-sample loss terms [L * C]
struct RankWS : LineWS { int64_t total; };
void build_rank_ws(const Dims& d, int L, int C, RankWS* r) {
  r->total = carve_line_ws(d, L, (int64_t)L * C, r).cur;
}
// the model types and shapes the pass covers, and its argument checks that need no device
int rank_dims(const score_config_t* cfg, int L, int C, Dims* d) {
  SCORE_TRY(make_dims(cfg, d));
  if (d->family != FAM_G4R && d->family != FAM_CASER) return SCORE_E_SHAPE;
  if (L <= 0 || C <= 0) return SCORE_E_BADARG;
  if (!score_rank_head_fits(L, C, d->Dhead, d->off_ti, d->Di, d->D, FC1, FC2)) return SCORE_E_SHAPE;
  return 0;
}
// What score_rank_forward and score_catalog_topk share, in front of their heads: the zero ids, the lines as a batch of L samples
// (*lb), pass_fill, fwd_open, the history encoder and the side stream's join.  c->d is set; label: [>= L] int32 (not read in
// front of the head)
int rank_prefix(Pass* c, FwdState* f, score_batch_t* lb, const score_state_t* st, const int32_t* user_seq, const int32_t* length,
                const int32_t* target_user, const int32_t* label, int L, int active_slices, int32_t* zero_ids, int64_t n_zero_ids,
                void* stream) {
  const Dims& d = c->d;
  hipStream_t s = (hipStream_t)stream;
  HIPTRY(hipMemsetAsync(zero_ids, 0, (size_t)n_zero_ids * sizeof(int32_t), s));
  // the lines as a batch of L samples: user_seq rides as user_1hop [L, T, 1, Fi], as in a point model's score_batch_t
  memset(lb, 0, sizeof(*lb));
  lb->user_1hop = user_seq; lb->user_2hop = lb->item_1hop = lb->item_2hop = zero_ids;
  lb->target_user = target_user; lb->target_item = zero_ids; lb->label = label ? label : zero_ids; lb->length = length;
  lb->B = L; lb->active_slices = active_slices;
  SCORE_TRY(pass_fill(c, st, lb, stream));
  SCORE_TRY(fwd_open(*c, f));
  float* ws = c->ws;
  if (d.family == FAM_G4R) {       // (fwd_g4r's launches in front of the head)
    HIPTRY(hipStreamWaitEvent(s, f->sd->wx, 0));
    G(g4r_grus_fwd(*c));
    G(score_launch_copy2d(L, c->H, ws + c->w.gru_final[1], c->H, ws + c->w.head_inp, d.Dhead, s));
  } else {                         // (fwd_caser's)
    CaserArgs a;
    caser_args(*c, nullptr, &a);
    G(score_caser_fwd(a, s));
  }
  HIPTRY(hipStreamWaitEvent(s, f->sd->join, 0));       // (the target-user rows and the L2 partial sums come from the side stream)
  return 0;
}
// the head's side of RankArgs: what the line kernel and the tile kernel read of the model
void rank_head_args(const Pass& c, const score_state_t* st, int L, int C, RankArgs* a) {
  const Dims& d = c.d; const float* W = c.W; const Params& P = c.P;
  memset(a, 0, sizeof(*a));
  a->L = L; a->C = C; a->Dh = d.Dhead; a->off_ti = d.off_ti; a->Di = d.Di; a->D = d.D; a->N1 = FC1; a->N2 = FC2;
  a->head = c.ws + c.w.head_inp; a->table = st->table;
  a->gamma = W + P.bn_g; a->beta = W + P.bn_b; a->rs = c.rs;
  a->W1 = W + P.fc_w[0]; a->b1 = W + P.fc_b[0]; a->W2 = W + P.fc_w[1]; a->b2 = W + P.fc_b[1]; a->W3 = W + P.fc_w[2]; a->b3 = W + P.fc_b[2];
  a->n_rows = c.n_rows; a->id_status = st->id_status;
}
}  // namespace

extern "C" int score_rank_workspace_bytes(const score_config_t* cfg, int32_t L, int32_t C, int64_t* bytes) {
  if (!cfg || !bytes) return SCORE_E_BADARG;
  Dims d;
  SCORE_TRY(rank_dims(cfg, L, C, &d));
  RankWS r;
  build_rank_ws(d, L, C, &r);
  *bytes = r.total * 4;
  return 0;
}

extern "C" int score_rank_forward(const score_config_t* cfg, const score_state_t* st, const score_rank_batch_t* rb,
                                  float reg_lambda, float* y_pred, float* loss, void* stream) {
  if (!cfg || !st || !rb || !y_pred || !loss) return SCORE_E_BADARG;
  Pass c;
  SCORE_TRY(rank_dims(cfg, rb->L, rb->C, &c.d));
  if (!st->table || !st->w || !st->workspace) return SCORE_E_BADARG;
  if (!rb->user_seq || !rb->length || !rb->target_user || !rb->cand_items || !rb->label) return SCORE_E_BADARG;
  const Dims& d = c.d;
  const int L = rb->L, C = rb->C;
  RankWS r;
  build_rank_ws(d, L, C, &r);
  if (r.total * 4 > st->workspace_bytes) return SCORE_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  score_batch_t lb;
  FwdState f = {reg_lambda, 1.f, nullptr, nullptr, 0, nullptr, nullptr, false};
  SCORE_TRY(rank_prefix(&c, &f, &lb, st, rb->user_seq, rb->length, rb->target_user, rb->label, L, rb->active_slices,
                        reinterpret_cast<int32_t*>(st->workspace + r.zero_ids), r.n_zero_ids, stream));
  float* ws = c.ws;
  RankArgs a;
  rank_head_args(c, st, L, C, &a);
  a.cand = rb->cand_items; a.label = rb->label;
  a.zline = ws + r.zline; a.y = y_pred; a.lossb = ws + r.mid;
  G(score_rank_head(a, s));
  return loss_tail_at(c, f.sd, reg_lambda, L * C, ws + r.mid, loss, global_batch(st, L * C));
}

// ---------------------------------------------------------------- top-K over a whole item catalogue (GRU4Rec, Caser; catalog.hip)
// score_catalog_build: zcat [N, 200], the catalogue's half of fc1's pre-activation.  score_catalog_topk: the prefix of the
// ranking pass at B = L, the line kernel alone, then a scoring workgroup per (line, chunk) and a merge per line.
namespace {
// The workspace of every catalogue pass: zline and the zero ids (LineWS, nothing between them), then the per-chunk region -- the
// selecting form's lists, [L, nchunk, k] 64-bit keys, or the counting form's integer partials, [L, nchunk, SCORE_CATALOG_RPART]
// int32.  span, what the plan cuts: N, or the candidate lists' max_count
struct CatalogWS : LineWS { int64_t part, total; int chunk, nchunk; };
void build_catalog_ws(const Dims& d, int L, int span, int k, bool counting, CatalogWS* r) {
  score_catalog_chunks(L, span, counting ? 1 : k, &r->chunk, &r->nchunk);
  Taker take = carve_line_ws(d, L, 0, r);
  r->part = take((int64_t)L * r->nchunk * (counting ? (int64_t)SCORE_CATALOG_RPART : (int64_t)k * 2));
  r->total = take.cur;
}
// what a *_struct_sizes function does with its value list: -> the number of values written, SCORE_E_BADARG for a null pointer or n
// too small
template <int32_t HAVE>
int copy_sizes(const int64_t (&v)[HAVE], int64_t* out, int32_t n) {
  if (!out || n < HAVE) return SCORE_E_BADARG;
  for (int32_t i = 0; i < HAVE; ++i) out[i] = v[i];
  return HAVE;
}
const int32_t CATALOG_NMAX = 1 << 30;        // (a step past the last item stays inside int32)
int catalog_dims(const score_config_t* cfg, int L, int N, int k, Dims* d) {
  SCORE_TRY(rank_dims(cfg, L, 1, d));
  if (N <= 0 || k < 1 || k > SCORE_CATALOG_KMAX) return SCORE_E_BADARG;
  if (N > CATALOG_NMAX) return SCORE_E_SHAPE;
  int chunk, nchunk;
  score_catalog_chunks(L, N, k, &chunk, &nchunk);
  if ((int64_t)L * nchunk >= (1LL << 31)) return SCORE_E_SHAPE;
  return 0;
}
void catalog_model_args(const Dims& d, const score_state_t* st, const score_catalog_t* cat, CatalogArgs* a) {
  Params P;
  build_layout(d, nullptr, 0, &P);
  const float* W = st->w;
  memset(a, 0, sizeof(*a));
  a->N = cat->N; a->Di = d.Di; a->D = d.D; a->off_ti = d.off_ti; a->N1 = FC1;
  a->table = st->table; a->item_rows = cat->item_rows; a->zcat = cat->zcat;
  a->gamma = W + P.bn_g; a->beta = W + P.bn_b; a->rs = (float)(1.0 / sqrt(1.0 + 1e-3));
  a->W1 = W + P.fc_w[0]; a->W2 = W + P.fc_w[1]; a->b2 = W + P.fc_b[1]; a->W3 = W + P.fc_w[2]; a->b3 = W + P.fc_b[2];
  a->n_rows = clamp_rows(st->n_table_rows); a->id_status = st->id_status;
}
// The front half of every catalogue pass -- THE place to extend for a new form: the checks (cands null: every line
// against the whole catalogue; else against its own list), the workspace, rank_prefix, the line kernel, and *a with the model's
// side and every field the forms share.  k: 1 for the counting form.  own_ok: the form's own pointer checks, tested where they
// have always stood, behind the shape checks and in front of the workspace's.  -> *part, the per-chunk region
int catalog_front(const score_config_t* cfg, const score_state_t* st, const score_catalog_t* cat, const score_catalog_lines_t* ln,
                  const score_catalog_cands_t* cands, int32_t k, bool counting, bool own_ok, void* stream, CatalogArgs* a,
                  float** part) {
  Pass c;
  SCORE_TRY(catalog_dims(cfg, ln->L, cat->N, k, &c.d));
  if (cands) SCORE_TRY(catalog_dims(cfg, ln->L, cands->max_count, k, &c.d));
  if (!st->table || !st->w || !st->workspace || !cat->item_rows || !cat->zcat) return SCORE_E_BADARG;
  if (!ln->user_seq || !ln->length || !ln->target_user || (ln->excl_off && !ln->excl_idx)) return SCORE_E_BADARG;
  if (cands && (!cands->cand_off || !cands->cand_idx)) return SCORE_E_BADARG;
  if (!own_ok) return SCORE_E_BADARG;
  const Dims& d = c.d;
  const int L = ln->L;
  CatalogWS r;
  build_catalog_ws(d, L, cands ? cands->max_count : cat->N, k, counting, &r);
  if (r.total * 4 > st->workspace_bytes) return SCORE_E_WORKSPACE;
  score_batch_t lb;
  FwdState f = {0.f, 1.f, nullptr, nullptr, 0, nullptr, nullptr, false};
  SCORE_TRY(rank_prefix(&c, &f, &lb, st, ln->user_seq, ln->length, ln->target_user, nullptr, L, ln->active_slices,
                        reinterpret_cast<int32_t*>(st->workspace + r.zero_ids), r.n_zero_ids, stream));
  float* ws = c.ws;
  RankArgs ra;
  rank_head_args(c, st, L, 1, &ra);
  ra.zline = ws + r.zline;
  G(score_rank_line(ra, (hipStream_t)stream));
  catalog_model_args(d, st, cat, a);
  a->L = L; a->k = k; a->chunk = r.chunk; a->nchunk = r.nchunk;
  a->zline = ws + r.zline; a->excl_off = ln->excl_off; a->excl_idx = ln->excl_idx;
  if (cands) { a->cand_off = cands->cand_off; a->cand_idx = cands->cand_idx; a->max_count = cands->max_count; }
  *part = ws + r.part;
  return 0;
}
// score_catalog_topk (cands null; logits = all_logits [L, N]) and score_catalog_topk_in (logits = cand_logits): the front, then
// the selection
int catalog_topk(const score_config_t* cfg, const score_state_t* st, const score_catalog_t* cat, const score_catalog_lines_t* ln,
                 const score_catalog_cands_t* cands, int32_t k, int32_t* top_idx, float* top_logit, float* logits, void* stream) {
  CatalogArgs a;
  float* part;
  SCORE_TRY(catalog_front(cfg, st, cat, ln, cands, k, false, true, stream, &a, &part));
  a.part = reinterpret_cast<unsigned long long*>(part);
  a.top_idx = top_idx; a.top_logit = top_logit; a.all_logits = logits;
  return score_catalog_sweep(a, cands != nullptr, false, (hipStream_t)stream);
}
// score_catalog_ranks / score_catalog_ranks_in, the exact rank of given items: the front, then the counting form of the scoring
// kernel and its reduce
int catalog_ranks(const score_config_t* cfg, const score_state_t* st, const score_catalog_t* cat, const score_catalog_lines_t* ln,
                  const score_catalog_cands_t* cands, const score_catalog_targets_t* tg, int32_t* ahead, float* tgt_logit,
                  int32_t* state, int32_t* n_scored, void* stream) {
  if (tg->max_targets < 1 || tg->max_targets > SCORE_CATALOG_TMAX) return SCORE_E_BADARG;
  CatalogArgs a;
  float* part;
  SCORE_TRY(catalog_front(cfg, st, cat, ln, cands, 1, true, tg->tgt_off && tg->tgt_idx, stream, &a, &part));
  a.tgt_off = tg->tgt_off; a.tgt_idx = tg->tgt_idx; a.max_targets = tg->max_targets;
  a.rpart = reinterpret_cast<int32_t*>(part);
  a.ahead = ahead; a.tgt_logit = tgt_logit; a.state = state; a.n_scored = n_scored;
  return score_catalog_sweep(a, cands != nullptr, true, (hipStream_t)stream);
}
// score_catalog_plan / score_catalog_ranks_plan (k = 1, counting)
int catalog_plan(const score_config_t* cfg, int32_t L, int32_t span, int32_t k, bool counting, int32_t* chunk, int32_t* nchunk,
                 int64_t* workspace_bytes) {
  if (!cfg || !chunk || !nchunk || !workspace_bytes) return SCORE_E_BADARG;
  Dims d;
  SCORE_TRY(catalog_dims(cfg, L, span, k, &d));
  CatalogWS r;
  build_catalog_ws(d, L, span, k, counting, &r);
  *chunk = r.chunk; *nchunk = r.nchunk; *workspace_bytes = r.total * 4;
  return 0;
}
}  // namespace

extern "C" int score_catalog_plan(const score_config_t* cfg, int32_t L, int32_t N, int32_t k, int32_t* chunk, int32_t* nchunk,
                                  int64_t* workspace_bytes) {
  return catalog_plan(cfg, L, N, k, false, chunk, nchunk, workspace_bytes);
}

extern "C" int score_catalog_build(const score_config_t* cfg, const score_state_t* st, const score_catalog_t* cat, void* stream) {
  if (!cfg || !st || !cat) return SCORE_E_BADARG;
  Dims d;
  SCORE_TRY(rank_dims(cfg, 1, 1, &d));
  if (!st->table || !st->w || !cat->item_rows || !cat->zcat || cat->N <= 0) return SCORE_E_BADARG;
  if (cat->N > CATALOG_NMAX) return SCORE_E_SHAPE;
  CatalogArgs a;
  catalog_model_args(d, st, cat, &a);
  return score_catalog_zcat(a, (hipStream_t)stream);
}

extern "C" int score_catalog_topk(const score_config_t* cfg, const score_state_t* st, const score_catalog_t* cat,
                                  const score_catalog_lines_t* ln, int32_t k, int32_t* top_idx, float* top_logit, float* all_logits,
                                  void* stream) {
  if (!cfg || !st || !cat || !ln || !top_idx || !top_logit) return SCORE_E_BADARG;
  return catalog_topk(cfg, st, cat, ln, nullptr, k, top_idx, top_logit, all_logits, stream);
}

// ---- ... within per-line candidate lists.  The plan: score_catalog_plan's with the longest list in N's place
extern "C" int score_catalog_cands_plan(const score_config_t* cfg, int32_t L, int32_t max_count, int32_t k, int32_t* chunk,
                                        int32_t* nchunk, int64_t* workspace_bytes) {
  return score_catalog_plan(cfg, L, max_count, k, chunk, nchunk, workspace_bytes);
}

extern "C" int score_catalog_topk_in(const score_config_t* cfg, const score_state_t* st, const score_catalog_t* cat,
                                     const score_catalog_lines_t* ln, const score_catalog_cands_t* cands, int32_t k,
                                     int32_t* top_idx, float* top_logit, float* cand_logits, void* stream) {
  if (!cfg || !st || !cat || !ln || !cands || !top_idx || !top_logit) return SCORE_E_BADARG;
  return catalog_topk(cfg, st, cat, ln, cands, k, top_idx, top_logit, cand_logits, stream);
}

extern "C" int score_catalog_cands_struct_sizes(int64_t* out, int32_t n) {
  const int64_t v[] = {(int64_t)sizeof(score_catalog_cands_t), (int64_t)offsetof(score_catalog_cands_t, cand_off),
                       (int64_t)offsetof(score_catalog_cands_t, cand_idx), (int64_t)offsetof(score_catalog_cands_t, max_count)};
  return copy_sizes(v, out, n);
}

// ---- ... the exact rank of given items (catalog_ranks)
extern "C" int score_catalog_ranks_plan(const score_config_t* cfg, int32_t L, int32_t span, int32_t* chunk, int32_t* nchunk,
                                        int64_t* workspace_bytes) {
  return catalog_plan(cfg, L, span, 1, true, chunk, nchunk, workspace_bytes);
}

extern "C" int score_catalog_ranks(const score_config_t* cfg, const score_state_t* st, const score_catalog_t* cat,
                                   const score_catalog_lines_t* ln, const score_catalog_targets_t* tg, int32_t* ahead,
                                   float* tgt_logit, int32_t* state, int32_t* n_scored, void* stream) {
  if (!cfg || !st || !cat || !ln || !tg || !ahead || !tgt_logit || !state || !n_scored) return SCORE_E_BADARG;
  return catalog_ranks(cfg, st, cat, ln, nullptr, tg, ahead, tgt_logit, state, n_scored, stream);
}

extern "C" int score_catalog_ranks_in(const score_config_t* cfg, const score_state_t* st, const score_catalog_t* cat,
                                      const score_catalog_lines_t* ln, const score_catalog_cands_t* cands,
                                      const score_catalog_targets_t* tg, int32_t* ahead, float* tgt_logit, int32_t* state,
                                      int32_t* n_scored, void* stream) {
  if (!cfg || !st || !cat || !ln || !cands || !tg || !ahead || !tgt_logit || !state || !n_scored) return SCORE_E_BADARG;
  return catalog_ranks(cfg, st, cat, ln, cands, tg, ahead, tgt_logit, state, n_scored, stream);
}

extern "C" int score_catalog_ranks_struct_sizes(int64_t* out, int32_t n) {
  const int64_t v[] = {(int64_t)sizeof(score_catalog_targets_t), (int64_t)offsetof(score_catalog_targets_t, tgt_off),
                       (int64_t)offsetof(score_catalog_targets_t, tgt_idx), (int64_t)offsetof(score_catalog_targets_t, max_targets),
                       (int64_t)SCORE_CATALOG_TMAX};
  return copy_sizes(v, out, n);
}

// sizes and late-field offsets of the catalogue call's structures, as score_abi_struct_sizes gives them for the others: -> the
// number of values written, SCORE_E_BADARG for a null pointer or n too small.  Host only.
extern "C" int score_catalog_struct_sizes(int64_t* out, int32_t n) {
  const int64_t v[] = {(int64_t)sizeof(score_catalog_t), (int64_t)sizeof(score_catalog_lines_t),
                       (int64_t)offsetof(score_catalog_t, zcat), (int64_t)offsetof(score_catalog_lines_t, excl_off),
                       (int64_t)offsetof(score_catalog_lines_t, excl_idx), (int64_t)SCORE_CATALOG_KMAX};
  return copy_sizes(v, out, n);
}

// ---------------------------------------------------------------- the layer-by-layer backward pass
// ONE function per family (bwd_slice .. bwd_delf), each the list of its stages: bwd_open, the head's backward, the attention's
// backward or the final states' gradients, bwd_side_products, the recurrences' backward, the input gradients, bwd_close.
namespace {
// score_backward's arguments behind the batch, and what the stages of a pass hand to each other
struct BwdState {
  float keep_prob; float* gw; float* grad_table; void* const* stage_events;
  SideStream* side;
  GradQueues q;
  const float* dfinal[2];     // dL/d final state of each recurrence (null: none enters there)
  int gru_bias_rows;          // GruArgs.bias_slab_rows of the backward recurrence that ran
};
// region of the first flush of the queued products (bwd_side_products) in the split-K slabs; the second one's (bwd_close) follows
inline int64_t slab_half(const WS& w) { return (w.dwslab_floats / 4) & ~(int64_t)3; }

// The dense gradient starts from zero (some of its pieces are accumulated, some variables of some model types get
// none).  Nothing on the main stream writes it before the side stream's join (bwd_side_products) -- every weight / bias
// gradient is queued -- so the fill runs on the side stream, off the chain of dependent launches.  Ends with EV(0).
int bwd_open(const Pass& c, BwdState* b) {
  hipStream_t s = c.s;
  void* const* stage_events = b->stage_events;
  SideStream* side = nullptr;
  G(side_stream(c.st, s, &side));
  b->side = side;
  // (the fill needs the side stream behind the LAST readers of grad_w -- the previous step's optimizer --, not behind this pass's
  //  forward: score_forward of this step, on this stream and context, forked the side stream behind them already.  A record between
  //  the head's forward and backward costs the launch stream a ~6-us bubble; only a caller that skipped the forward pays it.)
  const bool forked = side->fwd_on == s;
  side->fwd_on = nullptr;
  if (!forked) G(fork_side(side, s));
  HIPTRY(hipMemsetAsync(b->gw, 0, c.P.n_floats * sizeof(float), side->st));
  EV(0);
  return 0;
}

// ---- head (score.py:68-81)
int bwd_fc_head(const Pass& c, BwdState* b) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w;
  float* ws = c.ws; const float* W = c.W; float* gw = b->gw; const int B = c.B, x3 = c.x3; hipStream_t s = c.s;
  const float keep_prob = b->keep_prob; const int64_t SF = w.scratch_floats;
  // fc3: dz2 = [f2>0] dlogit w3 / keep
  if (c.fl.head_unfused || !score_head_fwd_fused_fits(B, d.Dhead, FC1, FC2))     // (else score_forward's fused head wrote dz2)
    G(score_launch_outer_relu_bwd(B, FC2, ws + w.dlogit, W + P.fc_w[2], ws + w.f2, keep_prob, ws + w.dz2, s));
  // dz1, d bn1, d head input and bn1's d gamma terms: one launch (head_fused.hip) ...
  int hbrc = c.fl.head_unfused ? SCORE_E_SHAPE
                 : score_launch_head_bwd_fused(B, d.Dhead, FC1, FC2, ws + w.dz2, W + P.fc_w[1], ws + w.f1, keep_prob,
                                               W + P.fc_w[0], ws + w.head_inp, W + P.bn_g, c.rs, ws + w.dz1, ws + w.dbn,
                                               ws + w.dhead, ws + w.dgstage, s);
  if (hbrc != 0 && hbrc != SCORE_E_SHAPE) return hbrc;
  // (bn1's d gamma / d beta behind the fused kernel: column sums of what it wrote)
  G(queue_head(c, &b->q, gw, hbrc == 0));
  if (hbrc == SCORE_E_SHAPE) {     // ... or layer by layer
    G(gemm_mode_call(x3, 1, B, FC1, FC2, ws + w.dz2, FC2, W + P.fc_w[1], FC2, ws + w.dz1, FC1, nullptr, GF_RELUGRAD, keep_prob,
                     reinterpret_cast<const uint8_t*>(ws + w.f1), 0, c.scratch, SF, s));   // relu/dropout mask of fc1 in the epilogue
    G(gemm_mode_call(x3, 1, B, d.Dhead, FC1, ws + w.dz1, FC1, W + P.fc_w[0], FC1, ws + w.dbn, d.Dhead, nullptr, 0, 1.f,
                     nullptr, 0, c.scratch, SF, s));
    G(score_launch_bn_bwd(B, d.Dhead, ws + w.head_inp, W + P.bn_g, c.rs, ws + w.dbn, ws + w.dhead, gw + P.bn_g,
                          gw + P.bn_b, ws + w.dgstage, c.scratch, SF, &b->q.cq, s));
  }
  return 0;
}

// ---- temporal attention (score.py:169-186, 214-215)
int bwd_attention(const Pass& c, BwdState* b) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w; const score_batch_t* bt = c.bt;
  float* ws = c.ws; const float* W = c.W; const int B = c.B, T = c.T, H = c.H, BT = c.BT, x3 = c.x3; hipStream_t s = c.s;
  const int64_t SF = w.scratch_floats;
  G(queue_attn(c, &b->q, b->gw));
  // pooling / softmax / dense_5 backward and, in the same launch, dense_4's (da1 with dense_3's relu mask)
  // (on small batches the fused attention backward below does this part too -- one launch less: 0.0218 -> 0.0183 ms for
  //  the stage at the reference's own shape; at cfg-3, where a workgroup per four samples serialises what 1024 small
  //  workgroups do side by side, the separate launch stays: 0.0613 vs 0.0629)
  const bool pool_in_fused = !c.fl.attn_unfused && (int64_t)B * T < 8192 &&
                             score_attn_inp_bwd_fused_fits(B, T, H, d.NI, AT1, AT2, d.Dhead, d.off_u, d.off_i, true);
  int prc = pool_in_fused ? 0 : c.fl.attn_unfused ? SCORE_E_SHAPE
                : score_launch_attn_pool_bwd(B, T, H, AT2, ws + w.a2, W + P.at_w[3], bt->length, ws + w.gru_out[0],
                                             ws + w.gru_out[1], ws + w.att_score, ws + w.dhead, d.Dhead, d.off_u,
                                             d.off_i, ws + w.ds, ws + w.da2, s, AT1, W + P.at_w[2], ws + w.a1, ws + w.da1);
  if (prc != 0 && prc != SCORE_E_SHAPE) return prc;
  const bool da1_done = prc == 0;
  if (!da1_done) {
    G(score_launch_attn_pool_bwd(B, T, H, AT2, ws + w.a2, W + P.at_w[3], bt->length, ws + w.gru_out[0],
                                 ws + w.gru_out[1], ws + w.att_score, ws + w.dhead, d.Dhead, d.off_u, d.off_i,
                                 ws + w.ds, ws + w.da2, s));
    G(gemm_mode_call(x3, 1, BT, AT1, AT2, ws + w.da2, AT2, W + P.at_w[2], AT2, ws + w.da1, AT1, nullptr, GF_RELUGRAD, 1.f,
                     reinterpret_cast<const uint8_t*>(ws + w.a1), 0, c.scratch, SF, s));    // relu mask of dense_3 in the epilogue
  }
  // (sum_t da1 -> adzsum feeds the query branch only: computed on the side stream, bwd_side_products)
  // d inp = da1 . Weff^T and its way into d (states, atten_info, q): one launch where the shape allows (head_fused.hip).
  // dq = sum_t d(q*k).k here; the per-sample q-term gradient dzsum . Wq^T is added, and the query projection's
  // backward runs, on the side stream (bwd_side_products: beside the recurrence, only the target rows consume them)
  int brc = c.fl.attn_unfused ? SCORE_E_SHAPE
            : pool_in_fused
                ? score_launch_attn_inp_bwd_fused(B, T, H, d.NI, AT1, nullptr, ws + w.weff, ws + w.q, ws + w.gru_out[0],
                                                  ws + w.gru_out[1], ws + w.info, ws + w.att_score, ws + w.dhead, d.Dhead,
                                                  d.off_u, d.off_i, ws + w.dgru[0], ws + w.dgru[1], ws + w.dinfo, ws + w.dq, s,
                                                  AT2, ws + w.a2, ws + w.a1, W + P.at_w[3], W + P.at_w[2], bt->length,
                                                  ws + w.ds, ws + w.da2, ws + w.da1)
                : score_launch_attn_inp_bwd_fused(B, T, H, d.NI, AT1, ws + w.da1, ws + w.weff, ws + w.q, ws + w.gru_out[0],
                                                  ws + w.gru_out[1], ws + w.info, ws + w.att_score, ws + w.dhead, d.Dhead,
                                                  d.off_u, d.off_i, ws + w.dgru[0], ws + w.dgru[1], ws + w.dinfo, ws + w.dq, s);
  if (pool_in_fused && brc != 0) return brc == SCORE_E_SHAPE ? SCORE_E_BADARG : brc;     // (the predicate said it fits)
  if (brc != 0 && brc != SCORE_E_SHAPE) return brc;
  if (brc == SCORE_E_SHAPE) {
    G(gemm_mode_call(x3, 1, BT, 2 * d.Dk, AT1, ws + w.da1, AT1, ws + w.weff, AT1, ws + w.dainp, 2 * d.Dk, nullptr, 0,
                     1.f, nullptr, 0, c.scratch, SF, s));
    G(score_launch_attn_inp_bwd(B, T, H, d.NI, ws + w.dainp, ws + w.q, ws + w.gru_out[0], ws + w.gru_out[1],
                                ws + w.info, ws + w.att_score, ws + w.dhead, d.Dhead, d.off_u, d.off_i,
                                nullptr, ws + w.dgru[0], ws + w.dgru[1], ws + w.dinfo, ws + w.dq, s));
  }
  return 0;
}

// atten_info is unused downstream of a model without attention
int bwd_zero_dinfo(const Pass& c) {
  HIPTRY(hipMemsetAsync(c.ws + c.w.dinfo, 0, (int64_t)c.BT * 4 * c.d.K * sizeof(float), c.s));
  return 0;
}
// Without attention the gradient enters a recurrence through its final state only: dL/d final state of recurrence sd from the
// H columns of dhead at head_col (head_col < 0: a head kernel wrote dfinal already), zeros as its dL/d out (zero_dout)
int bwd_final_state(const Pass& c, BwdState* b, int sd, int head_col, bool zero_dout) {
  const WS& w = c.w; float* ws = c.ws; const int H = c.H;
  if (head_col >= 0) G(score_launch_copy2d(c.B, H, ws + w.dhead + head_col, c.d.Dhead, ws + w.dfinal[sd], H, c.s));
  b->dfinal[sd] = ws + w.dfinal[sd];
  if (zero_dout) HIPTRY(hipMemsetAsync(ws + w.dgru[sd], 0, (int64_t)c.BT * H * sizeof(float), c.s));
  return 0;
}
// ... of both sides' recurrences (from_head: the states lie side by side at the front of dhead), then dinfo
int bwd_final_states(const Pass& c, BwdState* b, bool from_head) {
  for (int sd = 0; sd < 2; ++sd) G(bwd_final_state(c, b, sd, from_head ? sd * c.H : -1, true));
  return bwd_zero_dinfo(c);
}

// The weight gradients queued so far (head, attention) have everything they need: on the side stream, beside the recurrence,
// behind the attention's query branch; the `join` record
int bwd_side_products(const Pass& c, BwdState* b) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w; const score_state_t* st = c.st;
  float* ws = c.ws; const float* W = c.W; float* gw = b->gw; const int B = c.B, x3 = c.x3; hipStream_t s = c.s;
  const int64_t SF = w.scratch_floats;
  SideStream* side = b->side;
  G(fork_side(side, s));
  // Sharded path (scatter_mode 2): the caller runs several streams of its own (plan prefetch, gradient exchange,
  // two communicators) and the hardware queues are shared -- measured there, this side stream's kernels run 2-4x
  // slower and the join below stalls the scatter (0.27 -> 0.40 ms): the query branch stays on the main stream
  const bool q_on_side = st->scatter_mode != 2;
  hipStream_t qs = q_on_side ? side->st : s;
  if (d.attn) {
    float* scratch2 = q_on_side ? ws + w.scratch2 : c.scratch;
    G(score_launch_attn_dzsum(B, c.T, AT1, ws + w.da1, ws + w.adzsum, qs));
    // dq += dzsum . Wq^T ; dense_2 (query projection): dW, db queued, d query = dq . W^T
    G(gemm_mode_call(x3, 1, B, d.Dk, AT1, ws + w.adzsum, AT1, ws + w.wq, AT1, ws + w.dq, d.Dk, nullptr, GF_ACC, 1.f, nullptr,
                     0, scratch2, SF, qs));
    G(queue_query(c, &b->q, gw));
    G(gemm_mode_call(x3, 1, B, d.Dq, d.Dk, ws + w.dq, d.Dk, W + P.at_w[0], d.Dk, ws + w.dquery, d.Dq, nullptr, 0, 1.f,
                     nullptr, 0, scratch2, SF, qs));
    // d query is what the main stream needs from here (target_bwd_kernel): its own event, so that the wait there does not
    // also sit behind the weight-gradient products and column sums that follow on this stream (at the small shapes the
    // side chain is as long as the main one: the scatter stage waited ~30 us for it)
    if (q_on_side) HIPTRY(hipEventRecord(side->wx, side->st));
    else G(fork_side(side, s));       // dq is final on the main stream: the side stream (its weight-gradient product) follows it
  }
  G(gemm_queue_flush(&b->q.gq, x3 != 0, ws + w.dwslab, slab_half(w), side->st));
  // the folded first attention layer's gradient from the two products just reduced (head.hip): here, off the launch stream
  if (d.attn) G(score_launch_attn_w1_grad(d.Dk, AT1, ws + w.dweff, ws + w.dwq, gw + P.at_w[1], side->st));
  // the bias / bn1 gradients known so far (column sums of matrices that are final by now), same place
  if (q_on_side) G(colsum_queue_flush(&b->q.cq, ws + w.cs_part, w.cs_part_floats / 2, side->st));
  HIPTRY(hipEventRecord(side->join, side->st));
  return 0;
}

// ---- GRUs (score.py:205-208) of the slice models and GCMC: both sides' backward recurrences in one launch
int bwd_grus_two_sided(const Pass& c, BwdState* b) {
  GruArgs ga;
  gru_header(c, &ga);
  for (int sd = 0; sd < 2; ++sd) {
    gru_side(c, sd, &ga.s[sd]);
    gru_side_bwd(c, sd, b->dfinal[sd], &ga.s[sd]);
  }
  G(score_gru_bwd_multi(ga, 2, c.s));
  b->gru_bias_rows = ga.bias_slab_rows;
  return 0;
}

// the recurrences' queued weight gradients and d x = [dgates | dcand] . [Wx_gates | Wx_cand]^T into dxside, slice models
int bwd_dx_slice(const Pass& c, BwdState* b) {
  const Dims& d = c.d; const WS& w = c.w; float* ws = c.ws; const int H = c.H, BT = c.BT, x3 = c.x3; hipStream_t s = c.s;
  const int64_t SF = w.scratch_floats;
  for (int sd = 0; sd < 2; ++sd) {
    G(queue_gru_side(c, &b->q, b->gw, sd, b->gru_bias_rows));
    if (d.Is[sd] != d.I)     // RRN: the 2-hop columns of this side carry no gradient
      HIPTRY(hipMemsetAsync(ws + w.dxside[sd], 0, (int64_t)BT * d.I * sizeof(float), s));
    if (d.Is[0] != d.Is[1])
      G(gemm_mode_call(x3, 1, BT, d.Is[sd], 3 * H, ws + w.dxproj[sd], 3 * H, wxcat(c, sd), 3 * H, ws + w.dxside[sd], d.I, nullptr, 0,
                       1.f, nullptr, 0, c.scratch, SF, s));
  }
  if (d.Is[0] == d.Is[1]) {      // both sides' d x in ONE grouped launch: 2 x 576 tiles fill 512 slots better than twice 576
    const float* Ad[2] = {ws + w.dxproj[0], ws + w.dxproj[1]};
    float* Cd[2] = {ws + w.dxside[0], ws + w.dxside[1]};
    if (panel_gemms(d, c.st, BT, 1)) {      // (the images were written by the forward pass, like the concatenated copies)
      G(panel_launch(c, 1, Ad, Cd));
    } else {
      const float* Bd[2] = {wxcat(c, 0), wxcat(c, 1)};
      G(score_gemm_same_shape(1, 2, BT, d.Is[0], 3 * H, Ad, 3 * H, Bd, 3 * H, Cd, d.I, 0, x3 != 0, c.scratch, SF, s));
    }
  }
  return 0;
}

// ... GCMC: through its two denses (slice_model.py:186-190): dZ [Z>0] = (dxproj Wx^T) [Z>0] -> dWc = A^T (.) ; dA = (.) Wc^T [A>0] ->
// dWa = S^T dA ; dS = dA Wa^T, the gradient of the 1-hop sum (its 2-hop columns stay zero, as for RRN)
int bwd_dx_gcmc(const Pass& c, BwdState* b) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w;
  float* ws = c.ws; const float* W = c.W; float* gw = b->gw; const int H = c.H, BT = c.BT, x3 = c.x3; hipStream_t s = c.s;
  const int64_t SF = w.scratch_floats;
  GemmQueue& gq = b->q.gq;
  for (int sd = 0; sd < 2; ++sd) {
    G(queue_gru_side(c, &b->q, gw, sd, b->gru_bias_rows));
    HIPTRY(hipMemsetAsync(ws + w.dxside[sd], 0, (int64_t)BT * d.I * sizeof(float), s));
    const int Dx = d.Is[sd];
    float* dz = ws + w.gcmc_dz[sd];
    float* da = ws + w.gcmc_da[sd];
    G(gemm_mode_call(x3, 1, BT, Dx, 3 * H, ws + w.dxproj[sd], 3 * H, wxcat(c, sd), 3 * H, dz, Dx, nullptr, GF_RELUGRAD, 1.f,
                     reinterpret_cast<const uint8_t*>(ws + w.gcmc_z[sd]), 0, c.scratch, SF, s));
    G(gemm_queue_add(&gq, Dx, Dx, BT, ws + w.gcmc_a[sd], Dx, dz, Dx, gw + P.gm_c[sd], Dx));
    G(gemm_mode_call(x3, 1, BT, Dx, Dx, dz, Dx, W + P.gm_c[sd], Dx, da, Dx, nullptr, GF_RELUGRAD, 1.f,
                     reinterpret_cast<const uint8_t*>(ws + w.gcmc_a[sd]), 0, c.scratch, SF, s));
    G(gemm_queue_add(&gq, Dx, Dx, BT, ws + w.xside[sd], d.I, da, Dx, gw + P.gm_a[sd], Dx));
    G(gemm_mode_call(x3, 1, BT, Dx, Dx, da, Dx, W + P.gm_a[sd], Dx, ws + w.dxside[sd], d.I, nullptr, 0, 1.f, nullptr, 0,
                     c.scratch, SF, s));
  }
  return 0;
}

// ... GRU4Rec: layer 1's input gradient, for the row scatter (layer 2's went to layer 1 in g4r_grus_bwd); "side" 1 of dxside and
// the columns past Di of side 0 carry no gradient
int bwd_dx_g4r(const Pass& c, BwdState* b) {
  const Dims& d = c.d; const WS& w = c.w; float* ws = c.ws; const int H = c.H, BT = c.BT; hipStream_t s = c.s;
  G(queue_gru_side(c, &b->q, b->gw, 0, b->gru_bias_rows));
  HIPTRY(hipMemsetAsync(ws + w.dxside[0], 0, (int64_t)BT * d.I * sizeof(float), s));
  G(gemm_mode_call(c.x3, 1, BT, d.Di, 3 * H, ws + w.dxproj[0], 3 * H, wxcat(c, 0), 3 * H, ws + w.dxside[0], d.I, nullptr, 0, 1.f,
                   nullptr, 0, c.scratch, w.scratch_floats, s));
  G(queue_gru_side(c, &b->q, b->gw, 1, b->gru_bias_rows));
  HIPTRY(hipMemsetAsync(ws + w.dxside[1], 0, (int64_t)BT * d.I * sizeof(float), s));
  return 0;
}

// ---- co-attention + embedding rows (score.py:147-167, 196-201, 51-66), the remaining products and the finishers
int bwd_close(const Pass& c, BwdState* b) {
  const Dims& d = c.d; const Params& P = c.P; const WS& w = c.w; const score_state_t* st = c.st; const score_batch_t* bt = c.bt;
  float* ws = c.ws; const float* W = c.W; float* gw = b->gw; float* grad_table = b->grad_table;
  const int B = c.B, x3 = c.x3; hipStream_t s = c.s;
  void* const* stage_events = b->stage_events;
  SideStream* side = b->side;
  GemmQueue& gq = b->q.gq;
  ColsumJobs& cq = b->q.cq;
  const int64_t half = slab_half(w);
  // The recurrences' weight-gradient products (X^T dY: eight products, K = B*T) need what the backward recurrence has written and
  // nothing else, and nothing inside the pass reads them.  Round 6: issued HERE on the side stream -- behind the head's / attention's
  // products, which end about where the input-gradient product below does -- so the matrix-bound launch runs beside the co-attention
  // backward and the row scatter, which are bound by memory latency / bandwidth and were alone on the chip for ~250 us at cfg-3
  // (profiles/r05_cfg3_sequence.txt), instead of at the END of the launch stream's chain in front of the table's touched-row update
  // (125 us there beside the look-ahead catch-up; 65 us alone).  The join recorded behind them is the one the launch stream waits
  // for behind the scatter (below), so whatever the caller queues next on the launch stream is also behind their last read of the
  // workspace.  The sharded path (scatter_mode 2) keeps the round-5 placement, at the end of the launch stream's chain: its caller
  // runs the gradient exchange on streams of its own beside the scatter (score_amd/dist.py).  So does a pass with nothing queued.
  ReduceGroup rg; rg.n = rg.blocks = 0;
  const bool products_early = st->scatter_mode != 2 && gq.n > 0;
  // ... and with them the finishers of the dense gradient (slab reduce, column sums), when the caller takes them on the side stream
  // (score_state_t.grads_done_event): forked behind target_bwd_kernel, the last launch that feeds them, instead of behind the row
  // scatter -- they ran beside the table's touched-row update, 58 + 28 us there against 20 + 12 alone, with the dense ApplyAdam and
  // through it the next forward pass waiting for them
  const bool fin_side = st->grads_done_event != nullptr;
  const bool fin_early = products_early && fin_side;
  // (the fork HERE, behind the input-gradient product, and not one launch later beside the waits in front of target_bwd_kernel,
  //  where it would cost the launch stream no packet of its own: 872 k vs 884 k samples/s, profiles/r06_probes.md)
  if (products_early) {
    G(fork_side(side, s));
    G(gemm_queue_flush(&gq, x3 != 0, ws + w.dwslab + half, w.dwslab_floats - half, side->st, &rg));
    HIPTRY(hipEventRecord(side->join, side->st));
  }
  EV(3);
  const bool atomic = st->scatter_mode == 1;
  {
    CoattnArgs ca;
    CoattnCols k;
    coattn_args(c, &ca, &k);
    ca.gtable = grad_table;
    ca.all_rows = c.fl.coattn_all_rows ? 1 : 0;      // (debug_flags bit 15: the rows of relu-inactive k are loaded too, A/B)
    ca.meta_ahead = c.fl.coattn_meta_ahead ? 1 : 0;    // (debug_flags bit 16: a unit's ids and scalars requested a unit ahead, A/B)
    for (int i = 0; i < 2; ++i) {
      CoattnCall& cc = ca.c[i];
      cc.g1 = ws + w.dxside[0] + k.col1[i]; cc.g2 = ws + w.dxside[1] + k.col2[i]; cc.ginfo = ws + w.dinfo + k.info_col[i];
      cc.dzsum = ws + w.dzsum[i]; cc.pcoef = ws + w.pcoef[i]; cc.dzcoef = ws + w.dzcoef[i];
    }
    float* dWs[2] = {d.coattn ? gw + P.ca_w[0] : nullptr, d.coattn ? gw + P.ca_w[1] : nullptr};
    if (atomic || d.coattn)   // RCA in pull mode has nothing to prepare: every row gradient is G itself
      G(score_coattn_bwd_multi(ca, 2, d.D, B, dWs, ws + w.ca_slab, w.ca_slab_floats, atomic ? 1 : 0, &cq, s));
  }
  if (d.attn && st->scatter_mode != 2) HIPTRY(hipStreamWaitEvent(s, side->wx, 0));     // d query comes from the side stream
  // (the occurrence sort's event, which the row scatter below needs: waited for HERE, next to the wait above -- every wait or record
  //  between two launches costs the launch stream a bubble of ~6 us, two adjacent ones cost one)
  if (!atomic && st->plan_done_event) HIPTRY(hipStreamWaitEvent(s, (hipEvent_t)st->plan_done_event, 0));
  if (!d.reads_targets) {     // (GCMC reads no target row: their gradient is zero)
    if (!atomic) HIPTRY(hipMemsetAsync(ws + w.dtgt, 0, (int64_t)B * d.Dq * sizeof(float), s));
  } else
  G(score_launch_target_bwd(grad_table, d.D, d.Fu, d.Fi, B, c.T, bt->target_user, bt->target_item,
                            d.attn ? ws + w.dquery : nullptr, d.Dq, ws + w.dhead, d.Dhead, d.off_ti, d.off_tu,
                            ws + w.query, d.coattn ? W + P.ca_w[0] : nullptr, d.coattn ? W + P.ca_w[1] : nullptr,
                            ws + w.dzsum[0], ws + w.dzsum[1], ws + w.S, d.coattn ? gw + P.ca_w[0] : nullptr,
                            d.coattn ? gw + P.ca_b[0] : nullptr, d.coattn ? gw + P.ca_w[1] : nullptr,
                            d.coattn ? gw + P.ca_b[1] : nullptr, atomic ? nullptr : ws + w.dtgt, c.scratch, w.scratch_floats, &cq, &gq,
                            s, st->n_table_rows));
  float* cs_part2 = ws + w.cs_part + w.cs_part_floats / 2;      // the column sums' second half: the first was flushed beside the GRUs
  const int64_t cs_part2_floats = w.cs_part_floats - w.cs_part_floats / 2;
  if (fin_early) {
    G(fork_side(side, s));
    G(score_launch_finish(&rg, &cq, cs_part2, cs_part2_floats, side->st, 0));
    HIPTRY(hipEventRecord((hipEvent_t)st->grads_done_event, side->st));
    HIPTRY(hipEventRecord(side->join, side->st));      // (what the launch stream waits for behind the scatter, below)
  }
  // the plan: in score_state_t.plan_workspace under scatter_mode 0, as the header defines the field
  if (!atomic) G(row_scatter(c, (st->plan_workspace && st->scatter_mode == 0) ? st->plan_workspace : ws, grad_table));
  EV(4);
  // the remaining weight-gradient products of the pass, then the gradients assembled from them
  HIPTRY(hipStreamWaitEvent(s, side->join, 0));
  // The finishers of the dense gradient -- the split-K slab reduce and the column sums: TWO small launches behind the products
  // (score_launch_finish; four dependent ones before round 4, the folded attention layer's gradient among them -- that one now
  // follows the side stream's products, bwd_side_products) -- have ONE consumer, the dense variables' ApplyAdam.  A caller that passes
  // score_state_t.grads_done_event gets them on the side stream (idle by now: the launch stream has just waited for its join)
  // behind the products, and the event recorded behind them: it may run the table's touched-row update, which needs the row
  // gradients only, on the launch stream meanwhile, and waits for the event before anything reads grad_w.
  if (!products_early) G(gemm_queue_flush(&gq, x3 != 0, ws + w.dwslab + half, w.dwslab_floats - half, s, &rg));
  EV(5);
  if (fin_early) return 0;
  if (fin_side) G(fork_side(side, s));
  hipStream_t fs = fin_side ? side->st : s;
  G(score_launch_finish(&rg, &cq, cs_part2, cs_part2_floats, fs, 0));
  if (fin_side) HIPTRY(hipEventRecord((hipEvent_t)st->grads_done_event, fs));
  return 0;
}

int bwd_slice(const Pass& c, BwdState* b) {
  hipStream_t s = c.s;
  void* const* stage_events = b->stage_events;
  G(bwd_open(c, b));
  G(bwd_fc_head(c, b));
  EV(1);
  if (c.d.attn) G(bwd_attention(c, b));
  else G(bwd_final_states(c, b, true));       // RIA, RRN
  EV(2);
  G(bwd_side_products(c, b));
  G(bwd_grus_two_sided(c, b));
  G(bwd_dx_slice(c, b));
  return bwd_close(c, b);
}

int bwd_gcmc(const Pass& c, BwdState* b) {
  const Params& P = c.P; const WS& w = c.w; float* ws = c.ws; const float* W = c.W; const int B = c.B, H = c.H; hipStream_t s = c.s;
  void* const* stage_events = b->stage_events;
  G(bwd_open(c, b));
  // ---- GCMC's head (slice_model.py:199-201): dh_u, dh_i into dfinal, and the rows +-g h_u whose products with h_i are
  // dW4 / dW5 (gcmc.hip)
  G(score_launch_gcmc_head_bwd(B, H, ws + w.gru_final[0], W + P.gm_4, W + P.gm_5, ws + w.gcmc_pn, ws + w.gcmc_pn + (int64_t)B * H,
                               ws + w.gcmc_g, ws + w.dfinal[0], ws + w.dfinal[1], ws + w.gcmc_gu, ws + w.gcmc_gu + (int64_t)B * H, s));
  G(gemm_queue_add(&b->q.gq, H, H, B, ws + w.gru_final[1], H, ws + w.gcmc_gu, H, b->gw + P.gm_4, H));
  G(gemm_queue_add(&b->q.gq, H, H, B, ws + w.gru_final[1], H, ws + w.gcmc_gu + (int64_t)B * H, H, b->gw + P.gm_5, H));
  EV(1);
  G(bwd_final_states(c, b, false));       // (the head kernel wrote dfinal)
  EV(2);
  G(bwd_side_products(c, b));
  G(bwd_grus_two_sided(c, b));
  G(bwd_dx_gcmc(c, b));
  return bwd_close(c, b);
}

int bwd_g4r(const Pass& c, BwdState* b) {
  hipStream_t s = c.s;
  void* const* stage_events = b->stage_events;
  G(bwd_open(c, b));
  G(bwd_fc_head(c, b));
  EV(1);
  // GRU4Rec: the head reads layer 2's final state only; layer 1's dout comes from layer 2's backward
  // (the stacked kernel reads no dout of layer 2; the composed form's kernel does)
  G(bwd_final_state(c, b, 1, 0, !g4r_stacked(c.d, c.fl)));
  G(bwd_zero_dinfo(c));
  EV(2);
  G(bwd_side_products(c, b));
  G(g4r_grus_bwd(c, b->dfinal[1], &b->gru_bias_rows));
  G(bwd_dx_g4r(c, b));
  return bwd_close(c, b);
}

int bwd_caser(const Pass& c, BwdState* b) {
  hipStream_t s = c.s;
  void* const* stage_events = b->stage_events;
  G(bwd_open(c, b));
  G(bwd_fc_head(c, b));
  EV(1);
  G(bwd_zero_dinfo(c));       // (no state: dhead itself is what caser.hip reads)
  EV(2);
  G(bwd_side_products(c, b));
  // Caser: d X into dxside[0] on the launch stream (dxside[1] carries nothing) and, beside it on the side stream -- behind the
  // head's backward since the fork in bwd_side_products, and behind the fill of grad_w --, the six variables' gradients, each
  // batch sum in a fixed order; the join is recorded again behind them
  HIPTRY(hipMemsetAsync(c.ws + c.w.dxside[1], 0, (int64_t)c.BT * c.d.I * sizeof(float), s));
  CaserArgs a;
  caser_args(c, b->gw, &a);
  G(score_caser_bwd(a, s, b->side->st));
  HIPTRY(hipEventRecord(b->side->join, b->side->st));
  return bwd_close(c, b);
}

int bwd_delf(const Pass& c, BwdState* b) {
  hipStream_t s = c.s;
  void* const* stage_events = b->stage_events;
  G(bwd_open(c, b));
  // ---- DELF: the whole backward of the model between the scatter and the loss in ONE launch (delf.hip): dxside, dhead's
  // target columns, and the rows the queued products and column sums are taken from -- those run on the side stream
  // (bwd_side_products), forked behind this launch, beside the target rows' and the embedding rows' scatter
  DelfArgs a;
  delf_args(c, &a);
  G(score_delf_bwd(a, s));
  G(queue_delf(c, &b->q, b->gw));
  EV(1);
  G(bwd_zero_dinfo(c));       // (no state: dhead is what delf.hip wrote)
  EV(2);
  G(bwd_side_products(c, b));       // (no recurrence; delf.hip wrote both dxside above)
  return bwd_close(c, b);
}

int bwd_svdpp(const Pass& c, BwdState* b) {
  hipStream_t s = c.s;
  void* const* stage_events = b->stage_events;
  G(bwd_open(c, b));
  // ---- SVD++: the whole backward between the scatter and the loss in ONE launch (svdpp.hip): dxside[0], dhead's target columns
  // and the weight gradients' per-sample partials, whose batch sums run on the side stream (bwd_side_products); dxside[1] carries
  // nothing
  SvdppArgs a;
  svdpp_args(c, &a);
  G(score_svdpp_bwd(a, s));
  G(queue_svdpp(c, &b->q, b->gw));
  HIPTRY(hipMemsetAsync(c.ws + c.w.dxside[1], 0, (int64_t)c.BT * c.d.I * sizeof(float), s));
  EV(1);
  G(bwd_zero_dinfo(c));       // (no state: dhead is what svdpp.hip wrote)
  EV(2);
  G(bwd_side_products(c, b));
  return bwd_close(c, b);
}

int bwd_sasrec(const Pass& c, BwdState* b) {
  const WS& w = c.w; hipStream_t s = c.s;
  void* const* stage_events = b->stage_events;
  G(bwd_open(c, b));
  SasrecArgs a;
  sasrec_args(c, b->keep_prob, nullptr, nullptr, 0, &a);
  // ---- the shared head from dz2 (the forward pass's last launch left it): through fc2 with fc1's relu / dropout mask per
  // application, folded back onto the rows of z1, through fc1 to the head-input rows
  const int R1 = sasrec_rows1(c), R = sasrec_rows(c, a);
  G(gemm_mode_call(c.x3, 1, R, FC1, FC2, a.dz2, FC2, c.W + c.P.fc_w[1], FC2, a.dz1e, FC1, nullptr, GF_RELUGRAD, b->keep_prob,
                   reinterpret_cast<const uint8_t*>(a.f1), 0, c.scratch, w.scratch_floats, s));
  G(score_sasrec_fold(a, s));
  G(gemm_mode_call(c.x3, 1, R1, a.Dh, FC1, a.dz1, FC1, c.W + c.P.fc_w[0], FC1, a.dhin, a.Dh, nullptr, 0, 1.f, nullptr, 0, c.scratch,
                   w.scratch_floats, s));
  EV(1);
  // ---- residual, A V, softmax, the scaled Q K^T, the three projections and the layer norm in ONE launch (sasrec.hip): dxside[0],
  // dhead's target columns and the rows the queued products and column sums are taken from -- those run on the side stream
  // (bwd_side_products); dxside[1] carries nothing
  G(score_sasrec_attn_bwd(a, s));
  G(queue_sasrec(c, &b->q, b->gw, a));
  HIPTRY(hipMemsetAsync(c.ws + w.dxside[1], 0, (int64_t)c.BT * c.d.I * sizeof(float), s));
  G(bwd_zero_dinfo(c));       // (no state: dhead is what sasrec.hip wrote)
  EV(2);
  G(bwd_side_products(c, b));
  return bwd_close(c, b);
}

int bwd_deems(const Pass& c, BwdState* b) {
  const Dims& d = c.d; const WS& w = c.w; float* ws = c.ws; const int B = c.B, H = c.H, BT = c.BT; hipStream_t s = c.s;
  void* const* stage_events = b->stage_events;
  const int64_t SF = w.scratch_floats;
  G(bwd_open(c, b));
  // ---- both towers' heads: from dz2 (score_forward's fused head left it) to dz1, d bn, d head input in ONE launch (deems.hip)
  DeemsArgs a;
  deems_args(c, b->keep_prob, nullptr, nullptr, 0, &a);
  if (!deems_head_fused(c))
    for (int k = 0; k < 2; ++k)
      G(score_launch_outer_relu_bwd(B, FC2, a.t[k].dlogit, a.t[k].W3, a.t[k].f2, b->keep_prob, a.t[k].dz2, s));
  if (!c.fl.head_unfused) {
    G(score_deems_head_bwd(a, s));
  } else {      // ... or layer by layer, per tower
    for (int k = 0; k < 2; ++k) {
      const DeemsTower& t = a.t[k];
      G(gemm_mode_call(c.x3, 1, B, FC1, FC2, t.dz2, FC2, t.W2, FC2, t.dz1, FC1, nullptr, GF_RELUGRAD, b->keep_prob,
                       reinterpret_cast<const uint8_t*>(t.f1), 0, c.scratch, SF, s));
      G(gemm_mode_call(c.x3, 1, B, t.Dh, FC1, t.dz1, FC1, t.W1, FC1, a.dbn + t.col, a.ld, nullptr, 0, 1.f, nullptr, 0, c.scratch, SF, s));
    }
    G(score_deems_bn_bwd(a, s));
  }
  for (int k = 0; k < 2; ++k) G(queue_head_tower(c, &b->q, b->gw, a, k));
  EV(1);
  // the gradient enters each recurrence through its final state only: the first H columns of its tower's range of dhead
  G(bwd_final_state(c, b, 0, d.off_u, true));
  G(bwd_final_state(c, b, 1, d.off_i, true));
  G(bwd_zero_dinfo(c));
  EV(2);
  G(bwd_side_products(c, b));
  G(deems_grus_bwd(c, b->dfinal, &b->gru_bias_rows));
  // the recurrences' queued weight gradients and d x = [dgates | dcand] . [Wx_gates | Wx_cand]^T into the Is[sd] leading columns of
  // dxside[sd] (the other columns carry no gradient), as RRN's and GRU4Rec's layer 1
  for (int sd = 0; sd < 2; ++sd) {
    G(queue_gru_side(c, &b->q, b->gw, sd, b->gru_bias_rows));
    HIPTRY(hipMemsetAsync(ws + w.dxside[sd], 0, (int64_t)BT * d.I * sizeof(float), s));
    G(gemm_mode_call(c.x3, 1, BT, d.Is[sd], 3 * H, ws + w.dxproj[sd], 3 * H, wxcat(c, sd), 3 * H, ws + w.dxside[sd], d.I, nullptr, 0, 1.f,
                     nullptr, 0, c.scratch, SF, s));
  }
  return bwd_close(c, b);
}
}  // namespace

extern "C" int score_backward(const score_config_t* cfg, const score_state_t* st, const score_batch_t* bt,
                              float keep_prob, float* gw, float* grad_table, void* const* stage_events,
                              void* stream) {
  Pass c;
  SCORE_TRY(make_dims(cfg, &c.d));
  if (!st || !bt || !st->table || !st->w || !st->workspace || !gw || !grad_table || bt->B <= 0)
    return SCORE_E_BADARG;
  if ((c.d.family == FAM_DELF || c.d.family == FAM_DEEMS) && (!bt->length || !bt->length2)) return SCORE_E_BADARG;
  SCORE_TRY(pass_fill(&c, st, bt, stream));
  score_head_forms_begin(1);
  {
    PsPlan pp;
    if (!c.fl.ps_fwd_only && ps_path(c.d, st, bt, c.T, &pp))
      return backward_ps(c, pp, keep_prob, gw, grad_table, stage_events);
  }
  BwdState b;
  b.keep_prob = keep_prob; b.gw = gw; b.grad_table = grad_table; b.stage_events = stage_events;
  b.side = nullptr; b.dfinal[0] = b.dfinal[1] = nullptr; b.gru_bias_rows = 0;
  queues_init(&b.q);
  switch (c.d.family) {
    case FAM_SLICE: return bwd_slice(c, &b);
    case FAM_GCMC: return bwd_gcmc(c, &b);
    case FAM_G4R: return bwd_g4r(c, &b);
    case FAM_CASER: return bwd_caser(c, &b);
    case FAM_DELF: return bwd_delf(c, &b);
    case FAM_DEEMS: return bwd_deems(c, &b);
    case FAM_SVDPP: return bwd_svdpp(c, &b);
    case FAM_SASREC: return bwd_sasrec(c, &b);
  }
  return SCORE_E_BADARG;
}
