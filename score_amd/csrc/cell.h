// The pointwise arithmetic every recurrence and head kernel shares, written once: the tests pin the fused, per-sample,
// stacked, bf16x3, streaming and layer-by-layer forms against each other, which holds only while all of them round alike.
// One-expression helpers that return a value: inlined, they are the expressions the kernels used to spell out.
#pragma once
#include "common.h"

// fast transcendental forms for the recurrence epilogues (v_exp_f32 / v_rcp_f32; abs error ~1e-7).  NOT sigmoidf_ / tanhf,
// the correctly rounded forms of gru_fwd_kernel, the stepwise kernels and the heads.  A probe build may define
// SCORE_GRU_RCP before the include (__frcp_rn: the ten-instruction correctly rounded division).
#ifndef SCORE_GRU_RCP
#define SCORE_GRU_RCP(x) __builtin_amdgcn_rcpf(x)  // v_rcp_f32 (1 ulp)
#endif
__device__ __forceinline__ float gru_sigmoid(float x) { return SCORE_GRU_RCP(1.0f + __expf(-x)); }
__device__ __forceinline__ float gru_tanh(float x) { return 1.0f - 2.0f * SCORE_GRU_RCP(__expf(2.0f * x) + 1.0f); }
// GRUCell's new state h' = u*h + (1-u)*c
__device__ __forceinline__ float gru_blend(float u, float h, float c) { return u * h + (1.0f - u) * c; }
// backward, pre-activation gradients of a step with d = dL/dh': du = d*(h_prev - c), dc = d*(1-u);
// dpu = du*u*(1-u), dpc = dc*(1-c^2), dpr = d(rh)*h_prev*r*(1-r); 0 past the length (live == false).
// The state update (d*u, d(rh)*r) stays with the caller.  A call site forms dc and du first, then dpu and dpc: in that
// order the compiler schedules the kernels as it did when they were tuned and measured (profiles/kernel_helpers_isa.txt).
__device__ __forceinline__ float gru_du(float d, float hp, float c) { return d * (hp - c); }
__device__ __forceinline__ float gru_dc(float d, float u) { return d * (1.0f - u); }
__device__ __forceinline__ float gru_dpu(float du, float u, bool live) { return live ? du * u * (1.0f - u) : 0.f; }
__device__ __forceinline__ float gru_dpc(float dc, float c, bool live) { return live ? dc * (1.0f - c * c) : 0.f; }
__device__ __forceinline__ float gru_dpr(float drh, float hp, float r, bool live) {
  return live ? drh * hp * r * (1.0f - r) : 0.f;
}

// dense(activation=relu) + tf.nn.dropout (x / keep * Bernoulli(keep)) of element (row, col) of an [., N] layer: the
// element numbering is the GEMM epilogue's (kernels.h), so a fused kernel drops what the layer-by-layer path drops.
// `row` must be a row of the layer (< B): an explicit mask is exactly [B, N] bytes, so a kernel that computes the rows of a
// ragged 16-row tile past the batch hands in min(row, B - 1) -- what it computes for those rows is never stored
__device__ __forceinline__ float relu_dropout(float v, float bias, int drop, float keep, const uint8_t* mask, uint64_t seed,
                                              int row, int col, int N) {
  v = fmaxf(v + bias, 0.f);
  if (drop) {
    const uint64_t e = (uint64_t)row * (uint64_t)N + (uint64_t)col;
    const bool on = mask ? (mask[e] != 0) : (hash_uniform(seed, e) < keep);
    v = on ? v / keep : 0.f;
  }
  return v;
}

// the sigmoid heads' log-loss terms (score.py:74-81) of a sample with prediction p and label lab:
// loss_b = -y log(p+eps) - (1-y) log(1-p+eps) ; dlogit = dloss/dp * p(1-p) / B
#define SCORE_LOGLOSS_EPS 1e-7f
__device__ __forceinline__ float logloss_term(float p, float lab) {
  return -lab * logf(p + SCORE_LOGLOSS_EPS) - (1.0f - lab) * logf(1.0f - p + SCORE_LOGLOSS_EPS);
}
__device__ __forceinline__ float logloss_dlogit(float p, float lab, int Bglobal) {
  return (-lab / (p + SCORE_LOGLOSS_EPS) + (1.0f - lab) / (1.0f - p + SCORE_LOGLOSS_EPS)) / (float)Bglobal * p * (1.0f - p);
}
