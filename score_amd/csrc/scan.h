// The device builds' prefix sum (graphbuild.hip, targetgen.hip, logremap.hip, ccmr.hip, through devprep.h): reduce-then-scan --
// block sums, one workgroup over the block sums, a second pass --, so no workgroup waits on another and nothing is atomic.
#pragma once
#include "common.h"

namespace {

constexpr int SCAN_T = 256, SCAN_E = 16, SCAN_CHUNK = SCAN_T * SCAN_E, SCAN_TOP_T = 1024;

// out[i] = x[0] + .. + x[i - 1] for i = 0 .. n (n + 1 words), x >= 0: block sums, one workgroup over them, second pass
template <int T>
__device__ __forceinline__ int64_t gb_block_incl_scan(int64_t v, int64_t* s, int tid) {
  s[tid] = v;
  __syncthreads();
  for (int off = 1; off < T; off <<= 1) {
    const int64_t y = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += y;
    __syncthreads();
  }
  const int64_t r = s[tid];
  __syncthreads();                        // (s may be written again by the next call)
  return r;
}

__global__ __launch_bounds__(SCAN_T) void gb_scan_reduce_kernel(const int32_t* __restrict__ x, int64_t n,
                                                               int64_t* __restrict__ bsum) {
  __shared__ int64_t s[SCAN_T];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * SCAN_CHUNK;
  int64_t v = 0;
#pragma unroll
  for (int j = 0; j < SCAN_E; ++j) {
    const int64_t i = base + j * SCAN_T + tid;
    v += i < n ? (int64_t)x[i] : 0;
  }
  const int64_t incl = gb_block_incl_scan<SCAN_T>(v, s, tid);
  if (tid == SCAN_T - 1) bsum[blockIdx.x] = incl;
}

// bsum[b] <- sum of the blocks before b; *total <- the sum of all
__global__ __launch_bounds__(SCAN_TOP_T) void gb_scan_top_kernel(int64_t* __restrict__ bsum, int64_t nb,
                                                                int64_t* __restrict__ total) {
  __shared__ int64_t s[SCAN_TOP_T];
  const int tid = threadIdx.x;
  const int64_t per = (nb + SCAN_TOP_T - 1) / SCAN_TOP_T;
  const int64_t b0 = tid * per, b1 = b0 + per < nb ? b0 + per : nb;
  int64_t v = 0;
  for (int64_t b = b0; b < b1; ++b) v += bsum[b];
  const int64_t incl = gb_block_incl_scan<SCAN_TOP_T>(v, s, tid);
  int64_t run = incl - v;
  for (int64_t b = b0; b < b1; ++b) { const int64_t c = bsum[b]; bsum[b] = run; run += c; }
  if (tid == SCAN_TOP_T - 1) *total = incl;
}

__global__ __launch_bounds__(SCAN_T) void gb_scan_write_kernel(const int32_t* __restrict__ x, int64_t n,
                                                              const int64_t* __restrict__ bsum, int64_t* __restrict__ out) {
  __shared__ int64_t s[SCAN_T];
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * SCAN_CHUNK + (int64_t)tid * SCAN_E;      // SCAN_E consecutive words per thread
  int32_t c[SCAN_E];
  int64_t v = 0;
#pragma unroll
  for (int j = 0; j < SCAN_E; ++j) {
    c[j] = base + j < n ? x[base + j] : 0;
    v += c[j];
  }
  int64_t run = gb_block_incl_scan<SCAN_T>(v, s, tid) - v + bsum[blockIdx.x];
#pragma unroll
  for (int j = 0; j < SCAN_E; ++j) {
    if (base + j < n) out[base + j] = run;
    run += c[j];
  }
}

// out[0 .. n] <- exclusive prefix of x[0 .. n - 1] and the total (out[n]); bsum: cdiv(n, SCAN_CHUNK) words
int gb_scan(const int32_t* x, int64_t n, int64_t* bsum, int64_t* out, hipStream_t s) {
  const int64_t nb = cdiv64(n, SCAN_CHUNK);
  hipLaunchKernelGGL(gb_scan_reduce_kernel, dim3((unsigned)nb), dim3(SCAN_T), 0, s, x, n, bsum);
  SCORE_CHECK_LAUNCH();
  hipLaunchKernelGGL(gb_scan_top_kernel, dim3(1), dim3(SCAN_TOP_T), 0, s, bsum, nb, out + n);
  SCORE_CHECK_LAUNCH();
  hipLaunchKernelGGL(gb_scan_write_kernel, dim3((unsigned)nb), dim3(SCAN_T), 0, s, x, n, bsum, out);
  SCORE_CHECK_LAUNCH();
  return 0;
}

}  // namespace
