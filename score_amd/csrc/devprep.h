// What the device data builds share (pointhist.hip, graphbuild.hip, targetgen.hip, logremap.hip, ccmr.hip): the launch shape and
// grid-stride loop, key widths, the lower bound over sorted keys, a zero fill, the carving of a caller's workspace, the sort's
// ping-pong and the read-back of a few words with its wait.
#pragma once
#include <atomic>
#include "common.h"
#include "scan.h"

#define DP_THREADS 256
#define DP_LOOP(i, n) for (int64_t i = (int64_t)blockIdx.x * DP_THREADS + threadIdx.x; i < (n); i += (int64_t)gridDim.x * DP_THREADS)

namespace {

template <class T>                 // (a template: only a file that launches it carries its code)
__global__ __launch_bounds__(DP_THREADS) void dp_zero_kernel(T* __restrict__ x, int64_t n) {
  DP_LOOP(i, n) x[i] = 0;
}

// first position of the sorted keys whose (key >> shift) is >= c
__device__ __forceinline__ int64_t dp_lower_bound(const uint32_t* __restrict__ keys, int64_t n, int shift, uint32_t c) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((keys[mid] >> shift) < c) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int64_t dp_lower_bound(const uint32_t* __restrict__ keys, int64_t n, uint32_t c) {
  return dp_lower_bound(keys, n, 0, c);
}

int dp_bits_of(uint32_t x) {       // bits that hold the values 0 .. x
  int b = 1;
  while (b < 32 && (x >> b)) ++b;
  return b;
}

unsigned dp_grid(int64_t n) {      // workgroups of DP_THREADS for a DP_LOOP over n
  const int64_t g = cdiv64(n > 0 ? n : 1, DP_THREADS);
  return (unsigned)(g < 65536 ? g : 65536);
}

// keys and values of a sort with their alternates and score_sort_pairs' temp
struct SortBufs { uint32_t* k0; uint32_t* v0; uint32_t* k1; uint32_t* v1; void* sort_temp; int64_t sort_bytes; };

// Hands out a workspace front to back.  With a null base it only adds up (`off` is then the size to ask the caller for) and
// every pointer it returns is null: a pointer is only ever formed from a real base.
struct Carver {
  char* base; int64_t off;
  explicit Carver(void* temp) : base(static_cast<char*>(temp)), off(0) {}
  template <class T> T* take(int64_t count, int64_t align_words) {
    const int64_t at = off;
    off += align_up64(count, align_words) * (int64_t)sizeof(T);
    T* p = base ? reinterpret_cast<T*>(base + at) : nullptr;
#ifdef DP_CARVE_SEEN                   // (tools/devprep_carve_check.hip looks at every range)
    DP_CARVE_SEEN(p, off - at);
#endif
    return p;
  }
  template <class T> T* words(int64_t n) { return take<T>(n, 64); }             // n 32-bit words, 256-byte granules
  int64_t* prefix(int64_t n) { return take<int64_t>(n + 1, 32); }              // gb_scan's out for n inputs
  int64_t* block_sums(int64_t n) { return take<int64_t>(cdiv64(n, SCAN_CHUNK) + 1, 32); }      // gb_scan's bsum
  void scan(int32_t*& x, int64_t*& idx, int64_t*& bsum, int64_t n) { x = words<int32_t>(n); idx = prefix(n); bsum = block_sums(n); }
  void sort_pairs(SortBufs& b, int64_t n) {
    b.k0 = words<uint32_t>(n); b.v0 = words<uint32_t>(n); b.k1 = words<uint32_t>(n); b.v1 = words<uint32_t>(n);
  }
  void sort_temp(SortBufs& b, int64_t n) {                                      // (n == 0: no sort, no temp)
    b.sort_bytes = n > 0 ? score_sort_pairs_temp_bytes(n) : 0;
    b.sort_temp = take<char>(b.sort_bytes, 1);
  }
};

// stable sort of (k0, v0)[0 .. n) by the low key_bits; the result is in k0 / v0 and the scratch in k1 / v1, whatever the
// number of passes
int dp_sort(SortBufs& b, int64_t n, int key_bits, hipStream_t s) {
  int32_t in_alt = 0;
  SCORE_TRY(score_sort_pairs(b.k0, b.v0, b.k1, b.v1, n, key_bits, b.sort_temp, b.sort_bytes, &in_alt, s));
  if (in_alt) { uint32_t* x = b.k0; b.k0 = b.k1; b.k1 = x; x = b.v0; b.v0 = b.v1; b.v1 = x; }
  return 0;
}

// host[0 .. n) <- dev[0 .. n) and a wait for the stream; `counter` (may be null) counts the waits
int dp_read_words(const int64_t* dev, int64_t* host, int n, hipStream_t s, std::atomic<int>* counter) {
  if (counter) counter->fetch_add(1, std::memory_order_relaxed);
  hipError_t e = hipMemcpyAsync(host, dev, sizeof(int64_t) * n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return e == hipSuccess ? 0 : (int)e;
}

}  // namespace
