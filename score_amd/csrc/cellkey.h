// The device builds' counter-based draw (graphbuild.hip, targetgen.hip; graph._cell_keys on the host), uint64, wrapping:
//   key(seed, tag, c, j) = mix(mix(seed + G * ((tag << 40) + c + 1)) + G * (j + 1)) >> 32, mix = the finaliser of hash_uniform.
#pragma once
#include "common.h"

namespace {

constexpr uint64_t GB_G = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t gb_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t gb_cell_hash(uint64_t seed, uint64_t tag, uint64_t c) {
  return gb_mix(seed + GB_G * ((tag << 40) + c + 1ull));
}
__device__ __forceinline__ uint32_t gb_key(uint64_t cell_hash, uint64_t j) {
  return (uint32_t)(gb_mix(cell_hash + GB_G * (j + 1ull)) >> 32);
}

}  // namespace
