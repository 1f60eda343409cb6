// lcx_snapshot_kernels.hpp -- the checksum of a snapshot section, computed where the section lives (include/lcx_state.h).
//
// checksum64 of csrc/lcx_snapshot_format.hpp: the sum modulo 2^64 over the 8-byte words w_i of mix64(w_i + (i + 1) * GOLDEN).  The sum
// is of integers, so any order gives the same bits: a grid-stride pass in which a lane loads 16 bytes (two words) per trip, a butterfly
// inside the wave, one partial per workgroup written by a plain store, and a second launch of one workgroup that folds the partials.
// No float, no atomics.  The pass is bound by the reads from HBM: the grid is capped at eight workgroups of 256 per CU and strides.
#ifndef LCX_SNAPSHOT_KERNELS_HPP
#define LCX_SNAPSHOT_KERNELS_HPP

#include <hip/hip_runtime.h>
#include "lcx_snapshot_format.hpp"

namespace lcx {

constexpr int CKS_BS = 256, CKS_MAX_BLOCKS = 2048;

__device__ __forceinline__ uint64_t cks_mix(uint64_t z)
{
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint64_t cks_wave_sum(uint64_t v)
{
  for (int d = 32; d > 0; d >>= 1) v += (unsigned long long)__shfl_xor((unsigned long long)v, d);
  return v;
}
// sums the lanes of a workgroup of CKS_BS; the result is valid in thread 0
__device__ __forceinline__ uint64_t cks_block_sum(uint64_t v)
{
  __shared__ uint64_t part[CKS_BS / 64];
  v = cks_wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t s = 0;
  if (threadIdx.x == 0) for (int w = 0; w < CKS_BS / 64; ++w) s += part[w];
  return s;
}
// data: 16-byte aligned (a device allocation).  partial[gridDim.x]
__global__ void __launch_bounds__(CKS_BS) k_checksum64(const unsigned char *data, size_t bytes, uint64_t *partial)
{
  const size_t n16 = bytes / 16;
  const ulonglong2 *v = reinterpret_cast<const ulonglong2 *>(data);
  uint64_t sum = 0;
  for (size_t i = size_t(blockIdx.x) * CKS_BS + threadIdx.x; i < n16; i += size_t(gridDim.x) * CKS_BS) {
    const ulonglong2 w = v[i];
    sum += cks_mix(w.x + (2 * i + 1) * snap::GOLDEN) + cks_mix(w.y + (2 * i + 2) * snap::GOLDEN);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {       // the last 0 .. 15 bytes: at most two words, the second padded with zeros
    const size_t done = n16 * 16;
    for (size_t k = 0; done + 8 * k < bytes; ++k) {
      uint64_t w = 0;
      for (size_t b = 0; b < 8 && done + 8 * k + b < bytes; ++b) w |= uint64_t(data[done + 8 * k + b]) << (8 * b);
      sum += cks_mix(w + (2 * n16 + k + 1) * snap::GOLDEN);
    }
  }
  sum = cks_block_sum(sum);
  if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}
__global__ void __launch_bounds__(CKS_BS) k_checksum64_fold(const uint64_t *partial, unsigned n, uint64_t *out)
{
  uint64_t sum = 0;
  for (unsigned i = threadIdx.x; i < n; i += CKS_BS) sum += partial[i];
  sum = cks_block_sum(sum);
  if (threadIdx.x == 0) *out = sum;
}
static inline unsigned cks_blocks(size_t bytes)
{
  const size_t want = (bytes / 16 + CKS_BS - 1) / CKS_BS;
  return unsigned(want < 1 ? 1 : want > size_t(CKS_MAX_BLOCKS) ? size_t(CKS_MAX_BLOCKS) : want);
}

}  // namespace lcx
#endif
