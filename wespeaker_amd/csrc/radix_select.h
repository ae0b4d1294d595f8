// Exact k-th largest of one float row by a 4-pass most-significant-byte radix select, shared by the
// AS-norm cohort statistics (score.hip, topn_stats_kernel) and the spectral clusterer's pruning
// (spectral.hip, spectral_mask_kernel).  Device code only; one 256-thread workgroup per row.
//
// Ties at the threshold.  The select returns (thr_key, ties): every entry whose key is > thr_key is
// strictly inside the k largest, and `ties` copies of thr_key complete them (1 <= ties <= number of
// entries equal to the threshold).  A caller that needs only sums (topn_stats_kernel) adds ties *
// threshold; a caller that needs the SET (spectral_mask_kernel) keeps exactly k entries and, among
// equal values, the HIGHER column index wins -- the tail of a stable ascending argsort, which is what
// `np.argsort(row)[n:]` of spectral_clusterer.py:47-48 selects.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wsamd {

typedef float radix_f32x4 __attribute__((ext_vector_type(4)));

// Order-preserving map float -> uint32 (larger float <=> larger key; -0 < +0 is harmless here).
__device__ __forceinline__ uint32_t f2key(float v) {
  const uint32_t b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
  const uint32_t b = k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu);
  return __uint_as_float(b);
}

// Shared state of one select: one histogram per wavefront (4x fewer collisions) and the running
// (prefix, remaining) pair.
struct RadixSelectShared {
  unsigned hist[4][256];
  unsigned prefix, remaining;
};

// Called by all 256 threads of the workgroup.  row: n_cols floats, 16-byte aligned; 1 <= k < n_cols.
// On return *thr_key / *ties are as described above (the same values in every thread).
__device__ __forceinline__ void radix_select_row(const float* __restrict__ row, int n_cols, int k,
                                                 RadixSelectShared& sh, uint32_t* thr_key,
                                                 unsigned* ties) {
  const int tid = threadIdx.x, wave = tid >> 6;
  const int nvec = n_cols >> 2;
  const radix_f32x4* row4 = reinterpret_cast<const radix_f32x4*>(row);
  if (tid == 0) { sh.prefix = 0; sh.remaining = (unsigned)k; }
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    for (int i = tid; i < 4 * 256; i += 256) (&sh.hist[0][0])[i] = 0;
    __syncthreads();
    const uint32_t prefix = sh.prefix;
    auto vote = [&](float v) {
      const uint32_t key = f2key(v);
      if (pass == 0 || (key >> (shift + 8)) == prefix)
        atomicAdd(&sh.hist[wave][(key >> shift) & 255], 1u);
    };
    for (int i = tid; i < nvec; i += 256) {
      const radix_f32x4 v = row4[i];
      vote(v[0]); vote(v[1]); vote(v[2]); vote(v[3]);
    }
    for (int i = nvec * 4 + tid; i < n_cols; i += 256) vote(row[i]);
    __syncthreads();
    // bins from the top: find the one where the running count reaches `remaining`
    if (wave == 0) {
      const int lane = tid;
      // lane l owns bins 255-4l .. 252-4l (descending order)
      unsigned c[4], tot = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int b = 255 - (4 * lane + q);
        c[q] = sh.hist[0][b] + sh.hist[1][b] + sh.hist[2][b] + sh.hist[3][b];
        tot += c[q];
      }
      unsigned incl = tot;                 // inclusive prefix sum over lanes
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      const unsigned rem = sh.remaining;
      unsigned before = incl - tot;        // entries in strictly higher bins
      if (before < rem && incl >= rem) {   // exactly one lane
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (before < rem && before + c[q] >= rem) {
            sh.prefix = (prefix << 8) | (unsigned)(255 - (4 * lane + q));
            sh.remaining = rem - before;
            before = rem;                  // stop
          } else {
            before += c[q];
          }
        }
      }
    }
    __syncthreads();
  }
  *thr_key = sh.prefix;
  *ties = sh.remaining;
}

}  // namespace wsamd
