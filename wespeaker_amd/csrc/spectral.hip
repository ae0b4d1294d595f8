// Spectral clustering of sub-segment embeddings on gfx950: the n-sized half of
//   wespeaker/diar/spectral_clusterer.py:33-87   cluster(): affinity, prune, Laplacian, eigh
// (the k-means on the n x k spectral embedding and the b x b algebra stay on the host in float64,
// wespeaker_amd/diar.py).
//
// Stages ("Spectral clustering"):
//   a. graph      unit rows + exact-fp32 MFMA cosine matrix (score.hip / conv_gemm.hip), then per row the
//                 keep-th largest value by the shared radix select and the kept set as a bitmask
//                 (spectral_clusterer.py:39-50; 0.5 * (1 + cos) is monotone and never materialised)
//   b. symmetrise M = (P + P^T) / 2 with a zero diagonal (:51, :54) as CSR (int32 offsets from a device
//                 prefix sum, ascending int32 columns, values 0.5 / 1 as double) and deg = row sums (:55)
//   c. operator   Y = alpha * (L X) + beta * X + gamma * Z,  L X = deg (.) X - M X   (:56, never formed)
//   d. gram pair  G = X^T X and H = X^T (L X) with a fixed reduction order (no floating-point atomics)
//   e. rotate     out = X W + gamma * Z   (the Rayleigh-Ritz basis update, and the residual panel)
// L is sparse (a row keeps ~10 - 80 of up to 8192 neighbours), so c is a gather bound by L2 bandwidth and by
// launch latency: one wavefront per row, lane = column of the n x b panel, every neighbour's panel row is one
// coalesced read of b doubles.  No MFMA: there is no dense tile to feed one.
#include "kernels.h"
#include "radix_select.h"

namespace wsamd {

namespace {
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
}  // namespace

// ------------------------------------------------------------------------------- a. pruning mask
// One workgroup per affinity row.  words = ceil(n / 32) <= 256 (n <= SPECTRAL_MAX_N).  Exactly `keep`
// bits are set per row (0 < keep < n); ties at the threshold go to the higher column (radix_select.h).
__global__ __launch_bounds__(256) void spectral_mask_kernel(
    const float* __restrict__ S, int ld, int n, int keep, int words, uint32_t* __restrict__ mask) {
  __shared__ RadixSelectShared sel;
  __shared__ uint32_t gt[256], eq[256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int i = blockIdx.x;
  const float* row = S + (long long)i * ld;
  const bool none = keep <= 0, all = keep >= n;
  uint32_t thr_key = 0;
  unsigned ties = 0;
  if (!none && !all) radix_select_row(row, n, keep, sel, &thr_key, &ties);
  gt[tid] = 0;
  eq[tid] = 0;
  __syncthreads();
  for (int c0 = wave * 64; c0 < words * 32; c0 += 256) {
    const int col = c0 + lane;
    const bool in = col < n;
    const uint32_t key = f2key(in ? row[col] : 0.f);
    const bool g = in && !none && (all || key > thr_key);
    const bool e = in && !none && !all && key == thr_key;
    const unsigned long long bg = __ballot(g), be = __ballot(e);
    if (lane == 0) {
      const int w = c0 >> 5;
      gt[w] = (uint32_t)bg;
      eq[w] = (uint32_t)be;
      if (w + 1 < words) {
        gt[w + 1] = (uint32_t)(bg >> 32);
        eq[w + 1] = (uint32_t)(be >> 32);
      }
    }
  }
  __syncthreads();
  if (tid == 0) {                            // `ties` copies of the threshold, highest columns first
    unsigned rem = ties;
    for (int w = words - 1; w >= 0; --w) {
      uint32_t e = eq[w];
      if (!e) continue;
      uint32_t k = 0;
      while (e && rem) {
        const uint32_t top = 1u << (31 - __clz((int)e));
        k |= top;
        e &= ~top;
        --rem;
      }
      eq[w] = k;
    }
  }
  __syncthreads();
  if (tid < words) mask[(long long)i * words + tid] = gt[tid] | eq[tid];
}

// maskT[i][w] bit j = mask[32 w + j][i >> 5] bit (i & 31): the 32 x 32 bit tiles transposed, two tiles per
// wavefront (one per 32-lane half), 32 ballots per pair.
__global__ __launch_bounds__(256) void spectral_transpose_kernel(
    const uint32_t* __restrict__ mask, int n, int words, uint32_t* __restrict__ maskT) {
  const int lane = threadIdx.x & 63, half = lane >> 5, l = lane & 31;
  const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long t = 2 * g + half, tiles = (long long)words * words;
  const bool valid = t < tiles;
  const int tr = valid ? (int)(t / words) : 0, tc = valid ? (int)(t % words) : 0;
  const int r = 32 * tr + l;
  const uint32_t x = (valid && r < n) ? mask[(long long)r * words + tc] : 0u;
  uint32_t out = 0;
#pragma unroll
  for (int b = 0; b < 32; ++b) {
    const unsigned long long m = __ballot((x >> b) & 1u);
    if (l == b) out = (uint32_t)(m >> (32 * half));
  }
  const int dst = 32 * tc + l;
  if (valid && dst < n) maskT[(long long)dst * words + tr] = out;
}

// ------------------------------------------------------------------------------- b. symmetrise -> CSR
// One wavefront per row: count[i] = |{j != i : P_ij or P_ji}|.
__global__ __launch_bounds__(256) void spectral_count_kernel(
    const uint32_t* __restrict__ mask, const uint32_t* __restrict__ maskT, int n, int words,
    int32_t* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  int c = 0;
  for (int w = lane; w < words; w += 64) {
    uint32_t a = mask[(long long)i * words + w] | maskT[(long long)i * words + w];
    if (w == (i >> 5)) a &= ~(1u << (i & 31));
    c += __popc(a);
  }
  c = wave_sum_i32(c);
  if (lane == 0) count[i] = c;
}

// Exclusive prefix sum of n <= 8192 counts by one workgroup: 32 consecutive rows per thread.
__global__ __launch_bounds__(256) void spectral_scan_kernel(const int32_t* __restrict__ count, int n,
                                                            int32_t* __restrict__ rowptr) {
  __shared__ int part[256];
  const int tid = threadIdx.x;
  const int per = (n + 255) / 256;           // <= 32
  const int r0 = tid * per;
  int s = 0;
  for (int r = r0; r < r0 + per && r < n; ++r) s += count[r];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < 256; ++t) { const int v = part[t]; part[t] = run; run += v; }
    rowptr[n] = run;
  }
  __syncthreads();
  int run = part[tid];
  for (int r = r0; r < r0 + per && r < n; ++r) { rowptr[r] = run; run += count[r]; }
}

// One wavefront per row: columns ascending (word order, then bit order), value 1 where both P_ij and P_ji,
// 0.5 where one of them; deg[i] = sum of the row's values (multiples of 0.5: exact in any order).
__global__ __launch_bounds__(256) void spectral_fill_kernel(
    const uint32_t* __restrict__ mask, const uint32_t* __restrict__ maskT, int n, int words,
    const int32_t* __restrict__ rowptr, long long cap, int32_t* __restrict__ colidx,
    double* __restrict__ vals, double* __restrict__ deg) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const long long base = rowptr[i];
  int running = 0;
  double d = 0.0;
  for (int w0 = 0; w0 < words; w0 += 64) {
    const int w = w0 + lane;
    uint32_t r = 0, t = 0;
    if (w < words) {
      r = mask[(long long)i * words + w];
      t = maskT[(long long)i * words + w];
    }
    uint32_t a = r | t;
    if (w == (i >> 5)) a &= ~(1u << (i & 31));
    const uint32_t both = r & t;
    const int c = __popc(a);
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    long long pos = base + running + (incl - c);
    while (a) {
      const int bit = __ffs((int)a) - 1;
      a &= a - 1;
      const double v = ((both >> bit) & 1u) ? 1.0 : 0.5;
      if (pos < cap) {
        colidx[pos] = 32 * w + bit;
        vals[pos] = v;
      }
      ++pos;
      d += v;
    }
    running += __shfl(incl, 63, 64);
  }
  d = wave_sum_f64(d);
  if (lane == 0) deg[i] = d;
}

// Debug: L = diag(deg) - M into a zeroed n x n double matrix.
__global__ __launch_bounds__(256) void spectral_dense_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
    const double* __restrict__ vals, const double* __restrict__ deg, int n, double* __restrict__ L) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int k0 = rowptr[i], k1 = rowptr[i + 1];
  for (int k = k0 + lane; k < k1; k += 64) {
    const int c = colidx[k];
    if (c >= 0 && c < n) L[(long long)i * n + c] = -vals[k];
  }
  if (lane == 0) L[(long long)i * n + i] = deg[i];
}

// ------------------------------------------------------------------------------- c. operator
// Y = alpha * (deg (.) X - M X) + beta * X + gamma * Z on n x b row-major panels, b <= 64.  One wavefront per
// row, lane = column; the neighbour list is wave-uniform.  The sum over neighbours runs in CSR order, so the
// result is reproducible.  Y may alias Z (each lane reads and writes its own element) but not X.
__global__ __launch_bounds__(256) void spectral_apply_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
    const double* __restrict__ vals, const double* __restrict__ deg, int n, int b, double alpha,
    double beta, double gamma, const double* __restrict__ X, const double* Z, double* Y) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n || lane >= b) return;
  const int k0 = rowptr[i], k1 = rowptr[i + 1];
  double acc = 0.0;
  for (int k = k0; k < k1; ++k) acc += vals[k] * X[(long long)colidx[k] * b + lane];
  const long long o = (long long)i * b + lane;
  const double x = X[o];
  double y = alpha * (deg[i] * x - acc) + beta * x;
  if (gamma != 0.0) y += gamma * Z[o];
  Y[o] = y;
}

// ------------------------------------------------------------------------------- d. gram pair
// Workgroup g folds the 32-row chunks g, g + G, g + 2G, ... (G = gridDim.x) in that order into one padded
// 64 x 64 partial of X^T X and of X^T (LX); spectral_gram_fold_kernel then adds the G partials in index
// order.  The order depends on (n, b) alone, so two runs give the same bits.
#define SPECTRAL_GRAM_ROWS 32
__global__ __launch_bounds__(256) void spectral_gram_partial_kernel(
    const double* __restrict__ X, const double* __restrict__ LX, int n, int b,
    double* __restrict__ part) {
  __shared__ double xs[SPECTRAL_GRAM_ROWS][64], ls[SPECTRAL_GRAM_ROWS][64];
  const int tid = threadIdx.x, q = tid & 63, pg = tid >> 6;
  double g[16], h[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) g[i] = h[i] = 0.0;
  const int nchunks = (n + SPECTRAL_GRAM_ROWS - 1) / SPECTRAL_GRAM_ROWS;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int r0 = c * SPECTRAL_GRAM_ROWS;
    __syncthreads();
    for (int e = tid; e < SPECTRAL_GRAM_ROWS * 64; e += 256) {
      const int r = e >> 6, cc = e & 63;
      double v = 0.0, w = 0.0;
      if (r0 + r < n && cc < b) {
        v = X[(long long)(r0 + r) * b + cc];
        w = LX[(long long)(r0 + r) * b + cc];
      }
      xs[r][cc] = v;
      ls[r][cc] = w;
    }
    __syncthreads();
    for (int r = 0; r < SPECTRAL_GRAM_ROWS; ++r) {
      const double xq = xs[r][q], lq = ls[r][q];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const double xp = xs[r][pg + 4 * i];   // wave-uniform address: an LDS broadcast
        g[i] += xp * xq;
        h[i] += xp * lq;
      }
    }
  }
  double* pgm = part + (long long)blockIdx.x * 2 * 4096;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = pg + 4 * i;
    pgm[p * 64 + q] = g[i];
    pgm[4096 + p * 64 + q] = h[i];
  }
}

__global__ __launch_bounds__(256) void spectral_gram_fold_kernel(
    const double* __restrict__ part, int nparts, int b, double* __restrict__ G,
    double* __restrict__ H) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= b * b) return;
  const int p = e / b, q = e % b;
  double g = 0.0, h = 0.0;
  for (int k = 0; k < nparts; ++k) {
    g += part[(long long)k * 2 * 4096 + p * 64 + q];
    h += part[(long long)k * 2 * 4096 + 4096 + p * 64 + q];
  }
  G[e] = g;
  H[e] = h;
}

// ------------------------------------------------------------------------------- e. basis update
// out = X W + gamma * Z, W b x b row-major in LDS, one wavefront per row: the row is read into registers
// in full before anything is written, so out may be X (in place) or Z.
__global__ __launch_bounds__(256) void spectral_rotate_kernel(
    const double* X, const double* __restrict__ W, double gamma, const double* Z, double* out, int n,
    int b) {
  __shared__ double ws[64 * 64];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int e = tid; e < 64 * 64; e += 256) {
    const int p = e >> 6, q = e & 63;
    ws[e] = (p < b && q < b) ? W[p * b + q] : 0.0;
  }
  __syncthreads();
  for (int i = blockIdx.x * 4 + (tid >> 6); i < n; i += gridDim.x * 4) {
    const long long o = (long long)i * b + lane;
    const double x = lane < b ? X[o] : 0.0;
    const double z = (gamma != 0.0 && lane < b) ? Z[o] : 0.0;
    double acc = 0.0;
    for (int p = 0; p < b; ++p) acc += __shfl(x, p, 64) * ws[p * 64 + lane];
    if (lane < b) out[o] = acc + gamma * z;
  }
}

// ------------------------------------------------------------------------------- launchers
hipError_t launch_spectral_mask(const float* S, int ld, int n, int keep, uint32_t* mask,
                                uint32_t* maskT, hipStream_t stream) {
  if (n <= 0 || n > SPECTRAL_MAX_N || ld < n || (ld & 3)) return hipErrorInvalidValue;
  const int words = (n + 31) / 32;
  hipLaunchKernelGGL(spectral_mask_kernel, dim3(n), dim3(256), 0, stream, S, ld, n, keep, words, mask);
  const long long waves = ((long long)words * words + 1) / 2;
  hipLaunchKernelGGL(spectral_transpose_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream,
                     mask, n, words, maskT);
  return hipGetLastError();
}

hipError_t launch_spectral_csr(const uint32_t* mask, const uint32_t* maskT, int n, int32_t* count,
                               int32_t* rowptr, long long cap, int32_t* colidx, double* vals,
                               double* deg, hipStream_t stream) {
  if (n <= 0 || n > SPECTRAL_MAX_N || cap < 0) return hipErrorInvalidValue;
  const int words = (n + 31) / 32;
  const dim3 grid((n + 3) / 4), block(256);
  hipLaunchKernelGGL(spectral_count_kernel, grid, block, 0, stream, mask, maskT, n, words, count);
  hipLaunchKernelGGL(spectral_scan_kernel, dim3(1), block, 0, stream, count, n, rowptr);
  hipLaunchKernelGGL(spectral_fill_kernel, grid, block, 0, stream, mask, maskT, n, words, rowptr, cap,
                     colidx, vals, deg);
  return hipGetLastError();
}

hipError_t launch_spectral_dense(const int32_t* rowptr, const int32_t* colidx, const double* vals,
                                 const double* deg, int n, double* L, hipStream_t stream) {
  if (n <= 0 || n > SPECTRAL_MAX_N) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(L, 0, sizeof(double) * (size_t)n * n, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(spectral_dense_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, rowptr, colidx,
                     vals, deg, n, L);
  return hipGetLastError();
}

hipError_t launch_spectral_apply(const int32_t* rowptr, const int32_t* colidx, const double* vals,
                                 const double* deg, int n, int b, double alpha, double beta,
                                 double gamma, const double* X, const double* Z, double* Y,
                                 hipStream_t stream) {
  if (n <= 0 || b <= 0 || b > SPECTRAL_MAX_B) return hipErrorInvalidValue;
  hipLaunchKernelGGL(spectral_apply_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, rowptr, colidx,
                     vals, deg, n, b, alpha, beta, gamma, X, Z, Y);
  return hipGetLastError();
}

int spectral_gram_parts(int n) {
  const int nchunks = (n + SPECTRAL_GRAM_ROWS - 1) / SPECTRAL_GRAM_ROWS;
  return nchunks < 64 ? nchunks : 64;
}

hipError_t launch_spectral_gram(const double* X, const double* LX, int n, int b, double* G, double* H,
                                double* part, hipStream_t stream) {
  if (n <= 0 || b <= 0 || b > SPECTRAL_MAX_B) return hipErrorInvalidValue;
  const int parts = spectral_gram_parts(n);
  hipLaunchKernelGGL(spectral_gram_partial_kernel, dim3(parts), dim3(256), 0, stream, X, LX, n, b, part);
  hipLaunchKernelGGL(spectral_gram_fold_kernel, dim3((b * b + 255) / 256), dim3(256), 0, stream, part,
                     parts, b, G, H);
  return hipGetLastError();
}

hipError_t launch_spectral_rotate(const double* X, const double* W, double gamma, const double* Z,
                                  double* out, int n, int b, hipStream_t stream) {
  if (n <= 0 || b <= 0 || b > SPECTRAL_MAX_B) return hipErrorInvalidValue;
  int grid = (n + 3) / 4;
  if (grid > 256) grid = 256;
  hipLaunchKernelGGL(spectral_rotate_kernel, dim3(grid), dim3(256), 0, stream, X, W, gamma, Z, out, n, b);
  return hipGetLastError();
}

}  // namespace wsamd
