// XI pooling (xi-vector): Gaussian posterior inference over the frames of an utterance plus ONE prior pseudo-frame.
//
// Reference semantics: wespeaker/models/pooling_layers.py:380-401 (class XI, stddev=False -- the only form the
// constructors of xi_vector.py build).  Per utterance b and channel d, over the frame window [t0, t0 + n):
//   sp(v)  = v > 20 ? v : log1p(exp(v))                         torch Softplus(beta=1, threshold=20)
//   lp_t   = clamp(2 log(sp(z[t][d])), -15, 15)                 (sp underflows to 0 -> log gives -inf -> clamped to -15)
//   m      = max(max_t lp_t, prior_logprec[d])
//   phi_d  = (sum_t exp(lp_t - m) x[t][d] + exp(prior_logprec[d] - m) prior_mean[d])
//            / (sum_t exp(lp_t - m) + exp(prior_logprec[d] - m))
// x: the frame tensor, z: the output of XI's second 1x1 convolution, both fp32 rows [b*T + t][.] channels-last.
//
// grid = (B, ceil(D / 64)); block = 256 = time groups x channel lanes over 64 channels: 16 groups x 16 lanes of four
// channels (16-byte loads along d) when D, the row strides and the pointers allow it, else 4 groups x 64 lanes of one.
// ONE pass over x and z: a thread walks its frames t = grp, grp + G, ... four at a time (eight independent loads in
// flight), keeps a running maximum and rescales its two sums when the maximum moves (online softmax, one extra exp per
// four frames); the groups' (max, S0, S1) triples meet in LDS and are merged in group order, then the prior joins.
// The order of every sum depends on (t0, n) alone: a row's result does not depend on the batch it is in.
// (built without the packed-fp32 instruction forms, like simam_ops.hip's stem: DESIGN.md 6.0)
#include "kernels.h"

namespace wsamd {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int XI_U = 4;          // frames per thread in flight

// NaN stays NaN (a fmaxf / fminf clamp would turn it into an innocent -15)
__device__ __forceinline__ float xi_logprec(float z) {
  const float sp = z > 20.f ? z : log1pf(expf(z));
  const float lp = 2.f * logf(sp);
  return lp < -15.f ? -15.f : (lp > 15.f ? 15.f : lp);
}

template <int V> struct XiVec;
template <> struct XiVec<4> {
  typedef f32x4 T;
  static __device__ __forceinline__ T load(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
  static __device__ __forceinline__ float get(const T& v, int j) { return v[j]; }
};
template <> struct XiVec<1> {
  typedef float T;
  static __device__ __forceinline__ T load(const float* p) { return *p; }
  static __device__ __forceinline__ float get(const T& v, int) { return v; }
};

template <int V>
__attribute__((target("no-packed-fp32-ops"))) __global__ __launch_bounds__(256) void xi_pool_kernel(const XiPoolParams p) {
  constexpr int LANES = 64 / V, GROUPS = 256 / LANES;
  typedef XiVec<V> VT;
  __shared__ float red[3][GROUPS][64];
  const int b = blockIdx.x;
  const int lane = threadIdx.x % LANES, grp = threadIdx.x / LANES;
  const int cl = lane * V;                                 // first of this thread's V channels within the block's 64
  const int c = blockIdx.y * 64 + cl;
  const bool cok = c < p.D;                                // (V == 4: D % 4 == 0, so the quad is in or out as a whole)
  int t0, n;
  if (p.win) {
    t0 = p.win[2 * b];
    n = p.win[2 * b + 1];
  } else {
    t0 = p.trim;
    n = (p.lens ? p.lens[b] : p.T) - 2 * p.trim;
  }
  const long long row0 = (long long)b * p.T + t0;
  const float* xb = p.x + row0 * p.ldx + (cok ? c : 0);
  const float* zb = p.z + row0 * p.ldz + (cok ? c : 0);
  float m[V], s0[V], s1[V];
#pragma unroll
  for (int j = 0; j < V; ++j) { m[j] = -INFINITY; s0[j] = 0.f; s1[j] = 0.f; }
  for (int t = grp; t < n; t += GROUPS * XI_U) {
    typename VT::T zv[XI_U], xv[XI_U];
#pragma unroll
    for (int u = 0; u < XI_U; ++u) {
      const int tt = t + u * GROUPS;
      const long long r = tt < n ? tt : t;                 // (past the window: re-read frame t, weight 0 below)
      zv[u] = VT::load(zb + r * p.ldz);
      xv[u] = VT::load(xb + r * p.ldx);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float lp[XI_U];
      float cm = m[j];
#pragma unroll
      for (int u = 0; u < XI_U; ++u) {
        lp[u] = t + u * GROUPS < n ? xi_logprec(VT::get(zv[u], j)) : -INFINITY;
        cm = lp[u] > cm ? lp[u] : cm;
      }
      const float r = expf(m[j] - cm);                     // (first chunk: exp(-inf) = 0 times 0)
      float a0 = s0[j] * r, a1 = s1[j] * r;
#pragma unroll
      for (int u = 0; u < XI_U; ++u) {
        const float w = expf(lp[u] - cm);                  // (lp = -inf past the window: 0)
        a0 += w;
        a1 += w * VT::get(xv[u], j);
      }
      // (a NaN logit fails the comparison above, so the maximum ignores it, and reaches both sums through its weight)
      m[j] = cm; s0[j] = a0; s1[j] = a1;
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) {
    red[0][grp][cl + j] = m[j];
    red[1][grp][cl + j] = s0[j];
    red[2][grp][cl + j] = s1[j];
  }
  __syncthreads();
  const int ch = blockIdx.y * 64 + threadIdx.x;
  if (threadIdx.x >= 64 || ch >= p.D) return;
  const float lpr = p.prior_logprec[ch];
  float mx = lpr;
#pragma unroll
  for (int g = 0; g < GROUPS; ++g) mx = red[0][g][threadIdx.x] > mx ? red[0][g][threadIdx.x] : mx;
  float S0 = 0.f, S1 = 0.f;
#pragma unroll
  for (int g = 0; g < GROUPS; ++g) {                       // group order; a group without frames holds (-inf, 0, 0)
    const float r = expf(red[0][g][threadIdx.x] - mx);
    S0 += red[1][g][threadIdx.x] * r;
    S1 += red[2][g][threadIdx.x] * r;
  }
  const float wp = expf(lpr - mx);
  p.pooled[(long long)b * p.ldp + ch] = (S1 + wp * p.prior_mean[ch]) / (S0 + wp);
}

}  // namespace

const char* xi_pool_refusal(const XiPoolParams& p) {
  if (!p.x || !p.z || !p.prior_mean || !p.prior_logprec || !p.pooled) return "null pointer";
  if (p.B < 0 || p.B > 65535) return "batch must be in [0, 65535]";
  if (p.T <= 0 || p.D <= 0) return "T and D must be positive";
  if (p.ldx < p.D || p.ldz < p.D || p.ldp < p.D) return "a row stride is smaller than D";
  if (p.trim < 0) return "trim must not be negative";
  if (!p.win && !p.lens && p.T - 2 * p.trim < 1) return "the window is empty (n >= 1 frames)";
  return nullptr;
}

hipError_t launch_xi_pool(const XiPoolParams& p, hipStream_t stream) {
  if (xi_pool_refusal(p)) return hipErrorInvalidValue;
  if (p.B == 0) return hipSuccess;
  const dim3 grid(p.B, (p.D + 63) / 64);
  const unsigned long long al = reinterpret_cast<unsigned long long>(p.x) | reinterpret_cast<unsigned long long>(p.z);
  const bool vec = ((p.D | p.ldx | p.ldz) & 3) == 0 && (al & 15) == 0;
  if (vec) hipLaunchKernelGGL(xi_pool_kernel<4>, grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL(xi_pool_kernel<1>, grid, dim3(256), 0, stream, p);
  return hipGetLastError();
}

}  // namespace wsamd
