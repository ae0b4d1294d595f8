// Non-GEMM kernels of the SimAM-ResNet forward on channels-last fp32 activations.
//
// Reference semantics:
//   stem conv       wespeaker/models/samresnet.py:82-86,118  (Conv2d(1 -> in_planes, 3x3, pad 1) + bn1 + ReLU)
//   SimAM gate      wespeaker/models/samresnet.py:57-70      (between bn2 and the residual add)
//   ASP pooling     wespeaker/models/pooling_layers.py:188-204 (softmax over time, weighted mean / std, clamp 1e-5)
#include "kernels.h"

namespace wsamd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// -------------------------------------------------------------------------------------- stem
// The ResNet stem (cnn_ops.hip) for any channel count C % 4 == 0: the same 8 (f) x 32 (t) pixel tile with the
// 10 x 34 input patch in LDS, the C x 9 weights + C biases in LDS as well; a work item is (tile column, channel quad),
// channel quads fastest, so neighbouring threads store neighbouring 16-byte pieces of one pixel.
// (built without the packed-fp32 instruction forms: hipcc pairs the 4 x 9 multiply-adds into v_pk_fma_f32 with the op_sel
// form the library's build-time ISA check refuses)
constexpr int SS_FH = 8, SS_TW = 32;

__attribute__((target("no-packed-fp32-ops"))) __global__ __launch_bounds__(256) void stem_conv3x3_any_kernel(const float* __restrict__ feats, int T, int F,
                                                               const float* __restrict__ w,
                                                               const float* __restrict__ bias, int C,
                                                               float* __restrict__ out,
                                                               const int* __restrict__ lens) {
  __shared__ float in_s[SS_FH + 2][SS_TW + 2 + 1];
  extern __shared__ float w_s[];               // [C][9] weights, then [C] biases
  const int t0 = blockIdx.x * SS_TW, f0 = blockIdx.y * SS_FH, b = blockIdx.z;
  const int tid = threadIdx.x;
  const float* img = feats + (long long)b * T * F;
  for (int i = tid; i < (SS_FH + 2) * (SS_TW + 2); i += 256) {
    const int tx = i / (SS_FH + 2), fy = i - tx * (SS_FH + 2);   // f fastest: contiguous in feats
    const int tt = t0 + tx - 1, ff = f0 + fy - 1;
    in_s[fy][tx] = (tt >= 0 && tt < T && ff >= 0 && ff < F) ? img[(long long)tt * F + ff] : 0.f;
  }
  for (int i = tid; i < C * 9; i += 256) w_s[i] = w[i];
  for (int i = tid; i < C; i += 256) w_s[C * 9 + i] = bias[i];
  __syncthreads();
  const int q = C >> 2;
  const int len = lens ? lens[b] : T;
  for (int item = tid; item < SS_TW * q; item += 256) {
    const int tx = item / q, c4 = item - tx * q;
    const int t = t0 + tx;
    if (t >= T) continue;
    const bool padded = t >= len;               // ragged batch: columns beyond the utterance stay zero
    float wv[4][9], bv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int k = 0; k < 9; ++k) wv[j][k] = w_s[(c4 * 4 + j) * 9 + k];
      bv[j] = w_s[C * 9 + c4 * 4 + j];
    }
    float col[SS_FH + 2][3];
#pragma unroll
    for (int r = 0; r < SS_FH + 2; ++r)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) col[r][dx] = in_s[r][tx + dx];
#pragma unroll
    for (int fy = 0; fy < SS_FH; ++fy) {
      const int f = f0 + fy;
      if (f >= F) break;
      f32x4 r;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float a = bv[j];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) a += wv[j][dy * 3 + dx] * col[fy + dy][dx];
        r[j] = (padded || a < 0.f) ? 0.f : a;          // (relu_f: NaN stays NaN)
      }
      const long long pix = ((long long)b * F + f) * T + t;
      *reinterpret_cast<f32x4*>(out + pix * C + c4 * 4) = r;
    }
  }
}

hipError_t launch_stem_conv3x3_any(const float* feats, int B, int T, int F, const float* w, const float* b, int C,
                                   float* out, hipStream_t stream, const int* lens) {
  if (C <= 0 || (C & 3) || C > 1024 || B > 65535) return hipErrorInvalidValue;
  if (B <= 0) return hipSuccess;
  dim3 grid((T + SS_TW - 1) / SS_TW, (F + SS_FH - 1) / SS_FH, B);
  hipLaunchKernelGGL(stem_conv3x3_any_kernel, grid, dim3(256), (size_t)C * 10 * sizeof(float), stream, feats, T, F,
                     w, b, C, out, lens);
  return hipGetLastError();
}

// -------------------------------------------------------------------------------------- SimAM
// The activation of utterance b is a (rows = F * T) x C matrix, pixel row r = f * T + t; the columns t >= lens[b] of a
// ragged batch are padding.  A workgroup owns one SLICE of an utterance: 16 * rgroups consecutive pixel rows x all C
// channels, rgroups = 256 / (C / 4) -- thread (rg, c4) holds channels 4 c4 .. +3 of the rows rg + k * rgroups,
// k = 0 .. 15, as 16 independent 16-byte loads (64 KB per workgroup, one pass over memory).
//
// Plane statistics, centred and in a fixed order (same bits on every run and on every lane):
//   stats     per slice and channel: n_i valid rows, their mean m_i, M2_i = sum (x - m_i)^2 from the registers
//             -> part[b][slice][3][C]
//   finalize  per (b, c): N = sum n_i, mean = m_0 + sum n_i (m_i - m_0) / N, M2 = sum M2_i + n_i (m_i - mean)^2
//             (Chan's merge, slices in index order), v = M2 / (N - 1)  -> mu[b][c], 1 / (4 (v + 1e-4))
//   apply     out = relu(x * sigmoid((x - mu)^2 * k + 0.5) + res), zeros in the padding columns
constexpr int SM_RPT = 16;      // rows per thread

int simam_slice_rows(int C) { return (256 / (C >> 2)) * SM_RPT; }
int simam_slices(int rows, int C) { const int s = simam_slice_rows(C); return (rows + s - 1) / s; }

__global__ __launch_bounds__(256) void simam_stats_kernel(const float* __restrict__ y, int rows, int T, int C,
                                                          int rgroups, const int* __restrict__ lens,
                                                          float* __restrict__ part) {
  __shared__ f32x4 s_sum[256];
  __shared__ float s_cnt[64];
  const int q = C >> 2, tid = threadIdx.x;
  const int p = blockIdx.x, P = gridDim.x, b = blockIdx.y;
  const int rg = tid / q, c4 = tid - rg * q;
  const bool act = rg < rgroups;
  const int len = lens ? lens[b] : T;
  const int r0 = p * rgroups * SM_RPT;
  const float* base = y + (long long)b * rows * C + c4 * 4;
  f32x4 v[SM_RPT];
  unsigned mask = 0;
#pragma unroll
  for (int k = 0; k < SM_RPT; ++k) {
    const int r = r0 + rg + k * rgroups;
    const bool ok = act && r < rows && (r % T) < len;
    v[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (ok) {
      v[k] = *reinterpret_cast<const f32x4*>(base + (long long)r * C);
      mask |= 1u << k;
    }
  }
  f32x4 s = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
  s += ((v[8] + v[9]) + (v[10] + v[11])) + ((v[12] + v[13]) + (v[14] + v[15]));
  if (act) {
    s_sum[rg * q + c4] = s;
    if (c4 == 0) s_cnt[rg] = (float)__popc(mask);
  }
  __syncthreads();
  f32x4 tot = (f32x4){0.f, 0.f, 0.f, 0.f};
  float n = 0.f;
  if (act) {
    for (int g = 0; g < rgroups; ++g) {
      tot += s_sum[g * q + c4];
      n += s_cnt[g];
    }
  }
  const float inv_n = n > 0.f ? 1.f / n : 0.f;
  const f32x4 mean = tot * inv_n;
  __syncthreads();
  f32x4 m2 = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < SM_RPT; ++k) {
    if (mask & (1u << k)) {
      const f32x4 d = v[k] - mean;
      m2 += d * d;
    }
  }
  if (act) s_sum[rg * q + c4] = m2;
  __syncthreads();
  if (act && rg == 0) {
    f32x4 M2 = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int g = 0; g < rgroups; ++g) M2 += s_sum[g * q + c4];
    float* o = part + ((long long)b * P + p) * 3 * C + c4 * 4;
    *reinterpret_cast<f32x4*>(o) = (f32x4){n, n, n, n};
    *reinterpret_cast<f32x4*>(o + C) = mean;
    *reinterpret_cast<f32x4*>(o + 2 * C) = M2;
  }
}

__global__ __launch_bounds__(256) void simam_finalize_kernel(const float* __restrict__ part, int P, int C,
                                                             float* __restrict__ mu, float* __restrict__ kk) {
  const int b = blockIdx.x;
  const float* pb = part + (long long)b * P * 3 * C;
  for (int c = threadIdx.x; c < C; c += 256) {
    // (slice 0 always holds valid rows: it starts at pixel row 0, column 0 of the utterance)
    const float m0 = pb[C + c];
    float N = 0.f, S = 0.f;
    for (int p = 0; p < P; ++p) {
      const float n = pb[(long long)p * 3 * C + c];
      N += n;
      S += n * (pb[(long long)p * 3 * C + C + c] - m0);
    }
    const float mean = m0 + S / N;
    float M2 = 0.f;
    for (int p = 0; p < P; ++p) {
      const float n = pb[(long long)p * 3 * C + c];
      const float d = pb[(long long)p * 3 * C + C + c] - mean;
      M2 += pb[(long long)p * 3 * C + 2 * C + c] + n * d * d;
    }
    const float v = M2 / (N - 1.f);
    mu[(long long)b * C + c] = mean;
    kk[(long long)b * C + c] = 1.f / (4.f * (v + 1e-4f));
  }
}

// (y and out may be the same buffer: every element is read and written by the same thread)
__global__ __launch_bounds__(256) void simam_apply_kernel(const float* y, const float* __restrict__ res, int ldr,
                                                          float* out, int rows, int T, int C, int rgroups,
                                                          const int* __restrict__ lens,
                                                          const float* __restrict__ mu,
                                                          const float* __restrict__ kk) {
  const int q = C >> 2, tid = threadIdx.x;
  const int p = blockIdx.x, b = blockIdx.y;
  const int rg = tid / q, c4 = tid - rg * q;
  if (rg >= rgroups) return;
  const int len = lens ? lens[b] : T;
  const int r0 = p * rgroups * SM_RPT;
  const long long img = (long long)b * rows;
  const f32x4 m = *reinterpret_cast<const f32x4*>(mu + (long long)b * C + c4 * 4);
  const f32x4 kq = *reinterpret_cast<const f32x4*>(kk + (long long)b * C + c4 * 4);
  f32x4 xv[SM_RPT], rv[SM_RPT];
#pragma unroll
  for (int k = 0; k < SM_RPT; ++k) {
    const int r = r0 + rg + k * rgroups;
    xv[k] = rv[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (r < rows && (r % T) < len) {
      xv[k] = *reinterpret_cast<const f32x4*>(y + (img + r) * C + c4 * 4);
      rv[k] = *reinterpret_cast<const f32x4*>(res + (img + r) * ldr + c4 * 4);
    }
  }
#pragma unroll
  for (int k = 0; k < SM_RPT; ++k) {
    const int r = r0 + rg + k * rgroups;
    if (r >= rows) continue;
    f32x4 o = (f32x4){0.f, 0.f, 0.f, 0.f};
    if ((r % T) < len) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x = xv[k][j], d = x - m[j];
        const float e = d * d * kq[j] + 0.5f;
        const float sg = 1.f / (1.f + expf(-e));
        o[j] = relu_f(x * sg + rv[k][j]);
      }
    }
    *reinterpret_cast<f32x4*>(out + (img + r) * C + c4 * 4) = o;
  }
}

hipError_t launch_simam_residual_relu(const float* y, const float* res, int ldr, float* out, int B, int F, int T,
                                      int C, const int* lens, float* part, float* mu, float* kk,
                                      hipStream_t stream) {
  if (C < 16 || (C & 3) || C > 1024 || (ldr & 3) || ldr < C || F <= 0 || T <= 0 || B > 65535) return hipErrorInvalidValue;
  if (B <= 0) return hipSuccess;
  const int rows = F * T, rgroups = 256 / (C >> 2), P = simam_slices(rows, C);
  hipLaunchKernelGGL(simam_stats_kernel, dim3(P, B), dim3(256), 0, stream, y, rows, T, C, rgroups, lens, part);
  hipLaunchKernelGGL(simam_finalize_kernel, dim3(B), dim3(256), 0, stream, part, P, C, mu, kk);
  hipLaunchKernelGGL(simam_apply_kernel, dim3(P, B), dim3(256), 0, stream, y, res, ldr, out, rows, T, C, rgroups,
                     lens, mu, kk);
  return hipGetLastError();
}

// -------------------------------------------------------------------------------------- ASP
// x: the last stage, channels-last [(b*F + f)*T + t][C]; e: the attention logits [(b*T + t)][F*C], column f*C + c
// (the model packs the second attention conv's rows in that order, so that both reads are contiguous along c).
// grid = (B*F, ceil(C/64)); block = 256 = 4 time groups x 64 channels; per (b, f, c) over the valid t:
// max, then w = exp(e - max), S0 = sum w, S1 = sum w x, S2 = sum w x^2 -- folded through LDS in group order.
// pooled[b][c*F + f] = S1/S0, pooled[b][C*F + c*F + f] = sqrt(max(S2/S0 - mean^2, 1e-5))   (the reference's order)
__global__ __launch_bounds__(256) void asp_pool_kernel(const float* __restrict__ x, const float* __restrict__ e,
                                                       int F, int T, int C, float* __restrict__ pooled,
                                                       const int* __restrict__ lens) {
  __shared__ float red[3][4][64];
  const int bf = blockIdx.x, b = bf / F, f = bf - b * F;
  const int cl = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + cl;
  const bool cok = c < C;
  const long long D = (long long)F * C;
  const float* xb = x + (long long)bf * T * C + (cok ? c : 0);
  const float* eb = e + (long long)b * T * D + (long long)f * C + (cok ? c : 0);
  const int len = lens ? lens[b] : T;
  float mx = -INFINITY;
  for (int t = grp; t < len; t += 4) mx = fmaxf(mx, eb[(long long)t * D]);
  red[0][grp][cl] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0][0][cl], red[0][1][cl]), fmaxf(red[0][2][cl], red[0][3][cl]));
  __syncthreads();
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int t = grp; t < len; t += 4) {
    const float w = expf(eb[(long long)t * D] - mx);
    const float xv = xb[(long long)t * C];
    s0 += w;
    s1 += w * xv;
    s2 += w * xv * xv;
  }
  red[0][grp][cl] = s0;
  red[1][grp][cl] = s1;
  red[2][grp][cl] = s2;
  __syncthreads();
  if (grp == 0 && cok) {
    s0 = (red[0][0][cl] + red[0][1][cl]) + (red[0][2][cl] + red[0][3][cl]);
    s1 = (red[1][0][cl] + red[1][1][cl]) + (red[1][2][cl] + red[1][3][cl]);
    s2 = (red[2][0][cl] + red[2][1][cl]) + (red[2][2][cl] + red[2][3][cl]);
    const float mean = s1 / s0;
    const float var = s2 / s0 - mean * mean;
    pooled[(long long)b * 2 * D + (long long)c * F + f] = mean;
    pooled[(long long)b * 2 * D + D + (long long)c * F + f] = sqrtf(fmaxf(var, 1e-5f));
  }
}

hipError_t launch_asp_pool(const float* x, const float* e, int B, int F, int T, int C, float* pooled,
                           hipStream_t stream, const int* lens) {
  if (B <= 0) return hipSuccess;
  if (F <= 0 || T <= 0 || C <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(asp_pool_kernel, dim3(B * F, (C + 63) / 64), dim3(256), 0, stream, x, e, F, T, C, pooled, lens);
  return hipGetLastError();
}

}  // namespace wsamd
