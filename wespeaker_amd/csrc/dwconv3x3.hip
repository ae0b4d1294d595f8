// Depthwise 3x3 convolution + folded BatchNorm + ReLU on channels-last maps: the middle of Gemini DF-ResNet's
// inverted-bottleneck block (wespeaker/models/gemini_dfresnet.py:35-44: Conv2d(4 dim, 4 dim, 3, padding 1,
// groups = 4 dim) -> bn2 -> relu).
//
//   out[b,f,t,c] = relu( sum_{df,dt in -1..1} x[b,f+df,t+dt,c] * w[c][3 (df+1) + (dt+1)] + bias[c] )
//
// over rows x[((b*F + f)*T + t)][C], zero padding on both axes, stride 1; w / bias carry bn2 (folded on the host in
// float64).  There is no reduction over channels, so this is VALU work: 9 FMAs per output against 8 bytes of compulsory
// traffic -- the kernel is bound by memory, not arithmetic, and is laid out for that:
//
//   * a thread owns 4 channels (one 16-byte access along C) and DW_TT = 4 consecutive time steps, and walks DOWN the
//     frequency axis: the three input lines an output line needs live in registers (3 x 6 float4) and each step loads
//     ONE new line, so an input element is loaded once per walk (plus the two halo columns of the time tile, which the
//     neighbouring lanes of the same wave load in the same instruction: L1 / L2 hits, not HBM);
//   * consecutive lanes take consecutive channel quads, then consecutive time tiles: a wave's load is 1 KiB in
//     contiguous pieces of 16 C bytes;
//   * the 36 weights and 4 biases of the thread's channels stay in registers for the whole walk;
//   * the frequency axis is cut into walks of `fchunk` lines (grid.y) only when a whole-column walk would leave the
//     chip short of threads; a cut costs two halo lines per walk.
//
// Every output is the same chain of 9 FMAs in the same order wherever it lies (a tap outside the image, or at
// t >= row_len[b], enters as the value 0 by a select, never by skipping it or by multiplying what memory holds there):
// a row of a ragged batch is bit for bit its batch-of-one result, whatever the padding columns contain.
#include <cstdio>

#include "kernels.h"

namespace wsamd {

namespace {

constexpr int DW_TT = 4;          // time steps per thread
constexpr int DW_BLOCK = 256;

struct DwLine { float4 v[DW_TT + 2]; };

__device__ __forceinline__ void dw_load_line(DwLine& ln, const float* __restrict__ x, long long img, int f, int F, int T,
                                             int C, int t0, int tlim, int c0) {
  const bool fin = f >= 0 && f < F;
  const float* row = x + ((img * F + (fin ? f : 0)) * (long long)T) * C + c0;
#pragma unroll
  for (int j = 0; j < DW_TT + 2; ++j) {
    const int t = t0 - 1 + j;
    ln.v[j] = (fin && t >= 0 && t < tlim) ? *reinterpret_cast<const float4*>(row + (long long)t * C)
                                          : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

__device__ __forceinline__ float dw_get(const float4& v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }

// one output line from its three input lines
__device__ __forceinline__ void dw_out_line(const DwLine& a, const DwLine& b, const DwLine& c, const float (&w)[36],
                                            const float4& bias, float* __restrict__ out, long long img, int f, int F, int T,
                                            int C, int t0, int tlim, int c0) {
  float* row = out + ((img * F + f) * (long long)T) * C + c0;
#pragma unroll
  for (int j = 0; j < DW_TT; ++j) {
    const int t = t0 + j;
    float r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float acc = 0.f;
#pragma unroll
      for (int dt = 0; dt < 3; ++dt) acc = fmaf(dw_get(a.v[j + dt], i), w[i * 9 + dt], acc);
#pragma unroll
      for (int dt = 0; dt < 3; ++dt) acc = fmaf(dw_get(b.v[j + dt], i), w[i * 9 + 3 + dt], acc);
#pragma unroll
      for (int dt = 0; dt < 3; ++dt) acc = fmaf(dw_get(c.v[j + dt], i), w[i * 9 + 6 + dt], acc);
      r[i] = relu_f(acc + dw_get(bias, i));
    }
    if (t < T) {
      const bool live = t < tlim;            // columns at or beyond row_len[b]: exact zeros
      *reinterpret_cast<float4*>(row + (long long)t * C) =
          live ? make_float4(r[0], r[1], r[2], r[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
}

__global__ __launch_bounds__(DW_BLOCK) void dwconv3x3_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                             const float* __restrict__ w, const float* __restrict__ bias,
                                                             int B, int F, int T, int C, const int* __restrict__ row_len,
                                                             int fchunk, long long n_threads) {
  const long long gid = (long long)blockIdx.x * DW_BLOCK + threadIdx.x;
  if (gid >= n_threads) return;
  const int cq_n = C >> 2, tt_n = (T + DW_TT - 1) / DW_TT;
  const int cq = (int)(gid % cq_n);
  const long long rest = gid / cq_n;
  const int tt = (int)(rest % tt_n);
  const long long img = rest / tt_n;                       // < B by n_threads
  const int c0 = cq * 4, t0 = tt * DW_TT;
  int tlim = T;
  if (row_len) {
    const int L = row_len[img];
    tlim = L < 0 ? 0 : (L < T ? L : T);
  }
  const int f_begin = blockIdx.y * fchunk;
  const int f_end = f_begin + fchunk < F ? f_begin + fchunk : F;
  // the thread's 4 x 9 weights are 36 consecutive floats (16-byte aligned: c0 * 9 * 4 = 144 cq bytes)
  float wr[36];
  {
    const float4* wp = reinterpret_cast<const float4*>(w + (long long)c0 * 9);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float4 q = wp[k];
      wr[4 * k] = q.x; wr[4 * k + 1] = q.y; wr[4 * k + 2] = q.z; wr[4 * k + 3] = q.w;
    }
  }
  const float4 bs = *reinterpret_cast<const float4*>(bias + c0);
  DwLine l0, l1, l2;                                        // lines f - 1, f, f + 1, rotating through the three names
  dw_load_line(l0, x, img, f_begin - 1, F, T, C, t0, tlim, c0);
  dw_load_line(l1, x, img, f_begin, F, T, C, t0, tlim, c0);
  for (int f = f_begin; f < f_end; f += 3) {
    dw_load_line(l2, x, img, f + 1, F, T, C, t0, tlim, c0);
    dw_out_line(l0, l1, l2, wr, bs, out, img, f, F, T, C, t0, tlim, c0);
    if (f + 1 >= f_end) break;
    dw_load_line(l0, x, img, f + 2, F, T, C, t0, tlim, c0);
    dw_out_line(l1, l2, l0, wr, bs, out, img, f + 1, F, T, C, t0, tlim, c0);
    if (f + 2 >= f_end) break;
    dw_load_line(l1, x, img, f + 3, F, T, C, t0, tlim, c0);
    dw_out_line(l2, l0, l1, wr, bs, out, img, f + 2, F, T, C, t0, tlim, c0);
  }
}

}  // namespace

const char* dwconv3x3_refusal(const DwConv3x3Params& p) {
  if (!p.x || !p.out || !p.w || !p.bias) return "a null pointer among x / out / w / bias";
  if (p.B < 1 || p.F < 1 || p.T < 1) return "B, F and T must be at least 1";
  if (p.C < 4 || p.C % 4) return "C must be a positive multiple of 4";
  const long long n = (long long)p.B * p.F * p.T * p.C;
  if (n >= (1LL << 31)) return "the map has 2^31 elements or more";
  if ((reinterpret_cast<unsigned long long>(p.x) | reinterpret_cast<unsigned long long>(p.out) |
       reinterpret_cast<unsigned long long>(p.w) | reinterpret_cast<unsigned long long>(p.bias)) & 15)
    return "pointers must be 16-byte aligned";
  if (p.out < p.x + n && p.x < p.out + n) return "out aliases x";
  return nullptr;
}

bool dwconv3x3_supported(const DwConv3x3Params& p) { return dwconv3x3_refusal(p) == nullptr; }

hipError_t launch_dwconv3x3(const DwConv3x3Params& p, hipStream_t stream) {
  if (!dwconv3x3_supported(p)) return hipErrorInvalidValue;
  const long long n_threads = (long long)p.B * ((p.T + DW_TT - 1) / DW_TT) * (p.C / 4);
  // whole-column walks when they fill the chip four workgroups deep; otherwise walks of 8 lines
  const long long fill = (long long)current_device_cus() * 4 * DW_BLOCK;
  const int fchunk = n_threads >= fill || p.F <= 8 ? p.F : 8;
  const int fy = (p.F + fchunk - 1) / fchunk;
  const long long blocks = (n_threads + DW_BLOCK - 1) / DW_BLOCK;
  if (dispatch_log_enabled()) {
    char key[160];
    snprintf(key, sizeof(key), "rows=%lld C=%d F=%d walk=%d%s -> dwconv3x3_kernel (depthwise 3x3 + bias + ReLU)",
             (long long)p.B * p.F * p.T, p.C, p.F, fchunk, p.row_len ? " +mask" : "");
    dispatch_log_note_text(key);
  }
  hipLaunchKernelGGL(dwconv3x3_kernel, dim3((unsigned)blocks, (unsigned)fy), dim3(DW_BLOCK), 0, stream, p.x, p.out, p.w,
                     p.bias, p.B, p.F, p.T, p.C, p.row_len, fchunk, n_threads);
  return hipGetLastError();
}

}  // namespace wsamd
