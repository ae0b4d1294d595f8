// Attentional feature fusion of ERes2Net (wespeaker/models/eres2net.py:75-103) as ONE launch over channels-last rows:
//   h   = silu(W1' [x[m] | y[m]] + b1')          W1': [C/4][ldw1 >= 2C]  (1x1 conv bias + eval BatchNorm folded on the host)
//   a   = 1 + tanh(W2' h + b2')                  W2': [C][ldw2 >= C/4]
//   out = x[m] * a + y[m] * (2 - a)
// Built from the tile launchers this is a concat copy, two GEMM launches and an element-wise pass: five trips over
// tensors whose compulsory traffic is "read two, write one".  Here a workgroup of four wavefronts owns 32 pixels:
//   * phase 1: the hidden vector, in chunks of 128 rows (32 per wavefront, one 32x32 accumulator block each).  The
//     [x | y] concat is only an address: K-tile kt < C/32 comes from x, the others from y.  The K-tiles of the pixels
//     [32][32] and of W1' [128][32] go through LDS (registers one tile ahead); v_mfma_f32_32x32x2_f32 with A = weights,
//     B = pixels gives C^T blocks -- a lane owns four consecutive channels of ONE pixel.  Both operands are read as
//     16-byte pieces: lane half lh reads columns 8q + 4lh .. + 3, k-step 4q + e pairs the channels 8q + e and
//     8q + 4 + e (the same permutation on both sides, so the contraction is unchanged).  bias + SiLU, then the chunk
//     is written to the LDS plane Hs[32 pixels][C/4 rounded up to 32]: h never leaves the chip.
//   * phase 2: the gate, in chunks of 128 output channels, K = C/4 from Hs; the x / y values of the blend are
//     requested before the K loop (a second read of the rows phase 1 streamed, served by L2), the result is stored
//     once as 16-byte pieces.
// A C > 512 needs more than one hidden chunk and re-streams the pixel rows per chunk (L2 again; HBM sees x and y once).
// Rows beyond C/4 of the last hidden chunk are zero weights with a zero bias: silu(0) = 0, and W2's columns there are
// zero-filled as well.  Pixels beyond M are loaded as zeros and not stored.  A pixel is one MFMA column: whatever a
// padding pixel holds (NaN included) stays in its own column, and with row_len it is stored as exact zeros.
#include "kernels.h"
#include <cstdio>

namespace wsamd {

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int AF_PX = 32;       // pixels per workgroup
constexpr int AF_ROWS = 128;    // weight rows per chunk (32 per wavefront)
constexpr int AF_S = 36;        // floats per LDS row of a K-tile (144 B: 16-byte aligned, spreads the banks)

__device__ __forceinline__ float silu_f(float v) { return v / (1.f + expf(-v)); }

__global__ __launch_bounds__(256) void aff_fuse_kernel(const AffFuseParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int C = p.C, H = C >> 2, Hp = (H + 31) & ~31, HS = Hp + 4;
  float* const Ws = lds;                          // [128][36]
  float* const Xs = Ws + AF_ROWS * AF_S;          // [32][36]
  float* const Hs = Xs + AF_PX * AF_S;            // [32][HS]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int m0 = blockIdx.x * AF_PX;
  // staging roles: thread (row t >> 3 (+ 32 i), 16-byte piece t & 7)
  const int srow = tid >> 3, sc4 = (tid & 7) * 4;
  const int sm = m0 + srow;                       // the pixel this thread stages
  const bool sm_ok = sm < p.M;
  const float* const xrow = p.x + (long long)(sm_ok ? sm : 0) * p.ldx + p.x_off + sc4;
  const float* const yrow = p.y + (long long)(sm_ok ? sm : 0) * p.ldy + p.y_off + sc4;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 wreg[4], xreg;

  // K-tile kt of weight rows [n0, n0 + 128) of W[rows][ldw] (rows >= nrows and columns >= ncols are zeros)
  auto load_w = [&](const float* W, int ldw, int nrows, int ncols, int n0, int kt) {
    const int k = kt * 32 + sc4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = n0 + srow + 32 * i;
      wreg[i] = (n < nrows && k < ncols) ? *reinterpret_cast<const f32x4*>(W + (long long)n * ldw + k) : zero4;
    }
  };
  auto load_xy = [&](int kt) {
    const int k = kt * 32;
    xreg = !sm_ok ? zero4 : (k < C ? *reinterpret_cast<const f32x4*>(xrow + k)
                                   : *reinterpret_cast<const f32x4*>(yrow + (k - C)));
  };
  auto store_w = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(&Ws[(srow + 32 * i) * AF_S + sc4]) = wreg[i];
  };
  const float* const wfrag = Ws + (wave * 32 + li) * AF_S + 4 * lh;
  // 16 k-steps of one staged K-tile: A = this wavefront's 32 weight rows, B = 32 pixels at brow (row stride bs)
  auto mfma_tile = [&](f32x16& acc, const float* brow) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(wfrag + 8 * q);
      const f32x4 b = *reinterpret_cast<const f32x4*>(brow + 8 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc, 0, 0, 0);
    }
  };

  // ---------------------------------------------------------------- phase 1: Hs = silu(W1 [x | y] + b1)
  const int kt1 = 2 * C / 32;
  for (int h0 = 0; h0 < Hp; h0 += AF_ROWS) {
    const int r0 = h0 + wave * 32;                // this wavefront's hidden rows
    const bool active = r0 < Hp;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    load_w(p.W1, p.ldw1, H, 2 * C, h0, 0);
    load_xy(0);
    for (int kt = 0; kt < kt1; ++kt) {
      store_w();
      *reinterpret_cast<f32x4*>(&Xs[srow * AF_S + sc4]) = xreg;
      __syncthreads();
      if (kt + 1 < kt1) {
        load_w(p.W1, p.ldw1, H, 2 * C, h0, kt + 1);
        load_xy(kt + 1);
      }
      if (active) mfma_tile(acc, Xs + li * AF_S + 4 * lh);
      __syncthreads();
    }
    if (active) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int r = r0 + 8 * g + 4 * lh;        // rows r .. r + 3 (H % 4 == 0: all inside or all beyond)
        f32x4 v = zero4;
        if (r < H) {
          const f32x4 b = *reinterpret_cast<const f32x4*>(p.b1 + r);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = silu_f(acc[4 * g + e] + b[e]);
        }
        *reinterpret_cast<f32x4*>(&Hs[li * HS + r]) = v;
      }
    }
  }
  // (the first barrier of phase 2's K loop orders these Hs stores before its reads)

  // ---------------------------------------------------------------- phase 2: out = x a + y (2 - a), a = 1 + tanh(W2 h + b2)
  const int m = m0 + li;
  const bool m_ok = m < p.M;
  bool padded = false;
  if (p.row_len && m_ok) {
    const int img = m / p.HW, rem = m - img * p.HW;
    padded = rem - (rem / p.W) * p.W >= p.row_len[img];
  }
  const int kt2 = Hp / 32;
  for (int c0 = 0; c0 < C; c0 += AF_ROWS) {
    const int cw = c0 + wave * 32;                // this wavefront's output channels
    const bool active = cw < C;
    f32x4 xv[4], yv[4];
    if (active && m_ok) {
      const float* xp = p.x + (long long)m * p.ldx + p.x_off + cw + 4 * lh;
      const float* yp = p.y + (long long)m * p.ldy + p.y_off + cw + 4 * lh;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        xv[g] = *reinterpret_cast<const f32x4*>(xp + 8 * g);
        yv[g] = *reinterpret_cast<const f32x4*>(yp + 8 * g);
      }
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    load_w(p.W2, p.ldw2, C, H, c0, 0);
    for (int kt = 0; kt < kt2; ++kt) {
      store_w();
      __syncthreads();
      if (kt + 1 < kt2) load_w(p.W2, p.ldw2, C, H, c0, kt + 1);
      if (active) mfma_tile(acc, Hs + li * HS + kt * 32 + 4 * lh);
      __syncthreads();
    }
    if (active && m_ok) {
      float* op = p.out + (long long)m * p.ldo + p.o_off + cw + 4 * lh;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(p.b2 + cw + 8 * g + 4 * lh);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a = 1.f + tanhf(acc[4 * g + e] + b[e]);
          o[e] = xv[g][e] * a + yv[g][e] * (2.f - a);
        }
        if (padded) o = zero4;                    // ragged batch: columns beyond the utterance stay exact zeros
        *reinterpret_cast<f32x4*>(op + 8 * g) = o;
      }
    }
  }
}

// the floats [ptr + off, ..) of M rows of C columns at row stride ld share an element with those of another operand
bool rows_overlap(const float* a, int lda, int a_off, const float* b, int ldb, int b_off, int M, int C) {
  const float* a0 = a + a_off;
  const float* b0 = b + b_off;
  const float* a1 = a0 + (long long)(M - 1) * lda + C;
  const float* b1 = b0 + (long long)(M - 1) * ldb + C;
  if (a1 <= b0 || b1 <= a0) return false;
  if (lda != ldb) return true;
  // the same row stride: column windows of one interleaved buffer are disjoint when they do not meet modulo ld
  long long d = (b0 - a0) % lda;
  if (d < 0) d += lda;
  return !(d >= C && d + C <= lda);
}
}  // namespace

const char* aff_fuse_refusal(const AffFuseParams& p) {
  if (!p.x || !p.y || !p.out || !p.W1 || !p.b1 || !p.W2 || !p.b2) return "a null pointer among x / y / out / W1 / b1 / W2 / b2";
  if (p.M <= 0) return "M must be positive";
  if (p.C < 64 || p.C > 2048 || p.C % 32) return "C must be a multiple of 32 in [64, 2048]";
  if ((p.ldx | p.x_off | p.ldy | p.y_off | p.ldo | p.o_off | p.ldw1 | p.ldw2) & 3)
    return "row strides and channel offsets must be multiples of 4 floats";
  if (p.ldw1 < 2 * p.C || p.ldw2 < p.C / 4) return "a weight row stride is shorter than its row (ldw1 >= 2C, ldw2 >= C/4)";
  if (p.x_off < 0 || p.y_off < 0 || p.o_off < 0 || p.ldx < p.x_off + p.C || p.ldy < p.y_off + p.C || p.ldo < p.o_off + p.C)
    return "a row stride is shorter than its channel offset + C";
  if ((reinterpret_cast<unsigned long long>(p.x) | reinterpret_cast<unsigned long long>(p.y) |
       reinterpret_cast<unsigned long long>(p.out) | reinterpret_cast<unsigned long long>(p.W1) |
       reinterpret_cast<unsigned long long>(p.b1) | reinterpret_cast<unsigned long long>(p.W2) |
       reinterpret_cast<unsigned long long>(p.b2)) & 15)
    return "pointers must be 16-byte aligned";
  if (rows_overlap(p.out, p.ldo, p.o_off, p.x, p.ldx, p.x_off, p.M, p.C)) return "out aliases x";
  if (rows_overlap(p.out, p.ldo, p.o_off, p.y, p.ldy, p.y_off, p.M, p.C)) return "out aliases y";
  if (p.row_len && (p.HW <= 0 || p.W <= 0 || p.HW % p.W || p.M % p.HW))
    return "row_len needs whole images: HW a multiple of W, M a multiple of HW";
  return nullptr;
}

bool aff_fuse_supported(const AffFuseParams& p) { return aff_fuse_refusal(p) == nullptr; }

hipError_t launch_aff_fuse(const AffFuseParams& p, hipStream_t stream) {
  if (!aff_fuse_supported(p)) return hipErrorInvalidValue;
  const int Hp = ((p.C >> 2) + 31) & ~31;
  const size_t lds = (size_t)(AF_ROWS * AF_S + AF_PX * AF_S + AF_PX * (Hp + 4)) * sizeof(float);
  static size_t lds_granted[WS_MAX_DEVICES] = {};
  if (lds > 64 * 1024) {
    hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(aff_fuse_kernel), lds, lds_granted);
    if (e != hipSuccess) return e;
  }
  if (dispatch_log_enabled()) {
    char key[160];
    snprintf(key, sizeof(key), "rows=%d C=%d%s -> aff_fuse_kernel (1x1 + SiLU + 1x1 + tanh gate + blend)", p.M, p.C,
             p.row_len ? " +mask" : "");
    dispatch_log_note_text(key);
  }
  hipLaunchKernelGGL(aff_fuse_kernel, dim3((unsigned)((p.M + AF_PX - 1) / AF_PX)), dim3(256), lds, stream, p);
  return hipGetLastError();
}

}  // namespace wsamd
