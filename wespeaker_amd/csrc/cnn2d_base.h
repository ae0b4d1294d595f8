// What the 2-D CNN families (ResNet, SimAM-ResNet, ERes2Net, Gemini DF-ResNet) share on the host side, between
// ModelBase and each family's own layout table, block struct, block schedule and taps.
//
// Layout: the (B, T, F) feature tensor is the single-channel (F x T) image; every activation is channels-last
// [b][f][t][c] fp32, so each Conv2d is one implicit GEMM with K = kh*kw*Cin contiguous.  conv -> BN has no
// non-linearity in between, so every BatchNorm2d is folded into its conv's weights + bias on the host (float64).
#pragma once
#include "model_common.h"

namespace wsamd {

struct Cnn2dBase : ModelBase {
  static constexpr int kSplitK = 16;
  size_t stem_w = 0, stem_b = 0;               // ModelBase::pack_stem3x3
  using ModelBase::ModelBase;

  // ---- Activation buffers with a zero pad.  The CONV form of the persistent fp32 GEMM (gemm_f32_stream.hip: 3x3,
  // stride 1, Cin <= 512) reads the border taps of an image from kPad zero floats that lie BEHIND the input tensor's
  // buffer (ConvGemmParams::a_zero_off): whoever hands such a convolution a buffer carves it here and passes
  // zero_off_for().  launch_conv_gemm takes that form only when a_zero_off > 0; every other kernel of the conv-GEMM
  // family reads its out-of-image taps from ConvGemmParams::zeros (ModelBase::zeros_off), which needs no pad.
  struct PaddedBufs {
    enum { kMax = 14, kPad = 512 };
    int n = 0;
    bool bound = false;
    float* ptr[kMax] = {};
    size_t cap[kMax] = {}, off[kMax] = {};     // floats in front of the pad; workspace offset
    float* operator[](int i) const { return ptr[i]; }
    void carve(Carve& cv, size_t cap_floats) {
      cap[n] = cap_floats;
      off[n++] = cv.take(cap_floats + kPad);
    }
    int bind(float* base) {
      for (int i = 0; i < n; ++i) {
        ptr[i] = base + off[i];
        if (hipMemset(ptr[i] + cap[i], 0, kPad * sizeof(float)) != hipSuccess) {
          set_error("zero pad of activation buffer %d", i);
          return WS_ERR_HIP;
        }
      }
      // (hipMemset runs on the null stream, the forwards on the caller's: the pads are zero before reserve() returns)
      if (hipDeviceSynchronize() != hipSuccess) return WS_ERR_HIP;
      bound = true;
      return 0;
    }
    // a_zero_off of a convolution over `in` with Cin input channels: bytes from `in` to its buffer's pad, 0 = no pad
    long long zero_off_for(const float* in, int Cin) const {
      for (int i = 0; i < n; ++i)
        if (in == ptr[i] && Cin <= kPad) return (long long)cap[i] * (long long)sizeof(float);
      return 0;
    }
  } buf;

  //  Nothing may ever store into a pad -- a whole-tile store without a row guard would, and every later image
  // border would be silently wrong: ws_engine_check_range looks (2 KB per buffer device -> host, behind its
  // synchronisation).
  int check_invariants() override {
    if (!buf.bound) return 0;
    std::vector<float> pad(PaddedBufs::kPad);
    for (int i = 0; i < buf.n; ++i) {
      if (hipMemcpy(pad.data(), buf[i] + buf.cap[i], pad.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
        set_error("%s: reading the zero pad of activation buffer %d failed", name.c_str(), i);
        return WS_ERR_HIP;
      }
      for (int k = 0; k < PaddedBufs::kPad; ++k)
        if (pad[k] != 0.f) {
          set_error("%s: the zero pad behind activation buffer %d was overwritten (float %d = %g): a kernel stored "
                    "past its tensor; convolution borders of later forwards are wrong", name.c_str(), i, k, pad[k]);
          return WS_ERR_STATE;
        }
    }
    return 0;
  }

  // ---- The families without a binary16-tensor back-end.  set_precision(2) names the kernels that are fp32 only: a bad
  // argument, WS_ERR_INVALID_ARG.  forward_chunk's guard (never read fp32 buffers as halves) names none: WS_ERR_STATE.
  int no_f16io_backend(const char* what_is_fp32 = nullptr) {
    if (!what_is_fp32) {
      set_error("%s has no binary16-tensor back-end (precision mode 2)", name.c_str());
      return WS_ERR_STATE;
    }
    set_error("%s has no binary16-tensor back-end (precision mode 2): %s fp32; use mode 0 (fp32) or 1 (f16x3)",
              name.c_str(), what_is_fp32);
    return WS_ERR_INVALID_ARG;
  }

  // ---- reserve(): the taps address the old layout.  The family's capacity refusals come next: a refused reserve
  // leaves the previous workspace and buffers in place, so begin_carve() alone forgets the old padded buffers.  The
  // family carves its buffers, and the workspace ends with the seg head's pooled / split-K partials / emb_a and the
  // ragged path's feature copy, in this order.
  void begin_reserve(int max_batch, int max_frames) {
    maxB = max_batch; maxT = max_frames;
    last_chunk = LastChunk();
    block_taps = BlockTaps();
  }
  Carve begin_carve() {
    buf = PaddedBufs();
    return Carve();
  }
  int alloc_with_seg_head(Carve& cv) {
    const size_t o_pool = cv.take((size_t)maxB * 2 * stats_dim), o_part = cv.take((size_t)kSplitK * maxB * embed_dim),
                 o_emba = cv.take((size_t)maxB * embed_dim), o_feats = cv.take((size_t)maxB * maxT * feat_dim);
    if (int err = alloc_workspace(cv.total)) return err;
    float* base = ws.as<float>();
    pooled = base + o_pool; partial = base + o_part; emb_a = base + o_emba; feats_ws = base + o_feats;
    return buf.n ? buf.bind(base) : 0;           // (Gemini has no padded buffers: nothing to zero or to wait for)
  }

  // ---- The embedding head behind TSTP: seg_1 [, seg_bn_1, seg_2]   (resnet.py:187-202, the same in eres2net.py and
  // gemini_dfresnet.py); the family sets stats_dim
  ConvW seg1, seg2;
  bool two_emb = false;
  size_t seg_bn_scale = 0, seg_bn_shift = 0;
  int stats_dim = 0;
  float *pooled = nullptr, *partial = nullptr, *emb_a = nullptr;

  int pack_seg_head(const SD& sd) {
    int err = 0;
    if ((err = pack_linear(sd, "seg_1", embed_dim, 2 * stats_dim, true, &seg1))) return err;
    two_emb = sd.count("seg_2.weight") > 0;
    if (!two_emb) return 0;
    if ((err = add_bn_vectors(sd, "seg_bn_1", embed_dim, &seg_bn_scale, &seg_bn_shift, false))) return err;
    return pack_linear(sd, "seg_2", embed_dim, embed_dim, true, &seg2);
  }
  int run_seg_head(const float* stats, int B, float* emb, hipStream_t st) {
    if (!two_emb) {
      WS_LAUNCH(gemm_splitk(conv1d(seg1, stats, 2 * stats_dim, 0, emb, embed_dim, 0, B, 1, 1, ACT_NONE),
                            partial, kSplitK, st));
    } else {            // embed_b = seg_2(seg_bn_1(relu(seg_1(stats)))): relu -> BN(affine=False) is seg_1's epilogue
      ConvGemmParams a = conv1d(seg1, stats, 2 * stats_dim, 0, emb_a, embed_dim, 0, B, 1, 1, ACT_RELU);
      a.post_scale = arena.at(seg_bn_scale); a.post_shift = arena.at(seg_bn_shift);
      WS_LAUNCH(gemm_splitk(a, partial, kSplitK, st));
      WS_LAUNCH(gemm(conv1d(seg2, emb_a, embed_dim, 0, emb, embed_dim, 0, B, 1, 1, ACT_NONE), st));
    }
    return 0;
  }
  double seg_head_macs() const { return 2.0 * stats_dim * embed_dim + (two_emb ? (double)embed_dim * embed_dim : 0.0); }

  // ---- Stop points and taps.  What a chunk's last executed block left: one block's worth of pointers into the
  // family's buffers (host side only).  forward_chunk fills the notes begin_chunk() hands out; they become readable
  // (last_chunk.B) only when end_chunk() has seen the whole chunk enqueued.
  struct BlockTaps {
    int n_exec = -1;             // blocks the last chunk executed (0: the stem alone; -1: nothing to read)
    bool full = false;           // the chunk ran to its end: the pooling / head tensors exist
    bool half = false;           // the maps exist as binary16 only (f16 back-end)
    const float *stem = nullptr, *block = nullptr, *mid = nullptr, *sc = nullptr, *next_y1 = nullptr;
    int stem_rows = 0, stem_c = 0, rows = 0, block_c = 0, mid_c = 0, next_c = 0, head_rows = 0;
  } block_taps;
  BlockTaps& begin_chunk() {
    last_chunk.B = 0;
    return block_taps = BlockTaps();
  }
  // the chunk is enqueued: a stopped one (ws_debug_engine_stop_after) returns zeros
  int end_chunk(bool full, int B, int T, float* emb, hipStream_t st) {
    block_taps.full = full;
    if (!full)
      if (int r = stop_chunk(emb, B, st)) return r;
    last_chunk.B = B; last_chunk.T = T; last_chunk.prec = gemm_precision;
    return 0;
  }
  int n_stops = 0;                             // finalize(): the stop points behind the stem ...
  std::string stops_are = "residual blocks";   // ... and what they are, for the message
  int set_stop_after(int n) override {
    if (n < -1 || n > n_stops) {
      set_error("ws_debug_engine_stop_after: n_blocks = %d, %s has %d %s (-1 = the full forward, 0 = after the stem)", n,
                name.c_str(), n_stops, stops_are.c_str());
      return WS_ERR_INVALID_ARG;
    }
    stop_after = n;
    return WS_OK;
  }
  // the tail of a full forward: TSTP over the last map x (B x H x W x C; binary16 when the chunk's maps are), the head
  int pool_and_head(const float* x, int C, int B, int H, int W, int lvl, int T, float* emb, hipStream_t st) {
    const bool half = block_taps.half;
    WS_LAUNCH(other((half ? 4.0 : 8.0) * B * H * (double)W * C, st, [&] {
      if (half)
        return launch_tstp_f16(reinterpret_cast<const uint16_t*>(x), C, B, H, W, C, nullptr, nullptr, pooled, st,
                               cur_lens[lvl]);
      return launch_tstp(x, C, B, H, W, C, nullptr, nullptr, pooled, st, cur_lens[lvl]);
    }));
    if (int r = run_seg_head(pooled, B, emb, st)) return r;
    block_taps.head_rows = B;
    return end_chunk(true, B, T, emb, st);
  }

  // a tapped activation map ([b][f][t][c] as rows = B*H*W, cols = C; null: absent, for the reason `why`)
  int tap_map(const char* tname, const float* src, const char* why, int rows_n, int cols_n, float* dst,
              int64_t cap_floats, int32_t* rows, int32_t* cols, hipStream_t st) {
    if (block_taps.half) { src = nullptr; why = "the f16 back-end keeps every activation map in binary16 only"; }
    return tap_copy(tname, src, why, rows_n, cols_n, dst, cap_floats, rows, cols, st);
  }
  // The entries the families share: 'stem' (of a chunk stopped at 0), of the last executed block 'block' (its output),
  // 'mid' (conv1's) and 'sc' (the shortcut convolution's), after a full forward the head's 'pooled' and 'emb_a'.  A
  // family's tap() answers its own names and ends here; TapWords is what differs in the messages.
  struct TapWords {
    const char* names;                   // the family's full name set ("unknown tensor")
    const char* head_why = nullptr;      // why a stopped chunk has no pooled / emb_a (null: the family has its own head)
    const char* sc = "shortcut";         // the family's word for the shortcut convolution (null: no block / mid / sc)
    const char* units = "blocks";        // what its stop points count
  };
  int tap_shared(const char* tname, float* dst, int64_t cap_floats, int32_t* rows, int32_t* cols, hipStream_t st,
                 const TapWords& w) {
    const BlockTaps& t = block_taps;
    const std::string n = tname;
    char why[200];
    if (n == "stem") {
      std::snprintf(why, sizeof(why), "the last forward ran %d %s over the stem's buffer: stop it at 0 "
                    "(ws_debug_engine_stop_after)", t.n_exec, w.units);
      return tap_map(tname, t.n_exec == 0 ? t.stem : nullptr, why, t.stem_rows, t.stem_c, dst, cap_floats, rows, cols, st);
    }
    if (w.sc && (n == "block" || n == "mid" || n == "sc")) {
      if (t.n_exec < 1)
        return tap_map(tname, nullptr, "the last forward was stopped after the stem: no block ran", 0, 0, dst, cap_floats,
                       rows, cols, st);
      std::snprintf(why, sizeof(why), "block %d has no %s convolution", t.n_exec, w.sc);
      if (n == "block") return tap_map(tname, t.block, why, t.rows, t.block_c, dst, cap_floats, rows, cols, st);
      if (n == "mid") return tap_map(tname, t.mid, why, t.rows, t.mid_c, dst, cap_floats, rows, cols, st);
      return tap_map(tname, t.sc, why, t.rows, t.block_c, dst, cap_floats, rows, cols, st);
    }
    if (w.head_why && n == "pooled")
      return tap_copy(tname, t.full ? pooled : nullptr, w.head_why, t.head_rows, 2 * stats_dim, dst, cap_floats, rows,
                      cols, st);
    if (w.head_why && n == "emb_a")
      return tap_copy(tname, !two_emb ? nullptr : (t.full ? emb_a : nullptr),
                      two_emb ? w.head_why : "the model has one embedding layer (no seg_2)", t.head_rows, embed_dim, dst,
                      cap_floats, rows, cols, st);
    set_error("ws_debug_engine_tap: unknown tensor '%s' (%s: %s)", tname, name.c_str(), w.names);
    return WS_ERR_INVALID_ARG;
  }
};

}  // namespace wsamd
