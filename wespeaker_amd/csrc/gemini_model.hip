// Gemini DF-ResNet60/114/183/237 speaker-embedding forward scheduled onto the gfx950 kernels.
//
// Reference (file:line in wenet-e2e/wespeaker):
//   wespeaker/models/gemini_dfresnet.py:30-48    Inverted_Bottleneck (1x1 dim -> 4 dim, depthwise 3x3, 1x1 4 dim -> dim,
//                                                 each with its BatchNorm; += x; relu)
//   wespeaker/models/gemini_dfresnet.py:51-141   Gemini_DF_ResNet (stem, four strided 3x3 downsample layers WITHOUT an
//                                                 activation, four stages, TSTP, seg_1 [, seg_bn_1, seg_2])
//   wespeaker/models/gemini_dfresnet.py:145-178  the four constructors (depths; dims 32, 32, 64, 128, 256)
//   wespeaker/models/pooling_layers.py:78-85     TSTP
//
// Layout, BN folding, the seg_1 / seg_2 head and the shared taps: cnn2d_base.h (its zero-padded buffers are not used,
// see small_buf).  The frequency axis is halved by every downsample layer, the time axis by the second one only ("T14c"
// strides (2,1) (2,2) (2,1) (2,1)); both follow (n - 1) / 2 + 1.  The reference sizes seg_1 from
// int(feat_dim / 8 / 2), which agrees with that chain only when feat_dim is a multiple of 16: anything else is refused
// here (the reference's own forward fails in seg_1 then).
// Per block: conv1 (+ bn1, ReLU) and conv3 (+ bn3, the block input as residual, ReLU) are 1x1 layers of the conv-GEMM
// family; the depthwise 3x3 (+ bn2, ReLU) between them has no reduction over channels and is its own VALU kernel
// (dwconv3x3.hip), the same one for the fp32 and f16x3 back-ends.
//
// f16x3 and small weights.  The split-binary16 back-end cuts an operand into hi = half(x) and lo = half(x - hi); lo is
// about 2^-12 |x|, and below 2^-14 binary16 is subnormal: its spacing stays 2^-24, so an operand of magnitude m is
// represented to 2^-25 / m instead of 2^-22.  conv3's folded weights (rms ~0.005 .. 0.015, a damped residual branch) and
// the downsample layers' (~0.06) sit there: measured on depth 60, conv3 alone put 1.0e-6 and the downsample layers
// 5e-7 of relative error into the pooled statistics, conv1 (rms 0.13 .. 0.27) 5e-8.  The cure is an exact power of two:
// the binary16 planes of such a layer are cut from 2^k W (the fp32 plane stays W: the fp32 back-end is untouched), and
// the factor is taken out again, exactly, where the conv-GEMM family already has an operand for it --
//   downsample layer: (2^k W a + 2^k b) * 2^-k through the epilogue's post_scale (no activation in between), k such that
//                     the weights' rms lands in [1, 2);
//   conv3:            2^k W (2^-k a) through the A loader's pre_scale (a >= 0 behind the depthwise ReLU, so the loader's
//                     relu(a * 2^-k + 0) is a * 2^-k); here the activations pay what the weights gain, and with O(1)
//                     activations both sides are equally far from the subnormal range at 2^k = sqrt(1 / rms(W)).
#include "cnn2d_base.h"

namespace wsamd {

namespace {

struct GeminiLayout { const char* name; int depths[4]; };
const GeminiLayout kGeminiLayouts[] = {
    {"Gemini_DF_ResNet60", {3, 3, 9, 3}},
    {"Gemini_DF_ResNet114", {3, 3, 27, 3}},
    {"Gemini_DF_ResNet183", {3, 8, 45, 3}},
    {"Gemini_DF_ResNet237", {3, 8, 63, 3}},
};
const int kGeminiDims[5] = {32, 32, 64, 128, 256};
const int kStrideT[4] = {1, 2, 1, 1};        // gemini_dfresnet.py:74-75 (stride_f is 2 everywhere)

// one schedule step: a downsample layer (ds) or an inverted-bottleneck block
struct GeminiUnit {
  bool is_ds = false;
  int stage = 0;                 // ds: the layer index 1..4 - 1; block: its stage
  ConvW ds, c1, c3;
  size_t dw_w = 0, dw_b = 0;     // depthwise weights [4 dim][9] and bias [4 dim], bn2 folded
  int dim = 0;                   // ds: output channels; block: dim
  // f16x3 (see the head of the file): the binary16 planes hold 2^k W
  int ds_k = 0, c3_k = 0;
  size_t ds_bias_k = 0;          // 2^ds_k * bias
};

// rms of a packed weight matrix over its taps * Cin real columns (the row padding is zero)
double packed_rms(const std::vector<float>& host, const ConvW& cw) {
  double ss = 0;
  for (size_t i = 0, n = (size_t)cw.N * cw.ldw; i < n; ++i) ss += (double)host[cw.w + i] * host[cw.w + i];
  return std::sqrt(ss / ((double)cw.N * cw.Cin * cw.taps()));
}

struct GeminiModel : Cnn2dBase {
  GeminiLayout lay;
  std::vector<GeminiUnit> units;
  // No zero pads behind these buffers and no check_invariants tripwire, and none is needed: only the persistent fp32
  // GEMM's CONV form reads border taps from behind its input (ConvGemmParams::a_zero_off), and launch_conv_gemm takes
  // that form for 3x3 / stride 1 layers with a_zero_off > 0 only (gemm_f32_stream_is_conv3).  The 3x3 layers here, the
  // downsample layers that read small_buf, have stride 2 and pass a_zero_off = 0: they run on the tile kernels, whose
  // out-of-image taps read ConvGemmParams::zeros (the arena's zero page).  The stem and the depthwise 3x3 are kernels of
  // their own that test the image border.
  float* small_buf[2] = {nullptr, nullptr};    // dim-channel maps (stem, downsample outputs, block outputs)
  float* big_buf[2] = {nullptr, nullptr};      // 4 dim-channel maps (conv1 output, depthwise output)
  static constexpr int kVec = 1024;            // the widest scaled operand: conv3's 4 dim input channels of stage 4
  size_t zeros_vec = 0;                        // kVec zeros (post_shift / pre_shift)
  std::map<int, size_t> pow2_vec;              // k -> kVec floats of 2^-k

  size_t inv_pow2(int k) {
    auto it = pow2_vec.find(k);
    if (it != pow2_vec.end()) return it->second;
    std::vector<float> v(kVec, std::ldexp(1.0f, -k));
    return pow2_vec[k] = arena.add(v);
  }
  // the binary16 hi / lo planes of cw, cut again from 2^k W
  void resplit_scaled(const ConvW& cw, int k) {
    const size_t n = (size_t)cw.N * cw.ldw;
    const float s = std::ldexp(1.0f, k);
    uint16_t* hi = reinterpret_cast<uint16_t*>(arena.host.data() + cw.wh);
    uint16_t* lo = reinterpret_cast<uint16_t*>(arena.host.data() + cw.wl);
    for (size_t i = 0; i < n; ++i) {
      const float v = arena.host[cw.w + i] * s;
      hi[i] = float_to_half_bits(v);
      lo[i] = float_to_half_bits(v - half_bits_to_float(hi[i]));
    }
  }
  static int clamp_k(double k, int hi) { return k < 0 ? 0 : (k > hi ? hi : (int)k); }

  // taps of the last chunk beyond Cnn2dBase::BlockTaps (whose `block` is null when the last executed unit is a downsample
  // layer): that layer's output, or the block's conv1 and depthwise outputs
  const float *tap_ds = nullptr, *tap_exp = nullptr, *tap_dw = nullptr;

  GeminiModel(const GeminiLayout& l, int fd, int ed) : Cnn2dBase(l.name, fd, ed), lay(l) {}

  bool wants(const std::string& key) const override {
    return wants_prefixes(key, {"downsample_layers.", "stages.", "seg_1.", "seg_bn_1.", "seg_2."});
  }

  int set_precision(int mode) override {
    return mode == 2 ? no_f16io_backend("its depthwise 3x3 kernel is") : ModelBase::set_precision(mode);
  }

  int finalize(const SD& sd, int max_batch, int max_frames) override {
    int err = 0;
    if (feat_dim % 16) {
      set_error("%s needs feat_dim %% 16 == 0, got %d (the reference sizes seg_1 from int(feat_dim / 8 / 2), its maps "
                "shrink by (n - 1) / 2 + 1: they agree only for multiples of 16)", name.c_str(), feat_dim);
      return WS_ERR_INVALID_ARG;
    }
    const int* d = kGeminiDims;
    zeros_vec = arena.add(nullptr, kVec);
    // stem: Conv2d(1, 32, 3x3) + BN
    if ((err = pack_stem3x3(sd, "downsample_layers.0.0", "downsample_layers.0.1", d[0], &stem_w, &stem_b))) return err;
    for (int s = 0; s < 4; ++s) {
      const int dim = d[s + 1];
      {
        GeminiUnit u;
        u.is_ds = true; u.stage = s; u.dim = dim;
        const std::string p = "downsample_layers." + std::to_string(s + 1);
        if ((err = pack_conv2d(sd, p + ".0", dim, d[s], 3, 3, p + ".1", &u.ds))) return err;
        u.ds_k = clamp_k(std::ceil(std::log2(1.0 / packed_rms(arena.host, u.ds))), 12);     // rms -> [1, 2)
        if (u.ds_k) {
          resplit_scaled(u.ds, u.ds_k);
          std::vector<float> bk(dim);
          for (int c = 0; c < dim; ++c) bk[c] = arena.host[u.ds.b + c] * std::ldexp(1.0f, u.ds_k);
          u.ds_bias_k = arena.add(bk);
          (void)inv_pow2(u.ds_k);
        }
        units.push_back(u);
      }
      for (int b = 0; b < lay.depths[s]; ++b) {
        GeminiUnit u;
        u.stage = s; u.dim = dim;
        const std::string p = "stages." + std::to_string(s) + "." + std::to_string(b);
        if ((err = pack_conv2d(sd, p + ".conv1", 4 * dim, dim, 1, 1, p + ".bn1", &u.c1))) return err;
        // conv2: (4 dim, 1, 3, 3), groups = 4 dim, with bn2 folded -> [4 dim][9] + [4 dim]
        if ((err = pack_stem3x3(sd, p + ".conv2", p + ".bn2", 4 * dim, &u.dw_w, &u.dw_b))) return err;
        if ((err = pack_conv2d(sd, p + ".conv3", dim, 4 * dim, 1, 1, p + ".bn3", &u.c3))) return err;
        u.c3_k = clamp_k(std::floor(0.5 * std::log2(1.0 / packed_rms(arena.host, u.c3)) + 0.5), 8);   // 2^k ~ rms^-1/2
        if (u.c3_k) {
          resplit_scaled(u.c3, u.c3_k);
          (void)inv_pow2(u.c3_k);
        }
        units.push_back(u);
      }
    }
    n_stops = (int)units.size();
    stops_are = "stop points after the stem: its 4 downsample layers and " + std::to_string(n_stops - 4) +
                " blocks in forward order";
    stats_dim = (feat_dim / 16) * d[4];                    // gemini_dfresnet.py:63
    if ((err = pack_seg_head(sd))) return err;
    if ((err = upload_weights())) return err;
    return reserve(max_batch, max_frames);
  }

  int reserve(int max_batch, int max_frames) override {
    int err = 0;
    begin_reserve(max_batch, max_frames);
    tap_ds = tap_exp = tap_dw = nullptr;
    // dim-channel maps: the stem's (F x T x 32) is the largest; 4 dim-channel maps: stage 1's (F/2 x T x 128)
    const size_t small = (size_t)maxB * feat_dim * maxT * 32;
    const size_t big = (size_t)maxB * (feat_dim / 2) * maxT * 128;
    if ((err = refuse_map_too_large(big))) return err;
    Carve cv = begin_carve();
    const size_t o_s0 = cv.take(small), o_s1 = cv.take(small), o_b0 = cv.take(big), o_b1 = cv.take(big);
    if ((err = alloc_with_seg_head(cv))) return err;
    float* base = ws.as<float>();
    small_buf[0] = base + o_s0; small_buf[1] = base + o_s1; big_buf[0] = base + o_b0; big_buf[1] = base + o_b1;
    return 0;
  }

  int min_frames() const override { return 1; }

  int forward_chunk(const float* feats, int B, int T, float* emb, hipStream_t st) override {
    if (gemm_precision == 2) return no_f16io_backend();      // (set_precision refuses it)
    BlockTaps& tp = begin_chunk();             // host-side notes for ws_debug_engine_tap, readable when the chunk ends
    tap_ds = tap_exp = tap_dw = nullptr;
    int H = feat_dim, W = T, lvl = 0, cur = 0;
    float* x = small_buf[0];
    WS_LAUNCH(other(4.0 * B * H * (double)W * 33, st, [&] {
      return launch_stem_conv3x3(feats, B, T, feat_dim, arena.at(stem_w), arena.at(stem_b), 32, x, st, nullptr,
                                 cur_lens[0]);
    }));
    tp.n_exec = 0; tp.stem = x; tp.stem_rows = B * H * W; tp.stem_c = 32;
    if (stop_after == 0) return end_chunk(false, B, T, emb, st);
    for (size_t ui = 0; ui < units.size(); ++ui) {
      const GeminiUnit& u = units[ui];
      float* y = small_buf[cur ^ 1];
      if (u.is_ds) {
        // Conv2d(3x3, stride (2, stride_t), padding 1) + BN, NO activation (gemini_dfresnet.py:78-84)
        const int sw = kStrideT[u.stage];
        const int lo = lvl + (sw == 2 ? 1 : 0);
        ConvGemmParams p = conv2d(u.ds, x, u.ds.Cin, 0, y, u.dim, 0, B, H, W, 2, sw, 1, 1, 1, 1, ACT_NONE);
        p.row_len = cur_lens[lo];                          // stride level of the OUTPUT width
        if (gemm_precision == 1 && u.ds_k) {               // the binary16 planes hold 2^k W: (2^k W a + 2^k b) * 2^-k
          p.bias = arena.at(u.ds_bias_k);
          p.post_scale = arena.at(pow2_vec.at(u.ds_k)); p.post_shift = arena.at(zeros_vec);
        }
        WS_LAUNCH(gemm(p, st));
        H = p.Hout; W = p.Wout; lvl = lo;
      } else {
        const int dim = u.dim, C4 = 4 * dim;
        float *e = big_buf[0], *dwo = big_buf[1];
        ConvGemmParams p1 = conv2d(u.c1, x, dim, 0, e, C4, 0, B, H, W, 1, 1, 1, 1, 0, 0, ACT_RELU);
        p1.row_len = cur_lens[lvl];
        WS_LAUNCH(gemm(p1, st));
        DwConv3x3Params dp = {};
        dp.x = e; dp.out = dwo; dp.w = arena.at(u.dw_w); dp.bias = arena.at(u.dw_b);
        dp.B = B; dp.F = H; dp.T = W; dp.C = C4; dp.row_len = cur_lens[lvl];
        if (const char* why = dwconv3x3_refusal(dp)) {     // a missing kernel is an error, never a slower path
          set_error("%s: the depthwise 3x3 kernel refuses unit %d (%s)", name.c_str(), (int)ui + 1, why);
          return WS_ERR_STATE;
        }
        WS_LAUNCH(other(8.0 * B * H * (double)W * C4, st, [&] { return launch_dwconv3x3(dp, st); }));
        ConvGemmParams p3 = conv2d(u.c3, dwo, C4, 0, y, dim, 0, B, H, W, 1, 1, 1, 1, 0, 0, ACT_RELU);
        p3.row_len = cur_lens[lvl];
        p3.residual = x; p3.ldr = dim; p3.r_off = 0;
        if (gemm_precision == 1 && u.c3_k) {               // the binary16 planes hold 2^k W: the loader reads 2^-k a (a >= 0)
          p3.pre_scale = arena.at(pow2_vec.at(u.c3_k)); p3.pre_shift = arena.at(zeros_vec);
        }
        WS_LAUNCH(gemm(p3, st));
      }
      cur ^= 1;
      x = small_buf[cur];
      const bool stop = stop_after == (int)ui + 1;
      if (stop || ui + 1 == units.size()) {
        tp.n_exec = (int)ui + 1; tp.rows = B * H * W; tp.block_c = u.dim;
        tap_ds = u.is_ds ? x : nullptr;
        tp.block = u.is_ds ? nullptr : x;
        tap_exp = u.is_ds ? nullptr : big_buf[0];
        tap_dw = u.is_ds ? nullptr : big_buf[1];
        if (stop) return end_chunk(false, B, T, emb, st);
      }
    }
    return pool_and_head(x, kGeminiDims[4], B, H, W, lvl, T, emb, st);       // (gemini_dfresnet.py:129-139)
  }

  // ws_debug_engine_tap: stem (stopped at 0); of the last executed unit: ds (a downsample layer's output) or exp / dw /
  // block (conv1's, the depthwise kernel's and the block's output), rows = B*H*W in [b][f][t] order; pooled and emb_a
  // after a full forward
  int tap(const char* tname, float* dst, int64_t cap_floats, int32_t* rows, int32_t* cols, hipStream_t st) override {
    if (int r = tap_guard()) return r;
    const BlockTaps& t = block_taps;
    const std::string n = tname;
    char why[200];
    if (n == "ds" || n == "exp" || n == "dw" || n == "block") {
      if (t.n_exec < 1)
        return tap_copy(tname, nullptr, "the last forward was stopped after the stem", 0, 0, dst, cap_floats, rows, cols, st);
      if (n == "ds") {
        std::snprintf(why, sizeof(why), "stop point %d is a block, not a downsample layer", t.n_exec);
        return tap_copy(tname, tap_ds, why, t.rows, t.block_c, dst, cap_floats, rows, cols, st);
      }
      std::snprintf(why, sizeof(why), "stop point %d is a downsample layer, not a block", t.n_exec);
      if (n == "block") return tap_copy(tname, t.block, why, t.rows, t.block_c, dst, cap_floats, rows, cols, st);
      return tap_copy(tname, n == "exp" ? tap_exp : tap_dw, why, t.rows, 4 * t.block_c, dst, cap_floats, rows, cols, st);
    }
    std::snprintf(why, sizeof(why), "the last forward was stopped at %d: pooling and the head did not run", t.n_exec);
    return tap_shared(tname, dst, cap_floats, rows, cols, st,
                      {"stem, ds, exp, dw, block, pooled, emb_a", why, nullptr, "units"});
  }

  double flops(int batch, int T) const override {
    double macs = 0;
    int H = feat_dim, W = T;
    macs += (double)H * W * 9 * 32;
    for (const GeminiUnit& u : units) {
      if (u.is_ds) {
        H = (H - 1) / 2 + 1;
        if (kStrideT[u.stage] == 2) W = (W - 1) / 2 + 1;
        macs += (double)H * W * 9 * u.ds.Cin * u.dim;
      } else {
        macs += (double)H * W * (8.0 * u.dim * u.dim + 9.0 * 4 * u.dim);
      }
    }
    return 2.0 * (macs + seg_head_macs()) * batch;
  }
};

}  // namespace

Model* make_gemini(const std::string& model_name, int feat_dim, int embed_dim) {
  for (const GeminiLayout& l : kGeminiLayouts)
    if (model_name == l.name) return new GeminiModel(l, feat_dim, embed_dim);
  return nullptr;
}

}  // namespace wsamd
