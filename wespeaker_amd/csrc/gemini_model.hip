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
// Layout and BN folding as in resnet_model.hip (channels-last [b][f][t][c] fp32, conv -> BN folded on the host in float64).
// The frequency axis is halved by every downsample layer, the time axis by the second one only ("T14c" strides
// (2,1) (2,2) (2,1) (2,1)); both follow (n - 1) / 2 + 1.  The reference sizes seg_1 from int(feat_dim / 8 / 2), which
// agrees with that chain only when feat_dim is a multiple of 16: anything else is refused here (the reference's own
// forward fails in seg_1 then).
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
#include "model_common.h"

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

struct GeminiModel : ModelBase {
  GeminiLayout lay;
  size_t stem_w = 0, stem_b = 0;
  std::vector<GeminiUnit> units;
  ConvW seg1, seg2;
  bool two_emb = false;
  size_t seg_bn_scale = 0, seg_bn_shift = 0;
  float* small_buf[2] = {nullptr, nullptr};    // dim-channel maps (stem, downsample outputs, block outputs)
  float* big_buf[2] = {nullptr, nullptr};      // 4 dim-channel maps (conv1 output, depthwise output)
  float *pooled = nullptr, *partial = nullptr, *emb_a = nullptr;
  int stats_dim = 0;
  static constexpr int kSplitK = 16;
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

  // what the last chunk's last executed unit left (host-side notes for ws_debug_engine_tap)
  struct Taps {
    int n_exec = -1;
    bool full = false, last_is_ds = false;
    const float *stem = nullptr, *ds = nullptr, *exp = nullptr, *dw = nullptr, *block = nullptr;
    int stem_rows = 0, rows = 0, c = 0, B = 0;
  } taps;

  GeminiModel(const GeminiLayout& l, int fd, int ed) : ModelBase(l.name, fd, ed), lay(l) {}

  bool wants(const std::string& key) const override {
    if (key.size() > 20 && key.compare(key.size() - 19, 19, "num_batches_tracked") == 0) return false;
    static const char* prefixes[] = {"downsample_layers.", "stages.", "seg_1.", "seg_bn_1.", "seg_2."};
    for (auto p : prefixes)
      if (key.compare(0, std::strlen(p), p) == 0) return true;
    return false;
  }

  int set_precision(int mode) override {
    if (mode == 2) {
      set_error("%s has no binary16-tensor back-end (precision mode 2): its depthwise 3x3 kernel is fp32; use "
                "mode 0 (fp32) or 1 (f16x3)", name.c_str());
      return WS_ERR_INVALID_ARG;
    }
    return ModelBase::set_precision(mode);
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
    {   // stem: Conv2d(1, 32, 3x3) + BN folded -> [C][9] + [C]
      const HostTensor* wt = get(sd, "downsample_layers.0.0.weight", {d[0], 1, 3, 3}, &err);
      if (!wt) return err;
      std::vector<double> sc, sh;
      if ((err = bn_affine(sd, "downsample_layers.0.1", d[0], &sc, &sh))) return err;
      std::vector<float> wf(d[0] * 9), bf(d[0]);
      for (int c = 0; c < d[0]; ++c) {
        for (int k = 0; k < 9; ++k) wf[c * 9 + k] = (float)(wt->data[c * 9 + k] * sc[c]);
        bf[c] = (float)sh[c];
      }
      stem_w = arena.add(wf);
      stem_b = arena.add(bf);
    }
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
        {   // conv2: (4 dim, 1, 3, 3), groups = 4 dim, with bn2 folded -> [4 dim][9] + [4 dim]
          const int C = 4 * dim;
          const HostTensor* wt = get(sd, p + ".conv2.weight", {C, 1, 3, 3}, &err);
          if (!wt) return err;
          std::vector<double> sc, sh;
          if ((err = bn_affine(sd, p + ".bn2", C, &sc, &sh))) return err;
          std::vector<float> wf((size_t)C * 9), bf(C);
          for (int c = 0; c < C; ++c) {
            for (int k = 0; k < 9; ++k) wf[(size_t)c * 9 + k] = (float)((double)wt->data[(size_t)c * 9 + k] * sc[c]);
            bf[c] = (float)sh[c];
          }
          u.dw_w = arena.add(wf);
          u.dw_b = arena.add(bf);
        }
        if ((err = pack_conv2d(sd, p + ".conv3", dim, 4 * dim, 1, 1, p + ".bn3", &u.c3))) return err;
        u.c3_k = clamp_k(std::floor(0.5 * std::log2(1.0 / packed_rms(arena.host, u.c3)) + 0.5), 8);   // 2^k ~ rms^-1/2
        if (u.c3_k) {
          resplit_scaled(u.c3, u.c3_k);
          (void)inv_pow2(u.c3_k);
        }
        units.push_back(u);
      }
    }
    stats_dim = (feat_dim / 16) * d[4];                    // gemini_dfresnet.py:63
    if ((err = pack_linear(sd, "seg_1", embed_dim, 2 * stats_dim, true, &seg1))) return err;
    two_emb = sd.count("seg_2.weight") > 0;
    if (two_emb) {
      if ((err = add_bn_vectors(sd, "seg_bn_1", embed_dim, &seg_bn_scale, &seg_bn_shift, false))) return err;
      seg1.scale = seg_bn_scale; seg1.shift = seg_bn_shift;     // relu -> BN(affine=False) epilogue
      if ((err = pack_linear(sd, "seg_2", embed_dim, embed_dim, true, &seg2))) return err;
    }
    if ((err = upload_weights())) return err;
    return reserve(max_batch, max_frames);
  }

  int reserve(int max_batch, int max_frames) override {
    int err = 0;
    maxB = max_batch; maxT = max_frames;
    last_chunk = LastChunk();
    taps = Taps();
    // dim-channel maps: the stem's (F x T x 32) is the largest; 4 dim-channel maps: stage 1's (F/2 x T x 128)
    const size_t small = (size_t)maxB * feat_dim * maxT * 32;
    const size_t big = (size_t)maxB * (feat_dim / 2) * maxT * 128;
    if (big >= (size_t)1 << 31) {
      set_error("%s: max_batch %d x max_frames %d puts %zu elements in one activation map (limit 2^31); "
                "use a smaller engine chunk", name.c_str(), max_batch, max_frames, big);
      return WS_ERR_CAPACITY;
    }
    size_t total = 0;
    auto take = [&](size_t n) { size_t o = total; total += (n + 63) & ~size_t(63); return o; };
    const size_t o_s0 = take(small), o_s1 = take(small), o_b0 = take(big), o_b1 = take(big);
    const size_t o_pool = take((size_t)maxB * 2 * stats_dim), o_part = take((size_t)kSplitK * maxB * embed_dim),
                 o_emba = take((size_t)maxB * embed_dim), o_feats = take((size_t)maxB * maxT * feat_dim);
    if ((err = alloc_workspace(total))) return err;
    float* base = ws.as<float>();
    small_buf[0] = base + o_s0; small_buf[1] = base + o_s1; big_buf[0] = base + o_b0; big_buf[1] = base + o_b1;
    pooled = base + o_pool; partial = base + o_part; emb_a = base + o_emba; feats_ws = base + o_feats;
    return 0;
  }

  int min_frames() const override { return 1; }

  int forward_chunk(const float* feats, int B, int T, float* emb, hipStream_t st) override {
    if (gemm_precision == 2) {               // (set_precision refuses it)
      set_error("%s has no binary16-tensor back-end (precision mode 2)", name.c_str());
      return WS_ERR_STATE;
    }
    last_chunk.B = 0;
    int H = feat_dim, W = T, lvl = 0, cur = 0;
    float* x = small_buf[0];
    WS_LAUNCH(other(4.0 * B * H * (double)W * 33, st, [&] {
      return launch_stem_conv3x3(feats, B, T, feat_dim, arena.at(stem_w), arena.at(stem_b), 32, x, st, nullptr,
                                 cur_lens[0]);
    }));
    Taps tp;
    tp.B = B; tp.n_exec = 0; tp.stem = x; tp.stem_rows = B * H * W;
    if (stop_after == 0) return end_chunk(tp, false, B, T, emb, st);
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
        tp.exp = e; tp.dw = dwo;
      }
      cur ^= 1;
      x = small_buf[cur];
      const bool stop = stop_after == (int)ui + 1;
      if (stop || ui + 1 == units.size()) {
        tp.n_exec = (int)ui + 1; tp.rows = B * H * W; tp.c = u.dim; tp.last_is_ds = u.is_ds;
        tp.ds = u.is_ds ? x : nullptr;
        tp.block = u.is_ds ? nullptr : x;
        if (stop) return end_chunk(tp, false, B, T, emb, st);
      }
    }
    const int Cl = kGeminiDims[4];
    WS_LAUNCH(other(8.0 * B * H * (double)W * Cl, st, [&] {
      return launch_tstp(x, Cl, B, H, W, Cl, nullptr, nullptr, pooled, st, cur_lens[lvl]);
    }));
    if (!two_emb) {
      WS_LAUNCH(gemm_splitk(conv1d(seg1, pooled, 2 * stats_dim, 0, emb, embed_dim, 0, B, 1, 1, ACT_NONE),
                            partial, kSplitK, st));
    } else {            // embed_b = seg_2(seg_bn_1(relu(seg_1(stats))))   (gemini_dfresnet.py:134-139)
      ConvGemmParams a = conv1d(seg1, pooled, 2 * stats_dim, 0, emb_a, embed_dim, 0, B, 1, 1, ACT_RELU);
      a.post_scale = arena.at(seg_bn_scale); a.post_shift = arena.at(seg_bn_shift);
      WS_LAUNCH(gemm_splitk(a, partial, kSplitK, st));
      WS_LAUNCH(gemm(conv1d(seg2, emb_a, embed_dim, 0, emb, embed_dim, 0, B, 1, 1, ACT_NONE), st));
    }
    return end_chunk(tp, true, B, T, emb, st);
  }

  int end_chunk(Taps& tp, bool full, int B, int T, float* emb, hipStream_t st) {
    tp.full = full;
    if (!full)
      if (int r = stop_chunk(emb, B, st)) return r;
    taps = tp;
    last_chunk.B = B; last_chunk.T = T; last_chunk.prec = gemm_precision;
    return 0;
  }

  int set_stop_after(int n) override {
    if (n < -1 || n > (int)units.size()) {
      set_error("ws_debug_engine_stop_after: n_blocks = %d, %s has %d stop points after the stem: its 4 downsample layers "
                "and %d blocks in forward order (-1 = the full forward, 0 = after the stem)", n, name.c_str(),
                (int)units.size(), (int)units.size() - 4);
      return WS_ERR_INVALID_ARG;
    }
    stop_after = n;
    return WS_OK;
  }

  // ws_debug_engine_tap: stem (stopped at 0); of the last executed unit: ds (a downsample layer's output) or exp / dw /
  // block (conv1's, the depthwise kernel's and the block's output), rows = B*H*W in [b][f][t] order; pooled and emb_a
  // after a full forward
  int tap(const char* tname, float* dst, int64_t cap_floats, int32_t* rows, int32_t* cols, hipStream_t st) override {
    if (!last_chunk.B) {
      set_error("ws_debug_engine_tap: no forward has run on this engine since it was finalized / re-sized");
      return WS_ERR_INVALID_ARG;
    }
    const Taps& t = taps;
    const std::string n = tname;
    char why[200];
    if (n == "stem") {
      std::snprintf(why, sizeof(why), "the last forward ran %d units over the stem's buffer: stop it at 0 "
                    "(ws_debug_engine_stop_after)", t.n_exec);
      return tap_copy(tname, t.n_exec == 0 ? t.stem : nullptr, why, t.stem_rows, 32, dst, cap_floats, rows, cols, st);
    }
    if (n == "ds" || n == "exp" || n == "dw" || n == "block") {
      if (t.n_exec < 1)
        return tap_copy(tname, nullptr, "the last forward was stopped after the stem", 0, 0, dst, cap_floats, rows, cols, st);
      if (n == "ds") {
        std::snprintf(why, sizeof(why), "stop point %d is a block, not a downsample layer", t.n_exec);
        return tap_copy(tname, t.ds, why, t.rows, t.c, dst, cap_floats, rows, cols, st);
      }
      std::snprintf(why, sizeof(why), "stop point %d is a downsample layer, not a block", t.n_exec);
      if (n == "block") return tap_copy(tname, t.block, why, t.rows, t.c, dst, cap_floats, rows, cols, st);
      return tap_copy(tname, t.last_is_ds ? nullptr : (n == "exp" ? t.exp : t.dw), why, t.rows, 4 * t.c, dst, cap_floats,
                      rows, cols, st);
    }
    if (n == "pooled" || n == "emb_a") {
      std::snprintf(why, sizeof(why), "the last forward was stopped at %d: pooling and the head did not run", t.n_exec);
      if (n == "pooled")
        return tap_copy(tname, t.full ? pooled : nullptr, why, t.B, 2 * stats_dim, dst, cap_floats, rows, cols, st);
      return tap_copy(tname, !two_emb ? nullptr : (t.full ? emb_a : nullptr),
                      two_emb ? why : "the model has one embedding layer (no seg_2)", t.B, embed_dim, dst, cap_floats,
                      rows, cols, st);
    }
    set_error("ws_debug_engine_tap: unknown tensor '%s' (%s: stem, ds, exp, dw, block, pooled, emb_a)", tname, name.c_str());
    return WS_ERR_INVALID_ARG;
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
    macs += 2.0 * stats_dim * embed_dim;
    if (two_emb) macs += (double)embed_dim * embed_dim;
    return 2.0 * macs * batch;
  }
};

}  // namespace

Model* make_gemini(const std::string& model_name, int feat_dim, int embed_dim) {
  for (const GeminiLayout& l : kGeminiLayouts)
    if (model_name == l.name) return new GeminiModel(l, feat_dim, embed_dim);
  return nullptr;
}

}  // namespace wsamd
