// SimAM-ResNet34/100 + ASP speaker-embedding forward (the VoxBlink2 hub models) scheduled onto the gfx950 kernels.
//
// Reference (file:line in wenet-e2e/wespeaker):
//   wespeaker/models/samresnet.py:73-123   ResNet front (conv1+bn1+relu, 4 stages of SimAMBasicBlock, width in_planes)
//   wespeaker/models/samresnet.py:21-70    SimAMBasicBlock (conv-bn-relu, conv-bn, SimAM, += downsample, relu)
//   wespeaker/models/samresnet.py:134-167  SimAM_ResNet34_ASP / SimAM_ResNet100_ASP (front, ASP, bottleneck Linear)
//   wespeaker/models/pooling_layers.py:151-204 ASP (Conv1d, ReLU, BatchNorm1d, Conv1d, softmax over time)
//
// Layout, BN folding, the zero-padded activation buffers and the shared taps: cnn2d_base.h (its seg_1 head is not used:
// the ASP head is this file's).  The SimAM gate needs whole-plane statistics of conv2's output, so conv2 runs without
// residual / activation and the gate + residual + ReLU is its own kernel (simam_ops.hip).  ASP: the first attention
// conv reads the last stage as a kh = F', kw = 1 convolution (its K index f*C + c is a host-side permutation of the
// reference's c*F' + f); the eval BatchNorm1d sits AFTER the ReLU, so it is folded forward into the second conv
// (W2' = W2 diag(s), b2' = W2 t + b2, float64), whose rows are packed in the same f*C + c order for the pooling
// kernel.
#include "cnn2d_base.h"

namespace wsamd {

namespace {

struct SamLayout { const char* name; int blocks[4]; };
const SamLayout kSamLayouts[] = {
    {"SimAM_ResNet34_ASP", {3, 4, 6, 3}},
    {"SimAM_ResNet100_ASP", {6, 16, 24, 3}},
};

struct SamBlock {
  ConvW c1, c2, sc;
  bool has_sc = false;
  int stride = 1, in_planes = 0, planes = 0;
};

struct SamResNetModel : Cnn2dBase {            // (stats_dim = D = C_last * F_last; pooled, partial: the ASP head's)
  SamLayout lay;
  int m = 0;                                 // in_planes, read from front.conv1.weight at finalize
  static constexpr int kHidden = 128;        // ASP hidden width (pooling_layers.py:178)
  static constexpr size_t kTapCap = (size_t)1 << 22;   // floats kept for the 'block1' tap (larger chunks keep none)
  std::vector<SamBlock> blocks;
  ConvW asp1, asp2, bott;
  float *hid = nullptr, *logits = nullptr;
  float *sm_part = nullptr, *sm_mu = nullptr, *sm_k = nullptr, *tap_block1 = nullptr;
  bool tap_block1_valid = false;

  SamResNetModel(const SamLayout& l, int fd, int ed) : Cnn2dBase(l.name, fd, ed), lay(l) {}

  bool wants(const std::string& key) const override {
    return wants_prefixes(key, {"front.conv1.", "front.bn1.", "front.layer1.", "front.layer2.", "front.layer3.",
                                "front.layer4.", "pooling.attention.0.", "pooling.attention.2.", "pooling.attention.3.",
                                "bottleneck."});
  }

  int set_precision(int mode) override {
    return mode == 2 ? no_f16io_backend("its SimAM and ASP kernels are") : ModelBase::set_precision(mode);
  }

  int finalize(const SD& sd, int max_batch, int max_frames) override {
    int err = 0;
    if (feat_dim % 8) {
      set_error("%s needs feat_dim %% 8 == 0, got %d", name.c_str(), feat_dim);
      return WS_ERR_INVALID_ARG;
    }
    auto it = sd.find("front.conv1.weight");
    if (it == sd.end()) {
      set_error("missing tensor 'front.conv1.weight' for model %s", name.c_str());
      return WS_ERR_MISSING_TENSOR;
    }
    m = it->second.shape.empty() ? 0 : (int)it->second.shape[0];
    if (m < 16 || m % 16 || m > 128) {
      set_error("%s: in_planes = %d (leading dimension of front.conv1.weight) must be a multiple of 16 in [16, 128]",
                name.c_str(), m);
      return WS_ERR_SHAPE;
    }
    if ((err = pack_stem3x3(sd, "front.conv1", "front.bn1", m, &stem_w, &stem_b))) return err;   // Conv2d(1, m, 3x3) + bn1
    int in_planes = m;
    for (int s = 0; s < 4; ++s) {
      const int planes = m << s;
      for (int b = 0; b < lay.blocks[s]; ++b) {
        SamBlock blk;
        blk.stride = (b == 0 && s > 0) ? 2 : 1;
        blk.in_planes = in_planes; blk.planes = planes;
        const std::string p = "front.layer" + std::to_string(s + 1) + "." + std::to_string(b);
        if ((err = pack_conv2d(sd, p + ".conv1", planes, in_planes, 3, 3, p + ".bn1", &blk.c1))) return err;
        if ((err = pack_conv2d(sd, p + ".conv2", planes, planes, 3, 3, p + ".bn2", &blk.c2))) return err;
        if (blk.stride != 1 || in_planes != planes) {
          blk.has_sc = true;
          if ((err = pack_conv2d(sd, p + ".downsample.0", planes, in_planes, 1, 1, p + ".downsample.1", &blk.sc)))
            return err;
        }
        in_planes = planes;
        blocks.push_back(blk);
      }
    }
    n_stops = (int)blocks.size();
    const int Fl = feat_dim / 8, Cl = m * 8, D = Cl * Fl;
    stats_dim = D;                                         // pooling_layers.py:169-170
    // attention.0: Conv1d(D -> 128, k = 1) read as a (kh = F', kw = 1) convolution over [b][f][t][c]
    if ((err = pack_conv(sd, "pooling.attention.0", {kHidden, D, 1}, kHidden, Cl, Fl, 1,
                         [=](int n, int tp, int ci) { return (size_t)n * D + (size_t)ci * Fl + tp; }, true, "", "",
                         &asp1)))
      return err;
    {   // attention.3 with attention.2 (BatchNorm1d after the ReLU) folded in, rows in f*C + c order
      const HostTensor* w2 = get(sd, "pooling.attention.3.weight", {D, kHidden, 1}, &err);
      if (!w2) return err;
      const HostTensor* b2 = get(sd, "pooling.attention.3.bias", {D}, &err);
      if (!b2) return err;
      std::vector<double> sc, sh;
      if ((err = bn_affine(sd, "pooling.attention.2", kHidden, &sc, &sh))) return err;
      SD tmp;
      HostTensor wt, bt;
      wt.shape = {D, kHidden}; wt.data.resize((size_t)D * kHidden);
      bt.shape = {D}; bt.data.resize(D);
      for (int f = 0; f < Fl; ++f)
        for (int c = 0; c < Cl; ++c) {
          const size_t src = (size_t)c * Fl + f, dst = (size_t)f * Cl + c;
          double bias = (double)b2->data[src];
          for (int j = 0; j < kHidden; ++j) {
            const double w = (double)w2->data[src * kHidden + j];
            wt.data[dst * kHidden + j] = (float)(w * sc[j]);
            bias += w * sh[j];
          }
          bt.data[dst] = (float)bias;
        }
      tmp["asp2.weight"] = std::move(wt);
      tmp["asp2.bias"] = std::move(bt);
      if ((err = pack_linear(tmp, "asp2", D, kHidden, true, &asp2))) return err;
    }
    if ((err = pack_linear(sd, "bottleneck", embed_dim, 2 * D, true, &bott))) return err;
    if ((err = upload_weights())) return err;
    return reserve(max_batch, max_frames);
  }

  int reserve(int max_batch, int max_frames) override {
    int err = 0;
    begin_reserve(max_batch, max_frames);
    tap_block1_valid = false;
    // largest activation: every stage-1 map (F x T x in_planes); later stages halve
    const size_t act = (size_t)maxB * feat_dim * maxT * (size_t)m;
    if ((err = refuse_map_too_large(act)) || (err = refuse_batch_too_large())) return err;
    Carve cv = begin_carve();
    for (int i = 0; i < 4; ++i) buf.carve(cv, act);          // the block rotation
    const int Tl = level_len(maxT, 3);
    size_t part = 0;                       // SimAM slice partials: the largest stage
    for (int s = 0, H = feat_dim; s < 4; ++s) {
      if (s) H = (H - 1) / 2 + 1;
      const int C = m << s;
      const size_t n = (size_t)maxB * simam_slices(H * level_len(maxT, s), C) * 3 * C;
      part = n > part ? n : part;
    }
    const size_t o_hid = cv.take((size_t)maxB * Tl * kHidden), o_log = cv.take((size_t)maxB * Tl * stats_dim),
                 o_pool = cv.take((size_t)maxB * 2 * stats_dim), o_part = cv.take((size_t)kSplitK * maxB * embed_dim),
                 o_sp = cv.take(part), o_mu = cv.take((size_t)maxB * m * 8), o_k = cv.take((size_t)maxB * m * 8),
                 o_tap = cv.take(act < kTapCap ? act : kTapCap), o_feats = cv.take((size_t)maxB * maxT * feat_dim);
    if ((err = alloc_workspace(cv.total))) return err;
    float* base = ws.as<float>();
    hid = base + o_hid; logits = base + o_log; pooled = base + o_pool; partial = base + o_part;
    sm_part = base + o_sp; sm_mu = base + o_mu; sm_k = base + o_k; tap_block1 = base + o_tap;
    feats_ws = base + o_feats;
    return buf.bind(base);
  }

  int min_frames() const override { return 2; }

  // SimAM divides by (F * len - 1) on every plane; the smallest is the last stage's (F / 8) x len_3
  bool plane_too_small(int frames) const { return (feat_dim / 8) * level_len(frames, 3) < 2; }
  int refuse_small_plane(int frames) {
    set_error("%s: an utterance of %d frames leaves a last-stage plane of %d x %d = fewer than 2 elements; the SimAM "
              "variance divides by n - 1 = 0 there", name.c_str(), frames, feat_dim / 8, level_len(frames, 3));
    return WS_ERR_INVALID_ARG;
  }
  const int* upload_lens(const int32_t* lens_host, int batch, int frames, hipStream_t st) override {
    for (int b = 0; b < batch; ++b)
      if (lens_host[b] >= min_frames() && lens_host[b] <= frames && plane_too_small(lens_host[b])) {
        (void)refuse_small_plane(lens_host[b]);
        return nullptr;
      }
    return ModelBase::upload_lens(lens_host, batch, frames, st);
  }

  int forward_chunk(const float* feats, int B, int T, float* emb, hipStream_t st) override {
    if (gemm_precision == 2) return no_f16io_backend();      // (set_precision refuses it)
    if (!ragged() && plane_too_small(T)) return refuse_small_plane(T);
    BlockTaps& tp = begin_chunk();             // host-side notes for ws_debug_engine_tap, readable when the chunk ends
    tap_block1_valid = false;
    int H = feat_dim, W = T, lvl = 0;
    float* x = buf[0];
    WS_LAUNCH(other(4.0 * B * H * (double)W * (m + 1), st, [&] {
      return launch_stem_conv3x3_any(feats, B, T, feat_dim, arena.at(stem_w), arena.at(stem_b), m, x, st, cur_lens[0]);
    }));
    tp.n_exec = 0; tp.stem = x; tp.stem_rows = B * H * W; tp.stem_c = m;
    if (stop_after == 0) return end_chunk(false, B, T, emb, st);
    auto conv = [&](const ConvW& cw, const float* in, int Cin_, float* out, int Cout_, int Hin_, int Win_, int s_,
                    int pad, int act, int out_lvl) {
      ConvGemmParams p = conv2d(cw, in, Cin_, 0, out, Cout_, 0, B, Hin_, Win_, s_, s_, 1, 1, pad, pad, act);
      p.row_len = cur_lens[out_lvl];                       // stride level of this launch's OUTPUT width
      p.a_zero_off = buf.zero_off_for(in, Cin_);           // the zero pad behind the input's buffer
      return gemm(p, st);
    };
    int cur = 0;
    for (size_t bi = 0; bi < blocks.size(); ++bi) {
      const SamBlock& blk = blocks[bi];
      float* t1 = buf[(cur + 1) & 3];       // conv1's output
      float* t2 = buf[(cur + 2) & 3];       // the downsample conv's output
      float* y = buf[(cur + 3) & 3];        // conv2's output, gated in place: the block's result
      const int s = blk.stride;
      const int Ho = (H - 1) / s + 1, Wo = (W - 1) / s + 1;
      const int Cx = blk.in_planes, P = blk.planes;
      const int lo = lvl + (s == 2 ? 1 : 0);
      const float* res = x;
      if (blk.has_sc) {
        WS_LAUNCH(conv(blk.sc, x, Cx, t2, P, H, W, s, 0, ACT_NONE, lo));
        res = t2;
      }
      WS_LAUNCH(conv(blk.c1, x, Cx, t1, P, H, W, s, 1, ACT_RELU, lo));
      WS_LAUNCH(conv(blk.c2, t1, P, y, P, Ho, Wo, 1, 1, ACT_NONE, lo));
      // stats read y once, apply reads y + res and writes the result: 4 tensor passes (+ the slice partials)
      WS_LAUNCH(other(16.0 * B * Ho * (double)Wo * P, st, [&] {
        return launch_simam_residual_relu(y, res, P, y, B, Ho, Wo, P, cur_lens[lo], sm_part, sm_mu, sm_k, st);
      }));
      cur = (cur + 3) & 3;
      x = buf[cur];
      H = Ho; W = Wo;
      lvl = lo;
      if (bi == 0 && (size_t)B * H * W * P <= kTapCap) {
        WS_HIP_CHECK(hipMemcpyAsync(tap_block1, x, (size_t)B * H * W * P * sizeof(float), hipMemcpyDeviceToDevice, st));
        tap_block1_valid = true;
      }
      const bool stop = stop_after == (int)bi + 1;
      if (stop || bi + 1 == blocks.size()) {      // what this block left in the rotation
        tp.n_exec = (int)bi + 1; tp.rows = B * Ho * Wo;
        tp.block = x; tp.block_c = P;
        tp.mid = t1; tp.mid_c = P;
        tp.sc = blk.has_sc ? t2 : nullptr;
        if (stop) return end_chunk(false, B, T, emb, st);
      }
    }
    const int Cl = m * 8, D = stats_dim;             // H = F', W = T' here
    {
      ConvGemmParams g1 = conv2d(asp1, x, Cl, 0, hid, kHidden, 0, B, H, W, 1, 1, 1, 1, 0, 0, ACT_RELU);
      g1.row_len = cur_lens[lvl];
      WS_LAUNCH(gemm(g1, st));
      ConvGemmParams g2 = conv1d(asp2, hid, kHidden, 0, logits, D, 0, B, W, 1, ACT_NONE);
      g2.row_len = cur_lens[lvl];
      WS_LAUNCH(gemm(g2, st));
    }
    WS_LAUNCH(other(4.0 * B * W * (2.0 * D) + 8.0 * B * D, st, [&] {
      return launch_asp_pool(x, logits, B, H, W, Cl, pooled, st, cur_lens[lvl]);
    }));
    WS_LAUNCH(gemm_splitk(conv1d(bott, pooled, 2 * D, 0, emb, embed_dim, 0, B, 1, 1, ACT_NONE), partial, kSplitK, st));
    tp.head_rows = B * W;                      // rows of hid / logits: the last stage's frames
    return end_chunk(true, B, T, emb, st);
  }

  // ws_debug_engine_tap: 'block1' = the first block's output [b][f][t][c] as (B*F*T, in_planes) -- a copy made
  // during the forward, the buffer itself is reused by later blocks.  The last executed block (all of them through
  // ws_debug_engine_stop_after): 'block' = the gated result, 'mid' = conv1's output, 'sc' = the downsample conv's;
  // 'stem' when stopped at 0.  After a full forward: 'hid' (B*T', 128), 'logits' (B*T', D), 'pooled' = the ASP vector
  int tap(const char* tname, float* dst, int64_t cap_floats, int32_t* rows, int32_t* cols, hipStream_t st) override {
    if (int r = tap_guard()) return r;
    const int B = last_chunk.B;
    const BlockTaps& t = block_taps;
    const std::string n = tname;
    char why[200];
    if (n == "block1")
      return tap_copy(tname, tap_block1_valid ? tap_block1 : nullptr,
                      t.n_exec == 0 ? "the last forward was stopped after the stem: no block ran"
                                    : "the chunk's stage-1 map exceeds the tap buffer",
                      B * feat_dim * last_chunk.T, m, dst, cap_floats, rows, cols, st);
    if (n == "hid" || n == "logits" || n == "pooled") {
      std::snprintf(why, sizeof(why), "the last forward was stopped after block %d: the ASP head did not run", t.n_exec);
      if (n == "hid")
        return tap_copy(tname, t.full ? hid : nullptr, why, t.head_rows, kHidden, dst, cap_floats, rows, cols, st);
      if (n == "logits")
        return tap_copy(tname, t.full ? logits : nullptr, why, t.head_rows, stats_dim, dst, cap_floats, rows, cols, st);
      return tap_copy(tname, t.full ? pooled : nullptr, why, B, 2 * stats_dim, dst, cap_floats, rows, cols, st);
    }
    return tap_shared(tname, dst, cap_floats, rows, cols, st,
                      {"block1, stem, block, mid, sc, hid, logits, pooled", nullptr, "downsample"});
  }

  double flops(int batch, int T) const override {
    double macs = 0;
    int H = feat_dim, W = T;
    macs += (double)H * W * 9 * m;
    for (const SamBlock& blk : blocks) {
      const int s = blk.stride, Ho = (H - 1) / s + 1, Wo = (W - 1) / s + 1;
      const double in = blk.in_planes, P = blk.planes;
      macs += (double)Ho * Wo * 9 * in * P + (double)Ho * Wo * 9 * P * P;
      if (blk.has_sc) macs += (double)Ho * Wo * in * P;
      H = Ho; W = Wo;
    }
    macs += 2.0 * W * (double)stats_dim * kHidden;         // the two attention convs
    macs += 2.0 * stats_dim * embed_dim;
    return 2.0 * macs * batch;
  }
};

}  // namespace

Model* make_samresnet(const std::string& model_name, int feat_dim, int embed_dim) {
  for (const SamLayout& l : kSamLayouts)
    if (model_name == l.name) return new SamResNetModel(l, feat_dim, embed_dim);
  return nullptr;
}

}  // namespace wsamd
