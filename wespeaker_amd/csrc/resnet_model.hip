// ResNet speaker-embedding forward (ResNet18/34/50/101/152/221/293) scheduled onto the gfx950
// kernels.
//
// Reference (file:line in wenet-e2e/wespeaker):
//   wespeaker/models/resnet.py:110-204  ResNet (conv1+bn1+relu, 4 stages, TSTP, seg_1 [, seg_bn_1, seg_2])
//   wespeaker/models/resnet.py:35-69    BasicBlock;  :72-107 Bottleneck (stride on the 3x3)
//   wespeaker/models/resnet.py:207-260  ctor names
//   wespeaker/models/pooling_layers.py:78-85 TSTP
//
// Layout, BN folding, the zero-padded activation buffers, the seg_1 / seg_2 head and the shared taps: cnn2d_base.h.  The
// residual add and ReLU live in the GEMM epilogue.
#include "cnn2d_base.h"

namespace wsamd {

namespace {

struct Layout { const char* name; bool bottleneck; int blocks[4]; };
const Layout kLayouts[] = {
    {"ResNet18", false, {2, 2, 2, 2}},   {"ResNet34", false, {3, 4, 6, 3}},
    {"ResNet50", true, {3, 4, 6, 3}},    {"ResNet101", true, {3, 4, 23, 3}},
    {"ResNet152", true, {3, 8, 36, 3}},  {"ResNet221", true, {6, 16, 48, 3}},
    {"ResNet293", true, {10, 20, 64, 3}},
};

struct Block {
  ConvW c1, c2, c3, sc;
  bool has_sc = false;
  int stride = 1, in_planes = 0, planes = 0;
};

struct ResNetModel : Cnn2dBase {
  Layout lay;
  int exp = 1;
  std::vector<Block> blocks;                 // (the four rotating activation buffers: Cnn2dBase::buf)

  ResNetModel(const Layout& l, int fd, int ed) : Cnn2dBase(l.name, fd, ed), lay(l) {
    exp = l.bottleneck ? 4 : 1;
  }

  bool wants(const std::string& key) const override {
    return wants_prefixes(key, {"conv1.", "bn1.", "layer1.", "layer2.", "layer3.", "layer4.", "seg_1.", "seg_bn_1.",
                                "seg_2."});
  }

  int finalize(const SD& sd, int max_batch, int max_frames) override {
    int err = 0;
    const int m = 32;
    if (feat_dim % 8) {
      set_error("ResNet needs feat_dim %% 8 == 0, got %d", feat_dim);
      return WS_ERR_INVALID_ARG;
    }
    if ((err = pack_stem3x3(sd, "conv1", "bn1", m, &stem_w, &stem_b))) return err;      // Conv2d(1, 32, 3x3) + bn1
    int in_planes = m;
    for (int s = 0; s < 4; ++s) {
      const int planes = m << s;
      for (int b = 0; b < lay.blocks[s]; ++b) {
        Block blk;
        blk.stride = (b == 0 && s > 0) ? 2 : 1;
        blk.in_planes = in_planes; blk.planes = planes;
        const std::string p = "layer" + std::to_string(s + 1) + "." + std::to_string(b);
        if (lay.bottleneck) {
          if ((err = pack_conv2d(sd, p + ".conv1", planes, in_planes, 1, 1, p + ".bn1", &blk.c1))) return err;
          if ((err = pack_conv2d(sd, p + ".conv2", planes, planes, 3, 3, p + ".bn2", &blk.c2))) return err;
          if ((err = pack_conv2d(sd, p + ".conv3", planes * 4, planes, 1, 1, p + ".bn3", &blk.c3))) return err;
        } else {
          if ((err = pack_conv2d(sd, p + ".conv1", planes, in_planes, 3, 3, p + ".bn1", &blk.c1))) return err;
          if ((err = pack_conv2d(sd, p + ".conv2", planes, planes, 3, 3, p + ".bn2", &blk.c2))) return err;
        }
        if (blk.stride != 1 || in_planes != planes * exp) {
          blk.has_sc = true;
          if ((err = pack_conv2d(sd, p + ".shortcut.0", planes * exp, in_planes, 1, 1,
                                 p + ".shortcut.1", &blk.sc)))
            return err;
        }
        in_planes = planes * exp;
        blocks.push_back(blk);
      }
    }
    n_stops = (int)blocks.size();
    stats_dim = (feat_dim / 8) * m * 8 * exp;          // C_last * F_last   (resnet.py:123)
    if ((err = pack_seg_head(sd))) return err;
    if ((err = upload_weights())) return err;
    return reserve(max_batch, max_frames);
  }

  int reserve(int max_batch, int max_frames) override {
    begin_reserve(max_batch, max_frames);
    // largest activation: stage-1 output (F x T x 32*exp); scratch planes are never larger
    // (below 2^31 elements: ~4200 x 2 s utterances for BasicBlock nets, ~1060 for Bottleneck nets)
    const size_t act = (size_t)maxB * feat_dim * maxT * (size_t)(32 * exp);
    if (int err = refuse_map_too_large(act)) return err;
    Carve cv = begin_carve();
    for (int i = 0; i < 4; ++i) buf.carve(cv, act);          // the block rotation
    return alloc_with_seg_head(cv);
  }

  int min_frames() const override { return 2; }

  int forward_chunk(const float* feats, int B, int T, float* emb, hipStream_t st) override {
    int H = feat_dim, W = T;
    // ragged chunk: the time axis of utterance b holds cur_lens[level][b] valid columns at stride level
    // `level`; every convolution stores zeros beyond them (row_len), TSTP runs over the valid columns
    int lvl = 0;
    // f16 back-end: every activation map lives in HBM as binary16 only (same buffers, half used);
    // all convolutions then run on the LDS-DMA kernel (conv form), residuals are read as halfs
    const bool f16io = gemm_precision == 2;
    float* x = buf[0];
    BlockTaps& tp = begin_chunk();             // host-side notes for ws_debug_engine_tap, readable when the chunk ends
    WS_LAUNCH(other(4.0 * B * H * (double)W * 33, st, [&] {
      return launch_stem_conv3x3(feats, B, T, feat_dim, arena.at(stem_w), arena.at(stem_b), 32, x, st,
                                 f16io ? reinterpret_cast<uint16_t*>(x) : nullptr, cur_lens[0]);
    }));
    tp.half = f16io;
    tp.n_exec = 0; tp.stem = x; tp.stem_rows = B * H * W; tp.stem_c = 32;
    if (stop_after == 0) return end_chunk(false, B, T, emb, st);
    // in -> out convolution with the optional residual, in the tensor format of the active back-end
    auto conv = [&](const ConvW& cw, const float* in, int Cin_, float* out, int Cout_, int Hin_, int Win_,
                    int s_, int pad, int act, const float* res, int ldr, int out_lvl) {
      ConvGemmParams p = conv2d(cw, in, Cin_, 0, out, Cout_, 0, B, Hin_, Win_, s_, s_, 1, 1, pad, pad, act);
      p.row_len = cur_lens[out_lvl];                       // stride level of this launch's OUTPUT width
      p.a_zero_off = buf.zero_off_for(in, Cin_);           // the zero pad behind the input's buffer
      if (f16io) {
        p.A16 = reinterpret_cast<const uint16_t*>(in); p.lda16 = Cin_;
        p.D = nullptr; p.D16 = reinterpret_cast<uint16_t*>(out); p.ldd16 = Cout_;
        if (res) { p.residual16 = reinterpret_cast<const uint16_t*>(res); p.ldr = ldr; p.r_off = 0; }
      } else if (res) {
        p.residual = res; p.ldr = ldr; p.r_off = 0;
      }
      return gemm(p, st);
    };
    int cur = 0;          // index of the buffer holding x
    bool have_y1 = false; // the current block's conv1 output already lies in buf[y1_idx] (written by the previous block)
    int y1_idx = 0;
    for (size_t bi = 0; bi < blocks.size(); ++bi) {
      const Block& blk = blocks[bi];
      // buffer roles of this block: x = buf[cur]; y1 (conv1's output, later the block's result) = buf[ia]; the spare
      // one (shortcut output, or the NEXT block's y1 when conv3 is fused with its conv1) = buf[ic]; y2 = buf[ib].
      // Without a y1 handed over by the previous block this is the plain rotation cur + 1 / + 2 / + 3.
      const int ia = (lay.bottleneck && have_y1) ? y1_idx : (cur + 1) & 3;
      int rest[2], nrest = 0;
      for (int k = 1; k <= 3; ++k)
        if (((cur + k) & 3) != ia) rest[nrest++] = (cur + k) & 3;
      const int ic = rest[0], ib = rest[1];
      float* t1 = buf[ia];
      float* t2 = buf[ic];
      float* out = buf[ib];
      const int s = blk.stride;
      const int Ho = (H - 1) / s + 1, Wo = (W - 1) / s + 1;
      const int Cx = blk.in_planes, P = blk.planes, Co = P * exp;
      const int lo = lvl + (s == 2 ? 1 : 0);               // stride level of the block's output
      const float* res = x;
      int ldr = Cx;
      if (blk.has_sc) {     // 1x1 stride-s conv + BN on the block input
        WS_LAUNCH(conv(blk.sc, x, Cx, t2, Co, H, W, s, 0, ACT_NONE, nullptr, 0, lo));
        res = t2;
        ldr = Co;
      }
      if (lay.bottleneck) {
        if (!have_y1) WS_LAUNCH(conv(blk.c1, x, Cx, t1, P, H, W, 1, 0, ACT_RELU, nullptr, 0, lvl));
        have_y1 = false;                // (else: the previous block's fused launch left this block's y1 in buf[ia])
        WS_LAUNCH(conv(blk.c2, t1, P, out, P, H, W, s, 1, ACT_RELU, nullptr, 0, lo));
        // conv3 (+ residual, ReLU) of this block and conv1 (+ ReLU) of the next one in ONE pass over the block output
        // (bneck_fuse.hip): fp32, 32 / 64 planes, the next block with the same or twice the planes
        // (its conv1 has no stride: a block's stride sits in conv2).  The next block's y1 goes into the one buffer that
        // is dead by now: the spare one, or -- when this block has a shortcut convolution, whose output IS the spare
        // one -- the block's own input x (read by conv1 and the shortcut only)
        const Block* nb = bi + 1 < blocks.size() ? &blocks[bi + 1] : nullptr;
        BneckFuseParams fp = {};
        if (gemm_precision == 0 && nb && (nb->planes == P || nb->planes == 2 * P) && nb->in_planes == Co &&
            blk.c3.has_b && nb->c1.has_b && !blk.c3.has_post && !nb->c1.has_post) {
          fp.y2 = out; fp.W3 = arena.at(blk.c3.w); fp.ldw3 = blk.c3.ldw; fp.b3 = arena.at(blk.c3.b);
          fp.res = res; fp.ldr = ldr; fp.out = t1;
          fp.W1 = arena.at(nb->c1.w); fp.ldw1 = nb->c1.ldw; fp.b1 = arena.at(nb->c1.b);
          fp.y1 = blk.has_sc ? buf[cur] : t2;
          fp.M = B * Ho * Wo; fp.P = P; fp.PN = nb->planes;
          fp.row_len = cur_lens[lo]; fp.HW = Ho * Wo; fp.W = Wo;      // (a ragged chunk: null otherwise)
        }
        if (fp.y2 && bneck_fuse_supported(fp)) {
          const double M_ = (double)fp.M;
          if (prof.enabled) prof.begin(0, 2.0 * M_ * (P * (double)Co + Co * (double)P), 4.0 * M_ * (P + 2.0 * Co + P), st);
          hipError_t fe = launch_bneck_fuse(fp, st);
          prof.end(st);
          WS_LAUNCH(fe);
          have_y1 = true;
          y1_idx = blk.has_sc ? cur : ic;
        } else {
          WS_LAUNCH(conv(blk.c3, out, P, t1, Co, Ho, Wo, 1, 0, ACT_RELU, res, ldr, lo));
        }
        cur = ia;                       // result in t1
      } else {
        WS_LAUNCH(conv(blk.c1, x, Cx, t1, P, H, W, s, 1, ACT_RELU, nullptr, 0, lo));
        WS_LAUNCH(conv(blk.c2, t1, P, out, Co, Ho, Wo, 1, 1, ACT_RELU, res, ldr, lo));
        cur = (cur + 3) & 3;            // result in out
      }
      x = buf[cur];
      H = Ho; W = Wo;
      lvl = lo;
      const bool stop = stop_after == (int)bi + 1;
      if (stop || bi + 1 == blocks.size()) {      // what this block left in the rotation (see the roles above)
        tp.n_exec = (int)bi + 1; tp.rows = B * Ho * Wo;
        tp.block = x; tp.block_c = Co;
        tp.mid = lay.bottleneck ? out : t1; tp.mid_c = P;
        tp.sc = blk.has_sc ? t2 : nullptr;
        tp.next_y1 = have_y1 ? buf[y1_idx] : nullptr;
        tp.next_c = have_y1 ? blocks[bi + 1].planes : 0;
        if (stop) return end_chunk(false, B, T, emb, st);
      }
    }
    const int Cl = 256 * exp;           // channels of the last stage
    return pool_and_head(x, Cl, B, H, W, lvl, T, emb, st);
  }

  // ws_debug_engine_tap: what the last chunk's last executed block left in the four rotating buffers and the head's
  // tensors after a full forward (Cnn2dBase::tap_shared), and 'next_y1': the next block's conv1 output when the block's
  // conv3 ran fused with it
  int tap(const char* tname, float* dst, int64_t cap_floats, int32_t* rows, int32_t* cols, hipStream_t st) override {
    if (int r = tap_guard()) return r;
    const BlockTaps& t = block_taps;
    char why[200];
    if (!std::strcmp(tname, "next_y1")) {
      if (t.n_exec < 1) std::snprintf(why, sizeof(why), "the last forward was stopped after the stem: no block ran");
      else std::snprintf(why, sizeof(why), "block %d did not run the fused conv3 + next-conv1 kernel (bneck_c3c1): the "
                         "next block's conv1 has not run", t.n_exec);
      return tap_map(tname, t.next_y1, why, t.rows, t.next_c, dst, cap_floats, rows, cols, st);
    }
    std::snprintf(why, sizeof(why), "the last forward was stopped after block %d: pooling and the head did not run",
                  t.n_exec);
    return tap_shared(tname, dst, cap_floats, rows, cols, st, {"stem, block, mid, sc, next_y1, pooled, emb_a", why});
  }

  double flops(int batch, int T) const override {
    double macs = 0;
    int H = feat_dim, W = T;
    macs += (double)H * W * 9 * 32;
    for (const Block& blk : blocks) {
      const int s = blk.stride, Ho = (H - 1) / s + 1, Wo = (W - 1) / s + 1;
      const double in = blk.in_planes, P = blk.planes, Co = P * exp;
      if (lay.bottleneck)
        macs += (double)H * W * in * P + (double)Ho * Wo * 9 * P * P + (double)Ho * Wo * P * Co;
      else
        macs += (double)Ho * Wo * 9 * in * P + (double)Ho * Wo * 9 * P * P;
      if (blk.has_sc) macs += (double)Ho * Wo * in * Co;
      H = Ho; W = Wo;
    }
    return 2.0 * (macs + seg_head_macs()) * batch;
  }
};

}  // namespace

Model* make_resnet(const std::string& model_name, int feat_dim, int embed_dim) {
  for (const Layout& l : kLayouts)
    if (model_name == l.name) return new ResNetModel(l, feat_dim, embed_dim);
  return nullptr;
}

}  // namespace wsamd
