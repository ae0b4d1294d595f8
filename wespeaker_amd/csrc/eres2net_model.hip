// ERes2Net34 (Base / Large / aug) speaker-embedding forward -- the hub's eres2net asset -- scheduled onto the gfx950
// kernels.
//
// Reference (file:line in wenet-e2e/wespeaker):
//   wespeaker/models/eres2net.py:44-52     ReLU = Hardtanh(0, 20): every block activation (ACT_RELU20); the stem uses F.relu
//   wespeaker/models/eres2net.py:75-103    AFF (attentional feature fusion)                        -> aff_fuse.hip
//   wespeaker/models/eres2net.py:106-168   BasicBlockERes2Net (layers 1 - 2): 1x1 (stride) -> split chain of 3x3 -> 1x1, += shortcut
//   wespeaker/models/eres2net.py:171-240   BasicBlockERes2Net_diff_AFF (layers 3 - 4): the same, AFF in place of the add
//   wespeaker/models/eres2net.py:243-391   ERes2Net (4 stages, 3 stride-2 downsample convs, 3 global AFFs, TSTP, seg_1 [seg_2])
//   wespeaker/models/eres2net.py:394-430   the three constructors
//
// Layout, BN folding, the zero-padded activation buffers, the seg_1 / seg_2 head and the shared taps: cnn2d_base.h.  A
// block keeps conv1's output (`mid`, width * scale channels) and the concat that conv3 reads (`cat`) as two buffers of
// that row width: branch i reads the channel slice i of mid (ConvGemmParams::a_off) plus -- layers 1 - 2, i >= 1 --
// slice i - 1 of cat through ConvGemmParams::A2, and writes slice i of cat (d_off); in layers 3 - 4 aff_fuse blends
// slice i - 1 of cat with slice i of mid into a width-wide scratch that the branch convolution reads.  The global
// fusions run as soon as their inputs exist (fuse12 right after layer 2, ...): same values, shorter lifetimes.
#include "cnn2d_base.h"

#include <algorithm>

namespace wsamd {

namespace {

struct ERes2Layout { const char* name; int m, base_width, scale, expansion; };
const ERes2Layout kERes2Layouts[] = {
    {"ERes2Net34_Base", 32, 32, 2, 2},
    {"ERes2Net34_Large", 64, 32, 2, 2},
    {"ERes2Net34_aug", 64, 24, 3, 4},
};
const int kERes2Blocks[4] = {3, 4, 6, 3};

struct AffW { ConvW l1, l2; int C = 0; };      // local_att.0 + .1 folded, local_att.3 + .4 folded

struct ERes2Block {
  ConvW c1, c3, sc;
  std::vector<ConvW> br;                       // the scale branch convolutions (AFF blocks: conv2_1, then convs.*)
  std::vector<AffW> aff;                       // AFF blocks: scale - 1 of them
  bool has_sc = false, fuse = false;
  int stride = 1, in_planes = 0, planes = 0, width = 0, stage = 0;
};

struct ERes2NetModel : Cnn2dBase {
  ERes2Layout lay;
  std::vector<ERes2Block> blocks;
  ConvW down[3];
  AffW gfuse[3];
  // the fourteen activation buffers (Cnn2dBase::buf, carved in this order): the stage outputs L[0..3], the block ping-pong
  // P[0..1], conv1's output, the concat, the shortcut's output, the AFF scratch, the downsample output, the three global
  // fusions
  enum { B_L0 = 0, B_P0 = 4, B_MID = 6, B_CAT = 7, B_SC = 8, B_SP = 9, B_DS = 10, B_F0 = 11 };
  // taps of the last chunk beyond Cnn2dBase::BlockTaps
  const float* tap_cat = nullptr;
  int tap_cat_c = 0;
  int fuse_rows[3] = {0, 0, 0};

  ERes2NetModel(const ERes2Layout& l, int fd, int ed) : Cnn2dBase(l.name, fd, ed), lay(l) {}

  bool wants(const std::string& key) const override {
    return wants_prefixes(key, {"conv1.", "bn1.", "layer1.", "layer2.", "layer3.", "layer4.", "layer1_downsample.",
                                "layer2_downsample.", "layer3_downsample.", "fuse_mode12.", "fuse_mode123.",
                                "fuse_mode1234.", "seg_1.", "seg_bn_1.", "seg_2."});
  }

  int set_precision(int mode) override {
    return mode == 2 ? no_f16io_backend("its AFF kernel is") : ModelBase::set_precision(mode);
  }

  // AFF(channels = C): Conv2d(2C -> C/4, 1x1, bias) + BN, SiLU, Conv2d(C/4 -> C, 1x1, bias) + BN   (eres2net.py:81-95)
  int pack_aff(const SD& sd, const std::string& p, int C, AffW* out) {
    if (C < 64 || C > 2048 || C % 32) {
      set_error("%s: '%s' fuses %d channels; the AFF kernel takes multiples of 32 in [64, 2048]", name.c_str(), p.c_str(), C);
      return WS_ERR_SHAPE;
    }
    const int H = C / 4;
    out->C = C;
    int err = pack_conv(sd, p + ".local_att.0", {H, 2 * C, 1, 1}, H, 2 * C, 1, 1,
                        [=](int n, int, int ci) { return (size_t)n * 2 * C + ci; }, true, p + ".local_att.1", "", &out->l1);
    if (err) return err;
    return pack_conv(sd, p + ".local_att.3", {C, H, 1, 1}, C, H, 1, 1,
                     [=](int n, int, int ci) { return (size_t)n * H + ci; }, true, p + ".local_att.4", "", &out->l2);
  }

  int finalize(const SD& sd, int max_batch, int max_frames) override {
    int err = 0;
    if (feat_dim % 8) {
      set_error("%s needs feat_dim %% 8 == 0, got %d", name.c_str(), feat_dim);
      return WS_ERR_INVALID_ARG;
    }
    auto it = sd.find("conv1.weight");
    if (it == sd.end()) {
      set_error("missing tensor 'conv1.weight' for model %s", name.c_str());
      return WS_ERR_MISSING_TENSOR;
    }
    const int m = lay.m, E = lay.expansion;
    const int got = it->second.shape.empty() ? 0 : (int)it->second.shape[0];
    if (got != m) {
      set_error("%s: conv1.weight has %d output channels, the name stands for m_channels = %d (ERes2Net34_Base 32, "
                "ERes2Net34_Large / ERes2Net34_aug 64)", name.c_str(), got, m);
      return WS_ERR_SHAPE;
    }
    if ((err = pack_stem3x3(sd, "conv1", "bn1", m, &stem_w, &stem_b))) return err;      // Conv2d(1, m, 3x3) + bn1
    int in_planes = m;
    for (int s = 0; s < 4; ++s) {
      const int planes = m << s;
      const int width = planes * lay.base_width / 64;            // floor(planes * baseWidth / 64)
      for (int b = 0; b < kERes2Blocks[s]; ++b) {
        ERes2Block blk;
        blk.stage = s; blk.fuse = s >= 2;
        blk.stride = (b == 0 && s > 0) ? 2 : 1;
        blk.in_planes = in_planes; blk.planes = planes; blk.width = width;
        const std::string p = "layer" + std::to_string(s + 1) + "." + std::to_string(b);
        if ((err = pack_conv2d(sd, p + ".conv1", width * lay.scale, in_planes, 1, 1, p + ".bn1", &blk.c1))) return err;
        blk.br.resize(lay.scale);
        for (int i = 0; i < lay.scale; ++i) {
          std::string cn, bn;
          if (!blk.fuse) { cn = p + ".convs." + std::to_string(i); bn = p + ".bns." + std::to_string(i); }
          else if (i == 0) { cn = p + ".conv2_1"; bn = p + ".bn2_1"; }
          else { cn = p + ".convs." + std::to_string(i - 1); bn = p + ".bns." + std::to_string(i - 1); }
          if ((err = pack_conv2d(sd, cn, width, width, 3, 3, bn, &blk.br[i]))) return err;
        }
        if (blk.fuse) {
          blk.aff.resize(lay.scale - 1);
          for (int i = 0; i + 1 < lay.scale; ++i)
            if ((err = pack_aff(sd, p + ".fuse_models." + std::to_string(i), width, &blk.aff[i]))) return err;
        }
        if ((err = pack_conv2d(sd, p + ".conv3", planes * E, width * lay.scale, 1, 1, p + ".bn3", &blk.c3))) return err;
        if (blk.stride != 1 || in_planes != planes * E) {
          blk.has_sc = true;
          if ((err = pack_conv2d(sd, p + ".shortcut.0", planes * E, in_planes, 1, 1, p + ".shortcut.1", &blk.sc)))
            return err;
        }
        in_planes = planes * E;
        blocks.push_back(blk);
      }
    }
    n_stops = (int)blocks.size();
    static const char* fnames[3] = {"fuse_mode12", "fuse_mode123", "fuse_mode1234"};
    for (int k = 0; k < 3; ++k) {
      const int cin = m * E << k, cout = cin * 2;
      const std::string dn = "layer" + std::to_string(k + 1) + "_downsample";
      if ((err = pack_conv2d(sd, dn, cout, cin, 3, 3, "", &down[k]))) return err;
      if ((err = pack_aff(sd, fnames[k], cout, &gfuse[k]))) return err;
    }
    stats_dim = (feat_dim / 8) * m * 8 * E;                      // eres2net.py:261,326-327
    if ((err = pack_seg_head(sd))) return err;
    if ((err = upload_weights())) return err;
    return reserve(max_batch, max_frames);
  }

  int stage_c(int s) const { return (lay.m * lay.expansion) << s; }           // channels of a stage's output
  int stage_w(int s) const { return (lay.m << s) * lay.base_width / 64; }     // branch width of a stage

  int reserve(int max_batch, int max_frames) override {
    int err = 0;
    begin_reserve(max_batch, max_frames);
    tap_cat = nullptr; tap_cat_c = 0;
    auto map = [&](int s, int c) { return (size_t)maxB * level_len(feat_dim, s) * level_len(maxT, s) * (size_t)c; };
    size_t big = 0, mid = 0, sp = 0;
    for (int s = 0; s < 4; ++s) {
      big = std::max(big, map(s, stage_c(s)));
      // a stage's first block reads the previous level, its conv1 already writes this one (the stride sits on it)
      mid = std::max(mid, map(s, stage_w(s) * lay.scale));
      if (s >= 2) sp = std::max(sp, map(s, stage_w(s)));
    }
    big = std::max(big, map(0, lay.m));
    if ((err = refuse_map_too_large(big)) || (err = refuse_batch_too_large())) return err;
    Carve cv = begin_carve();
    for (int s = 0; s < 4; ++s) buf.carve(cv, map(s, stage_c(s)));                 // B_L0 + s
    // B_P0, B_P0 + 1, B_MID, B_CAT, B_SC, B_SP, B_DS
    for (size_t c : {big, big, mid, mid, big, sp, map(1, stage_c(1))}) buf.carve(cv, c);
    for (int k = 0; k < 3; ++k) buf.carve(cv, map(k + 1, stage_c(k + 1)));         // B_F0 + k
    return alloc_with_seg_head(cv);
  }

  // TSTP's unbiased variance needs two frames at the last stage: 9 -> 5 -> 3 -> 2
  int min_frames() const override { return 9; }

  hipError_t aff(const AffW& w, const float* x, int ldx, int x_off, const float* y, int ldy, int y_off, float* out,
                 int ldo, int o_off, int M, int HW, int W, const int* row_len, hipStream_t st) {
    AffFuseParams p;
    std::memset(&p, 0, sizeof(p));
    p.x = x; p.ldx = ldx; p.x_off = x_off;
    p.y = y; p.ldy = ldy; p.y_off = y_off;
    p.out = out; p.ldo = ldo; p.o_off = o_off;
    p.W1 = arena.at(w.l1.w); p.ldw1 = w.l1.ldw; p.b1 = arena.at(w.l1.b);
    p.W2 = arena.at(w.l2.w); p.ldw2 = w.l2.ldw; p.b2 = arena.at(w.l2.b);
    p.M = M; p.C = w.C;
    p.row_len = row_len; p.HW = HW; p.W = W;
    // compulsory bytes: read two, write one
    return other(12.0 * M * (double)w.C, st, [&] { return launch_aff_fuse(p, st); });
  }

  int forward_chunk(const float* feats, int B, int T, float* emb, hipStream_t st) override {
    if (gemm_precision == 2) return no_f16io_backend();      // (set_precision refuses it)
    BlockTaps& tp = begin_chunk();             // host-side notes for ws_debug_engine_tap, readable when the chunk ends
    tap_cat = nullptr; tap_cat_c = 0;
    const int m = lay.m, SC = lay.scale;
    int H = feat_dim, W = T, lvl = 0;
    float* x = buf[B_P0];
    WS_LAUNCH(other(4.0 * B * H * (double)W * (m + 1), st, [&] {
      return launch_stem_conv3x3_any(feats, B, T, feat_dim, arena.at(stem_w), arena.at(stem_b), m, x, st, cur_lens[0]);
    }));
    tp.n_exec = 0; tp.stem = x; tp.stem_rows = B * H * W; tp.stem_c = m;
    if (stop_after == 0) return end_chunk(false, B, T, emb, st);
    auto conv = [&](const ConvW& cw, const float* in, int lda, int a_off, float* out, int ldd, int d_off, int Hin_,
                    int Win_, int s_, int pad, int act, int out_lvl) {
      ConvGemmParams p = conv2d(cw, in, lda, a_off, out, ldd, d_off, B, Hin_, Win_, s_, s_, 1, 1, pad, pad, act);
      p.row_len = cur_lens[out_lvl];                       // stride level of this launch's OUTPUT width
      p.a_zero_off = buf.zero_off_for(in, cw.Cin);         // the zero pad behind the input's buffer
      return p;
    };
    float* const mid = buf[B_MID];
    float* const cat = buf[B_CAT];
    float* const scb = buf[B_SC];
    float* const sp = buf[B_SP];
    for (size_t bi = 0; bi < blocks.size(); ++bi) {
      const ERes2Block& blk = blocks[bi];
      const bool last_of_stage = bi + 1 == blocks.size() || blocks[bi + 1].stage != blk.stage;
      // a stage's last block leaves its result in the stage buffer, the others ping-pong
      float* out = last_of_stage ? buf[B_L0 + blk.stage] : (x == buf[B_P0] ? buf[B_P0 + 1] : buf[B_P0]);
      const int s = blk.stride;
      const int Ho = (H - 1) / s + 1, Wo = (W - 1) / s + 1;
      const int Cx = blk.in_planes, Co = blk.planes * lay.expansion, w = blk.width, ws_ = w * SC;
      const int lo = lvl + (s == 2 ? 1 : 0);
      const int M = B * Ho * Wo;
      const float* res = x;
      if (blk.has_sc) {
        WS_LAUNCH(gemm(conv(blk.sc, x, Cx, 0, scb, Co, 0, H, W, s, 0, ACT_NONE, lo), st));
        res = scb;
      }
      WS_LAUNCH(gemm(conv(blk.c1, x, Cx, 0, mid, ws_, 0, H, W, s, 0, ACT_RELU20, lo), st));
      for (int i = 0; i < SC; ++i) {
        if (blk.fuse && i >= 1) {
          // sp = AFF(previous branch output, spx[i])   (eres2net.py:228)
          WS_LAUNCH(aff(blk.aff[i - 1], cat, ws_, (i - 1) * w, mid, ws_, i * w, sp, w, 0, M, Ho * Wo, Wo, cur_lens[lo], st));
          WS_LAUNCH(gemm(conv(blk.br[i], sp, w, 0, cat, ws_, i * w, Ho, Wo, 1, 1, ACT_RELU20, lo), st));
          continue;
        }
        ConvGemmParams p = conv(blk.br[i], mid, ws_, i * w, cat, ws_, i * w, Ho, Wo, 1, 1, ACT_RELU20, lo);
        if (i >= 1) { p.A2 = cat; p.lda2 = ws_; p.a2_off = (i - 1) * w; }      // sp = sp + spx[i]   (eres2net.py:153)
        WS_LAUNCH(gemm(p, st));
      }
      {
        ConvGemmParams p = conv(blk.c3, cat, ws_, 0, out, Co, 0, Ho, Wo, 1, 0, ACT_RELU20, lo);
        p.residual = res; p.ldr = Co; p.r_off = 0;
        WS_LAUNCH(gemm(p, st));
      }
      x = out;
      H = Ho; W = Wo; lvl = lo;
      const bool stop = stop_after == (int)bi + 1;
      if (stop || bi + 1 == blocks.size()) {      // what this block left
        tp.n_exec = (int)bi + 1; tp.rows = M;
        tp.block = x; tp.block_c = Co;
        tp.mid = mid; tp.mid_c = ws_;
        tp.sc = blk.has_sc ? scb : nullptr;
        tap_cat = cat; tap_cat_c = ws_;
        if (stop) return end_chunk(false, B, T, emb, st);
      }
      if (last_of_stage && blk.stage >= 1) {
        // bottom-up fusion (eres2net.py:361-368): fuse_k = AFF(out_k, downsample(previous)), previous = out1 / fuse12 / fuse123
        const int k = blk.stage - 1;
        const float* prev = k == 0 ? buf[B_L0] : buf[B_F0 + k - 1];
        const int Hp = level_len(feat_dim, k), Wp = level_len(T, k), Cp = stage_c(k);
        WS_LAUNCH(gemm(conv(down[k], prev, Cp, 0, buf[B_DS], Co, 0, Hp, Wp, 2, 1, ACT_NONE, lo), st));
        WS_LAUNCH(aff(gfuse[k], x, Co, 0, buf[B_DS], Co, 0, buf[B_F0 + k], Co, 0, M, H * W, W, cur_lens[lo], st));
        fuse_rows[k] = M;
      }
    }
    // pooling and the head read the last global fusion   (eres2net.py:370-389)
    return pool_and_head(buf[B_F0 + 2], stage_c(3), B, H, W, lvl, T, emb, st);
  }

  // ws_debug_engine_tap: 'stem' when stopped at 0; of the last executed block 'block' (its output), 'mid' (conv1's
  // output, width * scale), 'cat' (the concat conv3 reads) and 'sc' (the shortcut convolution's output); after a full
  // forward 'fuse12' / 'fuse123' / 'fuse1234' (the global fusions, [b][f][t][c] rows), 'pooled' and -- two-embedding
  // models -- 'emb_a' (seg_1's output after its relu + seg_bn_1 epilogue, what seg_2 reads)
  int tap(const char* tname, float* dst, int64_t cap_floats, int32_t* rows, int32_t* cols, hipStream_t st) override {
    if (int r = tap_guard()) return r;
    const BlockTaps& t = block_taps;
    const std::string n = tname;
    char why[200];
    if (n == "cat")                            // (null only when no block ran)
      return tap_copy(tname, tap_cat, "the last forward was stopped after the stem: no block ran", t.rows, tap_cat_c, dst,
                      cap_floats, rows, cols, st);
    std::snprintf(why, sizeof(why), "the last forward was stopped after block %d: the global fusions, pooling and the "
                  "head did not run", t.n_exec);
    for (int k = 0; k < 3; ++k) {
      static const char* fn[3] = {"fuse12", "fuse123", "fuse1234"};
      if (n == fn[k])
        return tap_copy(tname, t.full ? buf[B_F0 + k] : nullptr, why, fuse_rows[k], stage_c(k + 1), dst, cap_floats, rows,
                        cols, st);
    }
    return tap_shared(tname, dst, cap_floats, rows, cols, st,
                      {"stem, block, mid, cat, sc, fuse12, fuse123, fuse1234, pooled, emb_a", why});
  }

  double flops(int batch, int T) const override {
    double macs = 0;
    int H = feat_dim, W = T;
    macs += (double)H * W * 9 * lay.m;
    auto aff_macs = [](double C) { return 2.0 * C * (C / 4) + C * (C / 4); };
    for (const ERes2Block& blk : blocks) {
      const int s = blk.stride, Ho = (H - 1) / s + 1, Wo = (W - 1) / s + 1;
      const double px = (double)Ho * Wo, in = blk.in_planes, w = blk.width, ws_ = w * lay.scale,
                   Co = (double)blk.planes * lay.expansion;
      macs += px * in * ws_ + px * 9 * w * w * lay.scale + px * ws_ * Co;
      if (blk.fuse) macs += px * aff_macs(w) * (lay.scale - 1);
      if (blk.has_sc) macs += px * in * Co;
      H = Ho; W = Wo;
    }
    for (int k = 0; k < 3; ++k) {
      const double px = (double)level_len(feat_dim, k + 1) * level_len(T, k + 1), cin = stage_c(k), cout = stage_c(k + 1);
      macs += px * 9 * cin * cout + px * aff_macs(cout);
    }
    return 2.0 * (macs + seg_head_macs()) * batch;
  }
};

}  // namespace

Model* make_eres2net(const std::string& model_name, int feat_dim, int embed_dim) {
  for (const ERes2Layout& l : kERes2Layouts)
    if (model_name == l.name) return new ERes2NetModel(l, feat_dim, embed_dim);
  return nullptr;
}

}  // namespace wsamd
