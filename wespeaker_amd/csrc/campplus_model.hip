// CAM++ (CAMPPlus) forward scheduled onto the gfx950 kernels.
//
// Reference (file:line in wenet-e2e/wespeaker):
//   wespeaker/models/campplus.py:333-413  CAMPPlus (FCM head -> TDNN k5 s2 -> 3 dense blocks
//                                         (12/24/16 layers, dilation 1/2/2) + transit -> BN-ReLU ->
//                                         TSTP -> dense 1x1 + BN(affine=False))
//   wespeaker/models/campplus.py:282-330  FCM;  :245-279 BasicResBlock (freq-only stride (2,1))
//   wespeaker/models/campplus.py:138-170  CAMDenseTDNNLayer;  :86-135 CAMLayer
//
// Layout: channels-last everywhere.  FCM activations are [b][f][t][c]; its (B, C*F', T) reshape
// is never materialised: the TDNN layer is run as a (kh = F', kw = 5) convolution over the
// (F' x T) image with the weight re-indexed on the host.  A dense block owns ONE [B*T'][Cmax] buffer
// and every layer appends its 32 channels at a channel offset (concat-free).  Pre-activation
// BN-ReLU (CAM++ is BN -> ReLU -> conv) is applied while the GEMM stages its A operand; BN that
// directly follows a conv is folded into the weights; the context mask multiplies in the epilogue.
#include <cstdint>
#include "model_common.h"

namespace wsamd {

namespace {

struct ResBlk { ConvW c1, c2, sc; bool has_sc = false; int stride = 1; };
struct DenseLayerW {
  size_t pre_s = 0, pre_b = 0;        // nonlinear1 BN (on the layer input)
  ConvW lin1;                         // 1x1 Cin -> 128, nonlinear2 BN folded, ReLU
  ConvW local;                        // k3 dilated 128 -> 32
  size_t cw1 = 0, cb1 = 0, cw2 = 0, cb2 = 0;   // context FCs 128 -> 64 -> 32
  int cin = 0;
};
struct Transit { size_t pre_s = 0, pre_b = 0; ConvW lin; int cin = 0; };

struct CamppModel : ModelBase {
  size_t stem_w = 0, stem_b = 0;
  ResBlk res[4];
  ConvW head_conv2, tdnn, dense;
  std::vector<DenseLayerW> layers[3];
  Transit transit[3];
  size_t out_s = 0, out_b = 0;
  int fprime = 10;
  static constexpr int kLayers[3] = {12, 24, 16};
  static constexpr int kDil[3] = {1, 2, 2};
  static constexpr int kSplitK = 8;
  float *fa = nullptr, *fb = nullptr, *fc = nullptr, *xbuf = nullptr, *xbuf2 = nullptr, *hbuf = nullptr,
        *mask = nullptr, *pooled = nullptr, *partial = nullptr, *colsum = nullptr;
  int max_segs = 1;
  // ---- debug stop points and taps (ws_debug_engine_stop_after / ws_debug_engine_tap).  Stage numbering: 0 = the stem,
  // 1..4 = the FCM residual blocks, 5 = head.conv2, 6 = the TDNN layer, 7 / 8 / 9 = dense block 1 / 2 / 3 with its
  // transit.  Host-side notes on what the last chunk left in fa / fb / fc, xbuf / xbuf2, hbuf and mask.
  static constexpr int kStages = 10;
  struct CamTaps {
    int stage = -1;              // last executed stage (kStages - 1 on a full forward; -1: nothing to read)
    bool full = false;           // the chunk ran to its end: pooled exists
    bool half = false;           // the FCM maps exist as binary16 only (f16 back-end)
    int B = 0, T = 0, Tp = 0, segs = 0;
    const float *stem = nullptr, *block = nullptr, *mid = nullptr, *sc = nullptr, *fcm = nullptr, *tdnn = nullptr,
                *dense = nullptr, *transit = nullptr, *h = nullptr, *mask = nullptr;
    int n_res = 0, res_H = 0, fcm_H = 0, tdnn_ld = 0, dense_ld = 0, transit_ld = 0, transit_c = 0;
    const char* why_no_h = "";   // h / mask absent: the reason
    const char* why_no_mask = "";
  } cam_taps;

  CamppModel(int fd, int ed) : ModelBase("CAMPPlus", fd, ed) {}

  bool wants(const std::string& key) const override {
    return wants_prefixes(key, {"head.", "xvector."});
  }

  int finalize(const SD& sd, int max_batch, int max_frames) override {
    int err = 0;
    if (feat_dim % 8) { set_error("CAMPPlus needs feat_dim %% 8 == 0"); return WS_ERR_INVALID_ARG; }
    fprime = feat_dim / 8;
    if ((err = pack_stem3x3(sd, "head.conv1", "head.bn1", 32, &stem_w, &stem_b))) return err;
    for (int i = 0; i < 4; ++i) {
      const std::string p = std::string("head.layer") + (i < 2 ? "1." : "2.") + std::to_string(i & 1);
      res[i].stride = (i & 1) ? 1 : 2;
      if ((err = pack_conv2d(sd, p + ".conv1", 32, 32, 3, 3, p + ".bn1", &res[i].c1))) return err;
      if ((err = pack_conv2d(sd, p + ".conv2", 32, 32, 3, 3, p + ".bn2", &res[i].c2))) return err;
      if (!(i & 1)) {
        res[i].has_sc = true;
        if ((err = pack_conv2d(sd, p + ".shortcut.0", 32, 32, 1, 1, p + ".shortcut.1", &res[i].sc))) return err;
      }
    }
    if ((err = pack_conv2d(sd, "head.conv2", 32, 32, 3, 3, "head.bn2", &head_conv2))) return err;
    {   // TDNN: Conv1d(32*F' -> 128, k5, stride 2, pad 2), input channel index = c*F' + f.
        // Run as a conv over the (F' x T) image: tap (ty = f, tx = j), Cin = 32.
      const int Fp = fprime;
      if ((err = pack_conv(sd, "xvector.tdnn.linear", {128, 32 * Fp, 5}, 128, 32, Fp, 5,
                           [=](int n, int tp, int ci) {
                             const int f = tp / 5, j = tp % 5;
                             return ((size_t)n * 32 * Fp + (size_t)ci * Fp + f) * 5 + j;
                           },
                           false, "xvector.tdnn.nonlinear.batchnorm", "", &tdnn)))
        return err;
    }
    int ch = 128;
    for (int k = 0; k < 3; ++k) {
      for (int j = 0; j < kLayers[k]; ++j) {
        const std::string p = "xvector.block" + std::to_string(k + 1) + ".tdnnd" + std::to_string(j + 1);
        DenseLayerW L;
        L.cin = ch + 32 * j;
        if ((err = add_bn_vectors(sd, p + ".nonlinear1.batchnorm", L.cin, &L.pre_s, &L.pre_b))) return err;
        if ((err = pack_conv(sd, p + ".linear1", {128, L.cin, 1}, 128, L.cin, 1, 1,
                             [=](int n, int, int ci) { return (size_t)n * L.cin + ci; }, false,
                             p + ".nonlinear2.batchnorm", "", &L.lin1)))
          return err;
        if ((err = pack_conv1d(sd, p + ".cam_layer.linear_local", 32, 128, 3, false, "", "", &L.local))) return err;
        const HostTensor* t;
        if (!(t = get(sd, p + ".cam_layer.linear1.weight", {64, 128, 1}, &err))) return err;
        L.cw1 = arena.add(t->data);
        if ((err = add_vec(sd, p + ".cam_layer.linear1.bias", 64, &L.cb1))) return err;
        if (!(t = get(sd, p + ".cam_layer.linear2.weight", {32, 64, 1}, &err))) return err;
        L.cw2 = arena.add(t->data);
        if ((err = add_vec(sd, p + ".cam_layer.linear2.bias", 32, &L.cb2))) return err;
        layers[k].push_back(L);
      }
      ch += 32 * kLayers[k];
      const std::string p = "xvector.transit" + std::to_string(k + 1);
      transit[k].cin = ch;
      if ((err = add_bn_vectors(sd, p + ".nonlinear.batchnorm", ch, &transit[k].pre_s, &transit[k].pre_b))) return err;
      const int cin = ch;
      if ((err = pack_conv(sd, p + ".linear", {ch / 2, ch, 1}, ch / 2, ch, 1, 1,
                           [=](int n, int, int ci) { return (size_t)n * cin + ci; }, false, "", "",
                           &transit[k].lin)))
        return err;
      ch /= 2;
    }
    if ((err = add_bn_vectors(sd, "xvector.out_nonlinear.batchnorm", ch, &out_s, &out_b))) return err;
    {   // dense: Conv1d(2*ch -> E, k1, no bias) + BN(affine=False), folded
      const int cin = 2 * ch;
      if ((err = pack_conv(sd, "xvector.dense.linear", {embed_dim, cin, 1}, embed_dim, cin, 1, 1,
                           [=](int n, int, int ci) { return (size_t)n * cin + ci; }, false,
                           "xvector.dense.nonlinear.batchnorm", "", &dense, /*fold_affine=*/false)))
        return err;
    }
    if ((err = upload_weights())) return err;
    return reserve(max_batch, max_frames);
  }

  int reserve(int max_batch, int max_frames) override {
    int err = 0;
    maxB = max_batch; maxT = max_frames;
    last_chunk = LastChunk();                  // the taps address the old layout
    cam_taps = CamTaps();
    const size_t img = (size_t)maxB * feat_dim * maxT * 32;        // FCM full-resolution activation
    if ((err = refuse_map_too_large(img))) return err;
    const int Tp = (maxT - 1) / 2 + 1;
    const size_t Mp = (size_t)maxB * Tp;
    max_segs = (Tp + 99) / 100;
    Carve cv;
    size_t o_fa = cv.take(img), o_fb = cv.take(img / 2 + 64), o_fc = cv.take(img / 2 + 64),
           o_x = cv.take(Mp * 1024), o_x2 = cv.take(Mp * 1024), o_h = cv.take(Mp * 128),
           o_mask = cv.take((size_t)maxB * max_segs * 32), o_pool = cv.take((size_t)maxB * 1024),
           o_colsum = cv.take(((Mp + 63) / 64 + 2) * 2 * 128),
           o_part = cv.take((size_t)kSplitK * maxB * embed_dim),
           o_feats = cv.take((size_t)maxB * maxT * feat_dim);
    if ((err = alloc_workspace(cv.total))) return err;
    float* base = ws.as<float>();
    fa = base + o_fa; fb = base + o_fb; fc = base + o_fc; xbuf = base + o_x; xbuf2 = base + o_x2;
    colsum = base + o_colsum;
    hbuf = base + o_h; mask = base + o_mask; pooled = base + o_pool; partial = base + o_part;
    feats_ws = base + o_feats;
    return 0;
  }

  int min_frames() const override { return 3; }

  int forward_chunk(const float* feats, int B, int T, float* emb, hipStream_t st) override {
    // ragged chunk: lens at full resolution (FCM head) and after the stride-2 TDNN layer (trunk); every
    // convolution stores zeros beyond them, the context masks / TSTP run over the valid frames
    const int* L0 = cur_lens[0];
    const int* L1 = cur_lens[1];
    // ---------------- FCM head (2-D, stride only along frequency)
    // f16 back-end: the head's activation maps are binary16 only and its convolutions (and the TDNN
    // layer that consumes them) run on the LDS-DMA kernel in convolution form
    const bool f16io = gemm_precision == 2;
    int H = feat_dim;
    last_chunk.B = 0;                          // (taps: nothing to read until this chunk has been enqueued)
    WS_LAUNCH(other(4.0 * B * H * (double)T * 33, st, [&] {
      return launch_stem_conv3x3(feats, B, T, feat_dim, arena.at(stem_w), arena.at(stem_b), 32, fa, st,
                                 f16io ? reinterpret_cast<uint16_t*>(fa) : nullptr, L0);
    }));
    CamTaps tp;                                // host-side notes for ws_debug_engine_tap, stored when the chunk ends
    tp.half = f16io; tp.B = B; tp.T = T; tp.Tp = (T - 1) / 2 + 1;
    tp.stem = fa;
    if (stop_after == 0) return end_chunk(tp, 0, false, emb, st);
    auto to16 = [&](ConvGemmParams& p, const float* in, float* out, const float* res) {
      if (!f16io) { if (res) { p.residual = res; p.ldr = 32; p.r_off = 0; } return; }
      p.A16 = reinterpret_cast<const uint16_t*>(in); p.lda16 = 32;
      if (out) { p.D = nullptr; p.D16 = reinterpret_cast<uint16_t*>(out); p.ldd16 = 32; }
      if (res) { p.residual16 = reinterpret_cast<const uint16_t*>(res); p.ldr = 32; p.r_off = 0; }
    };
    float* x = fa;          // block input
    float* t1 = fb;
    float* t2 = fc;
    for (int i = 0; i < 4; ++i) {
      const int s = res[i].stride, Ho = (H - 1) / s + 1;
      const float* r = x;
      if (res[i].has_sc) {
        ConvGemmParams ps = conv2d(res[i].sc, x, 32, 0, t2, 32, 0, B, H, T, s, 1, 1, 1, 0, 0, ACT_NONE);
        to16(ps, x, t2, nullptr);
        ps.row_len = L0;
        WS_LAUNCH(gemm(ps, st));
        r = t2;
      }
      ConvGemmParams p1 = conv2d(res[i].c1, x, 32, 0, t1, 32, 0, B, H, T, s, 1, 1, 1, 1, 1, ACT_RELU);
      to16(p1, x, t1, nullptr);
      p1.row_len = L0;
      WS_LAUNCH(gemm(p1, st));
      // conv2 writes over the block input buffer when that is no longer needed (shortcut case),
      // otherwise into t2
      float* out = res[i].has_sc ? x : t2;
      ConvGemmParams p2 = conv2d(res[i].c2, t1, 32, 0, out, 32, 0, B, Ho, T, 1, 1, 1, 1, 1, 1, ACT_RELU);
      to16(p2, t1, out, r);
      p2.row_len = L0;
      WS_LAUNCH(gemm(p2, st));
      // what this block left in fa / fb / fc: its result, conv1's output, the shortcut convolution's output
      tp.stem = nullptr; tp.block = out; tp.mid = t1; tp.sc = res[i].has_sc ? t2 : nullptr;
      tp.n_res = i + 1; tp.res_H = Ho;
      if (!res[i].has_sc) { float* tmp = x; x = t2; t2 = tmp; }
      H = Ho;
      if (stop_after == i + 1) return end_chunk(tp, i + 1, false, emb, st);
    }
    {   // head.conv2: 3x3 stride (2,1) + BN + ReLU  -> [b][F'][T][32]
      ConvGemmParams ph = conv2d(head_conv2, x, 32, 0, t1, 32, 0, B, H, T, 2, 1, 1, 1, 1, 1, ACT_RELU);
      to16(ph, x, t1, nullptr);
      ph.row_len = L0;
      WS_LAUNCH(gemm(ph, st));
      H = (H - 1) / 2 + 1;
      tp.mid = nullptr;                        // (head.conv2 wrote over block 4's conv1 output)
      tp.fcm = t1; tp.fcm_H = H;
      if (stop_after == 5) return end_chunk(tp, 5, false, emb, st);
    }
    // ---------------- TDNN (k5, stride 2) over the (F' x T) image -> [B*T'][128] at channel 0 of xbuf
    const int Tp = (T - 1) / 2 + 1;
    float* X = xbuf;
    float* Xn = xbuf2;
    int ldx = 128 + 32 * kLayers[0];
    {
      ConvGemmParams pt0 = conv2d(tdnn, t1, 32, 0, X, ldx, 0, B, H, T, 1, 2, 1, 1, 0, 2, ACT_RELU);
      to16(pt0, t1, nullptr, nullptr);          // binary16 input, fp32 output (the dense blocks stay fp32)
      pt0.row_len = L1;
      WS_LAUNCH(gemm(pt0, st));
      tp.tdnn = X; tp.tdnn_ld = ldx;
      if (stop_after == 6) return end_chunk(tp, 6, false, emb, st);
    }
    const int segs = (Tp + 99) / 100;
    int ch = 128;
    for (int k = 0; k < 3; ++k) {
      // fp32, utterances of <= 128 trunk frames: the whole dense block is one launch, one workgroup per utterance
      // (cam_dense_block_kernel); a block the launch cannot take (more layers than its argument block holds, an
      // unaligned trunk buffer) falls back to one launch per layer below
      bool block_done = false;
      bool h_is_half = false;
      if (gemm_precision == 0 && (int)layers[k].size() <= WS_CAM_MAX_LAYERS &&
          !layers[k].empty() && (reinterpret_cast<uintptr_t>(X) & 127) == 0 && (ldx & 31) == 0) {
        bool ok = true;
        for (size_t j = 0; j < layers[k].size(); ++j)
          ok = ok && layers[k][j].cin == layers[k][0].cin + 32 * (int)j &&
               cam_dense_fused_applies(Tp, layers[k][j].cin, kDil[k]);
        if (ok) {
          CamDenseBlockParams bp = {};
          CamDenseParams& cp = bp.base;
          cp.X = X; cp.Xout = X; cp.ldx = ldx; cp.cin = layers[k][0].cin; cp.c_off = cp.cin; cp.Tp = Tp; cp.lens = L1;
          cp.dil = kDil[k];
          bp.n_layers = (int)layers[k].size();
          double fl = 0, by = 0;
          for (size_t j = 0; j < layers[k].size(); ++j) {
            const DenseLayerW& L = layers[k][j];
            CamDenseLayerW& w = bp.layers[j];
            w.pre_s = arena.at(L.pre_s); w.pre_b = arena.at(L.pre_b);
            w.W1 = arena.at(L.lin1.w); w.b1 = arena.at(L.lin1.b); w.ldw1 = L.lin1.ldw;
            w.Wl = arena.at(L.local.w); w.ldwl = L.local.ldw;
            w.cw1 = arena.at(L.cw1); w.cb1 = arena.at(L.cb1); w.cw2 = arena.at(L.cw2); w.cb2 = arena.at(L.cb2);
            fl += 2.0 * B * (double)Tp * (128.0 * L.cin + 3.0 * 128 * 32);
            by += 4.0 * (B * (double)Tp * (L.cin + 32) + 128.0 * L.cin + 3.0 * 128 * 32);
          }
          if (prof.enabled) prof.begin(0, fl, by, st);
          hipError_t ce = launch_cam_dense_block(bp, B, st);
          prof.end(st);
          WS_LAUNCH(ce);
          block_done = true;
        }
      }
      for (size_t j = 0; !block_done && j < layers[k].size(); ++j) {
        const DenseLayerW& L = layers[k][j];
        // ... or one kernel per layer
        if (gemm_precision == 0 && cam_dense_fused_applies(Tp, L.cin, kDil[k])) {
          CamDenseParams cp = {};
          cp.X = X; cp.Xout = X; cp.ldx = ldx; cp.cin = L.cin; cp.c_off = L.cin; cp.Tp = Tp; cp.lens = L1;
          cp.pre_s = arena.at(L.pre_s); cp.pre_b = arena.at(L.pre_b);
          cp.W1 = arena.at(L.lin1.w); cp.b1 = arena.at(L.lin1.b); cp.ldw1 = L.lin1.ldw;
          cp.Wl = arena.at(L.local.w); cp.ldwl = L.local.ldw;
          cp.cw1 = arena.at(L.cw1); cp.cb1 = arena.at(L.cb1); cp.cw2 = arena.at(L.cw2); cp.cb2 = arena.at(L.cb2);
          cp.dil = kDil[k];
          if (prof.enabled)
            prof.begin(0, 2.0 * B * (double)Tp * (128.0 * L.cin + 3.0 * 128 * 32),
                       4.0 * (B * (double)Tp * (L.cin + 32) + 128.0 * L.cin + 3.0 * 128 * 32), st);
          hipError_t ce = launch_cam_dense_layer(cp, B, st);
          prof.end(st);
          WS_LAUNCH(ce);
          continue;
        }
        // BN-ReLU -> 1x1 (Cin -> 128) -> BN -> ReLU
        ConvGemmParams p1 = conv1d(L.lin1, X, ldx, 0, hbuf, 128, 0, B, Tp, 1, ACT_RELU);
        p1.pre_scale = arena.at(L.pre_s); p1.pre_shift = arena.at(L.pre_b);
        // one context segment (T' <= 100) and >= 64 rows per utterance: the time mean of the
        // bottleneck output comes out of this GEMM's epilogue, the mask kernel never reads hbuf
        const bool ctx_from_colsum = segs == 1 && Tp >= 64;
        if (ctx_from_colsum) p1.colsum = colsum;
        // f16 back-end: the bottleneck output feeds only the k3 conv (and the statistics above): keep it
        // as binary16 (hbuf reused), read by the conv DMA kernel
        const bool h_half = f16io && ctx_from_colsum;
        if (h_half) { p1.D = nullptr; p1.D16 = reinterpret_cast<uint16_t*>(hbuf); p1.ldd16 = 128; }
        h_is_half = h_half;
        p1.row_len = L1;
        WS_LAUNCH(gemm(p1, st));
        // context mask m[b][seg][32]
        WS_LAUNCH(other(ctx_from_colsum ? 0.0 : 4.0 * B * (double)Tp * 128, st, [&] {
          if (ctx_from_colsum)
            return launch_cam_context_from_colsum(colsum, B, Tp, 128, arena.at(L.cw1), arena.at(L.cb1), 64,
                                                  arena.at(L.cw2), arena.at(L.cb2), 32, mask, st, L1);
          return launch_cam_context(hbuf, 128, B, Tp, 128, 100, arena.at(L.cw1), arena.at(L.cb1), 64,
                                    arena.at(L.cw2), arena.at(L.cb2), 32, mask, st, L1);
        }));
        // local k3 dilated conv 128 -> 32, times the mask, appended at channel offset cin
        ConvGemmParams p2 = conv1d(L.local, hbuf, 128, 0, X, ldx, L.cin, B, Tp, kDil[k], ACT_NONE);
        p2.seg_scale = mask; p2.seg_len = 100; p2.segs_per_img = segs;
        if (h_half) { p2.A16 = reinterpret_cast<const uint16_t*>(hbuf); p2.lda16 = 128; }
        p2.row_len = L1;
        WS_LAUNCH(gemm(p2, st));
      }
      ch += 32 * kLayers[k];
      // transit: BN-ReLU -> 1x1 (ch -> ch/2), written to channel 0 of the next block's buffer
      const int ld_next = k < 2 ? ch / 2 + 32 * kLayers[k + 1] : ch / 2;
      ConvGemmParams pt = conv1d(transit[k].lin, X, ldx, 0, Xn, ld_next, 0, B, Tp, 1, ACT_NONE);
      pt.pre_scale = arena.at(transit[k].pre_s); pt.pre_shift = arena.at(transit[k].pre_b);
      pt.row_len = L1;
      WS_LAUNCH(gemm(pt, st));
      // what this block left: its whole buffer, the transit output at the next buffer's row stride, and -- where the
      // three-launch path ran -- the last layer's bottleneck output and mask
      tp.dense = X; tp.dense_ld = ldx; tp.transit = Xn; tp.transit_ld = ld_next; tp.transit_c = ch / 2; tp.segs = segs;
      if (k > 0) tp.tdnn = nullptr;            // (transit 2 wrote over block 1's buffer)
      const bool generic = !block_done && !(gemm_precision == 0 && cam_dense_fused_applies(Tp, layers[k][0].cin, kDil[k]));
      tp.h = generic && !h_is_half ? hbuf : nullptr;
      tp.mask = generic ? mask : nullptr;
      tp.why_no_mask = "cam_dense_block_kernel ran the block: the bottleneck and the mask stay in LDS";
      tp.why_no_h = generic ? "the f16 back-end keeps the bottleneck output in binary16 only" : tp.why_no_mask;
      float* tmp = X; X = Xn; Xn = tmp;
      ldx = ld_next;
      ch /= 2;
      if (stop_after == 7 + k) return end_chunk(tp, 7 + k, false, emb, st);
    }
    // out_nonlinear BN-ReLU fused into TSTP, then dense 1x1 + BN(affine=False)
    WS_LAUNCH(other(8.0 * B * (double)Tp * ch, st, [&] {
      return launch_tstp(X, ldx, B, 1, Tp, ch, arena.at(out_s), arena.at(out_b), pooled, st, L1);
    }));
    WS_LAUNCH(gemm_splitk(conv1d(dense, pooled, 2 * ch, 0, emb, embed_dim, 0, B, 1, 1, ACT_NONE),
                          partial, kSplitK, st));
    return end_chunk(tp, kStages - 1, true, emb, st);
  }

  // the chunk is enqueued: remember what it left; a stopped one (ws_debug_engine_stop_after) returns zeros
  int end_chunk(CamTaps& tp, int stage, bool full, float* emb, hipStream_t st) {
    tp.stage = stage; tp.full = full;
    if (!full)
      if (int r = stop_chunk(emb, tp.B, st)) return r;
    cam_taps = tp;
    last_chunk.B = tp.B; last_chunk.T = tp.T; last_chunk.prec = gemm_precision;
    return 0;
  }

  int set_stop_after(int n) override {
    if (n < -1 || n >= kStages) {
      set_error("ws_debug_engine_stop_after: n = %d, %s has %d stop points 0 .. %d (0 the stem, 1-4 the FCM residual "
                "blocks, 5 head.conv2, 6 the TDNN layer, 7-9 dense block 1-3 with its transit; -1 = the full forward)",
                n, name.c_str(), kStages, kStages - 1);
      return WS_ERR_INVALID_ARG;
    }
    stop_after = n;
    return WS_OK;
  }

  // ws_debug_engine_tap: what the last chunk's last executed stages left in the workspace (see CamTaps)
  int tap(const char* tname, float* dst, int64_t cap_floats, int32_t* rows, int32_t* cols, hipStream_t st) override {
    if (int r = tap_guard()) return r;
    const CamTaps& t = cam_taps;
    const std::string n = tname;
    char why[200] = "";
    const char* half = "the f16 back-end keeps the FCM maps in binary16 only";
    auto map = [&](const float* src, int H) {       // an FCM map [b][f][t][32]
      return tap_copy(tname, t.half ? nullptr : src, t.half ? half : why, t.B * H * t.T, 32, dst, cap_floats, rows, cols, st);
    };
    const int M = t.B * t.Tp;
    if (n == "stem") {
      std::snprintf(why, sizeof(why), "the last forward ran on to stage %d and FCM block 1 wrote over the stem: stop it "
                    "at 0 (ws_debug_engine_stop_after)", t.stage);
      return map(t.stem, feat_dim);
    }
    if (n == "block" || n == "mid" || n == "sc") {
      if (t.n_res < 1) {
        std::snprintf(why, sizeof(why), "the last forward was stopped after the stem: no FCM block ran");
        return map(nullptr, 0);
      }
      if (n == "block") return map(t.block, t.res_H);
      if (n == "mid") {
        std::snprintf(why, sizeof(why), "head.conv2 wrote over FCM block 4's conv1 output: stop at 1 .. 4");
        return map(t.mid, t.res_H);
      }
      std::snprintf(why, sizeof(why), "FCM block %d has no shortcut convolution", t.n_res);
      return map(t.sc, t.res_H);
    }
    if (n == "fcm") {
      std::snprintf(why, sizeof(why), "the last forward was stopped at %d, before head.conv2 (stop 5)", t.stage);
      return map(t.fcm, t.fcm_H);
    }
    if (n == "tdnn") {
      if (t.stage < 6)
        std::snprintf(why, sizeof(why), "the last forward was stopped at %d, before the TDNN layer (stop 6)", t.stage);
      else
        std::snprintf(why, sizeof(why), "the last forward ran on to stage %d and transit 2 wrote over dense block 1's "
                      "buffer: stop at 6 or 7", t.stage);
      return tap_copy(tname, t.tdnn, why, M, 128, dst, cap_floats, rows, cols, st, t.tdnn_ld);
    }
    if (n == "dense" || n == "transit" || n == "h" || n == "mask") {
      if (!t.dense) {
        std::snprintf(why, sizeof(why), "the last forward was stopped at %d: no dense block ran (stops 7 .. 9)", t.stage);
        return tap_copy(tname, nullptr, why, 0, 0, dst, cap_floats, rows, cols, st);
      }
      if (n == "dense") return tap_copy(tname, t.dense, why, M, t.dense_ld, dst, cap_floats, rows, cols, st);
      if (n == "transit") return tap_copy(tname, t.transit, why, M, t.transit_c, dst, cap_floats, rows, cols, st, t.transit_ld);
      if (n == "h") return tap_copy(tname, t.h, t.why_no_h, M, 128, dst, cap_floats, rows, cols, st);
      return tap_copy(tname, t.mask, t.why_no_mask, t.B * t.segs, 32, dst, cap_floats, rows, cols, st);
    }
    if (n == "pooled") {
      std::snprintf(why, sizeof(why), "the last forward was stopped at %d: pooling and the head did not run", t.stage);
      return tap_copy(tname, t.full ? pooled : nullptr, why, t.B, 1024, dst, cap_floats, rows, cols, st);
    }
    set_error("ws_debug_engine_tap: unknown tensor '%s' (%s: stem, block, mid, sc, fcm, tdnn, dense, transit, h, mask, "
              "pooled)", tname, name.c_str());
    return WS_ERR_INVALID_ARG;
  }

  double flops(int batch, int T) const override {
    double macs = 0;
    int H = feat_dim;
    macs += (double)H * T * 9 * 32;
    for (int i = 0; i < 4; ++i) {
      const int s = res[i].stride, Ho = (H - 1) / s + 1;
      macs += (double)Ho * T * 9 * 32 * 32 * 2;
      if (res[i].has_sc) macs += (double)Ho * T * 32 * 32;
      H = Ho;
    }
    H = (H - 1) / 2 + 1;
    macs += (double)H * T * 9 * 32 * 32;
    const int Tp = (T - 1) / 2 + 1;
    macs += (double)Tp * 128 * 32 * fprime * 5;
    int ch = 128;
    for (int k = 0; k < 3; ++k) {
      for (int j = 0; j < kLayers[k]; ++j)
        macs += (double)Tp * ((double)(ch + 32 * j) * 128 + 128.0 * 32 * 3) + 128.0 * 64 + 64.0 * 32;
      ch += 32 * kLayers[k];
      macs += (double)Tp * ch * (ch / 2);
      ch /= 2;
    }
    macs += 2.0 * ch * embed_dim;
    return 2.0 * macs * batch;
  }
};

constexpr int CamppModel::kLayers[3];
constexpr int CamppModel::kDil[3];

}  // namespace

Model* make_campplus(const std::string& model_name, int feat_dim, int embed_dim) {
  if (model_name == "CAMPPlus") return new CamppModel(feat_dim, embed_dim);
  return nullptr;
}

}  // namespace wsamd
