// TDNN x-vector forward scheduled onto the gfx950 kernels (host side).
//
// Architecture and parameter names follow the reference (file:line in wenet-e2e/wespeaker):
//   wespeaker/models/tdnn.py:23-54      TdnnLayer: Conv1d (no padding) -> ReLU -> BatchNorm1d(affine=False)
//   wespeaker/models/tdnn.py:57-115     XVEC: frame_1..5 (k 5/3/3/1/1, dilation 1/2/3/1/1), pool, seg_1 -> ReLU ->
//                                       seg_bn_1 -> seg_2; every caller takes embed_b, the tuple's last element
//   wespeaker/models/xi_vector.py:48    XI_VEC_XVEC = XVEC(pooling_func='XI')
//   wespeaker/models/pooling_layers.py:67-85, 344-416   TSTP, XI
//
// Layout: channels-last [utterance*frame][channel] fp32 rows, every layer T rows long.  The reference's convolutions
// are VALID ones (T shrinks by 4 + 4 + 6 = 14); here each runs as the "same"-padded conv1d of the GEMM family and the
// pooling reads the frame window [7, len - 7) only: the receptive field of a frame is +-7, so no frame of the window
// ever sees a padded tap, and what lies outside the window is never read.  BN comes after the ReLU: an epilogue affine
// (ConvGemmParams::post_scale / post_shift).  hid_dim and stats_dim come from the checkpoint's shapes; frame_5's output
// width (and XI's lin2) is padded to a multiple of 64 with zero weights, zero bias and zero scale / shift on pack, so
// the wide GEMM kernels take them -- the padding columns hold exact zeros and the pooling kernels skip them.
#include "model_common.h"

namespace wsamd {

namespace {

constexpr int kTrim = 7;                 // frames lost on each side by the three context layers (2 + 2 + 3)
constexpr int kMinFrames = 2 * kTrim + 1;

struct TdnnModel : ModelBase {
  static constexpr int kSplitK = 16;
  bool xi = false;
  int hid = 0, stats = 0, stats_pad = 0, xi_hid = 0;
  ConvW fr[5], lin1, lin2, seg1, seg2;
  size_t prior_mean = 0, prior_logprec = 0, seg_bn_scale = 0, seg_bn_shift = 0;
  float *act[2] = {nullptr, nullptr}, *f5 = nullptr, *xh = nullptr, *xz = nullptr, *pooled = nullptr, *partial = nullptr,
        *emb_a = nullptr;
  int layers_run = 0;                    // of the last chunk (taps)

  TdnnModel(const std::string& n, int fd, int ed) : ModelBase(n, fd, ed) { xi = n == "XI_VEC_XVEC"; }

  bool wants(const std::string& key) const override {
    return wants_prefixes(key, {"frame_1.", "frame_2.", "frame_3.", "frame_4.", "frame_5.", "pool.", "seg_1.", "seg_bn_1.",
                                "seg_2."});
  }
  int pooled_dim() const { return xi ? stats : 2 * stats; }

  int finalize(const SD& sd, int max_batch, int max_frames) override {
    int err = 0;
    auto w1 = sd.find("frame_1.conv_1d.weight"), w5 = sd.find("frame_5.conv_1d.weight");
    if (w1 == sd.end() || w5 == sd.end() || w1->second.shape.size() != 3 || w5->second.shape.size() != 3) {
      set_error("missing tensor 'frame_1.conv_1d.weight' / 'frame_5.conv_1d.weight' for model %s", name.c_str());
      return WS_ERR_MISSING_TENSOR;
    }
    hid = (int)w1->second.shape[0];
    stats = (int)w5->second.shape[0];
    if (hid <= 0 || stats <= 0 || (hid & 3) || (stats & 3)) {
      set_error("%s: hid_dim %d and stats_dim %d (frame_1 / frame_5.conv_1d.weight) must be positive multiples of 4",
                name.c_str(), hid, stats);
      return WS_ERR_SHAPE;
    }
    stats_pad = round_up(stats, 64);
    static const int taps[5] = {5, 3, 3, 1, 1};
    for (int k = 0; k < 5; ++k) {
      const std::string p = "frame_" + std::to_string(k + 1);
      const int N = k == 4 ? stats : hid, Cin = k == 0 ? feat_dim : hid, kw = taps[k];
      const HostTensor* wt = get(sd, p + ".conv_1d.weight", {N, Cin, kw}, &err);
      if (!wt) return err;
      const HostTensor* bs = get(sd, p + ".conv_1d.bias", {N}, &err);
      if (!bs) return err;
      std::vector<double> sc, sh;
      if ((err = bn_affine(sd, p + ".bn", N, &sc, &sh, false))) return err;
      pack_dense(N, k == 4 ? stats_pad : N, Cin, kw,
                 [&](int n, int tp, int ci) { return (double)wt->data[((size_t)n * Cin + ci) * kw + tp]; },
                 [&](int n) { return (double)bs->data[n]; }, sc, sh, &fr[k]);
    }
    if (xi && (err = pack_xi(sd, "pool", stats, stats_pad, &lin1, &lin2, &prior_mean, &prior_logprec, &xi_hid))) return err;
    if ((err = pack_linear(sd, "seg_1", embed_dim, pooled_dim(), true, &seg1))) return err;
    if ((err = add_bn_vectors(sd, "seg_bn_1", embed_dim, &seg_bn_scale, &seg_bn_shift, false))) return err;
    if ((err = pack_linear(sd, "seg_2", embed_dim, embed_dim, true, &seg2))) return err;
    if ((err = upload_weights())) return err;
    return reserve(max_batch, max_frames);
  }

  int reserve(int max_batch, int max_frames) override {
    maxB = max_batch; maxT = max_frames;
    last_chunk = LastChunk();                  // the taps address the old layout
    if (int r = refuse_batch_too_large()) return r;
    const size_t M = (size_t)maxB * maxT;
    if (int r = refuse_map_too_large(M * (size_t)stats_pad)) return r;
    Carve cv;
    const size_t o_a = cv.take(M * hid), o_b = cv.take(M * hid), o_f5 = cv.take(M * stats_pad),
                 o_xh = cv.take(xi ? M * xi_hid : 0), o_xz = cv.take(xi ? M * stats_pad : 0),
                 o_pool = cv.take((size_t)maxB * 2 * stats), o_part = cv.take((size_t)kSplitK * maxB * embed_dim),
                 o_emba = cv.take((size_t)maxB * embed_dim), o_feats = cv.take(M * feat_dim);
    if (int err = alloc_workspace(cv.total)) return err;
    float* base = ws.as<float>();
    act[0] = base + o_a; act[1] = base + o_b; f5 = base + o_f5; xh = base + o_xh; xz = base + o_xz;
    pooled = base + o_pool; partial = base + o_part; emb_a = base + o_emba; feats_ws = base + o_feats;
    return 0;
  }

  int min_frames() const override { return kMinFrames; }

  // The reference's Conv1d raises on an utterance shorter than its receptive field: a bad argument, not a capacity
  int refuse_short(int frames) {
    if (frames >= kMinFrames) return 0;
    set_error("%s: num_frames %d, the five TDNN layers need at least 15 frames (receptive field 15, no padding)",
              name.c_str(), frames);
    return WS_ERR_INVALID_ARG;
  }
  int forward(const float* feats, int batch, int frames, float* emb, hipStream_t st) override {
    if (int r = refuse_short(frames)) return r;
    return ModelBase::forward(feats, batch, frames, emb, st);
  }
  int forward_ragged(const float* feats, int batch, int frames, const int32_t* lens_host, float* emb, hipStream_t st,
                     int cmvn_mode = 0) override {
    if (int r = refuse_short(frames)) return r;      // (a short ROW: upload_lens, "valid range is [15, ...]")
    return ModelBase::forward_ragged(feats, batch, frames, lens_host, emb, st, cmvn_mode);
  }

  int set_precision(int mode) override {
    if (mode == 2) {
      set_error("%s has no binary16-tensor back-end (precision mode 2): %s fp32; use mode 0 (fp32) or 1 (f16x3)",
                name.c_str(), xi ? "its XI pooling kernel is" : "its pooling kernel is");
      return WS_ERR_INVALID_ARG;
    }
    return ModelBase::set_precision(mode);
  }

  int forward_chunk(const float* feats, int B, int T, float* emb, hipStream_t st) override {
    if (gemm_precision == 2) {                 // (set_precision refuses it)
      set_error("%s has no binary16-tensor back-end (precision mode 2)", name.c_str());
      return WS_ERR_STATE;
    }
    const int* L0 = cur_lens[0];
    static const int dil[5] = {1, 2, 3, 1, 1};
    last_chunk.B = 0;
    const float* in = feats;
    int ldin = feat_dim;
    for (int k = 0; k < 5; ++k) {
      float* out = k == 4 ? f5 : act[k & 1];
      const int ldo = k == 4 ? stats_pad : hid;
      ConvGemmParams p = conv1d(fr[k], in, ldin, 0, out, ldo, 0, B, T, dil[k], ACT_RELU);
      p.row_len = L0;
      WS_LAUNCH(gemm(p, st));
      in = out; ldin = ldo;
      if (stop_after == k + 1) return end_chunk(k + 1, false, B, T, emb, st);
    }
    const double m = (double)B * T;
    if (xi) {
      // log-precision estimator: two 1x1 GEMMs (lin1 reads the zero padding columns of frame_5 against zero weights)
      ConvGemmParams a = conv1d(lin1, f5, stats_pad, 0, xh, xi_hid, 0, B, T, 1, ACT_RELU);
      a.K = stats_pad; a.Cin = stats_pad;
      a.row_len = L0;
      WS_LAUNCH(gemm(a, st));
      ConvGemmParams z = conv1d(lin2, xh, xi_hid, 0, xz, stats_pad, 0, B, T, 1, ACT_NONE);
      z.row_len = L0;
      WS_LAUNCH(gemm(z, st));
      WS_LAUNCH(other(8.0 * m * stats, st, [&] {
        XiPoolParams q = {};
        q.x = f5; q.ldx = stats_pad; q.z = xz; q.ldz = stats_pad;
        q.prior_mean = arena.at(prior_mean); q.prior_logprec = arena.at(prior_logprec);
        q.pooled = pooled; q.ldp = stats; q.B = B; q.T = T; q.D = stats; q.lens = L0; q.trim = kTrim;
        return launch_xi_pool(q, st);
      }));
    } else {
      WS_LAUNCH(other(8.0 * m * stats, st, [&] {
        return launch_tstp(f5, stats_pad, B, 1, T, stats, nullptr, nullptr, pooled, st, L0, kTrim);
      }));
    }
    // embed_b = seg_2(seg_bn_1(relu(seg_1(stats)))): relu -> BN(affine=False) is seg_1's epilogue
    ConvGemmParams s1 = conv1d(seg1, pooled, pooled_dim(), 0, emb_a, embed_dim, 0, B, 1, 1, ACT_RELU);
    s1.post_scale = arena.at(seg_bn_scale); s1.post_shift = arena.at(seg_bn_shift);
    WS_LAUNCH(gemm_splitk(s1, partial, kSplitK, st));
    WS_LAUNCH(gemm(conv1d(seg2, emb_a, embed_dim, 0, emb, embed_dim, 0, B, 1, 1, ACT_NONE), st));
    return end_chunk(5, true, B, T, emb, st);
  }

  int end_chunk(int n, bool full, int B, int T, float* emb, hipStream_t st) {
    if (!full)
      if (int r = stop_chunk(emb, B, st)) return r;
    layers_run = n;
    last_chunk.B = B; last_chunk.T = T; last_chunk.prec = gemm_precision; last_chunk.full = full;
    return 0;
  }

  int set_stop_after(int n) override {
    if (n != -1 && (n < 1 || n > 5)) {
      set_error("ws_debug_engine_stop_after: n_blocks = %d, %s has 5 TDNN layers: 1 .. 5 (-1 = the full forward)", n,
                name.c_str());
      return WS_ERR_INVALID_ARG;
    }
    stop_after = n;
    return WS_OK;
  }

  // frame: the last executed TDNN layer after its BN, every utterance T rows long (the rows outside [7 - r, len - 7 + r)
  // -- r what the later layers still take off -- have seen padded taps: the reference has no such rows)
  int tap(const char* tname, float* dst, int64_t cap_floats, int32_t* rows, int32_t* cols, hipStream_t st) override {
    if (int r = tap_guard()) return r;
    const LastChunk& lc = last_chunk;
    const int M = lc.B * lc.T;
    const char* stopped = "the forward was stopped after a TDNN layer: pooling and the head did not run";
    const char* noxi = "only XI_VEC_XVEC has the XI log-precision estimator";
    const std::string n = tname;
    if (n == "frame") {
      if (layers_run == 5) return tap_copy(tname, f5, "", M, stats, dst, cap_floats, rows, cols, st, stats_pad);
      return tap_copy(tname, act[(layers_run - 1) & 1], "", M, hid, dst, cap_floats, rows, cols, st);
    }
    const bool full = lc.full;
    if (n == "pooled") return tap_copy(tname, full ? pooled : nullptr, stopped, lc.B, pooled_dim(), dst, cap_floats, rows, cols, st);
    if (n == "emb_a") return tap_copy(tname, full ? emb_a : nullptr, stopped, lc.B, embed_dim, dst, cap_floats, rows, cols, st);
    if (n == "xi_hid")
      return tap_copy(tname, !xi ? nullptr : (full ? xh : nullptr), xi ? stopped : noxi, M, xi_hid, dst, cap_floats, rows, cols, st);
    if (n == "xi_z")
      return tap_copy(tname, !xi ? nullptr : (full ? xz : nullptr), xi ? stopped : noxi, M, stats, dst, cap_floats, rows,
                      cols, st, stats_pad);
    set_error("ws_debug_engine_tap: unknown tensor '%s' (%s: frame, pooled, emb_a, xi_hid, xi_z)", tname, name.c_str());
    return WS_ERR_INVALID_ARG;
  }

  double flops(int batch, int T) const override {
    double macs = (double)feat_dim * 5 * hid + 2.0 * hid * 3 * hid + (double)hid * hid + (double)hid * stats;
    if (xi) macs += 2.0 * stats * xi_hid;
    double per_utt = macs * T;                  // (every layer runs T rows long)
    per_utt += (double)pooled_dim() * embed_dim + (double)embed_dim * embed_dim;
    return 2.0 * per_utt * batch;
  }
};

}  // namespace

Model* make_tdnn(const std::string& model_name, int feat_dim, int embed_dim) {
  if (model_name == "XVEC" || model_name == "XI_VEC_XVEC") return new TdnnModel(model_name, feat_dim, embed_dim);
  return nullptr;
}

}  // namespace wsamd
