/*
 * wespeaker_amd.h -- C-ABI of the MI355X-native speaker-embedding + PLDA engine.
 *
 * This is the drop-in boundary for the hot path of wenet-e2e/wespeaker
 * (fbank -> ECAPA-TDNN / ResNet / CAM++ forward -> two-covariance PLDA LLR).
 * The reference has no FFI of its own for this path (it is torch.nn.Modules + numpy); each entry
 * point below names the reference interface it replaces (file:line relative to the reference
 * repo).  INTEGRATION.md shows the ctypes / C++ bindings a reference maintainer would add.
 *
 * Conventions:
 *   - extern "C", plain pointers and sizes only; no C++ or torch types cross the boundary.
 *   - every call returns int: 0 = ok, negative = error (never aborts);
 *     ws_last_error() returns a thread-local human-readable message for the last failure.
 *   - the caller owns every input/output buffer; the handle owns weights + workspace.
 *   - pointers marked DEVICE are HIP device pointers on the handle's device; HOST are host pointers.
 *   - all GPU work is enqueued on the caller's stream (a hipStream_t passed as void*; NULL = the
 *     default stream); no call synchronises the device unless documented.
 *   - one handle per (process, GPU); handles are not thread-safe.  Every call that takes a handle makes the
 *     handle's device the calling thread's current HIP device (hipSetDevice) and leaves it so; the handle-less
 *     helpers (ws_cos_*, ws_cohort_stats, ws_asnorm_pairs, ws_plda_stats, ws_rows_affine, ws_resample) launch
 *     on the calling thread's current device: make the device of their DEVICE pointers current first.
 */
#ifndef WESPEAKER_AMD_H_
#define WESPEAKER_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: only the entry points below are exported. */
#if defined(__GNUC__) || defined(__clang__)
#define WS_API __attribute__((visibility("default")))
#else
#define WS_API
#endif

#define WS_OK 0
#define WS_ERR_INVALID_ARG (-1)
#define WS_ERR_UNKNOWN_MODEL (-2)
#define WS_ERR_MISSING_TENSOR (-3)
#define WS_ERR_SHAPE (-4)
#define WS_ERR_HIP (-5)
#define WS_ERR_STATE (-6)
#define WS_ERR_CAPACITY (-7)
#define WS_ERR_RANGE (-8) /* binary16 back-end: an activation left the binary16 range */

#define WS_WINDOW_HAMMING 0 /* Speaker default, cli/speaker.py:50 */
#define WS_WINDOW_POVEY 1   /* Speaker.set_window_type('povey'), cli/speaker.py:66-67 */

#define WS_WAV_INT16 0 /* PCM16 samples (torchaudio.load(normalize=False), cli/speaker.py:126) */
#define WS_WAV_FLOAT32 1

typedef struct ws_engine ws_engine;     /* one speaker-embedding model on one GPU */
typedef struct ws_frontend ws_frontend; /* Kaldi fbank + CMN frontend on one GPU  */
typedef struct ws_plda ws_plda;         /* two-covariance PLDA scorer on one GPU  */
typedef void* ws_stream;                /* hipStream_t */

/* ------------------------------------------------------------------------------------ misc */
/* Bumped whenever an exported signature changes (101: ws_plda_stats takes `emb_is_f64` and a void* table since
 * round 2 -- a caller built against 100 would pass shifted arguments; 104: ws_frontend_set_cmvn / ws_cmvn added, the
 * `cmn` flags now mean "apply the frontend's CMVN"; 105: ws_forward_ragged_cmvn added; 106: ws_debug_engine_tap added;
 * 107: ws_debug_engine_stop_after added; 108: ws_debug_engine_stop_after and ws_debug_engine_tap serve CAM++ -- a
 * caller that relied on their refusing that family sees other results; 109: ws_debug_aff_fuse added, ws_engine_create
 * knows the ERes2Net34 names, ws_debug_engine_tap / ws_debug_engine_stop_after serve them; 110:
 * ws_debug_engine_stop_after serves ECAPA-TDNN (1 .. 3) and ws_debug_engine_tap reads its binary16 tensors -- a caller
 * that relied on the refusals sees other results; 111: the ws_spectral_* entries, ws_debug_spectral_dense and
 * ws_debug_spectral_mask added; 112: ws_debug_dwconv3x3 added, ws_engine_create knows the Gemini_DF_ResNet names,
 * ws_debug_engine_tap / ws_debug_engine_stop_after serve them; 113: ws_debug_xi_pool added, ws_engine_create knows
 * XVEC, XI_VEC_XVEC and the XI_VEC_ECAPA_TDNN names, ws_debug_engine_tap / ws_debug_engine_stop_after serve them).
 * ws_version() returns the library's value: compare it with the header's before calling anything else. */
#define WS_VERSION 113
WS_API int ws_version(void);
WS_API const char* ws_last_error(void);
/* Number of fbank frames for num_samples at snip_edges=True (25 ms / 10 ms):
 * 1 + (N - 400) / 160 at 16 kHz; 0 if N < frame length. */
WS_API int ws_num_frames(int num_samples, int sample_rate);

/* ------------------------------------------------------------------------ host-side wave loader
 * Decode threads of the batch driver (no GPU work): what the reference does in DataLoader worker processes
 * (dataset/processor.py:119-136 parse_raw / read_audio; bin/extract.py:99-103) and in wenet::WavReader
 * (runtime/core/frontend/wav.h:71-117).  RIFF/WAVE 16-bit integer PCM only; channel 0 is kept.
 * ws_wav_probe: per file the number of samples per channel (-1: not readable as PCM16) and the sample rate;
 * returns the number of unreadable files.
 * ws_wav_load_rows: samples [start[i], start[i] + count[i]) of file i (start NULL = 0) into row i of dst
 * (HOST, e.g. pinned; n rows of row_stride int16; the tail of a row is left untouched).  WS_OK or a negative
 * error naming the first file that could not supply its samples.  `threads` std::threads share the files. */
WS_API int ws_wav_probe(const char* const* paths, int n, int threads, int32_t* num_samples, int32_t* sample_rate);
WS_API int ws_wav_load_rows(const char* const* paths, int n, int threads, int16_t* dst, int64_t row_stride,
                     const int32_t* start, const int32_t* count);

/* -------------------------------------------------------------------------------- frontend */
/* Replaces torchaudio.compliance.kaldi.fbank as called at cli/speaker.py:92-97 and
 * dataset/processor.py:518-525 (+ CMN cli/speaker.py:98-99, dataset_utils.py:19-26); native twin
 * runtime/core/frontend/fbank.h:33-97 (constructor: mel banks, window).  dither is always 0.
 * Any sample rate whose 25 ms frame pads to a transform of 16 .. 4096 points (fbank.h:33-52: fft_points =
 * UpperPowerOfTwo(frame_length)): 8 kHz (the SRE recipe, examples/sre/v2/conf/resnet.yaml:31) -> 256, 16 kHz -> 512,
 * 32 kHz -> 1024, 44.1 / 48 kHz -> 2048; 1..128 mel bins; low_freq 20 Hz, high_freq = Nyquist as in the reference's
 * calls.  WS_ERR_INVALID_ARG outside that range. */
WS_API int ws_frontend_create(int sample_rate, int num_mel_bins, int device_id, ws_frontend** out);
WS_API void ws_frontend_destroy(ws_frontend* fe);
/* Which apply_cmvn (dataset/dataset_utils.py:19-26) the frontend's CMVN step is: test_conf['cmvn_args'] of
 * bin/extract.py:124-127.  norm_mean subtracts the per-utterance mean over T from every mel bin; norm_var divides by
 * sqrt(var + 1e-7), var = the unbiased estimate over T (torch.var).  Default (1, 0) = cli/speaker.py:98-99.
 * (0, 0) = `cmvn: False`: no normalisation anywhere.  Applies wherever a call of this frontend normalises:
 * ws_fbank / ws_fbank_ragged with cmn != 0 and the fused ws_extract / ws_extract_ragged. */
WS_API int ws_frontend_set_cmvn(ws_frontend* fe, int norm_mean, int norm_var);
/* wav: DEVICE (B, wav_stride) samples, the first num_samples of each row are used.
 * scale multiplies samples on load (1.0 for int16-range input; 32768.0 reproduces
 * processor.py:516 `waveform * (1 << 15)` for [-1,1] floats).
 * feats: DEVICE (B, T, num_mel_bins) float32, T = ws_num_frames(num_samples).
 * cmn != 0 subtracts the per-utterance mean over T from every mel bin. */
WS_API int ws_fbank(ws_frontend* fe, const void* wav, int wav_dtype, int batch, int num_samples,
             int64_t wav_stride, float scale, int window_type, int cmn, float* feats,
             ws_stream stream);

/* ---------------------------------------------------------------------------------- engine */
/* Replaces get_speaker_model(name)(**model_args) + load_checkpoint (models/speaker_model.py:31-62,
 * utils/checkpoint.py:20-85, cli/speaker.py:306-335).  model_name is the reference constructor
 * name ("ECAPA_TDNN_GLOB_c512", "ECAPA_TDNN_c1024", ...).  Tensors are supplied under the
 * reference's state_dict key names (e.g. "layer2.se_res2block.1.convs.3.weight"); unknown keys
 * ("projection.*", "*.num_batches_tracked") are ignored like strict=False does.  Returns the
 * native twin of runtime/core/speaker/speaker_model.h:25-32 (SpeakerModel). */
WS_API int ws_engine_create(const char* model_name, int feat_dim, int embed_dim, int device_id,
                     ws_engine** out);
/* data: HOST float32, C-contiguous, ndim <= 4.  Returns 1 if the key was consumed, 0 if ignored. */
WS_API int ws_engine_set_tensor(ws_engine* eng, const char* key, const float* data, int ndim,
                         const int64_t* shape);
/* Checks that every required tensor arrived (WS_ERR_MISSING_TENSOR names the first missing key),
 * folds/re-lays-out the weights, uploads them and allocates workspace for max_batch utterances
 * of max_frames frames per forward chunk (larger batches are processed in chunks). */
WS_API int ws_engine_finalize(ws_engine* eng, int max_batch, int max_frames);
/* create + set_tensor x N + finalize from one flat weight file (wespeaker_amd.engine.save_native_model;
 * layout in csrc/c_api.hip): what OnnxSpeakerModel(model_path) is to the reference's native runtime
 * (runtime/core/speaker/onnx_speaker_model.cc:40-75, speaker_engine.cc:28-60) -- a caller without
 * Python hands over a path and gets a ready engine. */
WS_API int ws_engine_load(const char* path, int device_id, int max_batch, int max_frames, ws_engine** out);
/* Re-sizes the workspace of a finalized engine (weights stay): the reference accepts utterances of any
 * length (cli/speaker.py:125-167 has no cap), so callers grow the engine when a longer one arrives.
 * Synchronises the device (earlier launches may still use the old workspace). */
WS_API int ws_engine_reserve(ws_engine* eng, int max_batch, int max_frames);
WS_API int ws_engine_max_batch(const ws_engine* eng);
WS_API int ws_engine_max_frames(const ws_engine* eng);
WS_API void ws_engine_destroy(ws_engine* eng);
WS_API int ws_engine_embed_dim(const ws_engine* eng);
WS_API int ws_engine_feat_dim(const ws_engine* eng);
/* Replaces model(feats)[-1] (cli/speaker.py:163-166; bin/extract.py:133-135):
 * feats DEVICE (B, T, feat_dim) float32 (already CMN'd) -> emb DEVICE (B, embed_dim) float32. */
WS_API int ws_forward(ws_engine* eng, const float* feats, int batch, int num_frames, float* emb,
               ws_stream stream);
/* Fused Speaker.extract_embedding_from_pcm (cli/speaker.py:156-166): wav -> fbank -> CMN ->
 * forward, feature tensor kept inside the engine's workspace. */
WS_API int ws_extract(ws_engine* eng, ws_frontend* fe, const void* wav, int wav_dtype, int batch,
               int num_samples, int64_t wav_stride, float scale, int window_type, float* emb,
               ws_stream stream);
/* ---- ragged batches: utterances of DIFFERENT lengths in one device batch.
 * The reference extracts test sets one utterance at a time (batch_size 1, bin/extract.py:95,
 * cli/speaker.py:169-178) because its modules have no length argument; a batch-1 loop leaves an MI355X
 * launch-bound.  Here utterance b occupies the first num_*[b] entries of its row of the padded
 * (batch, max_*) tensor; the result of every row equals what the batch-1 call returns for it: padding never
 * enters a convolution tap (it is the conv's zero padding), CMN / SE means / attentive and statistics pooling
 * / CAM++ context segments run over the utterance's own frames (pooling_layers.py:78-85,119-144;
 * campplus.py:108-135; ecapa_tdnn.py:120-126).  The length arrays are HOST pointers (read before the call
 * returns).
 * Streams: a ws_frontend may be shared by calls on DIFFERENT streams as long as the calls themselves come from one
 * host thread at a time (no handle is thread-safe).  ws_fbank / ws_extract* only read the frontend's constant tables.
 * ws_fbank_ragged also uploads a per-call frame-count table; those tables live in a ring of 4 slots, a slot is reused
 * only after the kernels that read it have finished (the call then waits on the host for that earlier call), so up to
 * 4 ragged calls may be in flight on any mix of streams. */
WS_API int ws_fbank_ragged(ws_frontend* fe, const void* wav, int wav_dtype, int batch, const int32_t* num_samples,
                    int max_samples, int64_t wav_stride, float scale, int window_type, int cmn, float* feats,
                    ws_stream stream);   /* feats (batch, ws_num_frames(max_samples), bins); rows beyond an utterance's frames = 0 */
WS_API int ws_forward_ragged(ws_engine* eng, const float* feats, int batch, int max_frames, const int32_t* num_frames,
                      float* emb, ws_stream stream);   /* feats (batch, max_frames, feat_dim); padding rows are ignored */
/* ws_forward_ragged on features that are NOT normalised yet: apply_cmvn(norm_mean, norm_var) over every utterance's own
 * frames first (dataset/dataset_utils.py:19-26), on the engine's masked copy -- the caller's tensor is left as it is.
 * The path of `data_type: feat` lists (dataset/processor.py:171-196 parse_feat -> bin/extract.py:112-127): Kaldi
 * feature matrices come from disk, CMVN and the forward run here. */
WS_API int ws_forward_ragged_cmvn(ws_engine* eng, const float* feats, int batch, int max_frames,
                           const int32_t* num_frames, int norm_mean, int norm_var, float* emb, ws_stream stream);
WS_API int ws_extract_ragged(ws_engine* eng, ws_frontend* fe, const void* wav, int wav_dtype, int batch,
                      const int32_t* num_samples, int max_samples, int64_t wav_stride, float scale,
                      int window_type, float* emb, ws_stream stream);
/* Polyphase windowed-sinc resampling of one channel: the arithmetic of
 * torchaudio.transforms.Resample(orig_freq, new_freq) as Speaker.extract_embedding_from_pcm applies it
 * (cli/speaker.py:157-160).  orig / new are the rates divided by their gcd; kernel DEVICE float32
 * [new][2 * width + orig] is the filter bank (host-built: wespeaker_amd.audio.resample_kernel);
 * x DEVICE float32[n_in]; y DEVICE float32[n_out], n_out = ceil(new * n_in / orig). */
WS_API int ws_resample(const float* x, int64_t n_in, const float* kernel, int orig, int new_rate, int width,
                float* y, int64_t n_out, ws_stream stream);

/* Chunk-and-average extraction of ONE utterance, the native runtime's
 * SpeakerEngine::ExtractEmbedding(const int16_t*, int, std::vector<float>* avg_emb)
 * (runtime/core/speaker/speaker_engine.cc:83-159; SamplesPerChunk ctor argument speaker_engine.h:29-31).
 * fbank over the whole waveform; frames cut into chunks of 1 + (samples_per_chunk - 25 ms) / 10 ms
 * frames; a trailing partial chunk is completed with the head frames of the first chunk, an utterance
 * shorter than one chunk is tiled cyclically; per-chunk CMN (ApplyMean); all chunks go through the
 * model as one batch; emb = mean of the chunk embeddings.  samples_per_chunk <= 0 = "full mode" (one
 * chunk holding every frame).  wav DEVICE (num_samples) int16 or float32 as in ws_fbank;
 * emb DEVICE float32[embed_dim].  Returns the number of chunks (>= 1) or a negative WS_ERR_*.
 * Grows an engine-owned scratch on first use / larger input (synchronises then). */
WS_API int ws_extract_chunked(ws_engine* eng, ws_frontend* fe, const void* wav, int wav_dtype,
                       int num_samples, int samples_per_chunk, float scale, int window_type,
                       float* emb, ws_stream stream);

/* Cepstral mean normalisation of features that already live on the device, in place:
 * feats[b, t, :] -= mean_t feats[b, :, :]  (cli/speaker.py:98-99; the per-window form of
 * Speaker.extract_embedding_from_feats(..., subseg_cmn=True), cli/speaker.py:108-112, and
 * diar/extract_emb.py:88-90).  feats DEVICE float32 (batch, num_frames, feat_dim). */
WS_API int ws_cmn(float* feats, int batch, int num_frames, int feat_dim, ws_stream stream);
/* apply_cmvn(feats, norm_mean, norm_var) (dataset/dataset_utils.py:19-26) in place on device features. */
WS_API int ws_cmvn(float* feats, int batch, int num_frames, int feat_dim, int norm_mean, int norm_var,
            ws_stream stream);

/* Diarization sub-segment extraction of ONE speech segment in one call: the loop body of Speaker.diarize
 * (cli/speaker.py:232-251) = compute_features(cmn=False) -> subsegment() (diar/extract_emb.py:55-83) ->
 * extract_embedding_from_feats (cli/speaker.py:108-123).
 * fbank over the whole segment; windows of `window_frames` frames every `period_frames` (150 / 75 for the
 * reference's 1.5 s / 0.75 s at a 10 ms shift), laid out from `seg_length` -- the reference derives it from the
 * segment's time stamps, (end_ms - begin_ms) / frame_shift, which is ws_num_frames() + 2 for its own VAD segments
 * (the comment at extract_emb.py:62-65) -- with every slice clipped to the frames that exist and completed to a
 * full window by tiling its own rows cyclically (np.resize); seg_length <= window_frames: ONE window tiled from
 * the whole fbank.  Optional per-window CMN; all windows go through the model as one batch.
 * ws_num_windows: how many windows that is (0 for a non-positive argument).
 * wav DEVICE (num_samples) int16 or float32 as in ws_fbank; emb DEVICE float32 [max_windows][embed_dim], rows
 * [0, n) are written.  Returns n (>= 1) or a negative WS_ERR_* (WS_ERR_CAPACITY: more windows than max_windows,
 * or window_frames beyond the finalized frame capacity).  Shares the engine-owned scratch of ws_extract_chunked. */
WS_API int ws_num_windows(int seg_length, int window_frames, int period_frames);
WS_API int ws_extract_windows(ws_engine* eng, ws_frontend* fe, const void* wav, int wav_dtype, int num_samples,
                       int seg_length, int window_frames, int period_frames, float scale, int window_type,
                       int subseg_cmn, float* emb, int max_windows, ws_stream stream);

/* Contraction back-end of every conv/linear GEMM (the reference computes them in fp32):
 *   WS_PREC_FP32    exact fp32 products on v_mfma_f32_32x32x2_f32 (default; 157 TF peak)
 *   WS_PREC_F16X3   each fp32 operand split x = hi + lo into two binary16 values (22 significant
 *                   bits) and the product formed as hi*hi + hi*lo + lo*hi on
 *                   v_mfma_f32_32x32x16_f16 with fp32 accumulation: ~2^-21 relative product error,
 *                   i.e. fp32-grade results at 3/16 of the fp32-MFMA issue cost.
 *   WS_PREC_F16     operands rounded to binary16, ONE MFMA pass, fp32 accumulation -- the arithmetic
 *                   of the reference's own GPU deployment (TensorRT fp16, runtime/server/x86_gpu):
 *                   ~5e-4 relative on the embedding, 1 - cos ~ 4e-7 against the fp32 reference
 *                   (the 1e-4 bar holds with > 100x margin); inputs and activations must stay inside
 *                   the binary16 range (65504), which int16-scale fbank + CMN features and BN-normalised
 *                   activations do -- ws_engine_check_range reports a checkpoint that does not.
 * May be switched at any time between forwards. */
#define WS_PREC_FP32 0
#define WS_PREC_F16X3 1
#define WS_PREC_F16 2
WS_API int ws_engine_set_precision(ws_engine* eng, int mode);
/* Range guard of WS_PREC_F16 / WS_PREC_F16X3: a checkpoint whose activations pass 65504 turns them into
 * inf, which reaches the embedding as inf / NaN.  Every forward in those modes ends with a tiny kernel
 * that counts non-finite embedding values into a host-visible counter; this call synchronises `stream`,
 * returns WS_ERR_RANGE (message in ws_last_error) if any were produced since the last call, else WS_OK,
 * and clears the counter.  (The reference's fp32 path has no such limit: switch to WS_PREC_FP32.) */
WS_API int ws_engine_check_range(ws_engine* eng, ws_stream stream);
/* Diagnostic (no reference counterpart): which kernel every distinct conv / linear problem was given.  The
 * dispatcher chooses among a dozen tile shapes and staging forms by shape and operand type; a layer that falls
 * off the fast forms costs speed, never correctness, so nothing else would show it.  mode 0 off, 1 on, 2 on and
 * forget what was noted (also: environment WS_DISPATCH_LOG=1 at load time).  The report is text, one line per
 * distinct (problem, kernel) with its launch count; the call returns the bytes the whole report needs
 * (including the terminator) and writes at most cap of them -- call with (NULL, 0) for the size.
 * tests/golden/dispatch_*.txt pin the tables of the BASELINE models. */
WS_API int ws_debug_dispatch_log(int mode);
WS_API long long ws_debug_dispatch_report(char* buf, long long cap);
/* Gather yardstick of bench.py's PLDA roofline (no reference counterpart): out[p] = sum of the row_len doubles of row
 * idx[p] of `table` -- the row-gather path of ws_plda_llr_pairs (tables resident in L2 / Infinity Cache) with no second
 * operand.  Device pointers; row_len even. */
WS_API int ws_debug_row_gather(const double* table, int row_len, const int32_t* idx, int64_t n, double* out,
                               ws_stream stream);
/* Clock probe of bench.py's sustained leg (no reference counterpart): ONE wavefront that stores `samples` pairs
 * (shader-clock counter, constant-rate counter) into out[2 * samples] (DEVICE), one pair every `period_ticks` ticks of
 * the constant-rate counter, sleeping in between.  Enqueued on a side stream it runs next to whatever the other
 * streams execute and shows the shader clock the chip held under that load.  1..4096 samples, period 1..2^24 ticks. */
WS_API int ws_debug_clock_probe(uint64_t* out, int samples, int64_t period_ticks, ws_stream stream);
/* Reproducer switch of the fbank kernel (process-wide; tests and tools/fbank_race_probe.py only -- DESIGN.md 6.0).
 * The round-3 build of runtime/core/frontend/fbank.h:138-198's arithmetic used the packed-fp32 instruction forms in
 * its power-spectrum loop; next to binary16 GEMMs on another stream those returned wrong values in lanes 48..63.
 * mode 0 = the shipped kernels (no packed-fp32 forms), 1 = the round-3 packed build, 2 = the any-length kernel (the one
 * that serves every rate whose 25 ms frame does not pad to 512 points) also for 512-point frontends: at 16 kHz its
 * outputs are the specialised kernel's bits, which is how the tests pin it.  Returns 0, or WS_ERR_INVALID_ARG for an
 * unknown mode. */
WS_API int ws_debug_fbank_mode(int mode);
/* ERes2Net's attentional feature fusion (wespeaker/models/eres2net.py:75-103) as the engine runs it, on caller-supplied
 * DEVICE buffers (tests/test_gpu_aff_fuse.py): per row m of channels-last tensors
 *   h = silu(w1 [x[m] | y[m]] + b1),  a = 1 + tanh(w2 h + b2),  out[m] = x[m] * a + y[m] * (2 - a)
 * w1 float32[channels / 4][2 * channels], b1 [channels / 4], w2 [channels][channels / 4], b2 [channels]: the two 1x1
 * convolutions with their biases and eval BatchNorms already folded in.  x / y / out: a pointer, a row stride and a
 * channel offset in floats each (multiples of 4; a channel slice of a wider row is fine), `rows` rows; out shares no
 * element with x or y.  channels: a multiple of 32 in [64, 2048].  row_len (DEVICE int32[rows / image_pixels], or NULL):
 * rows are images of image_pixels pixels in lines of image_width, and pixels whose column is >= row_len[image] are
 * stored as exact zeros whatever the inputs hold there (ragged batches).  WS_ERR_INVALID_ARG with the reason in
 * ws_last_error for anything outside that contract; nothing is launched then. */
WS_API int ws_debug_aff_fuse(const float* x, int ldx, int x_off, const float* y, int ldy, int y_off, float* out, int ldo,
                             int o_off, const float* w1, const float* b1, const float* w2, const float* b2, int rows,
                             int channels, const int32_t* row_len, int image_pixels, int image_width, ws_stream stream);
/* Gemini DF-ResNet's depthwise 3x3 convolution (wespeaker/models/gemini_dfresnet.py:35-44: conv2 + bn2 + relu) as the
 * engine runs it, on caller-supplied DEVICE buffers (tests/test_gpu_dwconv.py): over channels-last maps
 * x[((b * height + f) * width + t)][channels]
 *   out[b,f,t,c] = relu(sum_{df,dt in -1..1} x[b,f+df,t+dt,c] * w[c][3 (df+1) + (dt+1)] + bias[c])
 * with zero padding on both axes and stride 1; w float32[channels][9] and bias [channels] carry the eval BatchNorm.
 * channels: a multiple of 4; batch, height, width >= 1; fewer than 2^31 elements; pointers 16-byte aligned; out shares
 * no element with x.  row_len (DEVICE int32[batch], or NULL): input pixels with t >= row_len[b] count as padding
 * whatever they hold, output pixels there are stored as exact zeros, so a row of a ragged batch equals its batch-of-one
 * result bit for bit.  WS_ERR_INVALID_ARG with the reason in ws_last_error for anything outside that contract; nothing
 * is launched then. */
WS_API int ws_debug_dwconv3x3(const float* x, float* out, const float* w, const float* bias, int batch, int height,
                              int width, int channels, const int32_t* row_len, ws_stream stream);
/* XI pooling (wespeaker/models/pooling_layers.py:380-401, stddev=False: the xi-vector's Gaussian posterior inference) as
 * the engines run it, on caller-supplied DEVICE buffers (tests/test_gpu_tdnn.py).  x and z are fp32 rows
 * [b * num_frames + t][ldx / ldz >= channels]: the frame tensor and the output of XI's second 1x1 convolution.  Per
 * utterance b, over the frames [t0_b, t0_b + n_b) with (t0_b, n_b) = windows[2 b], windows[2 b + 1] (HOST int32; NULL:
 * every utterance's whole num_frames), and per channel d, with sp(v) = v > 20 ? v : log1p(exp(v)):
 *   lp_t = clamp(2 log(sp(z[t][d])), -15, 15),  m = max(max_t lp_t, prior_logprec[d])
 *   pooled[b][d] = (sum_t exp(lp_t - m) x[t][d] + exp(prior_logprec[d] - m) prior_mean[d])
 *                  / (sum_t exp(lp_t - m) + exp(prior_logprec[d] - m))
 * pooled: [batch][channels] contiguous; prior_mean, prior_logprec: DEVICE float32[channels].  Any channels >= 1 (16-byte
 * loads when channels, ldx and ldz are multiples of 4 and x, z are 16-byte aligned); 0 <= t0_b, n_b >= 1,
 * t0_b + n_b <= num_frames; batch <= 65535.  A row's result does not depend on the batch it is in.  Synchronises the
 * stream when windows are given.  WS_ERR_INVALID_ARG with the reason in ws_last_error for anything outside that
 * contract; nothing is launched then. */
WS_API int ws_debug_xi_pool(const float* x, int ldx, const float* z, int ldz, const float* prior_mean,
                            const float* prior_logprec, float* pooled, int batch, int num_frames, int channels,
                            const int32_t* windows, ws_stream stream);
/* Read-only tap on the activations a forward leaves in the engine's workspace (no reference counterpart; the per-layer
 * parity tests of tests/test_gpu_layers.py).  A stream-ordered device-to-device copy of the named fp32 tensor as the
 * LAST chunk of the LAST forward on this engine left it (a batch beyond max_batch runs in chunks: the tap holds the
 * utterances of the last one).  ECAPA-TDNN names, workspace layout, channels contiguous:
 *   frame level, rows = B * T_slot:  out1 (C)  cat = out2 | out3 | out4 (3C)  h (1536)
 *                                    y1, y2, y3 (C): conv1 / Res2 / conv3 output of the last block (layer4), before SE
 *                                    att (128): linear1 + tanh of the pooling, where astp_fused_kernel did not run
 *   utterance level, rows = B:       se_s (C, layer4's gate)  stats = [mean; std] (3072, GLOB models)
 *                                    bias_img (128, GLOB models)  pooled (3072)
 *   binary16 tensors of WS_PREC_F16, widened exactly to fp32 (the plain names stay the fp32 tensors, or an error where
 *   the back-end keeps none -- both exist together for T < 64):
 *                                    out1_16 (C)  cat16 (3C)  h16 (1536)  att16 (128)  y2_16 (C)
 *                                    y3_16 (C, T >= 64 only)  col16 (layer 1's im2col image, 5 * F rounded up to 64)
 *   after a stop point (ws_debug_engine_stop_after, 1 .. 3) y1 / y2 / y3 / se_s and their binary16 forms are those of
 *   THAT block, cat / cat16 hold the block outputs up to it (the later columns are stale), and h, att, stats,
 *   bias_img, pooled are refused.
 * ResNet names (tests/test_gpu_resnet_layers.py), maps in the layout [b][f][t][c] as rows = B * H * W, cols = C.  The
 * model rotates four activation buffers, so only the LAST EXECUTED block's tensors survive a forward: set a stop point
 * (ws_debug_engine_stop_after) to read an earlier block.
 *   stem     the stem's output (32)                        -- only when stopped at 0
 *   block    the last executed block's output
 *   mid      its BasicBlock conv1 / Bottleneck conv2 output (planes)
 *   sc       its shortcut convolution's output             -- only when the block has one
 *   next_y1  the NEXT block's conv1 output                 -- only when the fused conv3 + conv1 kernel ran for the block
 *   pooled (B, 2 * stats_dim)   emb_a (B, E; two-embedding models: seg_1's output after its relu + seg_bn_1 epilogue,
 *   what seg_2 reads)                                      -- only after a full forward
 * SimAM-ResNet names: block (the gated result), mid (conv1's output), sc (the downsample convolution's output), and
 * after a full forward hid (B * T', 128: the first attention layer), logits (B * T', D; D in f * C + c order),
 * pooled (B, 2D); block1 = a copy of the first block's output made during the forward.
 * ERes2Net names (tests/test_gpu_eres2net.py): stem (stopped at 0); of the last executed block: block, mid (conv1's
 * output, width * scale channels), cat (the concat conv3 reads), sc; after a full forward fuse12 / fuse123 / fuse1234
 * (the global fusions, rows = B * H * W of their level), pooled, and emb_a for two-embedding models.
 * Gemini DF-ResNet names (tests/test_gpu_gemini.py): stem (stopped at 0); of the last executed stop point: ds (a
 * downsample layer's output, no activation) or -- a block -- exp (conv1's output, 4 dim channels), dw (the depthwise
 * kernel's output, 4 dim) and block (dim); pooled, and emb_a for two-embedding models, after a full forward.
 * CAM++ names (tests/test_gpu_campplus_layers.py).  The FCM head rotates three buffers and the trunk ping-pongs two, so
 * a stop point (ws_debug_engine_stop_after, stages 0 .. 9) selects what is read:
 *   stem     the stem's output, [b][f][t][32] as rows = B * F * T      -- only when stopped at 0
 *   block    the last executed FCM residual block's output [b][f][t][32] (F = 40 after blocks 1 - 2, 20 after 3 - 4)
 *   mid      its conv1 output                                -- stops 1 .. 4 (head.conv2 writes over it)
 *   sc       its shortcut convolution's output               -- blocks 1 and 3
 *   fcm      head.conv2's output [b][F / 8][t][32]           -- from stop 5 on
 *   tdnn     the TDNN layer's output (B * T', 128), T' = (T - 1) / 2 + 1      -- stops 6 and 7
 *   dense    the last executed dense block's whole buffer (B * T', 512 / 1024 / 1024): the block input (the TDNN or
 *            the previous transit output) followed by 32 columns per layer       -- from stop 7 on
 *   transit  that block's transit output (B * T', 256 / 512 / 512), gathered from the next buffer's row stride
 *   h        (B * T', 128) the LAST layer's bottleneck output (after BN-ReLU) of that block, and
 *   mask     (B * segments, 32) that layer's context mask, segments = ceil(T' / 100) per slot -- only where the
 *            three-launch path ran (f16x3 at every length, fp32 above T' = 128): cam_dense_block_kernel keeps both in
 *            LDS; WS_PREC_F16 with one segment and T' >= 64 keeps h in binary16 only (mask still taps)
 *   pooled   (B, 1024)                                       -- only after a full forward
 * Rows beyond an utterance's own frames (ragged forward) are the zeros the kernels stored there.
 * dst DEVICE float32[cap_floats], or NULL to ask for the shape only; rows / cols (HOST, may be NULL) receive it.
 * WS_ERR_INVALID_ARG (message in ws_last_error): unknown name; a tensor the last forward did not leave in fp32
 * (WS_PREC_F16 with T >= 64 keeps the block chain and h in binary16 only, and every ResNet map; stats / bias_img exist
 * for GLOB models; a block without a shortcut has no sc, an unfused one no next_y1, a stopped forward no pooled);
 * a CAM++ tensor the stop point does not leave (above); no forward since the engine was finalized / its workspace
 * re-sized.
 * WS_ERR_CAPACITY: cap_floats < rows * cols.  The forward path itself is unchanged: a few host-side integers remember
 * the last chunk. */
WS_API int ws_debug_engine_tap(ws_engine* eng, const char* name, float* dst, int64_t cap_floats, int32_t* rows,
                               int32_t* cols, ws_stream stream);
/* Debug stop point (ResNet, SimAM-ResNet, ERes2Net, Gemini DF-ResNet, CAMPPlus, ECAPA-TDNN; no reference counterpart): every later forward on this
 * engine returns after the stem (n_blocks = 0) or after the last launch of the n-th residual block (a fused
 * conv3 + next-conv1 launch belongs to block n), so that ws_debug_engine_tap can read what those launches left.
 * Pooling and the head do not run; the embedding output is zero-filled on the stream.  -1 (the default) = the full
 * forward: with it no launch, store or dispatch decision differs from a library without the stop point (one host-side
 * integer, tested once per block).  CAM++ counts stages instead of residual blocks: 0 = the stem, 1 .. 4 = the FCM
 * residual blocks, 5 = head.conv2, 6 = the TDNN layer, 7 / 8 / 9 = dense block 1 / 2 / 3 AND its transit.  ECAPA-TDNN
 * takes 1, 2 or 3: return after that SE-Res2 block (its SE scale + residual launch), layer 1 has no stop of its own.
 * Gemini DF-ResNet counts its downsample layers too: 0 = the stem, then in forward order downsample layer 1, the blocks
 * of stage 1, downsample layer 2, ... (4 + the number of blocks stop points).
 * WS_ERR_INVALID_ARG: n_blocks < -1 or beyond the model's block / stage count (ECAPA-TDNN: 0 as well); an engine that
 * is not finalized. */
WS_API int ws_debug_engine_stop_after(ws_engine* eng, int n_blocks);
/* Algorithmic FLOPs (2 x MACs of every conv/linear) of one forward at (batch, num_frames). */
WS_API double ws_engine_flops(const ws_engine* eng, int batch, int num_frames);

/* Measurement hooks (bench.py roofline leg; no reference counterpart -- the reference only has the
 * wall-clock Timer of runtime/core/utils/timer.h:22-36).  While enabled, every kernel launch of
 * ws_forward/ws_extract is bracketed by HIP events on the launch stream.  ws_engine_profile_read
 * synchronises them and fills 4-element arrays indexed by kernel class
 * (0 = conv/linear GEMM launches with N > 64 -- whichever tile / back-end kernel the dispatcher picks:
 * the dominant class, 1 = narrow GEMMs (N <= 64) and the fused Res2 chain, 2 = reductions / element-wise
 * / frontend, 3 = split-K GEMMs): summed milliseconds, algorithmic FLOPs, algorithmic bytes, launch counts.
 * `on` is a bit mask of the classes to record (0 = off, 0xF = all, 1 = only the dominant GEMM):
 * timing events between kernels cost a few per cent of throughput, so the headline run records
 * only the dominant kernel.  Returns the number of classes. */
WS_API int ws_engine_profile_enable(ws_engine* eng, int on);
WS_API int ws_engine_profile_read(ws_engine* eng, double* ms, double* flops, double* bytes, int* launches);

/* ------------------------------------------------------------------------------------ PLDA */
/* Replaces TwoCovPLDA.load_model's in-memory state (utils/plda/two_cov_plda.py:341-363):
 * mu, psi, offset HOST float64[dim]; transform HOST float64[dim*dim] row-major. */
WS_API int ws_plda_create(int dim, const double* mu, const double* transform, const double* psi,
                   const double* offset, int normalize_length, int device_id, ws_plda** out);
WS_API void ws_plda_destroy(ws_plda* plda);
/* eval_sv pre-processing for enrollment models (two_cov_plda.py:216-235): rows of emb are grouped
 * contiguously, group g = rows [group_offsets[g], group_offsets[g+1]).  Per group: subtract
 * mean_vec (HOST float64[dim] or NULL), mean over rows, length-norm of the mean if
 * normalize_length, transform_embedding.  emb DEVICE float32 (n_rows, dim); group_offsets DEVICE
 * int32[n_groups+1]; out DEVICE float64 (n_groups, dim). */
WS_API int ws_plda_prepare_enroll(ws_plda* plda, const float* emb, const int32_t* group_offsets,
                           int n_groups, const double* mean_vec, double* out, ws_stream stream);
/* eval_sv pre-processing for test utterances (two_cov_plda.py:237-244) == transform_embedding
 * (:156-163) after optional mean subtraction / length-norm.  emb DEVICE float32 (n, dim);
 * out DEVICE float64 (n, dim). */
WS_API int ws_plda_prepare_test(ws_plda* plda, const float* emb, int n, const double* mean_vec,
                         double* out, ws_stream stream);
/* TwoCovPLDA.transform_embedding (two_cov_plda.py:156-163) verbatim: y = transform x + offset, then
 * y *= sqrt(D)/|y| iff normalize_length.  x DEVICE float64 (n, dim); out DEVICE float64 (n, dim). */
WS_API int ws_plda_transform(ws_plda* plda, const double* x, int n, double* out, ws_stream stream);
/* Dense LLR matrix: log_likelihood_ratio (two_cov_plda.py:165-184) for every (enroll i, test j).
 * enroll DEVICE float64 (n_enroll, dim) transformed; n_sessions DEVICE int32[n_enroll] (the `n`
 * argument: 1 if multisession_avg else #utts, :219-222), or NULL when every model has the same
 * count n_uniform > 0 (multisession_avg=True => n_uniform = 1): the score is then one dim-long
 * contraction plus a per-model and a per-test constant; test DEVICE float64 (n_test, dim);
 * out DEVICE float64 (n_enroll, n_test). */
WS_API int ws_plda_llr_matrix(ws_plda* plda, const double* enroll, const int32_t* n_sessions,
                       int n_uniform, int n_enroll, const double* test, int n_test, double* out,
                       ws_stream stream);
/* Explicit trial list (the eval_sv trial loop :246-256): out[p] = LLR(enroll[idx_e[p]],
 * test[idx_t[p]], n_sessions[idx_e[p]]).  idx_* DEVICE int32[num_trials]; out DEVICE float64. */
WS_API int ws_plda_llr_pairs(ws_plda* plda, const double* enroll, const int32_t* n_sessions,
                      int n_uniform, int n_enroll, const double* test, int n_test,
                      const int32_t* idx_e, const int32_t* idx_t, int64_t num_trials, double* out,
                      ws_stream stream);

/* ------------------------------------------------------------------ PLDA training statistics
 * The N x D^2 part of TwoCovPLDA training / adaptation: PldaStats.add_samples over every speaker
 * (two_cov_plda.py:48-66) after the constructor's pre-processing (:95-107: subtract the train-set
 * mean, optional length normalisation), and -- with one group -- the mean / np.cov of adapt() (:261-275).
 * emb DEVICE (n, dim) float32 (emb_is_f64 = 0) or float64 (1: rows that already went through a link of
 * the embedding-processing chain, which the reference keeps in float64), rows grouped by class: class c = rows [group_offsets[c],
 * group_offsets[c+1]); group_offsets DEVICE int32[n_groups+1]; mean_vec DEVICE float64[dim] or NULL;
 * class_mean DEVICE float64 (n_groups, dim) <- mu_c; scatter DEVICE float64 (dim, dim) <-
 * sum_c sum_{i in c} (y_i - mu_c)(y_i - mu_c)^T with y = normalised (x - mean_vec);
 * scratch DEVICE float64[>= ws_plda_stats_scratch(n, dim)].  The D x D algebra of the EM steps
 * (inv / cholesky / eigh, :116-154) stays with the caller in float64. */
WS_API int64_t ws_plda_stats_scratch(int n, int dim);
WS_API int ws_plda_stats(const void* emb, int emb_is_f64, int n, int dim, const int32_t* group_offsets, int n_groups,
                  const double* mean_vec, int normalize_length, double* class_mean, double* scatter,
                  double* scratch, int64_t scratch_doubles, ws_stream stream);

/* One link of the embedding-processing chain (wespeaker/utils/embedding_processing.py: MeanSubtraction
 * :204-216, Length_norm :181-195, Lda.__call__ :177-178) applied to n rows:
 *   y = (x - sub) M ;  if normalize: y /= |y|.
 * x DEVICE (n, d_in) float32 (x_is_f64 = 0) or float64 (1); sub DEVICE float64[d_in] or NULL;
 * M DEVICE float64 (d_in, d_out) row-major or NULL (identity, d_out must equal d_in);
 * out DEVICE float64 (n, d_out).  The LDA / mean statistics come from ws_plda_stats. */
WS_API int ws_rows_affine(const void* x, int x_is_f64, int n, int d_in, const double* sub, const double* M,
                   int d_out, int normalize, double* out, ws_stream stream);

/* ------------------------------------------------------------------ cosine scoring + AS-norm
 * Stateless device functions replacing the numpy/sklearn back-end of wespeaker/bin/score.py:38-72
 * (trials_cosine_score) and wespeaker/bin/score_norm.py:26-36,93-115 (get_mean_std + the
 * normalisation loop).  A "unit table" holds mean-subtracted, L2-normalised embeddings as
 * (ws_cos_table_rows(n), ws_cos_table_ld(dim)) float32, zero padded on both axes. */
WS_API int ws_cos_table_rows(int n);   /* n rounded up to a multiple of 4 */
WS_API int ws_cos_table_ld(int dim);   /* dim rounded up to a multiple of 32 (floats per row) */
/* emb DEVICE float32 (n, dim) dense; mean_vec DEVICE float32[dim] or NULL (score.py:44-53:
 * emb - mean_vec); unit DEVICE table as above (written in full, padding zeroed); mag DEVICE
 * float32[n] or NULL receives |emb - mean_vec| (the enroll_mag/test_mag columns, score_norm.py:107). */
WS_API int ws_cos_prepare(const float* emb, const float* mean_vec, int n, int dim, float* unit, float* mag,
                   ws_stream stream);
/* out[p] = <unit_a[idx_a[p]], unit_b[idx_b[p]]> = cosine_similarity (score.py:62-63).
 * idx_* DEVICE int32[num_trials]; out DEVICE float32[num_trials]. */
WS_API int ws_cos_pairs(const float* unit_a, const float* unit_b, int dim, const int32_t* idx_a,
                 const int32_t* idx_b, int64_t num_trials, float* out, ws_stream stream);
/* Dense cosine matrix out[i][j] = <unit_a[i], unit_b[j]> (score_norm.py:29 np.matmul(emb, cohort.T))
 * on the exact-fp32 MFMA GEMM.  out DEVICE float32 (n_a, ldo), ldo >= ws_cos_table_rows(n_b);
 * columns n_b..ws_cos_table_rows(n_b)-1 receive zeros. */
WS_API int ws_cos_matrix(const float* unit_a, int n_a, const float* unit_b, int n_b, int dim, float* out,
                  int ldo, ws_stream stream);
/* get_mean_std (score_norm.py:26-36): for every row of `unit`, mean and population standard
 * deviation (np.std) of its min(top_n, n_cohort) largest cosine scores against the cohort
 * (asnorm: top_n; snorm: top_n >= n_cohort).  scratch DEVICE float32[scratch_floats] holds score
 * rows in flight; it needs at least 128 * ws_cos_table_rows(n_cohort) floats and the rows are
 * processed in as few chunks as it allows.  mean, sd DEVICE float32[n]. */
WS_API int ws_cohort_stats(const float* unit, int n, const float* unit_cohort, int n_cohort, int dim,
                    int top_n, float* scratch, int64_t scratch_floats, float* mean, float* sd,
                    ws_stream stream);
/* score_norm.py:100-103: out[p] = 0.5 * ((s[p] - e_mean[ie]) / e_sd[ie] + (s[p] - t_mean[it]) / t_sd[it]).
 * All DEVICE; score/out float32[num_trials]. */
WS_API int ws_asnorm_pairs(const float* score, const int32_t* idx_e, const int32_t* idx_t,
                    const float* e_mean, const float* e_sd, const float* t_mean, const float* t_sd,
                    int64_t num_trials, float* out, ws_stream stream);

/* ------------------------------------------------------------------------ spectral clustering
 * The n-sized half of the reference's diarization clusterer, wespeaker/diar/spectral_clusterer.py:33-87
 * (cluster()): affinity, pruning, Laplacian, and the products an iterative eigen-solver needs.  The b x b
 * algebra of the solver and the k-means (:65-69) stay with the caller in float64 (wespeaker_amd/diar.py).
 * 3 <= n <= 8192 everywhere (spectral_clusterer.py:72-73 answers n <= 2 without a graph; above 8192
 * WS_ERR_CAPACITY: the transient n x n fp32 affinity is 256 MB there).  Panels X, Z, Y, LX are DEVICE
 * float64 (n, b) row-major with 1 <= b <= 64. */
/* spectral_clusterer.py:40-44: how many entries of a row of n survive prune(M, p) -- n - max(n - 10, 2)
 * below 1000 rows, n - int((1 - p) * n) from 1000 on -- clamped to 0 .. n.  Pure function. */
WS_API int ws_spectral_keep(int n, double p);
/* Bytes of DEVICE scratch that ws_spectral_graph / ws_spectral_gram need for n rows of dim floats
 * (0 for an n or dim they refuse). */
WS_API int64_t ws_spectral_scratch(int n, int dim);
/* Bytes of DEVICE scratch that ws_spectral_gram alone needs for n rows (its partial sums; at most 4 MiB): a
 * caller that has released the graph's scratch -- it holds the n x n affinity -- keeps only this much for the
 * solve (spectral_clusterer.py:59).  0 for an n it refuses. */
WS_API int64_t ws_spectral_gram_scratch(int n);
/* spectral_clusterer.py:35-56 up to the Laplacian's parts.  emb DEVICE float32 (n, dim) dense, rows are
 * L2-normalised here (:36, no mean subtraction); the cosine matrix runs on the exact-fp32 MFMA GEMM of
 * ws_cos_matrix (:37; 0.5 * (1 + cos) is monotone and is not materialised); each row keeps its `keep`
 * largest entries (:46-50, keep = ws_spectral_keep(n, p)) -- EXACTLY keep of them: among values equal to
 * the keep-th largest the higher column index stays, which is what the stable `np.argsort(row)[n:]` of :47-48
 * keeps; P holds 1 there, M = (P + P^T) / 2 (:51), its diagonal is zeroed (:54).
 * Out, all DEVICE: CSR of M -- rowptr int32[n + 1] (rowptr[n] = number of non-zeros), colidx int32[cap]
 * ascending inside a row, vals float64[cap] (0.5 or 1) -- and deg float64[n] = row sums of M (:55), so that
 * L = diag(deg) - M (:56).  cap >= min(n * (n - 1), 2 * n * keep) always suffices; nothing is written at
 * or past cap, and a caller that passed less must compare rowptr[n] with it. */
WS_API int ws_spectral_graph(const float* emb, int n, int dim, int keep, void* scratch, int64_t scratch_bytes,
                      int32_t* rowptr, int32_t* colidx, double* vals, int64_t cap, double* deg,
                      ws_stream stream);
/* Y = alpha * (L X) + beta * X + gamma * Z with L X = deg (.) X - M X from the CSR (the Laplacian of
 * spectral_clusterer.py:53-56 is never formed): one step of a three-term (Chebyshev) recurrence in one
 * launch; beta = gamma = 0 gives the plain product.  Z may be NULL when gamma == 0; Y may be Z, not X.  The
 * sum over a row's neighbours runs in CSR order: results are reproducible. */
WS_API int ws_spectral_apply(const int32_t* rowptr, const int32_t* colidx, const double* vals, const double* deg,
                      int n, int b, double alpha, double beta, double gamma, const double* X, const double* Z,
                      double* Y, ws_stream stream);
/* G = X^T X and H = X^T LX (DEVICE float64 (b, b) each) in one call: the reduced pair whose eigen-problem
 * replaces scipy.linalg.eigh of the n x n Laplacian (spectral_clusterer.py:59).  The reduction order
 * depends on (n, b) only -- no floating-point atomics -- so two calls give the same bits. */
WS_API int ws_spectral_gram(const double* X, const double* LX, int n, int b, double* G, double* H, void* scratch,
                     int64_t scratch_bytes, ws_stream stream);
/* out = X W + gamma * Z, W DEVICE float64 (b, b) row-major: the basis update X <- X W of a Rayleigh-Ritz
 * step (the eigenvectors of spectral_clusterer.py:59 are X W at convergence), and with W = -diag(theta),
 * Z = LX, the residual panel L V - V theta.  out may be X (in place) or Z; Z may be NULL when gamma == 0. */
WS_API int ws_spectral_rotate(const double* X, const double* W, double gamma, const double* Z, double* out, int n,
                       int b, ws_stream stream);
/* Debug / tests: the Laplacian of spectral_clusterer.py:53-56 densified, L DEVICE float64 (n, n). */
WS_API int ws_debug_spectral_dense(const int32_t* rowptr, const int32_t* colidx, const double* vals,
                            const double* deg, int n, double* L, ws_stream stream);
/* Debug / tests: the pruning mask (spectral_clusterer.py:46-50, before symmetrisation) that the last
 * ws_spectral_graph(n, dim) left in `scratch`; mask_out DEVICE uint32 (n, ceil(n / 32)), bit j of row i. */
WS_API int ws_debug_spectral_mask(const void* scratch, int n, int dim, uint32_t* mask_out, ws_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* WESPEAKER_AMD_H_ */
