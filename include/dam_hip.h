/*
 * dam_hip.h -- C ABI of libdam_hip.so, the MI355X (gfx950) implementation of the
 * deep-audio-mixer hot path.
 *
 * The reference (apelykh/deep-audio-mixer) has no FFI: its hot path is reached through
 * torch.stft / torch.nn on one device.  Each entry point below names the reference
 * code (file:line, relative to the reference root) whose arithmetic it replaces; the
 * Python mirror of the reference interface (deep-audio-mixer_amd/) binds these through
 * ctypes, see INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller unless the name ends in
 *     _host; the library allocates nothing and keeps no state;
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*), never
 *     synchronises, and is hipGraph-capturable;
 *   - returns DAM_OK (0) or a negative dam_status; never throws across the ABI;
 *   - activations are NHWC float32 ("pixels x channels", channel count a multiple of 16
 *     unless stated); tensors the reference API exposes (features, masked, gains) are in
 *     the reference's own layout ([B,S,F,T] / [B,F,T] / [B,S]).
 */
#ifndef DAM_HIP_H
#define DAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum dam_status {
    DAM_OK = 0,
    DAM_ERR_BAD_ARG = -1,        /* null pointer, non-positive size, N <= n_fft/2 ... */
    DAM_ERR_UNSUPPORTED = -2,    /* shape/dtype outside what the gfx950 kernels implement */
    DAM_ERR_LAUNCH = -3,         /* hipGetLastError() != hipSuccess after the launch */
    DAM_ERR_WORKSPACE = -4       /* caller-provided workspace too small */
} dam_status;

/* Sample types the front-end reads.  DAM_PCM_S16 / DAM_PCM_S32: integer PCM exactly as the WAV file holds it (interleaved or
 * mono), scaled by 1/2^15 / 1/2^31 as soundfile.read does (data/dataset.py:194) -- no host conversion, half the PCIe bytes
 * for 16-bit files; results are bit-identical to DAM_PCM_F32 on host-converted samples.  24-bit files: the reader unpacks
 * them to left-justified DAM_PCM_S32 (value << 8).  Strides are counted in samples of the given type. */
typedef enum dam_pcm_dtype { DAM_PCM_F32 = 0, DAM_PCM_F64 = 1, DAM_PCM_S16 = 2, DAM_PCM_S32 = 3 } dam_pcm_dtype;
/* OR-ed into pcm_dtype: `pcm` is a DEVICE word holding the address of the PCM (const void* const*), read when the kernel
 * starts.  A launch captured in a hipGraph then follows whichever resident batch the word points at -- the caller re-points
 * the word (8 bytes) instead of copying a batch into the graph's fixed input buffer.  Layout arguments describe the pointee. */
#define DAM_PCM_INDIRECT 0x100
/* OR-ed into pcm_dtype instead: `pcm` is a DEVICE table of int64 words {address of an int64 step counter, n, offset, addr[0] ...
 * addr[n-1]} and the launch reads the batch at addr[(counter + offset) % n].  With the optimizer's device-side step count as the
 * counter (dam_adam_l2_step_f32 advances it inside the captured step) a replayed step walks n resident batches -- or the n
 * staging buffers of an uploader -- with NO launch between the replays: re-pointing the DAM_PCM_INDIRECT word was a 4.8 us fill
 * launch behind an 8 us gap per step (profiles/r05_C3_step_timeline.txt, the last line).  n >= 1, counter + offset >= 0. */
#define DAM_PCM_ROTATE 0x200
struct dam_bn_bwd_sums; /* defined in the BatchNorm section */
struct dam_bn_bwd_in;

/* Library / build identification ("gfx950").  DAM_ABI_VERSION is bumped whenever a signature below changes; a binding
 * compares dam_abi_version() of the library it loaded with the version it was written against and refuses a stale one
 * (deep-audio-mixer_amd/_lib.py: EXPECTED_ABI). */
#define DAM_ABI_VERSION 39
const char* dam_arch(void);
int dam_abi_version(void);

/* Host-side fork guard for the loaders of the reference's notebooks: training.ipynb cell 6 / training_ignite.ipynb cell 6 build
 * DataLoader(d_train, num_workers=6, pin_memory=True) over data/dataset.py:270-292, i.e. the process that owns the GPU forks
 * six workers at the start of EVERY epoch.  On this stack page-locked host memory (hipHostMalloc: torch's pinned tensors,
 * the runtime's staging buffers) is anonymous memory registered with the GPU as user pointers and NOT marked MADV_DONTFORK:
 * a fork write-protects it for copy-on-write, the driver's MMU notifier evicts the process's GPU queues and restores them
 * only later -- measured 0.2-0.6 s of GPU stall per fork batch in a toy process, 4-5 s per epoch in the C3 training loop
 * (profiles/r05_fork_stall.txt).  This call marks the private anonymous mappings of the calling process that ARE page-locked
 * data buffers handed out by the HIP layer (hipPointerGetAttributes: hipMemoryTypeHost; extent from hsa_amd_pointer_info)
 * MADV_DONTFORK: children forked afterwards do not inherit those buffers (they cannot use the GPU anyway) and the fork no
 * longer write-protects them.  The runtime's internal pools are left alone (a child that runs a destructor of an inherited
 * GPU object reads them).  No device pointers, no stream, nothing enqueued; call it from the GPU-owning process only, after
 * the runtime is initialised.
 *   n_mappings_host / n_bytes_host : optional outputs, ranges and bytes marked by this call (re-marking is harmless). */
int dam_host_dontfork_pinned(int64_t* n_mappings_host, int64_t* n_bytes_host);

/* Step marks (ABI 15): a point INSIDE a captured training step that another stream can wait for.  The reference uploads every
 * batch on the training stream, `train_features.to(self.device)` at model_trainer.py:34 and `gt_features.to(...)` at :35, from
 * the page-locked batches of DataLoader(pin_memory=True) (training.ipynb cell 6).  Here the step is ONE hipGraph and the upload
 * of batch k+1 runs on a copy stream beside step k; measured (profiles/r05_pcie_trace.txt), a 1.3 ms host-to-device copy beside
 * the FORWARD half of the step costs its latency-bound launches (the BatchNorm finalize kernels: 4.7 -> 7.7 us each) 0.13 ms per
 * step, beside the shallow layers' backward it costs a third of that.  A mark is a HIP event recorded with
 * hipEventRecordExternal while the step is being captured (an event-record node of the graph, re-recorded by every replay;
 * outside a capture: an ordinary record), so the copy stream waits for "step k has reached its backward pass" -- the graph is
 * not cut.  The front-end has read the step's PCM long before any mark of the step, so the same wait also says the previous
 * staging buffer is free.
 *   dam_step_mark_create : *mark_host receives the handle (timing disabled).
 *   dam_step_mark_record : on `stream`; captured as an external event-record node when the stream is capturing.
 *   dam_step_mark_wait   : makes `stream` (never a capturing one: DAM_ERR_BAD_ARG) wait for the latest record that has been
 *                          enqueued -- directly or through a graph launch -- before this call; a no-op if there is none.
 *   dam_step_mark_synchronize: the HOST waits for that record.  This is the form the uploader uses: measured on this stack
 *                          (profiles/r05_sync_cost_probe.txt), ANY stream that waits for an event of the training stream costs
 *                          the training stream 0.09 ms per step (4.125 -> 4.212 ms; event flags make no difference), a host
 *                          wait costs nothing (4.138-4.143 against 4.139-4.145 ms) -- so the host waits for the mark and then
 *                          enqueues the copy, and only the cheap direction (the training stream waiting for the copy stream's
 *                          event) stays on the device.
 *   dam_step_mark_destroy: after the graphs that hold the mark are gone. */
int dam_step_mark_create(void** mark_host);
int dam_step_mark_record(void* mark, void* stream);
int dam_step_mark_wait(void* mark, void* stream);
int dam_step_mark_synchronize(void* mark);
int dam_step_mark_destroy(void* mark);

/* ---------------------------------------------------------------------------------
 * Feature front-end.  Replaces data/dataset.py:132-162 (compute_features: torch.stft ->
 * abs -> amplitude_to_DB), :181-183 (_stereo_to_mono), :164-168 (_augment_audio) and the
 * stacking at :207-210, for a whole batch of tracks in one launch.
 * --------------------------------------------------------------------------------- */

/* Host helper: number of float2 entries of the twiddle table for n_fft (n_fft entries:
 * W_{n_fft}^k = exp(-2 pi i k / n_fft)), and a routine that fills it (computed in double). */
int64_t dam_stft_twiddle_count(int n_fft);
int dam_stft_fill_twiddles_host(int n_fft, float* table_host /* [2*count] re,im */);

/* out[track][f][t] = 20*log10(max(|STFT(mean_c pcm[track][:, c] * gain[track])|, amin))
 *   pcm      : [n_tracks][n_samples][channels], dtype per pcm_dtype, interleaved channels;
 *              track k starts at pcm + k*pcm_track_stride elements
 *   window   : [n_fft] float32 (the caller uploads torch.hann_window(n_fft))
 *   twiddles : table from dam_stft_fill_twiddles_host
 *   gain     : optional [n_tracks] float32 (nullptr = 1), the augmentation draw
 *   normalize: 0, or 1 = divide every frame (column) by its max-abs over bins
 *              (librosa.util.normalize semantics of the call disabled at data/dataset.py:159-160)
 *   out      : [n_tracks][n_fft/2+1][T] float32, T = 1 + n_samples/hop
 * center=True / reflect padding / onesided / unnormalised, as torch.stft's defaults.
 * Supported: channels 1 or 2, n_samples > n_fft/2, hop >= 1; n_fft == 2048 with an even hop (every call site of the
 * reference: data/dataset.py:132-133 defaults) runs the tuned in-register kernel, any other power of two from 64 to 16384
 * (or an odd hop) a generic one-workgroup-per-frame kernel; window then has n_fft entries (torch.hann_window(n_fft)). */
int dam_stft_logmag_f32(const void* pcm, int pcm_dtype, int64_t n_tracks, int64_t n_samples, int channels,
                        int64_t pcm_track_stride, const float* window, const float* twiddles,
                        const float* gain, int n_fft, int hop, float amin, int normalize,
                        float* out, void* stream);

/* The same front-end over strided PCM, so that tracks need not be gathered first.  Track (o, i), o < n_outer,
 * i < n_inner, is output row o*n_inner + i and starts at pcm + o*outer_stride + i*inner_stride (elements); sample p of
 * channel c is at + p*sample_stride + c*channel_stride.  Two layouts are implemented: interleaved channels
 * (sample_stride == channels, channel_stride == 1: what a WAV decoder / soundfile hands over, data/dataset.py:194) and
 * planar channels (sample_stride == 1, channel_stride >= n_samples: the [channels, n] arrays that
 * inference_utils.py:116-119 slices chunk by chunk -- outer = chunk (stride chunk_samples), inner = stem).
 * gain (optional) has one entry per track, index o*n_inner + i.
 * n_tail > 0 splits the output the way a dataset item is split (data/dataset.py:207-210: train_features = the stems,
 * gt_features = the mix): tracks i < n_inner - n_tail go to out [n_outer][n_inner - n_tail][F][T], the last n_tail
 * tracks of every outer group to out_tail [n_outer][n_tail][F][T] -- one launch for a whole batch of clips. */
int dam_stft_logmag_strided_f32(const void* pcm, int pcm_dtype, int64_t n_outer, int64_t outer_stride, int64_t n_inner,
                                int64_t inner_stride, int64_t n_samples, int channels, int64_t sample_stride,
                                int64_t channel_stride, const float* window, const float* twiddles, const float* gain,
                                int n_fft, int hop, float amin, int normalize, float* out, float* out_tail, int n_tail,
                                void* stream);

/* Complex spectra and their inverse (ABI 17).  The reference listens to a prediction in experiments.ipynb: cell 44 takes
 * librosa.stft of every stem, cell 50 the stft of the stems' sum and keeps its PHASES, cell 53 re-synthesises
 * librosa.istft(db_to_amplitude(masked) * phases, hop_length=512) from the predicted dB spectrogram `masked`
 * (the quantity data/dataset.py:145-149 computes with torch.stft and every model here is trained on).
 *
 * dam_stft_complex_f32: the front-end above up to, but not including, |.| -> dB:
 *   out[track][f][t] = (re, im) float32 = torch.stft(sum_s mean_c pcm[track + s][:, c] * gain[track], n_fft, hop,
 *   window=w, center=True, return_complex=True).  PCM conventions as dam_stft_logmag_f32 (dtypes, 1 or 2 channels averaged
 *   at load, optional gain, float32 Hann table, the twiddle table).  n_sum >= 1 tracks, sum_stride elements apart, are
 *   ADDED at load (float32, ascending s): the "STFT of the stems' sum" of cell 50 without a torch kernel for the sum.
 *   dam_stft_complex_strided_f32 addresses tracks like dam_stft_logmag_strided_f32 (for all chunks of a planar song:
 *   outer = chunk, n_inner = 1, n_sum = stems).  out: [n_tracks][n_fft/2+1][T] float2, T = 1 + n_samples/hop; the
 *   imaginary parts of the DC and Nyquist bins are 0.  n_fft: a power of two from 64 to 16384, hop >= 1; every size runs
 *   the one-workgroup-per-frame kernel.
 *
 * dam_istft_f32: torch.istft(spec, n_fft, hop, window=w, center=True, normalized=False, onesided=True, length=length):
 *   out[track][n] = (sum_t w[j] irfft(X[track][:, t])[j]) / (sum_t w[j]^2),  j = n + n_fft/2 - t*hop in [0, n_fft),
 *   0 <= n < length; samples no frame covers (envelope <= 1e-11, torch's threshold) are 0.
 *   spec   : [n_tracks][n_fft/2+1][n_frames] float2 (re, im)
 *   mag_db : optional [n_tracks][n_fft/2+1][n_frames] float32; the bin used is then 10^(0.05 mag_db) * spec/|spec|, the phase
 *            of spec ((1, 0) where spec == 0): cell 53 without a phase tensor.  The imaginary parts of the DC and Nyquist
 *            bins are ignored, as irfft ignores them.
 *   window, twiddles : the tables the forward uses (synthesis window = analysis window)
 *   out    : [n_tracks][length] float32
 *   workspace : dam_istft_workspace_bytes(...) bytes (0 today: may be nullptr), DAM_ERR_WORKSPACE if smaller.
 * Accepted: n_fft a power of two from 64 to 16384 and 1 <= hop <= n_fft/2 (for Hann the envelope is then >= 0.5 on every
 * covered sample); anything else is DAM_ERR_UNSUPPORTED before the device is touched -- torch raises for a vanishing
 * envelope, this refuses the geometries where one can occur.  Deterministic: every sample is the sum of its covering
 * frames in frame order (a gather, no atomics), identical bits between runs and batch sizes.  Enqueued on `stream`,
 * no synchronisation, no allocation, capturable. */
int dam_stft_complex_f32(const void* pcm, int pcm_dtype, int64_t n_tracks, int64_t n_samples, int channels,
                         int64_t pcm_track_stride, int64_t n_sum, int64_t sum_stride, const float* window,
                         const float* twiddles, const float* gain, int n_fft, int hop, float* out, void* stream);
int dam_stft_complex_strided_f32(const void* pcm, int pcm_dtype, int64_t n_outer, int64_t outer_stride, int64_t n_inner,
                                 int64_t inner_stride, int64_t n_sum, int64_t sum_stride, int64_t n_samples, int channels,
                                 int64_t sample_stride, int64_t channel_stride, const float* window, const float* twiddles,
                                 const float* gain, int n_fft, int hop, float* out, void* stream);
int64_t dam_istft_workspace_bytes(int64_t n_tracks, int64_t n_frames, int n_fft, int hop, int64_t length);
int dam_istft_f32(const float* spec, const float* mag_db, int64_t n_tracks, int64_t n_frames, int n_fft, int hop,
                  int64_t length, const float* window, const float* twiddles, float* out, void* workspace,
                  int64_t workspace_bytes, void* stream);

/* The augmentation draw of data/dataset.py:164-168,198-199 (one uniform gain per track of an item, the mix included)
 * made on the device and reproducibly: gains[i][k] = lo + (hi - lo) * u(seed, item_i, k), u in [0, 1) a counter-based
 * hash (splitmix64) of (seed, GLOBAL item index, track).  items: optional DEVICE int64[n_items] of global item (chunk)
 * indices; nullptr = first_item, first_item + 1, ...  gains [n_items][n_tracks] feeds dam_stft_logmag_*'s `gain`. */
int dam_augment_gains_f32(uint64_t seed, const int64_t* items, int64_t first_item, int n_items, int n_tracks,
                          float lo, float hi, float* gains, void* stream);

/* ---------------------------------------------------------------------------------
 * Convolutions.  Replace nn.Conv2d forward and its autograd data-gradient in
 * models/model_resnet.py:11-21,64 (BasicBlock / stem convs) and
 * models/model_scalar_1s.py:167-172, models/model_scalar_2s.py:25-30 (ConvBlock2d.conv).
 * Implicit GEMM on the fp32 matrix cores; activations NHWC float32.
 * --------------------------------------------------------------------------------- */

/* Number of floats of the packed weight image for an operator with n_out output and k_in
 * reduction channels: [kh*kw][ceil(k_in/16)][ceil(n_out/16)][4][16][4]. */
int64_t dam_conv_packed_weight_count(int n_out, int k_in, int kh, int kw);

/* Pack torch-layout weights [O][I][KH][KW] for the forward (transpose=0: n_out=O, k_in=I)
 * or the data-gradient operator (transpose=1: n_out=I, k_in=O); channels are zero-padded to 16. */
int dam_conv_pack_weights_f32(const float* w_oihw, int O, int I, int KH, int KW, int transpose,
                              float* packed, void* stream);

/* The same packing for many tensors in one launch.  desc_dev: DEVICE array [n_tensors][8] of int64 =
 * {w_oihw pointer, packed pointer, O, I, KH, KW, transpose, packed float count}; max_total = largest count. */
int dam_conv_pack_weights_multi_f32(const int64_t* desc_dev, int n_tensors, int64_t max_total, void* stream);

/* y[b, oh*out_stride+out_off_h, ow*out_stride+out_off_w, :] = g( res [* (res_mask > 0)] +
 *     bias + sum_{a<nA, b<nB, k} Wp[wt_base + a*wt_sa + b*wt_sb][k][:] *
 *            f(x[b, oh*in_stride + off_h + a*step_h, ow*in_stride + off_w + b*step_w, k])
 * for oh < Ho, ow < Wo, with x = 0 outside [0,H)x[0,W) and f(v) = v, or v*in_scale[k]+in_shift[k]
 * (then ReLU if relu_in; without it the loaders clamp at -inf, so a NaN input reads as -inf) -- the producer's BatchNorm apply fused into the load -- and g(v) = v, or max(v, 0) if relu_out:
 * with an eval-mode BatchNorm folded into the weights (scale) and `bias` (shift), one launch is the reference's
 * relu(bn(conv(x)) [+ shortcut]) (models/model_resnet.py:23-28,97).
 *   x : NHWC [B][H][W][C] (C % 16 == 0, k_chunks == C/16), or with in_nchw=1 the reference's
 *       [B][C][H][W] planes with C <= 16 (first layer, k_chunks == 1)
 *   y : NHWC [B][OHt][OWt][n_out], n_out % 16 == 0;  res/res_mask (optional): same shape as y
 * Forward conv: in_stride=stride, off=-pad, step=dilation, taps (kh,kw) as is.  Stride-1 dgrad:
 * off=+pad, step=-dilation on dy with transposed packing.  Stride-2 dgrad: one call per output parity
 * class (out_stride=2).  in_stride must be 1 or 2.
 * bn_partial (optional, >= dam_bn_workspace_floats(n_out) floats): if the launch can also produce the BatchNorm
 * partial statistics of y (records (n, mean, M2) per workgroup and channel) it does so and stores the record count
 * in *bn_parts_host (a HOST int); 0 there means "not produced" and the caller runs dam_bn_stats_f32 instead.
 * Feed the records to dam_bn_finalize_f32 or dam_bn_finalize_apply_f32.
 * bn_bwd (optional, see dam_bn_bwd_sums below; needs bn_partial; with res only if res_mask_bits is set there): the launch is a data gradient whose
 * output dy feeds the backward pass of y = relu(bn(x)); if it can, it also writes that pass's two per-channel sums as records
 * [*bn_parts_host][n_out][2] into bn_partial (then hand them to dam_bn_backward_f32 as partials_given); 0 records = not produced.
 * bn_in (optional, ABI 36; see dam_bn_bwd_in below): x is the gradient dy that reaches relu(bn(c)); the launch applies that
 * BatchNorm's backward (dc = a * (dy * mask) + b * c + k, coefficients from dam_bn_backward_finalize_f32) in its row loaders,
 * convolves dc and stores it to bn_in->dc -- bitwise dam_bn_backward_f32(partials_given) followed by this call on its dx.  Only
 * for the layers the plan names (out16[13] != 0, see dam_conv2d_tapgrid_plan); DAM_ERR_UNSUPPORTED for every other.
 * workspace (optional): scratch for split-K over the input channels (used for small-spatial, wide layers; at most
 * 8 * B*OHt*OWt*n_out floats are used, fewer if less is given); partial slabs are summed in a fixed order.
 * Which kernel a call gets (1x1 direct, row-ring strip, loader-wave pipe, pipe on column ranges, tile) is decided by host
 * arithmetic on the scalar arguments and on which optional operands are given: dam_conv2d_tapgrid_plan below answers it without
 * launching, on a machine without a GPU too. */
int dam_conv2d_tapgrid_f32(const float* x, int B, int H, int W, int C, int in_nchw, const float* w_packed,
                           int k_chunks, int n_out, const float* bias, const float* in_scale,
                           const float* in_shift, int relu_in, int relu_out, float* y, int OHt, int OWt, int Ho, int Wo,
                           int out_stride, int out_off_h, int out_off_w, int in_stride, int nA, int nB,
                           int off_h, int step_h, int off_w, int step_w, int wt_base, int wt_sa, int wt_sb,
                           const float* res, const float* res_mask, float* bn_partial, int* bn_parts_host,
                           const struct dam_bn_bwd_sums* bn_bwd, const struct dam_bn_bwd_in* bn_in, float* workspace,
                           int64_t workspace_floats, void* batch, void* stream);

/* Two single-tap operators into the same output pixels in ONE launch:
 *   y[b, oh*out_stride+out_off_h, ow*out_stride+out_off_w, :] = W1p[tap1] . x1[b, oh, ow, :] + W2p[tap2] . x2[b, oh, ow, :]
 * x1, x2: NHWC [B][H][W][C]; W1p / W2p: packed images (dam_conv_pack_weights_f32) with k_in = C and n_out outputs, of which tap
 * tap1 / tap2 is used.  The data gradient of a down-sampling block's input (models/model_resnet.py:17-21,26: x feeds the 3x3 /
 * stride-2 conv1 AND the 1x1 / stride-2 shortcut convolution) receives, at its (even, even) pixels, exactly these two terms: the
 * centre tap of conv1's transposed operator applied to d conv1 and the shortcut's transposed operator applied to d shortcut. */
int dam_conv1x1_pair_f32(const float* x1, const float* w1_packed, int tap1, const float* x2, const float* w2_packed, int tap2,
                         int B, int H, int W, int C, int n_out, float* y, int OHt, int OWt, int out_stride, int out_off_h,
                         int out_off_w, void* stream);

/* The whole data gradient of a 3x3 / stride-2 / pad-1 convolution's input in ONE launch -- all four output parity classes from
 * one read of dy -- optionally with a second, 1x1 / stride-2 operator of the same input added at the (even, even) pixels (a
 * down-sampling block: conv1 and the shortcut convolution both read x, models/model_resnet.py:17-21,26):
 *   dx[b, u, v, :] = sum_{a,b} W[a][b]^T dy[b, (u+1-a)/2, (v+1-b)/2, :]  (integer quotients only)  [+ Wp^T dy_pair[b, u/2, v/2, :]]
 * dy, dy_pair: NHWC [B][Hd][Wd][Co] with Hd = (H+1)/2, Wd = (W+1)/2; w_packed_t / w_pair_packed_t: dam_conv_pack_weights_f32
 * images with transpose = 1 (nine taps / one tap); dx: NHWC [B][H][W][Ci].  Every byte of dx is written.
 * Co = 32 -> Ci = 16 and Co = 64 -> Ci = 32 keep the packed weights in LDS for the life of a persistent workgroup; other layers
 * with Co % 32 == 0 and Ci % 16 == 0 stream the weight fragments from L2 (one (pixel block, channel block) unit per wave).
 * DAM_ERR_UNSUPPORTED for anything else; the caller then runs the parity classes through dam_conv2d_tapgrid_f32.
 * bn_bwd / bn_partial / bn_parts_host (optional, all three or none; see dam_bn_bwd_sums below, `mask_bits` form only): dx is the
 * gradient reaching relu(bn(u) + shortcut), the output of the block in front (models/model_resnet.py:26-27); the two thin layers'
 * kernels then also write that BatchNorm's two backward sums as records [*bn_parts_host][Ci][2] into bn_partial (hand them to
 * dam_bn_backward_f32 as partials_given); *bn_parts_host == 0: not produced, run the separate pass. */
int dam_dgrad_s2_3x3_f32(const float* dy, const float* w_packed_t, const float* dy_pair, const float* w_pair_packed_t, int B,
                         int Hd, int Wd, int Co, int Ci, float* dx, int H, int W, const struct dam_bn_bwd_sums* bn_bwd,
                         float* bn_partial, int* bn_parts_host, void* stream);

/* Forward of the same block: conv1 (3x3 / stride 2 / pad 1, no bias) and the shortcut convolution (1x1 / stride 2) of one input
 * in ONE launch, with the BatchNorm statistics records of both outputs (models/model_resnet.py:17-21,24-26: both feed a
 * training-mode BatchNorm).  x: NHWC [B][H][W][Ci]; w_packed / wsc_packed: dam_conv_pack_weights_f32 images with transpose = 0;
 * y, ysc: NHWC [B][(H+1)/2][(W+1)/2][Co].  partial / partial_sc (both or neither; >= dam_bn_workspace_floats(Co) floats each):
 * records [*parts_host][Co][3] = (n, mean, M2), one per workgroup, for dam_bn_finalize_pair_f32 / dam_bn_finalize_f32 /
 * dam_bn_finalize_apply_f32.  Ci = 16 -> Co = 32 and Ci = 32 -> Co = 64 keep both weight images resident in LDS (one record per
 * workgroup); other layers with Ci % 32 == 0 and Co % 16 == 0 stream the weight fragments from L2 (one (16 pixels, 16 channels) unit
 * per wave, one record per 64 pixels); DAM_ERR_UNSUPPORTED otherwise: the caller runs dam_conv2d_tapgrid_f32 twice and
 * dam_bn_stats_pair_f32. */
int dam_conv_s2_pair_fwd_f32(const float* x, const float* w_packed, const float* wsc_packed, int B, int H, int W, int Ci, int Co,
                             float* y, float* ysc, float* partial, float* partial_sc, int* parts_host, void* stream);

/* Which kernel the last call of the CALLING THREAD to one of the three entry points above (dam_conv1x1_pair_f32,
 * dam_dgrad_s2_3x3_f32, dam_conv_s2_pair_fwd_f32) launched (ABI 31): each picks between kernels and template instantiations by
 * channel counts, pixel count, the device's CU count and an occupancy answer -- a plan made by host arithmetic before the launch,
 * which the three plan entries below give out without launching (ABI 37).  The record is that plan's note, copied: a test that means
 * to exercise one instantiation, or the unit loop of a persistent kernel, asks here (as dam_wgrad_last_launch for the weight
 * gradient) and may compare with the plan of the same call.  A host
 * variable: reset to "none" at the entry of every call of the three, written after the launch was made -- no device work, no kernel
 * argument, nothing synchronised; the choice of kernel is unchanged.  out16_host (host memory, 16 ints) receives
 *   [0] entry: 0 none (no call yet, or the call was refused or failed), 1 dam_conv_s2_pair_fwd_f32, 2 dam_dgrad_s2_3x3_f32,
 *       3 dam_conv1x1_pair_f32
 *   [1] family: 1 persistent kernel with the weight images resident in LDS, 2 streaming kernel with a chunk's weight fragments
 *       staged in LDS per workgroup (one 16-pixel block per wave), 3 streaming kernel with the fragments straight from L2 (two
 *       pixel blocks per wave; data gradient only), 4 the 1x1 pair kernel
 *   [2] NB                         16-channel blocks of the OUTPUT (forward: Co / 16, data gradient: Ci / 16; 1x1 pair: blocks per
 *                                  workgroup, 1 or 2)
 *   [3] NCH                        16-channel chunks of the INPUT (forward: Ci / 16, data gradient: Co / 16, 1x1 pair: C / 16)
 *   [4] MB                         16-pixel blocks per wave unit (1x1 pair: 0)
 *   [5] WAVES                      waves per workgroup; 1x1 pair: R, the chunk slots per operand and round
 *   [6] pair                       data gradient: dy_pair given; forward: 1; 1x1 pair: BOTH (all chunks of both operands in one round)
 *   [7] sums                       forward: statistics records written; data gradient: the BatchNorm-backward sums written
 *   [8] workgroups                 of the grid (streaming kernels: including the surplus ones that leave at once)
 *   [9] units                      wave units of the launch (16 * MB pixels; streaming kernels: x one channel block; 1x1 pair: (image,
 *                                  row, 16-pixel segment))
 *   [10] rounds                    the largest number of units one wave takes: the persistent kernels' loop count, from the same
 *                                  arithmetic as the kernel's (per_xcd, ustride); 1 for the others
 *   [11] n_xcd                     persistent kernels: 8 when the grid is a multiple of 8 (every XCD takes a contiguous eighth of the
 *                                  units), else 1; streaming kernels with LDS staging: 8 (group g on XCD g % 8); else 1
 *   [12] records                   the count stored in *parts_host / *bn_parts_host
 *   [13..15] 0 */
int dam_s2_last_launch(int* out16_host);

/* The same answer BEFORE a call (ABI 37): one plan entry per entry point above, with its scalar arguments and its operand flags
 * (stats: partial / partial_sc given; pair: dy_pair given; sums: bn_bwd / bn_partial / bn_parts_host given).  out16_host receives
 * the 16 ints dam_s2_last_launch would hold after that call; the status is the one the call would return for these arguments
 * (DAM_OK, DAM_ERR_BAD_ARG, DAM_ERR_UNSUPPORTED: the caller's fall-back), and after anything but DAM_OK out16_host is all zero, the
 * "none" record.  cus, resident_per_cu: the only two facts the decision takes from the device -- its CU count, and how many
 * workgroups of the persistent kernel the channel counts name one CU holds (the runtime's occupancy answer).  Both > 0: host
 * arithmetic only, on a machine without a GPU too.  0 for either: taken from the calling thread's current device exactly as the
 * launching entry takes it, so the record of a call equals the plan of the same call.  dam_conv1x1_pair_f32 asks the device
 * nothing. */
int dam_conv_s2_pair_fwd_plan(int B, int H, int W, int Ci, int Co, int stats, int cus, int resident_per_cu, int* out16_host);
int dam_dgrad_s2_3x3_plan(int B, int Hd, int Wd, int Co, int Ci, int H, int W, int pair, int sums, int cus, int resident_per_cu,
                          int* out16_host);
int dam_conv1x1_pair_plan(int B, int H, int W, int C, int n_out, int OHt, int OWt, int out_stride, int out_off_h, int out_off_w,
                          int* out16_host);

/* Sibling launches in one.  The parity classes of a strided data gradient are up to four small launches over the same
 * tensors, weights and tile that differ only in their tap grid.  With a batch (caller-owned HOST memory of
 * dam_conv_batch_bytes() bytes, dam_conv_batch_init() once) dam_conv2d_tapgrid_f32 records a launch that would take the tile
 * kernel instead of making it (launches that take another kernel run at once, as without a batch);
 * dam_conv_batch_flush packs consecutive records that differ only in geometry into ONE launch (class in blockIdx.z).
 * Every tensor of a recorded call must stay valid until the flush; batch = NULL launches at once. */
int64_t dam_conv_batch_bytes(void);
int dam_conv_batch_init(void* batch);
int dam_conv_batch_flush(void* batch, void* stream);

/* The plan of a dam_conv2d_tapgrid_f32 call without the call (ABI 29): the same scalar arguments, `operands` = which optional
 * operands the call would be given (DAM_CONV_HAS_* below; the BWD bits describe *bn_bwd and count only with DAM_CONV_HAS_BN_BWD,
 * i.e. bn_bwd->x set) and workspace_floats.  Writes the 16 ints of dam_conv_last_launch that the call would leave into out16_host
 * and the record count it would store in *bn_parts_host into bn_parts_host (both HOST memory, both required), and returns what
 * the call would return wherever that does not depend on the device or on a pointer's value: DAM_OK, DAM_ERR_BAD_ARG,
 * DAM_ERR_UNSUPPORTED, and DAM_ERR_LAUNCH for a layer whose column ranges fit only in part.  Host arithmetic only: no device
 * work, no GPU needed.  The diagnostic switches DAM_NO_PIPE, DAM_TILE and DAM_PIPE_KS are read as by the call (DAM_PIPE_WGS
 * only sizes a grid and is not part of the plan). */
#define DAM_CONV_HAS_BIAS 0x001u
#define DAM_CONV_HAS_IN_SCALE 0x002u
#define DAM_CONV_HAS_IN_SHIFT 0x004u
#define DAM_CONV_HAS_RES 0x008u
#define DAM_CONV_HAS_RES_MASK 0x010u
#define DAM_CONV_HAS_BN_PARTIAL 0x020u
#define DAM_CONV_HAS_BN_BWD 0x040u
#define DAM_CONV_HAS_BWD_MASK_BITS 0x080u
#define DAM_CONV_HAS_BWD_RES_MASK_BITS 0x100u
#define DAM_CONV_HAS_BWD_MASK_SCALE 0x200u     /* mask_scale and mask_shift */
#define DAM_CONV_HAS_WORKSPACE 0x400u
#define DAM_CONV_HAS_BATCH 0x800u
#define DAM_CONV_HAS_BN_IN 0x1000u             /* bn_in (ABI 36) */
#define DAM_CONV_HAS_BN_IN_BITS 0x2000u        /* ... with its mask as sign bytes (else mask_scale / mask_shift) */
int dam_conv2d_tapgrid_plan(int B, int H, int W, int C, int in_nchw, int k_chunks, int n_out, int relu_in, int relu_out,
                            int OHt, int OWt, int Ho, int Wo, int out_stride, int out_off_h, int out_off_w, int in_stride,
                            int nA, int nB, int off_h, int step_h, int off_w, int step_w, int wt_base, int wt_sa, int wt_sb,
                            unsigned operands, int64_t workspace_floats, int* out16_host, int* bn_parts_host);

/* Which kernel the last dam_conv2d_tapgrid_f32 call of the CALLING THREAD launched (ABI 26): the entry point falls back from
 * kernel to kernel without telling, so a test that means to exercise one family asks here.  A host variable, the plan's record
 * copied after a successful launch -- no device work, nothing synchronised.  out16_host (host memory, 16 ints) receives
 *   [0] family: 0 none (no call yet; after a call that FAILED the record is unspecified), 1 row-ring strip kernel, 2 loader-wave (pipe) kernel,
 *       3 the pipe kernel on column ranges, 4 tile kernel, 5 tile kernel recorded into a batch (launched by the flush), 6 direct 1x1
 *   [1] MB  [2] NB                 M / N tile in 64-pixel / 16-channel blocks (1x1: NB only)
 *   [3] NCH                        strip: resident K chunks; 1x1: chunk slots (NCHMAX)
 *   [4] T33 [5] LW [6] EPI [7] SO  strip: compile-time 3x3 / stride-1 grid, wide-row loader, statistics epilogue, self-overlapped
 *                                  form and its write-out variant (0: ping-pong form)
 *   [8] PU  [9] STATS [10] KS      pipe: items per loader thread, statistics mode, K split over the wave pairs
 *   [11] ksplit                    tile: split-K factor (> 1: splitk_reduce_kernel wrote the result)
 *   [12] ranges                    column ranges launched (family 3; the tile fields are those of the last range), else 1
 *   [13] BNF                       strip: the BatchNorm-backward apply of bn_in ran in the row loaders, 2 = mask from (scale, shift),
 *                                  3 = from sign bytes; 0 = not fused (a call WITH bn_in then returns DAM_ERR_UNSUPPORTED)
 *   [14..15] 0 */
int dam_conv_last_launch(int* out16_host);

/* Weight gradient of the same convolutions (autograd of nn.Conv2d reached from loss.backward(),
 * model_trainer.py:36):  dw[n][k][kh][kw] = sum_{b,oh,ow} dy[b,oh,ow,n] * f(x[b, oh*stride+kh*dil-pad, ow*stride+kw*dil-pad, k])
 *   x  : as for dam_conv2d_tapgrid_f32 (NHWC, or in_nchw planes for the first layer), same fused f() -- for NHWC input
 *        only: in_nchw together with in_scale is DAM_ERR_UNSUPPORTED (the loader of the NCHW planes applies no affine, and
 *        the first layer reads raw features)
 *   dy : NHWC [B][Ho][Wo][n_chan], n_chan % 16 == 0; only the first n_out channels are real
 *   dw : torch layout [n_out][c_real][kh][kw], fully overwritten; c_real <= C is the number of REAL input channels
 *        (0 = C): the zero-padded planes of the re-laid stem input (dam_nchw_to_nhwc16_f32) drop out, so the result can
 *        be written straight into the parameter's slice of a flat gradient buffer
 *   workspace : at least dam_conv2d_wgrad_workspace_floats(...) floats; holds the split-K slabs that a
 *               second kernel sums in a fixed order (bitwise reproducible, no float atomics)
 * Supported kernels: 3x3, 1x1, and kw in {5,7,9} with any kh; stride 1 or 2. */
int64_t dam_conv2d_wgrad_workspace_floats(int n_out, int c_in, int kh, int kw);
int dam_conv2d_wgrad_f32(const float* x, int B, int H, int W, int C, int in_nchw, const float* in_scale,
                         const float* in_shift, int relu_in, const float* dy, int Ho, int Wo, int n_chan,
                         int n_out, int kh, int kw, int stride, int pad, int dil, float* dw, int c_real,
                         float* workspace, int64_t workspace_floats, void* reduce_queue, void* stream);

/* Deferred slab reductions.  Nothing in loss.backward() (model_trainer.py:36) reads a weight gradient before
 * optimizer.step() (model_trainer.py:37), and the reduction that turns a convolution's slabs into dw is a few
 * microseconds of mostly launch latency -- twenty of them in a ResNet18 step.  With a queue,
 * dam_conv2d_wgrad_f32 launches only the slab kernel and records the reduction; dam_wgrad_queue_flush runs every
 * recorded reduction in ONE launch (descriptors travel as kernel arguments: nothing to upload, hipGraph-capturable).
 *   queue : caller-owned HOST memory of dam_wgrad_queue_bytes() bytes, dam_wgrad_queue_init() once;
 *           reduce_queue = NULL in dam_conv2d_wgrad_f32 reduces at once (dw valid when the call's work is done)
 *   Until the flush, every queued call's `workspace` (its slabs) and `dw` must stay allocated and untouched, so
 *   queued calls need distinct workspaces; dw is written by the flush.  A full queue flushes itself on `stream`. */
int64_t dam_wgrad_queue_bytes(void);
int dam_wgrad_queue_init(void* queue);
int dam_wgrad_queue_pending(const void* queue);     /* recorded, not yet flushed; -1: not an initialised queue */
int dam_wgrad_queue_flush(void* queue, void* stream);
/* Batched slab launches (ABI 14).  The deep ResNet stages (models/model_resnet.py:70-71: 128 / 256 channels on 65x9 / 33x5 pixels)
 * have three weight gradients of ONE geometry each, 20-28 us launches of which ~13 us are launch + pipeline fill, and each split
 * eight ways over the pixels to fill 256 CUs (eight 2.4 MB slabs for a 2.4 MB gradient).  With batching on, a queued
 * dam_conv2d_wgrad_f32 that takes the tile kernel only RECORDS its launch; recorded launches of the same instantiation and geometry
 * (at most 4) run as ONE launch (blockIdx.z = job) when another geometry arrives or at dam_wgrad_queue_flush -- with a third of
 * the pixel splits, i.e. a third of the slab bytes the reduction reads back.  Calls that take the DIRECT kernel (the 1x1 / stride-2
 * shortcut convolutions, models/model_resnet.py:18-21: 11-16 us launches of a latency-bound kernel) are recorded too and run, up
 * to 8 of one instantiation with whatever geometries, as one flat launch whose jobs share the chip (each a fraction of the pixel
 * splits it would take alone).  Off by default.
 *   Contract while on: x, dy, in_scale / in_shift of a queued call must stay valid and unmodified until the flush as well
 *   (not only its workspace and dw).  Switching needs an empty queue (DAM_ERR_BAD_ARG otherwise).
 * on = 2 (ABI 35): as 1, and a call that takes the stride-1 ROW kernel is recorded too where its instantiation is in the batching
 * table (dam_wgrad_plan.h: ROWS_BATCHED).  The 3x3 convolutions of a ResNet stage have one geometry (stem + layer1: five, the other
 * stages three each); recorded, up to 8 of one instantiation, geometry and grid run as ONE launch whose workgroups keep their tile and
 * strip and walk the jobs in order, the loader waves asking for the next job's first rows while the current job's last slots are
 * multiplied: a job boundary costs a slab write-out instead of a launch, a wave start and a cold ring.  The slabs are bitwise those of
 * launches of their own.  Recorded row launches run when another instantiation or geometry arrives, when the table is full, or at
 * the flush.  The mode says what becomes of the NEXT call, so 1 <-> 2 may be switched with launches recorded (a caller that batches
 * only some of its calls); to or from 0 still needs an empty queue.  Any other value: DAM_ERR_BAD_ARG. */
int dam_wgrad_queue_set_batching(void* queue, int on);

/* Which kernel the last dam_conv2d_wgrad_f32 call of the CALLING THREAD committed to (ABI 27): the entry point picks between four
 * kernel families with 29 instantiations by row width and channel counts and falls through to the tile kernel without
 * telling, so a test that means to exercise one instantiation asks here (as dam_conv_last_launch for the forward kernels).  A host
 * variable: reset to "none" at the entry of every call, written from the call's plan where the launcher has passed its last refusal --
 * no device work, no kernel argument, nothing synchronised.  out16_host (host memory, 16 ints) receives
 *   [0] family: 0 none (no call yet, or the call failed before committing), 1 row-streaming kernel (3x3 / stride 1), 2 row-streaming
 *       kernel on column-parity planes (3x3 / stride 2), 3 direct kernel, 4 tile kernel
 *   [1] TNB [2] TKB                output / input channel blocks of the workgroup's tile (family 2: TKB = 1)
 *   [3] STEPS [4] KP               row kernels: MFMA steps per wave and row part, planes per loader wave
 *   [5] GPP (family 2: GPPX) [6] GPPD   row kernels: 1 KB pieces per X row plane; family 2 also per dY row plane
 *   [7] HV [8] NL                  row kernels: row parts per compute wave's row (1 or 2), loader waves
 *   [9] TA [10] TB                 tile kernel: kernel rows / columns per tap group; direct kernel: KH / KW
 *   [11] nx [12] nsplit            grid: channel (x tap group) tiles, pixel splits = slabs.  With [15] == 2 the split is decided when
 *                                  the recorded launch runs: 0 for the tile kernel, the direct kernel's upper bound
 *   [13] [14]                      row kernels: strips per image, output rows per strip; tile kernel: pixels per tile (TMW), 0
 *   [15] how it was issued: 0 launched and reduced now, 1 launched, the reduction queued, 2 the launch itself recorded in the
 *        batching queue (it runs with others of its kind at dam_wgrad_queue_flush or when the queue makes room; a recorded
 *        tile launch has its LDS, workspace and LDS-limit refusals still ahead of it: they are returned by the call that runs it)
 * Fields foreign to the family are 0. */
int dam_wgrad_last_launch(int* out16_host);
/* The same answer BEFORE a call and without a GPU (ABI 32): the dispatch of dam_conv2d_wgrad_f32 is host arithmetic on its scalar
 * arguments, on which optional operands are given (has_affine: in_scale, has_shift: in_shift) and on what the queue does with the
 * launch (queue_mode: 0 no queue, 1 a queue without batching, 2 a batching queue, 4 a batching queue in mode 2: row launches
 * recorded too; 3 is no mode: DAM_ERR_BAD_ARG).  out16_host receives the 16 ints
 * dam_wgrad_last_launch would report after that call; returns the status the launching call would return for everything that
 * needs no pointer and no device (DAM_ERR_BAD_ARG, DAM_ERR_UNSUPPORTED, DAM_ERR_WORKSPACE), with the 16 ints zero then. */
int dam_conv2d_wgrad_plan(int B, int H, int W, int C, int in_nchw, int relu_in, int Ho, int Wo, int n_chan, int n_out, int kh, int kw,
                          int stride, int pad, int dil, int c_real, int has_affine, int has_shift, int queue_mode,
                          int64_t workspace_floats, int* out16_host);

/* Diagnostic builds of the library only (libdam_hip_diag.so: dam_conv_strip.hip compiled with -DDAM_STRIP_DIAG_TAGS): the row-ring
 * convolution's loader waves tag every geometry-table entry with the tile it describes and its compute waves check the tag of every
 * entry they consume (the slip-bound argument in dam_conv_strip.hip, checked on the device).  out2_host receives {checks made,
 * mismatches seen} since the last reset; synchronises the device.  The shipped library returns DAM_ERR_UNSUPPORTED. */
int dam_strip_diag_counters(uint32_t* out2_host, int reset);

/* ---------------------------------------------------------------------------------
 * BatchNorm2d on NHWC float32 [n_pixels][C], C % 16 == 0.  Replaces nn.BatchNorm2d + F.relu (+ the
 * residual add) of models/model_resnet.py:12-27,65,97 and models/model_scalar_1s.py:174-186,
 * models/model_scalar_2s.py:32-44, forward and backward.
 * --------------------------------------------------------------------------------- */
int64_t dam_bn_workspace_floats(int C);

typedef struct dam_bn_fin {       /* host struct of device pointers: what dam_bn_finalize_f32 takes, for the pair and finalize-apply entry points */
    const float* gamma; const float* beta;
    float* running_mean; float* running_var; int64_t* num_batches_tracked;    /* may be NULL */
    float momentum, eps;
    float* save_mean; float* save_invstd; float* scale; float* shift;
} dam_bn_fin;

/* BatchNorm-backward sums from a data-gradient epilogue (dam_conv2d_tapgrid_f32's bn_bwd): the backward pass of
 * y = relu(bn(x)) (models/model_resnet.py:24 of the reference, reached from loss.backward()) needs sum(dz) and sum(dz * xhat)
 * per channel, dz = dy * (x*mask_scale + mask_shift > 0), xhat = (x - mean) * invstd.  dy is the convolution data gradient
 * that was just computed, so the launch that produces it takes the sums from its output registers and one read of x.
 * Host struct of device pointers (x: the BatchNorm's input, shape of the launch's output; the rest: per channel). */
typedef struct dam_bn_bwd_sums {
    const float* x; const float* mean; const float* invstd; const float* mask_scale; const float* mask_shift;
    /* A data gradient that also carries an identity shortcut (res / res_mask given: dy = conv^T(..) + res * (res_mask > 0), the
     * gradient reaching the block INPUT) can take the sums of the BatchNorm that produced that input -- the ResNet stem's
     * relu(bn1(conv1(x))), models/model_resnet.py:97 -- if the shortcut's mask is also available as the sign bytes
     * dam_bn_apply_f32 wrote (one byte per channel quad); res_mask stays the fallback of launches that cannot. */
    const uint8_t* res_mask_bits;
    /* mask_bits (instead of mask_scale / mask_shift): the BatchNorm's ReLU mask as sign bytes -- the upstream layer is
     * relu(bn(x) + shortcut), a residual block's bn2 (models/model_resnet.py:26-27), whose mask is that of the block output.
     * Only together with res / res_mask_bits. */
    const uint8_t* mask_bits;
} dam_bn_bwd_sums;

/* BatchNorm-backward apply in a data gradient's row loaders (dam_conv2d_tapgrid_f32's bn_in, ABI 36): the call's x is dy, the
 * gradient reaching y = relu(bn(c)) [+ shortcut]; mask as in dam_bn_backward_f32: (c*mask_scale + mask_shift > 0) or the sign
 * bytes of dam_bn_apply_f32 (exactly one form).  coef: [3][C] from dam_bn_backward_finalize_f32.  dc (shape of c) receives what
 * dam_bn_backward_f32 would have written to dx.  Host struct of device pointers. */
typedef struct dam_bn_bwd_in {
    const float* c; const float* coef; const float* mask_scale; const float* mask_shift; const uint8_t* mask_bits; float* dc;
} dam_bn_bwd_in;

/* Training-mode statistics of x: save_mean, save_invstd = 1/sqrt(biased var + eps), the fused affine
 * scale = gamma*invstd, shift = beta - mean*scale, and torch's running-stat update
 * (running = (1-momentum)*running + momentum*stat, unbiased variance; ++*num_batches_tracked).
 * running_mean/running_var/num_batches_tracked may be NULL. */
int dam_bn_stats_f32(const float* x, int64_t n_pixels, int C, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, int64_t* num_batches_tracked,
                     float momentum, float eps, float* save_mean, float* save_invstd, float* scale,
                     float* shift, float* workspace, void* stream);

/* dam_bn_stats_f32 for TWO tensors of one shape in one partial + one finalize launch (a residual block's conv1 output and its
 * shortcut convolution's output, models/model_resnet.py:17-21,24-26: two independent BatchNorms that become ready together).
 * a, b: the parameters / outputs of each (struct dam_bn_fin above); workspace:
 * 2 * dam_bn_workspace_floats(C) floats. */
int dam_bn_stats_pair_f32(const float* x_a, const float* x_b, int64_t n_pixels, int C, const struct dam_bn_fin* a,
                          const struct dam_bn_fin* b, float* workspace, void* stream);

/* Second half of dam_bn_stats_f32 on its own: merges `parts` partial records [parts][C][3] = (n, mean, M2) (as written
 * by dam_conv2d_tapgrid_f32's bn_partial output) and produces the same outputs / running-stat update. */
int dam_bn_finalize_f32(const float* partial, int parts, int C, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, int64_t* num_batches_tracked,
                        float momentum, float eps, float* save_mean, float* save_invstd, float* scale,
                        float* shift, void* stream);

/* dam_bn_finalize_f32 for the two BatchNorms of a pair in one launch (records of equal count and channel number, e.g. from
 * dam_conv_s2_pair_fwd_f32).  a, b: struct dam_bn_fin. */
int dam_bn_finalize_pair_f32(const float* partial_a, const float* partial_b, int parts, int C, const struct dam_bn_fin* a,
                             const struct dam_bn_fin* b, void* stream);

/* First half of dam_bn_stats_f32 on its own: the partial records [*parts_host][C][3] (a HOST int receives the count), sized
 * for dam_bn_finalize_apply_f32 (or dam_bn_finalize_f32).  workspace: dam_bn_workspace_floats(C) floats. */
int dam_bn_stats_partial_f32(const float* x, int64_t n_pixels, int C, float* workspace, int* parts_host, void* stream);

/* dam_bn_finalize_f32 + dam_bn_apply_f32 in ONE launch (relu(bn2(conv2(..)) + shortcut), models/model_resnet.py:26-27; the stem's
 * and ConvBlock2d's relu(bn(conv(x))), models/model_resnet.py:97, models/model_scalar_1s.py:184-186): every workgroup merges the
 * records of the 16 or 32 channels it applies in its prologue -- no finalize launch (4.6-5 us each, whatever it does).
 * fin: the BatchNorm's parameters and outputs as dam_bn_finalize_f32 takes them (all four outputs and the running statistics
 * are written); the remaining arguments as dam_bn_apply_f32.  Tables beyond 24 KB per workgroup take the separate finalize and
 * apply launches instead. */
int dam_bn_finalize_apply_f32(const float* partial, int parts, int C, const struct dam_bn_fin* fin, const float* x,
                              int64_t n_pixels, const float* res, const float* res_scale, const float* res_shift, int relu,
                              float* y, uint8_t* sign_bits, void* stream);

/* Eval-mode equivalent: the same four outputs from the running statistics. */
int dam_bn_eval_affine_f32(int C, const float* gamma, const float* beta, const float* running_mean,
                           const float* running_var, float eps, float* save_mean, float* save_invstd,
                           float* scale, float* shift, void* stream);

/* y = relu?( x*scale + shift  [+ res]  or  [+ res*res_scale + res_shift] ).
 * sign_bits (optional, n_pixels * C/4 bytes): one byte per channel quad, bit i = (y[4q + i] > 0) -- the ReLU mask the
 * backward passes need from the block output, in 1/16 of its bytes (mask_bits of dam_bn_backward*_f32). */
int dam_bn_apply_f32(const float* x, int64_t n_pixels, int C, const float* scale, const float* shift,
                     const float* res, const float* res_scale, const float* res_shift, int relu, float* y,
                     uint8_t* sign_bits, void* stream);

/* Backward of y = [relu](bn(x) [+ ...]): dz = dy * mask, where mask is (y_mask > 0) if y_mask (the saved output) is given,
 * the sign bytes dam_bn_apply_f32 wrote if mask_bits is given, (x*mask_scale + mask_shift > 0) if the forward's fused affine
 * is given instead (plain relu(bn(x)): the saved output is then not read at all), 1 if all are NULL (at most one form);
 * dgamma = sum dz*xhat, dbeta = sum dz, dx = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat))
 * (training) or gamma*invstd*dz (training == 0, running statistics).
 * partials_given > 0: `workspace` already holds that many records [partials_given][C][2] of (sum dz, sum dz*xhat) -- written by
 * a data-gradient launch with bn_bwd -- and the pass over dy and x that would produce them is skipped. */
int dam_bn_backward_f32(const float* dy, const float* y_mask, const float* x, int64_t n_pixels, int C,
                        const float* gamma, const float* save_mean, const float* save_invstd, int training,
                        const float* mask_scale, const float* mask_shift, const uint8_t* mask_bits, float* dx,
                        float* dgamma, float* dbeta, float* workspace, int partials_given, void* stream);

/* The finalize of dam_bn_backward_f32(partials_given = parts) on its own (ABI 36): merges the records [parts][C][2] with the
 * arithmetic that call uses, writes dgamma / dbeta (bitwise that call's) and coef = [3][C]: dx = coef[0] * dz + coef[1] * x + coef[2]
 * per channel -- for a consumer that applies it itself (dam_conv2d_tapgrid_f32's bn_in).  One small launch. */
int dam_bn_backward_finalize_f32(const float* partial, int parts, int64_t n_pixels, int C, const float* gamma,
                                 const float* save_mean, const float* save_invstd, int training, float* dgamma, float* dbeta,
                                 float* coef, void* stream);

/* The same for TWO BatchNorms that share dy and the mask (exactly one of y_mask / mask_bits) -- a residual block's bn2 and the BatchNorm of its shortcut
 * convolution, both fed by the gradient of relu(bn2(..) + bn_sc(..)) (models/model_resnet.py:23-28): dy and the mask are
 * read once per pass instead of twice, three launches instead of six; bitwise the results of two dam_bn_backward_f32 calls.
 * workspace: dam_bn_pair_workspace_floats(C) floats. */
int64_t dam_bn_pair_workspace_floats(int C);
int dam_bn_backward_pair_f32(const float* dy, const float* y_mask, const uint8_t* mask_bits, int64_t n_pixels, int C,
                             int training,
                             const float* x_a, const float* gamma_a, const float* mean_a, const float* invstd_a,
                             float* dx_a, float* dgamma_a, float* dbeta_a,
                             const float* x_b, const float* gamma_b, const float* mean_b, const float* invstd_b,
                             float* dx_b, float* dgamma_b, float* dbeta_b, float* workspace, void* stream);

/* out[c] = sum_p x[p][c] for c < n_real (gradient of a convolution bias, models/model_scalar_1s.py:167). */
int dam_channel_sum_f32(const float* x, int64_t n_pixels, int C, int n_real, float* out, float* workspace,
                        void* stream);

/* Inverted dropout of ConvBlock2d (models/model_scalar_1s.py:177,187-188; applied only in training mode).  The mask is a
 * counter-based function of (seed, call offset, element index): dam_dropout_tick snapshots and advances the DEVICE
 * call counter by n (graph replays draw fresh masks), dam_dropout_apply_f32 computes y = keep ? x/(1-p) : 0 for the
 * snapshot -- called again on the gradient with the same snapshot in backward.  n % 4 == 0. */
int dam_dropout_tick(int64_t* counter, int64_t n, int64_t* snapshot, void* stream);
int dam_dropout_apply_f32(const float* x, int64_t n, float p, uint64_t seed, const int64_t* snapshot, float* y,
                          void* stream);

/* ---------------------------------------------------------------------------------
 * Gain heads, gain-weighted sum and MSE.  Replace models/model_resnet.py:75-85,108-126 (same code in
 * models/model_scalar_1s.py:222-273, models/model_scalar_2s.py:79-132) and nn.MSELoss at
 * model_trainer.py:21,35.  trunk: NHWC [B][P][C]; conv_w [S][C], conv_b [S], fc_w [S][P], fc_b [S];
 * h [B][S][P] (post-ReLU head activations, kept for backward); gains [B][S]; x [B][S][FT]; masked/gt [B][FT].
 * --------------------------------------------------------------------------------- */
int dam_heads_fwd_f32(const float* trunk, int B, int P, int C, int S, const float* conv_w, const float* conv_b,
                      const float* fc_w, const float* fc_b, float* h, float* gains, void* stream);
int64_t dam_heads_bwd_workspace_floats(int B, int P, int C, int S);
int dam_heads_bwd_f32(const float* dgains, const float* h, const float* trunk, int B, int P, int C, int S,
                      const float* conv_w, const float* fc_w, float* dtrunk, float* dconv_w, float* dconv_b,
                      float* dfc_w, float* dfc_b, float* workspace, void* stream);
int dam_masksum_fwd_f32(const float* x, const float* gains, int B, int S, int64_t FT, float* masked, void* stream);
int64_t dam_masksum_workspace_floats(int B, int S);
int dam_masksum_bwd_f32(const float* dmasked, const float* x, int B, int S, int64_t FT, float* dgains,
                        float* workspace, void* stream);
/* Fused: masked (optional output), loss = mean((masked-gt)^2), dgains = d loss / d gains, one pass over x. */
int dam_masksum_mse_f32(const float* x, const float* gains, const float* gt, int B, int S, int64_t FT,
                        float* masked, float* loss, float* dgains, float* workspace, void* stream);

/* ---------------------------------------------------------------------------------
 * Optimizer.  Replaces optimizer.step() at model_trainer.py:37 for torch.optim.Adam(params,
 * weight_decay=wd) (training.ipynb cell 11; L2 folded into the gradient, not AdamW) over one flat
 * parameter buffer.  step: device int64 counter (incremented here); derived2: device float[2] scratch.
 * grads are multiplied by grad_scale first (1/world_size after a sum all-reduce).
 * hyper_dev (optional): DEVICE float[8] = {lr, beta1, beta2, eps, weight_decay, grad_scale, 1-beta1, 1-beta2} read at
 * run time instead of the scalar arguments, so that a captured graph follows param_groups edits / LR schedulers
 * (1-beta formed in double by the caller, as torch does).
 * All four buffers must be 16-byte aligned.
 * --------------------------------------------------------------------------------- */
int dam_adam_l2_step_f32(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                         int64_t* step, float* derived2, float lr, float beta1, float beta2, float eps,
                         float weight_decay, float grad_scale, const float* hyper_dev, void* stream);

/* Replica digest (ABI 16).  The reference trains on one device; the data-parallel ModelTrainer (model_trainer.py) checks
 * after every training epoch that its replicas still hold bit-identical parameters by comparing this digest over ranks.
 *   *out (+)= sum over i in [0, n) of mix64(x[i] + (index_base + i) * 0x9E3779B97F4A7C15)   (modulo 2^64)
 * x: n 32-bit words (any 4-byte type, read as bit patterns: NaN payloads and -0.0 count as distinct); mix64 = splitmix64's
 * finaliser.  The sum is order-independent: the result does not depend on the launch geometry, and a buffer digested in
 * pieces (accumulate = 1, each piece with its index_base) equals the one-launch digest.  accumulate = 0 zeroes *out first.
 * max_blocks: 0 = the library's choice, else an upper bound on the grid (tests vary it).  out: device uint64, 8-byte
 * aligned, written with a global atomic. */
int dam_digest64_u32(const uint32_t* x, int64_t n, int64_t index_base, int max_blocks, int accumulate, uint64_t* out,
                     void* stream);

/* ---------------------------------------------------------------------------------
 * Full-song inference tail (BASELINE config C5), all on the device so that the whole of
 * inference_utils.py:105-145 + the callers' sum / normalise is one hipGraph-capturable sequence.
 * --------------------------------------------------------------------------------- */

/* inference_utils.py:125-130 and :136-141.  raw_db [n_chunks][n_stems] float32 = the model's gain outputs per chunk;
 *   amp[s][c]    = 10 ** (0.5 * raw_db[c][s])                       (data/dataset_utils.py:46-50, float64)
 *   smooth[s][:] = scipy.signal.savgol_filter(amp[s], window, polyorder)   (default mode 'interp': the first / last
 *                  window/2 outputs come from the polynomial fitted to the first / last window)
 * amp, smooth: [n_stems][n_chunks] float64; smooth_f32 (optional): the same values rounded to float32.
 * Argument rules are scipy's (odd window, polyorder < window <= n_chunks -> otherwise DAM_ERR_BAD_ARG);
 * polyorder <= 5 and n_chunks <= 8192 are supported. */
int dam_gains_smooth(const float* raw_db, int n_chunks, int n_stems, int window, int polyorder, double* amp,
                     double* smooth, float* smooth_f32, void* stream);

/* inference_utils.py:12-41 (interpolate_mask) fused with :143 (loaded_tracks[track] * mask):
 *   out[r][n] = audio[r][n] * gains[r / rows_per_gain][min(n / (n_samples / n_gains), n_gains-1)]
 * audio [rows][n_samples] float32 or float64 (audio_is_f64); gains [ceil(rows/rows_per_gain)][n_gains] float64 (one gain
 * sequence per stem = per `rows_per_gain` channel rows); out float32 or float64 (out_is_f64; the reference's numpy
 * product of a float32 track with the float64 mask is float64). */
int dam_gain_ramp_apply(const void* audio, int audio_is_f64, const double* gains, int64_t rows, int64_t rows_per_gain,
                        int64_t n_samples, int n_gains, void* out, int out_is_f64, void* stream);

/* The caller's next step (inference.ipynb cells 9/11, evaluation.py:59-66) fused with the gain ramp:
 *   mix[r][n] = sum_s audio[s][r][n] * gains[s][min(n / (n_samples / n_gains), n_gains-1)]
 * and, if normalize, each row divided by its max-abs (librosa.util.normalize(track_sum, axis=1)).
 * audio [n_stems][rows][n_samples] float32/float64, gains [n_stems][n_gains] float64, mix [rows][n_samples]
 * float32/float64 (mix_is_f64).  workspace: dam_mixdown_workspace_elems(rows) elements of mix's dtype. */
int64_t dam_mixdown_workspace_elems(int64_t rows);
int dam_mixdown_peak_normalize(const void* audio, int audio_is_f64, const double* gains, int n_stems, int64_t rows,
                               int64_t n_samples, int n_gains, int normalize, void* mix, int mix_is_f64,
                               void* workspace, void* stream);

/* ---------------------------------------------------------------------------------
 * ITU-R BS.1770 loudness.  Replaces what the reference gets from the third-party pyloudnorm
 * package (`pyln.Meter(sr).integrated_loudness`): data/dataset.py:115-130, evaluation.py:39-46,59-66,
 * models/baselines/mean_loudness_model.py:10-20.
 *   dam_loudness_kweight_coeffs (host): the two normalised biquads of pyloudnorm's "K-weighting" at `rate`,
 *     coef12 = {b0,b1,b2,1,a1,a2} for the high shelf then the high pass.
 *   dam_loudness_block_energy (device): y = lfilter(high pass, lfilter(high shelf, x)) per channel in float64 and
 *     z[ch][j] = sum_{n in [blk_lo[j], min(blk_hi[j], n_samples))} y[n]^2 / block_len  (the caller supplies the block
 *     bounds exactly as the reference's int() truncations produce them; blk_lo/blk_hi/z are device pointers).
 *     x: float32 or float64 (x_is_f64), sample n of channel ch at x[ch*channel_stride + n*sample_stride].
 *     workspace: dam_loudness_workspace_bytes(n_samples, channels) bytes.
 * For these one-track calls the gating of the block energies (absolute -70 LUFS, relative -10 LU) is host logic
 * (loudness.gated_loudness); the batched calls below have it on the device.
 *
 * Batched, sync-free form (evaluation.py:77-116 measures 4 stems for each of 9 variants of a song).  Every call below
 * is stateless, does not allocate, does not synchronise with the host and is hipGraph-capturable.
 *   dam_loudness_block_energy_batch: the block energies of n_tracks tracks of n_samples x channels in one set of
 *     launches.  Sample n of channel ch of track t is x[t*track_stride + n*sample_stride + ch*channel_stride] (element
 *     strides: [N][channels][n] planar storage and its transposes are read in place).  coef12_host, blk_lo, blk_hi
 *     (device, each nondecreasing) and block_len as above, shared by all tracks.  gains (device, may be NULL):
 *     [n_tracks][n_gains] float64; sample n of every channel of track t is filtered as
 *       (double)x * gains[t][min(n / (n_samples / n_gains), n_gains-1)]
 *     -- the index and the float64 product of dam_gain_ramp_apply with out_is_f64, so the scaled stems are never
 *     written (n_gains = 1: a constant gain per track).  z [n_tracks][channels][n_blocks] float64.  y^2 is not stored per
 *     sample: the second filter pass sums it between consecutive block bounds, a block is the fixed-order sum of its
 *     pieces; no atomics, and a track's result does not depend on the other tracks of the call (bitwise).
 *     workspace: dam_loudness_batch_workspace_bytes(n_tracks, n_samples, channels, n_blocks) bytes, 8-byte aligned.
 *     n_tracks * channels <= 65535.
 *   dam_loudness_gate: lufs[t] (device float64) from z [n_tracks][channels <= 5][n_blocks], exactly
 *     loudness.gated_loudness: channel weights 1, 1, 1, 1.41, 1.41; stage 1 keeps l_j >= -70; stage 2 keeps
 *     l_j > Gamma_r and l_j > -70 with Gamma_r = loudness of the stage-1 means - 10; an empty stage-2 set gives -inf.
 *     Fixed-order float64 reductions, any n_blocks >= 1.
 *   dam_loudness_target_gains: gains[i] = 10^((target[i] - lufs[i]) / 20) (pyloudnorm normalize.loudness), all device
 *     float64.  A silent track (lufs = -inf) gets the IEEE result +inf, as np.power gives; it is not special-cased.
 *     The scaled audio itself is dam_gain_ramp_apply with n_gains = 1.
 * --------------------------------------------------------------------------------- */
int dam_loudness_kweight_coeffs(double rate, double* coef12);
int64_t dam_loudness_workspace_bytes(int64_t n_samples, int channels);
int dam_loudness_block_energy(const void* x, int x_is_f64, int64_t n_samples, int channels, int64_t sample_stride,
                              int64_t channel_stride, const double* coef12_host, const int64_t* blk_lo,
                              const int64_t* blk_hi, int n_blocks, double block_len, double* z, void* workspace,
                              void* stream);
int64_t dam_loudness_batch_workspace_bytes(int n_tracks, int64_t n_samples, int channels, int n_blocks);
int dam_loudness_block_energy_batch(const void* x, int x_is_f64, int n_tracks, int64_t n_samples, int channels,
                                    int64_t track_stride, int64_t sample_stride, int64_t channel_stride,
                                    const double* gains, int n_gains, const double* coef12_host, const int64_t* blk_lo,
                                    const int64_t* blk_hi, int n_blocks, double block_len, double* z, void* workspace,
                                    void* stream);
int dam_loudness_gate(const double* z, int n_tracks, int channels, int n_blocks, double* lufs, void* stream);
int dam_loudness_target_gains(const double* lufs, const double* target, int n, double* gains, void* stream);

/* ---------------------------------------------------------------------------------
 * PCM encoder: the payload of the WAV file every caller of the reference ends with (inference.ipynb `sf.write`,
 * evaluation.py:58-66, data/listening_test_data_preparation.py), quantised on the device.
 *   x: planar [channels][n_samples] float32 or float64 (x_is_f64), contiguous -- the layout of the master and of each
 *      mixed stem; channels 1 .. DAM_PCM_MAX_CHANNELS.
 *   scale (device float64, n_scale = 0: none, 1, or channels): v = (double)x * scale[..], one float64 rounding.
 *   out: interleaved [n_samples][channels], little endian, DAM_WAV_S24 = 3 packed bytes; 4-byte aligned.
 *   Integer formats, B = 16 / 24 / 32: a NaN v is written as 0 and counted; w = v * 2^(B-1) (exact); with `dither`
 *   w = w + d, d = u1 - u2 with u1, u2 the high and low 32 bits of r over 2^32, r = the 64-bit splitmix64 finaliser of
 *   seed * 0xD1342543DE82EF95 + (n * channels + c) (TPDF, +-1 LSB, a pure function of seed and element); q = rint(w)
 *   (ties to even) clamped to [-2^(B-1), 2^(B-1) - 1].  DAM_WAV_F32 writes (float)v: no dither, nothing counted.
 *   clip_count (device int64 [channels], may be NULL): OVERWRITTEN with the number of clamped (or NaN) elements per channel.
 * The launch is capped at DAM_PCM_MAX_BLOCKS workgroups of 256 lanes x 16 input bytes per channel row; larger buffers are
 * walked tile by tile.  Parity with libsndfile's converters is not claimed.
 * --------------------------------------------------------------------------------- */
typedef enum dam_wav_format { DAM_WAV_S16 = 0, DAM_WAV_S24 = 1, DAM_WAV_S32 = 2, DAM_WAV_F32 = 3 } dam_wav_format;
#define DAM_PCM_MAX_CHANNELS 8
#define DAM_PCM_MAX_BLOCKS 2048
/* The launch geometry, for callers and tests that need the grid-stride boundary: frames of one tile (256 lanes x 16 input
 * bytes per channel row) and the workgroup cap; one pass of the full grid covers their product. */
int64_t dam_pcm_tile_frames(int x_is_f64);
int dam_pcm_max_blocks(void);
int dam_pcm_encode(const void* x, int x_is_f64, int channels, int64_t n_samples, const double* scale, int n_scale,
                   int format, int dither, uint64_t seed, void* out, int64_t* clip_count, void* stream);

/* ---------------------------------------------------------------------------------
 * True peak (ITU-R BS.1770 Annex 2 / EBU R128: the peak of the 4x oversampled signal) and the gain ceiling built on it --
 * what keeps a master "at -20 LUFS" from being clipped by dam_pcm_encode, which can only count.  Also the missing piece of
 * the pyloudnorm surface (`pyln.normalize.peak`), measured on the reconstructed waveform instead of the samples.
 *   Interpolator (dam_true_peak_taps_host, host float64, closed form): 49-tap Hann-windowed sinc
 *     h[k] = sinc((k - 24) / 4) * 0.5 * (1 - cos(2 pi k / 48)), k = 0..48; h[24] = 1, h[24 +- 4m] = 0 exactly, symmetric.
 *   For a row x[0..n) (x = 0 outside), p = 1, 2, 3 and i in [0, n):
 *     y_p[i] = sum_{j=-6..5} x[i - j] * h[24 + p + 4 j]          (x[i-5 .. i+6]: the value between x[i] and x[i+1])
 *     TP = max(max_i |x[i]|, max_{p,i} |y_p[i]|), linear; >= the sample peak by construction.
 *   tests/_truepeak_ref.py restates this in numpy.  Parity with libebur128 or the ITU conformance table is not claimed.
 *   dam_true_peak_batch: every (track, channel) row of the batch in one set of launches; addressing (element strides) and
 *     `gains` exactly as dam_loudness_block_energy_batch: sample n of channel ch of track t is
 *     x[t*track_stride + n*sample_stride + ch*channel_stride], measured as (double)x * gains[t][min(n / (n_samples /
 *     n_gains), n_gains-1)] when gains (device [n_tracks][n_gains] float64) is not NULL.  sample_peak (may be NULL) and
 *     true_peak: device float64 [n_tracks][channels].  workspace: dam_true_peak_workspace_bytes(...) bytes, 8-byte
 *     aligned.  n_tracks * channels <= 65535.  Stateless, allocates nothing, does not synchronise, no atomics,
 *     hipGraph-capturable; each y_p is 12 products summed in the fixed order j = -6 .. 5 and the result is a maximum, so
 *     a row's two outputs do not depend on the other rows of the call or on the launch geometry (bitwise).  Argument
 *     errors (NULL x / true_peak / workspace; a non-positive count; gains with n_gains < 1 or > n_samples; too many rows,
 *     in this order) return DAM_ERR_BAD_ARG.  Non-finite samples are outside the contract: a NaN sample and the
 *     interpolated values it reaches are skipped by the maximum, an infinite sample gives an infinite peak.
 *   dam_true_peak_tile_samples / dam_true_peak_max_blocks: the launch geometry -- samples of one workgroup tile and the
 *     workgroup cap of a launch (a row gets max(1, cap / rows) workgroups, each striding over the row's tiles) -- for
 *     tests that place tile boundaries and the grid-stride wrap.
 *   dam_peak_limit_gains: gains[i] = min(gains[i], ceiling_lin / max_{q < peaks_per_gain} peaks[i*peaks_per_gain + q]),
 *     all device float64, ceiling_lin > 0 linear (10^(dBTP/20)).  A zero peak leaves the gain as it is (ceiling / 0 =
 *     +inf); one static gain, no look-ahead limiter.
 * --------------------------------------------------------------------------------- */
int dam_true_peak_taps_host(double* h49);
int64_t dam_true_peak_tile_samples(void);
int dam_true_peak_max_blocks(void);
int64_t dam_true_peak_workspace_bytes(int n_tracks, int64_t n_samples, int channels);
int dam_true_peak_batch(const void* x, int x_is_f64, int n_tracks, int64_t n_samples, int channels, int64_t track_stride,
                        int64_t sample_stride, int64_t channel_stride, const double* gains, int n_gains,
                        double* sample_peak, double* true_peak, void* workspace, void* stream);
int dam_peak_limit_gains(double* gains, const double* peaks, int n_gains, int peaks_per_gain, double ceiling_lin,
                         void* stream);

/* ---------------------------------------------------------------------------------
 * Look-ahead true-peak limiter: a time-varying gain that holds the reconstructed waveform of a row set (the channels of one
 * master, limited together) under a ceiling, where dam_peak_limit_gains can only turn the whole signal down.  Everything is
 * float64 and closed form: no recurrence, no state, every output sample a function of a bounded input window.
 *   Per row set: rows x[c][i] (c < channels, i in [0, n)), the scalar s = pre_gain[set] (1 if pre_gain is NULL), the linear
 *   ceiling `ceil` = 10^(dBTP/20) > 0, the look-ahead L >= 1 and the hold H >= 1 in samples.
 *     1. xs[c][i] = (double)x[c][i] * s                                              (one rounding)
 *     2. demand   d[i] = max_c max(|xs[c][i]|, |y_1[c][i]|, |y_2[c][i]|, |y_3[c][i]|), y_p exactly the interpolated phase of
 *        dam_true_peak_batch: the same 49 taps, xs = 0 outside the row, 12 products added in the order j = -6 .. 5.
 *     3. required gain  r[i] = min(1, ceil / d[i]); r[i] = 1 where d[i] = 0 and for i outside [0, n).
 *     4. hold and look-ahead  m[j] = min_{k in [j-H, j+L]} r[k]                      (a minimum: exact and order-free)
 *     5. attack / release ramp  g[i] = (sum_{j=i-L..i} m[j]) / (double)(L+1), each g[i] its own sum of L+1 terms added in
 *        the order j = i-L .. i -- never a running sum or a prefix difference (as dam_loudness_window_power).  Every
 *        window [j-H, j+L] with j in [i-L, i] contains [i-H, i], so g[i] <= r[k] for k in [i-H, i]: the samples on both
 *        sides of every inter-sample value carry a gain no larger than that value asks for (hence H >= 1).
 *     6. out[c][i] = xs[c][i] * g[i], converted to the output type.
 *     7. min_gain = min_i g[i];  n_limited = #{i : g[i] < 1}.
 *   Latency is zero in file time (the look-ahead reads samples that are already resident).  Where d <= ceil over
 *   [i-H-L, i+2L], g[i] = (L+1) * 1.0 / (L+1) = 1.0 exactly and out == xs bit for bit.  The true peak of `out` can exceed the
 *   ceiling by a few 1e-5 dB (interpolating a product is not the product of the interpolations): callers that need the
 *   ceiling exactly measure `out` and trim (inference_utils.MasterChain).  tests/_limiter_ref.py restates this in numpy.
 *   dam_limiter_apply: n_sets row sets in one set of launches.  Sample i of channel c of set b is
 *     x[b*set_stride + i*sample_stride + c*channel_stride] (element strides, float32 or float64 by x_is_f64), as
 *     dam_true_peak_batch addresses a track.  pre_gain: device float64 [n_sets] or NULL.  out: planar, contiguous
 *     [n_sets][channels][n_samples], float32 or float64 (out_is_f64); it must not overlap x.  min_gain (device float64
 *     [n_sets]) and n_limited (device int64 [n_sets]) may each be NULL.  workspace: dam_limiter_workspace_bytes(n_sets,
 *     n_samples) bytes, 8-byte aligned (r per sample and two partials per tile).  Stateless, allocates nothing, does not
 *     synchronise, no atomics, hipGraph-capturable; out, min_gain and n_limited of a row set depend on neither the launch
 *     geometry nor the other row sets (bitwise).  Argument errors (NULL x / out / workspace; a non-positive count; more than
 *     65535 row sets; a ceiling that is not > 0; lookahead outside 1 .. dam_limiter_max_lookahead(); hold outside
 *     1 .. dam_limiter_max_hold(), in this order) return DAM_ERR_BAD_ARG.  Non-finite samples or gains are outside the
 *     contract.
 *   dam_limiter_tile_samples: the samples one workgroup owns, for tests that place tile boundaries.
 *   dam_limiter_max_lookahead / dam_limiter_max_hold: the caps (512 / 4096 samples: 10 ms / 85 ms at 48 kHz), set by the
 *     LDS image of a tile and its halo.
 * --------------------------------------------------------------------------------- */
int64_t dam_limiter_tile_samples(void);
int dam_limiter_max_lookahead(void);
int dam_limiter_max_hold(void);
int64_t dam_limiter_workspace_bytes(int n_sets, int64_t n_samples);
int dam_limiter_apply(const void* x, int x_is_f64, int n_sets, int64_t n_samples, int channels, int64_t set_stride,
                      int64_t sample_stride, int64_t channel_stride, const double* pre_gain, double ceiling_lin, int lookahead,
                      int hold, void* out, int out_is_f64, double* min_gain, int64_t* n_limited, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------
 * Feed-forward compressor with attack and release: the dynamics stage of a mixer, per stem or on the bus before the
 * limiter.  It is the recurrence the limiter above leaves out.  Everything is float64.
 *   Per row set (the 1 .. C channels of one track, compressed with ONE gain: stereo link): rows x[c][i], i in [0, n), the
 *   scalar s = pre_gain[set] (1 if pre_gain is NULL), threshold T dB, ratio R >= 1 (+inf allowed), knee width W >= 0 dB,
 *   slope = 1 - 1/R, knee_start = 10^((T - W/2)/20), aA = exp(-1 / (attack_ms * 1e-3 * rate)), aR likewise from release_ms,
 *   M = 10^(makeup_db/20).  knee_start, aA, aR and M are computed ONCE by the caller (ops.compressor_constants) and cross
 *   this interface as doubles, so that a reference uses bit-identical constants.
 *     1. xs[c][i] = (double)x[c][i] * s                                              (one rounding)
 *     2. detector  d[i] = max_c |xs[c][i]|
 *     3. static curve, the gain reduction c[i] >= 0 in dB:
 *          d[i] <= knee_start:  c[i] = 0, exactly, no logarithm taken;
 *          else o = 20 log10(d[i]) - T and
 *            W > 0 and o < W/2:  c = slope * (t * t) / (2 W),  t = max(o + W/2, 0);
 *            otherwise:          c = slope * max(o, 0).
 *     4. ballistics, the decoupled smooth peak detector of Giannoulis, Massberg and Reiss (JAES 2012) on the reduction:
 *          p[i] = max(c[i], aR * p[i-1])                      p[-1] = 0     (release: peak hold with exponential decay)
 *          q[i] = fma(aA, q[i-1], (1 - aA) * p[i])            q[-1] = 0     (attack: one pole on p; 1 - aA rounded once)
 *     5. g[i] = exp(-(q[i] * K)) * M,  K = 0.11512925464970228 (ln 10 / 20);   out[c][i] = xs[c][i] * g[i], rounded once to
 *        the output type.
 *     6. max_reduction = max_i q[i] (dB, >= 0);  n_over = #{i : d[i] > knee_start} (an exact integer).
 *     7. reduction[i] = q[i], only where a pointer is given: the gain-reduction curve, for plotting and metering.
 *   Parallel form.  Both recurrences are scans over closed families of maps: y -> max(c, a y) composes as
 *   (c2, a2) o (c1, a1) = (max(c2, a2 c1), a2 a1) with identity (0, 1) (c, y >= 0); y -> A y + B composes as
 *   (B2, A2) o (B1, A1) = (fma(A2, B1, B2), A2 A1).  A row is cut into chunks of K = dam_compressor_chunk_samples() samples:
 *   every chunk is walked from a zero state, the chunk maps (end state, a^K with a^K formed by K - 1 multiplications) are
 *   composed per tile of dam_compressor_tile_samples() samples (a shuffle scan over 64 chunks, the four 64-chunk totals
 *   left to right) and the tile totals left to right along the row (256 at a time, the same scan, with a carried state),
 *   and the chunks are walked again from their true entry states -- first p, then q on the true p.  The order of every
 *   combination is a function of the position in the row only; K is therefore part of the definition of the rounding, and
 *   the result agrees with the sequential definition to a few roundings per effective step (tests/test_compressor_gpu.py
 *   derives the bound).  Bitwise properties: a row set does not depend on the other row sets of the call, on its strides or
 *   on the launch geometry; out[..][:m+1] and q[:m+1] depend on x[..][:m+1] only; where no sample so far exceeded knee_start,
 *   q == 0.0 and out == xs * M bit for bit; permuting the channels permutes out and leaves q alone.
 *   dam_compressor_apply: n_sets row sets in one set of launches, addressed and laid out as dam_limiter_apply's (x by
 *     element strides, float32 or float64; out planar [n_sets][channels][n_samples], float32 or float64, not overlapping
 *     x; pre_gain device float64 [n_sets] or NULL).  reduction (device float64 [n_sets][n_samples]), max_reduction (device
 *     float64 [n_sets]) and n_over (device int64 [n_sets]) may each be NULL.  workspace:
 *     dam_compressor_workspace_bytes(n_sets, n_samples) bytes, 8-byte aligned (c per sample, four doubles per chunk, eight
 *     per tile).  Stateless, allocates nothing, does not synchronise, no atomics, hipGraph-capturable.  Returns
 *     DAM_ERR_BAD_ARG without a launch for: NULL x / out / workspace; n_sets outside 1 .. 65535; n_samples < 1;
 *     channels < 1; R < 1 or NaN; W < 0 or not finite; a knee_start that is not positive or whose 20 log10 differs from
 *     T - W/2 by more than 1e-9 dB; an alpha outside (0, 1) or of a time constant above
 *     dam_compressor_max_time_samples() = 2^17 samples; a makeup that is not positive and finite.  Non-finite samples or
 *     gains are outside the contract.
 * --------------------------------------------------------------------------------- */
int64_t dam_compressor_chunk_samples(void);
int64_t dam_compressor_tile_samples(void);
int64_t dam_compressor_max_time_samples(void);
int64_t dam_compressor_workspace_bytes(int n_sets, int64_t n_samples);
int dam_compressor_apply(const void* x, int x_is_f64, int n_sets, int64_t n_samples, int channels, int64_t set_stride,
                         int64_t sample_stride, int64_t channel_stride, const double* pre_gain, double threshold_db, double ratio,
                         double knee_db, double knee_start, double alpha_attack, double alpha_release, double makeup_lin,
                         void* out, int out_is_f64, double* reduction, double* max_reduction, int64_t* n_over, void* workspace,
                         void* stream);

/* ---------------------------------------------------------------------------------
 * Loudness over time: momentary (400 ms) and short-term (3 s) loudness as EBU R128 names them, the loudness range of
 * EBU Tech 3342 and a per-window loudness-profile error.  All float64, all device pointers; every entry is stateless,
 * allocates nothing, does not synchronise with the host, uses no atomics and is hipGraph-capturable.
 *   Hop energies.  h = round(0.1 * rate) samples, H = n / h hops (a shorter tail is dropped),
 *     e[c][j] = (sum of y^2 over [j h, (j+1) h)) / h with y the K-weighted row, gain ramp included: this is
 *     dam_loudness_block_energy_batch with blk_lo[j] = j h, blk_hi[j] = (j+1) h, block_len = h.  No other filter exists.
 *   dam_loudness_window_power: e [n_tracks][channels <= 5][H], window of w hops (4: momentary, 30: short-term), one value
 *     per hop, W = H - w + 1 >= 1:
 *       s_c = sum_{k=0..w-1} e[c][i+k] (k ascending);  p_i = (sum_c G_c s_c, c ascending) / w, G = 1, 1, 1, 1.41, 1.41;
 *       l_i = -0.691 + 10 log10(p_i)   (silence: p = 0, l = -inf).
 *     Every value is its own fixed-order sum (no running sum, no prefix difference), so it depends on neither its
 *     neighbours nor the rest of the batch.  power [n_tracks][W]; lufs [n_tracks][W] or NULL.  n_tracks <= 65535.
 *   dam_loudness_curve_stats: the gated statistics of each track's power curve p[0..W), one workgroup per track.  Gates act
 *     on powers, so no decision hangs on a log10 rounding:
 *       absolute gate  keep p_i >= DAM_LOUDNESS_ABS_GATE_POWER (-70 LUFS);
 *       relative gate  m = mean of the absolutely gated p_i (thread t sums t, t + 256, ..., then a tree over the 256
 *                      partials, as dam_loudness_gate does); keep p_i >= 0.01 m as well (-20 LU, Tech 3342);
 *       percentiles    n values pass both gates, q[] is those in ascending order:
 *                      lo = q[((n-1)*10 + 50) / 100], hi = q[((n-1)*95 + 50) / 100]  (Tech 3342's round((n-1) P / 100) in
 *                      integers), selected among the exact input doubles by an MSB-first radix select over their
 *                      order-preserving 64-bit keys, read from global memory: any W, no sort, no workspace.
 *     out [n_tracks][6] = { LRA = l(hi) - l(lo), l(lo), l(hi), Gamma_r = -0.691 + 10 log10(m) - 20, n, max_i l_i over
 *     all W values (ungated) } with l(p) = -0.691 + 10 log10(p).  n = 0: LRA 0.0, both percentiles NaN; Gamma_r is NaN
 *     when the absolute gate is already empty; the maximum of an all-silent curve is -inf.  A track's six values do not
 *     depend on the other tracks of the call (bitwise).  Non-finite or negative powers are outside the contract.
 *   dam_loudness_profile_error: ref_lufs [S][W] (the reference mix's stems), cand_lufs [V][S][W] (V candidate mixes).
 *     Window i of variant v is ACTIVE when every ref_lufs[s][i] >= -70 and every cand_lufs[v][s][i] >= -70;
 *       err[v] = mean over active i and all s of |(C[s][i] - mean_s C[.][i]) - (R[s][i] - mean_s R[.][i])|
 *     (sums over s ascending; thread t takes windows t, t + 256, ..., then the tree), NaN when no window is active;
 *     active[v] = the number of active windows as a double.  One workgroup per variant.
 * Parity with libebur128 is not claimed: its short-term hop for LRA and its percentile interpolation differ.
 * --------------------------------------------------------------------------------- */
#define DAM_LOUDNESS_ABS_GATE_POWER 0x1.f791ec6e1d5b7p-24 /* 10^((-70 + 0.691) / 10) */
int dam_loudness_window_power(const double* e, int n_tracks, int channels, int n_hops, int w, double* power, double* lufs,
                              void* stream);
int dam_loudness_curve_stats(const double* power, int n_tracks, int n_windows, double* out, void* stream);
int dam_loudness_profile_error(const double* ref_lufs, const double* cand_lufs, int n_variants, int n_stems,
                               int n_windows, double* err, double* active, void* stream);

/* ---------------------------------------------------------------------------------
 * Band spectrum (long-term average spectrum, LTAS, in fractional-octave bands) of gain-ramped stem sums, and the
 * spectral-balance error built on it -- the tonal counterpart of the loudness profile of evaluation.py:39-53.  Neither the
 * mix nor its STFT is written.  Every entry is stateless, allocates nothing, does not synchronise with the host, uses no
 * atomics and is hipGraph-capturable.  tests/_spectrum_ref.py restates the definition in numpy float64.
 *   Mix signal.  Mix r of n_mixes, stems s = 0 .. n_stems-1 of `channels` (1 or 2), sample p in [0, n_samples):
 *     element (r, s, p, c) is x[r*mix_stride + s*stem_stride + p*sample_stride + c*channel_stride] (element strides,
 *     float32 or float64 by x_is_f64; mix_stride = 0: every mix reads the same stems; n_stems = 1 with mix_stride the
 *     track stride: n_mixes independent tracks);
 *     m_s[p]  = ((double)a + (double)b) * 0.5 for the two channels a, b, or (double)a for one channel;
 *     xm_r[p] = (float)( sum_s m_s[p] * g[r][s][min(p / (n_samples / n_gains), n_gains-1)] ), the sum in double in ascending
 *     s, every product its own rounding (no fused multiply-add) -- the gain index and the float64 product of
 *     dam_gain_ramp_apply and dam_loudness_block_energy_batch.  gains: device float64 [n_mixes][n_stems][n_gains] or NULL;
 *     NULL means every gain is exactly 1.0 (the products are skipped: m * 1.0 == m).
 *   Frames are the front-end's (dam_stft_complex_f32, torch.stft(center=True, pad_mode='reflect')): T = 1 + n_samples / hop,
 *     frame_t[j] = xm[reflect(t*hop - n_fft/2 + j)] * w[j] in float32, j in [0, n_fft), w = `window` (device float32
 *     [n_fft], the periodic Hann table), twiddles as dam_stft_fill_twiddles_host fills them.  n_fft a power of two
 *     64 .. 16384, hop >= 1, n_samples > n_fft/2.
 *   Band power.  X_t = the float32 FFT of frame_t, bins k = 0 .. n_fft/2 (imaginary parts of bins 0 and n_fft/2 taken as 0),
 *     P[r][b] = ( sum_t sum_{k = edges[b]}^{edges[b+1]-1} c_k * ((double)re^2 + (double)im^2) ) / (double)T,
 *     c_k = 1 for k = 0 and k = n_fft/2, else 2: one band over all bins is (n_fft / T) * sum_t sum_j frame_t[j]^2 (Parseval).
 *     edges: device int32 [n_bands + 1], 0 <= edges[0] < ... < edges[n_bands] <= n_fft/2 + 1, 1 <= n_bands <=
 *     dam_spectrum_max_bands() (64).  The table lives on the device, so its CONTENT is the caller's to check
 *     (spectrum.py does, on the host copy it uploads); the kernel clamps every edge to [0, n_fft/2 + 1], so a bad table
 *     gives wrong numbers, never an access out of bounds.
 *     Order of the float64 additions: one workgroup owns F = dam_spectrum_frames_per_block() consecutive frames
 *     [i F, (i+1) F) of one mix; lane l of its 256 keeps one running sum per bin l, l + 256, ... over those frames in
 *     ascending t; bins are then folded into a band by 64 lanes (lane q adds bins edges[b] + q, + 64, ... ascending, then an
 *     xor-butterfly over the 64 partials, distances 1, 2, .. 32); a second kernel adds a mix's workgroup partials in
 *     ascending i and divides by T.  The order depends on (n_samples, n_fft, hop, edges) only: a row is bitwise
 *     reproducible and does not depend on the other rows of the call or on how many there are.
 *     power: device float64 [n_mixes][n_bands].  workspace: dam_spectrum_workspace_bytes(n_mixes, n_samples, hop, n_bands)
 *     bytes, 8-byte aligned.  n_mixes <= 65535.
 *     Argument errors (NULL x / window / twiddles / edges / power / workspace; a non-positive count; channels not 1 or 2;
 *     n_fft not a power of two in 64 .. 16384; hop < 1; n_samples <= n_fft/2; gains with n_gains < 1 or > n_samples;
 *     n_bands outside 1 .. dam_spectrum_max_bands(); more than 65535 mixes) return DAM_ERR_BAD_ARG before any launch.
 *   dam_spectrum_balance_error: ref_power [B], cand_power [V][B] (device float64), B <= dam_spectrum_max_bands().  For a
 *     spectrum P: tot = sum_b P[b] (ascending b), L[b] = 10 log10(P[b] / tot).  Band b of candidate v is KEPT iff
 *     ref[b] >= DAM_SPECTRUM_GATE * tot_ref and cand[v][b] >= DAM_SPECTRUM_GATE * tot_cand (a gate on powers, -70 dB under
 *     the total: no decision hangs on a log10);
 *       err[v] = (sum over kept b, ascending, of |L_cand[b] - L_ref[b]|) / n_kept,   NaN when n_kept = 0;
 *     n_kept[v] (device int32) = the number of kept bands.  Level-independent by construction: a common gain on all stems
 *     leaves every L[b] unchanged.  A spectrum that is zero everywhere passes the gate with 0 >= 0 and yields NaN.
 *     One 64-lane workgroup per candidate; err [V] float64.
 * Parity with any other analyser's band definitions (IEC 61260 filter skirts, A/K weighting) is not claimed: bands are
 * sums of FFT bins between edges computed in spectrum.band_edges.
 * --------------------------------------------------------------------------------- */
#define DAM_SPECTRUM_GATE 0x1.ad7f29abcaf48p-24 /* 1e-7 = 10^(-70 / 10) */
int dam_spectrum_frames_per_block(void);
int dam_spectrum_max_bands(void);
int64_t dam_spectrum_workspace_bytes(int n_mixes, int64_t n_samples, int hop, int n_bands);
int dam_spectrum_band_power(const void* x, int x_is_f64, int n_mixes, int n_stems, int channels, int64_t n_samples,
                            int64_t mix_stride, int64_t stem_stride, int64_t sample_stride, int64_t channel_stride,
                            const double* gains, int n_gains, const float* window, const float* twiddles, int n_fft, int hop,
                            const int32_t* edges, int n_bands, double* power, void* workspace, void* stream);
int dam_spectrum_balance_error(const double* ref_power, const double* cand_power, int n_variants, int n_bands, double* err,
                               int32_t* n_kept, void* stream);

/* ---------------------------------------------------------------------------------
 * Gain fit: the per-stem gains a reference mix used, by windowed least squares "stems x gains ~ reference mix", the share
 * of the reference such gains cannot explain, and the distance in dB of candidate gain curves from the fitted ones.  Every
 * entry is stateless, allocates nothing, does not synchronise with the host, uses no atomics and is hipGraph-capturable.
 * tests/_gainfit_ref.py restates the definitions in numpy float64.
 *   Signals.  Stems s = 0 .. S-1, 1 <= S <= DAM_GAINFIT_MAX_STEMS, of `channels` (1 or 2), samples p in [0, n_samples):
 *     element (s, p, c) is x[s*stem_stride + p*sample_stride + c*channel_stride] (element strides, float32 or float64 by
 *     x_is_f64).  The target y is one track of the same length and channel count: element (p, c) is
 *     y[p*y_sample_stride + c*y_channel_stride], float32 or float64 by y_is_f64, independently of x.
 *     Window of a sample: w(p) = min(p / (n_samples / W), W-1) in integer division -- the gain index of dam_gain_ramp_apply,
 *     so window w of the fit is gain w of the mixer.  1 <= W <= n_samples.  With seg = n_samples / W, window w starts at
 *     w*seg and holds seg samples, the last one n_samples - (W-1)*seg.
 *   dam_gainfit_moments: the symmetric moment matrix of the S+1 signals u = (x_0 .. x_{S-1}, y) of every window,
 *       M[w][i][j] = sum over p in window w, c of (double)u_i * (double)u_j,
 *     device float64 [W][S+1][S+1], both triangles written from one computation of each pair (exactly symmetric).
 *     Every addend enters its sum through one fused multiply-add, acc = fma(u_i, u_j, acc): for float32 inputs the
 *     product is exact in float64 either way, so only the additions round.
 *     Order of the additions, for a window of L samples (q = p - window start, 0 <= q < L): workgroup t of the window owns
 *     the T = dam_gainfit_tile_samples() samples q in [t T, min((t+1) T, L)); lane l of its 256 adds the samples
 *     q = t T + l, + 256, ... in ascending q, channel 0 before channel 1, to a running sum that starts at +0.0 (a lane
 *     without a sample keeps +0.0); the 64 lanes of a wave are folded by an xor-butterfly, distances 1, 2, .. 32
 *     (v = v + v[lane ^ m]); the four waves are added as ((w0 + w1) + w2) + w3; a second kernel adds the window's
 *     ceil(L / T) tile sums in ascending t, starting from the first.  The order depends on (L, channels, S) only -- not on
 *     W, on the window's index or on the alignment of its first sample: the same samples passed as a call of their own
 *     with W = 1 give the same bits.
 *     workspace: dam_gainfit_workspace_bytes(W, n_samples, S) bytes, 8-byte aligned (one record of (S+1)(S+2)/2 doubles
 *     per tile).  More than 2^31 - 1 tiles in all: DAM_ERR_UNSUPPORTED.
 *   dam_gainfit_solve: moments [W][S+1][S+1] -> gains [S][W] (the mixer's layout), residual [W] (device float64),
 *     status [W] (device int32).  pool = h >= 0, ridge >= 0.  For window w:
 *       A = sum of M[v], v = max(0, w-h) .. min(W-1, w+h) ascending (starting from the first); G = A[:S,:S], b = A[:S,S],
 *       Y = A[S][S].  Stem s is ACTIVE iff G_ss > 0 and G_ss >= DAM_GAINFIT_GATE * Y.
 *       Y == 0 or no active stem: every gain NaN, residual NaN, status 0.
 *       Otherwise, on the active stems in ascending order: d_s = sqrt(G_ss), R_ij = G_ij / (d_i * d_j) + ridge * [i == j];
 *       Cholesky R = L L^T in float64, column by column (pivot_j = R_jj less L_jk^2, k < j, one by one in ascending k); a pivot that is
 *       not > DAM_GAINFIT_PIVOT makes the window rank-deficient: every gain NaN, residual NaN, status -1.
 *       Else R h = (b_s / d_s) by forward and back substitution; active stems get g_s = h_s / d_s, inactive stems NaN;
 *       status = the number of active stems; with g of inactive stems taken as 0,
 *       residual = max(0, (Y - 2 (b . g) + g . (G g)) / Y), every dot product in ascending index from +0.0.
 *     One 64-lane workgroup per window; the elimination itself runs on one lane.
 *   dam_gainfit_gain_error: fit [S][W], cand [V][S][n_cand] (device float64), n_cand = W or 1 (a constant per stem).
 *       d[v][s][w] = 20 log10(cand / fit); an entry is KEPT iff both values are finite and > 0 (a negative fitted gain is
 *       inverted polarity, not a level).  A window with at least two kept stems contributes |d - mu| for each of them,
 *       mu = (sum of its kept d, ascending s) / their number; a window with fewer contributes nothing: a common gain on
 *       all stems of a window is a master fader, not a balance decision.
 *       err[v] = (sum of all contributions, windows ascending, stems ascending within a window) / their number,
 *       err_stem[v][s] = the same over stem s alone (windows ascending), n_kept[v] (device int32) = the number of
 *       contributions; NaN where that number is 0.  One 64-lane workgroup per variant.
 *   Argument errors (a NULL pointer; S outside 1 .. DAM_GAINFIT_MAX_STEMS; channels not 1 or 2; a non-positive count; W outside
 *     1 .. n_samples; negative pool or ridge, or a NaN ridge; n_cand not W or 1) return DAM_ERR_BAD_ARG before any launch.
 * --------------------------------------------------------------------------------- */
#define DAM_GAINFIT_MAX_STEMS 8
#define DAM_GAINFIT_GATE 0x1.5798ee2308c3ap-27 /* 1e-8: a stem 80 dB under the target's energy is not fitted */
#define DAM_GAINFIT_PIVOT 0x1p-40
int64_t dam_gainfit_tile_samples(void);
int64_t dam_gainfit_workspace_bytes(int n_windows, int64_t n_samples, int n_stems);
int dam_gainfit_moments(const void* x, int x_is_f64, int n_stems, int channels, int64_t n_samples, int64_t stem_stride,
                        int64_t sample_stride, int64_t channel_stride, const void* y, int y_is_f64, int64_t y_sample_stride,
                        int64_t y_channel_stride, int n_windows, double* moments, void* workspace, void* stream);
int dam_gainfit_solve(const double* moments, int n_windows, int n_stems, int pool, double ridge, double* gains,
                      double* residual, int32_t* status, void* stream);
int dam_gainfit_gain_error(const double* fit, const double* cand, int n_variants, int n_stems, int n_windows, int n_cand,
                           double* err, double* err_stem, int32_t* n_kept, void* stream);

/* ---------------------------------------------------------------------------------
 * Band gain fit (ABI 30): the gain fit above taken per frequency band -- the same least squares over the STFT bins of a band
 * and the frames of a window, which gives the per-stem, per-band gains a reference mix used (its EQ curve per stem), and the
 * share of the reference that per-band gains leave unexplained.  Every entry is stateless, allocates nothing, does not
 * synchronise with the host, uses no atomics and is hipGraph-capturable.  tests/_bandfit_ref.py restates the definitions in
 * numpy float64.
 *   Signals.  Stems s = 0 .. S-1, 1 <= S <= DAM_GAINFIT_MAX_STEMS, and one mix y, of `channels` (1 or 2) and n = n_samples
 *     samples, addressed exactly as dam_gainfit_moments addresses them (element strides, float32 or float64, the mix
 *     independently of the stems).  u = (x_0 .. x_{S-1}, y).
 *   Transforms.  Every channel of every signal is transformed on its own (no mono down-mix: the time-domain fit sums over the
 *     channels too).  U_i[c][t][k] = the front-end's float32 STFT of channel c of u_i, with the conventions of
 *     dam_stft_complex_f32 for a mono track without a gain: a float64 sample is rounded to float32 first, center = True with
 *     reflect padding, frame_t[j] = u[reflect(t*hop - n_fft/2 + j)] * w[j] in float32, w = `window` (device float32 [n_fft], the
 *     periodic Hann table), twiddles as dam_stft_fill_twiddles_host fills them, T = 1 + n / hop frames, n_fft a power of two
 *     64 .. 16384, hop >= 1, n > n_fft/2, bins k = 0 .. n_fft/2 with the imaginary parts of bins 0 and n_fft/2 taken as 0.
 *   Window of a frame.  w(t) = min(min(t*hop, n-1) / (n / W), W-1) in integer division: the gain index, in
 *     dam_gain_ramp_apply, of the frame's centre sample -- window w of this fit is gain w of the mixer, as in the time-domain
 *     fit.  1 <= W <= n, and every window must own at least one frame (DAM_ERR_BAD_ARG otherwise).  A frame reaches n_fft/2
 *     samples to either side of its centre, so frames straddle the window borders: a gain step in the reference is smeared
 *     over one frame, and the fitted gains of the two windows at a step are each pulled towards the other's.
 *   Bands.  edges as dam_spectrum_band_power takes it: device int32 [B + 1], 0 <= edges[0] < ... < edges[B] <= n_fft/2 + 1,
 *     1 <= B <= dam_spectrum_max_bands(); band b is the bins edges[b] .. edges[b+1]-1.  The CONTENT is the caller's to check
 *     (gainfit.py does, on the host copy it uploads); the kernel clamps every edge to [0, n_fft/2 + 1].
 *   dam_bandfit_moments:
 *       M[b][w][i][j] = sum over t with w(t) = w, k in band b, c of  c_k * ( (double)Re U_i (double)Re U_j + (double)Im U_i (double)Im U_j ),
 *     c_k = 1 for k = 0 and k = n_fft/2, else 2 (as in the band spectrum; the real part of conj(U_i) U_j: the gains are real).
 *     device float64 [B][W][S+1][S+1], both triangles written from one computation of each pair (exactly symmetric).  One band
 *     over all bins is the time-domain moment of the windowed frames times n_fft (Parseval), about n_fft * sum(w^2) / hop
 *     times dam_gainfit_moments' value.
 *     Every element (t, k, c) enters the sum of pair (i, j) through two fused multiply-adds, acc = fma(c_k Re U_i, Re U_j, acc),
 *     then acc = fma(c_k Im U_i, Im U_j, acc); the float32 values are converted to float64 first and c_k U_i is exact.
 *     Order of the additions, for the cell (b, w) of nb bins and nf frames: its E = nf * nb elements are numbered
 *     q = (t - first frame) * nb + (k - edges[b]); tile r owns q in [r D, min((r+1) D, E)), D = dam_bandfit_tile_elements();
 *     lane l of the tile's 256 adds q = r D + l, + 256, ... in ascending q, channel 0 before channel 1, to a running sum that
 *     starts at +0.0; the 64 lanes of a wave are folded by an xor-butterfly, distances 1, 2, .. 32; the four waves are added as
 *     ((w0 + w1) + w2) + w3; a second kernel adds the cell's ceil(E / D) tile sums in ascending r, starting from the first.  The
 *     order depends on (nf, nb, channels) only, and an entry (i, j) on signals i and j only: a cell does not depend on the
 *     other bands of the table, on the other windows, on the other stems or on how the call is cut into slabs (bitwise).
 *     Stages and workspace.  The spectra are written to the workspace ([signal][channel][frame][bin] float2) and read back once;
 *     those of a whole song do not fit (about 0.85 GB for four minutes of four stereo stems and a mix at 4096 / 2048), so the
 *     entry walks the windows in slabs: as many whole windows as hold at most slab_bytes of spectra (at least one window), four
 *     launches per slab (transform of the stems, of the mix, moments, reduce), no synchronisation between them.  slab_bytes = 0
 *     means DAM_BANDFIT_SLAB_BYTES (128 MiB: half the last-level cache, so that a slab's spectra can still be there
 *     when the moment kernel reads them).  workspace: dam_bandfit_workspace_bytes(the same arguments) bytes, 8-byte
 *     aligned: the slab's spectra and one record of (S+1)(S+2)/2 doubles per tile; 0 for arguments the entry refuses.
 *     A cell of more than 2^31 - 1 elements, or more than 2^30 - 1 frames: DAM_ERR_UNSUPPORTED.
 *   dam_bandfit_solve_grouped: moments [G][W][S+1][S+1] -> gains [G][S][W], residual [G][W], target [G][W] (device float64),
 *     status [G][W] (device int32): every group g (a band) is dam_gainfit_solve on moments[g], bit for bit -- one kernel serves
 *     both -- so windows are pooled over w-pool .. w+pool OF THE SAME GROUP only.  target[g][w] = Y, the mix's energy in the
 *     pooled matrix the residual was divided by (written for every cell, whatever its status).
 *   dam_bandfit_summary: residual, target, status [G][W] -> total [W] (device float64).  For window w, in ascending b from
 *     +0.0: a cell with Y = target[b][w] > 0 adds num = num + r * Y (a product, then a sum) and den = den + Y, where
 *     r = residual[b][w] if status[b][w] > 0 and 1 otherwise (status -1, or 0 with Y > 0: nothing is explained there); a cell
 *     with Y = 0 adds nothing.  total[w] = num / den, NaN if den = 0: the share of the mix's energy that per-band gains leave
 *     unexplained, the counterpart of dam_gainfit_solve's broadband residual[w]; the difference of the two in dB is what
 *     per-band gains explain beyond scalar gains.  One lane per window.
 *   Argument errors (a NULL pointer; S outside 1 .. DAM_GAINFIT_MAX_STEMS; channels not 1 or 2; n_fft not a power of two in
 *     64 .. 16384; hop < 1; n <= n_fft/2; W outside 1 .. n; a window without a frame; B outside 1 .. dam_spectrum_max_bands();
 *     a negative slab_bytes; a non-positive count; negative pool or ridge, or a NaN ridge) return DAM_ERR_BAD_ARG before any launch.
 * Not covered: complex (phase-shifting) band gains.  Rendering the fitted band gains to audio is the band-gain mixer below.
 * --------------------------------------------------------------------------------- */
#define DAM_BANDFIT_SLAB_BYTES 134217728
int64_t dam_bandfit_tile_elements(void);
int64_t dam_bandfit_workspace_bytes(int n_windows, int64_t n_samples, int n_stems, int channels, int n_fft, int hop,
                                         int n_bands, int64_t slab_bytes);
int dam_bandfit_moments(const void* x, int x_is_f64, int n_stems, int channels, int64_t n_samples, int64_t stem_stride,
                             int64_t sample_stride, int64_t channel_stride, const void* y, int y_is_f64, int64_t y_sample_stride,
                             int64_t y_channel_stride, const float* window, const float* twiddles, int n_fft, int hop,
                             const int32_t* edges, int n_bands, int n_windows, int64_t slab_bytes, double* moments,
                             void* workspace, void* stream);
int dam_bandfit_solve_grouped(const double* moments, int n_groups, int n_windows, int n_stems, int pool, double ridge,
                              double* gains, double* residual, double* target, int32_t* status, void* stream);
int dam_bandfit_summary(const double* residual, const double* target, const int32_t* status, int n_groups, int n_windows,
                             double* total, void* stream);

/* ---------------------------------------------------------------------------------
 * Band-gain mixer (ABI 33): the audio of per-stem, per-band, per-window gains -- what the band fit above fits, rendered: every
 * stem's STFT scaled bin by bin with the gain of the bin's band and of the frame's window, the stems summed, the sum inverted
 * and overlap-added.  One fused pass: no stem spectrum and no mix spectrum is written to memory.  Every entry is stateless,
 * allocates nothing, does not synchronise with the host, uses no atomics and is hipGraph-capturable.  tests/_bandmix_ref.py
 * restates the definition in numpy float64.
 *   Inputs.  Stems s = 0 .. S-1, 1 <= S <= DAM_GAINFIT_MAX_STEMS, of `channels` (1 or 2) and n = n_samples samples, addressed
 *     exactly as dam_bandfit_moments addresses them (element strides, float32 or float64).  gains: device float64 [B][S][W],
 *     the layout dam_bandfit_solve_grouped writes; fill: device float64 [S][W]; edges: device int32 [B + 1] as the band fit takes
 *     it, 1 <= B <= dam_spectrum_max_bands() (the CONTENT is the caller's to check -- gainfit.py does, on the host copy it
 *     uploads; the kernel clamps every edge to [0, n_fft/2 + 1]); window, twiddles: the front-end's tables; n_fft a power of two
 *     64 .. 16384; 1 <= hop <= n_fft/2 (dam_istft_f32's rule: a larger hop is DAM_ERR_UNSUPPORTED before the device is touched);
 *     n > n_fft/2; 1 <= W <= n and every window owns a frame, as in the band fit.
 *   Transforms and frames.  X_s[c][t][k] = the float32 STFT of channel c of stem s, exactly the band fit's U_s (a float64 sample
 *     rounded to float32 first, reflect padding, the periodic Hann table, the imaginary parts of bins 0 and n_fft/2 taken as 0,
 *     the same operations in the same order); T = 1 + n / hop frames; the window of frame t is the band fit's w(t).
 *   Effective gain of stem s at bin k of a frame of window w.  The band of k is the lowest b with edges[b] <= k < edges[b+1]
 *     (clamped edges).  In a band: e = gains[b][s][w] if that is finite, else fill[s][w] if that is finite, else 0.  Outside
 *     every band: fill[s][w] if finite, else 0.  e is rounded to float32.  The gain is piecewise constant over a band: the model
 *     the fit assumes.
 *   Mix spectrum.  Y[c][t][k] = sum_s e X_s[c][t][k] in float32, in ascending s from +0, every step one FUSED multiply-add per
 *     component: re = fmaf(e, Re X_s, re), im = fmaf(e, Im X_s, im).
 *   Output.  y_t = irfft(Y[c][t]) (n_fft samples; the imaginary parts of bins 0 and n_fft/2 ignored), as dam_istft_f32 inverts
 *     a frame: the real-FFT pre-twiddle, an n_fft/2-point inverse transform, the scale 1/n_fft riding on the window.
 *     v_t[j] = (w[j] / n_fft) * y_t[j] in float32 (the frame as the workspace holds it), and with j = p + n_fft/2 - t hop:
 *       out[c][p] = (sum over the t with 0 <= j < n_fft of v_t[j]) / (sum over the same t of w[j]^2),  0 <= p < n,
 *     both sums in float32 in ascending t from +0, the first by additions, the second by fused multiply-adds; 0 where the
 *     envelope is not above 1e-11 (torch.istft's threshold; with hop <= n_fft/2 it is above it everywhere).  This is
 *     dam_istft_f32's formula with length = n.  A gather, no atomics: device float32 [channels][n].
 *     A sample depends on its covering frames only, and a frame on its own window's gains only (bitwise): the samples at least
 *     n_fft/2 inside window w do not change when the gains of the other windows do.
 *   What follows (tests/test_bandmix_ref_cpu.py, in float64 to 1e-12): unit gains and unit fill give the stems' sum; gains
 *     constant over the bands and W = 1 give sum_s g_s x_s; with W > 1 a sample p with w n/W + n_fft/2 <= p < (w+1) n/W - n_fft/2
 *     (no margin at the two ends of the signal) is the gain-ramp mix's: only the frames that straddle a border cross-fade.
 *   What it is NOT: the inverse of the fit.  Piecewise-constant bin gains are a circular filter whose response the synthesis
 *     window truncates, so rendering gains and fitting the render does not give the gains back (planted random third-octave
 *     gains came back only to 0.3); the render of FITTED gains, though, leaves of the fit's target about what the fit's own
 *     residual says.
 *   dam_bandmix_render: one workgroup per (frame, channel) writes v_t to the workspace, one lane per output sample gathers.
 *     workspace: dam_bandmix_workspace_bytes(n_samples, channels, n_fft, hop) = 4 * channels * T * n_fft bytes (the synthesised
 *     frames, nothing else), 4-byte aligned; 0 for arguments the entry refuses.  workspace_bytes below that: DAM_ERR_WORKSPACE.
 *   Argument errors (a NULL pointer; S outside 1 .. DAM_GAINFIT_MAX_STEMS; channels not 1 or 2; n_fft not a power of two in
 *     64 .. 16384; hop < 1; n <= n_fft/2; W outside 1 .. n; a window without a frame; B outside 1 .. dam_spectrum_max_bands())
 *     return DAM_ERR_BAD_ARG before any launch.
 * Not covered: gains interpolated between the band centres, complex (phase-shifting) gains.
 * --------------------------------------------------------------------------------- */
int64_t dam_bandmix_workspace_bytes(int64_t n_samples, int channels, int n_fft, int hop);
int dam_bandmix_render(const void* x, int x_is_f64, int n_stems, int channels, int64_t n_samples, int64_t stem_stride,
                       int64_t sample_stride, int64_t channel_stride, const double* gains, const double* fill,
                       const int32_t* edges, int n_bands, int n_windows, const float* window, const float* twiddles, int n_fft,
                       int hop, float* out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Spectrogram distance (ABI 34): the frame-by-frame, bin-by-bin distance between the dB spectrogram of R candidate mixes
 * "stems x gain ramps" and that of one reference mix -- the criterion the models are trained on (model_trainer.py:34-35, a mean
 * squared error of amplitude_to_DB(|STFT|) features, data/dataset.py:145-155), measured on the audio that is rendered rather than
 * on the surrogate sum_s g_s dB(X_s) the network forms.  The band spectrum above and the short-term loudness error are its two
 * marginals (time averaged away; frequency summed away).  Neither a mix nor a spectrogram is written.  Every entry is stateless,
 * allocates nothing, does not synchronise with the host, uses no atomics and is hipGraph-capturable.  tests/_specdist_ref.py
 * restates the definition in numpy float64.
 *   Mix signal.  xm exactly as dam_spectrum_band_power forms it (channel mean of every stem times its gain, gain index
 *     min(p / (n / n_gains), n_gains-1), added in double in ascending stem order, rounded to float once; gains NULL: every gain
 *     exactly 1).  Candidates: stems x [S][n][channels] by element strides (float32 or float64), gains device float64
 *     [R][S][n_gains] or NULL (every row the plain sum), 1 <= R <= 65535.  Reference: its own stems ref [S_ref][n][ref_channels]
 *     with its own strides and type, ref_gains device float64 [S_ref][ref_n_gains] or NULL.  Both have n = n_samples samples.
 *   Frames and transform.  Those of the band spectrum: T = 1 + n / hop, frame_t[j] = xm[reflect(t*hop - n_fft/2 + j)] * w[j] in
 *     float32, the float32 LDS FFT, bins k = 0 .. n_fft/2, the imaginary parts of bins 0 and n_fft/2 taken as 0.
 *   Level.  p = re*re + im*im in float32 (every operation its own rounding);  L[t][k] = p <= amin*amin ? floor_db :
 *     3.01029995663981195f * log2f(p), the front-end's power_to_db, floor_db = (float)(20 log10((double)amin)), amin*amin a
 *     float32 product.  amin > 0; the model's is 1e-5 (floor -100 dB).  Every bin has weight 1: no c_k.
 *   Difference.  d_r[t][k] = (double)L_cand,r[t][k] - (double)L_ref[t][k]; d^2 = d*d in double.
 *   Cells.  Band b = bins edges[b] .. edges[b+1]-1, edges as dam_spectrum_band_power takes it (device int32 [B + 1], the CONTENT
 *     the caller's to check, clamped to [0, n_fft/2 + 1] by the kernels, 1 <= B <= dam_spectrum_max_bands()).  Window of frame t:
 *     the band fit's w(t) = min(min(t*hop, n-1) / (n / W), W-1), 1 <= W <= n, every window must own a frame.
 *       sums[r][b][w] = (sum d, sum d^2) over the frames of window w and the bins of band b   device float64 [R][B][W][2]
 *       count[b][w]   = frames of w times bins of b (geometry only)                            device int64 [B][W]
 *   Order of the float64 additions.  Per (row, frame, band), for sum d and sum d^2 alike: lane q of 64 adds the bins edges[b] + q,
 *     + 64, ... in ascending order from +0.0, then an xor-butterfly over the 64 partials, distances 1, 2, .. 32: one record.  A
 *     cell adds its frames' records in ascending t from +0.0.  So a cell depends on its own frames and bins and on its row's
 *     stems and gains only: it is bitwise reproducible and independent of R, of the other rows, of the other bands and of every
 *     sample further than n_fft/2 outside the centres of its own frames.
 *   dam_specdist_sums: two launches (frames: one workgroup per frame transforms the reference frame once and then every row's;
 *     cells).  workspace: dam_specdist_workspace_bytes(R, n, n_fft, hop, B, W) = 16 R T B bytes (the records), 16-byte aligned;
 *     0 for arguments the entry refuses.
 *   dam_specdist_summary: one launch; out device float64 [R][1 + B + W][3] = (mse, bias, rms_centred) of the whole row (index
 *     0), of every band (1 + b) and of every window (1 + B + w).  S1, S2, N are the sums of a figure's cells from +0.0: a band adds
 *     its cells in ascending window, a window in ascending band, and the row adds its bands' sums in ascending band.
 *     mse = S2 / N (dB^2, the criterion),  bias = S1 / N (dB),  rms_centred =
 *     sqrt(max(0, mse - bias*bias)) (dB; it does not move under a common gain wherever both levels are above the floor).
 *     N = 0: all three NaN.
 *   Argument errors (a NULL pointer other than gains / ref_gains; R outside 1 .. 65535; no stem; channels not 1 or 2; n_fft not a
 *     power of two in 64 .. 16384; hop < 1; n <= n_fft/2; gains with n_gains < 1 or > n; amin not above 0; B outside
 *     1 .. dam_spectrum_max_bands(); W outside 1 .. n; a window without a frame) return DAM_ERR_BAD_ARG before any launch.
 * Not covered: per-channel distances, perceptual (mel / loudness-weighted) bins.
 * --------------------------------------------------------------------------------- */
int64_t dam_specdist_workspace_bytes(int n_rows, int64_t n_samples, int n_fft, int hop, int n_bands, int n_windows);
int dam_specdist_sums(const void* x, int x_is_f64, int n_rows, int n_stems, int channels, int64_t n_samples,
                      int64_t stem_stride, int64_t sample_stride, int64_t channel_stride, const double* gains, int n_gains,
                      const void* ref, int ref_is_f64, int ref_stems, int ref_channels, int64_t ref_stem_stride,
                      int64_t ref_sample_stride, int64_t ref_channel_stride, const double* ref_gains, int ref_n_gains,
                      const float* window, const float* twiddles, int n_fft, int hop, float amin, const int32_t* edges,
                      int n_bands, int n_windows, double* sums, int64_t* count, void* workspace, void* stream);
int dam_specdist_summary(const double* sums, const int64_t* count, int n_rows, int n_bands, int n_windows, double* out,
                         void* stream);

/* ---------------------------------------------------------------------------------
 * Spectrogram distance: gradient (ABI 39): the gradient in the gains of the criterion above with one band over every bin --
 * what turns the figure into a loss for the gains a model put out, and what tells which stem pulls it in which window.  The
 * entry is stateless, allocates nothing, does not synchronise with the host, uses no atomics and is hipGraph-capturable.
 * tests/_specgrad_ref.py restates the definition in numpy float64.
 *   Clips.  n_clips independent problems in one call, 1 <= n_clips <= 65535: clip c has its stems at x + c * x_clip_stride and
 *     its reference at ref + c * ref_clip_stride (element strides), gains device float64 [n_clips][R][S][n_gains] or NULL (every
 *     gain exactly 1, R rows alike; the gradient is still defined), ref_gains device float64 [n_clips][S_ref][ref_n_gains] or
 *     NULL.  Everything else is addressed and typed as dam_specdist_sums takes it.
 *   Forward.  Mix signal, frames, transform, level and difference d_r[t][k] are dam_specdist_sums', operation for operation.
 *     Objective, per clip and row:  J_r = sum_t sum_{k = 0 .. n_fft/2} d_r[t][k]^2  (S2); the entry also returns S1 = sum d.
 *   Gradient.  dJ/dg[r][s][j] = sum_t sum_i z_t[i] * m_s[q(t,i)] * [gain_index(q(t,i)) == j],  q(t,i) = reflect(t*hop - n_fft/2 + i),
 *     m_s the stem's channel mean in double (((double)l + (double)r) * 0.5, or the single channel), gain_index(p) =
 *     min(p / (n / n_gains), n_gains-1);  z_t[i] = w[i] * y_t[i],  y_t[i] = Re sum_{k = 0 .. n_fft/2} u_k e^{+2 pi i ik / n_fft},
 *     u_k = (40 / ln 10) d_k X_k / p_k, and u_k = 0 where the candidate's p_k <= amin*amin (a floored level has no derivative;
 *     a floored REFERENCE bin still contributes its d).  The imaginary parts of X at DC and Nyquist are 0, as in the forward.
 *     The rounding of the mix signal to float is treated as the identity.
 *     Form the kernel uses: u_k = c_k X_k in float32 with c_k = (float)((40 / ln 10) d_k / (double)p_k);  y = half the
 *     UNNORMALISED inverse real transform (the float32 LDS FFT of dam_istft, its pre-twiddle included) of v, v_0 = 2 u_0,
 *     v_{n_fft/2} = 2 u_{n_fft/2}, v_k = u_k otherwise;  z_t[i] = w[i] * (0.5f * irfft_unnormalised(v)[i]) in float32; the
 *     products (double)z_t[i] * m_s[q] and their sums are float64.
 *   Gain segments.  With n_gains == 1 (or gains NULL) or n / n_gains >= n_fft a frame touches at most two gain segments:
 *     a(t) = gain_index(clamp(t*hop - n_fft/2, 0, n-1)) and a(t) + 1 (reflected samples fall in segment 0 and in the last one).
 *     Any other n_gains: DAM_ERR_UNSUPPORTED before a launch.
 *   Order of the float64 additions.  Per (clip, row, frame, stem) and per segment a(t), a(t)+1: lane l of 256 adds its positions
 *     i = l, l + 256, ... in ascending order from +0.0, then an xor-butterfly over the 64 lanes of a wave, distances 1, 2, .. 32,
 *     then the four waves as ((w0 + w1) + w2) + w3: one record.  (sum d, sum d^2) of a frame: lane l adds its bins l, l + 256,
 *     ... < n_fft/2 in ascending order from +0.0, lane 0 then bin n_fft/2; butterfly and waves as above.  grad[c][r][s][j] adds
 *     the records of the frames that touch node j in ascending t from +0.0: first t with t*hop + n_fft/2 - 1 >= j (n / n_gains)
 *     (j > 0) up to the last t with t*hop - n_fft/2 < (j + 1)(n / n_gains) (j < n_gains - 1); value[c][r] = (S1, S2) adds every
 *     frame's in ascending t from +0.0.  So an entry of grad depends on its own clip, its row's gains and the frames that touch
 *     its node only: it is bitwise reproducible and independent of R, of the other rows, of the other clips and of every sample
 *     that none of its node's frames covers.  S2 is dam_specdist_sums' sum d^2 over one band and one window in another order
 *     of addition: equal within rounding of the sums, not bit for bit.
 *   dam_specgrad: two launches (frames: one workgroup per (frame, clip) transforms the reference frame once and then, per row,
 *     the candidate frame forward and u backward; reduce).  value device float64 [n_clips][R][2] = (S1, S2); grad device
 *     float64 [n_clips][R][S][max(n_gains, 1)] (n_gains = 0 with gains NULL).  workspace:
 *     dam_specgrad_workspace_bytes(n_clips, R, S, n, n_fft, hop, n_gains) = 16 n_clips R T (S + 1) bytes (the records), 16-byte
 *     aligned; 0 for arguments the entry refuses.
 *   Argument errors (a NULL pointer other than gains / ref_gains; n_clips or R outside 1 .. 65535; no stem; channels not 1 or 2;
 *     n_fft not a power of two in 64 .. 16384; hop < 1; n <= n_fft/2; gains with n_gains < 1 or > n; amin not above 0) return
 *     DAM_ERR_BAD_ARG before any launch; outputs and workspace are untouched then, and for DAM_ERR_UNSUPPORTED alike.
 * Not covered: band or window weights in the objective, per-sample gain ramps (n / n_gains < n_fft), gradients in the stems or
 * in the reference, and a fitter on this gradient (records why).
 * --------------------------------------------------------------------------------- */
int64_t dam_specgrad_workspace_bytes(int n_clips, int n_rows, int n_stems, int64_t n_samples, int n_fft, int hop, int n_gains);
int dam_specgrad(const void* x, int x_is_f64, int n_clips, int n_rows, int n_stems, int channels, int64_t n_samples,
                 int64_t x_clip_stride, int64_t stem_stride, int64_t sample_stride, int64_t channel_stride, const double* gains,
                 int n_gains, const void* ref, int ref_is_f64, int ref_stems, int ref_channels, int64_t ref_clip_stride,
                 int64_t ref_stem_stride, int64_t ref_sample_stride, int64_t ref_channel_stride, const double* ref_gains,
                 int ref_n_gains, const float* window, const float* twiddles, int n_fft, int hop, float amin, double* value,
                 double* grad, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------
 * Alignment (ABI 28): the time offset of every stem against a mix by block cross-correlation, and the sample shift that removes
 * it -- what the gain fit above needs before it can be trusted on a mix that is not the sum of the same arrays (a dataset's
 * own mix file, a bounce with plug-in delay, a file trimmed by hand).  Every entry is stateless, allocates nothing, does not
 * synchronise with the host, uses no atomics and is hipGraph-capturable.  tests/_align_ref.py restates the definitions in
 * numpy float64.
 *   Signals.  Stems s = 0 .. S-1, 1 <= S <= 8, and one mix y, of `channels` (1 or 2) and n = n_samples samples, addressed as
 *     dam_gainfit_moments addresses them (element strides, float32 or float64, the mix independently of the stems).
 *     Mono signal: a_s[p] = (float)(((double)l + (double)r) * 0.5) for the two channels l, r, or (float) of the single
 *     channel; y[p] likewise for the mix.  A sample outside [0, n) is 0.
 *   Cross-correlation.  R_s[l] = sum_p a_s[p] * y[p + l], l in [-L, L], L = max_lag, 1 <= L <= dam_align_max_lag() (4096).
 *     A positive lag means the mix is late: y[q] = a[q - d] peaks at l = d.
 *   Framing.  N = dam_align_fft_size(L) = max(64, 4 * 2^ceil(log2 L)), H = N/2, T = ceil(n / H) frames.  Frame t of a stem
 *     holds a[t H + j] at j in [0, H) and zeros above; frame t of the mix holds y[t H - N/4 + j] at j in [0, N).  No window.
 *     A'_t, Y'_t = the float32 FFTs of the frames (twiddles as dam_stft_fill_twiddles_host(N) fills them), bins k = 0 .. N/2,
 *     the imaginary parts of bins 0 and N/2 taken as 0;
 *       C_s[k] = sum_t conj(A'_t[k]) * Y'_t[k]   in float64:
 *       re += (double)Ar (double)Yr + (double)Ai (double)Yi,  im += (double)Ar (double)Yi - (double)Ai (double)Yr.
 *     With this placement the circular correlation of a frame pair has no wrap-around for lags in [-N/4, N/4], so the sum
 *     over the frames is the LINEAR correlation: irfft(C_s)[l + N/4] = R_s[l], whatever n is and however it is cut.
 *     Energies: E_a = sum_p (double)a[p]^2, E_y likewise (every sample once: the stem frame's H samples, the mix frame's
 *     samples j in [N/4, N/4 + H)).
 *     Order of the float64 additions: one workgroup owns F = dam_align_frames_per_block() consecutive frames [i F, (i+1) F)
 *     of one (stem, mix) pair; lane l of its 256 keeps one running sum per bin l, l + 256, ... over those frames in
 *     ascending t (bin N/2 on lane 0), and one running sum per energy over the sample pairs (2m, 2m + 1) of its frames,
 *     m = l, l + 256, ..., frames ascending; the energies' 64 lanes of a wave are folded by an xor-butterfly, distances
 *     1, 2, .. 32, the four waves added as ((w0 + w1) + w2) + w3; a second kernel adds a pair's workgroup records in
 *     ascending i, starting from the first.  The order depends on (n, L) only: a pair is bitwise reproducible and does not
 *     depend on the other stems of the call or on how many there are.
 *   Weighting.  DAM_ALIGN_PLAIN: c = R_s.  DAM_ALIGN_PHAT: c = irfft(C_s[k] / (|C_s[k]| + DAM_ALIGN_PHAT_FLOOR * mean_k |C_s[k]|)),
 *     the mean over the N/2 + 1 bins (lane sums ascending, butterfly, four waves, as above).  The floor is smooth on
 *     purpose: no bin is switched on or off by a comparison.  The inverse transform is the float32 LDS FFT on the weighted
 *     spectrum scaled to unit peak magnitude, scaled back in float64.
 *   Estimate, per stem.  l* = argmax_l |c[l]|; ties go to the smallest |l|, then to the negative lag.  sign = the sign of
 *     c[l*] (-1: inverted polarity).  frac = 0.5 (y0 - y2) / (y0 - 2 y1 + y2) of y = |c| at l* - 1, l*, l* + 1; 0 at
 *     |l*| = L and where y0 - 2 y1 + y2 is not negative.  peak = |c[l*]| / sqrt(E_a E_y) for PLAIN, |c[l*]| for PHAT.
 *     status = 1; status = 0 for a silent stem or mix (E = 0) or a cross-spectrum that is zero in every bin: lag 0, frac 0,
 *     sign 0, peak NaN, curve 0.
 *   dam_align_estimate: lag, sign, status device int32 [S]; frac, peak device float64 [S]; curve: NULL or device float64
 *     [S][2 L + 1], c[l] at index l + L.  workspace: dam_align_workspace_bytes(S, n, L) bytes, 8-byte aligned.  Three launches
 *     (cross spectrum, reduce, finish).  More than 2^31 - 1 frames: DAM_ERR_UNSUPPORTED.
 *   dam_align_shift: out[s][p][c] = x[s][p - lag[s]][c], 0 where p - lag[s] is outside [0, n).  lag: DEVICE int32 [S] -- what
 *     dam_align_estimate wrote, so estimate -> shift -> fit needs no host round trip; + lag makes a stem as late as the mix is.
 *     x and out: float32 or float64 alike (x_is_f64), each with its own element strides; they must not overlap.
 *   Argument errors (a NULL pointer other than curve; S outside 1 .. 8; channels not 1 or 2; max_lag outside
 *     1 .. dam_align_max_lag(); non-positive n; an unknown weighting) return DAM_ERR_BAD_ARG before any launch;
 *     dam_align_fft_size and dam_align_workspace_bytes return 0 for them.
 * Not covered: offsets beyond dam_align_max_lag() (a decimated coarse stage would come first), drift and varispeed, and
 * sub-sample shifting (frac is reported, not applied).
 * --------------------------------------------------------------------------------- */
#define DAM_ALIGN_PLAIN 0
#define DAM_ALIGN_PHAT 1
#define DAM_ALIGN_PHAT_FLOOR 0x1.47ae147ae147bp-7 /* 1e-2 */
int dam_align_max_lag(void);
int dam_align_frames_per_block(void);
int dam_align_fft_size(int max_lag);
int64_t dam_align_workspace_bytes(int n_stems, int64_t n_samples, int max_lag);
int dam_align_estimate(const void* x, int x_is_f64, int n_stems, int channels, int64_t n_samples, int64_t stem_stride,
                       int64_t sample_stride, int64_t channel_stride, const void* y, int y_is_f64, int64_t y_sample_stride,
                       int64_t y_channel_stride, int max_lag, int weighting, const float* twiddles, int32_t* lag, double* frac,
                       double* peak, int32_t* sign, int32_t* status, double* curve, void* workspace, void* stream);
int dam_align_shift(const void* x, int x_is_f64, int n_stems, int channels, int64_t n_samples, int64_t stem_stride,
                    int64_t sample_stride, int64_t channel_stride, const int32_t* lag, void* out, int64_t out_stem_stride,
                    int64_t out_sample_stride, int64_t out_channel_stride, void* stream);

/* ---------------------------------------------------------------------------------
 * Stem input layout: x [B][C][HW] (C <= 16 planes, the reference's [B,S,F,T] feature stack) -> y [B][HW][16] with
 * channels C..15 zero, so that the first convolution (models/model_resnet.py:64,97) runs the NHWC kernels.
 * --------------------------------------------------------------------------------- */
int dam_nchw_to_nhwc16_f32(const float* x, int B, int C, int64_t HW, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DAM_HIP_H */
