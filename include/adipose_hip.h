/*
 * libadipose_hip — C ABI of the MI355X-native adipose U-Net hot path (gfx950 / CDNA4).
 *
 * The reference (MAGIC-SCAN/adipose_tissue-unet, TF 2.13 / Keras 2.13) has no FFI: its hot path is
 * the Keras graph built by AdiposeUNetV3.build_model (Segmentation/train_adipose_unet_v3.py:660-758)
 * plus the loss callables (:217-363), executed by TF/cuDNN. Each entry point below replaces one of
 * those implicit TF ops; the reference line it stands in for is cited on each declaration.
 *
 * Conventions
 *   - Every call returns 0 on success, <0 on error; adp_last_error() returns a thread-local message.
 *   - Pointers are DEVICE pointers unless stated; the caller owns every buffer.
 *   - Calls are asynchronous on the given hipStream_t (passed as void* so the header needs no HIP
 *     include). The library keeps a device workspace of its own: per device the BatchNorm accumulator
 *     replicas and the tile-claim counters, per (device, stream) scratch buffers and the deferral arena.
 *     The first use of a device or of a (device, stream) allocates, and so does a launch that needs more
 *     scratch or arena than the stream holds (growing scratch synchronises the device and frees the old
 *     buffer); no other call allocates, frees or synchronises, so a launch sequence that has run once
 *     on a stream can be captured in a hipGraph. adp_wgrad_release frees a stream's workspace.
 *   - dtype: ADP_DTYPE_F32 (parity path, exact f32 MFMA) or ADP_DTYPE_BF16 (throughput path,
 *     f32 accumulation); ADP_DTYPE_FP8 (e4m3fn operands, block-scaled MFMA, f32 accumulation) for
 *     forward-only launches (BASELINE.json configs[4]). Activations are NHWC with channel stride a
 *     multiple of 8.
 *   - GEMM weights are packed [Npad][Kpad] (output-channel major, K = taps*Cin_stride contiguous,
 *     Kpad = round_up(K,32), Npad = round_up(N,64)); tap order is row-major over (ky,kx).
 */
#ifndef ADIPOSE_HIP_H
#define ADIPOSE_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define ADP_DTYPE_F32 0
#define ADP_DTYPE_BF16 1
#define ADP_DTYPE_FP8 2 /* OCP e4m3fn, inference (forward) launches only */
#define ADP_ABI_VERSION 21 /* v4: adp_threshold_hist; v5: adp_maxpool2_bwd_bnr; v6: adp_aug_*, adp_percentile_normalize;
                              v7: handle engine adp_create / adp_forward / adp_*_param / adp_destroy;
                              v8: adp_train_step / adp_set_comm / adp_comm_*, adp_auc_metrics, adp_distance_transform, adp_boundary_metrics, adp_pack_weights_batch,
                              adp_bn_apply_maxpool2, adp_head_sigmoid_bwd_bnr;
                              v9: adp_conv_desc.bn_defer_fold + adp_bn_finalize_fold;
                              v10: adp_bn_bwd_apply_head, adp_head_sigmoid_bwd_bnr with dx = NULL, adp_conv_wgrad_bn;
                              v11: adp_sum_bf16; v12: adp_timing / adp_timing_read, unet_bn handle preset;
                              v13: adp_vec_mul (eval BatchNorm folded into the fp8 dequantisation scale);
                              v14: adp_scale_rows (eval BatchNorm folded into bf16 / f32 forward weights);
                              v15: adp_conv_wgrad_bn with dY = NULL (dz not stored), input-layer fused form;
                              v16: adp_bn_fold_reset, adp_debug_grad_flat;
                              v17: adp_wgrad_defer / adp_wgrad_flush
                              v18: adp_conv_io.act_outA;
                              v19: adp_conv_desc.CA_real / CB_real / Nout_real (zero-weight hints);
                              v20: adp_wgrad_release / adp_wgrad_arena_chunks (deferral arenas per (device, stream)), adp_get_option;
                              v21: adp_timing_filter; added under v21 (new exports only, nothing changed):
                              adp_morph_pack / adp_morph_bits / adp_morph_unpack;
                              adp_clahe_hist / adp_clahe_lut / adp_clahe_apply, adp_gray_stats, adp_u8_stretch;
                              adp_gray_morph / adp_gray_bgsum / adp_illum_finish;
                              adp_gray_colstats / adp_gray_colparams / adp_gray_colnorm / adp_gray_normalize;
                              adp_gray_blur / adp_gray_sharpen;
                              adp_fat_counts;
                              adp_poly_raster;
                              adp_resample_u8 / adp_resample_nearest_u8 */

typedef void* adp_stream_t; /* hipStream_t */

/* Geometry + epilogue of one implicit-GEMM convolution launch. */
typedef struct adp_conv_desc {
  int N, Hs, Ws;            /* source tensor(s) batch and spatial dims */
  int CA_stride, CB_stride; /* channel strides of source A / B (B = concat partner, 0 if none) */
  int upsample;             /* 1: nearest x2 upsample folded into the gather (UpSampling2D) */
  int Ho, Wo, stride;       /* output grid; input coord = o*stride + tap*dil - pad */
  int kh, kw, dil, pad;     /* tap grid */
  int Nout;                 /* GEMM N: output channels (padded) or 4*C for ConvTranspose */
  int relu;                 /* ReLU in the epilogue */
  float dropout_rate;       /* >0: inverted dropout after ReLU, stateless hash mask */
  unsigned dropout_seed;
  int out_stride;           /* channel stride of out */
  int out_mode;             /* 0 plain, 1 pixel-shuffle 2x2 (ConvTranspose), 2 channel split */
  int shuffle_c;            /* out_mode 1: channels per sub-pixel */
  int out2_stride, split_c; /* out_mode 2: channels >= split_c go to out2 */
  int mask_stride;          /* out = (acc [+addend]) * (mask>0) * mask_scale */
  float mask_scale;
  int mask2_stride;         /* same for the out2 part of a split store */
  float mask2_scale;
  int accum_stride;         /* accum (f32) += stored value */
  int bnr_stride;           /* channel stride of io->bnr_z */
  int out_fp8;              /* ADP_DTYPE_FP8 launches: 1 stores the output as fp8 e4m3 (else bf16); ADP_BF16
                               launches: 1 on an input layer (one 8-channel source, Nout 64) stores fp8 */
  int bn_defer_fold;        /* 1: leave this launch's BatchNorm statistics in the library's accumulator
                               replicas instead of adding them into io->bn_sum / bn_sqsum; the next launch
                               on the stream must be adp_bn_finalize_fold for those two vectors */
  int CA_real, CB_real;     /* v19, optional (0 = unknown): real channels of source A / B when the weight
                               columns of the pad channels [real, stride) are zeros (packed layers) */
  int Nout_real;            /* v19, optional (0 = unknown): real GEMM columns when weight rows [real, Nout)
                               are zeros. With these hints a kernel may skip products with zero weights
                               (f32 44-channel layers in 64-channel strides); results are unchanged.
                               Weight-gradient launches: the hints also require the pad channels of the
                               sources and of dY to be zeros, and the gradient of the pad rows and columns
                               is not accumulated */
} adp_conv_desc;

typedef struct adp_conv_io {
  const void* srcA;
  const void* srcB;
  const float* bn_scaleA; /* optional BatchNorm-apply + ReLU on load: x' = max(x*scale+shift, 0) */
  const float* bn_shiftA;
  const float* bn_scaleB;
  const float* bn_shiftB;
  const void* W;     /* packed weights, dtype of the launch */
  const float* bias; /* [Nout] or NULL */
  void* out;
  void* out2;
  const void* addend;
  const void* mask;
  const void* mask2;
  float* accum;
  float* bn_sum;     /* per-channel sum / sum of squares of the output (atomics), or NULL */
  float* bn_sqsum;
  /* optional fused BatchNorm-backward reduction over the stored output dA (out_mode 0; the
     adp_bn_bwd_reduce of the layer whose activation relu(z*scale+shift) this output is the
     gradient of): dbeta[c] += sum db, dgamma[c] += sum db*(z-mean)*invstd, db = dA*(z*scale+shift>0) */
  const void* bnr_z;
  const float* bnr_scale;
  const float* bnr_shift;
  const float* bnr_mean;
  const float* bnr_invstd;
  float* bnr_dgamma;
  float* bnr_dbeta;
  /* ADP_DTYPE_FP8 launches: per-GEMM-column dequantisation scale of W (adp_pack_weights_fp8) */
  const float* w_scale;
  /* (v18) with bn_scaleA / bn_shiftA on a one-source adp_conv_fwd: relu(srcA*scale+shift) is also stored here
     (srcA's shape and layout), bit-identical to adp_bn_apply(srcA) -> act_outA followed by the launch on
     act_outA; the persistent halo forward (3x3, 64 / 128 channels, BatchNorm statistics) does both in one
     launch, every other geometry runs exactly that pair */
  void* act_outA;
} adp_conv_io;

/* ---- library ---------------------------------------------------------------------------- */
const char* adp_last_error(void);
/* Name of the kernel instantiation the calling thread's last adp_conv_fwd / adp_conv_wgrad launched
   (as rocprofv3 prints it), for per-kernel timing and roofline accounting. */
const char* adp_last_kernel(void);
int adp_abi_version(void);
/* Build record: sha256 (hex) of the library's sources, in the Makefile's HASHED order (a caller can check that
 * a prebuilt binary matches the sources it ships with). */
const char* adp_source_hash(void);
/* Runtime switches, process-global (A/B of kernel variants in one process). value == INT_MIN restores
 * the built-in default. Kernel selection: "conv_fast" (2 = LDS-DMA kernels, default; 1 = register-staged;
 * 0 = generic), "fwd_tap64" / "wgrad_tap64" (0 off, 1 auto, 2+c force tile configuration c),
 * "tap64_bal", "tap64_korder", "wgrad_ra", "wgrad_blocks", "wgrad_min_chunk", "wgrad_glds_tn64";
 * epilogue store width (round 3, bit-identical either way): "tap64p_wide" (1), "tap64p_wide_f8" (0), "halop_wide"
 * (0 off, 1 tile-serial forms, 2 all, 3 default: all but the pipelined statistics forms), "cin8_wide" (1);
 * "wgrad_cin8_bna" (1: the input layer's fused BN-backward weight gradient when dY = NULL), "tap64_kpipe" (0:
 * mid-step barrier in the tap64 K loop); "wgrad_debug" / "fwd_debug" are timing-only ablations (results invalid).
 * "wgrad_arena_max_kb" (0 = no limit, default): the most KiB a stream's deferral arena may hold in total; a new chunk
 * is max(request, min(256 MiB, what is left under the limit)), and a request that would pass the limit takes its slabs
 * from scratch and is reduced at once, as after a failed allocation (same bits). */
int adp_set_option(const char* name, int value);
/* The value adp_set_option gave `name`, INT_MIN when unset (v20). "tap64_ksplit_last" is a report, not an option: the
 * split-K factor of the calling thread's last tap64 forward launch (0 = unsplit, INT_MIN before the first); setting it
 * is an error. */
int adp_get_option(const char* name);
/* Per-launch timing of the conv kernels (bench roofline; no reference counterpart). mode 1: clear the record
 * and start recording a HIP event pair around the MAIN kernel of every adp_conv_fwd / adp_conv_wgrad(_bn)
 * launch (the kernel adp_last_kernel names; statistic folds, split reduces, bias sums and BatchNorm applies
 * around it are excluded, so each pair times exactly one kernel of rocprofv3's list); 0: stop recording (the
 * record is kept); 2: stop and clear. */
int adp_timing(int mode);
/* Restricts the recording to launches whose kernel name (adp_last_kernel) equals `name` (NULL or "": every
 * launch): the bench times only its dominant kernel inside the timed region, where each event pair costs the
 * step time. */
int adp_timing_filter(const char* name);
/* Reads the record (synchronises on its events): *n = number of timed launches; for i < max: names[i *
 * name_len] = kernel name, ms[i] = its duration (-1 if its end was not marked). max = 0 only counts. */
int adp_timing_read(int max, char* names, int name_len, float* ms, int* n);

/* ---- dense layers (replace Conv2D / Conv2DBackpropInput / Conv2DBackpropFilter / BiasAdd /
 *      Relu / ResizeNearestNeighbor / ConcatV2 / AddN / Dropout of
 *      Segmentation/train_adipose_unet_v3.py:668-710, and ConvTranspose2D of the unet_bn preset) */
int adp_conv_fwd(int dtype, const adp_conv_desc* d, const adp_conv_io* io, adp_stream_t s);
/* ADP_DTYPE_FP8: srcA/srcB/W fp8 e4m3, channel strides and K multiples of 128 (one 128-channel K step
 * per tap), acc[m][n] * w_scale[n] (+ bias, ReLU) stored as bf16 or fp8 (desc.out_fp8); out_mode 0 or 1;
 * no BatchNorm / addend / mask / accumulate / dropout epilogue terms. */
/* dW[Npad][Kpad] (+)= sum_m dY[m][n] * X_tap(k)[m]; dB[n] (+)= sum_m dY[m][n]. f32 accumulators,
 * caller zeroes them. The gather is described by d/io exactly as for the forward launch. */
int adp_conv_wgrad(int dtype, const adp_conv_desc* d, const adp_conv_io* io, const void* dY,
                   int dy_stride, float* dW, float* dB, adp_stream_t s);
/* The BatchNorm backward of the layer this conv feeds (adp_bn_bwd_apply's arguments): dY of the weight
 * gradient is dz = bn_bwd_apply(dA, z) (dgamma / dbeta already reduced). */
typedef struct adp_bn_bwd_args {
  const void* dA;      /* gradient wrt relu(z*scale + shift), [M][dy_stride] */
  const void* z;       /* the layer's pre-BatchNorm output, [M][dy_stride] */
  const float *scale, *shift, *mean, *invstd, *gamma, *dgamma, *dbeta;
  float count;
} adp_bn_bwd_args;
/* adp_bn_bwd_apply(bn -> dY) followed by adp_conv_wgrad(dY), as one launch where the persistent halo
 * weight-gradient kernel takes the shape (3x3 stride-1 layers with <= 2 64-channel input chunks): dz is
 * computed while the weight gradient loads its tiles and stored into dY (for the data-gradient launch),
 * bit-identical to the two-launch form, which runs otherwise. dY may be NULL when dB is NULL and nothing
 * reads dz (the input layer has no data gradient): the fused forms then store nothing -- and the
 * input-layer kernel (one 8-channel source, 64 outputs) takes the fused form too -- while the two-launch
 * form computes dz in library scratch. */
int adp_conv_wgrad_bn(int dtype, const adp_conv_desc* d, const adp_conv_io* io, const adp_bn_bwd_args* bn,
                      void* dY, int dy_stride, float* dW, float* dB, adp_stream_t s);

/* Repack f32 master weights into the launch layout: mode 0 = cast only (forward);
 * mode 1 = 3x3 flip+transpose (data-gradient of a conv), mode 2 = ConvTranspose transpose. */
int adp_pack_weights(int dtype_out, int mode, int taps, int Cin_s, int Nout, const float* src,
                     int src_kpad, void* dst, int dst_rows, int dst_kpad, adp_stream_t s);
/* Modes 1/2 of adp_pack_weights for up to ADP_PACK_MAX_JOBS layers in one launch (LDS-tiled transpose,
 * coalesced both ways): dst[ci][t*Nout + co] = src[co][(taps-1-t)*Cin_s + ci], zeros elsewhere. */
#define ADP_PACK_MAX_JOBS 24
typedef struct adp_pack_job {
  const float* src;
  void* dst;
  int taps, Cin_s, Nout, src_kpad, dst_rows, dst_kpad;
} adp_pack_job;
int adp_pack_weights_batch(int dtype_out, int n, const adp_pack_job* jobs, adp_stream_t s);
/* Forward-layout fp8 weights with a per-row (output channel) scale: scale[r] = max_k |src[r][k]| / 448
 * (1 for an all-zero row), dst[r][k] = e4m3(src[r][k] / scale[r]) (saturating, round to nearest even). */
int adp_pack_weights_fp8(int rows, const float* src, int src_kpad, void* dst, int dst_kpad, float* scale,
                         adp_stream_t s);

/* ---- pooling / upsampling (MaxPooling2D :670,674,678; UpSampling2D grad) ------------------- */
int adp_maxpool2_fwd(int dtype, int N, int H, int W, int C_stride, const void* src,
                     const float* bn_scale, const float* bn_shift, void* dst, adp_stream_t s);
/* 2x2 max-pool with an fp8 e4m3 output; src of dtype dtype_in (F32, BF16 or FP8) */
int adp_maxpool2_fwd_fp8(int dtype_in, int N, int H, int W, int C_stride, const void* src, void* dst_fp8,
                         adp_stream_t s);
int adp_maxpool2_bwd(int dtype, int N, int H, int W, int C_stride, const void* src,
                     const float* bn_scale, const float* bn_shift, const void* dpool,
                     const void* addend, const void* mask, float mask_scale, void* dsrc,
                     adp_stream_t s);
/* unet_bn encoder pool backward: dsrc = route_argmax(dpool) + addend (no BN-on-load, no mask), with the
 * BatchNorm-backward reduction of the layer whose activation src = relu(z*scale+shift) fused in:
 * dbeta += sum db, dgamma += sum db*(z-mean)*invstd, db = dsrc*(z*scale+shift > 0) over the stored dsrc
 * (replaces adp_maxpool2_bwd + adp_bn_bwd_reduce; train_adipose_unet_v3.py:670 MaxPooling2D grad).
 * src may be NULL: the argmax then runs over relu(z*scale+shift) recomputed and rounded to dtype, the
 * values adp_bn_apply / adp_bn_apply_maxpool2 store (one full-resolution read less) */
int adp_maxpool2_bwd_bnr(int dtype, int N, int H, int W, int C_stride, const void* src, const void* dpool,
                         const void* addend, void* dsrc, const void* z, const float* scale, const float* shift,
                         const float* mean, const float* invstd, float* dgamma, float* dbeta, adp_stream_t s);
/* unet_bn encoder: act = relu(z * scale + shift) (adp_bn_apply) and pool = maxpool2(act) in one pass */
int adp_bn_apply_maxpool2(int dtype, int N, int H, int W, int C_stride, const void* z, const float* scale,
                          const float* shift, void* act, void* pool, adp_stream_t s);
int adp_upsample2_bwd(int dtype, int N, int Hs, int Ws, int C_stride, const void* dup,
                      const void* addend, const void* mask, float mask_scale, void* dsrc,
                      adp_stream_t s);
/* out = (a [+ b]) * (mask>0 ? mask_scale : 0) [mask optional]; elementwise over n elements */
int adp_ew_add_mask(int dtype, size_t n, const void* a, const void* b, const void* mask,
                    float mask_scale, void* out, adp_stream_t s);
int adp_cast(int dtype_in, int dtype_out, size_t n, const void* src, void* dst, adp_stream_t s);
int adp_fill_f32(size_t n, float value, float* dst, adp_stream_t s);
/* out = bf16(sum of nsrc (1..8) bf16 maps of n elements, f32 sum in source order): the dilated
   bottleneck's Add (train_adipose_unet_v3.py:688) as one pass after its six convs; n % 8 == 0, srcs is a
   host array of 16-B aligned device pointers */
int adp_sum_bf16(int nsrc, const void* const* srcs, size_t n, void* out, adp_stream_t s);

/* ---- BatchNorm (unet_bn preset; training-mode batch statistics) -------------------------- */
int adp_bn_finalize(int C, float count, const float* sum, const float* sqsum, const float* gamma,
                    const float* beta, float eps, float momentum, float* scale, float* shift,
                    float* mean, float* invstd, float* running_mean, float* running_var,
                    adp_stream_t s);
/* adp_bn_finalize of statistics a conv launch left in the accumulator replicas (bn_defer_fold): first
 * sum[c] += replicas, sqsum[c] += replicas (the replicas are re-zeroed), then the finalize; one launch in
 * place of the fold + finalize pair. */
int adp_bn_finalize_fold(int C, float count, float* sum, float* sqsum, const float* gamma, const float* beta,
                         float eps, float momentum, float* scale, float* shift, float* mean, float* invstd,
                         float* running_mean, float* running_var, adp_stream_t s);
/* Drops a bn_defer_fold record that never reached its adp_bn_finalize_fold (an error or exception between the
 * two) and re-zeroes the replicas, stream-ordered on s; a no-op when nothing is pending, and when the pending
 * record was made on another stream (another caller's fold, possibly still in flight). Trainer steps and
 * adp_train_step call it first, so a failed step cannot poison the replicas for the rest of the process. */
int adp_bn_fold_reset(adp_stream_t s);
/* Deferred weight-gradient reductions (round 5). The weight / bias gradient launches (adp_conv_wgrad, _bn) sum per-block
 * partial slabs in a fixed order (deterministic) with a small reduce launch each. Between adp_wgrad_defer(1, s) and
 * adp_wgrad_flush(s), launches on stream s write their slabs to a per-stream arena and only record the reduction;
 * adp_wgrad_flush launches every recorded reduction as one kernel (same arithmetic: bit-identical gradients) and ends
 * the deferral. Until the flush the dW / dB buffers of those launches are NOT final: call it before anything reads
 * them (the optimizer, a gradient all-reduce). adp_wgrad_defer(0, s) with reductions pending is an error. */
int adp_wgrad_defer(int on, adp_stream_t s);
int adp_wgrad_flush(adp_stream_t s);
/* Frees the whole workspace of (current device, stream s) and forgets the stream (v20): the deferral arena -- chunks of
 * 256 MiB or the request if larger (option "wgrad_arena_max_kb" limits them), allocated by the first deferred steps and
 * reused afterwards -- and the stream's scratch buffers. Synchronises s if it holds anything; an error with reductions
 * pending. Call it before destroying a stream the library has launched on. adp_wgrad_arena_chunks: the number of arena
 * chunks of (device, s) (test hook). */
int adp_wgrad_release(adp_stream_t s);
int adp_wgrad_arena_chunks(adp_stream_t s);
/* a = relu(z*scale + shift), the post-BatchNorm activation, materialised once per layer */
int adp_bn_apply(int dtype, size_t M, int C, const void* z, const float* scale, const float* shift,
                 void* out, adp_stream_t s);
/* the same activation stored as fp8 e4m3 (z of dtype dtype_in): the operand of an fp8 conv launch */
int adp_bn_apply_fp8(int dtype_in, size_t M, int C, const void* z, const float* scale, const float* shift,
                     void* out_fp8, adp_stream_t s);
/* out[i] = a[i] * b[i] (f32 vectors): e.g. an fp8 layer's per-column dequantisation scale times its eval
   BatchNorm scale, so that the conv epilogue writes relu(bn(z)) directly (UNetBN.forward_fp8) */
int adp_vec_mul(size_t n, const float* a, const float* b, float* out, adp_stream_t s);
/* dst[r][c] = src[r][c] * scale[r] (0 for r >= nscale), c < cols, stored as dtype_out (ADP_DTYPE_F32 / BF16): a
   layer's forward weights ([Npad][Kpad] master layout) with its eval BatchNorm scale folded in, so that the conv
   epilogue (bias = BN shift, ReLU) writes relu(bn(z)) directly (UNetBN.forward(train=False)) */
int adp_scale_rows(int dtype_out, int rows, int cols, const float* src, int src_ld, const float* scale, int nscale,
                   void* dst, int dst_ld, adp_stream_t s);
/* dBN = dA * (relu(z*scale+shift) > 0); dgamma += sum dBN*xhat; dbeta += sum dBN */
int adp_bn_bwd_reduce(int dtype, size_t M, int C, const void* dA, const void* z, const float* scale,
                      const float* shift, const float* mean, const float* invstd, float* dgamma,
                      float* dbeta, adp_stream_t s);
int adp_bn_bwd_apply(int dtype, size_t M, int C, const void* dA, const void* z, const float* scale,
                     const float* shift, const float* mean, const float* invstd,
                     const float* gamma, const float* dgamma, const float* dbeta, float count,
                     void* dz, adp_stream_t s);
/* adp_bn_bwd_apply of the layer under the unet_bn sigmoid head with dA recomputed instead of read:
 * dA[m][c] = dtype(dp[m] * p[m] * (1 - p[m]) * W[c]) (0 for c >= Cin; Cin % 8 == 0, W 16-B aligned), the value adp_head_sigmoid_bwd_bnr
 * stores, so that launch can run with dx = NULL (one full-resolution write and read fewer; bit-identical dz) */
int adp_bn_bwd_apply_head(int dtype, size_t M, int C, int Cin, const float* W, const float* p, const float* dp,
                          const void* z, const float* scale, const float* shift, const float* mean,
                          const float* invstd, const float* gamma, const float* dgamma, const float* dbeta,
                          float count, void* dz, adp_stream_t s);

/* ---- heads (Conv2D(2,1,softmax)[...,1] :729-731; Conv2D(1,1,sigmoid) :715,722) ------------- */
/* p = softmax(W x + b)[1] = sigmoid(z1 - z0); W f32 [2][Cin], b f32 [2] */
int adp_head_softmax2_fwd(int dtype, size_t M, int C_stride, int Cin, const void* x, const float* W,
                          const float* b, const float* bn_scale, const float* bn_shift, float* p,
                          adp_stream_t s);
int adp_head_softmax2_bwd(int dtype, size_t M, int C_stride, int Cin, const void* x, const float* W,
                          const float* bn_scale, const float* bn_shift, const float* p,
                          const float* dp, const void* addend, const void* mask, float mask_scale,
                          void* dx, float* dW, float* db, adp_stream_t s);
/* bn_scale / bn_shift non-NULL (forward and backward alike): x is a pre-BN map and the head reads
   dtype(relu(x*scale+shift)), the value adp_bn_apply would materialize; dW is taken from that rounded value */
/* p = sigmoid(W x + b); W f32 [Cin], b f32 [1] */
int adp_head_sigmoid_fwd(int dtype, size_t M, int C_stride, int Cin, const void* x, const float* W,
                         const float* b, const float* bn_scale, const float* bn_shift, float* p,
                         adp_stream_t s);
int adp_head_sigmoid_bwd(int dtype, size_t M, int C_stride, int Cin, const void* x, const float* W,
                         const float* bn_scale, const float* bn_shift, const float* p,
                         const float* dp, const void* addend, const void* mask, float mask_scale,
                         void* dx, float* dW, float* db, adp_stream_t s);
/* unet_bn head backward with the BatchNorm-backward reduction of the layer under it fused (adp_bn_bwd_reduce):
 * z = that layer's pre-BN output (the head reads relu(z*sc+sh)), dx = dL/d relu(bn(z)) stored, and
 * dbeta += sum db, dgamma += sum db*(z-mean)*invstd with db = dx*(z*sc+sh > 0) over the (rounded) dx;
 * dx may be NULL (the sums are the same; adp_bn_bwd_apply_head then recomputes dx) */
int adp_head_sigmoid_bwd_bnr(int dtype, size_t M, int C_stride, int Cin, const void* z, const float* W,
                             const float* scale, const float* shift, const float* mean, const float* invstd,
                             const float* p, const float* dp, void* dx, float* dW, float* db, float* dgamma,
                             float* dbeta, adp_stream_t s);
/* tf.image.resize(..., method='bilinear') (half-pixel centres, no antialias), 1 channel, f32
 * (:716-719, :723-726) and its adjoint. */
int adp_resize_bilinear_fwd(int N, int Hs, int Ws, int Ho, int Wo, const float* src, float* dst,
                            adp_stream_t s);
int adp_resize_bilinear_bwd(int N, int Hs, int Ws, int Ho, int Wo, const float* dout, float* dsrc,
                            adp_stream_t s);

/* ---- losses & metrics (dice_loss / combined_loss_* / OHEM :217-363; dice_coef model.py:93-98) */
/* stats[0..7] += {sum y*p', sum y, sum p', sum y*p, sum y, sum p (raw y, p), #((p>0.5)==y),
 *                 sum y*(p>0.5)} where
 * p' = clip(p,1e-7,1-1e-7) and y is the (optionally smoothed) label; row_bce[b*H+h] = mean_w BCE. */
int adp_loss_rows(int N, int H, int W, const float* p, const float* y, int smooth, float eps_pos,
                  float eps_neg, float* row_bce, double* stats, adp_stream_t s);
/* One block per image: selects rows (OHEM top-k with k = int(H*keep_ratio) or all rows), writes
 * row_coef[b*H+h] = weight/(norm_rows*W) for selected rows else 0, and out[0] += weight*bce_part,
 * with norm_rows the GLOBAL number of selected rows (all ranks). */
int adp_loss_select(int N, int H, int W, const float* row_bce, int ohem, float keep_ratio,
                    float weight, float norm_rows, float* row_coef, double* out, adp_stream_t s);
/* dp (+)= row_coef*dBCE/dp + weight*dDice/dp (through the clip), given GLOBAL dice stats. */
int adp_loss_grad(int N, int H, int W, const float* p, const float* y, int smooth, float eps_pos,
                  float eps_neg, const float* row_coef, const double* stats, float weight,
                  int accumulate, float* dp, adp_stream_t s);
/* tp, fp, fn, tn of (pred>thr) vs (true>0.5) (full_evaluation_enhanced.py:721-785), int64 out */
int adp_pixel_counts(size_t n, const float* pred, const float* truth, float thr,
                     unsigned long long* counts, adp_stream_t s);
/* Threshold sweep of optimize_threshold_f1(_slide_level) (full_evaluation_enhanced.py:891-980) in one pass:
 * thr = nthr (<= 64) ascending HOST doubles; hist[b*(nthr+1) + j] (+)= #pixels with truth bit b
 * (truth > 0.5) and j = #{t : pred > thr[t]}. tp(t) = sum_{j>t} hist[nthr+1+j], fp(t) = sum_{j>t} hist[j]. */
int adp_threshold_hist(size_t n, const float* pred, const float* truth, int nthr, const double* thr,
                       unsigned long long* hist, adp_stream_t s);

/* ---- the rest of the src/utils/model.py loss / metric surface (not on the v3 training step) ---------- */
/* weighted_dice_loss / weighted_bce_dice_loss weight map (model.py:104-116, 140-151): y (B,H,W) f32 is expanded
 * to (1,B,H,W) channels_last, so K.pool2d(ksize x ksize, stride 1, 'same', 'avg') averages over (B, H) per W
 * (TF 'SAME' average: padding excluded from the count); weight = 1 + 2 * (0.005 < avg < 0.995); wsum[0] +=
 * sum(weight) (f64, caller zeroes). tmp: B*H*W f32 scratch. ksize odd (21 in the reference). */
int adp_border_weight(int B, int H, int W, int ksize, const float* y, float* tmp, float* weight, double* wsum,
                      adp_stream_t s);
/* With w = weight * (n / wsum[0]) (f32, the w0/w1 renormalisation): stats[0..4] += {sum w^2 y p, sum w^2 y,
 * sum w^2 p, sum bce_w, sum w}, bce_w = (1-y) l + (1 + (w-1) y)(log(1 + exp(-|l|)) + max(-l, 0)),
 * l = log(p'/(1-p')), p' = clip(p, 1e-7, 1-1e-7) (weighted_dice_coeff :120-125, weighted_bce_loss :127-136). */
int adp_weighted_loss_stats(size_t n, const float* y, const float* p, const float* weight, const double* wsum,
                            double* stats, adp_stream_t s);
/* dp = wbce * d(stats[3]/stats[4])/dp + wdice * d(1 - (2 stats[0] + 1)/(stats[1] + stats[2] + 1))/dp (TF's
 * subgradients of clip / abs / maximum), from the final stats. */
int adp_weighted_loss_grad(size_t n, const float* y, const float* p, const float* weight, const double* wsum,
                           const double* stats, float wbce, float wdice, float* dp, adp_stream_t s);
/* K.mean / K.min / K.max / K.std (population) of n floats (act_mean, act_min, act_max, act_std, mean_diff
 * model.py:21-34): out (device f64[4]) = {mean, min, max, std}; work >= 1024 * 40 bytes. */
int adp_value_stats(size_t n, const float* x, void* work, double* out, adp_stream_t s);
/* argmax / argmin over the last axis (first occurrence) of y and p, rows x W (model.py:36-91): out (int64[7],
 * caller zeroes) += {tru_pos = sum at*ap, fls_pos = sum clip(ap-at,0,1), tru_neg = sum it*ip,
 * fls_neg = sum clip(ip-it,0,1), #(at*ap >= 1), #(ap >= 1), #(at >= 1)} (the last three: precision_onehot /
 * recall_onehot's rounded counts). */
int adp_onehot_counts(int rows, int W, const float* y, const float* p, unsigned long long* out, adp_stream_t s);

/* ---- training-time augmentation + normalisation of gray (H, W) f32 planes (src/utils/data.py:13-264,
 * 398-429); random parameters are drawn by the host in the reference's RandomState order ---------- */
/* np.rot90(k) then fliplr then flipud (random_rotation_90 / random_flip, data.py:13-29); out of place */
int adp_aug_geom(int H, int W, const float* src, float* dst, int k, int flip_lr, int flip_ud, adp_stream_t s);
/* mode 0 brightness clip(x*f,0,255), 1 contrast clip((x-m)*f+m,0,255), 2 gamma (x/255)^f*255 (:32-50),
 * 3 z-score (x-m)/f (TileDataset, train_adipose_unet_v3.py:589-590) */
int adp_aug_photometric(size_t n, const float* src, float* dst, int mode, float f, float m, adp_stream_t s);
/* clip(x + noise, 0, 255) with noise f64 (random_gaussian_noise, :63-69) */
int adp_aug_noise(size_t n, const float* src, const double* noise, float* dst, adp_stream_t s);
/* *out += sum(src) in f64 (contrast's image.mean()) */
int adp_aug_sum(size_t n, const float* src, double* out, adp_stream_t s);
/* separable Gaussian (cv2.GaussianBlur, BORDER_REFLECT_101), taps[2r+1]; dtype64: src/tmp/dst are f64 */
int adp_aug_blur(int dtype64, int H, int W, const void* src, void* tmp, void* dst, const float* taps, int radius,
                 adp_stream_t s);
/* random_scale (:72-106): cv2.resize to (Hn, Wn) (linear, or nearest for masks) + center crop / pad */
int adp_aug_scale(int H, int W, int Hn, int Wn, const float* src, float* dst, int nearest, adp_stream_t s);
/* elastic_transform (:109-145): remap image (linear, reflect) and mask (nearest, 0) by (x+dx*alpha, y+dy*alpha) */
int adp_aug_remap(int H, int W, const float* src, const float* msrc, const double* dx, const double* dy, double alpha,
                  float* dst, float* mdst, adp_stream_t s);
/* normalize_image(method='percentile') (:398-429) with exact order statistics (radix select on the
 * device); work >= 64 + 32768 bytes; p_out (nullable) receives (p_low, p_high) values */
int adp_percentile_normalize(size_t n, const float* src, float* dst, double p_low, double p_high, void* work,
                             float* p_out, adp_stream_t s);

/* ---- Reinhard stain normalisation of packed uint8 RGB tiles (N, H, W, 3), each tile with its own statistics
 *      (src/utils/stain_normalization.py:32-146; build_dataset.py:1234-1238 applies it tile by tile). rgb2lab /
 *      lab2rgb are skimage's documented D65 / 2-degree conversions; per-pixel maths f32, sums f64 ------------- */
/* per-tile LAB statistics: stats[n] = {meanL, meanA, meanB, stdL, stdA, stdB} f64, population std
 * (ReinhardStainNormalizer._calculate_lab_stats, :76-92). Deterministic (fixed-order partials, no float atomics);
 * sums are of deviations from the tile's first pixel, so a constant tile has std exactly 0 */
int adp_stain_lab_stats(int N, int H, int W, const uint8_t* rgb, double* stats, adp_stream_t s);
/* normalize_image (:94-146): (lab - src_mean) * (tgt_std / src_std) + tgt_mean per channel (tgt_mean where
 * src_std == 0), lab2rgb, clip to [0, 1], uint8 by truncation of x * 255. src_stats (N, 6) device f64 as written by
 * adp_stain_lab_stats; tgt[6] HOST f64 in the same order. rgb_out (N, H, W, 3) u8 and / or gray_out (N, H, W) f32 =
 * (R*19595 + G*38470 + B*7471 + 0x8000) >> 16 of the output bytes (PIL mode L); either may be NULL, not both */
int adp_stain_reinhard_apply(int N, int H, int W, const uint8_t* rgb, const double* src_stats, const double* tgt,
                             uint8_t* rgb_out, float* gray_out, adp_stream_t s);

/* ---- tile quality control (classify_tiles_batch, Segmentation/build_dataset.py:1253-1284): integer sums behind
 *      white_ratio and the variance of the Laplacian; exact, so independent of N, the grid and the run ---------- */
/* Per-tile quality sums of packed uint8 RGB tiles. Byte c of pixel (y, x) of tile n is
 * rgb[origin(n) + y*row_pitch + 3*x + c]; origin(n) = origins[n] (device array of N byte offsets, so the
 * tiles may be overlapping windows of one image), or n*H*row_pitch when origins is NULL. row_pitch >= 3*W
 * (0 means 3*W). sums: (N, 4) int64 on the device: {white, S1, S2, H*W}.
 * white: pixels with R, G and B all >= white_threshold; gray = (R*9798 + G*19235 + B*3735 + 16384) >> 15 (OpenCV's
 * 8-bit BGR2GRAY); lap = g(y-1,x) + g(y+1,x) + g(y,x-1) + g(y,x+1) - 4 g(y,x) with reflect-101 borders within the
 * tile (cv2.Laplacian, ksize 1); S1 = sum lap, S2 = sum lap^2. Fails (message, nothing launched, sums untouched) on a
 * NULL rgb or sums, N < 1, H < 2 or W < 2, or a non-zero row_pitch below 3*W */
int adp_tile_qc(int N, int H, int W, const uint8_t* rgb, long long row_pitch, const long long* origins,
                int white_threshold, long long* sums, adp_stream_t s);

/* ---- connected components of binary maps (remove_small_components, Segmentation/build_dataset.py:1122-1131 and
 *      build_test_dataset.py:374, flag --min-cc-px: cv2.connectedComponentsWithStats(connectivity=8), keep
 *      area >= min_px; analyze_cell_characteristics, pre-post-processing_tools/analysis/morphology
 *      parameter_analysis/analyze_training_data.py:76-130: num_cells, areas, tissue_coverage). All stream-ordered,
 *      none synchronises; integer results, exact and independent of N, the grid, the schedule and the run ---------- */
#define ADP_CC_SRC_U8 0  /* foreground: byte != 0 */
#define ADP_CC_SRC_F32 1 /* foreground: value > thr */
/* region of the in-LDS labelling stage (tests place their shapes around it) */
#define ADP_CC_REGION_ROWS 32
#define ADP_CC_REGION_COLS 64
/* labels (N, H, W) int32: 0 for background, else 1 + the raster index y*W + x, within the pixel's own image, of the
 * first pixel (smallest index) of its component. src (N, H, W) of src_dtype; thr is used by ADP_CC_SRC_F32 only.
 * connectivity 8 (cv2 connectivity=8, skimage measure.label's 2-D default) or 4 (scipy.ndimage.label's default).
 * Fails (message, nothing launched) on a NULL pointer, N, H or W < 1, H*W > 2^31 - 2, a connectivity other than 4 / 8,
 * or an unknown src_dtype */
int adp_cc_label(int N, int H, int W, const void* src, int src_dtype, float thr, int connectivity, int* labels,
                 adp_stream_t s);
/* area (N, H, W) int32: the pixel count of a component at the position of its first pixel, 0 everywhere else.
 * labels as written by adp_cc_label */
int adp_cc_areas(int N, int H, int W, const int* labels, int* area, adp_stream_t s);
/* remove_small_components: 1 where the pixel's component has area >= min_px, else 0; as uint8 and / or f32
 * (either may be NULL, not both). area as written by adp_cc_areas */
int adp_cc_filter(int N, int H, int W, const int* labels, const int* area, int min_px, uint8_t* out_u8, float* out_f32,
                  adp_stream_t s);
/* counts[n] = the number of components of image n (always the true number). table (N, max_rows, 8) int64, rows
 * {first, area, x_min, y_min, x_max, y_max, sum_x, sum_y} in ascending order of `first` (row k: the component a raster
 * scan meets k-th); components beyond max_rows are dropped, rows past counts[n] are zero. cv2's stats: width =
 * x_max - x_min + 1, height = y_max - y_min + 1, centroid = (sum_x / area, sum_y / area). max_rows = 0 (table may
 * then be NULL) only counts */
int adp_cc_table(int N, int H, int W, const int* labels, int max_rows, long long* table, int* counts, adp_stream_t s);
/* dense (N, H, W) int32: 0 for background, else 1 + the row of the pixel's component in adp_cc_table's order
 * (labels 1..K in raster order of first pixel, as cv2 numbers them) */
int adp_cc_relabel(int N, int H, int W, const int* labels, int* dense, adp_stream_t s);
/* tile of adp_cc_shape's kernel (tests place their shapes around it; the kernel reads a two-pixel halo around it) */
#define ADP_CC_SHAPE_TILE_ROWS 64
#define ADP_CC_SHAPE_TILE_COLS 128
/* the integer sums behind analyze_cell_characteristics' perimeter, circularity, aspect ratio and eccentricity.
 * shape (N, max_rows, 8) int64, rows {first, S_xx, S_yy, S_xy, p_straight, p_diag, p_mixed, border_px} in
 * adp_cc_table's order and with its truncation (components beyond max_rows dropped, unused rows zero). S_xx = sum x^2,
 * S_yy = sum y^2, S_xy = sum x*y over the component's pixels (x the column, y the row). A border pixel has an edge
 * neighbour that is not in its component (another label, or outside the image); its code is 1 + 2*n4 + 10*nd with n4 /
 * nd its edge / diagonal neighbours that are border pixels of the same component. p_straight counts the codes
 * {5, 7, 15, 17, 25, 27}, p_diag {21, 33}, p_mixed {13, 23}, border_px all border pixels; perimeter = p_straight +
 * sqrt(2)*p_diag + (1 + sqrt(2))/2*p_mixed. Stream-ordered, no synchronisation. Fails (message, nothing launched) on a
 * NULL pointer (shape may be NULL only with max_rows = 0, which does nothing), max_rows < 0, a shape the other calls
 * refuse, or H*W*(max(H, W) - 1)^2 >= 2^63 (the moment sums are int64) */
int adp_cc_shape(int N, int H, int W, const int* labels, int max_rows, long long* shape, adp_stream_t s);

/* ---- binary mask morphology on bit-packed planes (morph_close, Segmentation/build_dataset.py:1190 and
 *      build_test_dataset.py:596, flag --morph-close-k: cv2.morphologyEx(MORPH_CLOSE, getStructuringElement(
 *      MORPH_ELLIPSE, (k, k))), the step before remove_small_components). A plane is (N, H, WW) 64-bit words,
 *      WW = ceil(W / 64); bit b of word w of a row is pixel x = 64 w + b; the bits past W in a row's last word are 0 and
 *      every call that writes a plane keeps them 0. All stream-ordered, none synchronises; exact and independent of N,
 *      the grid and the run. N = 0 returns 0 without a launch ------------------------------------------------------ */
#define ADP_MORPH_DILATE 0
#define ADP_MORPH_ERODE 1
#define ADP_MORPH_KMAX 63
/* words a block of adp_morph_bits produces (tests place their shapes around it) */
#define ADP_MORPH_TILE_ROWS 32
#define ADP_MORPH_TILE_WORDS 8
/* bits = the packed foreground of src (N, H, W) of src_dtype (ADP_CC_SRC_U8: byte != 0; ADP_CC_SRC_F32: value > thr) */
int adp_morph_pack(int N, int H, int W, const void* src, int src_dtype, float thr, unsigned long long* bits,
                   adp_stream_t s);
/* dst = dilation (ADP_MORPH_DILATE) or erosion (ADP_MORPH_ERODE) of src by the footprint of ksize rows of column extents
 * [row_lo[a], row_hi[a]) (HOST arrays, as adp_boundary_refine's), anchor ksize / 2 both ways:
 *   dilate(M)(y, x) = OR  over row_lo[a] <= b < row_hi[a] of M(y + a - ksize/2, x + b - ksize/2)
 *   erode(M)(y, x)  = AND over the same offsets (not the reflected ones)
 * positions outside the image take no part in either (OpenCV's default morphology border: an all-ones mask erodes to
 * all ones). 1 <= ksize <= ADP_MORPH_KMAX; src must not overlap dst. Fails (message, nothing launched) on a NULL
 * pointer, N < 0, H or W < 1, a ksize out of range, a row with row_lo < 0, row_hi > ksize or row_lo > row_hi, an unknown
 * op, or overlapping planes */
int adp_morph_bits(int N, int H, int W, const unsigned long long* src, unsigned long long* dst, int ksize,
                   const int* row_lo, const int* row_hi, int op, adp_stream_t s);
/* the plane as 0 / 1 uint8 and / or 0.0 / 1.0 f32, (N, H, W) each (either may be NULL, not both) */
int adp_morph_unpack(int N, int H, int W, const unsigned long long* bits, uint8_t* out_u8, float* out_f32,
                     adp_stream_t s);

/* ---- annotation polygons -> ground-truth planes (create_binary_mask, Segmentation/build_dataset.py:903-911: one
 *      cv2.fillPoly over all polygons of an image), in the plane format above. mask = interior | boundary:
 *        interior(y, x) = parity over every non-horizontal edge of every polygon of the image of
 *                         [ylo <= y < yhi and X(y) <= x], X(y) = xlo + (y - ylo)(xhi - xlo) / (yhi - ylo) exactly
 *                         (even-odd filling: where two polygons overlap the interior cancels)
 *        boundary       = every edge's 8-connected line from the endpoint (xa, ya) with the smaller x, dx = xb - xa,
 *                         dy = yb - ya, s = sign(dy): |dy| > dx: (xa + floor((2 dx k + |dy| - 1) / (2 |dy|)), ya + s k),
 *                         k = 0 .. |dy|; otherwise (xa + k, ya + s floor((2 |dy| k + dx - 1) / (2 dx))), k = 0 .. dx
 *                         (one point for dx = dy = 0); only pixels inside the raster count
 *      A restatement of OpenCV's construction: parity with cv2.fillPoly itself is unpinned (OpenCV clips a line to the
 *      image before it walks it). Integers only (int64): the words do not depend on the grid or the run. Stream-ordered,
 *      no synchronisation, no scratch. N = 0 returns 0 without a launch --------------------------------------------- */
/* vertices are accepted in |x|, |y| <= ADP_POLY_COORD_MAX (an edge with a vertex beyond it takes no part) */
#define ADP_POLY_COORD_MAX 16777216
/* words of a row that one step of the row scan covers (tests place their widths around it) */
#define ADP_POLY_SCAN_WORDS 64
/* bits (N, H, ceil(W / 64)) = the raster of the polygons: xy (V, 2) int32 vertices (x = column, y = row; they may lie
 * outside the raster), polygon p is the cyclic run xy[poly_off[p] .. poly_off[p + 1]) (edges join consecutive vertices
 * and the last to the first; an empty run is no polygon), image n has the polygons [img_off[n], img_off[n + 1]).
 * poly_off (P + 1) and img_off (N + 1) ascend from 0 to V and to P; a vertex or a polygon that they do not bracket
 * takes no part. All four are DEVICE pointers. Fails (message, nothing launched) on a NULL pointer (with N > 0), N < 0,
 * H or W < 1, P < 0, V < 0 or V >= 2^31 */
int adp_poly_raster(int N, int H, int W, const int* xy, const int* poly_off, const int* img_off, int P, long long V,
                    unsigned long long* bits, adp_stream_t s);

/* ---- contrast-limited adaptive histogram equalisation of 8-bit gray planes (cv2.createCLAHE(clip_limit, (tx, ty))
 *      .apply: pre-post-processing_tools/preprocess_small_MS_SIMs.py:393-431 --enhance-contrast,
 *      large_wsi_to_small_wsi_MS.py:202-210 enhance_clahe, adaptive_clahe_function.py). The definition (OpenCV 4's
 *      clahe.cpp for 8-bit input, restated) is in contrast.py. A plane is (N, H, W) uint8, or float32 (src_f32 != 0)
 *      rounded to nearest and clamped to 0 .. 255 on load. The grid has ty rows of tx tiles, each 1 .. ADP_CLAHE_MAX_GRID;
 *      the image is extended by reflect-101 at the bottom and right to (He, We) -- both axes by a full ty - H % ty /
 *      tx - W % tx unless both divide evenly -- by index arithmetic; tiles are th x tw = He / ty x We / tx. All
 *      stream-ordered, none synchronises; integer up to the tables and single float32 operations after, so exact and
 *      independent of N, the grid and the run. Every call fails (message, nothing launched, outputs untouched) on a
 *      NULL pointer, N < 1, a grid outside 1 .. 64, or an extension beyond dim - 1 ------------------------------------ */
#define ADP_CLAHE_MAX_GRID 64
/* rows x columns of a tile that one block of adp_clahe_hist counts (tests place their shapes around them) */
#define ADP_CLAHE_SLAB_ROWS 64
#define ADP_CLAHE_SLAB_COLS 1024
/* hist (N, ty, tx, 256) uint32: the histograms of the extended image's tiles; the call zeroes it. With ty = tx = 1
 * the global histogram adp_u8_stretch reads */
int adp_clahe_hist(int N, int H, int W, const void* src, int src_f32, int ty, int tx, uint32_t* hist, adp_stream_t s);
/* lut (N, ty, tx, 256) uint8 from hist of tiles of `area` pixels: clip = max(int(clip_limit * area / 256), 1) (none
 * if clip_limit <= 0), the excess redistributed as OpenCV does, lut[i] = saturate(rint(float(cumsum[i]) * (255f / area))) */
int adp_clahe_lut(int N, int ty, int tx, int area, double clip_limit, const uint32_t* hist, uint8_t* lut, adp_stream_t s);
/* dst (N, H, W) = the bilinear blend of the four neighbouring tiles' tables at src's value; uint8, or float32
 * (dst_f32 != 0) holding the same integers. lut must be 16-byte aligned */
int adp_clahe_apply(int N, int H, int W, const void* src, int src_f32, int ty, int tx, const uint8_t* lut, void* dst,
                    int dst_f32, adp_stream_t s);
/* sums (N, 5) int64 {sum g, sum g^2, sum lap, sum lap^2, H * W}; lap = g(y-1,x) + g(y+1,x) + g(y,x-1) + g(y,x+1) -
 * 4 g(y,x) with reflect-101 borders (cv2.Laplacian, ksize 1). H and W at least 2. The call zeroes sums */
int adp_gray_stats(int N, int H, int W, const void* src, int src_f32, long long* sums, adp_stream_t s);
/* dst (N, n_px) f32 = clip((src - lo) / den, 0, 1) per image; lo / hi are the image's p_low / p_high percentiles
 * (numpy's "linear" method, float64, found on the device from hist (N, 256), the image's histogram as adp_clahe_hist
 * writes it on a 1 x 1 grid); den = (hi - lo) + 1e-3 (mode 0) or max(hi - lo, 1e-3) (mode 1); float64 arithmetic,
 * rounded to float32 once */
int adp_u8_stretch(int N, size_t n_px, const uint8_t* src, const uint32_t* hist, double p_low, double p_high, int mode,
                   float* dst, adp_stream_t s);

/* ---- gray-scale (flat) morphology of 8-bit planes and the background corrections built on it
 *      (pre-post-processing_tools/preprocess_small_MS_SIMs.py:217-246 remove_banding_morphological, 293-326
 *      correct_illumination_rolling_ball, 357-390 correct_illumination_tophat). The definitions are in illumination.py.
 *      A plane is (N, H, W) uint8, or float32 (the _f32 flag != 0) rounded to nearest and clamped to 0 .. 255 on load.
 *      All stream-ordered, none synchronises; integers and single exact float32 operations, so exact and independent of
 *      N, the grid and the run. N = 0 returns 0 without a launch. Every call fails (message, nothing launched, outputs
 *      untouched) on a NULL pointer, N < 0, H or W < 1, or an output that overlaps an input -------------------------- */
#define ADP_GMORPH_ERODE 0
#define ADP_GMORPH_DILATE 1
#define ADP_GMORPH_KMAX 513 /* rows and box width of a footprint: the reference's 512 x 1 line, 301 ellipse, 401 disc */
/* pixels a block of adp_gray_morph produces (tests place their shapes around them) */
#define ADP_GMORPH_TILE_ROWS 64
#define ADP_GMORPH_TILE_COLS 256
/* dst (N, H, W) uint8 = erosion (ADP_GMORPH_ERODE) or dilation (ADP_GMORPH_DILATE) of src by the footprint of kh rows of
 * column extents [row_lo[a], row_hi[a]) (HOST arrays) in a box kw wide, anchor (kh / 2, kw / 2):
 *   erode(M)(y, x)  = min over rows a, row_lo[a] <= b < row_hi[a], of M(y + a - kh/2, x + b - kw/2)
 *   dilate(M)(y, x) = max over the same offsets (not the reflected ones)
 * positions outside the image take no part (OpenCV's default morphology border); an empty footprint erodes to 255 and
 * dilates to 0; a footprint may be larger than the image. 1 <= kh, kw <= ADP_GMORPH_KMAX. Also fails on a size out of
 * range, a row with row_lo < 0, row_hi > kw or row_lo > row_hi, or an unknown op */
int adp_gray_morph(int N, int H, int W, const void* src, int src_f32, uint8_t* dst, int kh, int kw, const int* row_lo,
                   const int* row_hi, int op, adp_stream_t s);
/* sums (N) int64 = the sum of every image of the uint8 plane src (integer atomics: exact in any order). H * W < 2^31,
 * N <= 65535. The call zeroes sums */
int adp_gray_bgsum(int N, int H, int W, const uint8_t* src, long long* sums, adp_stream_t s);
#define ADP_ILLUM_SUBTRACT_MEAN 0 /* dst = trunc(clip(float(v - b) + mean32, 0, 255)), mean32 = float(double(sums[n]) / double(H * W)) */
#define ADP_ILLUM_TOPHAT_HALF 1   /* dst = trunc(clip(float(v) + float(max(v - b, 0)) * 0.5f, 0, 255)); b = open(v) */
#define ADP_ILLUM_DIFF 2          /* dst = max(v - b, 0): the white top-hat (v, open(v)) and the black one (close(v), v) */
/* the element-wise end of the corrections: v (N, H, W) uint8 or float32, b (N, H, W) uint8 (the background, or the
 * opening), sums (N) int64 as adp_gray_bgsum writes it (read on the device; may be NULL for the other two modes),
 * dst uint8 or float32 (dst_f32 != 0) holding the same integers. Also fails on an unknown mode or N > 65535 */
int adp_illum_finish(int N, int H, int W, const void* v, int v_f32, const uint8_t* b, const long long* sums, int mode,
                     void* dst, int dst_f32, adp_stream_t s);

/* ---- the statistical steps of the gray-image preparation (pre-post-processing_tools/preprocess_small_MS_SIMs.py:249-286
 *      remove_banding_column_normalize, 92-114 normalize_zscore, 117-138 normalize_percentile; definitions in
 *      normalization.py). A plane is (N, H, W) uint8, or float32 (the _f32 flag != 0) rounded to nearest and clamped to
 *      0 .. 255 on load; every image on its own. Exact integer sums, histograms and minima / maxima, then float64
 *      operations rounded one by one in the definition's order, so exact and independent of N, the grid and the run.
 *      All stream-ordered, none synchronises. N = 0 returns 0 without a launch. Every call fails (message, nothing
 *      launched, outputs untouched) on a NULL pointer, N < 0 or N > 65535, H or W < 1, H * W >= 2^31, or an output that
 *      overlaps an input ------------------------------------------------------------------------------------------- */
/* rows x columns of the plane that one block of adp_gray_colstats reduces (tests place their shapes around them) */
#define ADP_GNORM_BAND_ROWS 64
#define ADP_GNORM_BAND_COLS 256
/* a plane of more than ADP_GNORM_TALL_BLOCKS such blocks (N * bands) that takes the 16-byte path (uint8, W % 16 == 0,
 * aligned) is reduced by blocks of ADP_GNORM_TALL_FACTOR bands of rows: fewer atomics per column. The result is the same
 * integers either way */
#define ADP_GNORM_TALL_BLOCKS 1024
#define ADP_GNORM_TALL_FACTOR 4
#define ADP_GNORM_ZSCORE 0
#define ADP_GNORM_PERCENTILE 1
/* colsums (N, W, 2) int64 {S1 = sum v, S2 = sum v^2} and colminmax (N, W, 2) uint32 {min, max} of every column, in one
 * pass over the plane (integer atomics: exact in any order). The call initialises both */
int adp_gray_colstats(int N, int H, int W, const void* src, int src_f32, long long* colsums, uint32_t* colminmax,
                      adp_stream_t s);
/* from adp_gray_colstats' outputs: col (N, W, 2) float64 {cm, d}: cm = S1 / H, d = sqrt(max(S2 / H - cm * cm, 0)) + 1e-10;
 * glob (N, 4) float64 {gm, gs, lo, hi}: mean and population deviation of the image from the exact totals, and the
 * minimum of (min_x - cm_x) / d_x and maximum of (max_x - cm_x) / d_x over the columns */
int adp_gray_colparams(int N, int H, int W, const long long* colsums, const uint32_t* colminmax, double* col, double* glob,
                       adp_stream_t s);
/* dst (N, H, W) uint8 or float32 (dst_f32 != 0) = trunc(clip(t', 0, 255)), t = (v - cm_x) / d_x and
 * t' = t * gs + gm (preserve_global != 0) or ((t - lo) / ((hi - lo) + 1e-10)) * 255 */
int adp_gray_colnorm(int N, int H, int W, const void* src, int src_f32, const double* col, const double* glob,
                     int preserve_global, void* dst, int dst_f32, adp_stream_t s);
/* dst (N, n_px) uint8 or float32 = table[src] per image; the table is built on the device from hist (N, 256), the
 * image's histogram as adp_clahe_hist writes it on a 1 x 1 grid:
 *   ADP_GNORM_ZSCORE      table[i] = trunc(clip((((i - mean) / (std + 1e-10)) + 3) / 6 * 255, 0, 255))
 *   ADP_GNORM_PERCENTILE  table[i] = trunc(clip((i - lo) / max(hi - lo, 1e-3), 0, 1) * 255), lo / hi the p_low / p_high
 *                         percentiles (numpy's "linear" method, as adp_u8_stretch finds them)
 * Also fails on an unknown method, or percentiles that break 0 <= p_low <= p_high <= 100. n_px in 1 .. 2^31 - 1 */
int adp_gray_normalize(int N, size_t n_px, const void* src, int src_f32, const uint32_t* hist, int method, double p_low,
                       double p_high, void* dst, int dst_f32, adp_stream_t s);

/* ---- unsharp mask, the last step of the gray-image preparation (preprocess_small_MS_SIMs.py:434-455 sharpen_image;
 *      definition in sharpen.py). A plane is (N, H, W) uint8, or float32 (the _f32 flag != 0) rounded to nearest and
 *      clamped to 0 .. 255 on load; every image on its own. taps is a HOST pointer to the r + 1 integer taps q0 .. qr of
 *      the Gaussian (sharpen.taps), which the call checks (q0 + 2 sum qi = 2^24) and hands to the kernels by value. The
 *      blur is the exact integer S(y, x) = sum_j q|j| sum_i q|i| v(fold(y + j), fold(x + i)) <= 255 * 2^48 with
 *      BORDER_REFLECT_101 folded as often as needed (images smaller than r are legal), so exact and independent of the
 *      grid and the run. r <= ADP_SHARP_FUSED_RMAX is one launch and rowbuf may be NULL; a larger r is two launches
 *      through rowbuf, a uint32 (N, H, W) plane of row sums the caller supplies. Stream-ordered, no synchronisation.
 *      N = 0 returns 0 without a launch. Every call fails (message, nothing launched, outputs untouched) on N < 0 or
 *      N > 65535, H or W < 1, H * W >= 2^31, r outside 0 .. ADP_SHARP_RMAX, taps that do not sum to 2^24, a non-finite
 *      amount, a NULL pointer (rowbuf when it is needed), or an output or rowbuf that overlaps src or each other --- */
#define ADP_SHARP_RMAX 64
#define ADP_SHARP_FUSED_RMAX 16
/* rows x columns of the output tile one block makes (tests place their shapes around them) */
#define ADP_SHARP_TILE_ROWS 32
#define ADP_SHARP_TILE_COLS 64
/* S_out (N, H, W) int64 = S */
int adp_gray_blur(int N, int H, int W, const void* src, int src_f32, const uint32_t* taps, int r, uint32_t* rowbuf,
                  long long* S_out, adp_stream_t s);
/* dst (N, H, W) uint8 or float32 (dst_f32 != 0) = trunc(clip(t, 0, 255)), t = f64(v) + amount * (f64(v * 2^48 - S) * 2^-48)
 * in float64, each operation rounded on its own */
int adp_gray_sharpen(int N, int H, int W, const void* src, int src_f32, const uint32_t* taps, int r, double amount,
                     uint32_t* rowbuf, void* dst, int dst_f32, adp_stream_t s);

/* ---- Pillow-exact resampling of 8-bit images (pre-post-processing_tools/ECM_scaling.py:175, :184: an ECM image brought
 *      to its Pseudocolored counterpart's size with PIL.Image.resize(size, Image.LANCZOS); definition in resample.py).
 *      src is (N, H, W, C) uint8 and dst (N, Ho, Wo, C) uint8, C in 1 .. 4, channels interleaved; every image and channel
 *      on its own. The tables are HOST arrays (resample.coefficients / nearest_table make them): the call checks them,
 *      copies them into the stream's workspace and has read them when it returns. Integers only: the result does not
 *      depend on the grid, the form or the run. Stream-ordered, no device synchronisation (the first use of a stream
 *      and a larger table grow its workspace). N = 0 returns 0 without a launch. Every call fails (message, nothing
 *      launched, outputs untouched) on N < 0 or N > 65535, C outside 1 .. 4, an extent < 1, H * W * C, Ho * Wo * C or
 *      H * Wo * C >= 2^31, a NULL pointer that is needed, a table that breaks its rules below, or buffers that overlap -- */
#define ADP_RESAMPLE_KMAX 193 /* taps per output: Lanczos down to 1 / 32, bicubic 1 / 48, bilinear 1 / 96, box 1 / 192 */
/* rows x columns of the output tile one block of the fused form makes, and the bytes of LDS a block may hold: the fused
 * form runs when the most input rows a row tile spans, times ADP_RESAMPLE_TILE_COLS * C, fit them (tests place their
 * shapes around all three) */
#define ADP_RESAMPLE_TILE_ROWS 32
#define ADP_RESAMPLE_TILE_COLS 64
#define ADP_RESAMPLE_LDS_BYTES 32768
/* The convolution filters. Per axis with n inputs and m outputs: bounds [m][2] int32 {lo, cnt} and taps [m][ks] int32
 * (row i: the cnt taps of output i, read from input lo on; entries beyond cnt are not read);
 *   one pass: out = clamp((2^21 + sum_j taps[i][j] * v[lo + j]) >> 22, 0, 255) in int32, the shift arithmetic
 * The horizontal pass (xb, xk, xks; W -> Wo) runs first and makes a uint8 image, the vertical pass (yb, yk, yks;
 * H -> Ho) runs on it. An axis whose extent does not change is skipped and its tables are not read (they may be NULL);
 * with neither changed dst is a copy of src. A table must hold 0 <= lo, 0 <= cnt <= ks <= ADP_RESAMPLE_KMAX,
 * lo + cnt <= n, lo and lo + cnt never descending with i, and 2^21 + 255 sum_j |taps[i][j]| < 2^31. When both extents
 * change the call is one fused launch if the tile fits (above) and option resample_fused (adp_set_option: -1 auto,
 * 0 never, 1 whenever it fits; auto is 1) allows it, otherwise two launches through tmp, a uint8 buffer of
 * N * H * Wo * C bytes, which then must be non-NULL. dst must not overlap src; tmp, when used, neither */
int adp_resample_u8(int N, int H, int W, int C, int Ho, int Wo, const uint8_t* src, const int* xb, const int* xk, int xks,
                    const int* yb, const int* yk, int yks, uint8_t* tmp, uint8_t* dst, adp_stream_t s);
/* Nearest: dst[n][y][x][c] = src[n][yi[y]][xi[x]][c]; xi (Wo) and yi (Ho) int32 HOST arrays with every index inside
 * 0 .. W - 1 and 0 .. H - 1 */
int adp_resample_nearest_u8(int N, int H, int W, int C, int Ho, int Wo, const uint8_t* src, const int* xi, const int* yi,
                            uint8_t* dst, adp_stream_t s);

/* ---- per-tile fat counts of the tile-level "Has Fat / No Fat" evaluation (tile_classification_evaluation.py:211-226
 *      calculate_fat_percentage of the prediction, and of the ground truth after its normalisation :478-489; definition
 *      in tile_classification.py). Integers only: the result does not depend on the grid or the run. Stream-ordered, no
 *      synchronisation. N = 0 returns 0 without a launch. The call fails (message, nothing launched, out untouched) on
 *      N < 0 or N > 65535, n_px < 1 (or above 2^36), both inputs NULL, out NULL, or a cut outside 0 .. 256 --- */
/* rows x 1 pixels that one block counts (tests place their shapes around it) */
#define ADP_FAT_BLOCK_PX 32768
/* out (N, 4) uint64, zeroed by the call, per image i of n_px pixels:
 *   out[4i+0] = #(pred[i] > pred_thr)      IEEE '>' in float32: NaN on either side counts nothing
 *   out[4i+1] = max gt[i]                  (0 for gt == NULL)
 *   out[4i+2] = #(gt[i] >= cut_raw)        cut_* in 0 .. 256 (256: nothing counts)
 *   out[4i+3] = #(gt[i] >= cut_scaled)
 * pred (N, n_px) float32 or NULL, gt (N, n_px) uint8 or NULL, not both NULL; columns of a NULL input stay 0. */
int adp_fat_counts(int N, size_t n_px, const float* pred, float pred_thr, const uint8_t* gt, int cut_raw,
                   int cut_scaled, unsigned long long* out, adp_stream_t s);

/* ---- optimizer (Keras Adam / AdamW, :800-806) --------------------------------------------- */
int adp_adam(size_t n, float* param, const float* grad, float* m, float* v, float lr, float beta1,
             float beta2, float eps, int step, float weight_decay, float grad_scale, adp_stream_t s);
int adp_ema(size_t n, float* ema, const float* param, float decay, adp_stream_t s);

/* ---- input / inference plumbing (predict_single :153-158, TTA :181-229, SW/blend
 *      full_evaluation_enhanced.py:115-329) ------------------------------------------------- */
/* dst[n, y, x, c] = (src_view(view)[n, y, x, c] - mean) / (std + 1e-10); src f32 rows of Cin
 * interleaved channels with a row stride of src_row_stride pixels and an image stride of
 * src_img_stride floats (<= 0: dense), so a sliding-window tile is read in place from the full
 * image; dst NHWC with C_stride >= Cin (pad channels zeroed); view 0..7 = TTA forward transform. */
int adp_prep_input(int dtype, int N, int H, int W, int Cin, const float* src,
                   long long src_row_stride, long long src_img_stride, float mean, float std,
                   int view, int C_stride, void* dst, adp_stream_t s);
/* out[y,x] = mean_v inverse_view(v)(probs[v])[y,x] over nviews views listed in views[] (host) */
int adp_tta_merge(int H, int W, int nviews, const int* views, const float* probs, float* out,
                  adp_stream_t s);
int adp_blend_accum(int H, int W, int T, int y0, int x0, const float* tile, const float* weight,
                    float* acc, float* wsum, adp_stream_t s);
int adp_blend_finalize(size_t n, const float* acc, const float* wsum, float floor_, float* out,
                       adp_stream_t s);

/* ROC AUC and average precision of a probability map against a mask (full_evaluation_enhanced.py:847-888:
 * roc_auc_score / average_precision_score on the flattened pixels, truth > 0.5 positive; ties grouped by
 * identical score). out: device f64[2] = {roc_auc, pr_auc}, NaN when only one class is present. */
int adp_auc_metrics(size_t n, const float* pred, const float* truth, double* out, adp_stream_t s);
/* scipy.ndimage.distance_transform_edt(~(src > thr), sampling=(sy, sx)): dist (device f64 H x W) = Euclidean
 * distance to the nearest pixel with src > thr (inf if there is none). Exact (separable lower envelope). */
int adp_distance_transform(int H, int W, const float* src, float thr, double sy, double sx, double* dist,
                           adp_stream_t s);
/* calculate_boundary_metrics (full_evaluation_enhanced.py:788-844) on the GPU: out (HOST f64[2]) =
 * {hausdorff95, assd}; 0 / 0 for two empty masks, inf for one empty mask or an empty surface. The
 * reference's pairing is kept (each distance map is sampled at its own mask's surface). Synchronises s. */
int adp_boundary_metrics(int H, int W, const float* pred, const float* truth, float thr, double sy, double sx,
                         double* out, adp_stream_t s);

/* BoundaryRefiner.refine (full_evaluation_enhanced.py:357-393) of one (H, W) f32 probability map: m = u8(mask*255),
 * ellipse (ksize; row_lo / row_hi = HOST arrays of ksize column extents, getStructuringElement(MORPH_ELLIPSE))
 * erode / dilate -> band = dilated>0 xor eroded>0, bilateral filter (d, sigma_color, sigma_space;
 * cv2.bilateralFilter semantics, BORDER_REFLECT_101) inside the band, MORPH_OPEN then MORPH_CLOSE, out = f32(x / 255).
 * work: >= 4*H*W bytes. ksize <= 31, d / 2 <= 15. */
int adp_boundary_refine(int H, int W, const float* mask, int ksize, const int* row_lo, const int* row_hi, int d,
                        float sigma_color, float sigma_space, void* work, float* out, adp_stream_t s);

/* ---- handle-level engine: native adipose_v3 inference for non-Python callers ---- */
#define ADP_PRESET_ADIPOSE_V3 0 /* AdiposeUNetV3.build_model (train_adipose_unet_v3.py:660-758) */
#define ADP_PRESET_UNET_BN 1    /* BASELINE.json configs 2/3/5: L levels, base width, [conv3x3 -> BatchNorm -> ReLU] x 2,
                                   MaxPool 2x2, ConvTranspose 2x2/s2 + skip concat, 1x1 sigmoid head (no reference
                                   code; the Python schedule is nets.UNetBN) */
typedef struct adp_handle adp_handle; /* opaque: topology, packed weights, activation buffers */
typedef struct adp_config {
  int preset;            /* ADP_PRESET_ADIPOSE_V3 or ADP_PRESET_UNET_BN */
  int tile;              /* S (the reference hard-codes 1024), multiple of 8 (unet_bn: of 2^(levels-1)) */
  int max_batch;         /* images x TTA views per forward (activation buffers are sized for it) */
  int dtype;             /* ADP_DTYPE_F32 (the reference's fp32 numerics) or ADP_DTYPE_BF16 */
  int deep_supervision;  /* adipose_v3: 1 = the aux_out1 / aux_out2 heads exist (checkpoint layout); inference = main_out */
  int init_nb;           /* adipose_v3 base width, 44 (build_model(init_nb=44)) */
  /* v12 */
  int levels;            /* unet_bn: resolution levels (0 -> 5; configs[2] = 5, configs[1] = 4) */
  int base;              /* unet_bn: level-0 width (0 -> 64) */
  int in_ch;             /* unet_bn: input channels (0 -> 3), tiles (S, S, in_ch) interleaved f32 */
  float dropout_rate;    /* adipose_v3: build_model(dropout_rate) (0.3), used by adp_train_step when its cfg's
                            dropout_rate < 0; unet_bn has no dropout layers (ignored) */
  unsigned seed;         /* dropout mask stream: step k uses hash seed (seed + k) * 7919 + 17 (0 = the Python
                            Trainer's stream) */
} adp_config;
int adp_create(const adp_config* cfg, int device, adp_handle** out);
int adp_destroy(adp_handle* h);
/* i-th parameterised layer name (Keras layer names), NULL past the end */
const char* adp_param_name(const adp_handle* h, int i);
/* adipose_v3: slot 0 = kernel (Keras HWIO for convs, (1,1,Cin,Nout) for heads), 1 = bias. unet_bn: conv layers
 * (enc*_conv*, dec*_conv*) 0 = kernel HWIO, 1 = gamma, 2 = beta, 3 = moving mean, 4 = moving variance;
 * ConvTranspose dec*_up 0 = kernel (Cin, Cout, 2, 2), 1 = bias; head 0 = kernel (1,1,Cin,1), 1 = bias.
 * n = element count. unet_bn parameter I/O is synchronous (the device is synchronised first). */
int adp_param_size(adp_handle* h, const char* layer, int slot, size_t* n);
int adp_set_param(adp_handle* h, const char* layer, int slot, const float* host, size_t n);
int adp_get_param(adp_handle* h, const char* layer, int slot, float* host, size_t n);
/* The gradient of a parameter slot from the last adp_train_step (after its all-reduce), same layout as
 * adp_get_param; synchronous. Errors before the first step and for the running-statistics slots. */
int adp_get_grad(adp_handle* h, const char* layer, int slot, float* host, size_t n);
/* Test hook of the bucketed all-reduce (v16): which = 0 copies the whole flat gradient buffer of the last
 * adp_train_step (n = its element count, adp_debug_grad_flat(h, 0, NULL, 0) -> error message names it);
 * which = 1 copies the snapshot taken on the communication stream as each bucket's all-reduce was issued,
 * recorded only while option "dp_snapshot" is 1. With a one-rank communicator (the in-place SUM changes
 * nothing) the two are equal iff no gradient was written after its bucket started. Synchronous. */
int adp_debug_grad_flat(adp_handle* h, int which, float* host, size_t n);
/* predict_single / TTA (segmentation_inference.py:153-229): images = n device f32 (S,S) raw gray tiles
 * img_stride floats apart (<= 0: dense); prob = n device f32 (S,S) main_out probabilities;
 * (x - mean)/(std + 1e-10) on load; tta_mode 0 none, 1 minimal (id, flipH), 2 basic (+flipV, rot90),
 * 3 full (8 views). Stream-ordered; the first call after adp_set_param uploads the weights
 * (synchronous). One handle per device and thread. */
int adp_forward(adp_handle* h, const float* images, int n, long long img_stride, float mean, float std,
                int tta_mode, float* prob, adp_stream_t s);

/* unet_bn: images are n device f32 (S, S, in_ch) interleaved tiles (img_stride floats apart, <= 0: dense);
 * BatchNorm uses the running statistics (eval). */
/* One training step of AdiposeUNetV3 (model.net.fit, train_adipose_unet_v3.py:1316-1324) on the handle:
 * forward with dropout -> main / deep-supervision losses and their gradients (compile_model :780-879:
 * OHEM or BCE+Dice main head, BCE+Dice aux heads, label smoothing :244-279, weights 1.0 / 0.4 / 0.3) ->
 * backward -> [SUM all-reduce of the gradients over the communicator of adp_set_comm] -> Adam / AdamW
 * (Keras 2.13 update, :800-806). Frozen encoder (freeze_encoder_layers :760-772): no encoder
 * gradients or updates. x: n device f32 (S,S) normalised images, y: n device f32 (S,S) labels in {0,1};
 * n <= max_batch. metrics (host, 6 floats, the call synchronises the stream): loss, main_out_loss,
 * aux_out1_loss, aux_out2_loss, main_out_dice_coef, main_out_binary_accuracy (Keras' per-batch values;
 * with a communicator: of the global batch). The first call allocates the optimizer state (m, v = 0).
 * With a communicator the gradients are SUM-all-reduced in ~16 MB buckets on a communication stream, each as
 * soon as the backward has produced all of its layers (overlapping the remaining backward launches).
 * unet_bn: x is n (S, S, in_ch) f32 normalised tiles; the loss is the main head's (OHEM or BCE + Dice per
 * use_hard_mining, label smoothing), BatchNorm uses batch statistics and updates the running ones
 * (momentum 0.1, eps 1e-5); freeze_encoder must be 0. */
typedef struct adp_train_cfg {
  int use_hard_mining;       /* OHEM main loss (--use-hard-mining, default on) */
  float hard_example_ratio;  /* 0.7 */
  int use_label_smoothing;
  float epsilon_pos, epsilon_neg;          /* 0.03, 0.07 */
  float w_main, w_aux1, w_aux2;            /* 1.0, 0.4, 0.3 */
  int optimizer;             /* 0 Adam, 1 AdamW (weight_decay) */
  float beta1, beta2, eps, weight_decay;   /* 0.9, 0.999, 1e-7, 0.01 */
  float dropout_rate;        /* 0.3 (build_model dropout_rate) */
  int freeze_encoder;        /* phase 1 */
} adp_train_cfg;
int adp_train_step(adp_handle* h, const float* x, const float* y, int n, const adp_train_cfg* cfg, float lr,
                   float* metrics, adp_stream_t s);
/* Data-parallel training: comm is an RCCL ncclComm_t (one rank per GPU); NULL detaches. RCCL is loaded
 * at run time (librccl.so.1). The helpers create a communicator without another framework:
 * adp_comm_unique_id fills 128 bytes on one rank, which every rank passes to adp_comm_init. */
int adp_set_comm(adp_handle* h, void* comm);
int adp_comm_unique_id(void* id128);
int adp_comm_init(int nranks, const void* id128, int rank, void** comm);
int adp_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif
