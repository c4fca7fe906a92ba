/*
 * mau_hip.h -- C ABI of libmau_hip.so: the MI355X (gfx950) hot path of the
 * Metadata-Augmented U-Net (forward + backward of src/model.py as driven by
 * src/train.py:243-256 in the reference repository).
 *
 * Boundary rules:
 *   - plain pointers and sizes only, no torch / C++ types;
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (the caller passes its current stream);
 *   - no hidden allocation, no retained pointers: every workspace is an argument;
 *   - re-entrant per stream; safe to capture into a hipGraph (no sync, no malloc);
 *   - return value: 0 = ok, non-zero = error (message via mau_last_error()).
 *
 * Internal activation layout ("NHWC-ld"): element (n, y, x, c) of a tensor lives at
 *   base + ((n*H + y)*W + x)*ld + c,   ld % 8 == 0,  ld >= C,
 * and channels [C, roundup(C,8)) are always zero.  `dtype` selects the arithmetic type of
 * activations and packed weights: MAU_F32 (parity mode, exact fp32 MFMA),
 * MAU_BF16 (throughput mode, bf16 MFMA with fp32 accumulation) or MAU_F16 (the same kernels on
 * fp16 operands: 3 more mantissa bits, no loss scaling -- meant for inference).  Parameters,
 * gradients of parameters, BatchNorm statistics and the model's external
 * inputs/outputs are always fp32 in the reference's own layouts (NCHW, OIHW).
 *
 * Each entry point names the reference code it replaces (file:line in the
 * reference repo).  The rank tests of checkpoints (mau_rank_tests) return exact
 * int64 rank sums, obtained by counting: see "statistical comparison" below.
 */
#ifndef MAU_HIP_H
#define MAU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAU_F32 0
#define MAU_BF16 1
#define MAU_F16 2     /* fp16 activations / packed weights, v_mfma_f32_32x32x16_f16, fp32 accumulation (BASELINE configs[4]) */

#define MAU_OK 0
#define MAU_ERR_ARG 1      /* bad argument (shape, alignment, dtype)      */
#define MAU_ERR_HIP 2      /* a HIP runtime call / kernel launch failed   */
#define MAU_ERR_DEVICE 3   /* no gfx950 device                             */

typedef void* mau_stream_t;

/* ---- library ---------------------------------------------------------- */
#define MAU_ABI_VERSION 5  /* 2: single-launch reductions (tickets), multi-tensor weight pack, fused BatchNorm passes; 3: first-layer kernels;
                            * 4: mau_set_cu_budget (an experiment, measured a loss); 5: mau_set_cu_budget removed, mau_conv3x3_variant reports K groups,
                            *    mau_conv3x3_fwd_pool */
int mau_abi_version(void);
const char* mau_last_error(void);
/* 0 when the current HIP device is a gfx950 (MI355X); MAU_ERR_DEVICE otherwise. */
int mau_device_check(void);

/* ---- layout at the module boundary ------------------------------------ */
/* maps (B,C,H,W) fp32 as handed over by collate_fn (src/dataset.py:99-106) -> NHWC-ld. */
int mau_nchw_to_nhwc(const float* src, void* dst, int dtype, int N, int C, int H, int W, int ld,
                     mau_stream_t stream);
/* inverse (tests, debugging, gradient w.r.t. maps). */
int mau_nhwc_to_nchw(const void* src, float* dst, int dtype, int N, int C, int H, int W, int ld,
                     mau_stream_t stream);

/* Input pipeline (reference src/dataset.py:53-72 hands over 23 fp32 planes per tile, 18 of them the one-hot
 * expansion of two class maps, src/data/processing_10m/process.py:176-181 + normalization.py:96-100): the class maps
 * travel as uint8 (N,H,W) and the one-hot channels are generated on the device.
 * out (N,H,W,ldo) = [onehot(cls_a) num_classes | cont (N,ncont,H,W) fp32 | onehot(cls_b) num_classes | zero pad];
 * flip (N) uint8 or NULL: nonzero mirrors that tile along W (RandomFlip, src/dataset.py:134-141). ncont <= 8. */
int mau_pack_tile_onehot(const unsigned char* cls_a, const unsigned char* cls_b, const float* cont,
                         const unsigned char* flip, void* out, int ldo, int dtype, int N, int H, int W,
                         int num_classes, int ncont, mau_stream_t stream);
/* dst[n,c,y,x] = src[n,c,y, flip[n] ? W-1-x : x]: the target half of RandomFlip (src/dataset.py:139). */
int mau_flip_rows(const float* src, float* dst, const unsigned char* flip, int N, int C, int H, int W,
                  mau_stream_t stream);

/* ---- 3x3 convolution, stride 1, pad 1 (nn.Conv2d(.,.,3,padding=1), src/model.py:12,14) ---- */
/* Channel-chunk size of the packed weights for `dtype` (K-chunk of the implicit GEMM). */
int mau_conv3x3_kc(int dtype);
/* Elements (of `dtype`) of a packed weight buffer with `nout` output and `nin` input channels. */
size_t mau_conv3x3_packed_elems(int dtype, int nout, int nin);
/* OIHW fp32 weights (Cout,Cin,3,3) -> forward pack `wf` [Cin/KC][9][Cout64][KC] and/or data-gradient
 * pack `wd` [Cout/KC][9][Cin64][KC] (taps rotated by 180 degrees); either may be NULL, not both.  The packs are opaque
 * inputs of mau_conv3x3_fwd for the same dtype (MAU_BF16 permutes the rows inside every 64-row block). */
int mau_conv3x3_pack_weights(const float* w_oihw, void* wf, void* wd, int dtype, int Cout, int Cin,
                             mau_stream_t stream);
/* Every convolution of a network in ONE launch (an optimizer step changes all of them: 18 launches -> 1 in the U-Net).
 * The caller keeps a table of mau_conv3x3_pack_desc_bytes()-sized rows: it fills row `index` on the HOST with
 * mau_conv3x3_pack_desc_fill (arguments as mau_conv3x3_pack_weights; tile0 = *next_tile_host of the previous row, 0 for
 * row 0; device pointers are only recorded), copies the table to the device once, and calls
 * mau_conv3x3_pack_weights_multi(device table, rows, total tiles = the last *next_tile_host, dtype, stream). */
size_t mau_conv3x3_pack_desc_bytes(void);
int mau_conv3x3_pack_desc_fill(void* descs_host, int index, const float* w_oihw, void* wf, void* wd, int dtype, int Cout,
                               int Cin, int tile0, int* next_tile_host);
int mau_conv3x3_pack_weights_multi(const void* descs, int n, int total_tiles, int dtype, mau_stream_t stream);
/* Rows of the BatchNorm partial-statistics slab the forward launch writes for an N x H x W batch with Cout output
 * channels: one per 8x16-pixel tile for MAU_F32; one per (workgroup tile of 16x16 or 32x16 pixels, wave row) for
 * MAU_BF16 -- the tile height is chosen per layer from how well its work items fill the 256 CUs. */
int mau_conv3x3_num_pixel_tiles(int dtype, int N, int H, int W, int Cout);
/* Inference form of an ENCODER block's second convolution (reference src/model.py:18-21 in eval mode, then `self.pool`, :218,268-271):
 * y = relu(post_scale * (conv3x3(x) + bias) + post_shift) as mau_conv3x3_fwd writes it AND pooled = MaxPool2d(2,2)(y) (floor mode),
 * (N, H/2, W/2, ldpool), in one launch: the 16-bit epilogues take the window maxima from the registers they store (activations are
 * >= 0, whose 16-bit patterns order like integers); MAU_F32 runs mau_maxpool2x2_fwd behind the convolution -- the same bits as the two
 * calls either way.  One tensor source (no x1, no broadcast embedding). */
int mau_conv3x3_fwd_pool(const void* x, int ldx, int C0, const void* wpk, const float* bias, const float* post_scale,
                         const float* post_shift, void* y, int ldy, int Cout, void* pooled, int ldpool, int dtype, int N, int H,
                         int W, mau_stream_t stream);
/* Which tile variant of the convolution kernel runs such a layer (diagnostics and tests: "did the big-tile variant run?"):
 * pixel rows of a workgroup tile (16 pixels wide), waves per workgroup, output channels per workgroup -- written to HOST ints.
 * 16-bit: (64,8,64) = <64,4,8>, (32,4,64) = <64,4,4> (two workgroups per CU, level 0), (32,8,128) = <128,4,8>, (16,..) / (8,..) =
 * the small-image forms; MAU_F32: the fp32 kernel's one tiling. */
int mau_conv3x3_variant(int dtype, int N, int H, int W, int Cin, int Cout, int* tile_rows_host, int* waves_host, int* cout_block_host,
                        int* k_groups_host);
/* The network's FIRST convolution (reference src/model.py:222 / :67 conv0_0.conv1; nn.Conv2d(spatial_channels, 64, 3, padding=1),
 * src/model.py:12) for inputs of at most mau_conv3x3_first_max_channels() = 8 channels, 16-bit modes: reads the input AS THE
 * REFERENCE'S collate_fn DELIVERS IT -- x (N,Cin,H,W) fp32 contiguous (src/dataset.py:99-106) -- and the fp32 master weights
 * w (Cout,Cin,3,3) directly (no layout kernel, no weight pack); writes y (N,H,W,ldy) in `dtype` (MAU_BF16 | MAU_F16; ldy % 8 == 0,
 * channels [Cout, ldy) zero) = conv + bias, and either
 *   slab != NULL : BatchNorm partial sums from the fp32 accumulators, [rows][2 * roundup(Cout,64)] with
 *                  rows = mau_conv3x3_first_rows(N,H,W) (one row per persistent workgroup; feed it to
 *                  mau_bn_stats_finalize_train / mau_bn_stats_sums_f64 exactly like the slab of mau_conv3x3_fwd), or
 *   post_scale/post_shift != NULL : y = relu(post_scale * (conv + bias) + post_shift) (eval-mode BatchNorm + ReLU folded in).
 * x8 (optional): the input converted to `dtype` as an NHWC tensor of 8 channels (N,H,W,8), channels >= Cin zero -- what the
 * weight gradient of this layer reads (mau_conv3x3_wgrad2 with ldx = 8); written from the same pass over x. */
int mau_conv3x3_first_max_channels(void);
int mau_conv3x3_first_rows(int N, int H, int W);
/* The same layer's weight gradient (autograd's conv weight gradient of conv0_0.conv1, src/train.py:252 with src/model.py:12,222):
 * dw (Cout,Cin,3,3) fp32 = sum over pixels of dz (x) x, complete (no second call), bitwise reproducible.  x8 = the NHWC-8 copy of the
 * input written by mau_conv3x3_first_fwd; dz (N,H,W,lddz) the gradient w.r.t. the convolution's output in `dtype`; ws = workspace of
 * mau_conv3x3_first_wgrad_ws_elems(N,H,W,Cout) floats (one compact slab per persistent workgroup).  Cin <= 8, 16-bit types. */
size_t mau_conv3x3_first_wgrad_ws_elems(int N, int H, int W, int Cout);
int mau_conv3x3_first_wgrad(const void* x8, const void* dz, int lddz, float* dw_oihw, float* ws, int Cin, int Cout, int dtype, int N,
                            int H, int W, mau_stream_t stream);
/* The same weight gradient with dz formed inside the kernel (loss.backward() through conv0_0's first BatchNorm + ReLU into its
 * convolution, src/train.py:252 with src/model.py:12,19-20,222): dz = mau_bn_relu_bwd_apply(da, z, ...) is never written -- this layer's
 * input needs no gradient, so the weight gradient is dz's only reader.  da (N,H,W,ldda), z (N,H,W,ldz) in `dtype`; scale, shift, mean,
 * invstd, sums, count exactly as mau_bn_relu_bwd_apply takes them (count = 0: the count is sums[2 * Cout]).  dw has EXACTLY the bits
 * of mau_bn_relu_bwd_apply followed by mau_conv3x3_first_wgrad; same workspace.  Additive to ABI 5. */
int mau_conv3x3_first_wgrad_bn(const void* x8, const void* da, int ldda, const void* z, int ldz, const float* scale, const float* shift,
                               const float* mean, const float* invstd, const double* sums, double count, float* dw_oihw, float* ws,
                               int Cin, int Cout, int dtype, int N, int H, int W, mau_stream_t stream);
int mau_conv3x3_first_fwd(const float* x_nchw, int Cin, const float* w_oihw, const float* bias, const float* post_scale,
                          const float* post_shift, void* y, int ldy, int Cout, float* slab, void* x8, int dtype, int N, int H,
                          int W, mau_stream_t stream);
/* y = conv3x3(cat([x, broadcast(emb)], C)) + bias.
 *   x     NHWC-ld with C0 channels;
 *   emb   optional fp32 (N,E): E extra input channels, constant over (y,x) inside the image and
 *         zero in the padding halo -- fuse_embeddings (src/model.py:248-259) without ever
 *         materialising the tiled map; NULL/E=0 for ordinary convolutions;
 *   emb_ws  workspace of N*E elements of `dtype` (the embedding in the activation dtype; needed for
 *         MAU_BF16 when E > 0, ignored otherwise);
 *   wpk   forward pack for Cin = C0+E;  bias fp32 (Cout) or NULL;
 *   post_scale/post_shift  optional fp32 (Cout) pair: y = relu(post_scale*(conv+bias) + post_shift) -- eval-mode
 *         nn.BatchNorm2d + nn.ReLU (src/model.py:13-16) folded into the epilogue for the inference path
 *         (app/model_utils.py:102-109, test/evaluate.py:181-186); NULL, NULL = plain convolution;
 *   slab  optional fp32 [num_pixel_tiles][2][Cout64]: per-tile sum / sum of squares of y over the
 *         tile's valid pixels (first half of train-mode nn.BatchNorm2d, src/model.py:13,15).
 * The same entry point computes the data gradient when given dy and the `wd` pack.
 * Which channels of y a call writes (mau_conv3x3_fwd, _fwd2, _fwd_pool; MAU_F32, MAU_BF16 and MAU_F16 alike): channels [0, Cout) hold
 * the result, channels [Cout, min(roundup(Cout,64), ldy)) are written as ZERO under every epilogue (the kernels store whole 64-channel
 * blocks, clipped at ldy), channels behind that and pixels outside the tensor are untouched.  With ldy == roundup(Cout,8) these are
 * the pad lanes; with ldy > roundup(Cout,8) -- y a channel slot of a wider row buffer -- a call with Cout % 64 != 0 overwrites its
 * neighbour's first channels, which is why functional.py's out_view demands Cout % 64 == 0.  (tests/test_gpu_conv_pinned.py pins this.)
 * A source is read in whole 16-channel stages: lanes [C0, min(roundup(C0,16), ldx)) of x must hold finite values (they meet zero
 * weights: the same test pins that finite values there leave y unchanged; that a NaN there reaches y follows and is not tested);
 * with C0 % 16 == 0 nothing outside [0, C0) is read. */
int mau_conv3x3_fwd(const void* x, int ldx, int C0, const float* emb, void* emb_ws, int E, const void* wpk,
                    const float* bias, const float* post_scale, const float* post_shift, void* y, int ldy,
                    int Cout, float* slab, int dtype, int N, int H, int W, mau_stream_t stream);
/* Same with the input channels taken from TWO tensors and the broadcast vector -- torch.cat([x, x1, broadcast(emb)], 1)
 * without materialising the concatenation: the decoder's cat([skip, up(low)], 1) (src/model.py:279-282) and U-Net++'s
 * node inputs (src/model.py:136-177).  x1 (N,H,W) NHWC-ld with C1 channels, ldx1 % 8 == 0; 16-bit dtypes only,
 * C0 % 16 == 0 (a 16-channel stage reads one tensor); C1 = 0 / x1 = NULL reduces to mau_conv3x3_fwd. */
int mau_conv3x3_fwd2(const void* x, int ldx, int C0, const void* x1, int ldx1, int C1, const float* emb, void* emb_ws,
                     int E, const void* wpk, const float* bias, const float* post_scale, const float* post_shift,
                     void* y, int ldy, int Cout, float* slab, int dtype, int N, int H, int W, mau_stream_t stream);
/* Weight gradient  dW = x (*) dy  reduced over all pixels, in two steps:
 *   mau_conv3x3_wgrad        -> acc: fp32 split-K partial slabs [nsplit][9][Cout64][Cin64], plain stores, every dtype
 *                               (nsplit = mau_conv3x3_wgrad_splits(...))
 *   mau_conv3x3_unpack_wgrad -> sums the splits in fixed order and writes OIHW fp32 (Cout,Cin,3,3).
 * x is the convolution's input (with the optional broadcast `emb` / `emb_ws` as in mau_conv3x3_fwd). */
int mau_conv3x3_wgrad_splits(int dtype, int N, int H, int W, int Cout, int Cin);
size_t mau_conv3x3_wgrad_acc_elems(int dtype, int N, int H, int W, int Cout, int Cin);
int mau_conv3x3_wgrad(const void* x, int ldx, int C0, const float* emb, void* emb_ws, int E, const void* dy,
                      int lddy, int Cout, float* acc, int dtype, int N, int H, int W, mau_stream_t stream);
/* weight gradient w.r.t. the two-tensor input of mau_conv3x3_fwd2 (Cin = C0 + C1 + E; C0 % 8 == 0). */
int mau_conv3x3_wgrad2(const void* x, int ldx, int C0, const void* x1, int ldx1, int C1, const float* emb, void* emb_ws,
                       int E, const void* dy, int lddy, int Cout, float* acc, int dtype, int N, int H, int W,
                       mau_stream_t stream);
int mau_conv3x3_unpack_wgrad(const float* acc, int nsplit, float* dw_oihw, int Cout, int Cin,
                             mau_stream_t stream);

/* ---- BatchNorm2d (+ReLU) (src/model.py:13,15,16) ------------------------ */
/* slab [rows][M] fp32 -> sums[M] fp64: column sums in two deterministic levels; `ws` is an fp64
 * workspace of mau_reduce_rows_ws_elems(rows, M) elements (NULL = single level, slow for many rows).
 * `tickets`: NULL = the two levels are two launches; else a ZEROED uint32 buffer of mau_reduce_tickets_elems() entries
 * (zero again when the call's work has finished; not to be shared by calls running concurrently on two streams): the two
 * levels are ONE launch -- the workgroup that draws a column block's last ticket adds that block's partials, in the same
 * fixed order as the two-launch form (bit-identical results). */
size_t mau_reduce_rows_ws_elems(int rows, int M);
int mau_reduce_tickets_elems(void);
int mau_reduce_rows_f64(const float* slab, int rows, int M, int ldrow, double* sums, double* ws, unsigned* tickets,
                        mau_stream_t stream);
/* same, and additionally the sums rounded to fp32 in `sums32` (the BatchNorm weight/bias gradients that autograd
 * returns, next to the fp64 sums the backward formula uses).  append > 0 (single-launch form only): sums[M] = append --
 * the local pixel count that is all-reduced together with the sums under data parallelism. */
int mau_reduce_rows_f64_f32(const float* slab, int rows, int M, int ldrow, double* sums, float* sums32,
                            double* ws, unsigned* tickets, double append, mau_stream_t stream);
/* same, result rounded to fp32. */
int mau_reduce_rows_f32(const float* slab, int rows, int M, int ldrow, float* out, double* ws, unsigned* tickets,
                        mau_stream_t stream);
/* Data-parallel forward: the statistics slab of mau_conv3x3_fwd [rows][2*Cout64] -> sums = [sum(y) (C) | sum(y^2) (C)]
 * (+ sums[2*C] = append when append > 0), one launch; ws: mau_reduce_rows_ws_elems(rows, 2*C) fp64 elements. */
int mau_bn_stats_sums_f64(const float* slab, int rows, int C, double* sums, double* ws, unsigned* tickets, double append,
                          mau_stream_t stream);
/* Train mode: sums = [sum(y) | sum(y^2)] (2*C fp64, already all-reduced over ranks when data
 * parallel), count = number of pixels summed.  Writes scale = gamma*invstd, shift = beta - mean*scale,
 * mean, invstd and updates running_mean / running_var (unbiased) / num_batches_tracked exactly as
 * nn.BatchNorm2d(momentum, eps).forward does in training.
 * count == 0: `sums` has 2*C + 1 elements and sums[2*C] is the pixel count (all-reduced together with the sums, so that
 * ranks with different local batch sizes still agree on the global statistics). */
int mau_bn_finalize_train(const double* sums, double count, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, int64_t* num_batches_tracked,
                          float momentum, float eps, float* scale, float* shift, float* mean,
                          float* invstd, int C, mau_stream_t stream);
/* Single-GPU training shortcut: conv slab [rows][2*Cout64] -> (fp64 partials in `ws`,
 * mau_bn_stats_ws_elems(rows, C) elements) -> the outputs of mau_bn_finalize_train; one launch with `tickets` (see
 * mau_reduce_rows_f64), two launches with tickets == NULL. */
size_t mau_bn_stats_ws_elems(int rows, int C);
int mau_bn_stats_finalize_train(const float* slab, int rows, double count, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                float momentum, float eps, float* scale, float* shift, float* mean, float* invstd,
                                double* ws, unsigned* tickets, int C, mau_stream_t stream);
/* Eval mode: scale/shift from the running statistics (mean/invstd outputs optional, may be NULL). */
int mau_bn_coeffs_eval(const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* scale, float* shift, float* mean,
                       float* invstd, int C, mau_stream_t stream);
/* a = relu(scale*y + shift) on NHWC-ld (pad channels written as 0). */
int mau_bn_relu_apply(const void* y, int ldy, const float* scale, const float* shift, void* a, int lda,
                      int dtype, int64_t npix, int C, mau_stream_t stream);
/* a = relu(scale*y + shift) AND pooled (N,H/2,W/2) = nn.MaxPool2d(2,2)(a) in ONE pass over y: an encoder block's
 * output feeds the next level through the pool and the decoder through the skip (src/model.py:268-271). */
/* argidx (optional, NULL to skip) [N][H/2][W/2][roundup(C,8)/8] uint16: per pooled window and 8-channel vector, 2 bits per
 * channel = position 2*dy + dx of the window's first maximum (ATen's scan order, strict '>'): the pool's backward routing,
 * consumed by mau_pool_bn_bwd_reduce / _apply. */
int mau_bn_relu_apply_pool(const void* y, int ldy, const float* scale, const float* shift, void* a, int lda,
                           void* pooled, int ldp, unsigned short* argidx, int dtype, int N, int H, int W, int C,
                           mau_stream_t stream);
/* Backward, pass 1: dz = da * [scale*y+shift > 0]; per-block partial sums of dz and dz*xhat
 * (xhat = (y-mean)*invstd) into slab [rows][2][ldslab]; returns rows via *rows_out (host). */
int mau_bn_relu_bwd_reduce(const void* da, int ldda, const void* y, int ldy, const float* scale,
                           const float* shift, const float* mean, const float* invstd, float* slab,
                           int ldslab, int dtype, int64_t npix, int C, mau_stream_t stream);
/* Backward, pass 2: dy = scale*(dz - s1/count - xhat*s2/count); sums = [s1 | s2] fp64 (2*C);
 * count == 0: the count is sums[2*C] (see mau_bn_finalize_train). */
int mau_bn_relu_bwd_apply(const void* da, int ldda, const void* y, int ldy, const float* scale,
                          const float* shift, const float* mean, const float* invstd, const double* sums,
                          double count, void* dy, int lddy, int dtype, int64_t npix, int C,
                          mau_stream_t stream);
int mau_bn_bwd_rows(int64_t npix);

/* ---- BatchNorm2d + ReLU fused with the streaming operator behind it (csrc/bn_fused.hip) ----
 * An encoder block's output feeds nn.MaxPool2d(2,2) AND a skip connection (src/model.py:268-271 / :279-282).  Backward of its
 * second BatchNorm without ever writing the incoming gradient da = dskip + maxpool_backward(dpl): both passes recompute it
 * (the arg-max from `argidx`, written by mau_bn_relu_apply_pool in the forward pass).  dpl (N,H/2,W/2) [with argidx] or
 * dskip (N,H,W) may be NULL, not both.  slab / sums / count as mau_bn_relu_bwd_reduce / _apply; bit-identical to
 * mau_maxpool2x2_bwd_add + mau_bn_relu_bwd_reduce + mau_bn_relu_bwd_apply. */
int mau_pool_bn_bwd_reduce(const void* y, int ldy, const void* dpl, int lddpl, const unsigned short* argidx,
                           const void* dskip, int lddskip,
                           const float* scale, const float* shift, const float* mean, const float* invstd, float* slab,
                           int ldslab, int dtype, int N, int H, int W, int C, mau_stream_t stream);
int mau_pool_bn_bwd_apply(const void* y, int ldy, const void* dpl, int lddpl, const unsigned short* argidx,
                          const void* dskip, int lddskip,
                          const float* scale, const float* shift, const float* mean, const float* invstd,
                          const double* sums, double count, void* dy, int lddy, int dtype, int N, int H, int W, int C,
                          mau_stream_t stream);
/* The final 1x1 conv + tanh (src/model.py:241,284-292) directly behind the last block's second BatchNorm (C <=
 * mau_head_bn_max_channels()): out = head(relu(scale*y + shift)) from the RAW conv output y -- the activation is never
 * written; backward in two passes over y: (1) BatchNorm partial sums (slab as mau_bn_relu_bwd_reduce) + the head's dW / db
 * partials (head_slab as mau_head_bwd), (2) dy of the conv; da = W^T dz is recomputed from dout both times.  Bit-identical
 * to mau_bn_relu_apply + mau_head_fwd / mau_head_bwd + mau_bn_relu_bwd_reduce + mau_bn_relu_bwd_apply.
 * Images of at least 32 pixels (HW >= 32) and N * HW < 2^31: a thread walks pixels in steps of 32 with one conditional wrap into
 * the next image (smaller images: the separate kernels). */
int mau_head_bn_max_channels(void);
int mau_head_bn_fwd(const void* y, int ldy, const float* scale, const float* shift, const float* w, const float* b, float* out,
                    int tanh0, int dtype, int N, int HW, int C, int Co, mau_stream_t stream);
int mau_head_bn_bwd_reduce(const void* y, int ldy, const float* scale, const float* shift, const float* mean,
                           const float* invstd, const float* w, const float* out, const float* dout, float* bn_slab,
                           int ldslab, float* head_slab, int tanh0, int dtype, int N, int HW, int C, int Co,
                           mau_stream_t stream);
int mau_head_bn_bwd_apply(const void* y, int ldy, const float* scale, const float* shift, const float* mean,
                          const float* invstd, const double* sums, double count, const float* w, const float* out,
                          const float* dout, void* dy, int lddy, int tanh0, int dtype, int N, int HW, int C, int Co,
                          mau_stream_t stream);

/* dst = srcs[0] + srcs[1] + ... + srcs[k-1] (k <= mau_sum_tensors_max() NHWC-ld tensors of C channels, pixel pitches lds[i]; HOST
 * arrays of k device pointers / pitches): the sum autograd forms when an activation has several readers (the row slots of the U-Net++,
 * src/model.py:136-177), in one pass -- fp32 sums in the order given, one rounding. */
int mau_sum_tensors_max(void);
int mau_sum_tensors(const void* const* srcs, const int* lds, int k, void* dst, int lddst, int dtype, int64_t npix, int C,
                    mau_stream_t stream);

/* ---- the broadcast embedding of a convolution as a rank-one term (csrc/embfold.hip) ----
 * fuse_embeddings / the U-Net++ nodes' emb_map (src/model.py:248-259, :111-121) put E spatially constant channels behind the tensors a
 * 3x3 conv reads.  W_eff = [ W[:, :Ct] | T ], T[co][i][tap] = sum_e W[co][Ct+e][tap] * emb[i][e]  (Cout x (Ct+Ep) x 3 x 3, Ep >= N,
 * columns i >= N zero): the same convolution over Ct tensor channels + the N x Ep IDENTITY as "embedding" gives the same output with
 * Ct + Ep instead of Ct + E input channels.  bwd: dW (Cout x (Ct+E) x 3 x 3) and demb (N x E) from dW_eff (either may be NULL).
 * fp32, fixed summation order. */
int mau_emb_fold_fwd(const float* w, const float* emb, float* weff, int Cout, int Ct, int E, int N, int Ep, mau_stream_t stream);
size_t mau_emb_fold_ws_elems(int Cout, int N, int E);   /* floats of ws (needed when demb is asked for) */
int mau_emb_fold_bwd(const float* w, const float* emb, const float* dweff, float* dw, float* demb, float* ws, int Cout, int Ct, int E,
                     int N, int Ep, mau_stream_t stream);

/* ---- MaxPool2d(2,2) (src/model.py:57,218) -------------------------------- */
int mau_maxpool2x2_fwd(const void* x, int ldx, void* y, int ldy, int dtype, int N, int H, int W, int C,
                       mau_stream_t stream);
/* dx (N,H,W) = scatter of dy (N,H/2,W/2) to the first maximum of each window; rest zero. */
int mau_maxpool2x2_bwd(const void* x, int ldx, const void* dy, int lddy, void* dx, int lddx, int dtype,
                       int N, int H, int W, int C, mau_stream_t stream);
/* dx = dskip + maxpool2x2 backward: x feeds the pool AND a skip connection (src/model.py:268-271 / :279-282); the two
 * gradients autograd would add in a separate pass are combined while dx is written. */
int mau_maxpool2x2_bwd_add(const void* x, int ldx, const void* dy, int lddy, const void* dskip, int lddskip, void* dx,
                           int lddx, int dtype, int N, int H, int W, int C, mau_stream_t stream);

/* ---- bilinear resize, align_corners=True (src/model.py:111-121,219,243-246) ---- */
/* dst[..., choff:choff+C] = resize(src (N,h,w,C)) to (H,W); other channels of dst untouched. */
int mau_resize_bilinear_fwd(const void* src, int ldsrc, int h, int w, void* dst, int lddst, int choff,
                            int dtype, int N, int H, int W, int C, mau_stream_t stream);
/* The same upsampling (h <= H, w <= W) reading the RAW conv output y of a block whose BatchNorm + ReLU has this resize as its
 * only consumer (the U-Net's bottleneck and decoder blocks, src/model.py:279-282): relu(scale*y + shift), rounded to `dtype`,
 * is formed on the four corners in registers; bit-identical to mau_bn_relu_apply + mau_resize_bilinear_fwd. */
int mau_resize_bilinear_bn_fwd(const void* y, int ldy, int h, int w, const float* scale, const float* shift, void* dst,
                               int lddst, int choff, int dtype, int N, int H, int W, int C, mau_stream_t stream);
/* dsrc (N,h,w,C) = adjoint of the above applied to ddst[..., choff:choff+C] (gather form, no atomics). */
int mau_resize_bilinear_bwd(const void* ddst, int ldddst, int choff, int H, int W, void* dsrc, int lddsrc,
                            int dtype, int N, int h, int w, int C, mau_stream_t stream);
/* Which kernels such a resize runs (host-only query, no launch; diagnostics and tests: "did this shape reach the path it is meant
 * to?"), written to HOST ints, any of which may be NULL.  The launchers above read the same plan.
 * fwd_kernel: MAU_RESIZE_FWD_ROWCOL (h <= H, w <= W and at most 3 destination columns per source column, whatever the height ratio,
 * h = 1 included: a column of fwd_rows source cells per thread), MAU_RESIZE_FWD_CELL (any other h <= H, w <= W: one source cell per
 * thread), MAU_RESIZE_FWD_DEST (h > H or w > W: one destination pixel per thread).  fwd_rows: source rows per workgroup (8, 4, 2 or 1 by how many
 * workgroups the launch has; 1 for the other kernels).  bwd_kernel: MAU_RESIZE_BWD_2X2 (adjoint of an upsampling with h, w >= 2)
 * or MAU_RESIZE_BWD_GATHER. */
#define MAU_RESIZE_FWD_ROWCOL 0
#define MAU_RESIZE_FWD_CELL 1
#define MAU_RESIZE_FWD_DEST 2
#define MAU_RESIZE_BWD_2X2 0
#define MAU_RESIZE_BWD_GATHER 1
int mau_resize_bilinear_plan(int N, int h, int w, int H, int W, int C, int* fwd_kernel_host, int* fwd_rows_host, int* bwd_kernel_host);
/* dst[..., choff:choff+C] = src[..., :C]  (channel concat building block, src/model.py:279-282);
 * also zero-fills dst channels [choff+C, zero_to) when zero_to > choff+C. */
int mau_copy_channels(const void* src, int ldsrc, void* dst, int lddst, int choff, int zero_to, int dtype,
                      int64_t npix, int C, mau_stream_t stream);
/* dst[n, :, choff:choff+E] = emb[n] broadcast over the HW pixels (materialised form of
 * fuse_embeddings, src/model.py:248-259; the fused form is the `emb` source of mau_conv3x3_fwd). */
int mau_bcast_fill(const float* emb, void* dst, int lddst, int choff, int zero_to, int dtype, int N, int HW,
                   int E, mau_stream_t stream);
/* demb (N,E) fp32 = sum over pixels of dx[..., choff:choff+E]  (adjoint of the embedding broadcast). */
/* ws: fp32 workspace of mau_bcast_bwd_ws_elems(N, HW, E) elements (per-chunk partial sums, summed in
 * fixed order); NULL selects the slow element-granular path. */
size_t mau_bcast_bwd_ws_elems(int N, int HW, int E);
int mau_bcast_bwd(const void* dx, int lddx, int choff, float* demb, float* ws, int dtype, int N, int HW, int E,
                  mau_stream_t stream);

/* ---- head: 1x1 conv + tanh on channel 0 (src/model.py:241,284-292) -------- */
/* out (N,Co,H,W) fp32 NCHW; tanh on channel 0 iff tanh0 != 0 (the reference does so iff Co == 2). */
int mau_head_fwd(const void* a, int lda, const float* w, const float* b, float* out, int tanh0, int dtype,
                 int N, int HW, int C, int Co, mau_stream_t stream);
/* Head and per-sample spatial mean in ONE launch (the metadata-sensitivity sweeps keep only the mean of every output map):
 *   means[n][o] = scale[o] * mean over HW of head(a[n])[o] + shift[o]        (fp64, shape (N, Co))
 * Per pixel the value is the one mau_head_fwd writes, bit for bit; the (N,Co,H,W) map is never written.  scale / shift:
 * Co fp64 values each, NULL = identity, applied once to the fp64 mean.  Sums are fp64 in a fixed order: a workgroup owns
 * a run of pixels of ONE sample, the workgroup that draws the sample's last ticket adds the sample's partials in index
 * order -- a sample's result does not depend on N or on the grid and is bitwise repeatable.
 * ws: fp64 workspace of mau_head_mean_ws_elems(N, HW, Co) elements; tickets: a ZEROED mau_reduce_tickets_elems() buffer
 * (left zeroed; see mau_reduce_rows_f64).  One launch per mau_reduce_tickets_elems() samples. */
size_t mau_head_mean_ws_elems(int N, int HW, int Co);
int mau_head_mean(const void* a, int lda, const float* w, const float* b, const double* scale, const double* shift,
                  double* means, double* ws, unsigned* tickets, int tanh0, int dtype, int N, int HW, int C, int Co,
                  mau_stream_t stream);
/* da NHWC-ld = W^T dz with dz = dout * (1 - out^2 on the tanh channel); slab
 * [mau_head_bwd_rows][mau_head_bwd_rowlen] holds per-block partial sums: for output channel o,
 * row[o*(C8+8) + c] = partial dW[o][c] and row[o*(C8+8) + C8] = partial db[o]  (C8 = roundup(C,8)). */
int mau_head_bwd(const void* a, int lda, const float* w, const float* out, const float* dout, void* da,
                 int ldda, float* slab, int tanh0, int dtype, int N, int HW, int C, int Co,
                 mau_stream_t stream);
int mau_head_bwd_rows(int N, int HW);
int mau_head_bwd_rowlen(int C, int Co);

/* ---- MetadataEncoder: Linear(F,32) -> ReLU -> Linear(32,D) (src/model.py:38-48) ---- */
int mau_meta_mlp_fwd(const float* md, const float* w0, const float* b0, const float* w2, const float* b2,
                     float* hidden, float* emb, int N, int F, int Hd, int D, mau_stream_t stream);
/* dhidden_ws: fp32 workspace (N,Hd). */
int mau_meta_mlp_bwd(const float* md, const float* w0, const float* w2, const float* hidden,
                     const float* demb, float* dw0, float* db0, float* dw2, float* db2, float* dhidden_ws,
                     int N, int F, int Hd, int D, mau_stream_t stream);

/* ---- TemporalEncoder recurrence: nn.LSTM(input_size=1, hidden_size=H, batch_first=True), last hidden state
 *      (src/model.py:23-34; the sequence is 828 monthly temperatures in the reference's data, conf/config.yaml:20) ---- */
/* Largest hidden size the persistent kernels support (one gate row per thread). */
int mau_lstm_max_hidden(void);
/* x (B,T) fp32; w_ih (4H) [input_size 1], w_hh (4H,H), b_ih, b_hh (4H): torch's parameter layout, gate order i,f,g,o.
 * h_last (B,H) = h_T.  gates (B,T,4H) post-activation and cells (B,T,H), both or neither: saved for mau_lstm_bwd. */
int mau_lstm_fwd(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                 float* h_last, float* gates, float* cells, int B, int T, int H, mau_stream_t stream);
/* dh_last (B,H) -> dw_ih (4H), dw_hh (4H,H), db_ih = db_hh (4H); ws: fp32 workspace of mau_lstm_bwd_ws_elems(B,T,H)
 * elements (pre-activation gate gradients of every step + partial sums, added in a fixed order). */
size_t mau_lstm_bwd_ws_elems(int B, int T, int H);
int mau_lstm_bwd(const float* x, const float* w_hh, const float* gates, const float* cells, const float* dh_last,
                 float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, float* ws, int B, int T, int H,
                 mau_stream_t stream);

/* nn.Linear of TemporalEncoder.fc (src/model.py:27,34): out (N,D) = x (N,F) w^T + b, w (D,F) as torch stores it. */
int mau_linear_fwd(const float* x, const float* w, const float* b, float* out, int N, int F, int D, mau_stream_t stream);
/* dx (N,F) (optional, NULL to skip), dw (D,F), db (D) from dout (N,D). */
int mau_linear_bwd(const float* x, const float* w, const float* dout, float* dx, float* dw, float* db, int N, int F,
                   int D, mau_stream_t stream);

/* ---- optimizer: torch.optim.AdamW (src/train.py:213-214,255) on every 3x3 convolution weight of a network, fused with the
 *      re-pack of the updated weights (mau_conv3x3_pack_weights): ONE launch, each parameter streamed once ----
 * Table rows (mau_adamw_pack_desc_bytes() each, filled on the HOST by mau_adamw_pack_desc_fill, copied to the device by the
 * caller): w OIHW fp32 (Cout,Cin,3,3) updated in place, grad, exp_avg, exp_avg_sq of the same shape, wf / wd = the packs of
 * mau_conv3x3_pack_weights for `dtype` (both NULL: no pack); tile0 = *next_tile_host of the previous row (0 for row 0).
 * step: DEVICE float, the step count t of this update (already incremented).  p <- p(1 - lr*wd); m <- b1 m + (1-b1) g;
 * v <- b2 v + (1-b2) g^2; p <- p - lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps). */
size_t mau_adamw_pack_desc_bytes(void);
int mau_adamw_pack_desc_fill(void* descs_host, int index, float* w, const float* grad, float* exp_avg, float* exp_avg_sq,
                             void* wf, void* wd, int Cout, int Cin, int tile0, int* next_tile_host);
int mau_adamw_pack_step(const void* descs, int n, int total_tiles, int dtype, const float* step, float lr, float beta1,
                        float beta2, float eps, float weight_decay, mau_stream_t stream);

/* ---- the same launch for the reference's three optimizers (src/train.py:209-216), and gradient clipping (src/train.py:253-254)
 *      inside it.  Additive to ABI 5: mau_adamw_pack_step is mau_opt_pack_step(MAU_OPT_ADAMW, grad_scale = NULL), same bits ----
 * rule, fp32, the operation order of torch's single-tensor implementations:
 *   MAU_OPT_ADAMW  torch.optim.AdamW (src/train.py:213-214): as above.
 *   MAU_OPT_ADAM   torch.optim.Adam  (src/train.py:211-212), L2 decay: g <- g + wd p, then the moments and the step of AdamW
 *                  without the decoupled decay.
 *   MAU_OPT_SGD    torch.optim.SGD   (src/train.py:209-210), dampening 0: g <- g + wd p; buf <- momentum buf + g (a zero-filled
 *                  buffer makes the first step buf = g, torch's first-step rule); p <- p - lr (nesterov ? g + momentum buf : buf).
 *                  One state tensor: the rows' m is the momentum buffer (NULL when momentum == 0), v is NULL; step may be NULL.
 * Table rows: mau_opt_pack_desc_fill = mau_adamw_pack_desc_fill that accepts m == NULL / v == NULL (same row layout,
 * mau_adamw_pack_desc_bytes()).  grad_scale: DEVICE scalar (NULL: none) every gradient is multiplied by as it is loaded, before the
 * weight decay -- the coefficient mau_grad_norm_clip wrote; the gradients in memory are NOT rewritten. */
#define MAU_OPT_ADAMW 0
#define MAU_OPT_ADAM 1
#define MAU_OPT_SGD 2
int mau_opt_pack_desc_fill(void* descs_host, int index, float* w, const float* grad, float* m, float* v, void* wf, void* wd,
                           int Cout, int Cin, int tile0, int* next_tile_host);
int mau_opt_pack_step(const void* descs, int n, int total_tiles, int dtype, int rule, const float* step, const float* grad_scale,
                      float lr, float beta1_or_momentum, float beta2, float eps, float weight_decay, int nesterov,
                      mau_stream_t stream);

/* Global L2 norm of a set of fp32 gradients and the coefficient of torch.nn.utils.clip_grad_norm_ (src/train.py:253-254), ONE
 * launch, no host read-back: norm_out = sqrt(sum of squares) and coef_out = min(1, max_norm / (norm + 1e-6)) (clip_coef_clamped;
 * a non-finite gradient gives a non-finite norm, as torch does with error_if_nonfinite=False).  segs: DEVICE table of nsegs rows
 * (mau_grad_norm_seg_bytes() each) filled on the HOST by mau_grad_norm_seg_fill: a contiguous fp32 range (ptr, n) and block0 = the
 * first workgroup of the range = *next_block_host of the previous row (0 for row 0); total_blocks = the last row's *next_block_host.
 * A workgroup sums the squares of mau_grad_norm_chunk() consecutive floats of one range in fp64; the workgroup that draws the last
 * ticket adds the total_blocks partials in index order: the bits do not depend on the order the workgroups ran in.  ws: fp64
 * workspace of total_blocks elements; tickets: a ZEROED mau_reduce_tickets_elems() buffer (left zeroed). */
int mau_grad_norm_chunk(void);
size_t mau_grad_norm_seg_bytes(void);
int mau_grad_norm_seg_fill(void* segs_host, int index, const float* ptr, int64_t n, int block0, int* next_block_host);
int mau_grad_norm_clip(const void* segs, int nsegs, int total_blocks, double* ws, unsigned* tickets, float max_norm,
                       float* norm_out, float* coef_out, mau_stream_t stream);

/* ---- test-split evaluation metrics (test/evaluate.py:210-275), ONE launch, the maps never leave the device.  Additive to ABI 5 ----
 * out, tgt (B,C,H,W) fp32 NCHW; cls (B,H,W) uint8 class ids (the land-cover map at t1); scale / shift: C fp64 values each
 * (NULL = 1 / 0) that un-normalise a channel, p = out * scale[c] + shift[c], g = tgt * scale[c] + shift[c]; ncls in [1,16].
 * Every value is a double from its load on; products and sums are fp64, not contracted, added in a fixed order: a workgroup
 * owns a run of image rows of ONE map (mau_eval_metrics_chunks(H, W) workgroups per map, a function of H and W alone), the
 * workgroup that draws the map's last ticket adds its partials in chunk order -- a row's bits do not depend on B, on the
 * sample's place in the batch or on the device, and repeat.
 * rows: (B*C) x mau_eval_metrics_row_elems(ncls) fp64, row b*C + c =
 *   [0] mean|p-g|  [1] sqrt(mean (p-g)^2)
 *   [2],[3] population variance of the 5-point Laplacian of p, of g (x[i-1,j] + x[i+1,j] + x[i,j-1] + x[i,j+1] - 4 x[i,j], the
 *           edge sample repeated beyond the border: scipy.ndimage.laplace's default mode), E[x^2] - E[x]^2 from fp64 sums
 *   [4],[5] number of non-finite values of out, of tgt   [6],[7] min, max of p   [8],[9] min, max of g  (NaNs skipped)
 *   [10] number of pixels whose class id is >= ncls (they count toward [0..9] only)
 *   [11 + k] pixels of class k   [11 + ncls + k] mean|p-g| over them   [11 + 2 ncls + k] sqrt(mean (p-g)^2) over them;
 *           the two means of a class without pixels are NaN.
 * ws: fp64 workspace of mau_eval_metrics_ws_elems(B, C, H, W, ncls) elements; tickets: a ZEROED mau_reduce_tickets_elems()
 * buffer (left zeroed; see mau_reduce_rows_f64).  One launch per mau_reduce_tickets_elems() rows. */
int mau_eval_metrics_row_elems(int ncls);
int mau_eval_metrics_chunks(int H, int W);
size_t mau_eval_metrics_ws_elems(int B, int C, int H, int W, int ncls);
int mau_eval_metrics(const float* out, const float* tgt, const unsigned char* cls, const double* scale, const double* shift,
                     double* rows, double* ws, unsigned* tickets, int B, int C, int H, int W, int ncls, mau_stream_t stream);

/* ---- statistical comparison of M checkpoints (test/statistical_tests.py, the numbers of app_dev/pages/3_Statistical_Comparison.py):
 *      the M models' metric rows in ONE launch, their joint moments per group in ONE more.  Additive to ABI 5 ----
 * mau_eval_metrics_multi: out (M,B,C,H,W) fp32, the M models' outputs; tgt, cls, scale, shift, ncls, tickets as mau_eval_metrics;
 * M in [1, mau_eval_metrics_multi_max_models() = 8] (MAU_ERR_ARG otherwise), every other argument by mau_eval_metrics's rules.
 *   rows: (M, B*C, mau_eval_metrics_row_elems(ncls)) fp64; row [m][b*C + c] has EXACTLY the bits mau_eval_metrics gives for out[m],
 *   tgt, cls: the same chunking, per-thread pixel order and joins.  A row does not depend on M or on the model's place.
 * A workgroup owns one chunk of one (sample, channel) and walks the M models over it: the chunk's un-normalised target values,
 * their Laplacians and the class ids are formed once and kept in registers, and what depends on the target alone ([3], [5], [8],
 * [9], [10] and the class counts) is joined once and written into every model's row -- 4 M + 5 bytes per pixel and channel instead
 * of 9 M.  (A map wider than 4096 pixels has more than 16 pixels per thread: its target values are formed again per model.)
 * ws: fp64 workspace of mau_eval_metrics_multi_ws_elems(M, B, C, H, W, ncls) elements; tickets: a ZEROED
 * mau_reduce_tickets_elems() buffer (left zeroed).  One launch per mau_reduce_tickets_elems() rows. */
int mau_eval_metrics_multi_max_models(void);
size_t mau_eval_metrics_multi_ws_elems(int M, int B, int C, int H, int W, int ncls);
int mau_eval_metrics_multi(const float* out, const float* tgt, const unsigned char* cls, const double* scale, const double* shift,
                           double* rows, double* ws, unsigned* tickets, int M, int B, int C, int H, int W, int ncls,
                           mau_stream_t stream);
/* mau_paired_accumulate: merges the samples of a batch into table [G][C][4 + 2 ncls] of entries (DEVICE resident, zeroed by the caller
 * before the first batch), G = mau_paired_groups() = 8 = 4 * is_known_city + temporal distance (0 long: t1_year <= 2021, 1 mid:
 * 2022-2023, 2 short: > 2023, 3 other; statistical_tests.py:12-20).
 *   rows: (M, B*C, mau_eval_metrics_row_elems(ncls)) fp64, as mau_eval_metrics_multi writes them; M in [1,8], ncls in [1,16];
 *   group: (B) uint8 on the device, the sample's group; an id >= G drops the sample.
 * Slot s of (group, channel): s < 4 the overall metrics, row entries [0] mae, [1] rmse, [2] laplacian_var_pred, [3]
 * laplacian_var_gt; s = 4 + 2 k + w the class k's mae (w = 0, row entry [11 + ncls + k]) or rmse (w = 1, [11 + 2 ncls + k]).
 * x = the M-vector of that row entry in the M models' rows of the sample.  A sample enters a class slot only if the class has pixels
 * in it (row entry [11 + k] > 0; the models share the class map); a sample with a non-finite x_i for any i is counted and left out
 * for all models.
 * An entry is mau_paired_entry_elems(M) = 2 + M + M (M + 1) / 2 fp64:
 *   [0] n, the samples that entered   [1] the samples skipped for a non-finite value   [2 + i] mean_i
 *   [2 + M + p] Cm_ij = sum (x_i - mean_i)(x_j - mean_j), the upper triangle row-major, p = 0, 1, ... over i <= j.
 * Update per entering sample, in sample order, fp64, not contracted:
 *   n' = n + 1;  d_i = x_i - mean_i;  mean_i' = mean_i + d_i / n';  Cm_ij' = Cm_ij + d_i * (x_j - mean_j').
 * One thread per entry, no atomics, no tickets: the table after any sequence of batches has the bits of the table after the same
 * samples in one batch.  mau_paired_table_elems(M, C, ncls) = G * C * (4 + 2 ncls) * mau_paired_entry_elems(M); the size queries
 * return 0 for arguments the call refuses. */
int mau_paired_groups(void);
int mau_paired_entry_elems(int M);
size_t mau_paired_table_elems(int M, int C, int ncls);
int mau_paired_accumulate(const double* rows, const unsigned char* group, double* table, int M, int B, int C, int ncls,
                          mau_stream_t stream);
/* mau_rank_tests: the rank tests of the same page (section 7 pairwise Wilcoxon, section 3 Mann-Whitney known against unknown cities,
 * sections 1-2 the pooled minimum and 98th percentile) as EXACT INTEGERS, ranks by counting: for element i of a multiset v,
 * less_i = #{j : v_j < v_i}, eq_i = #{j : v_j == v_i} (i included), twice the mid-rank = 2 less_i + eq_i + 1, the tie term
 * sum over tie groups (t^3 - t) = sum_i (eq_i^2 - 1).  Additive to ABI 5.
 *   cols: (Q, M, Ncap) fp64 column store, the first N entries of a column are read and nothing behind them; M in [1,8];
 *   Q in [1,4096]; 1 <= N <= mau_rank_max_samples() = 2^20 (sum eq^2 stays inside int64); Ncap >= N;  known: (N) uint8, non-zero =
 *   a known city.  For a q, a sample with a non-finite value in ANY model is dropped for all of them (`skipped`).
 *   table: mau_rank_table_elems(M, Q) = Q * (7 M (M - 1) / 2 + 4 M + 4) int64, written whole by the call; per q, in this order:
 *     per pair i < j (row-major: (0,1), (0,2), ..., (M-2,M-1)), d = x_i - x_j in fp64, |d| ranked over the kept samples with d != 0:
 *       [0] n_used  [1] n_zero (kept, d == 0)  [2] skipped  [3] 2 W+ (d > 0)  [4] 2 W- (d < 0)  [5] tie term
 *       [6] with at most 13 kept samples sum_i 16^less_i, else 0: bits [4 p, 4 p + 4) hold the size of the tie group that starts at
 *           rank position p (what the exact null distribution of a small sample WITH ties needs beyond the sums)
 *     per model, its kept values ranked, known and unknown cities pooled:
 *       [0] n_known  [1] n_unknown  [2] 2 R_known (twice the rank sum of the known cities)  [3] tie term
 *     the kept values of all M models pooled, n = M * kept samples:
 *       [0] n  [1] the minimum  [2], [3] the order statistics lo = floor(0.98 (n - 1)) = (n - 1) * 49 / 50 and min(lo + 1, n - 1),
 *       as fp64 bit patterns of x + 0.0 (0 when n = 0); element i is the k-th order statistic iff less_i <= k < less_i + eq_i.
 *   ws: mau_rank_ws_elems(Q, N) int64 of workspace (the kept counts and flags).
 * One thread per i, mau_rank_tile() = 256 values of j staged in LDS per step, int64 partial sums joined by integer atomic adds: the
 * bits do not depend on any order.  Four launches on the stream, no host synchronisation.  The size queries return 0 for
 * arguments the call refuses. */
int mau_rank_tile(void);
int mau_rank_max_samples(void);
size_t mau_rank_table_elems(int M, int Q);
size_t mau_rank_ws_elems(int Q, int N);
int mau_rank_tests(const double* cols, const unsigned char* known, int64_t* table, int64_t* ws, int M, int Q, int N, int Ncap,
                   mau_stream_t stream);

/* ---- scenario sessions: a painted canvas -> the network's input, the head's output -> temperature change (the app's per-click path,
 *      app/Home.py:333-411 with app/processing_utils.py:70-181), ONE launch each.  Additive to ABI 5 ----
 * mau_scenario_pack builds N scenario inputs from ONE base tile:
 *   dw_t1 (H,W) uint8 class ids; rgb (3,H,W) fp32, raw 0..255; ndvi (H,W) fp32; temp (H,W) fp32, raw degrees C;
 *   canvas (N,Hc,Wc,4) uint8 RGBA (4-byte aligned); yidx (H), xidx (W) int32: the canvas row / column a destination row / column
 *   samples (nearest-neighbour resize as two tables; an entry outside the canvas is clamped); palette (ncls,3) uint8 RGB, class order;
 *   norm: 8 fp64 = rgb_mean[3], rgb_std[3], temp_mean, temp_std.  ncls in [1, mau_scenario_max_classes()].
 * Per pixel p = canvas[n, yidx[y], xidx[x]]: alpha > 0 -> the class of the lowest-index palette entry of smallest squared RGB
 * distance (integers: equal to scipy's cdist + argmin, the first minimum on a tie), else dw_t1 (canvas_to_dw_map, :70-110).
 *   dw_t2 (N,H,W) uint8 = that class map;
 *   out (N,H,W,ldo) in `dtype`, ldo % 8 == 0, ldo >= 2 ncls + 5, the reference's channel order (:146-148):
 *     [one-hot dw_t1 (ncls) | rgb (3) | ndvi | temp | one-hot dw_t2 (ncls) | zeros up to ldo]
 *   rgb = ((double)v / 255.0 - mean) / std and temp = ((double)v - mean) / std in fp64 with IEEE division, rounded to float once
 *   (the float64 numpy of :136-139 followed by .float(), bit for bit), ndvi as it is; then rounded to `dtype` as
 *   mau_pack_tile_onehot does.  The base tile is read once per scenario. */
int mau_scenario_max_classes(void);
int mau_scenario_pack(const unsigned char* dw_t1, const float* rgb, const float* ndvi, const float* temp, const unsigned char* canvas,
                      const int* yidx, const int* xidx, const unsigned char* palette, const double* norm, void* out, int ldo,
                      unsigned char* dw_t2, int dtype, int N, int H, int W, int Hc, int Wc, int ncls, mau_stream_t stream);
/* mau_scenario_result: out (N,2,H,W) fp32 NCHW, the head's output (channel 0 NDVI, channel 1 normalised temperature);
 * temp_orig (H,W) fp32 raw degrees C, or NULL; dw_t1 (H,W), dw_t2 (N,H,W) uint8.
 *   ndvi (N,H,W) fp32   = channel 0;
 *   temp_c (N,H,W) fp32 = fl32(fl32(out * fl32(temp_std)) + fl32(temp_mean)): two separately rounded fp32 operations, never an
 *                         FMA -- numpy on a float32 array with Python-float scalars (denormalize_output, :179-181);
 *   delta (N,H,W) fp32  = fl32(temp_c - temp_orig) (app/Home.py:400);
 *   rows (N, mau_scenario_result_row_elems() = 5) fp64:
 *     [0] mean delta (:410)  [1] min delta  [2] max delta (NaNs skipped by both)  [3] pixels with dw_t2 != dw_t1
 *     [4] mean delta over those pixels, NaN when there are none.
 * temp_orig == NULL: delta (may be NULL) is not written and rows[0], [1], [2], [4] are NaN.
 * Sums are fp64 in a fixed order: a workgroup owns a run of pixels of ONE scenario (mau_scenario_result_chunks(H, W) workgroups
 * per scenario, a function of H * W alone), the workgroup that draws the scenario's last ticket adds its partials in chunk order --
 * no float atomics; a row's bits do not depend on N or on the scenario's place in the batch, and repeat.
 * ws: fp64 workspace of mau_scenario_result_ws_elems(N, H, W) elements; tickets: a ZEROED mau_reduce_tickets_elems() buffer (left
 * zeroed; see mau_reduce_rows_f64).  One launch per mau_reduce_tickets_elems() scenarios. */
int mau_scenario_result_row_elems(void);
int mau_scenario_result_chunks(int H, int W);
size_t mau_scenario_result_ws_elems(int N, int H, int W);
int mau_scenario_result(const float* out, const float* temp_orig, const unsigned char* dw_t1, const unsigned char* dw_t2, double temp_mean,
                        double temp_std, float* ndvi, float* temp_c, float* delta, double* rows, double* ws, unsigned* tickets, int N,
                        int H, int W, mau_stream_t stream);

/* ---- region forecasts: a raster larger than one tile as overlapping windows at the trained resolution (the reference resizes the
 *      whole region to one tile instead, app/gee_utils.py:40-87, app/processing_utils.py:122-128), ONE launch each.  Additive to ABI 5 ----
 * mau_region_gather builds B window inputs from ONE resident region:
 *   dw_t1, dw_t2 (Hr,Wr) uint8 class ids; rgb (3,Hr,Wr) fp32, raw 0..255; ndvi (Hr,Wr) fp32; temp (Hr,Wr) fp32, raw degrees C;
 *   origins (B,2) int32 ON THE DEVICE, rows of (y0, x0): a captured graph is replayed for the next batch after a device-to-device
 *   copy of B rows, no host synchronisation.  An origin is clamped to [0, Hr - T] x [0, Wr - T]: no index can leave the region;
 *   norm: 8 fp64 on the device, mau_scenario_pack's layout.
 *   out (B,T,T,ldo) in `dtype`, ldo % 8 == 0, ldo >= 2 ncls + 5 (MAU_ERR_ARG otherwise), 16-byte aligned:
 *     [one-hot dw_t1 (ncls) | rgb (3) | ndvi | temp | one-hot dw_t2 (ncls) | zeros up to ldo]
 *   with mau_scenario_pack's arithmetic exactly (one copy of the per-pixel code): fp64 normalisation with IEEE division rounded to
 *   float once, NDVI bits passed through, the cast to `dtype` and a class id >= ncls (no channel set) as mau_pack_tile_onehot.
 * MAU_ERR_ARG: T > min(Hr, Wr), T > 4096, ncls outside [1, mau_scenario_max_classes()], a bad ldo, B > 65535, Hr * Wr > 2^30. */
int mau_region_gather(const unsigned char* dw_t1, const unsigned char* dw_t2, const float* rgb, const float* ndvi, const float* temp,
                      const int* origins, const double* norm, void* out, int ldo, int dtype, int B, int T, int Hr, int Wr, int ncls,
                      mau_stream_t stream);
/* mau_region_stitch blends the windows' outputs into the region; pixel-owned, no atomics.
 *   win (ny * nx, C, T, T) fp32, window k = iy * nx + ix at origin (ys[iy], xs[ix]); ys (ny), xs (nx) int32 on the device; ramp >= 1;
 *   out (C,Hr,Wr) fp32.
 * Integer weights w1(i) = min(i + 1, T - i, ramp), w = w1(y - y0) * w1(x - x0).  For a region pixel, over the windows that cover it,
 * iy ascending and then ix ascending: num += (double)w * (double)v (every product exact in fp64), den += w (integer),
 * out = (float)(num / (double)den), fp64 without contraction.  A pixel no window covers gets NaN; a pixel under one window gets that
 * window's value bit for bit; the bits depend on neither the store width (16 bytes when Wr % 4 == 0 and out is 16-byte aligned, 4
 * bytes otherwise) nor on how the windows were batched through the network.
 * The tables are the caller's to check (the device cannot): strictly ascending, from 0 to Hr - T / Wr - T, no gap wider than T and at
 * most THREE windows over any coordinate (the three table entries from the first window that reaches a pixel are examined).  For
 * any other table the result is unspecified, but every access stays inside the four buffers.
 * MAU_ERR_ARG: T > min(Hr, Wr), T > 4096, ramp < 1, Hr > 65535, Hr * Wr > 2^30, ny * nx > 2^20. */
int mau_region_stitch(const float* win, const int* ys, const int* xs, float* out, int C, int T, int ramp, int Hr, int Wr, int ny, int nx,
                      mau_stream_t stream);

/* ---- placement sweeps: where on a tile does a ph x pw stamp of one land-cover class change the forecast most?  The stamp is written
 *      into the tile's second class map only (the app's canvas edit changes nothing else, app/processing_utils.py:70-110); its effect
 *      is the forecast with the stamp minus the forecast of the unedited tile.  ONE launch each.  Additive to ABI 5 ----
 * mau_placement_pack builds B stamped inputs from ONE resident tile:
 *   dw_t1, dw_t2 (H,W) uint8 class ids (dw_t2 == NULL: dw_t1); rgb (3,H,W), ndvi (H,W), temp (H,W) fp32 raw, norm 8 fp64 on the
 *   device: mau_region_gather's planes with Hr, Wr = H, W;
 *   edits (B,3) int32 ON THE DEVICE, rows of (y0, x0, cls): a captured graph is replayed for the next batch after a device-to-device
 *   copy of B rows.  Sample b, pixel (y, x): the second class id is cls when 0 <= cls < ncls and y0 <= y < y0 + ph and
 *   x0 <= x < x0 + pw (evaluated in 64-bit: every int32 is legal), else dw_t2[y, x].  A stamp over an edge is clipped; a stamp
 *   outside the tile or a cls outside [0, ncls) gives the unedited tile (a baseline sample, the padding of a ragged batch);
 *   out (B,H,W,ldo) in `dtype`, 16-byte aligned:
 *     [one-hot dw_t1 (ncls) | rgb (3) | ndvi | temp | one-hot second map (ncls) | zeros up to ldo]
 *   with mau_scenario_pack's / mau_region_gather's arithmetic exactly (one copy of the per-pixel code).
 * MAU_ERR_ARG: ph or pw < 1, ncls outside [1, mau_scenario_max_classes()], ldo % 8 != 0 or ldo < 2 ncls + 5, B > 65535,
 * H * W > 2^30, a NULL required pointer. */
int mau_placement_pack(const unsigned char* dw_t1, const unsigned char* dw_t2, const float* rgb, const float* ndvi, const float* temp,
                       const int* edits, const double* norm, void* out, int ldo, int dtype, int B, int H, int W, int ph, int pw, int ncls,
                       mau_stream_t stream);
/* mau_placement_result: out (B,2,H,W) fp32 NCHW, the head's output of the B samples; base (2,H,W) fp32, the head's output of the
 * unedited tile; edits as above (only y0, x0 are read: the stamp's rectangle, whatever its class); roi (H,W) uint8, nonzero =
 * inside, or NULL.  Per pixel, for out and base alike, t = fl32(fl32(o1 * fl32(temp_std)) + fl32(temp_mean)) (mau_scenario_result's
 * two roundings, never an FMA); dT = fl32(t - t_base), dN = fl32(o0 - b0).
 *   rows (B, mau_placement_row_elems() = 12) fp64:
 *     [0] pixels of the stamp inside the tile   [1] mean dT over the tile   [2] min dT   [3] max dT
 *     [4] mean dT inside the stamp (NaN when [0] == 0)   [5] mean dT outside it (NaN when the stamp covers the tile)
 *     [6] roi pixels (0 when roi == NULL)   [7] mean dT over the roi (NaN when [6] == 0)
 *     [8] mean dN over the tile   [9] mean dN inside the stamp (NaN when [0] == 0)   [10] mean dN over the roi (NaN when [6] == 0)
 *     [11] non-finite values among the sample's two out planes.
 *   fmin / fmax skip a NaN, the sums carry it.
 * Sums are fp64 in a fixed order: a workgroup owns 4096 consecutive pixels of ONE sample (mau_placement_chunks(H, W) per sample), a
 * thread joins its 16 slots in slot order, the 64 lanes by an xor butterfly 32..1, the four waves in wave order, and the workgroup
 * that draws the sample's last ticket joins the chunks in chunk order -- no float atomics; a row's bits do not depend on B or on the
 * sample's slot, and repeat.  Slots: when H * W % 4 == 0 and out, base are 16-byte and roi 4-byte aligned, slot 4k + j of thread t
 * is pixel (k * 256 + t) * 4 + j of the chunk (16-byte loads); otherwise slot k is pixel k * 256 + t (the two forms add in
 * different orders).  A sum over a subset (stamp, outside, roi) adds +0.0 for a pixel outside the subset.
 * ws: fp64 workspace of mau_placement_ws_elems(B, H, W) elements; tickets: a ZEROED mau_reduce_tickets_elems() buffer (left zeroed;
 * see mau_reduce_rows_f64).  One launch per mau_reduce_tickets_elems() samples.
 * MAU_ERR_ARG: ph or pw < 1, H * W > 2^30, a NULL required pointer. */
int mau_placement_row_elems(void);
int mau_placement_chunks(int H, int W);
size_t mau_placement_ws_elems(int B, int H, int W);
int mau_placement_result(const float* out, const float* base, const int* edits, const unsigned char* roi, double temp_mean,
                         double temp_std, double* rows, double* ws, unsigned* tickets, int B, int H, int W, int ph, int pw,
                         mau_stream_t stream);

/* ---- placement screening: every candidate stamp ranked from ONE input gradient.  The network's input is one-hot: a stamp changes
 *      exactly two channels of a pixel by +-1, so its first-order effect on a scalar objective is a plain sum of input-gradient
 *      entries over the stamp's rectangle, with no step size to choose.  ONE launch each, no allocation, no float atomics, graph-
 *      capturable.  Additive to ABI 5 ----
 * Definitions.
 *   Linearisation point: the resident tile with its second class map dw_t2, as mau_placement_pack writes it with every row cls = -1.
 *   Objective k, 0 <= k < K: row k of objs (K,2) int32 ON THE DEVICE, (ch_k, roi index or -1).  ch_k is 1 for temperature in degrees
 *     C or 0 for NDVI; the roi index names a plane of rois (R,H,W) uint8, nonzero = inside, -1 = the whole tile.  J_k is the mean
 *     over roi_k of the forecast: out1 * temp_std + temp_mean for temperature, out0 for NDVI; n_k is the roi's pixel count.
 *   Seed: dout[k, ch_k, p] = seed_scale * [p in roi_k], the other channel 0.  seed_scale is a positive power of two (default 1) that
 *     a float holds as a normal number: it moves fp16 gradients away from overflow or underflow and is undone exactly below.
 *   Gradient: G (K,H,W,ld) in `dtype`, the gradient of sum_k <dout_k, out_k> with respect to the packed input of K copies of the tile.
 *   Swap term of pixel p towards class c, cur(p) = dw_t2[p]:  s_k(p, c) = G[k,p,off+c] - (cur(p) < ncls ? G[k,p,off+cur(p)] : 0),
 *     formed in fp64 from the loaded values; off = ncls + 5 is the channel offset of the second one-hot block (mau_placement_pack).
 *   Coefficient: coef_k = (ch_k == 1 ? temp_std : 1) / (seed_scale * n_k) in fp64 (one product, one division), applied once, after
 *     the sum.
 * Every index made from a table value (y0, x0, cls, ch, the roi index) is range-checked in 64-bit before it is used.
 *
 * mau_screen_seed: objs, rois (may be NULL when no row names a plane) -> dout (K,2,H,W) fp32, EVERY element written, and counts (K)
 * fp64 holding the integers n_k (integer-valued additions: the same bits in any order).  A row whose ch is neither 0 nor 1 seeds
 * nothing; a roi index outside [-1, R), or >= 0 with rois == NULL, is an empty roi (n_k = 0).  One workgroup per objective.
 * MAU_ERR_ARG: a NULL required pointer, K outside [1, 65535], R < 0, H * W > 2^30, seed_scale no such power of two. */
int mau_screen_row_elems(void);
int mau_screen_seed(const int* objs, const unsigned char* rois, int R, double seed_scale, float* dout, double* counts, int K, int H, int W,
                    mau_stream_t stream);
/* mau_screen_rows: G with its pixel stride ld >= 2 ncls + 5 (elements) and dtype; dw_t2 (H,W) uint8 (required: the map the
 * linearisation point was packed with); edits (P,3) int32 ON THE DEVICE, rows of (y0, x0, cls) as mau_placement_pack reads them;
 * counts and objs as above ->
 *   rows (K, P, mau_screen_row_elems() = 4) fp64:
 *     [0] pixels of the stamp inside the tile
 *     [1] of those, pixels whose class changes (cur(p) != cls)
 *     [2] predicted change of J_k = coef_k * sum over the stamp's pixels inside the tile of s_k(p, cls)
 *     [3] non-finite gradient values read for this row: per pixel, G[k,p,off+cls], and G[k,p,off+cur(p)] when cur(p) < ncls.
 *   The stamp test is mau_placement_pack's: 64-bit, every int32 legal, a stamp over an edge is clipped.  cls outside [0, ncls) gives
 *   ([0], 0, +0.0, 0) and reads no gradient (the pack would leave the tile as it is).  n_k == 0: [2] is NaN, whatever cls is.  A
 *   non-finite value propagates into [2] and is counted in [3].
 * One 256-thread workgroup per (row, objective).  Slot i of the UNCLIPPED ph x pw rectangle, row-major, belongs to thread i % 256; a
 * thread joins its slots in increasing i and a slot outside the tile contributes nothing (it is skipped, not added as 0), so the order
 * does not depend on clipping; then the 64 lanes by an xor butterfly 32..1 and the four waves in wave order.  4-byte / 2-byte gathers,
 * two per pixel, any alignment of G.  A row's bits depend on nothing but its own table row, its objective and the tile -- not on P, on
 * the row's place in the table, or on K -- and repeat.  Any ph * pw works: the loop visits only the rectangle's rows and columns
 * inside the tile.
 * MAU_ERR_ARG: a NULL required pointer, ph or pw < 1, H * W > 2^30, ncls outside [1, mau_scenario_max_classes()], ld < 2 ncls + 5,
 * K outside [1, 65535], P < 1, a bad dtype or seed_scale. */
int mau_screen_rows(const void* G, int ld, int dtype, const unsigned char* dw_t2, const int* edits, const double* counts, const int* objs,
                    double temp_std, double seed_scale, double* rows, int K, int P, int H, int W, int ph, int pw, int ncls,
                    mau_stream_t stream);
/* mau_screen_maps: for ONE objective k of the K in G, maps (ncls,H,W) fp32 with maps[c, p] = fl32(coef_k * s_k(p, c)) for every class c
 * -- "what would this pixel do as class c"; NaN everywhere when n_k == 0.  Every element is written.  Pixel-owned: one thread per
 * pixel reads the groups of 8 channels that hold the second one-hot block (at most three).  Two load forms, chosen by the host from ld
 * and the alignment of G alone:
 *   ld % 8 == 0 and G 16-byte aligned: 16-byte loads (one per group for bf16 / fp16, two for fp32);
 *   otherwise: element by element, the same groups of 8 from channel (off & ~7) on, no channel at or beyond off + ncls.
 * The two forms load the same values and compute the same bits.
 * MAU_ERR_ARG: as mau_screen_rows, and k outside [0, K). */
int mau_screen_maps(const void* G, int ld, int dtype, const unsigned char* dw_t2, const double* counts, const int* objs, double temp_std,
                    double seed_scale, float* maps, int k, int K, int H, int W, int ncls, mau_stream_t stream);

/* ---- model comparison: M heads' outputs of ONE tile against one target (the developer app's Model Comparison page,
 *      app_dev/pages/1_Model_Comparison.py with app_dev/app_src/utils.py:170-271), ONE launch each.  Additive to ABI 5 ----
 * mau_compare_result: out (M,2,H,W) fp32 NCHW, the M heads' outputs (channel 0 NDVI, channel 1 normalised temperature);
 * tgt (2,H,W) fp32, the normalised target.
 *   pred_u (M,2,H,W) fp32: channel 0 as it is; channel 1 = fl32(fl32(out * fl32(temp_std)) + fl32(temp_mean)), two separately
 *                          rounded fp32 operations, never an FMA (utils.py:260-261; as mau_scenario_result);
 *   gt_u (2,H,W) fp32    = the same rule on the target, written once;
 *   err (M,2,H,W) fp32   = fl32(pred_u - gt_u);
 *   rows (M * 2, mau_compare_row_elems() = 40) fp64, row m * 2 + c: five regions of eight entries, in the order whole tile,
 *     top-left, top-right, bottom-left, bottom-right -- rows [0, H/2) | [H/2, H), columns [0, W/2) | [W/2, W), integer division
 *     (utils.py:173-178).  Entries of a region:
 *       [0] its pixel count  [1] gt min  [2] gt max  [3] pred min  [4] pred max  [5] max |err|  [6] sum |err|  [7] sum err^2.
 *     fmin / fmax skip a NaN, the sums carry it.  A region without pixels: count 0, minima +inf, maxima -inf, [5..7] 0.  The
 *     whole-tile entries are the join of the four quadrants' in that order: ((TL o TR) o BL) o BR.
 * Sums are fp64 in a fixed order: a workgroup owns a run of pixels of ONE (model, channel) plane (mau_compare_chunks(H, W)
 * workgroups per plane, a function of H * W alone), the workgroup that draws the plane's last ticket joins its partials in chunk
 * order -- no float atomics; a row's bits do not depend on M or on the model's place, and repeat.  16-byte accesses when
 * H * W % 4 == 0 and the five tensors are 16-byte aligned, 4-byte ones otherwise (the two forms add in different orders).
 * ws: fp64 workspace of mau_compare_ws_elems(M, H, W) elements; tickets: a ZEROED mau_reduce_tickets_elems() buffer (left zeroed;
 * see mau_reduce_rows_f64).  One launch per mau_reduce_tickets_elems() rows. */
int mau_compare_row_elems(void);
int mau_compare_chunks(int H, int W);
size_t mau_compare_ws_elems(int M, int H, int W);
int mau_compare_result(const float* out, const float* tgt, double temp_mean, double temp_std, float* pred_u, float* gt_u, float* err,
                       double* rows, double* ws, unsigned* tickets, int M, int H, int W, mau_stream_t stream);
/* mau_compare_inputs: the page's views of one compact sample (utils.py:224-252).  cls_a, cls_b (H,W) uint8 class ids; cont (5,H,W)
 * fp32, normalised rgb (3), ndvi, temperature; palette (ncls,3) uint8 RGB in class order, ncls in [1, mau_scenario_max_classes()];
 * norm: 8 fp64 = rgb_mean[3], rgb_std[3], temp_mean, temp_std.
 *   rgb8 (H,W,3) uint8   = clip(((double)x * rgb_std[c] + rgb_mean[c]) * 255.0, 0, 255) truncated toward zero: fp64, every operation
 *                          rounded on its own (a float32 array times a float64 array, utils.py:225-226); a NaN gives 0;
 *   temp_c (H,W) fp32    = the two-rounding fp32 rule above (utils.py:229);   ndvi (H,W) fp32 = the plane as it is;
 *   dw_t1_rgb, dw_t2_rgb (H,W,3) uint8 = palette[cls_a], palette[cls_b]; a class id >= ncls gives (0,0,0). */
int mau_compare_inputs(const unsigned char* cls_a, const unsigned char* cls_b, const float* cont, const unsigned char* palette,
                       const double* norm, unsigned char* rgb8, float* temp_c, float* ndvi, unsigned char* dw_t1_rgb,
                       unsigned char* dw_t2_rgb, int H, int W, int ncls, mau_stream_t stream);

/* ---- ground-truth sensitivity (test/generate_ground_truth_sensitivity.py): binned mean / standard deviation of the targets of a
 *      split, TWO launches per batch, no target kept on the host.  Additive to ABI 5 ----
 * A moment row is mau_moments_row_elems() = 4 fp64: [0] n, the number of values  [1] their mean  [2] M2 = sum (x - mean)^2
 * [3] the number of non-finite values among them (their arithmetic propagates: a NaN value gives a NaN mean and M2, as np.mean /
 * np.std do).  Two rows a, b merge by the pairwise update, in fp64 without contraction:
 *   delta = mean_b - mean_a;  n = n_a + n_b;  mean = mean_a + (delta * n_b) / n;
 *   M2 = (M2_a + M2_b) + (delta * delta) * ((n_a * n_b) / n);  an empty a (n_a == 0) gives b as it is.
 *
 * mau_plane_moments: x (B,C,H,W) fp32 NCHW, HW = H * W  ->  rows (B*C) x 4 fp64, row b*C + c = the moments of that plane.
 * A workgroup owns 4096 consecutive pixels of ONE plane (mau_plane_moments_chunks(HW) workgroups per plane, a function of HW
 * alone), keeps them in registers as doubles and makes two passes: the chunk mean, then sum (x - chunk mean)^2 -- not
 * E[x^2] - E[x]^2.  Sums are fp64 in a fixed order; the workgroup that draws the plane's last ticket merges the chunk rows in chunk
 * order.  A row's bits do not depend on B or on the plane's place in the batch, and repeat.  16-byte loads when HW % 4 == 0 and x
 * is 16-byte aligned, 4-byte loads otherwise (the two forms add in different orders: keep x 16-byte aligned for bits that are a
 * function of HW alone).  ws: fp64 workspace of mau_plane_moments_ws_elems(B, C, HW) elements; tickets: a ZEROED
 * mau_reduce_tickets_elems() buffer (left zeroed; see mau_reduce_rows_f64).  One launch per mau_reduce_tickets_elems() planes. */
int mau_moments_row_elems(void);
int mau_plane_moments_chunks(int64_t HW);
size_t mau_plane_moments_ws_elems(int B, int C, int64_t HW);
int mau_plane_moments(const float* x, double* rows, double* ws, unsigned* tickets, int B, int C, int64_t HW, mau_stream_t stream);
/* mau_bin_moments: merges the B*C rows of a batch into table [axes][bins][C] x 4 fp64 moment rows (DEVICE resident, zeroed by the
 * caller before the first batch), ONE workgroup, one thread per (axis, bin, channel): axes * bins * C <= mau_bin_moments_max_entries(),
 * axes <= 4.
 *   meta (B, meta_pitch) fp32: the normalised metadata, meta_pitch floats from row to row;
 *   cols_host, std_host, mean_host: HOST arrays of `axes` entries -- the metadata column of an axis and what un-normalises it:
 *     coordinate = (double)meta[b][col] * std + mean, a separately rounded fp64 product and sum (numpy: float32 array times
 *     np.float64 scalar);
 *   edges: DEVICE, axes x (bins + 1) fp64, the ASCENDING bin edges of axis a at edges + a * (bins + 1).  The device cannot check
 *     the order: the HOST does (ground_truth.BinStats), unordered edges give unspecified bins (never an access out of bounds).
 * Bin of a sample on an axis = np.digitize's: k = the number of edges <= coordinate; kept iff 1 <= k <= bins, bin k - 1 (on an edge:
 * the upper bin; on the last edge, beyond either end, or NaN: dropped).  A thread walks the samples in sample order and merges
 * those of its bin into its entry -- no atomics, no tickets: the table after any sequence of batches has the bits of the table
 * after the same samples in one batch. */
int mau_bin_moments_max_entries(void);
int mau_bin_moments(const double* rows, const float* meta, int meta_pitch, const int* cols_host, const double* std_host,
                    const double* mean_host, const double* edges, double* table, int B, int C, int axes, int bins,
                    mau_stream_t stream);

/* ---- dataset survey (src/utils/visualize_npz.py extract_metrics): what the per-tile CSV row needs from the pixels of a compact
 *      batch, ONE launch, every byte read once.  Additive to ABI 5 ----
 * cls_a, cls_b (B,H,W) uint8 class maps; cont (B,5,H,W) fp32: r, g, b, ndvi_t1, temp_t1; targets (B,2,H,W) fp32: ndvi_t2, temp_t2;
 * HW = H * W; num_classes in [1,16] (the dataset's layout: 9).  rows (B) x mau_tile_stats_row_elems() = 106 fp64, per sample:
 *   [0,16)   pixels of cls_a per class (0 for classes >= num_classes)     [16,32)  the same of cls_b
 *   [32], [33]  values >= num_classes in cls_a, in cls_b
 *   [34 + 8p, 34 + 8p + 8)  the plane row of value plane p:
 *        +0 n   +1 mean   +2 M2 = sum (x - mean)^2   +3 min   +4 max   +5 sum |x|   +6 NaN values   +7 non-finite values
 *     p = 0..4 the planes of cont, 5 and 6 those of targets, 7 = ndvi_t2 - ndvi_t1, 8 = temp_t2 - temp_t1: the differences of the
 *     values as stored (normalised), formed in fp64 from the loaded floats and never written to memory.
 * Geometry and arithmetic are mau_plane_moments': a workgroup owns 4096 consecutive pixels of ONE sample and walks its planes,
 * values as doubles from the load on, two passes over register-resident values (chunk mean, then squared distances), sums in a
 * fixed order; the workgroup that draws the sample's last ticket merges the chunk rows in chunk order ((n, mean, M2) by the
 * pairwise update above; min / max / counts exactly).  A row's bits depend on the sample's own bytes only -- not on B, not on its
 * place in the batch -- and repeat.  A NaN value is counted and propagates into mean and M2; min and max skip it (the caller sets
 * them to NaN when +6 is not zero, as np.min does).  16-byte loads of the fp32 planes and 4-byte loads of the class maps when
 * HW % 4 == 0, cont and targets are 16-byte and cls_a and cls_b 4-byte aligned; scalar loads otherwise (the two forms add in
 * different orders: keep the bases aligned for bits that are a function of HW alone).  ws: fp64 workspace of
 * mau_tile_stats_ws_elems(B, HW) elements; tickets: a ZEROED mau_reduce_tickets_elems() buffer (left zeroed; see
 * mau_reduce_rows_f64).  One launch per mau_reduce_tickets_elems() samples. */
int mau_tile_stats_row_elems(void);
size_t mau_tile_stats_ws_elems(int B, int64_t HW);
int mau_tile_stats(const unsigned char* cls_a, const unsigned char* cls_b, const float* cont, const float* targets, double* rows,
                   double* ws, unsigned* tickets, int B, int64_t HW, int num_classes, mau_stream_t stream);

/* ---- dataset build (src/data/processing_10m/process.py: the filter check and running statistics of :37-50 / :84-115, the
 *      normalisation of :175-183): what the build needs from the pixels of a batch of RAW samples, ONE launch, every byte read
 *      once.  Additive to ABI 5 ----
 * dw_t1, dw_t2 (B,H,W) uint8 class maps; rgb (B,3,H,W) fp32, raw 0..255 values; ndvi_t1, ndvi_t2, temp_t1, temp_t2 (B,H,W) fp32;
 * HW = H * W; num_classes in [1,16] (the dataset's layout: 9).  Three outputs, each optional (NULL skips it; cont and targets come
 * together):
 * rows (B) x mau_raw_tile_row_elems() = 38 fp64, per sample:
 *   [0,16)   pixels where (dw_t1 == c) != (dw_t2 == c), per class c (0 for classes >= num_classes): count / HW is the reference's
 *            per-channel mean |ohe2 - ohe1|                 [16], [17]  values >= num_classes in dw_t1, in dw_t2
 *   [18] sum |ndvi_t2 - ndvi_t1|   [19] non-finite values of that difference   [20], [21] the same of temp_t2 - temp_t1: the
 *            differences formed in fp64 from the loaded floats (exact) and never written to memory
 *   [22 + 4p, 22 + 4p + 4)  the moment row  +0 n  +1 mean  +2 M2 = sum (x - mean)^2  +3 non-finite values  of p = 0..2: r / 255,
 *            g / 255, b / 255 (the division in fp64), p = 3: temp_t1 -- two passes, not the reference's sum x^2 / n - mean^2.
 * cont (B,5,H,W), targets (B,2,H,W) fp32, the layout mau_tile_stats and mau_pack_tile_onehot take; they need norm, 8 fp64 on the
 * DEVICE: rgb_mean[3], rgb_std[3], temp_mean, temp_std.  numpy's arithmetic for float32 rasters, operation for operation, nothing
 * contracted:
 *   cont[0..2] = (float)(((double)rgb / 255.0 - mean_c) / std_c)     cont[3] = ndvi_t1, targets[0] = ndvi_t2, bits unchanged
 *   cont[4], targets[1] = (t - (float)temp_mean) / (float)temp_std in fp32, the division correctly rounded.
 * Geometry and order are mau_tile_stats': a workgroup owns 4096 consecutive pixels of ONE sample, sums in a fixed order, counts
 * from ballots, no float atomics; the workgroup that draws the sample's last ticket merges the chunk rows in chunk order.  A
 * row's bits and a plane's bits depend on the sample's own bytes only -- not on B, not on its place in the batch, not on which
 * outputs were asked for -- and repeat.  A non-finite value is counted and propagates into the sums it enters.  16-byte loads and
 * stores of the fp32 planes and 4-byte loads of the class maps when HW % 4 == 0, every fp32 tensor is 16-byte and both class maps
 * are 4-byte aligned; scalar accesses otherwise (the two forms add in different orders: keep the bases aligned for rows that are
 * a function of HW alone; the planes are the same bits either way).  ws: fp64 workspace of mau_raw_tile_ws_elems(B, HW) elements,
 * tickets: a ZEROED mau_reduce_tickets_elems() buffer (left zeroed; see mau_reduce_rows_f64) -- both needed for rows only.  One
 * launch per mau_reduce_tickets_elems() samples.  Refused (MAU_ERR_ARG): a NULL input, rows without ws / tickets, cont without
 * targets or either without norm, nothing asked for, B <= 0, HW <= 0, HW > 2^30, num_classes outside [1,16], an fp32 tensor not
 * 4-byte or an fp64 tensor not 8-byte aligned. */
int mau_raw_tile_row_elems(void);
size_t mau_raw_tile_ws_elems(int B, int64_t HW);
int mau_raw_tile_process(const unsigned char* dw_t1, const unsigned char* dw_t2, const float* rgb, const float* ndvi_t1,
                         const float* ndvi_t2, const float* temp_t1, const float* temp_t2, const double* norm, double* rows, float* cont,
                         float* targets, double* ws, unsigned* tickets, int B, int64_t HW, int num_classes, mau_stream_t stream);

/* ---- climate stage (src/data/process_temperature.py: the 1901-1950 baseline of :23-33, the normalised anomalies of :48-55,
 *      TemperatureQuery.query of :93-114).  Additive to ABI 5 ----
 * x (T,G) fp32: the year files concatenated along time, time-major, the G = lat * lon cells of a month contiguous.  A baseline row
 * is mau_climate_row_elems() = 4 fp64 per cell: [0] n, the number of non-NaN months  [1] their mean  [2] M2 = sum (x - mean)^2 over
 * them  [3] the number of NaN months (n + [3] = T).
 *
 * mau_climate_baseline: x (T,G) -> rows (G,4).  One thread per cell, consecutive threads on consecutive cells; two passes over time
 * in TIME ORDER in fp64, nothing contracted: sum of the non-NaN months, mean = sum / n, then M2.  A NaN is skipped and counted
 * (skipna); an infinity is not skipped and propagates (mean +-inf or NaN, M2 NaN), as np.nanmean lets it; a cell without a month
 * gets mean = M2 = NaN.  No workspace, no atomics: a cell's bits depend on its own column only -- not on G, not on its place.
 *
 * mau_climate_normalise: out (T,G) fp32 = (float)(((double)x - mean) / sqrt(M2 / n)), fp64 and rounded once, with the cell's row of
 * `rows`.  std == 0 and an empty cell give what IEEE division gives (+-inf, NaN).  16-byte accesses (four cells per thread) when
 * G % 4 == 0 and x and out are 16-byte aligned, 4-byte ones otherwise: the same bits either way.  T <= 65535 * 64.
 *
 * mau_climate_series: the batched nearest-grid-point query.  x is the RAW grid, rows its baseline; per query n the DEVICE arrays
 * cell[n] (the cell, in [0,G)) and keep[n] (the months to keep, in [0,T]; clamped to that range).  series (N,Tpad) fp32:
 * series[n][t] for t < keep[n] is the expression of mau_climate_normalise on x[t][cell[n]] (the same bits), 0 for t >= keep[n]
 * (pad_sequence's padding).  srows (N,4) fp64: the moment row (mau_moments_row_elems: n, mean, M2, non-finite values) of the kept
 * values of series[n], two passes, sums in a fixed order (one 256-thread workgroup per query, a series is one chunk of
 * mau_plane_moments: T <= mau_climate_series_max_months() = 4096).  keep[n] == 0 gives the row (0, NaN, 0, 0).  A cell outside
 * [0,G) cannot be refused without a read-back: its kept values are NaN and its row is (0, NaN, 0, 0); nothing is read out of
 * bounds.  No host work per query, no synchronisation: the launch can be captured.  A query's bits depend on its own cell and keep
 * only -- not on N, not on its place.
 * Refused (MAU_ERR_ARG): a NULL pointer, T, G or N <= 0, G or N > 2^30, an fp32 / int32 buffer not 4-byte or an fp64 buffer not
 * 8-byte aligned; for the series T > 4096 and Tpad < T. */
int mau_climate_row_elems(void);
int mau_climate_series_max_months(void);
int mau_climate_baseline(const float* x, double* rows, int T, int G, mau_stream_t stream);
int mau_climate_normalise(const float* x, const double* rows, float* out, int T, int G, mau_stream_t stream);
int mau_climate_series(const float* x, const double* rows, const int* cell, const int* keep, float* series, double* srows, int N,
                       int T, int G, int Tpad, mau_stream_t stream);

/* ---- loss: F.mse_loss (src/utils/losses.py:27-39) -------------------------- */
/* loss[0] = mean((out-tgt)^2) (fp64 accumulation, fixed order); dout (optional) = 2*(out-tgt)/n;
 * partial: fp64 workspace of mau_mse_blocks(n) elements. */
int mau_mse_blocks(int64_t n);
int mau_mse_fwd_bwd(const float* out, const float* tgt, double* partial, float* loss, float* dout, int64_t n,
                    mau_stream_t stream);

/* ---- L1 + gradient (finite-difference) losses (src/utils/losses.py:5-25 gradient_loss, :68 F.l1_loss) ---- */
/* out/tgt (B,C,H,W) fp32.  terms[0..2] = { mean|out-tgt|, mean| |dy out|-|dy tgt| |, mean| |dx out|-|dx tgt| | }
 * (gradient_loss = terms[1] + terms[2]);  dout (optional) = d/d out of  w_l1*terms[0] + w_grad*(terms[1]+terms[2]).
 * partial: fp64 workspace of 3*mau_l1_gradient_blocks(n) elements, n = B*C*H*W. */
int mau_l1_gradient_blocks(int64_t n);
int mau_l1_gradient_loss(const float* out, const float* tgt, double* partial, float* terms, float* dout, float w_l1,
                         float w_grad, int B, int C, int H, int W, mau_stream_t stream);

/* ---- SSIM term of compute_loss_l1_grad_ssim (src/utils/losses.py:70-97; piq.ssim defaults, PARITY UNPINNED: piq is
 *      not available to generate a fixture; value only -- the reference detaches it at :96) ---- */
/* out/tgt (B,C,H,W) fp32.  prep != 0 applies the reference's channel preparation while loading (:72-84): channel 0 ->
 * (v+1)/2, channel 1 -> clamp(v,0,1).  per_image (B) = SSIM per sample (mean over channels), loss[0] = 1 - mean(per_image).
 * ws: fp64 workspace of mau_ssim_ws_elems(B,C,H,W) elements (per-tile sums, added in a fixed order). */
size_t mau_ssim_ws_elems(int B, int C, int H, int W);
int mau_ssim_loss(const float* out, const float* tgt, double* ws, float* per_image, float* loss, int prep, int B, int C,
                  int H, int W, mau_stream_t stream);
/* The adjoint, for training ON the SSIM term (opt-in; the reference's own criterion detaches it).  Additive to ABI 5.
 * dout (B,C,H,W) fp32 = scale * d loss / d out, loss being exactly loss[0] of mau_ssim_loss for the same geometry, window and
 * prep.  EVERY element is written (no pre-zeroed buffer): +0.0 in the rows / columns avg_pool2d drops and, with prep != 0, where
 * channel 1 lies outside [0, 1] (bounds inclusive, torch.clamp's backward); the prepared channel 0 carries its factor 0.5.  tgt
 * gets no gradient.  One launch, pixel-owned: a workgroup owns a 16x16 tile of pooled pixels and recomputes the moments of the
 * 26x26 map pixels that reach it -- no float atomics, the results repeat bit for bit; scale is the last factor applied.
 * Refusals as in mau_ssim_loss. */
int mau_ssim_loss_grad(const float* out, const float* tgt, float* dout, float scale, int prep, int B, int C, int H, int W,
                       mau_stream_t stream);

/* ---- every term of compute_all_loss (src/utils/losses.py:101-115) for one batch in ONE launch: what the validation pass
 *      (src/train.py:20-60) averages.  Value only.  Additive to ABI 5 ----
 * out/tgt (B,2,H,W) fp32 (C != 2 is refused: the channel preparation of :72-84 is defined for NDVI and temperature only).
 * terms (8 fp32):
 *   [0] mse (:33)   [1] pixel = mean|out-tgt| (:67)   [2] mean| |dy out|-|dy tgt| | (:22)   [3] the same in x (:23)
 *   [4] gradient = [2] + [3] (:25)   [5] ssim = 1 - mean(ssim_per_image) (:89), geometry, window and channel preparation of
 *   mau_ssim_loss with prep != 0   [6] [0] + lambda_grad * [4] (:51)   [7] [1] + lambda_grad * [4] + lambda_ssim * [5] (:92);
 *   [4], [6] and [7] are fp32 operations in the reference's order, never contracted.
 * ssim_per_image (B fp32): SSIM per sample, as mau_ssim_loss gives it.
 * acc (8 fp64, or NULL): acc[k] += B * (double)terms[k] -- the reference's `v.item() * len(batch)` (src/train.py:42,48) kept on the
 *   device; a pass over a split reads it back once.  The caller zeroes it before the first batch.
 * Sums are fp64 in a fixed order: a workgroup owns one 16x16 tile of the SSIM map of one (image, channel) plane and a disjoint
 * rectangle of its full-resolution pixels, the workgroup that draws the last ticket adds the partials in index order -- no float
 * atomics; the results repeat bit for bit.  An image smaller than the 11x11 window after pooling is refused.
 * ws: fp64 workspace of mau_loss_terms_ws_elems(B, C, H, W) elements; tickets: a ZEROED buffer of at least one uint32
 * (mau_reduce_tickets_elems() entries will do), left zeroed; see mau_reduce_rows_f64. */
size_t mau_loss_terms_ws_elems(int B, int C, int H, int W);
int mau_loss_terms(const float* out, const float* tgt, double* ws, unsigned* tickets, float* terms, float* ssim_per_image,
                   double* acc, float lambda_grad, float lambda_ssim, int B, int C, int H, int W, mau_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MAU_HIP_H */
