/* clamd.h -- C ABI of libclamd.so: the MI355X (gfx950) kernels behind the UNet segmentation train step of
 * LorenzoFramba/Continual-Learning.
 *
 * The reference defines NO FFI for this path: its hot loop (trainer.py:168-176) calls PyTorch modules
 * (models/unet.py:8-92) whose kernels live in ATen/cuDNN.  This header is therefore the interface a maintainer
 * would bind INSTEAD of those torch operators; each entry point names the reference call site it replaces.
 * INTEGRATION.md shows the ctypes binding and the torch.autograd.Function glue.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, ints, doubles; `stream` is a hipStream_t passed as void*.
 *   - every call only ENQUEUES work on `stream`; no allocation, no host synchronisation, graph-capturable.
 *     Buffers are owned by the caller (PyTorch's allocator) and only borrowed for the enqueue.
 *   - return 0 on success, negative on error; clamd_last_error() returns the (thread-local) message.
 *   - activations are NHWC in the compute dtype with an explicit channel pitch `ldc` (elements) so that a
 *     tensor may be a channel slice of a concat buffer (replaces torch.cat, models/unet.py:83-87).
 *     Physical channel counts (`*_p`) are padded to a power of two >= 32; padded channels hold zeros.
 *   - dtype: CLAMD_F32 computes with v_mfma_f32_32x32x2_f32 (exact fp32), CLAMD_BF16 stores activations and
 *     packed weights as bf16 and accumulates in fp32 (v_mfma_f32_32x32x16_bf16).  CLAMD_SPLIT ("bf16x3") stores
 *     every activation and packed weight as the bf16 pair hi = rne(x), lo = rne(x - hi) (4 bytes per element) and
 *     multiplies hi*hi + hi*lo + lo*hi with fp32 accumulation (~2^-17 relative product error).  Its tensors keep the
 *     fp32 geometry (element counts, `ldc`, byte sizes), but each 16-channel group of a pixel is laid out as
 *     [16 x bf16 hi][16 x bf16 lo]; tensor and channel-slice bases must be 64-byte aligned and `ldc` a multiple of
 *     16 (checked on entry).  clamd_nchw_to_nhwc / clamd_nhwc_to_nchw convert at the boundary.
 */
#ifndef CLAMD_H
#define CLAMD_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { CLAMD_F32 = 0, CLAMD_BF16 = 1, CLAMD_SPLIT = 2 };
enum { CLAMD_WGRAD_CONV3 = 0, CLAMD_WGRAD_PW = 1, CLAMD_WGRAD_UP2 = 2 };

const char* clamd_last_error(void);
int clamd_version(void);
/* layout constants the host side needs to build device tables */
int clamd_sizeof_pack_job(void);
int clamd_sizeof_adam_tensor(void);
int clamd_adam_chunk_elems(void);
int clamd_sizeof_importance_tensor(void);   /* clamd_importance_accum: one table row {float* dst; const float* src; long long n} */
int clamd_pack_tile(void);            /* clamd_pack: blocks per job = ceil(Np/tile) * ceil(Kp/tile) */
int clamd_bn_bwd_nsums(void);

/* ---- per-call kernel-structure selection --------------------------------------------------------------------
 * The library keeps NO mutable process state (nn.DataParallel, trainer.py:122, drives one Python thread
 * per GPU through the same code).  Every entry point that chooses between kernel structures takes a
 * `const clamd_tuning*`; NULL = the defaults clamd_tuning_init() writes.  Activations are bit-identical under every
 * setting; statistics / weight gradients differ only in (fixed) summation order.
 *   igemm_pws      0|1|2   persistent conv kernel: never | <= 256 input channels | always
 *   igemm_ws       0..4    producer/consumer kernel: never | 256-px | heuristic | 512-px | 128-px tiles
 *   igemm_variant  0|1|2   baseline kernel prefetch variants
 *   pws_wres       0|1     persistent kernel: filter slab kept in LDS across tiles when a tile has two K-steps
 *   wgrad_ws 0|1, wgrad_dma 0|1|2 (LDS-DMA staging: never | heuristic | always), wgrad_xcd 0|1,
 *   wgrad_blocks 1..1024 (split-K target in workgroups on a whole chip, two per CU = 512 by default), wgrad_tw16 0|1
 *   wino_band      0 (per-launch choice) | 1..32 output-channel slabs per band of the Winograd block order
 *   wino_persist   0|1     one workgroup per tile | persistent tile loop
 *   wino_mt        0|1|2   tile height: per-launch choice | 8 | 16 pixels
 *   bn_reduce_blocks / chsum_blocks   0 (per-launch choice) | n: grid cap of the per-channel reductions
 *   cu_reserve     CUs the persistent grids leave free (for RCCL channel workgroups under data parallelism)
 *   wgrad_streamk  0|1|2   clamd_wgrad_winograd24_pre / 44_pre: split-K plan in whole rounds of the chip | per launch (stream-K from 96 items on) |
 *                          always the k-steps of all (plane, block) items dealt evenly to one workgroup per CU (static map, an item's slots
 *                          added in slot order: deterministic)
 *   wino_half      0|1     clamd_conv3x3_winograd24: 32 tiles x 64 channels, one workgroup per CU | 32 x 32, two per CU (wino24n.hip) */
typedef struct clamd_tuning {
    int igemm_pws, igemm_ws, igemm_variant, pws_wres;
    int wgrad_ws, wgrad_dma, wgrad_xcd, wgrad_blocks, wgrad_tw16;
    int wino_band, wino_persist, wino_mt;
    int bn_reduce_blocks, chsum_blocks;
    int cu_reserve;
    int wino_half;
    int wgrad_streamk;
    int reserved[7];
} clamd_tuning;
int clamd_sizeof_tuning(void);
void clamd_tuning_init(clamd_tuning* t);

/* ---- deterministic per-channel reductions ---------------------------------------------------------------------
 * BatchNorm statistics (sum, sum of squares) and the five BatchNorm-backward sums are never accumulated with float
 * atomics: every producing launch writes `rows` partial rows [row][nk][Cp] (nk = 2 or 5) with plain stores, one row per
 * workgroup (or per tile), and clamd_bn_finalize / clamd_bn_bwd_finalize add rows 0..rows-1 in a fixed order in fp64.
 * Two runs on the same inputs are bit-identical.  The caller sizes the buffer with clamd_stat_rows() for the SAME
 * arguments it launches with and passes that row count to the launch (checked) and to the finalize call. */
enum { CLAMD_OP_CONV3X3 = 0, CLAMD_OP_CONV3X3_WINOGRAD = 1, CLAMD_OP_CONV1X1 = 2, CLAMD_OP_CONVT2X2_DGRAD = 3,
       CLAMD_OP_BN_BWD_REDUCE = 4, CLAMD_OP_CONV3X3_WINOGRAD24 = 5, CLAMD_OP_CONV3X3_WINOGRAD44 = 6 };
/* rows a launch of `op` writes: (B,H,W) = pixel grid of the launch, Cin_p/Cout_p as passed to it (BN_BWD_REDUCE: Cout_p = Cp,
 * Cin_p != 0 means the pooled variant), fused_bn != 0 when bn_y/bn_sums are passed.  Negative on error. */
int clamd_stat_rows(int op, int B, int H, int W, int Cin_p, int Cout_p, int dtype, int fused_bn, const clamd_tuning* tune);

/* ---- implicit-GEMM convolutions (igemm.hip) ---------------------------------------------------------------
 * nn.Conv2d(k3,s1,p1)+bias followed by nn.ReLU (models/unet.py:13-14,16-17,28-29,31-32,50-51,53-54,66-67,69-70):
 *   y = relu?(conv3x3(x, w) + bias), and (if stats != NULL) per-channel sum / sum-of-squares of y written as
 *   partial rows stats[row][2][Cout_p] for the following nn.BatchNorm2d (unet.py:15,...).  The same entry point run
 *   on the flipped/transposed packing computes the data gradient of that conv (loss.backward(), trainer.py:175).
 *   w_packed: [9][Cout_p][Cin_p] compute dtype, Cin innermost (see clamd_pack).  m_fastest: block order hint.
 *   bn_y/bn_sums (optional, data-gradient launches): when y of THIS launch is the gradient w.r.t. a BatchNorm output,
 *   also accumulate the five per-channel sums of clamd_bn_bwd_reduce (bn_y = that unit's saved activation
 *   [B,H,W,Cout_p], bn_sums = [row][5][Cout_p]) in the epilogue, so the separate reduce pass is not needed.  bn_y has no pitch
 *   argument: it is read dense, at pitch Cout_p (a saved activation of its own, never a slice of a concat buffer).
 *   stat_rows = clamd_stat_rows(CLAMD_OP_CONV3X3, ...) (ignored when neither stats nor bn_sums is given).  With fused_bn that query
 *   describes the PLAIN data-gradient launch (no bias, ReLU, statistics), as clamd_conv3x3_bn_sums does: a bf16 launch that passes bn_y
 *   together with one of those is declined by the persistent kernel and writes one row per 256-pixel tile (or per tile of the
 *   producer/consumer kernel igemm_ws names); a stat_rows that does not match is refused, never mis-summed.
 *   relu: bit 0 = apply ReLU; bit 1 (CLAMD_BIAS_BORDER_CLASSES, forward launches behind a folded BatchNorm, see
 *   clamd_bn_fold_bias below) = `bias` is a [9][Cout_p] table indexed by the border class of the output pixel.  Bit 1 is taken by
 *   clamd_conv3x3 where clamd_conv3x3_border_bias_ok() says so (the persistent kernel), by clamd_conv3x3_winograd24 and by
 *   clamd_conv3x3_winograd24_direct_filters; every other entry point rejects it. */
enum { CLAMD_RELU = 1, CLAMD_BIAS_BORDER_CLASSES = 2 };
int clamd_conv3x3(const void* x, int x_ldc, const void* w_packed, const float* bias, void* y, int y_ldc,
                  float* stats, const void* bn_y, float* bn_sums, int stat_rows, int B, int H, int W, int Cin_p, int Cout_p,
                  int relu, int m_fastest, int dtype, const clamd_tuning* tune, void* stream);
int clamd_conv3x3_border_bias_ok(int B, int H, int W, int Cin_p, int Cout_p, int dtype, const clamd_tuning* tune);
/* How many of the five sums a PLAIN (no bias, ReLU, statistics) clamd_conv3x3 launch with bn_y / bn_sums takes: 5, or 2 where the
 * persistent bf16 kernel runs it (channels-in-the-lane epilogue: sum g and sum g y as running sums per accumulator register; rows
 * k = 2..4 are written as NaN -- clamd_bn_bwd_finalize with dbias != NULL on such rows returns NaN bias gradients instead of silent zeros --
 * and the convolution's bias gradient comes from clamd_bn_bwd_apply_sums, below).  0 on bad arguments. */
int clamd_conv3x3_bn_sums(int B, int H, int W, int Cin_p, int Cout_p, int dtype, const clamd_tuning* tune);
/* ---- nn.BatchNorm2d folded into the nn.Conv2d(k3,p1) behind it (models/unet.py:15-16,30-31; bnfold.hip) ---------------------
 * x = scale * r + shift with r the producer's saved conv+ReLU output and scale / shift from clamd_bn_finalize:
 *   conv3x3(x, W) = conv3x3(r, W * scale[ci]) + the sum of T[co][tap] = sum_ci W[co][ci][tap] * shift[ci] over the taps that read
 *   inside the image (nn.Conv2d pads x, not r, with zeros) -- nine border classes: 3 * (0 top row, 1 interior, 2 bottom row) +
 *   (0 left column, 1 interior, 2 right column); H, W >= 2.
 * The caller packs the filters with `kscale` = scale (PackJob / WinoPackJob, ops.PackTable / ops.WinoPackTable), fills the table
 * with clamd_bn_fold_bias (table[class][co] = bias[co] + sum of T over the class's valid taps; padded channels 0) and launches
 * the convolution on r with relu | CLAMD_BIAS_BORDER_CLASSES: the clamd_bn_apply pass over the producer's output is not needed.
 * Weight gradient (trainer.py:175): run the weight-gradient entry point on r instead of x, then clamd_bn_fold_wgrad in place:
 *   dW[co][ci][tap] = scale[ci] * dW[co][ci][tap] + shift[ci] * S[tap][co],  S = sum of gz over the pixels whose tap reads inside
 *   the image = sum_gz (the convolution's bias gradient, as clamd_bn_bwd_finalize writes it) - border row - border column + corner,
 *   the border sums taken here from gz in a fixed order.  dw = [Cout][Cin][3][3] fp32 (the parameter's own layout); workspace >=
 *   clamd_bn_fold_wgrad_workspace_bytes(B, Cout_p).  The data gradient (w.r.t. x) is unchanged. */
int clamd_bn_fold_bias(const float* w, const float* shift, const float* bias, float* table, int Cout, int Cin, int Cout_p, void* stream);
/* the filter pack of that convolution and its bias table in ONE launch (both sit between the producer's clamd_bn_finalize and the
 * convolution, on the critical path of the forward pass): form 0 = clamd_pack(jobs_dev, njobs, total_blocks, dtype), 16 =
 * clamd_wino_pack, 24 = clamd_wino24_pack, with the blocks of clamd_bn_fold_bias appended to the grid (taps = 9).
 * The 1x1 head behind the last BatchNorm (models/unet.py:70-72) folds the same way without border classes: taps = 1 (form 0), w
 * [Cout][Cin], table = one row [Cout_p] = bias + W . shift; its weight gradient on the un-normalised tensor is fixed up by
 * clamd_bn_fold_wgrad_pointwise: dW[co][ci] = scale[ci] * dW[co][ci] + shift[ci] * sum_g[co] (sum_g = the head's bias gradient). */
int clamd_bn_fold_pack(int form, const void* jobs_dev, int njobs, int total_blocks, int dtype, const float* w, int taps, const float* shift,
                       const float* bias, float* table, int Cout, int Cin, int Cout_p, void* stream);
int clamd_bn_fold_wgrad_pointwise(const float* sum_g, const float* scale, const float* shift, float* dw, int Cout, int Cin, void* stream);
size_t clamd_bn_fold_wgrad_workspace_bytes(int B, int Cout_p);
int clamd_bn_fold_wgrad(const void* gz, int gz_ldc, const float* sum_gz, const float* scale, const float* shift, float* dw,
                        void* workspace, size_t ws_bytes, int B, int H, int W, int Cout_p, int Cout, int Cin, int dtype, void* stream);
/* The same convolution (fp32 only; H, W even) by Winograd F(2x2,3x3): 2.25x fewer multiply-adds, fp32 transforms
 * (relative error vs fp64 3.5e-7 against 2.3e-7 for the direct sum).  w_wino = [Cin_p/8][16][Cout_p][8] written by
 * clamd_wino_pack (jobs: device table of WinoPackJob, see ops.WinoPackTable; the data gradient uses the tap-flipped,
 * transposed filter).  Epilogue: bias, ReLU, BN statistics as clamd_conv3x3 (wino.hip). */
int clamd_sizeof_wino_pack_job(void);
int clamd_wino_pack(const void* jobs_dev, int njobs, int total_blocks, void* stream);
int clamd_conv3x3_winograd(const float* x, int x_ldc, const float* w_wino, const float* bias, float* y, int y_ldc,
                           float* stats, int stat_rows, int B, int H, int W, int Cin_p, int Cout_p, int relu,
                           const clamd_tuning* tune, void* stream);
/* The same convolution by the hybrid Winograd F(2x4,3x3) (fp32 only; H even, W a multiple of 4): F(2,3) down the rows, F(4,3)
 * along the columns -- 3 multiply-adds per output instead of 4 (F(2x2)) or 9 (direct); fp32 error vs fp64 1e-6.
 * w_wino = [Cin_p/8][24][Cout_p][8] written by clamd_wino24_pack (same job table as clamd_wino_pack).  Arguments and epilogue
 * as clamd_conv3x3_winograd; stat_rows = clamd_stat_rows(CLAMD_OP_CONV3X3_WINOGRAD24, ...) (wino24.hip). */
int clamd_wino24_pack(const void* jobs_dev, int njobs, int total_blocks, void* stream);
int clamd_conv3x3_winograd24(const float* x, int x_ldc, const float* w_wino, const float* bias, float* y, int y_ldc,
                             float* stats, int stat_rows, int B, int H, int W, int Cin_p, int Cout_p, int relu,
                             const clamd_tuning* tune, void* stream);
/* Weight gradient of the same convolution by the hybrid F(2x4,3x3) (fp32; H even, W a multiple of 4): 24 instead of 32
 * (F(2x2)) or 72 (direct) multiply-adds per 8 output pixels; arguments as clamd_wgrad_winograd (wino24_wgrad.hip). */
size_t clamd_wgrad_winograd24_workspace_bytes(int Rp, int Cp);
int clamd_wgrad_winograd24(const float* gz, int gz_ldc, const float* x, int x_ldc, float* workspace, size_t ws_bytes, float* out,
                           int B, int H, int W, int Rp, int Cp, int R, int C, int r_seg0, int r_seg0p, int c_seg0, int c_seg0p,
                           const clamd_tuning* tune, void* stream);
/* ---- F(2x4,3x3) with PRE-TRANSFORMED operands (wino24g.hip): the wide (>= 256-channel) 3x3 convolutions of
 * models/unet.py:28-33,50-55 (enc3.4, enc4, dec1, dec2, dec3) and their gradients (trainer.py:175).
 * clamd_conv3x3_winograd24 forms B^T d B inside the K loop of every output-slab workgroup; here it is formed ONCE per
 * tensor (clamd_winograd24_transform_input: x [B,H,W,ldc] -> v, clamd_winograd24_input_elems() floats, 3x the
 * activation) and clamd_conv3x3_winograd24_pre runs a transform-free K loop (48 MFMAs + 18 buffer loads straight into
 * the operand registers, no LDS, no VALU) on the SAME packed filters, tile grid, epilogue and statistics rows:
 * bit-identical to clamd_conv3x3_winograd24.  Needs Cin_p % 32 == 0, Cin_p >= 64, Cout_p % 64 == 0.
 * scale / shift (optional, [Cp] each): the transform reads x * scale + shift instead of x -- the nn.BatchNorm2d in front of the
 * convolution (models/unet.py:15-16,30-31: clamd_bn_finalize's scale / shift on the producer's conv+ReLU output) folded into
 * the load, with the zero padding applied AFTER the affine as nn.Conv2d does; the clamd_bn_apply pass of that unit is then not
 * needed when nothing else reads its output. */
size_t clamd_winograd24_input_elems(int B, int H, int W, int Cp);
int clamd_winograd24_transform_input(const float* x, int x_ldc, const float* scale, const float* shift, float* v, int B, int H, int W,
                                     int Cp, void* stream);
int clamd_conv3x3_winograd24_pre(const float* v, const float* w_wino, const float* bias, float* y, int y_ldc,
                                 float* stats, int stat_rows, int B, int H, int W, int Cin_p,
                                 int Cout_p, int relu, const clamd_tuning* tune, void* stream);
/* The narrow layers (64 / 128 channels, levels 0-1 of models/unet.py:49-72, where 3x the activation bytes through HBM would
 * cost more than the in-kernel transform): clamd_conv3x3_winograd24 with the FILTER fragments loaded straight into the MFMA
 * operand registers instead of being staged through LDS (wino24h_kernel, wino24g.hip).  Same arguments, same packed filters,
 * bit-identical results and statistics rows; needs Cout_p % 64 == 0 and Cin_p % 32 == 0. */
int clamd_conv3x3_winograd24_direct_filters(const float* x, int x_ldc, const float* w_wino, const float* bias, float* y, int y_ldc,
                                            float* stats, int stat_rows, int B, int H, int W,
                                            int Cin_p, int Cout_p, int relu, const clamd_tuning* tune, void* stream);
/* Weight gradient of the same convolution as a batched GEMM over the 24 Winograd planes (K = tiles) on operands transformed
 * once: v = the forward image of the convolution INPUT (clamd_winograd24_transform_input, kept from the forward pass: it is
 * read in place as the x-side operand), yt = caller-provided scratch of clamd_wgrad_winograd24_pre_operand_elems(B,H,W,Rp)
 * floats for A4 dY A6^T of gz ([24][tiles][Rp], written here).  Every wave owns a 128 x 128 block of one plane (16 MFMAs per
 * two 16-byte loads, no LDS); split-K slabs in `workspace` (>= clamd_wgrad_winograd24_pre_workspace_bytes), fixed-order
 * reduce with G4^T . G6: deterministic.  Rp and Cp multiples of 128 (round 5; multiples of 256 before); other arguments as
 * clamd_wgrad_winograd24. */
size_t clamd_wgrad_winograd24_pre_operand_elems(int B, int H, int W, int Rp);
/* the gradient-side transform alone (a caller with several streams can run it beside another launch's GEMM); clamd_wgrad_winograd24_pre
 * with gz == NULL then takes yt as already transformed */
int clamd_wgrad_winograd24_pre_transform(const float* gz, int gz_ldc, float* yt, int B, int H, int W, int Rp, void* stream);
size_t clamd_wgrad_winograd24_pre_workspace_bytes(int B, int H, int W, int Rp, int Cp);
int clamd_wgrad_winograd24_pre(const float* gz, int gz_ldc, const float* v, float* yt, float* workspace, size_t ws_bytes, float* out,
                               int B, int H, int W, int Rp, int Cp, int R, int C, int r_seg0, int r_seg0p, int c_seg0, int c_seg0p,
                               const clamd_tuning* tune, void* stream);
/* ---- F(4x4,3x3) with PRE-TRANSFORMED operands (wino44g.hip): the wide 3x3 convolutions at 32x32 and 64x64 of models/unet.py:28-33,
 * 50-55 (enc3, enc4, dec2, dec3) and their gradients (trainer.py:175).  36 multiply-adds per 4 x 4 outputs = 2.25 per output against 3
 * (F(2x4)) and 9 (direct); fp32 error vs fp64 2-3.5e-6 relative.  H and W multiples of 4.  The same call structure as the F(2x4) family
 * above, argument for argument:
 *   clamd_wino44_pack                   filters G6 g G6^T as [Cin_p/8][36][Cout_p][8] (same job table as clamd_wino_pack)
 *   clamd_winograd44_transform_input    x [B,H,W,ldc] (optionally x * scale + shift, zero padding after the affine) -> v,
 *                                       clamd_winograd44_input_elems() floats = 2.25x the activation
 *   clamd_conv3x3_winograd44_pre        transform-free K loop (per wave 24 MFMAs + 12 buffer loads into the operand registers per
 *                                       8-channel chunk; 12 waves per workgroup: six Winograd rows x two 32-channel halves), bias, ReLU,
 *                                       statistics rows (stat_rows = clamd_stat_rows(CLAMD_OP_CONV3X3_WINOGRAD44, ...)); Cout_p % 64 == 0
 *   clamd_wgrad_winograd44_pre[_transform|_operand_elems|_workspace_bytes]   weight gradient as the batched plane GEMM of
 *                                       clamd_wgrad_winograd24_pre over 36 planes: v = the kept forward image, yt = A6 dY A6^T scratch,
 *                                       fixed-order reduce with G6^T . G6 (deterministic); Rp, Cp multiples of 128 (256 x 256 workgroup blocks where both are
 *                                       multiples of 256, 128 x 128 wave blocks dealt k-step by k-step otherwise) */
int clamd_wino44_pack(const void* jobs_dev, int njobs, int total_blocks, void* stream);
size_t clamd_winograd44_input_elems(int B, int H, int W, int Cp);
int clamd_winograd44_transform_input(const float* x, int x_ldc, const float* scale, const float* shift, float* v, int B, int H, int W,
                                     int Cp, void* stream);
int clamd_conv3x3_winograd44_pre(const float* v, const float* w_wino, const float* bias, float* y, int y_ldc,
                                 float* stats, int stat_rows, int B, int H, int W, int Cin_p,
                                 int Cout_p, int relu, const clamd_tuning* tune, void* stream);
size_t clamd_wgrad_winograd44_pre_operand_elems(int B, int H, int W, int Rp);
int clamd_wgrad_winograd44_pre_transform(const float* gz, int gz_ldc, float* yt, int B, int H, int W, int Rp, void* stream);
size_t clamd_wgrad_winograd44_pre_workspace_bytes(int B, int H, int W, int Rp, int Cp);
int clamd_wgrad_winograd44_pre(const float* gz, int gz_ldc, const float* v, float* yt, float* workspace, size_t ws_bytes, float* out,
                               int B, int H, int W, int Rp, int Cp, int R, int C, int r_seg0, int r_seg0p, int c_seg0, int c_seg0p,
                               const clamd_tuning* tune, void* stream);
/* Weight gradient of the same convolution by Winograd (fp32, H and W even): out [R][C][3][3] = G^T (sum over tiles of
 * (A dY A^T) x (B^T d B)) G; arguments as clamd_wgrad(CLAMD_WGRAD_CONV3, ...) (gz = d loss / d conv output, x = conv input). */
size_t clamd_wgrad_winograd_workspace_bytes(int Rp, int Cp);
int clamd_wgrad_winograd(const float* gz, int gz_ldc, const float* x, int x_ldc, float* workspace, size_t ws_bytes, float* out,
                         int B, int H, int W, int Rp, int Cp, int R, int C, int r_seg0, int r_seg0p, int c_seg0, int c_seg0p,
                         const clamd_tuning* tune, void* stream);
/* 1x1 convolution, NHWC output, same epilogue options as clamd_conv3x3 (bias, ReLU, BN statistics).  Used for the
 * data gradient of the head (unet.py:72) and, on an im2col'ed input (clamd_nchw_im2col3), for the first conv
 * enc1.0 (unet.py:50, Cin = 3).  w_packed [1][Cout_p][Cin_p]. */
int clamd_conv1x1(const void* x, int x_ldc, const void* w_packed, const float* bias, void* y, int y_ldc,
                  float* stats, const void* bn_y, float* bn_sums, int stat_rows, int B, int H, int W, int Cin_p, int Cout_p,
                  int relu, int dtype, void* stream);
/* the head nn.Conv2d(conv_dim, num_classes, k1) (unet.py:72): logits written as fp32 NCHW [B,num_classes,H,W]. */
int clamd_conv1x1_logits(const void* x, int x_ldc, const void* w_packed, const float* bias, float* logits_nchw,
                         int B, int H, int W, int Cin_p, int Cout_p, int num_classes, int dtype, void* stream);
/* The head with the arg-max over classes fused into its epilogue (eval forward, trainer.py:279 `torch.max(outputs, 1)`;
 * SURVEY.md §8f row 4): pred int64 [B,H,W], first maximum wins; logits_nchw may be NULL (the logits are then never written).
 * num_classes <= 64 and Cout_p <= 64 (the arg-max runs inside one 64-channel slab); anything else is refused with status -1, nothing launched. */
int clamd_conv1x1_argmax(const void* x, int x_ldc, const void* w_packed, const float* bias, long long* pred, float* logits_nchw,
                         int B, int H, int W, int Cin_p, int Cout_p, int num_classes, int dtype, void* stream);
/* nn.ConvTranspose2d(k2,s2)+bias (unet.py:34): x [B,h,w,Cin_p] -> y [B,2h,2w,(ldc)] channels [0,Cout_p) of the
 * slice y points at.  w_packed [4][Cout_p][Cin_p] (tap q = 2*dy+dx). */
int clamd_convT2x2_fwd(const void* x, int x_ldc, const void* w_packed, const float* bias, void* y, int y_ldc, int B,
                       int h, int w, int Cin_p, int Cout_p, int dtype, void* stream);
/* data gradient of the above: gy [B,2h,2w,...] -> gx [B,h,w,Cin_p].  w_packed [Cin_p][4][Cout_p]. */
int clamd_convT2x2_dgrad(const void* gy, int gy_ldc, const void* w_packed, void* gx, int gx_ldc, const void* bn_y,
                         float* bn_sums, int stat_rows, int B, int h, int w, int Cin_p, int Cout_p, int dtype, void* stream);

/* ---- weight gradients (wgrad.hip) --------------------------------------------------------------------------
 * out[r][c][t] = sum_pixels a[p, r] * b[nbr_t(p), c]  written in the parameter's own fp32 layout:
 *   CONV3: a = d(conv output), b = conv input  -> d weight [Cout][Cin][3][3]
 *   PW   : a = d logits,       b = head input  -> d weight [K][Cin][1][1]
 *   UP2  : a = convT input,    b = d(convT output) -> d weight [Cin][Cout][2][2]
 * R,C logical sizes.  Physical channel p maps to logical p (p < seg0p and p < seg0), to padding (seg0 <= p < seg0p),
 * or to seg0 + (p - seg0p): concat inputs keep each half padded separately; a single segment is (seg0, seg0p) =
 * (logical size, physical size).  workspace: fp32 split-K slabs, size >= clamd_wgrad_workspace_bytes(). */
size_t clamd_wgrad_workspace_bytes(int mode, int B, int H, int W, int Rp, int Cp, int dtype);
int clamd_wgrad(int mode, const void* a, int a_ldc, const void* b, int b_ldc, float* workspace, size_t ws_bytes,
                float* out, int B, int H, int W, int Rp, int Cp, int R, int C, int r_seg0, int r_seg0p, int c_seg0,
                int c_seg0p, int dtype, const clamd_tuning* tune, void* stream);

/* ---- BatchNorm / ReLU / MaxPool / concat plumbing (elementwise.hip) ------------------------------------------
 * nn.BatchNorm2d train mode (unet.py:15): partial rows stats[stat_rows][2][Cp] -> scale/shift (+ running stats,
 * momentum 0.1, unbiased var); rows are added in a fixed order in fp64, mean/variance formed in fp64.
 * stats == NULL: eval mode, normalise with the running statistics.  num_batches_tracked (optional, int64 scalar): nn.BatchNorm2d's
 * counter, incremented in train mode (stats != NULL).
 * Checked on the host, before any launch (status -1, clamd_last_error() names the check), for clamd_bn_finalize, clamd_bn_apply,
 * clamd_bn_bwd_reduce, clamd_bn_bwd_finalize and clamd_bn_bwd_apply: every pointer the selected kernel reads or writes is non-NULL, every
 * pitch of a tensor that is passed is >= Cp, B, H, W > 0, pooling has even H and W.  Optional (may be NULL): stats (eval mode, which then
 * needs running_mean and running_var), running_mean / running_var in train mode (both or neither), num_batches_tracked, pooled, gp, ga
 * where gp is given, dbias, and scale / shift of the backward launches without gp. */
int clamd_bn_finalize(const float* stats, int stat_rows, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, float* scale, float* shift, float* save_mean, float* save_istd,
                      int Cp, int C, double count, double momentum, double eps, long long* num_batches_tracked, void* stream);
/* out = y*scale+shift into `out` (possibly a concat slice: replaces torch.cat, unet.py:83-87); pooled (optional)
 * = nn.MaxPool2d(2,2) of out (unet.py:12,80). */
int clamd_bn_apply(const void* y, int y_ldc, const float* scale, const float* shift, void* out, int out_ldc,
                   void* pooled, int p_ldc, int B, int H, int W, int Cp, int dtype, void* stream);
/* backward of ReLU->BatchNorm (+ max-pool routing of `gp`, the gradient w.r.t. the pooled tensor):
 * reduce -> partial rows sums[sum_rows][5][Cp] (sum_rows = clamd_stat_rows(CLAMD_OP_BN_BWD_REDUCE, ...)),
 * finalize -> k0,k1,k2 + d gamma, d beta, d conv-bias, apply -> g_z. */
int clamd_bn_bwd_reduce(const void* ga, int ga_ldc, const void* gp, int gp_ldc, const void* y, int y_ldc,
                        const float* scale, const float* shift, float* sums, int sum_rows, int B, int H, int W, int Cp,
                        int dtype, const clamd_tuning* tune, void* stream);
int clamd_bn_bwd_finalize(const float* sums, int sum_rows, const float* gamma, const float* save_mean, const float* save_istd,
                          float* k012, float* dgamma, float* dbeta, float* dbias, int Cp, int C, double count,
                          void* stream);
int clamd_bn_bwd_apply(const void* ga, int ga_ldc, const void* gp, int gp_ldc, const void* y, int y_ldc,
                       const float* scale, const float* shift, const float* k012, void* gz, int gz_ldc, int B,
                       int H, int W, int Cp, int dtype, void* stream);
/* Two-sum form (the persistent bf16 convolution kernel, see clamd_conv3x3_bn_sums): the producing data-gradient launch wrote only
 * sum g and sum g y (rows k = 0, 1; k = 2..4 NaN), which is all k0, k1, k2, d gamma and d beta need; pass dbias = NULL to
 * clamd_bn_bwd_finalize and take the convolution's bias gradient (models/unet.py:13,16: d conv-bias = sum of g_z) where g_z is formed:
 * clamd_bn_bwd_apply_sums = clamd_bn_bwd_apply without pooling + partial rows gz_rows[nrows][Cp] of sum g_z (nrows =
 * clamd_bn_bwd_apply_sums_rows(B, H, W, Cp), one row per workgroup, plain stores), then clamd_rows_sum adds rows 0..nrows-1 in a
 * fixed order in fp64 and OVERWRITES out[0..C). */
int clamd_bn_bwd_apply_sums_rows(int B, int H, int W, int Cp);
int clamd_bn_bwd_apply_sums(const void* ga, int ga_ldc, const void* y, int y_ldc, const float* k012, void* gz, int gz_ldc,
                            float* gz_rows, int nrows, int B, int H, int W, int Cp, int dtype, void* stream);
int clamd_rows_sum(const float* rows, int nrows, float* out, int Cp, int C, void* stream);
/* Eval-mode form (nn.BatchNorm2d.eval(): normalised with the running statistics, clamd_bn_finalize with stats == NULL): scale and shift
 * are constants, so g_z = [y>0] * scale * g needs no reduction in front of it and the backward is ONE streaming pass.
 * clamd_bn_bwd_eval reads ga (+ the pooled gradient gp, routed to the first maximum of scale * y + shift of its window, as
 * clamd_bn_bwd_apply) and y, writes g_z (channels C..Cp-1 as zero) and partial rows rows[nrows][3][Cp] of sum g, sum g y and sum g_z
 * (nrows = clamd_bn_bwd_eval_rows(B, H, W, Cp, gp != NULL), one row per workgroup, plain stores).
 * clamd_bn_bwd_eval_finalize adds rows 0..nrows-1 in a fixed order in fp64: d gamma = save_istd * (sum g y - save_mean * sum g),
 * d beta = sum g, d conv-bias = sum g_z.  nsums = 3: rows of clamd_bn_bwd_eval; nsums = 5: the five-sum rows of a producing launch
 * (clamd_conv3x3 / clamd_conv1x1 / clamd_convT2x2_dgrad with bn_sums), d conv-bias = scale * sum g [y>0] -- dbias = NULL for the two-sum
 * form, whose bias gradient comes from clamd_bn_bwd_apply_sums.  k012 (optional) = (scale, 0, 0): the coefficients with which
 * clamd_bn_bwd_apply / clamd_bn_bwd_apply_sums form the eval-mode g_z from such rows.  save_mean / save_istd / scale: clamd_bn_finalize's
 * outputs of the forward.  No atomics: two runs are bit-identical. */
int clamd_bn_bwd_eval_rows(int B, int H, int W, int Cp, int pooled);
int clamd_bn_bwd_eval(const void* ga, int ga_ldc, const void* gp, int gp_ldc, const void* y, int y_ldc, const float* scale, const float* shift,
                      void* gz, int gz_ldc, float* rows, int nrows, int B, int H, int W, int Cp, int C, int dtype, void* stream);
int clamd_bn_bwd_eval_finalize(const float* rows, int nrows, int nsums, const float* scale, const float* save_mean, const float* save_istd,
                               float* k012, float* dgamma, float* dbeta, float* dbias, int Cp, int C, void* stream);
/* Synchronised BatchNorm (torch.nn.SyncBatchNorm): the statistics of a train-mode layer come from the whole global batch.  The partial rows
 * of one rank are added into fp64 totals, the caller all-reduces (SUM) the [2][Cp] + 1 doubles of `reduce` across ranks, and the *_total
 * finalizes read the result.  With one rank (or equal totals) the outputs are those of clamd_bn_finalize / clamd_bn_bwd_finalize on the
 * same rows, bit for bit.
 * clamd_bn_rows_total: rows[nrows][nk][Cp] (nk = 2: clamd_bn_finalize's statistics rows; nk = 5 = clamd_bn_bwd_nsums(): backward sums,
 * the two-sum form included) added in the fixed order of the finalize kernels -> totals[nk][Cp] (optional, this rank's own) and
 * reduce[0..2Cp) = totals k = 0, 1, reduce[2Cp] = count (optional; the buffer to all-reduce).  At least one of the two.
 * clamd_bn_finalize_total: clamd_bn_finalize in train mode from the all-reduced (sum x, sum x^2, count): scale / shift / save_mean /
 * save_istd, running statistics with the global count, num_batches_tracked += 1.
 * clamd_bn_bwd_finalize_total: clamd_bn_bwd_finalize with k0, k1, k2 from the all-reduced (sum g, sum g y, count) and d gamma, d beta,
 * d conv-bias from this rank's totals[5][Cp] (as torch: the parameter gradients are all-reduced with the others).  dbias = NULL: the
 * two-sum form (k = 2..4 unused). */
int clamd_bn_rows_total(const float* rows, int nrows, int nk, int Cp, double count, double* totals, double* reduce, void* stream);
int clamd_bn_finalize_total(const double* reduce, const float* gamma, const float* beta, float* running_mean, float* running_var,
                            float* scale, float* shift, float* save_mean, float* save_istd, int Cp, int C, double momentum, double eps,
                            long long* num_batches_tracked, void* stream);
int clamd_bn_bwd_finalize_total(const double* totals, const double* reduce, const float* gamma, const float* save_mean,
                                const float* save_istd, float* k012, float* dgamma, float* dbeta, float* dbias, int Cp, int C, void* stream);
/* nn.MaxPool2d(2,2) alone (models/unet.py:12: the first layer of a DownBlock run as a stand-alone block, blocks.py; inside the UNet step
 * the pool is part of clamd_bn_apply / clamd_bn_bwd_*): x [B,H,W,ldc] -> pooled [B,H/2,W/2,ldc]; backward: gx [B,H,W,ldc] = gp at the first
 * maximum of each window (the tie rule of clamd_bn_apply and of torch's CPU kernel), 0 elsewhere.
 * sign (optional, [Cp]): channels with sign[c] < 0 take the window MINIMUM instead -- the pool of a tensor scale * x + shift that is never
 * written (a BatchNorm folded into the consumers of the pooled tensor, see clamd_bn_fold_bias) taken on x: max(s x + t) = s min(x) + t. */
int clamd_maxpool2x2(const void* x, int x_ldc, const float* sign, void* pooled, int p_ldc, int B, int H, int W, int Cp, int dtype, void* stream);
int clamd_maxpool2x2_bwd(const void* x, int x_ldc, const float* sign, const void* gp, int gp_ldc, void* gx, int gx_ldc, int B, int H, int W, int Cp,
                         int dtype, void* stream);
/* out[c] = sum_pixels g[p,c]  (bias gradients of convT / head): per-block partial rows in `workspace`
 * (>= clamd_channel_sum_workspace_bytes(Cp)), then a fixed-order fp64 sum -- no float atomics, out is overwritten. */
size_t clamd_channel_sum_workspace_bytes(int Cp);
int clamd_channel_sum(const void* g, int ldc, float* out, long long npix, int Cp, int C, int dtype, float* workspace,
                      size_t ws_bytes, const clamd_tuning* tune, void* stream);
/* boundary layout conversion: visible tensors are fp32 NCHW; replaces images.to(device) layout
 * handling (trainer.py:168) and feeds grad_output into the backward. */
int clamd_nchw_to_nhwc(const float* src, void* dst, int ldc, int B, int C, int H, int W, int Cp, double mul,
                       int dtype, void* stream);
int clamd_nhwc_to_nchw(const void* src, int ldc, float* dst, int B, int C, int H, int W, int dtype, void* stream);
/* NCHW fp32 image -> NHWC with the 3x3 neighbourhood folded into channels: dst[p, c*9 + ky*3 + kx] (9*C <= Cp). */
int clamd_nchw_im2col3(const float* src, void* dst, int ldc, int B, int C, int H, int W, int Cp, int dtype, void* stream);

/* ---- parameters, metrics (misc.hip); the loss (loss.hip); the optimisers further down (optim.hip) ------------
 * clamd_pack: one fused launch re-packing every fp32 master parameter into the layouts above (job table built by
 * the host). */
int clamd_pack(const void* jobs_dev, int njobs, int total_blocks, int dtype, void* stream);
/* nn.CrossEntropyLoss() forward+backward (trainer.py:113,174-175) on fp32 NCHW logits / int64 labels, plus the
 * build-defined distillation term when old_logits != NULL.  loss3 = {total, ce, kd}. */
size_t clamd_ce_workspace_bytes(void);
/* byte offset inside the workspace of an unsigned int: pixels whose label is neither ignore_index nor a class (torch's
 * CrossEntropyLoss asserts on those; here they are left out of the mean and counted for the caller to check). */
size_t clamd_ce_bad_label_count_offset(void);
int clamd_ce_fwd_bwd(const float* logits, const long long* labels, const float* old_logits, int K_old_total, int c_old,
                     double temperature, double lam, float* dlogits, float* loss3, void* workspace, size_t ws_bytes,
                     int B, int K, int H, int W, long long ignore_index, double grad_scale, void* stream);
/* The same loss without the distillation term, in two launches that need no memset and no atomics: clamd_ce_count writes the count of
 * the pixels that take part in the mean as one partial pair per workgroup into the workspace (plain stores), the loss / gradient pass
 * (same workspace, ordered behind it by the caller) adds them.  Needs H * W % 4 == 0.  dl_nhwc (optional): d logits ALSO as
 * an NHWC tensor [B,H,W,dl_ldc] of compute dtype dl_dtype, channels K .. dl_ldc-1 zero (dl_ldc >= 32) -- the operand of the 1x1
 * head's data gradient (models/unet.py:72, trainer.py:175), which then needs no clamd_nchw_to_nhwc pass over d logits. */
int clamd_ce_count(const long long* labels, int B, int K, int H, int W, long long ignore_index, void* workspace, size_t ws_bytes, void* stream);
int clamd_ce_fwd_bwd_counted(const float* logits, const long long* labels, float* dlogits, void* dl_nhwc, int dl_ldc, int dl_dtype,
                             float* loss3, void* workspace, size_t ws_bytes, int B, int K, int H, int W, long long ignore_index,
                             double grad_scale, void* stream);
/* The class-incremental step (build-defined, parity unpinned: the reference has no continual-learning code; the two terms follow Cermelli
 * et al., "Modeling the Background for Incremental Learning in Semantic Segmentation", CVPR 2020).  Classes [0, c_old) are old, [c_old, K)
 * new, class 0 is background; LSE(S) = log sum_{k in S} exp(z_k), bgnew = {0} u [c_old, K).
 *   unbiased CE   -(LSE(old) - LSE(all)) for a label < c_old ("background or any old class"), -(z_y - LSE(all)) for a label >= c_old;
 *                 mean over the pixels whose label is not ignore_index and lies in [0, K) (others are counted as by clamd_ce_fwd_bwd)
 *   unbiased KD   q = softmax(old_logits[:, 0 .. c_old)), log p~_0 = LSE(bgnew) - LSE(all), log p~_k = z_k - LSE(all) for 1 <= k < c_old:
 *                 -(1 / c_old) sum_k q_k log p~_k, mean over ALL B * H * W pixels, times lam; no temperature
 * loss3 = {total, ce, kd}.  old_logits: [B, K_old_total, H, W] with K_old_total >= c_old; NULL or lam == 0: the CE term alone (kd = 0,
 * old_logits not read).  With c_old == 1 and no KD term the results equal clamd_ce_fwd_bwd_counted's bit for bit.  The workspace holds
 * clamd_ce_count's partial rows (same K, same stream, called before), as for clamd_ce_fwd_bwd_counted; dl_nhwc / dl_ldc / dl_dtype as
 * there.  One pass over four pixels per thread with 16-byte accesses when H * W % 4 == 0 and logits / old_logits / dlogits are 16-byte
 * and labels 32-byte aligned; any other size or alignment takes a one-pixel-per-thread variant of the same arithmetic inside this entry
 * point (same results, slower).  Enqueue only: no allocation, no synchronisation, no atomics (bit-reproducible), graph-capturable. */
int clamd_ce_unbiased_fwd_bwd(const float* logits, const long long* labels, const float* old_logits, int K_old_total, int c_old, double lam,
                              float* dlogits, void* dl_nhwc, int dl_ldc, int dl_dtype, float* loss3, void* workspace, size_t ws_bytes,
                              int B, int K, int H, int W, long long ignore_index, double grad_scale, void* stream);
/* ---- cross-entropy + soft Dice (loss.hip) ---------------------------------------------------------------------
 * Build-defined, parity unpinned (the reference trains with plain cross-entropy): the compound loss of nnU-Net and of MONAI's DiceCELoss.
 * Logits z fp32 NCHW [B,K,H,W], labels y int64 [B,H,W], 1 <= K <= 32.
 *   valid pixel   y != ignore_index and y in [0, K); invalid pixels contribute to nothing; a label that is neither ignore_index nor a
 *                 class is counted as a bad label, as by the clamd_ce_* entry points
 *   p             softmax(z) over the K classes of a pixel, in fp32, relative to the pixel's maximum
 *   group         per_image = 0: all images are one group (batch Dice, G = 1); per_image = 1: each image is a group (G = B)
 *   sums          per group g and class k over the valid pixels of g:  I = sum p_k [y = k],  P = sum p_k,  Y = sum [y = k] (an integer)
 *   class set     S_g = { k in [first_class, K) : not present_only or Y_gk > 0 };  first_class in {0, 1} (1 leaves the background out)
 *   Dice          N_gk = 2 I_gk + smooth,  D_gk = P_gk + Y_gk + smooth,  dice_gk = N_gk / D_gk  (D_gk == 0: dice_gk = 1, no gradient)
 *   L_dice        (1 / G) sum_g [ 1 - (1 / |S_g|) sum_{k in S_g} dice_gk ];  a group with empty S_g contributes 0 and no gradient
 *   CE            clamd_ce_fwd_bwd_counted's: the mean of -log p_y over the N valid pixels of the batch
 *   total         w_ce * CE + w_dice * L_dice;  loss3 = {total, w_ce * CE, w_dice * L_dice}, total the fp32 sum of the other two
 *   gradient      on a valid pixel of group g, with u = w_dice / (G |S_g|), for k in S_g:  c_gk = u N_gk / D_gk^2,  a_gk = -2 u / D_gk,
 *                 g_k = c_gk + [y = k] a_gk  (g_k = 0 outside S_g):
 *                 d total / d z_j = grad_scale * [ w_ce (p_j - [y = j]) / max(N, 1) + p_j (g_j - sum_k p_k g_k) ];   exactly 0 on invalid pixels
 * Four launches: a sums pass (logits and labels once; one partial row {I, P, Y, counts} per workgroup, plain stores, a workgroup inside one
 * image), a coefficient pass (the rows of each group added in a fixed order in fp64; N, D, |S|, {c, a} and the loss term in fp64; the table
 * [G][32][2] in fp32; the valid / bad totals, so no clamd_ce_count in front), a gradient pass (softmax recomputed; d logits in NCHW and,
 * with dl_nhwc, a second time as [B,H,W,dl_ldc] of dl_dtype, channels K .. dl_ldc-1 zero: clamd_ce_fwd_bwd_counted's contract byte for
 * byte) and a finalize.  Four pixels per thread with 16-byte logit and 32-byte label accesses when H * W % 4 == 0 and logits / dlogits are
 * 16-byte, labels 32-byte aligned; any other size or alignment takes a one-pixel variant of the same arithmetic inside the same entry
 * point.  Enqueue only: no allocation, no synchronisation, no memset, no float atomics (bit-reproducible), graph-capturable.
 * Workspace: clamd_ce_dice_workspace_bytes(B, K, H, W, per_image) bytes (0 for an invalid shape), 16-byte aligned; its first
 * clamd_ce_workspace_bytes() bytes are laid out as the CE workspace (clamd_ce_bad_label_count_offset() finds the bad-label counter, the
 * valid count sits in the word before it); the contents are otherwise undefined before and after.
 * Rejected before any launch: K outside [1, 32]; first_class outside {0, 1}; negative or non-finite w_ce, w_dice or smooth; dl_nhwc with
 * dl_ldc < 32; a workspace that is too small or unaligned; null logits / labels / dlogits / loss3 / workspace; B > 2048 (every image has a
 * partial row of its own and the coefficient pass adds at most 2048 rows; larger images share the 2048 rows, their workgroups loop). */
size_t clamd_ce_dice_workspace_bytes(int B, int K, int H, int W, int per_image);
int clamd_ce_dice_fwd_bwd(const float* logits, const long long* labels, float* dlogits, void* dl_nhwc, int dl_ldc, int dl_dtype,
                          float* loss3, void* workspace, size_t ws_bytes, int B, int K, int H, int W, long long ignore_index,
                          double w_ce, double w_dice, double smooth, int first_class, int present_only, int per_image,
                          double grad_scale, void* stream);
/* ---- class weights, label smoothing and the focal term (loss.hip) ---------------------------------------------
 * The generalised per-pixel cross-entropy: torch's F.cross_entropy(weight=, label_smoothing=, ignore_index=) and, build-defined, the focal
 * modulation of Lin et al. (ICCV 2017) with its exponent applied to q = 1 - p_y.
 * Logits z fp32 NCHW [B,K,H,W], labels y int64 [B,H,W], 1 <= K <= 32; class weights w fp32 [K], finite, each 0 or >= 1e-30 (grad_scale / D is
 * formed in fp32: a smaller positive D would overflow it; not checked here: a read-back would be needed; loss.py checks them when they are set); image weights nu fp32 [B], NULL = 1; eps = label_smoothing in [0, 1);
 * gamma = focal_gamma >= 0; eps > 0 and gamma > 0 together are rejected.
 *   valid pixel   y != ignore_index and y in [0, K); another non-ignore label is counted as a bad label, as by the clamd_ce_* entry points
 *   p = softmax(z),  p_y the target's probability,  q = sum_{k != y} p_k (summed, never 1 - p_y),  t = -log p_y,  W = sum_k w_k
 *   D     = sum_valid w_y                                 torch's denominator; NOT multiplied by nu, as clamd_ce_fwd_bwd_weighted keeps N
 *   nll   = sum_valid nu_b w_y q^gamma t
 *   smo   = sum_valid nu_b sum_k w_k (-log p_k)           a pixel whose own class weight is 0 keeps its smoothing term, as in torch
 *   loss  = ((1 - eps) nll + (eps / K) smo) / D;          loss3 = {loss, (1 - eps) nll / D, (eps / K) smo / D}, loss their fp32 sum
 *   f     = 1 (gamma == 0);  q^gamma (1 + gamma p_y t / q) (gamma > 0; t / q -> 1 as q -> 0)
 *   d loss / d z_k = grad_scale * nu_b / D * [ (1 - eps) w_y f (p_k - [k = y]) + (eps / K) (W p_k - w_k) ]     exactly 0 on invalid pixels
 * D == 0 (nothing valid, or every valid pixel on a class of weight 0): loss3 = {0, 0, 0} and every gradient exactly 0.  torch returns NaN
 * there; this library's convention is the max(N, 1) of the other criteria.
 * Four launches: a per-class count (one partial row {n_0 .. n_31, valid, bad} per workgroup: an integer histogram in LDS, plain stores), a
 * one-workgroup totals pass (the rows added; D = sum_k (double)w_k n_k and W in ascending k), the loss / gradient pass (clamd_ce_fwd_bwd_counted's
 * shape: four pixels per thread with 16-byte logit and 32-byte label accesses when H * W % 4 == 0 and logits / dlogits are 16-byte, labels
 * 32-byte aligned, else a one-pixel variant of the same arithmetic; dl_nhwc / dl_ldc / dl_dtype as there) and a finalize (both partial
 * columns in fp64 in a fixed order).  Enqueue only, counts for itself: no allocation, no synchronisation, no memset, no float atomics
 * (bit-reproducible), graph-capturable.
 * With every w_k == 1.0f, eps == 0 and gamma == 0 the results (d logits, the NHWC copy, loss3) equal clamd_ce_count +
 * clamd_ce_fwd_bwd_counted's bit for bit without image weights and clamd_ce_fwd_bwd_weighted's with them: the pixel's coefficient is
 * a = (grad_scale / (float)D) nu_b w_y, the gradient e_k (a / sum e) - [k = y] a.
 * Workspace: clamd_ce_class_workspace_bytes() bytes, 8-byte aligned; its first clamd_ce_workspace_bytes() bytes are laid out as the CE
 * workspace (clamd_ce_bad_label_count_offset() finds the bad-label counter, the valid count sits in the word before it).
 * Rejected before any launch: a null or misaligned class_weight; a misaligned image_weight; eps outside [0, 1); gamma negative or not
 * finite; eps and gamma both non-zero; a workspace that is too small or unaligned; everything clamd_ce_fwd_bwd_counted rejects but the
 * size and alignment that select the one-pixel variant. */
size_t clamd_ce_class_workspace_bytes(void);
int clamd_ce_class_fwd_bwd(const float* logits, const long long* labels, const float* class_weight, const float* image_weight, float* dlogits,
                           void* dl_nhwc, int dl_ldc, int dl_dtype, float* loss3, void* workspace, size_t ws_bytes, int B, int K, int H, int W,
                           long long ignore_index, double label_smoothing, double focal_gamma, double grad_scale, void* stream);
/* ---- pseudo-labelling of the old classes (pseudo.hip; its loss clamd_ce_fwd_bwd_weighted: loss.hip) -----------
 * Build-defined, parity unpinned (the reference has no continual-learning code): the classification half of PLOP (Douillard et al.,
 * CVPR 2021, section 3.2).  In a task-2 batch every pixel of an old class is labelled 0; the frozen old model labels the background
 * pixels it is confident about, the others are ignored, and each image's loss is scaled by the accepted share of its background.
 * Notation: zo = old_logits[:, 0:c_old] (fp32 NCHW; K_old_total >= c_old), NB = number of bins, ign = ignore_index.  Per pixel:
 *   c* = the LOWEST index of the maximum of zo over [0, c_old) (torch's arg-max tie rule);  q = softmax(zo);
 *   u = -(sum_k q_k ln q_k) / ln(c_old), in fp32 with the usual max-subtraction;  c_old == 1 gives u = 0, c* = 0;
 *   bin(u) = min(NB-1, floor(u * NB));  CANDIDATE pixels are exactly those with label == 0.
 * Calibration histogram: hist[c*][bin(u)] += 1 over the candidate pixels; int64 [c_old, NB], ADDED into what is there (several batches
 *   accumulate; the caller zeroes it once).
 * Thresholds (host side, integer arithmetic on the histogram): n_c = sum_j hist[c][j]; n_c == 0 gives tau_c = 0; otherwise j* is the
 *   smallest j with sum_{i<=j} hist[c][i] >= ceil(n_c / 2) and tau_c = (j* + 1) / NB: the per-class median entropy, rounded up to a bin edge.
 * Relabelling: a candidate is accepted iff u < tau_{c*} (strict); accepted: labels_out = c* (c* == 0 keeps it background); rejected:
 *   labels_out = ign; every other label (new classes, ign, out-of-range values, which the loss counts as bad labels) passes through
 *   unchanged.  labels_in is not modified.
 * Adaptive factor: per image b, n_bg[b] candidates and n_acc[b] accepted ones; nu_b = n_bg ? max(min_factor, float(n_acc) / float(n_bg)) : 1.
 * Image-weighted cross-entropy: N = number of pixels whose label is not ign and lies in [0, K) (unweighted, what clamd_ce_count counts);
 *   loss = (1 / max(N,1)) * sum_b nu_b * sum_{valid p in b} -log softmax(z_p)[y_p];
 *   d logits = nu_b * (softmax - onehot) / max(N,1) * grad_scale on valid pixels, 0 elsewhere;  loss3 = {total, ce, 0}.
 *   With every nu_b == 1.0f the results equal clamd_ce_fwd_bwd_counted's bit for bit (the same partial-row reduction order; the weight is
 *   multiplied in as one fp32 factor).
 * All three: enqueue only, no allocation, no host synchronisation, device taken from the stream; bit-reproducible (integer atomics only,
 * no float atomics).  c_old in [1, 32].  Four pixels per thread with 16-byte logit and 32-byte label accesses when H * W % 4 == 0 and the
 * logits are 16-byte / the labels 32-byte aligned; any other size or alignment takes a one-pixel variant of the same arithmetic inside the
 * same entry point.
 * clamd_pseudo_entropy_hist: c_old * nbins <= 8192.
 * clamd_pseudo_label: counts = unsigned int [B][2] = {n_bg, n_acc}, cleared by the entry point itself; image_weight = float [B] (nu_b), or
 *   NULL when the factor is not wanted; thresholds = device float [c_old]; B <= 4096.
 * clamd_ce_fwd_bwd_weighted: clamd_ce_fwd_bwd_counted's arguments plus image_weight (device, B floats, required); the workspace holds
 *   clamd_ce_count's partial rows (same K, same stream, called before), dl_nhwc / dl_ldc / dl_dtype and the bad-label counter as there. */
int clamd_pseudo_entropy_hist(const float* old_logits, int K_old_total, int c_old, const long long* labels, long long* hist, int nbins,
                              int B, int H, int W, void* stream);
int clamd_pseudo_label(const float* old_logits, int K_old_total, int c_old, const long long* labels_in, const float* thresholds,
                       long long* labels_out, unsigned int* counts, float* image_weight, double min_factor, int B, int H, int W,
                       long long ignore_index, void* stream);
int clamd_ce_fwd_bwd_weighted(const float* logits, const long long* labels, const float* image_weight, float* dlogits, void* dl_nhwc,
                              int dl_ldc, int dl_dtype, float* loss3, void* workspace, size_t ws_bytes, int B, int K, int H, int W,
                              long long ignore_index, double grad_scale, void* stream);
/* ---- Local POD distillation (pod.hip) -----------------------------------------------------------------------
 * Build-defined, parity unpinned (the reference has no continual-learning code): the distillation half of PLOP (Douillard et al., CVPR
 * 2021, section 3.1).  Multi-scale strip-pooled statistics of the new model's tensor are matched to the old model's.
 * Inputs: a = new tensor [B, Ca, H, W], b = old tensor [B, Cb, H, W], both fp32 NCHW; C compared channels, 1 <= C <= min(Ca, Cb); flags
 *   merge_extra, square, normalize; levels in {1, 2, 3}: k = 1, 2, 4 regions per side; H and W multiples of 2^(levels-1).
 * Channel view: channel c < C of b is b_c, of a it is a_c, except that with merge_extra channel 0 of a is m = a_0 + sum_{k=C}^{Ca-1} a_k,
 *   added in ascending k (the logits form: the old model's background against the new model's background plus its new classes).  Without
 *   merge_extra the channels >= C of a take no part.
 * Value: v = x^2 with square (for post-ReLU features; applied after the merge), else v = x.
 * Embedding of image n: at each level s (k = 2^s, h = H / k, w = W / k) and channel c
 *   row strips     r[s, c, y, j] = (1 / w) sum_{x in column segment j} v[c, y, x]        (H k values)
 *   column strips  q[s, c, i, x] = (1 / h) sum_{y in row segment i} v[c, y, x]           (k W values)
 *   concatenated over levels and channels: D = C (H + W) (2^levels - 1) entries.
 * Normalisation: with normalize e = emb / max(||emb||_2, 1e-12) per image, else e = emb.
 * Loss: loss1[0] = lam * (1 / B) sum_n ||e_a,n - e_b,n||_2.
 * Gradient: da [B, Ca, H, W] = grad_scale * d loss / d a, exact, all Ca channels written (the caller needs no memset): the channels >= C
 *   carry channel 0's gradient under merge_extra and zeros otherwise; an image whose distance is exactly 0 contributes gradient 0; none
 *   is taken with respect to b.  da == NULL: the loss alone (the same bits), nothing else written outside the workspace.
 * Three passes and a one-thread sum: the strip pass reads a and b once (16-byte accesses, four pixels per lane, when W % 4 == 0 and a, b
 *   are 16-byte aligned; a one-element variant of the same arithmetic inside the same entry point for any other width or alignment) and
 *   writes the finest level's unnormalised row sums per column slot and column sums per row band (a workgroup owns an image, a channel and
 *   a band of rows; the band split depends on the shape only); the finalize pass forms the coarser levels as fixed-order sums of those,
 *   the per-image norms, the distance (from the differences e_a - e_b, never from ||a||^2 + ||b||^2 - 2 a.b) and the normalisation
 *   Jacobian's dot product in fp64, and writes two coefficient tables Grow [B, C, H, kmax], Gcol [B, C, kmax, W] that fold every level,
 *   1 / w, 1 / h, the normalisation, lam / B and grad_scale; the gradient pass writes
 *   da[n, c, y, x] = (Grow[n, c, y, seg(x)] + Gcol[n, c, seg(y), x]) * (square ? 2 * value : 1) and reads a only with square.
 * No atomics, every element written whole with plain stores: bit-reproducible.  Enqueue only: no allocation, no synchronisation, the
 * device is the stream's (graph-capturable).  workspace: 16-byte aligned, at least clamd_pod_workspace_bytes(B, C, H, W, levels) bytes
 * (0 for an invalid shape), contents undefined afterwards.  levels outside 1..3, C outside [1, min(Ca, Cb)], a size that is not a
 * multiple of 2^(levels-1), a workspace too small, B > 32767: an error, nothing launched. */
size_t clamd_pod_workspace_bytes(int B, int C, int H, int W, int levels);
int clamd_local_pod_fwd_bwd(const float* a, int Ca, const float* b, int Cb, int C, int merge_extra, int square, int normalize,
                            int levels, double lam, float* da, float* loss1, void* workspace, size_t ws_bytes,
                            int B, int H, int W, double grad_scale, void* stream);
/* ---- exemplar replay (replay.hip) ----------------------------------------------------------------------------
 * Build-defined, parity unpinned (the reference has no continual-learning code): rehearsal -- a small on-device memory of exemplars from
 * finished tasks, mixed into every batch of the new task.  Which image goes to which slot is the host's policy (replay.assign_slots); the
 * three entries count, store and assemble.  Notation: K = number of classes, 1 <= K <= 255; ign = ignore_index; images fp32 NCHW
 * [B, C, H, W], labels int64 [B, H, W]; the store holds `cap` slots: store_images [cap, C, H, W] as uint8 (store_fp32 == 0) or fp32
 * (store_fp32 == 1), store_labels uint8 [cap, H, W].
 * Stored label: ign -> 255; a label in [0, K) -> itself; anything else -> 255 and counted in *bad.  Read back: 255 -> ign, else itself.
 * Stored uint8 pixel, in fp32 arithmetic: u = clamp(rintf((x * 0.5f + 0.5f) * 255.f), 0, 255) (round to nearest even; a NaN gives 0).
 *   Read back with clamd_voc_prepare's arithmetic: v = (float)u / 255.f; x = (v - 0.5f) / 0.5f.  encode(decode(u)) == u for every byte, so
 *   an image that came from clamd_voc_prepare survives the store bit for bit; any other x in [-1, 1] comes back within 1 / 255 (half a
 *   quantisation step in x units).  fp32 storage copies the bits.
 * clamd_class_pixel_counts: counts = int [B][K], cleared by the entry point itself; counts[b][k] = number of pixels of image b with label
 *   k.  Labels equal to ign are skipped; any other label outside [0, K) is skipped and ADDED to *bad (unsigned int [1], the caller zeroes
 *   it).  A workgroup takes (image, chunk of pixels) jobs with a histogram in LDS and adds it to the image's row with integer atomics: the
 *   result does not depend on the order.  32-byte label loads when H * W % 4 == 0 and labels is 32-byte aligned, one label per load else.
 * clamd_replay_store: store slot slot[r] = batch image src[r] (pixels and labels, encoded as above) for r in [0, n); src and slot are DEVICE
 *   int [n], 1 <= n <= cap.  The slots of one call must be distinct (two rows writing one slot would interleave), which the host checks
 *   before the launch along with 0 <= src[r] < B and 0 <= slot[r] < cap; the kernel moves nothing for an r that violates the ranges and adds
 *   1 to *bad for it.  *bad also takes the labels that were neither ign nor in [0, K).  The images and labels are not modified.
 * clamd_replay_mix: out_images [B + R, C, H, W], out_labels [B + R, H, W].  Rows [0, B) are bit-copies of cur_images / cur_labels.  Row
 *   B + r is exemplar slots[r] (DEVICE long long [R]) read back as above and flipped by flips[r] (DEVICE int [R], or NULL for no flips):
 *   bit 0 reverses W, bit 1 reverses H, for the image and the labels alike.  A slot outside [0, cap) gives a zero image and all-ign labels
 *   and adds 1 to *bad: a guard, not an expected path.  B == 0 with NULL cur_images / cur_labels is the plain gather; R == 0 the plain
 *   copy; B + R >= 1.  out must not overlap any input.
 * The two copies: a lane handles four consecutive pixels (one 4-byte access per uint8 channel, 16 bytes per fp32 channel, two 16-byte label
 *   accesses; a W flip reverses the four pixels inside the lane and mirrors the group index) when W % 4 == 0 and the bases are aligned --
 *   fp32 tensors 16 bytes, int64 labels 32 bytes, uint8 tensors 4 bytes --; a one-pixel variant of the same arithmetic inside the same entry
 *   point for any other width or alignment (fp32 needs 4, int64 8 bytes at least).
 * All three: enqueue only, no allocation, no host synchronisation, device taken from the stream; integer atomics only, no float atomics:
 * bit-reproducible. */
int clamd_class_pixel_counts(const long long* labels, int* counts, unsigned int* bad, int B, int K, int H, int W, long long ignore_index,
                             void* stream);
int clamd_replay_store(const float* images, const long long* labels, const int* src, const int* slot, int n, void* store_images,
                       unsigned char* store_labels, int store_fp32, int cap, unsigned int* bad, int B, int C, int H, int W, int K,
                       long long ignore_index, void* stream);
int clamd_replay_mix(const float* cur_images, const long long* cur_labels, int B, const void* store_images, const unsigned char* store_labels,
                     int store_fp32, int cap, const long long* slots, const int* flips, int R, float* out_images, long long* out_labels,
                     unsigned int* bad, int C, int H, int W, long long ignore_index, void* stream);
/* ---- training augmentation (augment.hip) ----------------------------------------------------------------------
 * Build-defined, parity unpinned (the reference stops at Pad + CenterCrop + Normalize): random scale, crop or pad, and horizontal flip of
 * a batch and its labels in one launch.  images fp32 [B, C, H, W] -> out_images of the same shape, labels int64 [B, H, W] -> out_labels;
 * either pair may be NULL (both members), not both pairs.  params: DEVICE long long [B][4] = {step, y0, x0, flags}.  step is the source
 * pitch per output pixel in Q16 (65536 = scale 1), accepted in [2^13, 2^19] (scale 8 ... 1/8); (y0, x0) the Q16 source coordinate of output
 * pixel (0, 0); flags bit 0 the horizontal flip.  H, W <= 4096.
 * Definition -- every coordinate in 64-bit integers, hence exact.  Output pixel (i, j'), j = flip ? W - 1 - j' : j':
 *   sy = y0 + i * step, sx = x0 + j * step;  inside <=> 0 <= sy + 32768 < H * 65536 and 0 <= sx + 32768 < W * 65536.
 *   label = inside ? labels[b][(sy + 32768) >> 16][(sx + 32768) >> 16] (copied verbatim, no class check) : ignore_index.
 *   image = fill (converted to fp32) when not inside; inside: fy = sy >> 16 (arithmetic shift), wy = (float)(sy & 65535) * 2^-16, rows
 *   clamp(fy, 0, H - 1) and clamp(fy + 1, 0, H - 1), the columns alike from sx; with the four taps a b / c d:
 *   top = a + wx * (b - a), bot = c + wx * (d - c), out = top + wy * (bot - top) in fp32 (the compiler may contract into fma).
 * That is resize(bilinear, align_corners = False) for the image and nearest-exact for the labels, then crop or pad, then flip; the image's
 * fill region and the labels' ignore region are the same pixels by construction.  step == 65536 with y0 == x0 == 0 returns the input's bits
 * (both weights are 0; the formula is evaluated all the same, so a -0.0 may come back as +0.0 and an infinity or NaN reaches the pixels
 * whose taps include it).
 * A step outside the range gives an all-fill image and all-ignore_index labels for that row and adds 1 to *bad (unsigned int [1], the caller
 * zeroes it): a guard like clamd_replay_mix's, not an expected path.
 * A lane owns four consecutive output pixels of a row (one 16-byte store per channel, two 16-byte label stores; the row's and the four
 * pixels' coordinates formed once for all channels) when W % 4 == 0 and the OUTPUT bases are aligned -- out_images 16 bytes, out_labels 32
 * bytes --; a one-pixel instantiation of the same arithmetic inside the same entry point for any other width or alignment (fp32 needs 4,
 * int64 8 bytes at least).  The taps are 4-byte gathers on either path.  out must not overlap any input.
 * Enqueue only: no allocation, no host synchronisation, device taken from the stream; no atomics except the guard's integer add:
 * bit-reproducible.  An empty problem, H or W above 4096, an input without its output or the reverse, a misaligned tensor: an error, nothing
 * launched. */
int clamd_augment_batch(const float* images, const long long* labels, const long long* params, int B, int C, int H, int W,
                        float* out_images, long long* out_labels, double fill, long long ignore_index, unsigned int* bad, void* stream);
/* torch.optim.Adam.step over all parameters in one launch (trainer.py:108-110,176); hyper/step/derived live on the
 * device so a captured graph can be replayed with a new learning rate.  l2_accum_dev (optional, with the L2-to-old-weights
 * term): 1 + nchunks floats, [0] = sum ||theta - theta_old||^2 of this step, [1..] = per-workgroup partials added in a fixed
 * order (no float atomics: the value is bit-reproducible). */
int clamd_adam_step(const void* tensors_dev, const void* chunks_dev, int nchunks, const float* hyper_dev, int* step_dev,
                    float* derived_dev, float* l2_accum_dev, void* stream);
/* The same step with the elastic-weight-consolidation term (build-defined, like the L2 term: the reference has neither):
 * g += lam_ewc * omega * (theta - theta_old) on top of 2 * l2_lambda * (theta - theta_old); one anchor (the `old` pointer of the
 * unchanged 48-byte Adam table, required here) serves both.  importance_dev: device array of one `const float*` per table row,
 * omega >= 0 of the row's shape.  lam_ewc = hyper_dev[6] (device memory: a replayed graph sees a changed value).
 * ewc_accum_dev: 1 + nchunks floats, [0] = sum omega (theta - theta_old)^2 of this step, reduced like l2_accum_dev (fixed order, no
 * float atomics, bit-reproducible); l2_accum_dev (optional): sum (theta - theta_old)^2 as in clamd_adam_step.  36 B / parameter.
 * A step without consolidation keeps calling clamd_adam_step: its kernel is untouched. */
int clamd_adam_step_consolidated(const void* tensors_dev, const void* importance_dev, const void* chunks_dev, int nchunks,
                                 const float* hyper_dev, int* step_dev, float* derived_dev, float* ewc_accum_dev, float* l2_accum_dev,
                                 void* stream);
/* dst = decay * dst + scale * (power == 2 ? src * src : src) over every tensor of a device table of clamd_sizeof_importance_tensor()-byte
 * rows {float* dst; const float* src; long long n}, in ONE launch through a (tensor, chunk) job list as the Adam step uses (chunks of
 * clamd_adam_chunk_elems() elements).  The three passes of the Fisher-diagonal estimate: accumulate g*g (decay 1, scale 1, power 2,
 * src = the gradient), normalise (decay 1/N, scale 0, src = dst) and the online merge (decay gamma, scale 1, power 1, src = the new
 * importance; or, kept in the new one, decay 1, scale gamma, src = the previous importance).  decay and scale must be finite and >= 0.  Enqueue only: no allocation, no synchronisation, no atomics; element-wise,
 * so bit-reproducible.  12 B / element; dst and src need 4-byte alignment only (16-byte accesses from dst's first 16-byte boundary). */
int clamd_importance_accum(const void* tensors_dev, const void* chunks_dev, int nchunks, double decay, double scale, int power, void* stream);
/* torch.optim.SGD.step (dampening 0, maximize off) over all parameters in one launch, with the two build-defined pulls of the Adam steps
 * added to the gradient in the same place.  Per element, in this order:
 *   g = grad * grad_scale;  g += (weight_decay * decay_mult) * p;
 *   d = p - old;  g += 2 * l2_lambda * d;  g += ewc_lambda * omega * d;      (rows with an anchor; omega only with importance_dev)
 *   buf = mu * buf + g;                                                       (rows with a momentum buffer)
 *   u = nesterov ? g + mu * buf : (buf ? buf : g);  p -= lr * u.
 * tensors_dev: clamd_sizeof_sgd_tensor()-byte rows {float* p; const float* g; float* buf (null: no momentum); const float* old (null: no
 * anchor); long long n; float decay_mult; float pad}; chunks_dev: the (tensor, chunk) job list of clamd_adam_step, chunks of
 * clamd_adam_chunk_elems() elements.  importance_dev (optional): device array of one `const float*` per row, omega >= 0 of the row's
 * shape.  hyper_dev: device fp32[8] = lr, mu, weight_decay, nesterov (0 or 1), grad_scale, l2_lambda, ewc_lambda, 0 (device memory: a
 * replayed graph sees a changed value).  ewc_accum_dev (required with importance_dev, refused without): 1 + nchunks floats, [0] = sum
 * omega d^2 of this step; l2_accum_dev (optional): [0] = sum d^2; both reduced as in clamd_adam_step (fixed order, no float atomics,
 * bit-reproducible).  20 B / parameter with momentum, 12 B without, +4 B with an anchor, +4 B with importance.  Every pointer needs
 * 4-byte alignment only (16-byte accesses from p's first 16-byte boundary); nothing outside [0, n) of a row is touched.  Enqueue only:
 * no allocation, no synchronisation, no process state. */
int clamd_sizeof_sgd_tensor(void);
int clamd_sgd_step(const void* tensors_dev, const void* importance_dev, const void* chunks_dev, int nchunks, const float* hyper_dev,
                   float* ewc_accum_dev, float* l2_accum_dev, void* stream);
/* Synaptic Intelligence (Zenke et al. 2017; build-defined like the two pulls): the steps above with the path integral accumulated in the
 * same launch.  Per element, on top of clamd_adam_step[_consolidated] / clamd_sgd_step:
 *   omega += -(grad * grad_scale) * (p_new - p_old)
 * with the gradient as handed over -- before weight decay and both pulls -- and the fp32 values the kernel read and stored, so the
 * per-step differences telescope to theta_end - theta_start.  path_dev (required): device array of one `float*` per table row, omega of
 * the row's shape, read and written with 4-byte alignment only; nothing outside [0, n) of a row is touched.  importance_dev (optional):
 * as in clamd_adam_step_consolidated (every row then needs an anchor) / clamd_sgd_step, with ewc_accum_dev required beside it and refused
 * without it; l2_accum_dev optional.  The row structs are unchanged.  Adam 36 B / parameter (44 B with importance); SGD 28 B with
 * momentum, 20 B without, +4 B with an anchor, +4 B with importance.  p, m, v / buf and the penalty sums are what the untracked entry
 * points compute (to rounding where the compiler may contract differently).  Enqueue only: no allocation, no synchronisation, no atomics,
 * no process state. */
int clamd_adam_step_tracked(const void* tensors_dev, const void* importance_dev, const void* path_dev, const void* chunks_dev, int nchunks,
                            const float* hyper_dev, int* step_dev, float* derived_dev, float* ewc_accum_dev, float* l2_accum_dev,
                            void* stream);
int clamd_sgd_step_tracked(const void* tensors_dev, const void* importance_dev, const void* path_dev, const void* chunks_dev, int nchunks,
                           const float* hyper_dev, float* ewc_accum_dev, float* l2_accum_dev, void* stream);
/* The task boundary of the path integral: importance = decay * importance + max(0, path) / ((p - start)^2 + xi) over every tensor of a
 * device table of clamd_sizeof_path_tensor()-byte rows {float* importance; const float* path; const float* p; const float* start; long
 * long n}, in ONE launch through the (tensor, chunk) job list of clamd_importance_accum.  path, p and start are only read.  decay must be
 * finite and >= 0 (1: Zenke's running sum), xi finite and > 0 (also as fp32).  20 B / element; every pointer needs 4-byte alignment only
 * (16-byte accesses from importance's first 16-byte boundary).  Enqueue only: no allocation, no synchronisation, no atomics; element-wise,
 * so bit-reproducible. */
int clamd_sizeof_path_tensor(void);
int clamd_path_importance(const void* tensors_dev, const void* chunks_dev, int nchunks, double decay, double xi, void* stream);
/* Clipping by the global gradient norm (torch.nn.utils.clip_grad_norm_, norm_type 2, error_if_nonfinite off) without rewriting a gradient:
 * one pass reads every gradient once and the steps above are then launched on hyper_eff, whose grad_scale carries the coefficient.
 * tensors_dev: ntensors rows of clamd_sizeof_grad_tensor() = 24 bytes {const float* g; long long n; int first_chunk; int nchunks}, where
 * [first_chunk, first_chunk + nchunks) are the row's jobs in chunks_dev, the (tensor, chunk) job list of clamd_adam_step (chunks of
 * clamd_adam_chunk_elems() elements, a tensor's chunks consecutive).  hyper_dev: the fp32[8] of the step that follows; gs = hyper_dev[4].
 * Launch 1 (one workgroup per job, 4 B / parameter): partials[job] = sum of g[i]^2 over the job's chunk (nchunks floats).
 * Launch 2 (one workgroup): per tensor the sum of its partials, then the sum of those, both in fp64 and in a fixed order, and
 *   tensor_norms[t] (optional, ntensors floats) = fp32(sqrt(sum_t) * |gs|)
 *   clip_out[0] = fp32(norm), norm = sqrt(total) * |gs|: the norm of the gradient the step consumes
 *   clip_out[1] = coef = fp32(min(1, max_norm / (norm + 1e-6))), a NaN norm giving a NaN coefficient
 *   clip_out[2] = fp32(gs) * coef, one fp32 product
 *   clip_out[3] = 1 when norm is infinite or NaN, else 0
 *   hyper_eff[0..7] = hyper_dev[0..7] with slot 4 replaced by clip_out[2].
 * max_norm > 0; infinity measures without clipping (coef == 1 exactly for a finite norm).  The gradients are only read, with 4-byte
 * alignment only (16-byte loads from g's first 16-byte boundary); nothing outside [0, n) of a row is touched.  No float atomics:
 * bit-reproducible.  Enqueue only: no allocation, no synchronisation, nothing read back, no process state. */
int clamd_sizeof_grad_tensor(void);
int clamd_grad_norm_clip(const void* tensors_dev, int ntensors, const void* chunks_dev, int nchunks, const float* hyper_dev, double max_norm,
                         float* partials, float* clip_out, float* tensor_norms, float* hyper_eff, void* stream);
/* argmax over classes + confusion matrix (trainer.py:183-188, metrics.py:32-38). */
int clamd_argmax_confusion(const float* logits, const long long* labels, long long* pred, unsigned long long* conf,
                           int B, int K, int Kc, int H, int W, void* stream);
/* Data path: Pad(10)+CenterCrop+ToTensor+Normalize(0.5,0.5) of an interleaved uint8 RGB image
 * (main.py:18-23) -> image_out fp32 [3,h,w]; Pad+CenterCrop+voc.to_mask of the RGB mask (datasets/voc.py:56-72,
 * 140-142) -> label_out int64 [h,w] (void -> 0).  (oy, ox): source coordinate of output pixel (0,0).  Pixels whose
 * colour is not in the palette are counted in *bad_count (the reference raises ValueError) and set to 0. */
int clamd_voc_prepare(const unsigned char* img_rgb, const unsigned char* mask_rgb, float* image_out, long long* label_out,
                      int Hs, int Ws, int oy, int ox, int h, int w, unsigned int* bad_count, void* stream);
/* voc.to_rgb (datasets/voc.py:74-89): labels int64 [N,H,W] -> palette colours [N,3,H,W] (0..255 as float). */
int clamd_label_to_rgb(const long long* labels, float* rgb, long long n_img, long long hw, void* stream);
int clamd_fill_f32(float* p, long long n, double v, void* stream);
/* `ncus` workgroups (1..256) that each keep one whole CU (96 KB of LDS) for `usec` microseconds of wall clock and touch no memory:
 * what an RCCL channel workgroup does to the one-workgroup-per-CU kernels of this library during a collective (trainer.py:120-122
 * becomes one process per GPU, ddp.py).  The data-parallel host code uses it with ncus = 1 to MEASURE how many hardware queues the
 * runtime multiplexes its streams onto (ddp.hw_queues); tools/cu_steal.py rehearses held CUs with it. */
int clamd_hold_cus(int ncus, int usec, void* stream);
/* Gradient exchange in bf16 (replaces the reduce of nn.DataParallel, trainer.py:120-122, for BASELINE.json configs[2]/[4]
 * "bf16 DDP"): a bucket of the flat fp32 gradient buffer rounded to bf16 (rne) for the RCCL all-reduce and widened back.
 * A bucket may start at any element: the bf16 buffer must sit at the same element phase, (address / element size) % 8. */
int clamd_f32_to_bf16(const float* src, void* dst_bf16, long long n, void* stream);
int clamd_bf16_to_f32(const void* src_bf16, float* dst, long long n, void* stream);
/* p[i] *= *scale_dev for a DEVICE scalar, nothing at all when it is exactly 1 (the upstream gradient loss.backward()
 * hands to the loss function, trainer.py:175): no host sync, no pass over d logits in the common case. */
int clamd_scale_by_device_scalar(float* p, long long n, const float* scale_dev, void* stream);
/* ... and for an NHWC tensor of a compute dtype (n logical elements, a multiple of 8; the second copy of d logits above); also_f32
 * (optional, n_f32 elements): an fp32 tensor scaled by the same launch. */
int clamd_scale_by_device_scalar_nhwc(void* p, long long n, int dtype, const float* scale_dev, float* also_f32, long long n_f32, void* stream);

#ifdef __cplusplus
}
#endif
#endif
