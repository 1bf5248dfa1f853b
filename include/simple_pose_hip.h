/*
 * simple_pose_hip.h - C ABI of libsimple_pose_hip.so (MI355X / gfx950 only).
 *
 * The upstream reference (liangheming/simple_pose) has no native code and no FFI: its hot path is
 * reached through Python objects that call torch.nn.functional.  This header is the boundary a
 * maintainer would bind instead (ctypes stubs in INTEGRATION.md); every entry point names the
 * reference lines it replaces.  Conventions:
 *
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller
 *     (the library never allocates, frees or retains pointers past the call);
 *   - asynchronous on the caller's `hipStream_t` passed as `void* stream`; no implicit device sync;
 *   - returns SP_OK (0) or a negative SP_E* code; sp_last_error() gives the message of the last
 *     failure on the calling thread; nothing throws or aborts across the boundary;
 *   - activations are fp32 NHWC inside the network (channels % 4 == 0); the public tensors keep
 *     the reference's NCHW fp32 layout (input [B,3,H,W], heat maps [B,J,H,W]).
 */
#ifndef SIMPLE_POSE_HIP_H
#define SIMPLE_POSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SP_OK 0
#define SP_EINVAL (-1)   /* bad argument / unsupported shape (message in sp_last_error) */
#define SP_ELAUNCH (-2)  /* HIP launch or runtime failure */

#define SP_ABI_VERSION 36

/* epilogue / layout flags of sp_conv_desc.flags */
#define SP_CONV_RELU 0x1u          /* y = max(y, 0) after scale/shift (+ residual) */
#define SP_CONV_OUT_NCHW 0x2u      /* store y as NCHW [B, N, out_h, out_w] (final_layer -> heat maps) */
#define SP_CONV_PIXEL_SHUFFLE 0x4u /* fused nn.PixelShuffle(2): weights packed with sp_pack order, see below */
#define SP_CONV_OUT_F32 0x10u      /* with SP_CONV_BF16: NHWC y and residual are fp32 (activation gradients in the bf16
                                      train step keep fp32 until the BatchNorm backward has removed their mean) */
#define SP_CONV_BN_Y_MASK 0x20u    /* sp_conv2d_dgrad_bn_bwd_stats* / sp_conv2d_dgrad_phases with bf16 activations AND gradients: `bn_y` is the
                                    * ReLU bit mask sp_bn_fold_apply_nhwc / sp_bn_apply_nhwc left (one byte per 8 channels), not the tensor y */
#define SP_CONV_BF16 0x8u          /* x, w_packed, residual and NHWC y are bf16 (fp32 accumulate; scale/shift and the NCHW
                                      output stay fp32); c_in % 8 == 0, k_pad % 64 == 0 */
#define SP_CONV_HARDSWISH 0x40u    /* y = h(acc * scale + shift) (+ residual, added AFTER h: the YOLOv5 BottleNeck shortcut), h(v) = v * min(max(v + 3, 0), 6) / 6
                                    * in torch's operation order (nn.Hardswish).  fp32 implicit-GEMM launches only (kernel 0, no SP_CONV_RELU, NHWC output);
                                    * every other kernel structure and every *_ok predicate refuses it */
#define SP_CONV_OUT_SLICE 0x80u    /* y is the channel slice [c0, c0 + c_out) of an NHWC tensor with out_c channels per pixel; the caller passes y already
                                    * offset by c0 elements (c0 % 4 == 0: 16-byte aligned).  out_c % 4 == 0, c_out % 4 == 0, c_out <= out_c, no residual.
                                    * fp32 implicit-GEMM launches only.  (Without the flag out_c must equal c_out, as before.)  Producers of a concat
                                    * write their slices of one buffer - torch.cat without a copy */

/*
 * One launch of the fp32 implicit-GEMM convolution family:
 *   rows    M = batch * grid_h * grid_w      (output pixels of one phase)
 *   columns N = c_out
 *   depth   K = taps_h * taps_w * c_in       (zero taps allowed through k_pad)
 *   x[b, iy, ix, c] with iy = gy * stride + dy0 + ty * dy_step  (same for x), zero outside the image
 *   y[b, gy * oy_mul + oy_add, gx * ox_mul + ox_add, n] = act(acc * scale[n] + shift[n] + res[...])
 * A stride-s conv with padding p is (dy0 = -p, dy_step = +1, oy_mul = 1, oy_add = 0); output phase
 * (py,px) of ConvTranspose2d(k=4, s=2, p=1) is a 2x2-tap launch with (stride = 1, dy0 = py,
 * dy_step = -1, oy_mul = 2, oy_add = py).  `w` is packed [phases][n_pad][k_pad] fp32, K contiguous,
 * K ordered (ty, tx, c) - see sp_conv_weight_index().
 */
typedef struct sp_conv_desc {
    int32_t batch, in_h, in_w, c_in; /* x: NHWC [batch, in_h, in_w, c_in], c_in % 4 == 0 */
    int32_t grid_h, grid_w;          /* logical output grid per phase */
    int32_t c_out;                   /* N (real) */
    int32_t n_pad;                   /* packed rows per phase: multiple of 32, >= c_out (extra rows are zero) */
    int32_t taps_h, taps_w;          /* taps as stored in the packed weights (taps_w may exceed the real kw) */
    int32_t k_pad;                   /* packed K per row: multiple of 32, >= taps_h*taps_w*c_in */
    int32_t stride;
    int32_t dy0, dy_step, dx0, dx_step;
    int32_t out_h, out_w, out_c;     /* y: NHWC [batch, out_h, out_w, out_c] (or NCHW with SP_CONV_OUT_NCHW) */
    int32_t oy_mul, oy_add, ox_mul, ox_add;
    int32_t phases_y, phases_x;      /* 1,1 for conv; 2,2 for the k4s2p1 transposed conv (dy0/oy_add become per-phase) */
    uint32_t flags;
    int32_t tile_m, tile_n;          /* workgroup tile (rows x columns); 0,0 = sp_conv2d_default_tile().  Results do not
                                        depend on the tile: every output's K reduction order is the same for all shapes. */
    int32_t stride_x;                /* 0: same as `stride`.  Otherwise the x stride where it differs from the y stride (`stride`):
                                        the bf16 stem reads the 4-channel image as x-PAIRS of 8 values, where a stride of two
                                        pixels is a stride of one pair */
    int32_t kernel;                  /* SP_CONV_KERNEL_IGEMM (0, default), SP_CONV_KERNEL_RING / _RING_LW or SP_CONV_KERNEL_PW: which kernel structure runs the
                                        launch; same results bit for bit (same K order, same MFMA chain per output) */
    int32_t c_in_group;              /* 0: dense.  > 0 (ABI 33): grouped convolution with c_out == c_in (ResNeXt's conv2, nets/pose_resnet_dconv.py:101):
                                        an N tile of tile_n == c_in_group output channels reads only the c_in_group input channels of its own groups;
                                        k_pad = taps * c_in_group and the weights are packed by sp_pack_conv_weights_grouped (one block-diagonal panel
                                        [tile_n][k_pad] per N tile).  Implicit-GEMM kernel only, c_in_group a whole number of K tiles and of groups. */
} sp_conv_desc;

/* sp_conv_desc.kernel */
#define SP_CONV_KERNEL_IGEMM 0 /* 4-wave workgroups, register-staged double buffer: every dtype / flag / tile listed at sp_conv2d_default_tile */
#define SP_CONV_KERNEL_RING 1  /* bf16 only: persistent 8-wave workgroups fed by an LDS-DMA ring (buffer_load ... lds, counted vmcnt);
                                  tiles 256x256 256x128 128x256 256x64 128x128 192x128 192x256; needs sp_conv2d_ring_ok(desc) == 1 */
#define SP_CONV_KERNEL_RING_LW 3 /* the same ring with four extra "loader" waves per workgroup (one per SIMD) that issue every LDS-DMA piece; the eight
                                  MFMA waves only read fragments and multiply (round 5; same bits as 0 / 1); tiles 256x128 128x256 256x64 128x128
                                  192x128; needs sp_conv2d_ring_ok(desc) == 1 with desc.kernel set to this id */
#define SP_CONV_KERNEL_RING_LW4 4 /* (ABI 34) the loader-wave ring with FOUR MFMA waves, one per SIMD, instead of eight: the same workgroup tile as four wave
                                  * tiles of twice the area (fewer LDS fragment bytes per MFMA), and the 96-row tiles eight waves cannot cut; tiles
                                  * 192x128, 128x128, 96x128, 256x128, 128x256, 96x256, 64x128; same bits */
#define SP_CONV_KERNEL_PW 2    /* fp32 1x1 stride-1 NHWC layers with c_in 64 / 128 and c_out % 256 == 0 (bottleneck conv3, projection shortcut):
                                  one persistent workgroup per CU streams 64-row tiles, weights in registers (sp_conv2d_pw_ok); tile_m / tile_n unused */

/* ---- library ---------------------------------------------------------------------------------- */
int sp_abi_version(void);
const char* sp_last_error(void);

/* ---- network ops: replace torch.nn.functional calls inside nets/pose_resnet_dconv.py:251-265,
 *      nets/pose_resnet_duc.py (_forward_impl), nets/pose_hrnet.py:419-454 ------------------------ */

/* input [B,C,H,W] fp32 NCHW (C<=4) -> NHWC4 [B,H,W,4] (channel C..3 = 0); feeds conv1 (pose_resnet_dconv.py:158) */
int sp_nchw_to_nhwc4(const float* x_nchw, float* y_nhwc4, int batch, int channels, int h, int w, void* stream);

/* nn.Conv2d / nn.ConvTranspose2d(4,2,1) + folded eval-mode nn.BatchNorm2d (scale/shift) or bias (shift)
 * + residual add + nn.ReLU + nn.PixelShuffle(2), one kernel.  Replaces: conv1/bn1/relu (:252-254),
 * Bottleneck.forward (:112-133), deconv_layers (:230-249), final_layer (:173-178), DUC (nets/commons.py:36-41).
 * scale/shift: [c_out] or NULL (scale NULL -> 1, shift NULL -> 0); residual: same layout as y or NULL. */
int sp_conv2d_fwd(const sp_conv_desc* desc, const void* x, const void* w_packed, const float* scale,
                  const float* shift, const void* residual, void* y, void* stream);

/* Tap skipping (an addition to ABI 36).  An fp32 inference launch of sp_conv2d_fwd on the implicit-GEMM kernel with more than one tap, whole
 * K tiles per tap (c_in % 32 == 0), no groups, an NHWC store without pixel shuffle and batch >= tile_m / 2 orders its rows (output position,
 * image) and does not multiply the K tiles whose tap lies outside the image for every row of a tile (conv_igemm_tapskip_kernel).  Same bits
 * as the full K loop under one PRECONDITION: the packed weights are finite (a skipped product was +-0 * w; an inf / NaN weight made it NaN).
 * Activations may hold inf / NaN: an in-image value is never skipped.  sp_conv_set_tap_skip(0) restores the (image, position) row order and
 * the full K loop for every later launch of the process, sp_conv_set_tap_skip(1) turns the path back on; the environment variable
 * SP_CONV_TAP_SKIP=0 is the same switch read once, at the first launch.  Default: on. */
int sp_conv_set_tap_skip(int on);

/* Single LDS stage (an addition to ABI 36).  An fp32 inference launch of sp_conv2d_fwd on the implicit-GEMM kernel at tile 128x128 that would take
 * the plain instantiation (whole K tiles per tap: c_in % 32 == 0, at most 32 taps; no groups) or the tap-skipping one keeps ONE operand stage in
 * LDS instead of two (conv_igemm_single_kernel / conv_igemm_tapskip_single_kernel): 34,816 bytes instead of 67,584, so three workgroups are
 * resident per CU instead of two and a launch of 3 x CUs workgroups is one round, at the price of a second barrier per K tile.  Same MFMA
 * sequence per accumulator, same epilogue operations: same bits, no precondition.  The rule holds for every workgroup and K-tile count.
 * sp_conv_set_single_stage(0) keeps the double-buffered kernels for every later launch of the process, sp_conv_set_single_stage(1) turns the
 * form back on; the environment variable SP_CONV_SINGLE_STAGE=0 is the same switch read once, at the first launch.  Default: on.
 * sp_conv2d_kernel_name answers with the same strings whatever the knob says; sp_conv2d_single_stage returns 1 when a launch of `desc` would
 * take a single-stage kernel under the current knob, 0 when not (or when `desc` is invalid: sp_last_error).
 * sp_conv_igemm_resident_workgroups: the workgroups of a 128x128 kernel one CU holds at the LDS size its launcher passes (which: 0 = plain
 * double-buffered, 1 = tap-skipping double-buffered, 2 = plain single-stage, 3 = tap-skipping single-stage).  workgroups NULL: only the byte count
 * (no GPU needed). */
int sp_conv_set_single_stage(int on);
int sp_conv2d_single_stage(const sp_conv_desc* desc, int has_residual);
int sp_conv_igemm_resident_workgroups(int which, int* workgroups, int* lds_bytes);

/* Direct (non-im2col) 3x3 stride-1 pad-1 convolution for 32 -> 32 and 64 -> 64 channels in bf16 (HRNet's two high-resolution branches,
 * nets/pose_hrnet.py BasicBlock; ResNet-50 layer1.*.conv2): the halo tile of an 8x16 / 16x8 output tile goes through LDS once instead of
 * once per tap; the filter stays in registers (32 channels) or in LDS in MFMA-fragment order (64 channels) for a persistent workgroup.  Same arguments and bit-identical results as sp_conv2d_fwd for
 * the descriptors sp_conv3x3_direct_ok accepts (returns 1 / 0); tile fields are ignored. */
int sp_conv3x3_direct_ok(const sp_conv_desc* desc);
int sp_conv3x3_direct(const sp_conv_desc* desc, const void* x, const void* w_packed, const float* scale, const float* shift,
                      const void* residual, void* y, void* stream);

/* One HRNet BasicBlock (nets/pose_hrnet.py:34-51) of a 32-channel branch in ONE launch, bf16: y = relu(bn2(conv3x3(relu(bn1(conv3x3(x))))) + x).
 * `desc` describes either of the block's two convolutions (same geometry; sp_basic_block_c32_ok(desc) == 1: what sp_conv3x3_direct_ok
 * accepts at 32 channels); w1 / w2 packed as for sp_conv2d_fwd, scale / shift = the folded BatchNorms.  The intermediate stays in LDS
 * (rounded to bf16 exactly as the two-launch path stores it) and the residual comes from the input halo the workgroup already holds:
 * 2.5x less HBM traffic, bit-identical results.  y must not alias x. */
int sp_basic_block_c32_ok(const sp_conv_desc* desc);
int sp_basic_block_c32(const sp_conv_desc* desc, const void* x, const void* w1_packed, const float* scale1, const float* shift1,
                       const void* w2_packed, const float* scale2, const float* shift2, void* y, void* stream);

/* (ABI 35) The same block on a 64-channel branch (HRNet's 32 x 24 maps): both 64 x 576 filters stay in registers because the eight waves take roles - four
 * run conv1 of strip j while four run conv2 of strip j - 1 (4 x 24-pixel strips, one barrier per strip; csrc/conv_block64.hip).  Same arguments and
 * contract as sp_basic_block_c32 (`desc` = either convolution, sp_basic_block_c64_ok(desc) == 1: what sp_conv3x3_direct_ok accepts at 64 channels);
 * bit-identical to the two launches. */
int sp_basic_block_c64_ok(const sp_conv_desc* desc);
int sp_basic_block_c64(const sp_conv_desc* desc, const void* x, const void* w1_packed, const float* scale1, const float* shift1,
                       const void* w2_packed, const float* scale2, const float* shift2, void* y, void* stream);

/* (ABI 34) The tail of a stage-opening Bottleneck with 64 mid channels as ONE launch (bf16 NHWC, stride 1: layer1.0 of the ResNet pose nets and of HRNet):
 *     y = relu( bn3(conv1x1_{64->256}(a_main)) + bn_d(conv1x1_{64->256}(a_short)) )          nets/pose_resnet_dconv.py:99-103,120-131
 * a_main = the block's 3x3 output, a_short = the block input ([rows][64] each), weights packed by sp_pack_conv_weights ([256][64]), the folded
 * BatchNorms as (scale, shift).  Replaces the projection shortcut's launch + conv3's launch (the 256-channel shortcut tensor is neither written nor
 * read: 703 -> 301 MB at bs=128) with the same bits: the shortcut value is rounded to bf16 where the two-launch program stores it. */
/* sp_dual_pw_f32: the fp32 twin (csrc/conv_pw.hip; c_out a multiple of 256): 1,406 -> 602 MB at bs=128, the same bits as the two fp32 launches. */
int sp_dual_pw_bf16_ok(int64_t rows, int c_main, int c_short, int c_out);
int sp_dual_pw_f32_ok(int64_t rows, int c_main, int c_short, int c_out);
int sp_dual_pw_f32(const float* a_main, const float* w_main_packed, const float* scale_main, const float* shift_main, const float* a_short,
                   const float* w_short_packed, const float* scale_short, const float* shift_short, float* y, int64_t rows, int c_main, int c_short,
                   int c_out, int relu, void* stream);
int sp_dual_pw_bf16(const void* a_main, const void* w_main_packed, const float* scale_main, const float* shift_main, const void* a_short,
                    const void* w_short_packed, const float* scale_short, const float* shift_short, void* y, int64_t rows, int c_main, int c_short,
                    int c_out, int relu, void* stream);
/* conv3 of an identity-shortcut Bottleneck with 64 mid channels and the NEXT block's conv1 as ONE launch (fp32 NHWC, stride 1; csrc/conv_pw.hip):
 *     y = relu( bn3(conv1x1_{64->256}(t)) + residual ),   t_next = relu( bn1(conv1x1_{256->c_next}(y)) )      nets/pose_resnet_dconv.py:112-133
 * t [rows][64], residual / y [rows][256], t_next [rows][c_next], c_next = 64 or 128; weights packed by sp_pack_conv_weights ([256][64], [c_next][256]), the
 * folded BatchNorms as (scale, shift) or null.  The second product reads y from the workgroup's LDS tile instead of HBM (403 MB at bs=128); y is still
 * stored.  Same bits as the two sp_conv2d_fwd launches.  Neither output may alias an input or the other output. */
int sp_pw_chain_f32_ok(int64_t rows, int c_mid, int c_out, int c_next);
int sp_pw_chain_f32(const float* t, const float* w3_packed, const float* scale3, const float* shift3, const float* residual, float* y,
                    const float* w1_packed, const float* scale1, const float* shift1, float* t_next, int64_t rows, int c_mid, int c_out, int c_next,
                    void* stream);
/* One ResNet Bottleneck (nets/pose_resnet_dconv.py:112-133) with an identity shortcut, stride 1, 256 -> 64 -> 64 -> 256 channels, in ONE
 * launch, bf16: y = relu(bn3(conv1x1(relu(bn2(conv3x3(relu(bn1(conv1x1(x)))))))) + x).  `desc` describes the block's 3x3 convolution
 * (sp_bottleneck_c64_ok(desc) == 1: what sp_conv3x3_direct_ok accepts at 64 channels); w1 [>=64][256], w2 [>=64][576], w3 [256][64]
 * packed as for sp_conv2d_fwd, scale / shift = the folded BatchNorms.  x is read once (halo included) and y written once: 2.4x less
 * HBM traffic than the three launches; the intermediates are rounded to bf16 exactly where those store them: bit-identical results.
 * y must not alias x. */
int sp_bottleneck_c64_ok(const sp_conv_desc* desc);
int sp_bottleneck_c64(const sp_conv_desc* desc, const void* x, const void* w1_packed, const float* scale1, const float* shift1,
                      const void* w2_packed, const float* scale2, const float* shift2, const void* w3_packed, const float* scale3,
                      const float* shift3, void* y, void* stream);

/* The ResNet stem (nets/pose_resnet_dconv.py:158-162: conv1 7x7 s2 p3, bn1, relu, maxpool 3x3 s2 p1) in ONE launch, fp32 or bf16 compute:
 * x fp32 NCHW [batch,3,h,w] -> y NHWC [batch,hp,wp,64] (fp32, or bf16 when `bf16`), hp = ((h+6-7)/2+1 + 2-3)/2+1.  w_packed / k_pad: the
 * stem weights exactly as sp_conv2d_fwd takes them for conv1 (fp32: sp_pack_conv_weights with c_in_packed 4, taps_w_packed 8 ->
 * [64][224]; bf16: c_in_packed 8, taps_w_packed 4, pair_s0 1 -> [64][256]); scale / shift = the folded bn1.  The 128 x 96 x 64 map
 * between conv and pooling never reaches HBM and K is not padded to a GEMM tile: bit-identical to
 * sp_nchw_to_nhwc4[_bf16] -> sp_conv2d_fwd -> sp_maxpool3x3s2_nhwc[_bf16].  sp_stem7_pool_ok: the sizes the kernel's 32-bit offsets cover. */
int sp_stem7_pool_ok(int batch, int h, int w);
int sp_stem7_pool(const float* x, const void* w_packed, int k_pad, const float* scale, const float* shift, void* y, int bf16,
                  int batch, int h, int w, void* stream);
/* The same launch on uint8 BGR crops [batch,h,w,3] (what cv.warpAffine / sp_warp_affine_u8c3 produce): the collate normalisation of
 * datasets/coco.py:136 (`x / 255 - mean`, BGR -> RGB; mean_rgb_host = {0.485, 0.456, 0.406}) happens while the patch is loaded - the
 * arithmetic of sp_u8hwc_bgr_to_nhwc, same bits as that launch followed by sp_conv2d_fwd and sp_maxpool3x3s2_nhwc. */
int sp_stem7_pool_u8(const unsigned char* crops_bgr, const float* mean_rgb_host, const void* w_packed, int k_pad, const float* scale,
                     const float* shift, void* y, int bf16, int batch, int h, int w, void* stream);

/* HRNet's stem (nets/pose_hrnet.py:419-425: conv1 3x3 s2 + bn1 + relu, conv2 3x3 s2 + bn2 + relu) in ONE launch, bf16 compute:
 * x fp32 NCHW [batch,3,h,w] -> y bf16 NHWC [batch,h/4,w/4,64].  w1_packed / k1_pad: conv1's weights as sp_conv2d_fwd takes them on the bf16
 * NHWC4 image (sp_pack_conv_weights with c_in_packed 8, taps_w_packed 2, pair_s0 1 -> [64][64]); w2_packed: conv2's [64][576]; scale / shift:
 * the folded bn1 / bn2.  conv1's map never reaches HBM: bit-identical to sp_nchw_to_nhwc4_bf16 -> sp_conv2d_fwd -> sp_conv2d_fwd. */
/* HRNet transition1 as ONE launch (bf16; nets/pose_hrnet.py:327-366, used at :431-437): y_hi = relu(bn(conv3x3(x, 256 -> 32, stride 1, pad 1))),
 * y_lo = relu(bn(conv3x3(x, 256 -> 64, stride 2, pad 1))) from one staging of x [batch, h, w, 256] (h, w even).  wa_packed / wb_packed:
 * sp_pack_conv_weights layouts [32][k_pad] / [64][k_pad] with k_pad = 2304 = (tap, channel); scale / shift: folded BatchNorm (sp_fold_bn).
 * Replaces the two sp_conv2d_fwd launches of those layers; reduction order (64-channel chunk, tap, channel): equal to them up to fp32
 * summation order.  sp_hrnet_transition1_ok: whether (c_in, h, w) is a shape the kernel takes. */
int sp_hrnet_transition1_ok(int c_in, int h, int w);
int sp_hrnet_transition1(const void* x, int batch, int h, int w, const void* wa_packed, int k_pad, const float* scale_a, const float* shift_a,
                         const void* wb_packed, const float* scale_b, const float* shift_b, void* y_hi, void* y_lo, void* stream);
int sp_hrnet_stem_ok(int batch, int h, int w);
int sp_hrnet_stem(const float* x, const void* w1_packed, int k1_pad, const float* scale1, const float* shift1, const void* w2_packed,
                  const float* scale2, const float* shift2, void* y, int batch, int h, int w, void* stream);

/* 1 when `desc` can run with kernel = SP_CONV_KERNEL_PW (see there).  Same bits as the tiled kernel. */
int sp_conv2d_pw_ok(const sp_conv_desc* desc);

/* 1 when `desc` (flags, shapes, tile_m x tile_n) can run with kernel = SP_CONV_KERNEL_RING: bf16 NHWC in and out (ReLU, residual and
 * fused PixelShuffle allowed; no NCHW / fp32 output), c_in % 64 == 0, taps <= 32, k_pad / 64 >= the tile's ring depth, tile_n | n_pad. */
int sp_conv2d_ring_ok(const sp_conv_desc* desc);

/* Name of the kernel instantiation a launch of `desc` resolves to, as rocprofv3's kernel trace reports it (without the
 * "void (anonymous namespace)::" prefix and the argument list).  variant 0 = sp_conv2d_fwd, 1 = sp_conv2d_fwd_bn_stats,
 * 2 = sp_conv2d_dgrad_bn_bwd_stats, 3 = sp_conv3x3_direct, 4 = sp_basic_block_c32, 5 = sp_bottleneck_c64, 6 = sp_basic_block_c64 (`desc` = the
 * block's 3x3 convolution).  Produced by the launch dispatch itself (nothing is launched), so
 * profiles and bench.py's roofline line key on exactly what ran. */
int sp_conv2d_kernel_name(const sp_conv_desc* desc, int has_residual, int variant, char* buf, int cap);

/* The tile sp_conv2d_fwd picks when desc->tile_m == tile_n == 0; legal tiles: 128x128 64x128 128x64 64x64 256x64 128x32
 * (tile_n must divide n_pad).  Host code may time the legal tiles once per layer shape and pin the fastest. */
int sp_conv2d_default_tile(const sp_conv_desc* desc, int* tile_m, int* tile_n);

/* nn.MaxPool2d(3, 2, 1) on NHWC fp32 (pose_resnet_dconv.py:162,255) */
int sp_maxpool3x3s2_nhwc(const float* x, float* y, int batch, int h, int w, int c, void* stream);

/* nn.PixelShuffle(2) on NHWC fp32: x [B,h,w,c] -> y [B,2h,2w,c/4], y[b,2Y+i,2X+j,k] = x[b,Y,X,4k+2i+j]
 * (the bare shuffle that opens the DUC head, nets/pose_resnet_duc.py:228; the two DUC blocks fuse theirs into the conv) */
int sp_pixel_shuffle2_nhwc(const float* x, float* y, int batch, int h, int w, int c, void* stream);

/* SELayer (nets/commons.py:4-18; first block of each layer when reduction=True, pose_resnet_dconv.py:108-110,126-127):
 * squeeze y[b,c] = mean_hw x[b,hw,c]; the two 1x1 FCs run through sp_conv2d_fwd on the [B,1,1,C] tensor;
 * excite + block tail y = relu(x * sigmoid(gate_logits[b,c]) + identity). */
int sp_global_avg_pool_nhwc(const float* x, float* y, int batch, int hw, int c, void* stream);
int sp_se_gate_add_relu_nhwc(const float* x, const float* gate_logits, const float* identity, float* y, int batch, int hw,
                             int c, void* stream);

/* y = base + nearest_upsample(x, factor) (+ ReLU): x NHWC [B,h,w,c], base / y NHWC [B,h*f,w*f,c] (base may alias y;
 * factor 1 = plain add).  HighResolutionModule fuse sum, nets/pose_hrnet.py:192-202,250-257 */
int sp_upsample_add_nhwc(const float* x, const float* base, float* y, int batch, int h, int w, int c, int factor, int relu,
                         void* stream);
/* All upsampled terms of one HRNet fuse output in one pass (pose_hrnet.py:250-257, `y = y + fuse_layers[i][j](x[j])` for j >= i):
 * y = [relu](((base + up(xs[0], f0)) + up(xs[1], f1)) + up(xs[2], f2)), 1..3 terms, factor 1 = the identity term; xs[k] is
 * [batch, out_h / fk, out_w / fk, c] of the tensors' dtype (bf16 != 0: bf16, else fp32).  fp32: the bits of the chained sp_upsample_add_nhwc
 * launches; bf16: the sum is formed in fp32 and rounded once (the chain rounded after every term).  xs / factors: host arrays. */
int sp_upsample_add_n_nhwc(const void* base, int bf16, int n_terms, const void* const* xs, const int32_t* factors, void* y, int batch,
                           int out_h, int out_w, int c, int relu, void* stream);

/* bf16 NHWC (8 channels = 16 B per lane) variants of the layout / pooling / fuse kernels, for SP_CONV_BF16 networks.
 * The network input stays the reference's fp32 NCHW tensor; channels are padded to 8. */
int sp_nchw_to_nhwc8_bf16(const float* x_nchw, void* y_nhwc8, int batch, int channels, int h, int w, void* stream);
int sp_maxpool3x3s2_nhwc_bf16(const void* x, void* y, int batch, int h, int w, int c, void* stream);
int sp_pixel_shuffle2_nhwc_bf16(const void* x, void* y, int batch, int h, int w, int c, void* stream);
int sp_upsample_add_nhwc_bf16(const void* x, const void* base, void* y, int batch, int h, int w, int c, int factor,
                              int relu, void* stream);
/* SELayer (nets/commons.py:4-18) on bf16 tensors: squeeze (fp64 sums, bf16 result [B, c]) and excite + add + ReLU; gate_logits = the
 * bf16 output of the second FC (a 1x1 sp_conv2d_fwd on the [B,1,1,c] tensor) */
int sp_global_avg_pool_nhwc_bf16(const void* x, void* y, int batch, int hw, int c, void* stream);
int sp_se_gate_add_relu_nhwc_bf16(const void* x, const void* gate_logits, const void* identity, void* y, int batch, int hw,
                                  int c, void* stream);

/* ---- decoders: metrics/pose_metrics.py --------------------------------------------------------- */

/* BasicKeyPointDecoder.heat_map_to_axis (:11-24): coords [B,J,2], max_val [B,J] */
int sp_heat_map_to_axis(const float* heat_nchw, int batch, int joints, int h, int w, float* coords, float* max_val,
                        void* stream);
/* GaussTaylorKeyPointDecoder.__call__ (:62-107), kernel_size odd <= 15; trans_inv [B,2,3]; kps [B,J,2]; max_val [B,J].
 * One workgroup stages a whole map in LDS: with p = kernel_size / 2 and PW = ((ceil(w / 12) * 12 + kernel_size + 6) / 4) * 4 + 4 it needs
 * ((h + 2 p) * PW + h * w) * 4 B, at most 160 KiB less 32 B (more than 64 KiB is opted in per device on first use).  kernel_size 11:
 * 64x48 32,416 B, 96x72 (384x288 inputs) 66,656 B, 128x96 113,184 B; 160x120 (172,000 B) is refused with SP_EINVAL and the byte count.
 * sp_heat_map_to_axis and sp_decode_basic stage h * ceil(w / 4) * 16 B under the same limit.  A NaN tap stays a NaN through the clamp
 * (torch.clamp), so a map whose maximum is +inf decodes to NaN key points as in the reference. */
int sp_decode_gauss_taylor(const float* heat_nchw, const float* trans_inv, int batch, int joints, int h, int w,
                           int kernel_size, float* kps, float* max_val, void* stream);
/* BasicKeyPointDecoder.__call__ (:26-52) */
int sp_decode_basic(const float* heat_nchw, const float* trans_inv, int batch, int joints, int h, int w, float* kps,
                    float* max_val, void* stream);

/* HeatMapAcc.__call__ (:212-245) on the arg-max coordinates of predictions and targets (two sp_heat_map_to_axis calls):
 * acc_out = one device float, no host sync (the reference's .item() calls at :237 are gone).  mask [B,J] (may be NULL): the
 * solver evaluates maps multiplied by the joint mask (ddp...:130-131); a zero mask takes the joint out exactly as that does */
int sp_heat_map_acc(const float* pred_coords, const float* label_coords, const float* mask, int batch, int joints, int h, int w,
                    float distance_thresh, float norm_frac, float* acc_out, void* stream);

/* ---- input contract: datasets/coco.py:124-148 (collate_fn) -----------------------------------------
 * BGR u8 HWC crops [B,h,w,3] (device) -> RGB fp32 NCHW [B,3,h,w] = x/255 - mean_rgb[c] (no std division, coco.py:136);
 * mean_rgb_host: 3 floats in HOST memory */
int sp_u8hwc_bgr_to_nchw_f32(const unsigned char* img, float* out, int batch, int h, int w, const float* mean_rgb_host,
                             void* stream);

/* person crops from the full image: dst[n] = cv.warpAffine(src, m_fwd[n], (out_w, out_h), flags=INTER_LINEAR) for
 * `crops` forward (src -> dst) 2x3 float64 matrices (HOST memory; inverted on the host as OpenCV does) over one uint8 HxWx3 image; BORDER_CONSTANT 0; OpenCV's
 * fixed-point bilinear arithmetic restated (not pinned against cv2: it is absent from the build image) - naive_data.py:50 */
int sp_warp_affine_u8c3(const unsigned char* src, int src_h, int src_w, const double* m_fwd, int crops, unsigned char* dst, int out_h,
                        int out_w, void* stream);
/* training batches (commons/transforms.py RefineSimpleTransform.__call__ + datasets/coco.py collate_fn): sample n is
 * cv.warpAffine(flip[n] ? np.fliplr(src[n]) : src[n], m_fwd[n], (out_w, out_h), flags=INTER_LINEAR) - the pixels of sp_warp_affine_u8c3,
 * the flip mirrored at read time - normalised as sp_u8hwc_bgr_to_nchw_f32 does into out fp32 [batch,3,out_h,out_w] RGB.  srcs[n] (device
 * pointers to uint8 [H,W,3] BGR), src_hw [batch,2] (H, W each <= 32767), flip [batch] (NULL: no flip), m_fwd [batch,2,3] and mean_rgb are
 * HOST arrays; out and crops are device memory; crops (uint8 [batch,out_h,out_w,3] BGR, what sp_warp_affine_u8c3 writes) may be NULL. */
int sp_warp_affine_batch_u8c3_to_nchw_f32(const unsigned char* const* srcs, const int* src_hw, const int* flip, const double* m_fwd, int batch,
                                          int out_h, int out_w, const float* mean_rgb_host, float* out, unsigned char* crops, void* stream);

/* ---- after decode: result scores and per-image OKS-NMS -----------------------------------
 * kps_to_dict_ (metrics/pose_metrics.py:172-179): score[b] = mean_j(max_val[b,j]) + max_j(max_val[b,j]) */
int sp_pose_score(const float* max_val, int batch, int joints, float* score, void* stream);
/* eval.py:166-174: score[p] = box_score[p] * mean(kps[p,:,2][kps[p,:,2] > in_vis_thre]) (0 without a visible joint), float64 as
 * the reference computes after its JSON round trip; kps [P,J,3] = (x, y, max_val) fp32 from the decoder; kps64 (may be NULL)
 * receives the float64 copy sp_oks_nms consumes */
int sp_pose_rescore(const float* kps, const double* box_score, int persons, int joints, double in_vis_thre, double* kps64,
                    double* score, void* stream);
/* oks_nms (datasets/naive_data.py:153-173; oks_iou :120-150) for `groups` images in one launch; the persons of image g are
 * rows seg[g]..seg[g+1]-1 (seg: device int32 [groups+1]; max_group = the largest image, <= 2048, known to the host).
 * sigmas_host: `joints` doubles in HOST memory or NULL (COCO's 17); vis_thresh < 0 = in_vis_thresh None.
 * keep [P]: for image g the picked GLOBAL row indices in pick order at keep[seg[g]..], padded with -1; keep_count [groups].
 * Order: descending score, equal scores: higher index first (numpy's own tie order is unspecified). */
int sp_oks_nms(const double* kps, const double* scores, const double* areas, const int32_t* seg, int groups, int max_group,
               int joints, const double* sigmas_host, double thresh, double vis_thresh, int32_t* keep, int32_t* keep_count,
               void* stream);

/* ---- COCO keypoint AP / AR: what metrics/pose_metrics.py:182-209 (evaluate_map) and eval.py:13-27 (eval_kps) hand to
 * pycocotools' COCOeval(gt, dt, "keypoints") - loadRes, evaluate() and accumulate() - in fp64 on the device.  (No new ABI version:
 * these are additions.)  Capacities, enforced (SP_EINVAL from the host-known maxima, a negative dt_count from the kernel), never
 * truncated to: */
#define SP_COCO_MAX_JOINTS 64
#define SP_COCO_MAX_GT_PER_IMAGE 128   /* ground truths of one image */
#define SP_COCO_MAX_DT_PER_IMAGE 2048  /* detections of one image before the cut to max_dets */
#define SP_COCO_MAX_DETS 32            /* max_dets (COCO keypoints: 20) */
#define SP_COCO_MAX_THRS 16            /* iouThrs (COCO: 10) */
#define SP_COCO_MAX_AREAS 4            /* areaRng (COCO keypoints: all, medium, large) */
#define SP_COCO_MAX_REC_THRS 128       /* recThrs (COCO: 101) */
#define SP_COCO_DT_XY_F64 1            /* dt_flags: dt_xy is float64 (else float32, widened as the JSON round trip does) */
#define SP_COCO_DT_SCORE_F64 2         /* dt_flags: dt_score is float64 (else float32) */
#define SP_COCO_GT_CROWD 1             /* gt_flag: iscrowd (may absorb several detections) */
#define SP_COCO_GT_IGNORE 2            /* gt_flag: ignore or iscrowd or num_keypoints == 0 */
/* loadRes + evaluate() (computeOks, evaluateImg) for `images` images in one launch, one workgroup per image.  Image i owns ground
 * truths gt_seg[i]..gt_seg[i+1]-1 (annotation order) and detections dt_seg[i]..dt_seg[i+1]-1 (list order); device int32 [images+1].
 * gt_kps [n_gt, J, 3] (x, y, v), gt_area [n_gt], gt_bbox [n_gt, 4] (x, y, w, h): float64; gt_flag [n_gt]: SP_COCO_GT_*.
 * Detection p of the segment order is row dt_index[p] (device int32, or NULL: row p) of dt_xy [P, J, 2] and dt_score [P].
 * max_gt / max_dt: the largest image's counts, known to the host.  sigmas_host: `joints` doubles in HOST memory or NULL (COCO's 17);
 * iou_thrs_host [n_thrs], area_rng_host [n_areas][2]: HOST doubles.  With S = images * max_dets slots (slot i * max_dets + k = the
 * k-th detection of image i in stable descending score order), the outputs are: dt_count [images] (kept detections; -1: more than
 * SP_COCO_MAX_DT_PER_IMAGE detections, -2: more than SP_COCO_MAX_GT_PER_IMAGE ground truths - nothing of that image is evaluated),
 * dt_keep [S] (row of dt_xy, -1 = empty slot), dt_kscore [S], dt_karea [S] (float64), oks [n_gt * max_dets] (image i: a
 * [dt_count[i], G_i] row-major matrix at offset gt_seg[i] * max_dets, ground truths in annotation order), dtm int32 [n_areas, n_thrs, S]
 * (matched ground-truth row, -1 = none), dt_ignore uint8 [n_areas, n_thrs, S], gt_ignore uint8 [n_areas, n_gt]. */
int sp_coco_kp_eval_images(const int32_t* gt_seg, const double* gt_kps, const double* gt_area, const double* gt_bbox,
                           const int32_t* gt_flag, const int32_t* dt_seg, const int32_t* dt_index, const void* dt_xy, const void* dt_score,
                           int dt_flags, int images, int n_gt, int max_gt, int max_dt, int joints, const double* sigmas_host, int max_dets,
                           const double* iou_thrs_host, int n_thrs, const double* area_rng_host, int n_areas, int32_t* dt_count,
                           int32_t* dt_keep, double* dt_kscore, double* dt_karea, double* oks, int32_t* dtm, unsigned char* dt_ignore,
                           unsigned char* gt_ignore, void* stream);
/* accumulate(): a stable descending-score order of the kept detections of all images (tiled rank by counting: S^2 comparisons), then
 * per (area range, threshold) the tp / fp scan over non-ignored detections, rc = tp / npig, pr = tp / (fp + tp + 2^-52), the
 * envelope from the right and pr[searchsorted(rc, rec_thrs, 'left')].  precision float64 [n_thrs, n_rec, n_areas], recall float64
 * [n_thrs, n_areas]; -1 where the range has no non-ignored ground truth.  rec_thrs_host: HOST doubles.  Two launches, no copy, no
 * synchronisation.  workspace: sp_coco_kp_accumulate_workspace bytes of device memory. */
int sp_coco_kp_accumulate_workspace(int images, int max_dets, int n_thrs, int n_areas, int64_t* bytes);
int sp_coco_kp_accumulate(const int32_t* dt_count, const double* dt_kscore, const int32_t* dtm, const unsigned char* dt_ignore,
                          const unsigned char* gt_ignore, int images, int n_gt, int max_dets, int n_thrs, int n_areas,
                          const double* rec_thrs_host, int n_rec, void* workspace, int64_t workspace_bytes, double* precision,
                          double* recall, void* stream);

/* the same normalisation written directly in the network's input layout (the stem's loader format): NHWC4 fp32 [B,h,w,4] or,
 * out_bf16 == 1: NHWC8 bf16 [B,h,w,8]; out_bf16 == 2: NHWC4 bf16 [B,h,w,4] (what the bf16 inference stem reads); pad channels are zero.  Replaces sp_u8hwc_bgr_to_nchw_f32 + sp_nchw_to_nhwc4 when the crops
 * arrive as uint8 (1 byte per value over PCIe, one pass on the GPU). */
int sp_u8hwc_bgr_to_nhwc(const unsigned char* img, void* out, int out_bf16, int batch, int h, int w, const float* mean_rgb_host,
                         void* stream);

/* NCHW fp32 [B,C<=4,h,w] -> NHWC4 bf16 [B,h,w,4] (8 bytes per pixel; w even: the stem conv reads pixel pairs as 8 channels) */
int sp_nchw_to_nhwc4_bf16(const float* x, void* y, int batch, int channels, int h, int w, void* stream);

/* ---- encoders: commons/transforms.py ----------------------------------------------------------- */

/* RefineSimpleTransform.get_heat_map (:167-191), batched: joints [B,J,3] (x,y,vis in heat-map px) ->
 * targets [B,J,h,w], weights [B,J] */
int sp_encode_gauss_refine(const float* joints, int batch, int joints_n, int h, int w, float sigma, float* targets,
                           float* weights, void* stream);
/* BasicSimpleTransform.get_heat_map (:80-116): joints in INPUT px, quantised centre, truncated patch */
int sp_encode_gauss_basic(const float* joints, int batch, int joints_n, int h, int w, float sigma, int stride,
                          float* targets, float* weights, void* stream);

/* ---- loss: processors/ddp_pose_resnet_solver.py:94,117 ------------------------------------------
 * loss = 0.5 * mean((pred*m - target*m)^2) over all B*J*h*w elements; grad (may be NULL) = d loss / d pred.
 * `loss_out` is one device float, written by the kernel (no host sync). `workspace`: >= 4096 bytes, zeroed by the call. */
int sp_masked_mse(const float* pred, const float* target, const float* mask, int batch, int joints, int hw,
                  float* loss_out, float* grad, void* workspace, void* stream);

/* ---- training step: processors/ddp_pose_resnet_solver.py:110-133 (model.train() forward, loss.backward(),
 *      optimizer.step()) ---------------------------------------------------------------------------------------------
 * Activations NHWC; argument `bf16`: bit 0 = activations (z, relu_src, dz, pool input) are bf16, bit 1 = activation
 * gradients (dy, dres, pool dx/dy) are bf16; statistics and the gradients of the affine parameters are always fp32;
 * `rows` = B*H*W.  `workspace` of the reductions: >= SP_REDUCE_WORKSPACE_BYTES(c) bytes (per-workgroup partial sums in fp64,
 * folded in a fixed order by a second small kernel: deterministic, no float atomics); c <= 4096.
 * Widths the reductions take: c % 4 == 0 and c/4 either <= 256 or a multiple of 256 (c <= 1024, 2048, 3072, 4096 - every width of the
 * nets here).  Their workgroups walk c/4 channel quads 256 at a time with a barrier in every trip, so a width such as 1536 (one and a
 * half trips) is refused with SP_EINVAL by every entry point that runs one: sp_bn_train_stats_nhwc, sp_bn_train_partial_nhwc,
 * sp_bn_train_bwd_reduce_nhwc, sp_bn_train_bwd_nhwc, sp_bn_maxpool_bwd_nhwc and sp_channel_sum_nhwc. */
#define SP_REDUCE_WORKSPACE_BYTES(c) ((int64_t)4 << 20)

/* nn.BatchNorm2d in train mode, statistics half: per-channel batch mean and 1/sqrt(biased var + eps) of z [rows, c];
 * running_mean/var (may both be NULL) are updated with `momentum` and the UNBIASED variance, as torch does. */
int sp_bn_train_stats_nhwc(const void* z, int bf16, int64_t rows, int c, float eps, float momentum, float* mean, float* invstd,
                           float* running_mean, float* running_var, void* workspace, void* stream);
/* The same statistics without a pass over z: sp_conv2d_fwd_bn_stats is sp_conv2d_fwd (no scale/shift/residual/ReLU, NHWC store in
 * the conv's dtype) whose epilogue also writes, per (phase, M tile) of the launch (the tile's wave rows are added inside the launch), the per-channel sum and sum of squares
 * of the values it stores ([partial_rows][n_pad] fp32 each; sp_conv2d_bn_stats_rows gives partial_rows for the tile the launch
 * will use); sp_bn_train_stats_from_conv folds them in index order in fp64 and finishes like sp_bn_train_stats_nhwc. */
int sp_conv2d_bn_stats_rows(const sp_conv_desc* desc, int* partial_rows);
int sp_conv2d_fwd_bn_stats(const sp_conv_desc* desc, const void* x, const void* w_packed, void* y, float* stats_sum,
                           float* stats_sumsq, int stats_rows_capacity, void* stream);
/* sp_conv2d_fwd_bn_stats of a bf16 1x1 stride-1 convolution (c_in <= 512) whose input is relu(BatchNorm(z_in)) of the previous layer
 * (`Bottleneck.forward`: out = relu(bn2(conv2(.))); out = conv3(out), nets/pose_resnet_dconv.py:118-122): the map is applied while z_in is staged
 * (in_mean / in_invstd: that layer's batch statistics, in_gamma / in_beta its affine pair), and the launch also writes the activation `y_in`
 * [same layout as z_in] and, when not null, its ReLU bit mask (one byte per 8 channels) - what the backward pass and the weight gradient read.
 * Replaces sp_bn_apply_nhwc(relu = 1) + sp_conv2d_fwd_bn_stats with the same bits (ABI 33). */
int sp_conv2d_fwd_bn_stats_abn(const sp_conv_desc* desc, const void* z_in, const float* in_mean, const float* in_invstd, const float* in_gamma,
                               const float* in_beta, void* y_in, void* relu_mask_in, const void* w_packed, void* y, float* stats_sum,
                               float* stats_sumsq, int stats_rows_capacity, void* stream);
int sp_bn_train_stats_from_conv(const float* stats_sum, const float* stats_sumsq, int partial_rows, int stride, int64_t rows, int c,
                                float eps, float momentum, float* mean, float* invstd, float* running_mean, float* running_var,
                                void* stream);
/* Backward counterpart: a dgrad launch (sp_conv2d_fwd on the dgrad packing, fp32 NHWC store, optional in-place accumulate) whose
 * output IS dy of a BatchNorm+ReLU layer.  Given that layer's saved output bn_y (ReLU mask), input bn_z and statistics, the
 * epilogue also writes the partial sums of g = dy*(bn_y > 0) and g*xhat, one row per (phase, M tile) as above;
 * several launches that together cover dy (the phases of a stride-2 dgrad) fill consecutive row ranges of the same buffers.
 * sp_bn_bwd_sums_from_conv folds them (index order, fp64) into dbeta / dgamma; sp_bn_train_bwd_apply_nhwc finishes the layer. */
int sp_conv2d_dgrad_bn_bwd_stats(const sp_conv_desc* desc, const void* dz, const void* w_packed, const void* accumulate, void* dx,
                                 const void* bn_y, const void* bn_z, const float* bn_mean, const float* bn_invstd, float* sum_g,
                                 float* sum_g_xhat, int stats_rows_capacity, void* stream);
int sp_bn_bwd_sums_from_conv(const float* sum_g, const float* sum_g_xhat, int partial_rows, int stride, int c, float* dgamma,
                             float* dbeta, void* stream);
/* The same launch when dy is the gradient of a block output y = relu(bn3(z) + bn_ds(z2)) with a projection shortcut (the first
 * Bottleneck of a stage, pose_resnet_dconv.py:124-131): the shortcut BatchNorm's dy is the same g, so the epilogue also leaves
 * the partial sums of g * xhat2 (its d gamma; its d beta is sum g): sp_bn_bwd_sums_from_conv(sum_g, sum_g_xhat2, ...) folds them. */
int sp_conv2d_dgrad_bn_bwd_stats2(const sp_conv_desc* desc, const void* dz, const void* w_packed, const void* accumulate, void* dx,
                                  const void* bn_y, const void* bn_z, const float* bn_mean, const float* bn_invstd, float* sum_g,
                                  float* sum_g_xhat, const void* bn2_z, const float* bn2_mean, const float* bn2_invstd,
                                  float* sum_g_xhat2, int stats_rows_capacity, void* stream);
/* sp_conv2d_dgrad_bn_bwd_stats(2) for conv1 of an identity Bottleneck with bf16 gradients: the block input's gradient also receives the
 * residual share g = dy_out * (ReLU mask of the block output, pose_resnet_dconv.py:124-131).  Instead of `accumulate` = g written by bn3's
 * backward pass, this launch takes (acc_dy = dy_out, acc_mask = the block output's ReLU bit mask) and adds dy_out where the bit is set: the
 * pass writes 2 bytes per element less, the bits are the same.  bn2_* all NULL: one BatchNorm. */
int sp_conv2d_dgrad_bn_bwd_stats_macc(const sp_conv_desc* desc, const void* dz, const void* w_packed, const void* acc_dy, const void* acc_mask,
                                      void* dx, const void* bn_y, const void* bn_z, const float* bn_mean, const float* bn_invstd, float* sum_g,
                                      float* sum_g_xhat, const void* bn2_z, const float* bn2_mean, const float* bn2_invstd, float* sum_g_xhat2,
                                      int stats_rows_capacity, void* stream);
/* The dgrad of a STRIDE-2 conv is a family of launches, one descriptor per output phase (their tap counts differ: 3x3 -> 2x2, 2x1, 1x2, 1x1).
 * This entry runs the family as ONE launch (blockIdx.y = phase, per-phase geometry / packed weights in the kernel arguments): descs[i] and
 * w_packed[i] are exactly what sp_conv2d_fwd / sp_conv2d_dgrad_bn_bwd_stats(2) would take phase by phase (same batch, tensors, flags and
 * tile; 2-4 phases), the partial rows land phase-major as that sequence leaves them, the bits of dx and of the sums are the same.
 * bn_z NULL: plain dgrad (bn_* / sum_* unused).  Replaces the input-gradient half of `loss.backward()` for nn.Conv2d(stride=2)
 * (nets/pose_resnet_dconv.py:100-101: conv2 of a stage's first Bottleneck). */
int sp_conv2d_dgrad_phases(const sp_conv_desc* descs, int n_phases, const void* dz, const void* const* w_packed, const void* accumulate,
                           void* dx, const void* bn_y, const void* bn_z, const float* bn_mean, const float* bn_invstd, float* sum_g,
                           float* sum_g_xhat, const void* bn2_z, const float* bn2_mean, const float* bn2_invstd, float* sum_g_xhat2,
                           int stats_rows_capacity, void* stream);
/* The fold as the prologue of the pass that consumes it (round 4): sp_bn_fold_apply_nhwc = sp_bn_train_stats_from_conv + sp_bn_apply_nhwc
 * in ONE launch - every workgroup folds the partial rows of its 64-channel slab itself (same order as the stand-alone fold: same bits),
 * the first row stripe publishes mean / invstd / running statistics; sp_bn_fold_bwd_apply_nhwc = sp_bn_bwd_sums_from_conv (+ the same for
 * a second BatchNorm sharing g: sum_g_xhat2 -> dgamma2, sum g -> dbeta2; all three NULL when there is none) + sp_bn_train_bwd_apply_nhwc.
 * Meant for tensors with few partial rows (the caller decides: layer3 / layer4 of a ResNet at 32 images have 24-96); replaces
 * `nn.BatchNorm2d` forward / backward of processors/ddp_pose_resnet_solver.py:115,118 together with the conv launch that left the rows. */
int sp_bn_fold_apply_nhwc(const void* z, int bf16, const float* stats_sum, const float* stats_sumsq, int partial_rows, int stride,
                          int64_t total_rows, float eps, float momentum, const float* gamma, const float* beta, const void* residual, void* y,
                          int64_t rows, int c, int relu, float* mean, float* invstd, float* running_mean, float* running_var, void* relu_mask,
                          void* stream);
/* `bf16` of the backward passes is a bit word: 1 = activations (z, relu_src, dz) are bf16; 2 = the activation gradients (dy, dres) are bf16 too
 * (PoseTrainer grad_dtype "bf16"); 4 = relu_src is the ReLU BIT MASK the forward pass left in `relu_mask` (uint8 [rows * c / 8], bit e of
 * byte i = channel 8 i + e passed the ReLU; bf16 activations, c % 8 == 0) instead of the tensor y: 1/16 of the bytes.  Flag 4 belongs to the
 * apply passes (sp_bn_fold_bwd_apply_nhwc, sp_bn_train_bwd_apply_nhwc); the reduction sp_bn_train_bwd_reduce_nhwc (and with it
 * sp_bn_train_bwd_nhwc) reads relu_src as the tensor y and refuses it. */
int sp_bn_fold_bwd_apply_nhwc(const void* dy, int bf16, const void* relu_src, const void* z, const float* sum_g, const float* sum_g_xhat,
                              const float* sum_g_xhat2, int partial_rows, int stride, const float* mean, const float* invstd,
                              const float* gamma, int64_t total_rows, int64_t rows, int c, float* dgamma, float* dbeta, float* dgamma2,
                              float* dbeta2, void* dz, void* dres, int dres_accumulate, void* stream);
/* y = [relu]((z - mean) * invstd * gamma + beta [+ residual])   (Bottleneck.forward tail, pose_resnet_dconv.py:124-131) */
int sp_bn_apply_nhwc(const void* z, int bf16, const float* mean, const float* invstd, const float* gamma, const float* beta,
                     const void* residual, void* y, int64_t rows, int c, int relu, void* relu_mask /* NULL, or see above */, void* stream);
/* backward of [relu](bn(z) [+ residual]): g = dy * (relu_src > 0) (relu_src NULL: g = dy); dgamma = sum g*xhat,
 * dbeta = sum g, dz = gamma*invstd*(g - dbeta/rows - xhat*dgamma/rows); dres (NULL or tensor) = g or += g */
int sp_bn_train_bwd_nhwc(const void* dy, int bf16, const void* relu_src, const void* z, const float* mean, const float* invstd,
                         const float* gamma, int64_t rows, int c, void* dz, float* dgamma, float* dbeta, void* dres,
                         int dres_accumulate, void* workspace, void* stream);
/* The ResNet stem in training (pose_resnet_dconv.py:251-256: bn1 -> relu -> maxpool): relu(bn1(z)) feeds the pooling only, so
 * sp_bn_apply_maxpool_nhwc applies the BatchNorm + ReLU map to the taps of each window and writes the POOLED map + the winning tap per element
 * (same values and indices as sp_bn_apply_nhwc + sp_maxpool3x3s2_idx_nhwc, without the full-resolution tensor in between), and
 * sp_bn_maxpool_bwd_nhwc is the backward of that pair from the pooled gradient: d gamma / d beta summed over the pooled grid (a pooled
 * gradient reaches exactly one stem pixel; xhat and the ReLU mask re-formed from z at the winner; fp64 partials, fixed order), then dz of
 * the stem conv by gathering each pixel's <= 4 windows.  `bf16`: bit 0 activations, bit 1 gradients (as the other backward passes);
 * workspace: SP_REDUCE_WORKSPACE_BYTES. */
int sp_bn_apply_maxpool_nhwc(const void* z, int bf16, const float* mean, const float* invstd, const float* gamma, const float* beta, void* y,
                             void* idx, int batch, int h, int w, int c, void* stream);
int sp_bn_maxpool_bwd_nhwc(const void* dy_pooled, int bf16, const void* idx, const void* z, const float* mean, const float* invstd,
                           const float* gamma, const float* beta, int batch, int h, int w, int c, float* dgamma, float* dbeta, void* dz,
                           void* workspace, void* stream);
/* nn.SyncBatchNorm (ddp...:89-90) = the same three steps with a cross-rank SUM between the halves:
 *   forward : sp_bn_train_partial_nhwc -> all-reduce(sums [c][2] fp64: sum, sum of squares) -> sp_bn_train_finalize(total_rows)
 *   backward: sp_bn_train_bwd_reduce_nhwc (LOCAL dgamma, dbeta = this rank's parameter gradients) -> all-reduce(copy of them)
 *             -> sp_bn_train_bwd_apply_nhwc(global sums, total_rows = rows over all ranks)
 * sp_bn_train_stats_nhwc / sp_bn_train_bwd_nhwc are exactly these halves back to back with total_rows = rows. */
int sp_bn_train_partial_nhwc(const void* z, int bf16, int64_t rows, int c, double* sums, void* workspace, void* stream);
/* the forward half without the pass over z: fold the partial rows sp_conv2d_fwd_bn_stats left into this rank's fp64 (sum, sum of
 * squares) per channel, [c][2] as above -> all-reduce -> sp_bn_train_finalize.  Several layers may fold into consecutive slices of
 * ONE buffer and share one all-reduce (the conv1 / downsample pair of a block's first bottleneck reads the same input). */
int sp_bn_sums_from_conv(const float* stats_sum, const float* stats_sumsq, int partial_rows, int stride, int c, double* sums, void* stream);
int sp_bn_train_finalize(const double* sums, int64_t total_rows, int c, float eps, float momentum, float* mean, float* invstd,
                         float* running_mean, float* running_var, void* stream);
/* SyncBatchNorm with one launch less on each side of the exchange: sp_bn_apply_sums_nhwc = sp_bn_train_finalize + sp_bn_apply_nhwc (every thread
 * finalises its own 4 channels from the all-reduced sums, the first row's threads publish mean / invstd / running statistics; same values);
 * sp_bn_bwd_sums_from_conv2 = sp_bn_bwd_sums_from_conv that ALSO writes the two sums where the message is assembled (the parameter gradients keep
 * this rank's sums, the message carries them to the other ranks: no concatenation launch). */
int sp_bn_apply_sums_nhwc(const void* z, int bf16, const double* sums, int64_t total_rows, float eps, float momentum, const float* gamma,
                          const float* beta, const void* residual, void* y, int64_t rows, int c, int relu, float* mean, float* invstd,
                          float* running_mean, float* running_var, void* stream);
/* sp_bn_bwd_sums_from_conv for a BatchNorm AND the projection shortcut's BatchNorm that shares its g (sum_g_xhat2: the third array of
 * sp_conv2d_dgrad_bn_bwd_stats2; d beta2 = the same sum g) in one launch; the bits of two separate calls. */
int sp_bn_bwd_sums_from_conv_pair(const float* sum_g, const float* sum_g_xhat, const float* sum_g_xhat2, int partial_rows, int stride, int c,
                                  float* dgamma, float* dbeta, float* dgamma2, float* dbeta2, void* stream);
int sp_bn_bwd_sums_from_conv2(const float* sum_g, const float* sum_g_xhat, int partial_rows, int stride, int c, float* dgamma, float* dbeta,
                              float* dgamma_copy, float* dbeta_copy, void* stream);
int sp_bn_train_bwd_reduce_nhwc(const void* dy, int bf16, const void* relu_src, const void* z, const float* mean, const float* invstd,
                                int64_t rows, int c, float* dgamma, float* dbeta, void* workspace, void* stream);
int sp_bn_train_bwd_apply_nhwc(const void* dy, int bf16, const void* relu_src, const void* z, const float* mean, const float* invstd,
                               const float* gamma, const float* sum_dgamma, const float* sum_dbeta, int64_t total_rows, int64_t rows,
                               int c, void* dz, void* dres, int dres_accumulate, void* stream);
/* backward of nn.PixelShuffle(2) (DUC head, nets/commons.py:36-41): dy [B,2h,2w,c/4] fp32 -> dx [B,h,w,c] fp32 */
int sp_pixel_unshuffle2_nhwc(const float* dy, float* dx, int batch, int h, int w, int c, void* stream);
/* the same permutation on a bf16 gradient (activation gradients kept in bf16: PoseTrainer grad_dtype "bf16" on the DUC head); c % 32 == 0 */
int sp_pixel_unshuffle2_nhwc_bf16(const void* dy, void* dx, int batch, int h, int w, int c, void* stream);
/* x [B,channels,h,w] fp32 -> y [B,h,w,c_pad] (fp32, or bf16 when y_bf16), channels >= `channels` zero-filled: puts
 * d loss / d heat-map (sp_masked_mse's grad) into the layout and K-tile padding the final layer's backward launches read */
int sp_nchw_to_nhwc_pad(const float* x, void* y, int y_bf16, int batch, int channels, int h, int w, int c_pad, void* stream);
/* sum over batch and pixels of an NCHW tensor [batch, channels, hw] -> [channels]: the final layer's bias gradient straight from
 * d loss / d heat maps (sp_masked_mse's grad), written where the caller's flat gradient buffer keeps it */
int sp_channel_sum_nchw(const float* x, int batch, int channels, int hw, float* sum, void* stream);
/* sum over rows of a [rows, c] tensor (conv bias gradient) */
int sp_channel_sum_nhwc(const float* a, int64_t rows, int c, float* sum, void* workspace, void* stream);
/* backward of nn.MaxPool2d(3,2,1) (first maximum of a window wins, as torch); x = the pool's input */
int sp_maxpool3x3s2_bwd_nhwc(const void* x, int bf16, const void* dy, void* dx, int batch, int h, int w, int c, void* stream);
/* the training pair: forward that also records the winning tap (ky*3+kx, one byte per output element, `idx` = [B,ho,wo,c] bytes),
 * and the backward that gathers through it (<= 4 (index, dy) pairs per input pixel); same results as the function above */
int sp_maxpool3x3s2_idx_nhwc(const void* x, int bf16, void* y, void* idx, int batch, int h, int w, int c, void* stream);
int sp_maxpool3x3s2_bwd_idx_nhwc(const void* idx, const void* dy, int bf16, void* dx, int batch, int h, int w, int c, void* stream);
/* torch.optim.Adam (amsgrad False, weight_decay 0) over flat buffers of n (multiple of 4) floats, `step` = 1,2,...;
 * grad is multiplied by grad_scale first (1/world_size after a SUM all-reduce) - ddp...:70-72,119.  lr / betas / eps are doubles:
 * 1 - beta, the bias corrections and lr / (1 - beta1^step) are formed in double and rounded to fp32 once, as torch does */
int sp_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1,
                 double beta2, double eps, int step, float grad_scale, void* stream);

/* The same update with the step's eight scalars (step size, betas, 1 - betas, eps, sqrt of the second bias correction, gradient scale) in
 * device memory: sp_adam_set_scalars forms them on the host exactly as sp_adam_step does and writes them with one tiny launch;
 * sp_adam_step_dev launches then have arguments that never change from step to step, so a captured train step (hipGraph: PoseTrainer.capture)
 * replays - bit-identical to sp_adam_step with the same hyper-parameters. */
int sp_adam_set_scalars(double lr, double beta1, double beta2, double eps, int step, float grad_scale, float* scalars8, void* stream);
int sp_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* scalars8, void* stream);
/* weight gradient of one conv / transposed-conv launch family: dW[n][(ty,tx,c)] = sum_m g[m][n] * im2col(a)[m][(ty,tx,c)],
 * `desc` describing how `a` is gathered (as in sp_conv2d_fwd; tile/out_* ignored; flags & SP_CONV_BF16: g and a are
 * bf16, dW stays fp32), g = [rows, g_channels] NHWC.
 * The result is written in the reference's weight layout: dw[n*dst_stride_n + c*dst_stride_c + ty*kw_valid + tx]
 * for n < n_valid, c < c_valid, tx < kw_valid (every such element is overwritten).
 *
 * sp_conv2d_wgrad_batched runs the weight gradients of up to 64 layers in a handful of launches (nets/pose_resnet_dconv.py:99-103,
 * 158,236-244 under loss.backward(), ddp...:117-119): the pixel range of every layer is cut into units of about equal cost (the
 * cut depends on the layer alone, so a layer's bits do not depend on its companions and equal sp_conv2d_wgrad's), all units of
 * the layers that share a dW tile shape run as ONE launch, every unit leaves its partial tile in `workspace`, and one fold
 * launch sums each layer's partials in index order into `dw`: deterministic, no float atomics.
 * workspace: sp_conv2d_wgrad_workspace(jobs, n_jobs, &bytes) bytes (the error message of a short one states the need). */
typedef struct sp_wgrad_job {
    sp_conv_desc desc;
    const void* g;   /* [rows, g_channels] */
    const void* a;   /* NHWC tensor gathered through desc */
    float* dw;
    int64_t dst_stride_n, dst_stride_c;
    int32_t g_channels, n_valid, c_valid, kw_valid;
} sp_wgrad_job;
int sp_conv2d_wgrad_workspace(const sp_wgrad_job* jobs, int n_jobs, int64_t* bytes);
int sp_conv2d_wgrad_batched(const sp_wgrad_job* jobs, int n_jobs, void* workspace, int64_t workspace_bytes, void* stream);
/* one layer: sp_conv2d_wgrad_batched with a single job */
int sp_conv2d_wgrad(const sp_conv_desc* desc, const void* g, int g_channels, const void* a, int n_valid, int c_valid,
                    int kw_valid, int64_t dst_stride_n, int64_t dst_stride_c, float* dw, void* workspace,
                    int64_t workspace_bytes, void* stream);
/* generic 4-D gather-copy used to (re)pack weights after every optimizer step:
 * dst[dst_offset + ((i0*d1 + i1)*d2 + i2)*d3 + i3] = all(i_k < valid[k]) ? src[src_base + sum i_k*src_strides[k]] : 0 */
int sp_permute4_f32(const float* src, void* dst, int dst_bf16, const int32_t* dst_dims, const int64_t* src_strides,
                    const int32_t* valid, int64_t src_base, int64_t dst_offset, void* stream);

/* every pack job of a network in one launch: `jobs_device` = device array of n_jobs records
 *   { int32 dst_dims[4]; int64 src_strides[4]; int32 valid[4]; int64 src_base; int64 dst_address; int64 total; int32 dst_bf16; int32 walk;
 *     int32 tap0; int32 tile0; }
 * (dst_address = device pointer of the destination incl. its offset), blocks_per_job workgroups grid-stride over a job.
 * walk: how the job's elements are visited (same result, other access pattern): 0 destination order (sources contiguous along the
 * last destination index), 1 multi-tap filters - a thread takes one (i0, i3) pair and loops over the (i1, i2) taps, whose sources
 * are one contiguous run, 2 a 2-D transpose (dims 1 and 2 of extent 1, source contiguous along i0) in 32x32 tiles through LDS,
 * 3 multi-tap filters whose fastest destination index is the source's slowest (stride[0] = floats per (i0, i3) block < |stride[3]|): tiles of
 * 32 i3 x tile0 i0 values through LDS, coalesced both ways; the record then ends in two more int32: tap0 (offset <= 0 from `base` to the
 * block's first tap) and tile0 (32 * (tile0 * stride[0] | 1) <= 10240).  Record size: 104 bytes (ABI 33; 96 before).
 * Walk 3 needs a 40 KB LDS tile: it exists only in sp_permute4_batched_tiled (ABI 34: same arguments, same results; a launch of its own so
 * that the default repack keeps 8 workgroups per CU); sp_permute4_batched visits a walk-3 job as walk 1. */
int sp_permute4_batched(const float* src, const void* jobs_device, int n_jobs, int blocks_per_job, void* stream);
int sp_permute4_batched_tiled(const float* src, const void* jobs_device, int n_jobs, int blocks_per_job, void* stream);

/* measurement aid: occupies `stream` for `us` microseconds (one idle wave on the 100 MHz constant clock) - bench.py's stand-in for the
 * latency of a SyncBatchNorm message (ddp...:89-90) on a box with a single GPU */
/* Backward of sp_upsample_add_nhwc (HRNet fuse layers, nets/pose_hrnet.py:192-202,250-257): dr = y_relu_src ? dy (y > 0) : dy (y in the
 * activation dtype, null when the forward had no ReLU); dbase (+)= dr at the high resolution [batch, h*factor, w*factor, c]; dx (+)= the sum
 * of dr over each factor x factor block [batch, h, w, c].  Gradients are fp32; the accumulate flags say whether the target already holds other
 * consumers' shares. */
int sp_upsample_add_bwd_nhwc(const float* dy, int bf16, const void* y_relu_src, int batch, int h, int w, int c, int factor, float* dbase,
                             int dbase_accumulate, float* dx, int dx_accumulate, void* stream);

/* SELayer backward (nets/commons.py:4-18 inside Bottleneck.forward, pose_resnet_dconv.py:124-131; `bf16`: dtype of the saved activations,
 * gradients w.r.t. activations are fp32):  y = relu(u * sigmoid(g[b,c]) + identity), u = bn3(conv3(.)), g = fc2(relu(fc0(mean_hw u))).
 *   sp_se_gate_bwd_reduce: da[b,c] = sum_hw (y > 0 ? dy : 0) * u
 *   sp_se_sigmoid_bwd:     dg = da * a (1 - a), a = sigmoid(g) (written in the activation dtype: the FC layers' MFMA operand); dbias[c] = sum_b dg
 *   sp_relu_bwd_rows:      out = dh (h > 0) on a [batch, c] map, dbias[c] = sum_b out (dbias may be null)
 *   sp_se_gate_bwd_apply:  du = (y > 0 ? dy : 0) * a + ds[b,c] / hw;  dres (+)= (y > 0 ? dy : 0)
 * The FC layers themselves run as 1x1 convolutions (sp_conv2d_fwd / dgrad re-packing / sp_conv2d_wgrad_batched). */
int sp_se_gate_bwd_reduce(const float* dy, int bf16, const void* y, const void* u, int batch, int hw, int c, float* da, void* stream);
int sp_se_sigmoid_bwd(const float* da, int bf16, const void* gate_logits, int batch, int c, void* dg, float* dbias, void* stream);
int sp_relu_bwd_rows(const float* dh, int bf16, const void* h, int batch, int c, void* out, float* dbias, void* stream);
int sp_se_gate_bwd_apply(const float* dy, int bf16, const void* y, const void* gate_logits, const float* ds, int batch, int hw, int c,
                         float* du, float* dres, int dres_accumulate, void* stream);

int sp_stream_delay_us(double us, void* stream);

/* RCCL called directly, for the collectives that sit on the train step's critical path (replaces the `SyncBatchNorm` exchanges and the
 * DistributedDataParallel gradient all-reduces of ddp...:89-93 issued through torch.distributed): sp_comm_allreduce_sum_f32 enqueues ONE
 * in-place fp32 SUM all-reduce on the caller's stream - stream order is the dependency, one host call per message.  librccl is resolved
 * at run time (sp_comm_available() == 0 where it is absent; everything single-GPU still works).  sp_comm_unique_id: rank 0 makes the 128-byte
 * id, the caller ships it to the other ranks (any channel), every rank calls sp_comm_create on its own device. */
int sp_comm_available(void);
int sp_comm_unique_id(void* id128);
int sp_comm_create(const void* id128, int world, int rank, void** comm);
int sp_comm_allreduce_sum_f32(void* comm, float* buf, int64_t n, void* stream);
/* the same for fp64 buffers (the SyncBatchNorm forward message: per-channel (sum, sum of squares) in double); n = number of doubles */
int sp_comm_allreduce_sum_f64(void* comm, double* buf, int64_t n, void* stream);
/* what RCCL reports for a communicator: ncclCommCount / ncclCommUserRank / ncclCommCuDevice */
int sp_comm_info(void* comm, int* world, int* rank, int* device);
int sp_comm_destroy(void* comm);

/* ---- parameter packing: the reference's tensors -> what the launches above read ------------------------------------------
 * (all pointers are device memory; every call fills its whole destination, padding included)
 *
 * sp_conv_packed_dims: rows / depth of a packed weight matrix: n_pad = c_out rounded up to the widest tile that fits (128, 64 or
 * 32), k_pad = k rounded up to one K tile (32 fp32 / 64 bf16 elements = 128 bytes). */
int sp_conv_packed_dims(int c_out, int k, int bf16, int* n_pad, int* k_pad);
/* nn.Conv2d weight [c_out, c_in, kh, kw] fp32 (nets/pose_resnet_dconv.py:19-27) -> w_packed [n_pad][k_pad] (fp32, or bf16 when
 * dst_bf16), K ordered (ty, tx, c) with c_in_packed >= c_in channels per tap and taps_w_packed >= kw taps per row (the stem's
 * 3-channel 7x7 filter on the NHWC4 image: c_in_packed 4, taps_w_packed 8).  pixel_shuffle: rows in sub-pixel-major order
 * n' = sub*(c_out/4) + c <- channel 4*c + sub, what SP_CONV_PIXEL_SHUFFLE expects (nets/commons.py:36-41).  pair_s0 >= 0: the bf16
 * stem's x-paired form (sp_conv_desc.stride_x): packed channel = sub*4 + c of pixel pair tx, i.e. kx = 2*tx + sub - pair_s0,
 * c_in_packed = 8; pair_s0 = -1: plain. */
int sp_pack_conv_weights(const float* w, int c_out, int c_in, int kh, int kw, int c_in_packed, int taps_w_packed, int pixel_shuffle,
                         int pair_s0, int n_pad, int k_pad, void* dst, int dst_bf16, void* stream);
/* nn.ConvTranspose2d(k=4, s=2, p=1) weight [c_in, c_out, 4, 4] (nets/pose_resnet_dconv.py:236-244) -> [4 phases][n_pad][4*c_in]:
 * phase (py,px) holds the 2x2 taps W[:, :, 2ty+1-py, 2tx+1-px] that reach output pixels (2y+py, 2x+px) - no multiply is spent
 * on the zeros a transposed conv inserts */
/* nn.Conv2d(groups = g) weight [c_out][c_in / g][kh][kw] with c_out == c_in -> block-diagonal panels [c_out][kh * kw * panel] (K = (tap, channel
 * within the panel); row n belongs to panel n / panel and holds its group's weights at the group's channels inside the panel, zeros elsewhere).
 * `panel` = sp_conv_desc.c_in_group = tile_n of the launch: a multiple of c_in / g and of the K tile (32 fp32 / 64 bf16 elements). */
int sp_pack_conv_weights_grouped(const float* w, int c_out, int groups, int kh, int kw, int panel, void* dst, int dst_bf16, void* stream);
/* (ABI 34) the same block-diagonal panels for the TRAIN step of that grouped conv (loss.backward() through nets/pose_resnet_dconv.py:101): a tap subset
 * (ky, kx) = (ky0 + ky_step * ty, kx0 + kx_step * tx), ty < taps_h, tx < taps_w, of the kh x kw filter (taps outside it are zero) - the forward
 * (0, 1, 0, 1), the flipped taps of the stride-1 input gradient (kh-1, -1, kw-1, -1), one output phase of the stride-2 input gradient (ky0, 2, kx0, 2) -
 * and, with `transpose`, rows = the layer's INPUT channels: the input gradient is a grouped conv of dz with Wd[c][o_local][tap] = W[o][c_local][tap].
 * dst: [c][taps_h * taps_w * panel]. */
int sp_pack_conv_weights_grouped_taps(const float* w, int c, int groups, int kh, int kw, int transpose, int taps_h, int taps_w, int ky0, int ky_step,
                                      int kx0, int kx_step, int panel, void* dst, int dst_bf16, void* stream);
/* (ABI 34) weight gradient of that grouped conv (c_out == c_in = c, `groups` groups): dw[o][cl][ky][kx] (fp32, the nn.Conv2d weight layout, WRITTEN) =
 * sum over (b, oy, ox) of dz[b, oy, ox, o] * x[b, oy*stride - pad + ky, ox*stride - pad + kx, group(o) * (c / groups) + cl]; x and dz NHWC, fp32 or
 * (bf16 = 1) bf16.  A streaming reduction (1 / groups of the dense layer's FLOPs): partial sums per row chunk in `workspace`, folded in a fixed
 * order in fp64 (no atomics).  c / groups must divide 256, kh * kw <= 9. */
int sp_conv2d_wgrad_grouped_workspace(int batch, int out_h, int c, int groups, int kh, int kw, int64_t* bytes);
int sp_conv2d_wgrad_grouped(const void* x, const void* dz, int bf16, int batch, int in_h, int in_w, int out_h, int out_w, int c, int groups, int kh,
                            int kw, int stride, int pad, float* dw, void* workspace, int64_t workspace_bytes, void* stream);
int sp_pack_deconv_k4s2p1(const float* w, int c_in, int c_out, int n_pad, void* dst, int dst_bf16, void* stream);
/* eval-mode nn.BatchNorm2d as the conv epilogue's (scale, shift): scale = weight / sqrt(running_var + eps),
 * shift = bias - running_mean * scale (each operation rounded on its own, as the torch expressions); weight / bias NULL = 1 / 0;
 * pixel_shuffle: outputs in the packed row order of sp_pack_conv_weights */
int sp_fold_bn(const float* weight, const float* bias, const float* running_mean, const float* running_var, int c, float eps,
               int pixel_shuffle, float* scale, float* shift, void* stream);

/* ---- person detector: detector/yolov5_detector.py + detector/nets/yolov5.py (csrc/detect.hip; fp32 throughout) ------------------------
 * ScalePadding.make_border (yolov5_detector.py:145) + the input glue of single_predict (:223-226) + Focus (commons.py:51) in one launch.
 * src: uint8 BGR [B, src_h, src_w, 3]; the image is resized to new_h x new_w (OpenCV INTER_LINEAR on 8-bit data restated: 11-bit
 * fixed-point coefficients, an exact 2x downscale in both axes takes INTER_AREA's 2x2 mean; new == src copies), placed at (top, left) of an
 * out_h x out_w canvas of 114.  mode SP_LETTERBOX_FOCUS: out = fp32 NHWC [B, out_h/2, out_w/2, 12], channel 3*g + c = RGB channel c / 255 of
 * canvas pixel (2*fy + dy_g, 2*fx + dx_g), (dy, dx)_g = (0,0), (1,0), (0,1), (1,1) (torch.cat order of Focus.forward); out_h, out_w even.
 * mode SP_LETTERBOX_U8: out = the uint8 BGR canvas [B, out_h, out_w, 3] (what make_border returns). */
#define SP_LETTERBOX_FOCUS 0
#define SP_LETTERBOX_U8 1
int sp_yolo_letterbox(const unsigned char* src, int batch, int src_h, int src_w, int new_h, int new_w, int top, int left, int out_h, int out_w,
                      int mode, void* out, void* stream);
/* Focus on an fp32 NCHW RGB image [B, 3, h, w] (YOLOv5.forward on a prepared tensor) -> fp32 NHWC [B, h/2, w/2, 12] as above */
int sp_yolo_focus_nchw(const float* x, int batch, int h, int w, float* out, void* stream);
/* SPP (commons.py:124): buf is fp32 NHWC [B, h, w, c_total]; slice [0, c) holds x; slices [c, 2c), [2c, 3c), [3c, 4c) receive
 * max_pool2d(x, k, stride 1, padding k // 2) for k = 5, 9, 13 (padding never wins: -inf).  c % 4 == 0, c_total % 4 == 0, c_total >= 4c */
int sp_yolo_spp_nhwc(float* buf, int batch, int h, int w, int c, int c_total, void* stream);
/* nn.UpsamplingNearest2d(scale_factor=2) from a channel slice into a channel slice: dst[b, y, x, j] = src[b, y/2, x/2, j], j < c; src / dst
 * point at channel c0 of NHWC tensors with src_c_total / dst_c_total channels; dst is [B, 2h, 2w, .].  c, both totals and both offsets % 4 == 0 */
int sp_upsample2_slice_nhwc(const float* src, int src_c_total, float* dst, int dst_c_total, int batch, int h, int w, int c, void* stream);
/* YOLOv5Head.forward, eval branch (yolov5.py:134-149): level l's head conv output heads[l] is NHWC [B, ny_l, nx_l, anchors * a_stride] with
 * anchor a's `no` values at [a * a_stride, a * a_stride + no) (a_stride >= no, % 4 == 0: the packed head pads every anchor's columns).
 * out[b, row, k] (fp32 [B, N, no], N = sum anchors * ny_l * nx_l, rows ordered (level, anchor, y, x)) = sigmoid(v), then
 * k < 2: (s * 2 - 0.5 + grid) * stride_l, k in {2, 3}: (s * 2)^2 * anchor_grid[l][a]; grid = (x, y).  3 levels; anchors <= 4;
 * grid_hw / strides / anchor_wh are HOST arrays: [3][2] (ny, nx), [3], [3][anchors][2] */
int sp_yolo_head_decode(const float* head0, const float* head1, const float* head2, int batch, const int* grid_hw, int anchors, int no, int a_stride,
                        const float* strides, const float* anchor_wh, float* out, void* stream);
/* non_max_suppression (yolov5_detector.py:52-128) of a batch: per image the candidates obj > conf_thresh, cls *= obj, multi-label expansion
 * (multi_label: every (row, class) with cls*obj > conf_thresh in row-major order; else the best class (first on ties) if > conf_thresh),
 * xywh -> xyxy, boxes offset by cls * 4096 unless agnostic, a descending score sort whose ties go to the lower candidate index, the greedy
 * scan of torchvision.ops.nms (suppress IoU > iou_thresh) truncated at max_det, then - merge and 1 < n < 3000 - merge-NMS (kept box =
 * score-weighted mean of the candidates with IoU > iou_thresh) and the redundancy filter (keep only kept boxes with another such candidate).
 * Exact (no truncation) up to SP_YOLO_NMS_MAX_CANDIDATES candidates per image after the expansion; above that it returns SP_EINVAL.
 * pred: fp32 [B, N, no]; out: fp32 [B, max_det, 6] (x1, y1, x2, y2, score, cls), rows [0, counts[b]) valid; counts: HOST int[B]; n_candidates: HOST int[B] or NULL, the
 * candidates after the expansion (0: the reference's None).
 * max_det <= SP_YOLO_NMS_MAX_DET.  Deterministic.  SYNCHRONOUS: it waits for the stream twice (candidate counts, then result counts). */
#define SP_YOLO_NMS_MAX_CANDIDATES 32768
#define SP_YOLO_NMS_MAX_DET 1024
int sp_yolo_nms_workspace(int batch, int64_t* bytes);
int sp_yolo_nms(const float* pred, int batch, int n_rows, int no, float conf_thresh, float iou_thresh, int merge, int multi_label, int agnostic,
                int max_det, void* workspace, int64_t workspace_bytes, float* out, int* counts, int* n_candidates, void* stream);
/* clip_coords + the un-letterbox of single_predict (yolov5_detector.py:233-237) on `rows` rows of 6 floats (in place):
 * x1, x2 clamped to [0, img_w], y1, y2 to [0, img_h], then x = (x - left) / ratio, y = (y - top) / ratio */
int sp_yolo_boxes_to_source(float* det, int rows, float img_h, float img_w, float left, float top, float ratio, void* stream);
/* sp_yolo_nms without the two host reads: the same workspace and the same three kernels; counts is DEVICE int32 [B], and DEVICE int32
 * status[B] receives bit 0 = "more than SP_YOLO_NMS_MAX_CANDIDATES candidates" (what sp_yolo_nms reports as SP_EINVAL; such an image gets
 * count 0, its neighbours are not affected).  The rank kernel runs on the fixed grid the cap implies; workgroups beyond an image's candidate
 * count return at once.  out[b, :counts[b]] and counts equal sp_yolo_nms's bit for bit; rows from counts[b] on are not written.  Plain launches
 * only: no copy, no synchronisation, safe inside a stream capture. */
int sp_yolo_nms_device(const float* pred, int batch, int n_rows, int no, float conf_thresh, float iou_thresh, int merge, int multi_label,
                       int agnostic, int max_det, void* workspace, int64_t workspace_bytes, float* out, int32_t* counts, int32_t* status,
                       void* stream);

/* ---- top-down pipeline: detections -> crop geometry -> crops, without a host round trip ----------------------------------------------
 * sp_topdown_plan: BasicTransform.__call__ (datasets/naive_data.py:33-56) for the selected rows of a batch of detections, on the device.
 * det fp32 [B, max_det, 6] (x1, y1, x2, y2, score, cls) in SOURCE pixels, counts int32 [B] (rows valid per image).  A row is selected when
 * cls == keep_cls (keep_cls < 0: every row) and score >= min_score.  Selected rows fill `capacity` (1 .. 2048) slots in (image, row)
 * order; rows that do not fit are dropped from the END of that order and counted in dropped[b].  Every output is DEVICE memory:
 *   seg int32 [B+1]           persons of image b are slots seg[b] .. seg[b+1]-1
 *   src_index int32 [capacity] image of the slot (-1: dead slot)
 *   m_inv double [capacity,6] dst -> src map of the in_w x in_h crop: get_affine_transform(center, scale, 0, (in_w, in_h))[0] inverted as
 *                             cv::warpAffine / sp_warp_affine_u8c3 invert it
 *   trans_inv fp32 [capacity,2,3]  heat-map (hm_w x hm_h) -> image, what the decoders take
 *   center, scale fp32 [capacity,2]; area double [capacity] (the float32 product scale_w * scale_h, widened); box_score double [capacity]
 *   (the float32 confidence, widened); box fp32 [capacity,5] (x1, y1, x2, y2, score of the row); dropped int32 [B].
 * Dead slots (>= seg[B]) are written as zeros (src_index -1).  float32 box arithmetic and float64 Cramer solves in the host functions'
 * operation order (commons/joint_utils.py), contraction off: every value has the host's bits. */
int sp_topdown_plan(const float* det, const int32_t* counts, int batch, int max_det, int keep_cls, float min_score, int capacity, int in_w,
                    int in_h, int hm_w, int hm_h, int32_t* seg, int32_t* src_index, double* m_inv, float* trans_inv, float* center,
                    float* scale, double* area, double* box_score, float* box, int32_t* dropped, void* stream);
/* The crops of a plan: src uint8 BGR [batch, src_h, src_w, 3]; m_inv, src_index, seg as sp_topdown_plan wrote them (DEVICE memory);
 * dst uint8 BGR [capacity, out_h, out_w, 3].  Live slots hold sp_warp_affine_u8c3's pixels bit for bit (one pixel function for every warp
 * kernel); dead slots are written as zeros, so that a forward over all `capacity` crops never reads undefined memory. */
int sp_warp_affine_plan_u8c3(const unsigned char* src, int batch, int src_h, int src_w, const double* m_inv, const int32_t* src_index,
                             const int32_t* seg, int capacity, unsigned char* dst, int out_h, int out_w, void* stream);

/* ---- batches of differently sized images: per-image geometry from a table in device memory ------------------------------------------------
 * (No new ABI version: these are additions.)  sp_image_ref describes one source image: contiguous uint8 BGR [h, w, 3] in device memory
 * (1 <= h, w <= 32767), its letterbox (ScalePadding.geometry: resized to new_h x new_w, placed at (top, left) of the canvas, ratio = the
 * resize factor as a float) and dst_index, its position in the caller's order.  The kernels read an array of `batch` of them from DEVICE
 * memory; the caller fills it on the host and uploads it.  Each entry point below is its counterpart above with the launch-wide scalars
 * replaced by the table's: the same device functions produce every pixel and every box, so image b's results have the bits of the
 * counterpart run on image b alone.  The table's contents cannot be checked on the host: the caller guarantees valid pointers and sizes,
 * top, left >= 0, and dst_index inside det_all / counts_all / status_all. */
typedef struct sp_image_ref {
    const unsigned char* data;              /* device pointer */
    int32_t h, w;
    int32_t new_h, new_w, top, left;
    float ratio;
    int32_t dst_index;
} sp_image_ref;                             /* 40 bytes */
/* sp_yolo_letterbox with every image's own source size, resize target and placement on the common out_h x out_w canvas of 114 (a canvas
 * pixel outside an image's new_h x new_w rectangle is padding, wherever the rectangle lies); both modes; out_h, out_w even. */
int sp_yolo_letterbox_images(const sp_image_ref* images_dev, int batch, int out_h, int out_w, int mode, void* out, void* stream);
/* sp_yolo_boxes_to_source, out of place, for one detector group of a larger batch: det_group fp32 [batch, max_det, 6], counts_group /
 * status_group int32 [batch] as sp_yolo_nms_device wrote them for images letterboxed to img_h x img_w.  Rows [0, counts_group[b]) of
 * block b are clipped and un-letterboxed with images[b]'s left, top, ratio and written to block images[b].dst_index of det_all
 * (fp32 [total, max_det, 6]); the block's other rows are written as zeros; counts_all / status_all [dst_index] receive the count and the
 * status word.  det_all must not overlap det_group.  One launch. */
int sp_yolo_boxes_to_source_images(const float* det_group, const int32_t* counts_group, const int32_t* status_group,
                                   const sp_image_ref* images_dev, int batch, int max_det, float img_h, float img_w, float* det_all,
                                   int32_t* counts_all, int32_t* status_all, void* stream);
/* sp_warp_affine_plan_u8c3 with the source pointer and size of slot s taken from images[src_index[s]] (src_index as sp_topdown_plan wrote
 * it: the image's position in the plan's det, which is the table's order here; dst_index is not read).  Dead slots are written as zeros. */
int sp_warp_affine_plan_images_u8c3(const sp_image_ref* images_dev, int batch, const double* m_inv, const int32_t* src_index,
                                    const int32_t* seg, int capacity, unsigned char* dst, int out_h, int out_w, void* stream);

/* ---- tiled detection: the detector on overlapping tiles of large frames, fused on the device ------------------------------------------------
 * (No new ABI version: these are additions.)  A "pass" is one rectangle of a frame that goes through the detector: the whole frame or one
 * of its tiles (simple_pose_amd/tiling.py plans them).  sp_tile_ref describes one pass: `data` points at the rectangle's first pixel INSIDE
 * its frame (uint8 BGR, `pitch` pixels per frame row, pitch >= w), h x w its size, then its letterbox as in sp_image_ref, (x0, y0) its
 * origin in the frame, `image` the frame's index in the call and `slot` the pass's index within its frame (0 .. passes - 1).  The kernels
 * read the table from DEVICE memory; the caller fills it on the host, uploads it and guarantees what it holds. */
typedef struct sp_tile_ref {
    const unsigned char* data;              /* device pointer: the frame's pixel (y0, x0) */
    int32_t h, w, pitch;
    int32_t new_h, new_w, top, left;
    float ratio;
    int32_t x0, y0;
    int32_t image, slot;
} sp_tile_ref;                              /* 56 bytes */
#define SP_TILE_MAX_TILES 64                /* tiles per frame */
#define SP_TILE_MAX_PASSES 65               /* the tiles and the whole frame: 65 x 300 rows stay below SP_YOLO_NMS_MAX_CANDIDATES */
#define SP_TILE_IOU 0                       /* merge metric: intersection over union (sp_yolo_nms's) */
#define SP_TILE_IOS 1                       /* intersection over the smaller of the two areas */
/* sp_yolo_letterbox_images with the row pitch of every source taken from the table: the same pixel function, so pass b's canvas has the
 * bits of sp_yolo_letterbox run on a contiguous copy of its rectangle.  Both modes; out_h, out_w even. */
int sp_yolo_letterbox_tiles(const sp_tile_ref* tiles_dev, int batch, int out_h, int out_w, int mode, void* out, void* stream);
/* One net-shape group of `batch` passes after sp_yolo_nms_device (det_group fp32 [batch, max_det, 6], counts_group / status_group int32
 * [batch], passes letterboxed to img_h x img_w): rows [0, counts_group[p]) of pass p are clipped and un-letterboxed as
 * sp_yolo_boxes_to_source does it, then x += x0, y += y0 (one fp32 add per coordinate, no contraction), and written to block
 * (tiles[p].image, tiles[p].slot) of cand fp32 [frames, passes, max_det, 6]; the block's other rows are written as zeros; cand_counts
 * int32 [frames, passes] receives the count; the pass's status word is OR-ed into status_frames[image] (the caller zeroes status_frames
 * before the first group of a call).  cand must not overlap det_group.  One launch. */
int sp_yolo_boxes_to_frame_tiles(const float* det_group, const int32_t* counts_group, const int32_t* status_group,
                                 const sp_tile_ref* tiles_dev, int batch, int passes, int max_det, float img_h, float img_w, float* cand,
                                 int32_t* cand_counts, int32_t* status_frames, void* stream);
/* The fusion of a frame's passes, per frame: the candidates are the frame's blocks of cand in slot order, rows [0, cand_counts) of each
 * in their order; a descending score sort whose ties go to the lower candidate index; a greedy scan in which a candidate is kept unless
 * an already kept candidate of the same class (agnostic: of any class) has metric > thresh - SP_TILE_IOU: sp_yolo_nms's IoU, SP_TILE_IOS:
 * the same intersection divided by fminf(area_a, area_b); a NaN metric (an empty box) does not suppress.  The kept rows, truncated at
 * max_det, go to det fp32 [frames, max_det, 6] (rows from the count on are zeros) and counts int32 [frames]: what sp_topdown_plan reads.
 * passes <= SP_TILE_MAX_PASSES, passes * max_det <= SP_YOLO_NMS_MAX_CANDIDATES, 0 < thresh <= 1; workspace: sp_yolo_nms_workspace(frames).
 * Deterministic.  Three plain launches: no copy, no synchronisation, safe inside a stream capture. */
int sp_yolo_merge_passes(const float* cand, const int32_t* cand_counts, int frames, int passes, int max_det, int metric, float thresh,
                         int agnostic, void* workspace, int64_t workspace_bytes, float* det, int32_t* counts, void* stream);

/* ---- flip test: the mirrored network input and the merge of the two sets of heat maps ----------------------------------------------------
 * sp_mirror_w: dst[r, x] = src[r, w-1-x] over `rows` rows of `w` elements of elem_bytes bytes: 3 = uint8 BGR NHWC crops (rows = N*H),
 * 4 = fp32 NCHW inputs (rows = N*C*H).  Out of place only: dst may be the second half of the allocation that holds src, overlapping ranges
 * are refused.  rows == 0 is a no-op.  One launch; 16-byte (fp32) / 12-byte (uint8x3) accesses when w % 4 == 0 and both pointers are
 * aligned for them, one element per lane otherwise. */
int sp_mirror_w(const void* src, void* dst, int64_t rows, int w, int elem_bytes, void* stream);
/* The flip test's merge, fp32 NCHW [batch, joints, h, w] in and out; perm_host: `joints` (<= 64) ints in HOST memory, a permutation of
 * 0..joints-1 (the left/right swap), copied into the kernel's arguments (no host-to-device copy: capturable):
 *   f[b,j,y,x]   = hm_flipped[b, perm[j], y, w-1-x]
 *   g[b,j,y,x]   = shift ? (x >= 1 ? f[b,j,y,x-1] : f[b,j,y,0]) : f[b,j,y,x]        (shift: Simple-Baselines' SHIFT_HEATMAP)
 *   out[b,j,y,x] = (hm[b,j,y,x] + g[b,j,y,x]) * 0.5f                                 (one fp32 add, one fp32 multiply)
 * out == hm (in place on the un-flipped maps) is allowed and gives the same bits; any other overlap of out with hm, and any overlap of out
 * with hm_flipped, is refused.  batch == 0 is a no-op.  One launch; 16-byte accesses when w % 4 == 0 and the pointers are 16-byte aligned. */
int sp_heat_map_flip_merge(const float* hm, const float* hm_flipped, const int32_t* perm_host, int batch, int joints, int h, int w, int shift,
                           float* out, void* stream);

/* ---- tracking: persistent identities across video frames, and the next frame's boxes without the detector ---------------------------------
 * (No new ABI version: these are additions.)  The track state is DEVICE memory the caller owns between frames, `slots` (1 .. 256) tracks:
 *   t_id int32 [slots] (0 = free), t_age int32 [slots] (frames the track was seen in), t_miss int32 [slots] (frames since it was last seen),
 *   t_kps double [slots, joints, 3], t_area double [slots], t_conf fp32 [slots] (the detector confidence carried along), next_id int32 [1]
 *   (the id the next new track gets; ids start at 1 when the caller initialises it to 1, and are never reused).
 * sp_track_associate: one image's kept poses - rows keep[seg[0] .. seg[0] + keep_count[0]) of kps [rows, joints, 3] / area [rows] /
 * box fp32 [rows, 5] (column 4: confidence), exactly what sp_topdown_plan, sp_pose_rescore and sp_oks_nms leave behind, in pick order;
 * n <= slots (more are ignored) - against the tracks:
 *   1. similarity [slots, slots] double: S[t, p] = oks_iou(track t's last pose, pose p) as sp_oks_nms computes it (the same function, no
 *      visibility threshold, sigmas_host: `joints` doubles in HOST memory or NULL = COCO's 17) for live t and p < n, -1 elsewhere;
 *   2. greedy matching over the pairs in (S descending, slot ascending, pose ascending) order: a pair matches when both sides are free and
 *      S >= match_thre (a NaN never matches);
 *   3. a matched track takes the pose (kps, area, confidence), miss = 0, age += 1;
 *   4. unmatched poses, in pick order, take the lowest free slot (free at the start of the call), and when none is left the unmatched track
 *      with the largest miss (ties: lowest slot): id = next_id++, age = 1, miss = 0;
 *   5. every other unmatched track: miss += 1, and freed (id = age = miss = 0) once miss > max_age;
 *   6. track_id int32 [rows]: the id of every kept row, 0 for the rest.
 * Two launches (a grid over the pairs, then one workgroup); no copy, no synchronisation, capturable.  Works with zero tracks and zero poses. */
int sp_track_associate(const double* kps, const double* area, const float* box, const int32_t* keep, const int32_t* keep_count,
                       const int32_t* seg, int rows, int joints, const double* sigmas_host, double match_thre, int max_age, int slots,
                       int32_t* t_id, int32_t* t_age, int32_t* t_miss, double* t_kps, double* t_area, float* t_conf, int32_t* next_id,
                       double* similarity, int32_t* track_id, void* stream);
/* The boxes of the tracks seen in the last frame (id != 0 && miss == 0), in slot order, as detector rows: det fp32 [1, max_det, 6] rows
 * (x1, y1, x2, y2, conf, cls), counts[0] = their number - the input sp_topdown_plan reads; max_det >= slots, rows counts[0] .. slots-1 are
 * zeroed.  fp32 from the key points cast to fp32, contraction off: min / max of the joints with c > in_vis_thre (of all joints when fewer
 * than two qualify; a NaN coordinate is skipped), scaled about its centre by box_expand, at least 1 px wide and high, clipped to
 * [0, img_w] x [0, img_h] (a NaN edge becomes 0).  One launch of one workgroup. */
int sp_track_boxes(const int32_t* t_id, const int32_t* t_miss, const double* t_kps, const float* t_conf, int slots, int joints,
                   float in_vis_thre, float box_expand, float cls, int img_w, int img_h, int max_det, float* det, int32_t* counts, void* stream);
/* Temporal smoothing of the tracked key points: the One-Euro filter (Casiez, Roussel, Vogel, CHI 2012) per track and joint, after
 * sp_track_associate and before the overlay.  (No new ABI version: an addition.)  It reads what sp_track_associate leaves behind for one
 * image - kps [rows, joints, 3], box fp32 [rows, 5], track_id [rows], keep / keep_count / seg (the count clamped to `slots` and to the keep
 * list's end as sp_track_associate clamps it), t_id [slots] - and now_dev, ONE double in DEVICE memory: the frame's time in seconds (not an
 * argument, so that a captured graph can be replayed with another time).  The filter state is DEVICE memory the caller owns between frames,
 * zero-initialised: s_id int32 [slots] (the track id a slot's filters belong to), s_x double [slots, joints, 2] (filtered position),
 * s_dx double [slots, joints, 2] (filtered speed, px / s), s_t double [slots, joints] (time of the last accepted sample), s_n int32
 * [slots, joints] (samples accepted; 0 = uninitialised).
 *   rows     kps_smooth [rows, joints, 3]: every row is the raw row, except a row the image kept (one of keep[seg[0] .. seg[0] + n)) whose
 *            track_id > 0 and is found in t_id: its slot is the lowest with t_id[slot] == track_id.  When s_id[slot] != track_id the slot
 *            was handed to another track: s_n[slot, :] = 0 and s_id[slot] = track_id (s_x, s_dx, s_t stay until a sample replaces them).
 *            Then every joint goes through the filter.  Tracks not seen in the frame keep their state.  The kept rows of one frame carry
 *            distinct ids (sp_track_associate's do).
 *   size     of the row: w = x2 - x1, h = y2 - y1 of its box in fp32, (w > h ? w : h) widened to double, replaced by 1.0 unless > 0:
 *            speeds are in body sizes per second, so the parameters do not depend on the resolution.
 *   joint    sample (x, y, c), state x^[2], dx^[2], t_last, n (simple_pose_amd/csrc/sp_smooth.h states it once for the device and the
 *            host).  fp64, contraction off, in this order, nothing but + - * / fabs and comparisons:
 *              not usable   c > in_vis_thre is false (a NaN c included), or x or y is not finite: the raw sample, state untouched;
 *              (re)start    else if n == 0, or now - t_last > 0 is false, or now - t_last > max_gap: x^ = (x, y), dx^ = 0, n = 1,
 *                           t_last = now, the raw sample;
 *              update       else Te = now - t_last and per axis  d = (x - x^) / Te;  rd = (TWO_PI * d_cutoff) * Te;  ad = rd / (rd + 1.0);
 *                           dx^ = ad * d + (1.0 - ad) * dx^;  fc = min_cutoff + beta * (fabs(dx^) / size);  r = (TWO_PI * fc) * Te;
 *                           a = r / (r + 1.0);  x^ = a * x + (1.0 - a) * x^ unless x == x^ (then x^ stays: the blend of two equal values rounds to
 *                           them only within an ulp, and a pose at rest comes out exactly unchanged);  then n += 1, t_last = now, and the
 *                           output is (x^x, x^y, c).
 *            TWO_PI is the double 6.283185307179586; c is never filtered.
 * slots 1 .. 256, joints 1 .. 64, rows >= 1; min_cutoff > 0, d_cutoff > 0, beta >= 0, max_gap > 0, all finite, in_vis_thre finite.
 * One launch (one 64-lane workgroup per row, lane = joint); no copy, no synchronisation, capturable.  Works with zero kept poses. */
int sp_track_smooth(const double* kps, const float* box, const int32_t* track_id, const int32_t* keep, const int32_t* keep_count,
                    const int32_t* seg, int rows, int joints, const int32_t* t_id, int slots, const double* now_dev, double min_cutoff,
                    double beta, double d_cutoff, double max_gap, double in_vis_thre, int32_t* s_id, double* s_x, double* s_dx, double* s_t,
                    int32_t* s_n, double* kps_smooth, void* stream);

/* The three tracker entries for `images` (1 .. 256) video streams in ONE call, with a launch count that does not depend on `images`.  (No new
 * ABI version: these are additions.)  The state is stream-major: every state array of the single-image entry gains a leading [images]
 * dimension - t_id / t_age / t_miss [images, slots], t_kps [images, slots, joints, 3], t_area / t_conf [images, slots], next_id [images] (ids
 * start at 1 per stream and are never reused within a stream), similarity [images, slots, slots], s_id [images, slots], s_x / s_dx [images,
 * slots, joints, 2], s_t / s_n [images, slots, joints], now_dev double [images] (one time per stream, in DEVICE memory).  Image s reads the
 * rows keep[seg[s] .. seg[s] + n_s) of the shared kps / area / box [rows, ...] - what sp_topdown_plan, sp_pose_rescore and sp_oks_nms leave
 * behind for a batch - with n_s = keep_count[s] clamped as the single-image entries clamp it (to 0, to `slots`, to rows - seg[s]); keep_count
 * and seg hold at least `images` entries.  Per stream the arithmetic, the greedy order and the tie rules are the single-image entry's (the
 * same kernels: the single-image entries are images = 1 calls), so every stream's result equals it bit for bit; streams never read each
 * other's state.  All are capturable, without copy or synchronisation, and work with zero tracks, zero poses and empty segments.
 * sp_track_associate_images: track_id int32 [rows] gets the id of every kept row of every image and 0 for every other row; the kept rows of
 *   different images are distinct rows (sp_oks_nms's are).  Two launches: a grid over (pairs, images), then one workgroup per image.
 * sp_track_boxes_images: det fp32 [images, max_det, 6] and counts [images] under sp_track_boxes' rules per stream (rows counts[s] .. slots-1
 *   of block s zeroed, rows from `slots` on untouched); img_w and img_h are shared.  One launch, one workgroup per image.
 * sp_track_smooth_images: a row is filtered with the state, the tracks (t_id block) and the time of the image that kept it (the lowest such
 *   image); every other row is the raw row.  One launch, one 64-lane workgroup per row. */
int sp_track_associate_images(const double* kps, const double* area, const float* box, const int32_t* keep, const int32_t* keep_count,
                              const int32_t* seg, int images, int rows, int joints, const double* sigmas_host, double match_thre, int max_age,
                              int slots, int32_t* t_id, int32_t* t_age, int32_t* t_miss, double* t_kps, double* t_area, float* t_conf,
                              int32_t* next_id, double* similarity, int32_t* track_id, void* stream);
int sp_track_boxes_images(const int32_t* t_id, const int32_t* t_miss, const double* t_kps, const float* t_conf, int images, int slots, int joints,
                          float in_vis_thre, float box_expand, float cls, int img_w, int img_h, int max_det, float* det, int32_t* counts,
                          void* stream);
int sp_track_smooth_images(const double* kps, const float* box, const int32_t* track_id, const int32_t* keep, const int32_t* keep_count,
                           const int32_t* seg, int images, int rows, int joints, const int32_t* t_id, int slots, const double* now_dev,
                           double min_cutoff, double beta, double d_cutoff, double max_gap, double in_vis_thre, int32_t* s_id, double* s_x,
                           double* s_dx, double* s_t, int32_t* s_n, double* kps_smooth, void* stream);

/* ---- overlay: the kept poses of one image drawn into it - boxes, limbs, joints, coloured by person (track id) or by part ------------------
 * (No new ABI version: these are additions.)  uint8 BGR [h, w, 3] in and out, 1 <= h, w <= 16384; it reads exactly what sp_oks_nms (and
 * sp_track_associate) leave behind: rows keep[seg[image] .. seg[image] + keep_count[image]) of kps [rows, joints, 3] / box fp32 [rows, 5] /
 * track_id int32 [rows] (or NULL), in pick order, the count clamped to `rows` and to the keep list's end as sp_track_associate clamps it.
 * The pixel rules (simple_pose_amd/csrc/sp_render.h states them once for the device and the host; all integer but one comparison):
 *   primitive    ONE kind, the capsule {ax, ay, bx, by, r}: every point within r of the segment A-B, int32 in 1/16 px, with a BGR colour.
 *                q(v) = (int32) rint(v * 16.0) (double, ties to even); a coordinate that is not finite or has |v| > 32768 makes the
 *                primitive empty (r = -1).  A joint is visible iff its c > in_vis_thre (a NaN c is not).
 *   per person   4 + edges + joints slots, in this order: the 4 box edges (top, right, bottom, left; radius box_r, all empty when
 *                box_r == 0), the limbs in skeleton order (A -> B of edge[e], radius limb_r, empty unless both joints are visible), the
 *                joints in index order (A == B, radius joint_r, empty when not visible).  No compaction: empty slots stay in the array.
 *   order        primitive index = p * (4 + edges + joints) + slot, applied in ascending order; person slot p holds the pose at pick
 *                position n - 1 - p, so persons are painted in reverse pick order and the best pose lies on top.
 *   coverage     of pixel (x, y): 16 samples S = (16x + 4i + 2, 16y + 4j + 2), i, j in 0..3.  In int64, exactly: t = AS.AB, L = AB.AB,
 *                c = ASx * ABy - ASy * ABx.  A sample is inside by the first rule that applies:  L == 0 or t <= 0: |AS|^2 <= r^2;
 *                t >= L: |BS|^2 <= r^2;  otherwise (double)c * (double)c <= (double)(r * r) * (double)L (two fp64 products, each rounded
 *                once; every conversion is exact).  k = the number of inside samples, 0..16.
 *   blend        a = k * opacity; per channel out = (in * (256 - a) + colour * a + 128) >> 8, primitive after primitive, each step on the
 *                previous step's result.
 *   colour       SP_RENDER_COLOUR_PERSON: palette[(track_id - 1) % palette_n] when track_id is given and > 0, else
 *                palette[pick position % palette_n].  SP_RENDER_COLOUR_PART: limb e palette[e % palette_n], joint j
 *                palette[j % palette_n], boxes the person colour.
 * style_host is HOST memory, validated and copied into the kernel arguments (no host-to-device copy: capturable). */
#define SP_RENDER_COLOUR_PERSON 0
#define SP_RENDER_COLOUR_PART 1
#define SP_RENDER_MAX_EDGES 64
#define SP_RENDER_MAX_PALETTE 32
#define SP_RENDER_MAX_RADIUS 1024 /* 1/16 px: 64 px */
typedef struct sp_render_style {
    int32_t edges;                          /* 0 .. 64 */
    int32_t edge[SP_RENDER_MAX_EDGES][2];   /* joint indices, each < joints */
    int32_t joint_r, limb_r, box_r;         /* radii in 1/16 px, 0 .. 1024; box_r == 0: no boxes */
    int32_t opacity;                        /* 0 .. 16 (sixteenths) */
    double in_vis_thre;
    int32_t colour_by;                      /* SP_RENDER_COLOUR_* */
    int32_t palette_n;                      /* 1 .. 32 */
    unsigned char palette[SP_RENDER_MAX_PALETTE][3];   /* BGR */
} sp_render_style;
/* bytes of the primitive array for `rows` person slots (1 .. 2048) */
int sp_render_workspace_bytes(int rows, int joints, int edges, int64_t* bytes);
/* Two launches (one thread per primitive slot; one 256-thread workgroup per 64 x 16 pixel tile, which scans the primitive array in chunks
 * of 256, lists the primitives whose box meets the tile in index order and applies them to pixels held in registers); no copy, no
 * synchronisation, capturable.  dst == src (in place) is allowed, a tile nothing touches is then skipped; any other overlap of src and dst
 * is refused; out of place, untouched tiles are copied.  4-byte accesses when w % 4 == 0 and both pointers are 4-byte aligned, bytes
 * otherwise.  rows == 0 is a no-op (a copy when dst != src; kps .. workspace are not read).  workspace: sp_render_workspace_bytes, 8-byte
 * aligned device memory, overwritten by every call. */
int sp_render_poses_u8c3(const unsigned char* src, unsigned char* dst, int h, int w, const double* kps, const float* box,
                         const int32_t* track_id /* may be NULL */, const int32_t* keep, const int32_t* keep_count, const int32_t* seg,
                         int image, int rows, int joints, const sp_render_style* style_host, void* workspace, void* stream);

/* ---- overlay text: one label per kept person (track id, scores) and one caption per image, formatted and rasterised on the device ------------
 * (No new ABI version: these are additions.)  uint8 BGR [h, w, 3] IN PLACE, 1 <= h, w <= 16384, behind sp_render_poses_u8c3 on the same
 * stream; it reads the same rows (kept count n and pick order as above) plus score fp64 [rows].  The rules (simple_pose_amd/csrc/sp_label.h
 * states them once for the device and the host; all integer but the two conversions marked (*)):
 *   font         sp_font.h: 5 x 7 pixels per glyph, the 95 printable ASCII characters 0x20 .. 0x7E; a glyph is 7 bytes, one per row from the
 *                top, bit 4 the leftmost column.  A character cell is 6 x 8 font pixels (an empty column right, an empty row below).
 *   template     up to 32 bytes: printable ASCII is literal, bytes 0x01 .. 0x05 are fields, anything else is refused.
 *                  0x01 {id}     label    track_id[row] in decimal when track_id is given and the id is > 0, else pick position + 1
 *                  0x02 {score}  label    score[row] (double)
 *                  0x03 {conf}   label    box[row][4] (float, widened to double)
 *                  0x04 {n}      caption  the image's kept count n
 *                  0x05 {image}  caption  the image index
 *                A label template holds label fields only (a caption field in it is refused).  The caption's text is DEVICE memory, row
 *                `image` of caption uint8 [images][64], ending at the first NUL or at byte 64: a printable byte is literal, 0x04 / 0x05
 *                are its fields, any other byte (a label field too) prints '?'.
 *   numbers      {score}, {conf}: a value that is not finite or is < 0 prints "?"; otherwise c = (int64) rint(min(v, 99.99) * 100.0) (*: one
 *                double product, ties to even) and the text is c / 100 in decimal, '.', c % 100 as two digits.
 *   truncation   formatted text longer than 24 characters (label) or 64 (caption) is cut there.  Empty text draws nothing.
 *   plate        text of L characters at scale s (1 .. 8): (6L + 1) * s wide, 9 * s high, its corner at (x0, y0).  Font pixel (col, row) of
 *                character i covers the s x s image pixels from (x0 + (1 + 6i + col) * s, y0 + (1 + row) * s).
 *   label at     bx = q(x1) >> 4, by = q(y1) >> 4 of the box's first corner (q as above (*), arithmetic shift; a coordinate q rejects draws
 *                no label).  y0 = by - 9s; if y0 < 0: y0 = by (inside the box).  x0 = bx; if x0 + width > w: x0 = w - width; if x0 < 0:
 *                x0 = 0.  Then the plate is clipped to the image.
 *   caption at   a corner, s pixels from both edges: x0 = s (left) or w - s - width (right), y0 = s (top) or h - s - height (bottom); then
 *                clipped to the image.
 *   colours      label plate: the person colour of SP_RENDER_COLOUR_PERSON (whatever the overlay's colour_by); its text black when
 *                29 * B + 150 * G + 77 * R >= 32768, white otherwise.  Caption: black plate, white text.
 *   blend        a = 16 * opacity (sixteenths, 0 .. 16); per channel out = (in * (256 - a) + c * a + 128) >> 8 with c the text colour
 *                where a glyph bit is set and the plate colour elsewhere on the plate.  One blend per label per pixel; a later label
 *                blends on the earlier result.
 *   order        record p < rows is person slot p = the pose at pick position n - 1 - p (empty for p >= n), applied in ascending order:
 *                the best pose's label lies on top.  The caption is the last record.  All of it after all capsules. */
#define SP_LABEL_MAX_TEMPLATE 32
#define SP_LABEL_MAX_CHARS 24
#define SP_LABEL_CAPTION_BYTES 64
#define SP_LABEL_MAX_SCALE 8
#define SP_LABEL_FIELD_ID 1
#define SP_LABEL_FIELD_SCORE 2
#define SP_LABEL_FIELD_CONF 3
#define SP_LABEL_FIELD_N 4
#define SP_LABEL_FIELD_IMAGE 5
#define SP_LABEL_CORNER_TL 0
#define SP_LABEL_CORNER_TR 1
#define SP_LABEL_CORNER_BL 2
#define SP_LABEL_CORNER_BR 3
typedef struct sp_label_style {
    int32_t template_len;                               /* 0 .. 32; 0: no labels */
    unsigned char label_template[SP_LABEL_MAX_TEMPLATE];
    int32_t label_scale, label_opacity;                 /* 1 .. 8; sixteenths, 0 .. 16 */
    int32_t caption_scale, caption_opacity;
    int32_t caption_corner;                             /* SP_LABEL_CORNER_* */
    int32_t palette_n;                                  /* 1 .. 32 */
    unsigned char palette[SP_RENDER_MAX_PALETTE][3];    /* BGR: the overlay's */
} sp_label_style;
/* HOST function: the 7 row bytes of character ch (0x20 .. 0x7E); -1 with sp_last_error() for any other ch or a null pointer */
int sp_render_font_glyph(int ch, unsigned char rows7[7]);
/* bytes of the record array for `rows` person slots (0 .. 2048) and the caption */
int sp_render_labels_workspace_bytes(int rows, int64_t* bytes);
/* Two launches (label_format_kernel: one thread per person slot and one for the caption formats the text and writes a record - clipped and
 * unclipped rectangle, two colours, alpha, scale, length, characters; no compaction.  label_tile_kernel: one 256-thread workgroup per
 * 64 x 16 pixel tile scans the records in chunks of 256, lists in index order those whose plate meets the tile and applies them to pixels
 * held in registers, the font in LDS; a tile nothing touches is neither read nor written).  No copy, no synchronisation, capturable.
 * 4-byte accesses when w % 4 == 0 and img is 4-byte aligned, bytes otherwise.  template_len == 0 draws no labels, caption_dev == NULL no
 * caption; neither, or rows == 0 without a caption, is a no-op.  style_host is HOST memory, validated (scales, opacities, corner,
 * palette_n, every template byte) and copied into the kernel arguments.  workspace: sp_render_labels_workspace_bytes, 4-byte aligned
 * device memory, overwritten by every call.  Every pointer but track_id and caption_dev is required (a null one is refused). */
int sp_render_labels_u8c3(unsigned char* img, int h, int w, const float* box, const double* score,
                          const int32_t* track_id /* may be NULL */, const int32_t* keep, const int32_t* keep_count, const int32_t* seg,
                          int image, int rows, const sp_label_style* style_host, const unsigned char* caption_dev /* may be NULL */,
                          void* workspace, void* stream);

/* ---- redaction: the heads or the whole persons of one image hidden behind a mosaic or a constant colour ------------------------------------
 * (No new ABI version: these are additions.)  uint8 BGR [h, w, 3] in and out, 1 <= h, w <= 16384; it reads the rows the overlay reads:
 * keep[seg[image] .. seg[image] + keep_count[image]) of kps fp64 [rows, joints, 3] / box fp32 [rows, 5], the count clamped as above.  The
 * rules (simple_pose_amd/csrc/sp_redact.h states them once for the device and the host; all integer but q, the overlay's quantisation
 * q(v) = (int32) rint(v * 16.0), which rejects a value that is not finite or has |v| > 32768):
 *   cells        the frame is cut into cell x cell pixel cells on a grid anchored at (0, 0), cell one of 4, 8, 16, 32, 64; the cells of the
 *                last column / row are clipped to the image.  A cell is redacted as a whole or left alone: no partial cells, no blending,
 *                so no original pixel of a redacted cell survives and the order of the persons does not matter.
 *   modes        SP_REDACT_MOSAIC: every pixel of a redacted cell becomes, per channel, (sum + n / 2) / n, the sum over the n pixels of
 *                the clipped cell in the SOURCE image (never the canvas: a cell two persons hit is the cell one person hits).
 *                SP_REDACT_FILL: every pixel of a redacted cell becomes the constant BGR colour `fill`.
 *   regions      one per kept person, in 1/16 px: a disc {cx, cy, r} or a rectangle {ax, ay, bx, by} (ax <= bx, ay <= by), or empty.  An
 *                empty slot stays in the array: no compaction.  "The box" below is (q(x1), q(y1), q(x2), q(y2)) of the person's box with
 *                both axes ordered by min / max; q rejecting any of the four rejects the box.
 *     SP_REDACT_PERSON   the rectangle of the box; empty when the box is rejected.
 *     SP_REDACT_HEAD     head joint head_joint[i], i < head_joints (1 .. 8 of them), is visible iff its c > in_vis_thre (a NaN c is not)
 *                and q accepts both of its coordinates.  With at least one visible head joint the region is a disc: (minx, maxx, miny,
 *                maxy) the bounding box of the visible head joints' quantised coordinates; cx = (minx + maxx) >> 1, cy = (miny + maxy) >> 1;
 *                e = max(maxx - minx, maxy - miny); s = the longer side of the box, 0 when the box is rejected;
 *                r0 = max(e >> 1, (s * head_min) >> 8); r = min((r0 * expand) >> 4, 1 << 20).  head_min: 1/256 of the box side, 0 .. 256;
 *                expand: sixteenths, 16 .. 64.  r == 0 is still a point: the cell that holds it is redacted.
 *                With no visible head joint, `fallback`: SP_REDACT_FALLBACK_BOX_TOP the rectangle with the box's x range and y from y1 to
 *                y1 + (((y2 - y1) * top_frac) >> 8) (top_frac: 1/256, 0 .. 256; empty when the box is rejected);
 *                SP_REDACT_FALLBACK_BOX the person rectangle; SP_REDACT_FALLBACK_NONE empty.
 *   hit          a cell is redacted iff its closed rectangle [16 X0, 16 X1 + 15] x [16 Y0, 16 Y1 + 15] (X0 .. X1, Y0 .. Y1 its clipped pixel
 *                range) meets a region.  Rectangle: the intervals overlap on both axes.  Disc: dx = max(lo - cx, 0, cx - hi) on x, dy
 *                likewise on y, and dx * dx + dy * dy <= r * r in int64.
 * style_host is HOST memory, validated and copied into the kernel arguments (no host-to-device copy: capturable). */
#define SP_REDACT_HEAD 0
#define SP_REDACT_PERSON 1
#define SP_REDACT_MOSAIC 0
#define SP_REDACT_FILL 1
#define SP_REDACT_FALLBACK_BOX_TOP 0
#define SP_REDACT_FALLBACK_BOX 1
#define SP_REDACT_FALLBACK_NONE 2
#define SP_REDACT_MAX_HEAD_JOINTS 8
#define SP_REDACT_MAX_RADIUS (1 << 20) /* 1/16 px */
typedef struct sp_redact_style {
    int32_t region;                                     /* SP_REDACT_HEAD / SP_REDACT_PERSON */
    int32_t mode;                                       /* SP_REDACT_MOSAIC / SP_REDACT_FILL */
    int32_t cell;                                       /* 4, 8, 16, 32 or 64 pixels */
    int32_t expand;                                     /* sixteenths, 16 .. 64 */
    int32_t head_min;                                   /* 1/256 of the box's longer side, 0 .. 256 */
    int32_t head_joints;                                /* 1 .. 8 */
    int32_t head_joint[SP_REDACT_MAX_HEAD_JOINTS];      /* joint indices, each < joints (read for SP_REDACT_HEAD only) */
    int32_t fallback;                                   /* SP_REDACT_FALLBACK_* */
    int32_t top_frac;                                   /* 1/256 of the box's height, 0 .. 256 */
    double in_vis_thre;
    unsigned char fill[3];                              /* BGR */
} sp_redact_style;
/* bytes of the region array for `rows` person slots (0 .. 2048) */
int sp_redact_workspace_bytes(int rows, int64_t* bytes);
/* Two launches (redact_regions_kernel: one thread per person slot writes a region record with its pixel bounding box; redact_tile_kernel:
 * one 256-thread workgroup per tile of 64 x max(16, cell) pixels scans the records in chunks of 256, marks the tile's hit cells, and only
 * if one is hit reads the tile's source pixels once, reduces the cell sums - shuffles inside a wave, LDS between waves - and writes the
 * tile once); no copy, no synchronisation, capturable.  dst == src (in place) is allowed: a tile nothing touches is then neither read nor
 * written; any other overlap of src and dst is refused; out of place, untouched tiles are copied.  4-byte accesses when w % 4 == 0 and
 * both pointers are 4-byte aligned, bytes otherwise.  rows == 0 is a no-op in place and a copy out of place (kps .. workspace are not
 * read).  workspace: sp_redact_workspace_bytes, 4-byte aligned device memory, overwritten by every call; kps 8-byte aligned. */
int sp_redact_u8c3(const unsigned char* src, unsigned char* dst, int h, int w, const double* kps, const float* box, const int32_t* keep,
                   const int32_t* keep_count, const int32_t* seg, int image, int rows, int joints, const sp_redact_style* style_host,
                   void* workspace, void* stream);

/* ---- heat overlay: the kept persons' joint heat maps blended into one image ----------------------------------------------------------------
 * (No new ABI version: these are additions.)  uint8 BGR [h, w, 3] in and out, 1 <= h, w <= 16384.  hm: fp32 [>= rows, joints, hm_h, hm_w]
 * (NCHW; slot `row` of the frame is map `row`), trans_inv fp32 [rows, 2, 3] (heat-map px -> image px, as sp_topdown_plan writes it).  The
 * live persons of `image` are the rows keep[lo + p], p < n, with (n, lo) the clamped count and offset the overlay uses; a row outside
 * 0 .. rows - 1 is skipped.  The rules (simple_pose_amd/csrc/sp_heat.h states them once for the device and the host; all integer
 * but the three floating-point steps named here, each one correctly rounded IEEE operation or a sequence run with contraction off):
 *   plane        per live person a u8 [hm_h, hm_w] plane: m(y, x) = the maximum of hm[row, j, y, x] over the joints j < joints whose bit is
 *                set in joint_mask (a NaN loses against every number; no such bit: the person is skipped); q8 = sp_heat_q(m, scale):
 *                v = m * scale (ONE fp32 multiply); NaN -> 0, v >= 255 -> 255, v > 0 -> (uint8) v by truncation, else 0.
 *   forward map  F = sp_invert_affine((double) trans_inv[row]) (image px -> heat-map px, pixel centres), c[i] = (int64) rint(F[i] * 65536.0).
 *                The person is skipped when an F[i] is not finite, when F[0] = F[1] = F[3] = F[4] = 0 (a singular trans_inv, a dead slot's
 *                zeros included), when a linear coefficient has |F| > 1024 or an offset |F| > 2^20.  Image pixel (X, Y), int64:
 *                U = c[0] X + c[1] Y + c[2], V = c[3] X + c[4] Y + c[5] (1/65536 px); u = U >> 8, v = V >> 8 (arithmetic);
 *                xi = u >> 8, fx = u & 255, yi = v >> 8, fy = v & 255.
 *   sample       taps p(xi + dx, yi + dy), dx, dy in {0, 1}; a tap outside [0, hm_w) x [0, hm_h) reads 0;
 *                val = ((256 - fx)(256 - fy) p00 + fx (256 - fy) p10 + (256 - fx) fy p01 + fx fy p11 + 32768) >> 16, in 0 .. 255.
 *   combine      Vmax = the maximum of val over the image's live persons (0 where none reaches): the order of the persons does not matter.
 *   blend        Vmax < threshold (1 .. 255): the pixel keeps its source bytes.  Otherwise colour = lut[Vmax] (lut: 256 BGR triples in
 *                DEVICE memory), w = opacity16 * a (opacity16 0 .. 16; a = 256 for SP_HEAT_ALPHA_CONSTANT, a = Vmax + (Vmax >> 7) for
 *                SP_HEAT_ALPHA_VALUE), and per channel out = (src (4096 - w) + colour w + 2048) >> 12.
 *   box          every record carries a pixel bounding box for binning persons to tiles: the image of [-2, hm_w + 1] x [-2, hm_h + 1]
 *                under trans_inv, padded by 2 px and clipped to 0 .. 16383; the record kernel then proves in int64, on the four rectangles
 *                around the box, that U and V cannot reach a tap there, and widens the box to everything when it cannot.  It never
 *                changes a pixel's value.
 * style_host is HOST memory, validated and copied into the kernel arguments (no host-to-device copy: capturable). */
#define SP_HEAT_ALPHA_CONSTANT 0
#define SP_HEAT_ALPHA_VALUE 1
#define SP_HEAT_MAX_MAP 256
typedef struct sp_heat_style {
    uint64_t joint_mask;                                /* bit j: joint j takes part in the maximum */
    float scale;                                        /* finite, >= 0; 255 maps [0, 1] onto 0 .. 255 */
    int32_t threshold;                                  /* 1 .. 255 */
    int32_t opacity16;                                  /* 0 .. 16 */
    int32_t alpha;                                      /* SP_HEAT_ALPHA_* */
} sp_heat_style;
/* bytes of the records and the u8 planes of `rows` person slots (0 .. 2048) with hm_h x hm_w maps (1 .. 256 each way) */
int sp_heat_overlay_workspace_bytes(int rows, int hm_h, int hm_w, int64_t* bytes);
/* Two launches (heat_planes_kernel: one 256-thread workgroup per person slot; a dead slot gets an empty record and reads nothing, a live
 * one has its `joints` maps reduced to the u8 plane - 16-byte loads along x when hm_w % 4 == 0 and hm is 16-byte aligned, scalar loads
 * otherwise - and its record written: c[6] and the box.  heat_tile_kernel: one 256-thread workgroup per 64 x 16 pixel tile scans the
 * records in chunks of 256 into an LDS list of the persons that can reach the tile, and every pixel takes the maximum over the listed
 * persons and is blended); no copy, no synchronisation, capturable.  dst == src (in place) is allowed: a tile with an empty list is then
 * neither read nor written; any other overlap of src and dst is refused; out of place such a tile is copied.  4-byte stores when
 * w % 4 == 0 and both pointers are 4-byte aligned, bytes otherwise.  rows == 0 is a no-op in place and a copy out of place (hm .. workspace
 * are not read).  workspace: sp_heat_overlay_workspace_bytes, 8-byte aligned device memory, overwritten by every call; hm and trans_inv
 * 4-byte aligned. */
int sp_heat_overlay_u8c3(const unsigned char* src, unsigned char* dst, int h, int w, const float* hm, int joints, int hm_h, int hm_w,
                         const float* trans_inv, const int32_t* keep, const int32_t* keep_count, const int32_t* seg, int image, int rows,
                         const sp_heat_style* style, const unsigned char* lut, void* workspace, void* stream);

/* ---- baseline JPEG decoding: file bytes in, uint8 BGR [H,W,3] images out ---------------------------------------------------------------------
 * (No new ABI version: these are additions.)  The pixels are libjpeg-turbo's default decode (cv2.imread, PIL) bit for bit: Huffman decode,
 * the "islow" integer IDCT, "fancy" chroma upsampling, 16.16 fixed-point YCbCr -> BGR; a grayscale file gives three equal channels.  EXIF
 * orientation is not applied.  Accepted: SOF0, 8-bit samples, 1 or 3 components, luma sampling 1x1, 2x1 or 2x2 with 1x1 chroma, one
 * interleaved scan, 8-bit quantisation tables, APPn / COM segments skipped.  Anything else is refused by sp_jpeg_parse with its own code
 * (progressive SOF2 files: SP_JPEG_EPROGRESSIVE, and sp_jpeg_parse_scans below takes them); there is no CPU decode path. */
#define SP_JPEG_ETRUNCATED (-10)   /* a header segment runs past the end of the buffer (the message names the byte offset) */
#define SP_JPEG_ENOT_JPEG (-11)    /* no SOI, or no marker where one has to be */
#define SP_JPEG_EPROGRESSIVE (-12) /* SOF2 */
#define SP_JPEG_EEXTENDED (-13)    /* SOF1, SOF3, SOF5 .. SOF7 (extended sequential, lossless, hierarchical) */
#define SP_JPEG_EARITHMETIC (-14)  /* SOF9 .. SOF15, DAC */
#define SP_JPEG_EPRECISION (-15)   /* sample precision other than 8 bits */
#define SP_JPEG_ECOMPONENTS (-16)  /* neither 1 nor 3 components */
#define SP_JPEG_ESAMPLING (-17)    /* sampling factors other than 1x1 / 2x1 / 2x2 luma with 1x1 chroma (4:4:0, 4:1:1, ...) */
#define SP_JPEG_EADOBE (-18)       /* Adobe APP14 segment with a colour transform other than YCbCr on a 3-component file */
#define SP_JPEG_ESCANS (-19)       /* more than one scan, a scan that does not interleave every component, no scan */
#define SP_JPEG_ENO_TABLE (-20)    /* a component selects a quantisation or Huffman table the file does not define */
#define SP_JPEG_EBAD_TABLE (-21)   /* malformed DQT / DHT (16-bit quantisation values, counts that are no prefix code, bad index) */
#define SP_JPEG_ESIZE (-22)        /* zero or > 16384 width / height, or a file of 2 GiB and more */

/* One file.  sp_jpeg_parse fills everything down to out_bytes; the caller fills the placement fields before sp_jpeg_decode_batch. */
typedef struct sp_jpeg_desc {
    int32_t width, height, components;                /* components: 1 (grayscale) or 3 (YCbCr) */
    int32_t h_samp[3], v_samp[3];                     /* sampling factors (1,1 for a single component) */
    int32_t quant_sel[3], dc_sel[3], ac_sel[3];       /* table selectors 0..3 per component */
    int32_t restart_interval;                         /* MCUs per restart segment, 0 = no restart markers */
    int32_t mcus_x, mcus_y;                           /* ceil(width / (8 hmax)), ceil(height / (8 vmax)) */
    int32_t ecs_offset, ecs_end;                      /* the entropy-coded data is bytes [ecs_offset, ecs_end) of the file */
    int32_t segments;                                 /* restart segments found by scanning for FF D0..D7 (1 without markers) */
    int32_t file_bytes;
    int32_t coef_count;                               /* int16 coefficients: 64 per block, MCU padding included */
    int32_t plane_bytes;                              /* uint8 component planes: 64 per block */
    int32_t out_bytes;                                /* height * width * 3 */
    int32_t seg_index;                                /* caller: this file's first entry in `seg_offsets` */
    int32_t reserved;
    int64_t file_offset;                              /* caller: the file's first byte in `bytes` */
    int64_t coef_offset;                              /* caller: in int16 elements into `coef` */
    int64_t plane_offset;                             /* caller: in bytes into `planes`, a multiple of 8 */
    int64_t out_offset;                               /* caller: in bytes into `out` */
    uint16_t quant[4][64];                            /* de-zigzagged to natural (row-major) order */
    uint8_t huff_counts[8][16];                       /* [4 * class + index]: codes of length 1..16 (class 0 = DC, 1 = AC) */
    uint8_t huff_values[8][256];                      /* the symbols in code order */
} sp_jpeg_desc;

/* Host only, no GPU call: parse the headers of one file (`size` bytes at `data`, HOST memory) into *desc.  Every marker length is checked
 * against the buffer.  seg_offsets (HOST, may be NULL with seg_capacity 0) receives the file offset of the first entropy byte of each
 * restart segment, at most seg_capacity of them; desc->segments is the number found (call again with a larger array when it exceeds the
 * capacity).  Segment s ends two bytes before segment s + 1 starts (at its FF Dn), the last one at ecs_end (the EOI marker, or the end
 * of a file that has none).  Returns SP_OK or one of SP_JPEG_E* with the reason, and where relevant the byte offset, in sp_last_error. */
int sp_jpeg_parse(const uint8_t* data, int64_t size, sp_jpeg_desc* desc, int32_t* seg_offsets, int32_t seg_capacity);

/* status bits sp_jpeg_decode_batch writes per image (0 = decoded) */
#define SP_JPEG_STATUS_TRUNCATED 1  /* entropy data of a segment ended before its last block */
#define SP_JPEG_STATUS_BAD_CODE 2   /* bits that are no Huffman code */
#define SP_JPEG_STATUS_BAD_RUN 4    /* AC run past coefficient 63 */
#define SP_JPEG_STATUS_SEGMENTS 8   /* segments != ceil(MCUs / restart interval) */
#define SP_JPEG_STATUS_BAD_TABLE 16 /* Huffman counts that are no prefix code */

/* sp_jpeg_decode_batch `stages` */
#define SP_JPEG_STAGE_ENTROPY 1
#define SP_JPEG_STAGE_IDCT 2
#define SP_JPEG_STAGE_COLOR 4
#define SP_JPEG_STAGE_ALL 7

/* Decode `count` files of mixed sizes and sampling.  descs_host / descs_dev: the same `count` descriptors in HOST and in DEVICE memory (the
 * host copy sizes the launches and is checked against every arena size below before anything is launched).  bytes: all files packed in
 * one DEVICE buffer of bytes_size bytes; seg_offsets int32 [seg_count] DEVICE: the arrays sp_jpeg_parse filled, file s at seg_index;
 * coef int16 [coef_size], planes uint8 [planes_size], out uint8 [out_size]: DEVICE arenas, image i at its *_offset; the regions of
 * different images must not overlap (not checked).  status int32 [count] DEVICE.  Image i: out + out_offset = uint8 [height, width, 3] BGR.
 * `stages`: SP_JPEG_STAGE_ALL, or a subset (a bench / test runs them one at a time; later stages read what earlier ones left):
 *   entropy  one launch that zeroes every image's coefficient region (and nothing between them), then jpeg_entropy_kernel: one wave per image builds the Huffman lookahead tables in
 *            LDS, lane s decodes restart segments s, s + 64, ... (a file without restart markers: lane 0 alone) into int16 coefficients in
 *            natural order, component after component, each a row-major grid of (mcus_x h) x (mcus_y v) blocks; writes status;
 *   idct     jpeg_idct_kernel: dequantise + islow IDCT, 8 lanes per block -> uint8 component planes (pitch = 8 * blocks per row);
 *   color    jpeg_color_kernel: fancy upsampling + YCbCr -> BGR.
 * A damaged stream ends in a non-zero status, never in an access outside the image's own regions; its pixels are unspecified.
 * Nothing synchronises; count == 0 is a no-op. */
int sp_jpeg_decode_batch(const sp_jpeg_desc* descs_host, const sp_jpeg_desc* descs_dev, int count, const uint8_t* bytes, int64_t bytes_size,
                         const int32_t* seg_offsets, int64_t seg_count, int16_t* coef, int64_t coef_size, uint8_t* planes, int64_t planes_size,
                         uint8_t* out, int64_t out_size, int32_t* status, int stages, void* stream);

/* ---- progressive JPEG decoding: a second parser and a second entropy stage that fill the same coefficient arena ---------------------------
 * (No new ABI version: these are additions.)  A complete progressive file goes through the same islow IDCT, fancy upsampling and colour
 * conversion as a baseline one, so sp_jpeg_parse_scans + sp_jpeg_progressive_entropy replace sp_jpeg_parse + the entropy stage, and
 * sp_jpeg_decode_batch(stages = IDCT | COLOR) finishes the image: the pixels are libjpeg-turbo's bit for bit.
 * Accepted: SOF2, 8-bit samples, 1 or 3 components, the sampling factors and the Adobe rule of the baseline parser, any number of scans
 * (spectral selection and successive approximation, DC scans interleaved or not, a new DHT / DRI before any scan).
 * Refused: a scan header libjpeg rejects or warns about (SP_JPEG_EBAD_SCAN); a progression that ends before every component has its DC
 * and its zigzag coefficients 1..9 down to bit 0 (SP_JPEG_EINCOMPLETE: libjpeg-turbo smooths such files between blocks, the ordinary
 * IDCT does not give its pixels; coefficients 10..63 may stay unsent or unrefined); a DQT after the first SOS (SP_JPEG_EBAD_TABLE);
 * SOF0 with several scans (SP_JPEG_ESCANS: baseline files go to sp_jpeg_parse); everything sp_jpeg_parse refuses, with the same codes.
 * Block geometry.  A scan of two or three components is interleaved over the frame's MCU grid (mcus_x x mcus_y, h x v blocks per
 * component per MCU), like the baseline scan.  A scan of ONE component is not interleaved: its MCU is one block, it covers
 * ceil(comp_width / 8) x ceil(comp_height / 8) blocks with comp_width = ceil(width * h / hmax) - not the MCU-padded grid - and its
 * restart interval counts blocks; the padding blocks keep what the interleaved scans gave them.  The arena layout is the baseline one. */
#define SP_JPEG_EBAD_SCAN (-23)    /* Ss / Se / Ah / Al or the component list of a scan is invalid, or does not continue the progression */
#define SP_JPEG_EINCOMPLETE (-24)  /* the progression ends before every component has DC and coefficients 1..9 down to bit 0 */

/* One scan of a progressive file, as sp_jpeg_parse_scans found it. */
typedef struct sp_jpeg_scan {
    int32_t components, comp[3];                      /* 1..3 frame component indices, ascending */
    int32_t ss, se, ah, al;                           /* spectral band (zigzag positions), successive approximation high / low bit */
    int32_t restart_interval;                         /* the DRI value in force at this SOS (it may change between scans) */
    int32_t ecs_offset, ecs_end;                      /* this scan's entropy bytes in the file */
    int32_t seg_index, segments;                      /* this scan's restart segments: seg_index is relative to the file's desc.seg_index */
    int32_t reserved;
    uint8_t huff_counts[3][16];                       /* the tables THIS scan uses, as in force at its SOS: first DC scan: one per scan */
    uint8_t huff_values[3][256];                      /* component; AC scan: [0]; a DC refinement scan uses none (all zero) */
} sp_jpeg_scan;

/* Host only, no GPU call: parse one progressive file.  *desc as sp_jpeg_parse fills it, with segments = the total over all scans,
 * ecs_offset = the first scan's start, ecs_end = the last scan's end, restart_interval = the first scan's, dc_sel / ac_sel and the
 * Huffman fields zero (the tables are per scan).  scans (HOST, may be NULL with scan_capacity 0) receives at most scan_capacity
 * records, *scan_count the number found; seg_offsets (HOST, may be NULL with seg_capacity 0) the first entropy byte of every restart
 * segment of every scan, in file order, at most seg_capacity of them (desc->segments is the number found): call again with larger
 * arrays when a count exceeds its capacity.  Nothing is written past a capacity.  Returns SP_OK or SP_JPEG_E* with the reason and the
 * byte offset in sp_last_error. */
int sp_jpeg_parse_scans(const uint8_t* data, int64_t size, sp_jpeg_desc* desc, sp_jpeg_scan* scans, int32_t scan_capacity,
                        int32_t* scan_count, int32_t* seg_offsets, int32_t seg_capacity);

/* The entropy stage of `count` progressive files: what sp_jpeg_decode_batch(stages = ENTROPY) is for baseline ones.  descs, bytes,
 * seg_offsets, coef, status: as there.  scans_host / scans_dev: scan_total records in HOST and DEVICE memory; scan_range_host /
 * scan_range_dev int32 [count + 1]: file i owns scans [r[i], r[i + 1]), 1..256 of them.  Every host-side range (scan ranges, each
 * scan's entropy bytes inside its file, its segments inside the table, the coefficient region inside the arena) is checked before
 * anything is launched, the device pointers last.  Two launches: one zeroes every file's coefficient region, then
 * jpeg_prog_entropy_kernel, one 64-lane workgroup per file, walks the file's scans in file order: per scan it builds the scan's
 * Huffman tables in LDS, lane s decodes restart segments s, s + 64, ... of the scan, and a workgroup barrier ends the scan (refinement
 * scans read what earlier scans wrote).  status[i]: the SP_JPEG_STATUS_* bits OR-ed over the file's scans (SEGMENTS: a scan whose
 * segment count is not ceil(scan MCUs / interval); the excess is ignored).  A damaged stream ends in a non-zero status, never in an
 * access outside the file's own regions.  Nothing synchronises; count == 0 is a no-op. */
int sp_jpeg_progressive_entropy(const sp_jpeg_desc* descs_host, const sp_jpeg_desc* descs_dev, int count, const sp_jpeg_scan* scans_host,
                                const sp_jpeg_scan* scans_dev, const int32_t* scan_range_host, const int32_t* scan_range_dev,
                                int64_t scan_total, const uint8_t* bytes, int64_t bytes_size, const int32_t* seg_offsets, int64_t seg_count,
                                int16_t* coef, int64_t coef_size, int32_t* status, void* stream);

/* ---- baseline JPEG encoding: uint8 BGR [H,W,3] images in, file bytes out ---------------------------------------------------------------------
 * (No new ABI version: these are additions.)  The file is the one libjpeg-turbo writes with its defaults (what PIL's save and cv2.imwrite
 * give without optimised tables) byte for byte: 16.16 fixed-point BGR -> YCbCr, chroma averaged 2x1 / 2x2 without smoothing, the "islow"
 * integer forward DCT, the Annex K quantisation tables scaled by `quality`, the Annex K Huffman tables, JFIF 1.01 header.  Baseline,
 * three components, one interleaved scan, optional restart markers.  There is no CPU encode path. */
#define SP_JPEG_ENC_HEADER_MAX 640          /* SOI .. SOS of any file this encoder writes is 623 bytes, 629 with a DRI segment */
#define SP_JPEG_ENC_STATUS_OVERFLOW 1       /* the file does not fit out_capacity: nothing of it is written, its length is 0 */

/* sp_jpeg_encode_batch `stages` */
#define SP_JPEG_ENC_STAGE_COEF 1            /* colour, downsampling, forward DCT, quantisation, per-block bit counts */
#define SP_JPEG_ENC_STAGE_SCAN 2            /* prefix sums: the bit offset of every block, the byte offset of every restart segment */
#define SP_JPEG_ENC_STAGE_EMIT 4            /* Huffman codes into the unstuffed stream at those offsets */
#define SP_JPEG_ENC_STAGE_STUFF 8           /* header, FF 00 stuffing, restart markers, EOI; length and status */
#define SP_JPEG_ENC_STAGE_ALL 15

/* bytes of workspace one image needs beyond desc.ws_bytes: they depend on the capacity the caller gives its file */
#define SP_JPEG_ENC_STREAM_WS(cap) ((((int64_t)(cap) / 4096 + 2) * 8 + 63) / 64 * 64 + ((int64_t)(cap) + 127) / 64 * 64)

/* One image.  sp_jpeg_enc_plan fills everything down to hlen; the caller fills the placement fields before sp_jpeg_encode_batch. */
typedef struct sp_jpeg_enc_desc {
    int32_t width, height;
    int32_t subsampling;                              /* 444, 422 or 420 */
    int32_t quality, restart_interval;                /* 1..100; MCUs per restart segment, 0 = no restart markers */
    int32_t h_samp, v_samp;                           /* the luma sampling factors (chroma is 1x1) */
    int32_t mcus_x, mcus_y;                           /* ceil(width / (8 h_samp)), ceil(height / (8 v_samp)) */
    int32_t wb[3], hb[3];                             /* real blocks per row / column of each component: ceil(samples / 8) */
    int32_t blocks_per_mcu;                           /* h_samp * v_samp + 2 */
    int32_t blocks;                                   /* mcus_x * mcus_y * blocks_per_mcu: the scan, dummy blocks included */
    int32_t segments;                                 /* ceil(MCUs / restart_interval), 1 without restart markers */
    int32_t header_bytes;                             /* SOI .. SOS */
    int64_t ws_bytes;                                 /* workspace of this image without its stream part (SP_JPEG_ENC_STREAM_WS) */
    int64_t ws_coef, ws_bits, ws_pos, ws_seg, ws_chunk;   /* where its arrays lie in that region (bytes from ws_offset; see below) */
    uint16_t quant[2][64];                            /* the scaled tables (0 luma, 1 chroma) in zigzag order */
    uint8_t header[SP_JPEG_ENC_HEADER_MAX];           /* the file's first header_bytes bytes */
    uint16_t hcode[4][256];                           /* code of symbol s in table 0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma */
    uint8_t hlen[4][256];                             /* ... and its length in bits (0: the table has no such symbol) */
    /* the caller's part */
    uint64_t src;                                     /* DEVICE address of the image: uint8 [height, width, 3] BGR, contiguous */
    int64_t ws_offset;                                /* in bytes into `workspace`, a multiple of 64 */
    int64_t out_offset;                               /* in bytes into `out` */
    int64_t out_capacity;                             /* bytes the file may take at out_offset */
} sp_jpeg_enc_desc;

/* Host only, no GPU call: plan one image.  1 <= width, height <= 16384 (else SP_JPEG_ESIZE), subsampling 444 / 422 / 420 (else
 * SP_JPEG_ESAMPLING), quality 1..100 and restart_interval 0..65535 (else SP_EINVAL).  Fills the geometry, the scaled tables, the complete
 * header bytes and the workspace layout; the caller's part is zeroed. */
int sp_jpeg_enc_plan(int width, int height, int subsampling, int quality, int restart_interval, sp_jpeg_enc_desc* desc);

/* Encode `count` images of mixed sizes, sampling and quality.  descs_host / descs_dev: the same descriptors in HOST and in DEVICE memory;
 * the host copy is planned again and compared, and its placement checked against workspace_size / out_size, before anything is launched.
 * workspace: DEVICE, 64-byte aligned; image i owns [ws_offset, ws_offset + ws_bytes + SP_JPEG_ENC_STREAM_WS(out_capacity)).  out: DEVICE;
 * image i's file is out + out_offset, length[i] bytes (header, entropy data, EOI).  length, status: int32 [count] DEVICE.  The regions of
 * different images must not overlap (not checked).  The image's workspace, from ws_offset:
 *   +0         uint64 [8]   total bits, unstuffed bytes, FF bytes, refused flag
 *   +ws_coef   int16 [blocks][64]  quantised coefficients in zigzag order, blocks in scan order, DC absolute, dummy blocks zero
 *   +ws_bits   uint16 [blocks]     bits of each block in the stream (at most 22 + 63 * 26)
 *   +ws_pos    uint64 [blocks + 1] exclusive prefix sum of ws_bits
 *   +ws_seg    uint64 [segments + 1]  first byte of each restart segment in the unstuffed stream
 *   +ws_chunk  uint64 []    chunk sums of the two scans above;  +ws_bytes: those of the third, then the unstuffed stream
 * `stages`: SP_JPEG_ENC_STAGE_ALL, or a subset (a bench / test runs them one at a time; later stages read what earlier ones left):
 *   coef   one lane per block: colour, chroma averaging, forward DCT, quantisation, AC bit count; then the DC differences' bits
 *   scan   three launches per prefix sum (256-element chunk sums; one workgroup per image scans the chunk sums; every chunk again, plus
 *          its offset): bits per block -> ws_pos, then bytes per restart segment -> ws_seg.  An image whose unstuffed stream alone
 *          exceeds out_capacity is refused here
 *   emit   zero the stream's words, then one lane per block ORs its codes in at 8 * ws_seg[segment] + ws_pos[block] - ws_pos[segment's
 *          first block]; the last block of a segment pads to the byte with 1-bits
 *   stuff  a third prefix sum, over the FF bytes of the stream in 4096-byte chunks; its last launch writes header, data with FF 00
 *          stuffing, FF D0..D7 between segments and FF D9, each lane 16 stream bytes.  length and status are written by this stage
 * No lane walks more than one block, 16 stream bytes or (the chunk sums) blocks / 65536 entries.  An image that does not fit gets
 * SP_JPEG_ENC_STATUS_OVERFLOW, length 0 and not one byte written to `out`.  Nothing synchronises; count == 0 is a no-op. */
int sp_jpeg_encode_batch(const sp_jpeg_enc_desc* descs_host, const sp_jpeg_enc_desc* descs_dev, int count, void* workspace, int64_t workspace_size,
                         uint8_t* out, int64_t out_size, int32_t* length, int32_t* status, int stages, void* stream);

/* ---- video frames: YUV 4:2:0 (NV12 / I420) <-> packed BGR on the device ------------------------------------------------------------------------
 * (No new ABI version: these are additions.)  What decoders hand out and encoders take: h x w luma samples (1 <= h, w <= 32767, odd sizes
 * legal) and ch x cw chroma samples, ch = (h + 1) / 2, cw = (w + 1) / 2.
 *   SP_YUV_NV12   a Y plane of pitch_y bytes per row and a UV plane of pitch_c bytes per row holding U, V byte pairs (`u` = the UV plane);
 *   SP_YUV_I420   Y, U and V planes; U and V share pitch_c.
 * Pitches are in bytes and may exceed the row (pitch_y >= w; pitch_c >= 2 * cw for NV12, >= cw for I420; pitch_bgr >= 3 * w); neither base
 * pointers nor pitches need any alignment.  The arithmetic is libjpeg's 16.16 fixed point, int32, `>>` arithmetic, clamp8 = clamp to 0..255:
 *   YUV -> BGR, pixel (r, c) with the chroma sample (r >> 1, c >> 1) (replication):  yy = Y - yoff, uu = U - 128, vv = V - 128,
 *       R = clamp8((ay*yy + rv*vv + 32768) >> 16)   G = clamp8((ay*yy - gu*uu - gv*vv + 32768) >> 16)   B = clamp8((ay*yy + bu*uu + 32768) >> 16)
 *   BGR -> YUV, per pixel  Yp = (yr*R + yg*G + yb*B + (yoff << 16) + 32768) >> 16,  Up = (ur*R + ug*G + ub*B + (128 << 16) + 32767) >> 16,
 *       Vp likewise with vr, vg, vb; chroma sample (i, j) = (sum of Up + 2) >> 2 over the pixels (min(2i + a, h - 1), min(2j + b, w - 1)),
 *       a, b in {0, 1} (an edge pixel counts twice at an odd size).  No clamp: Y 0..255 / 16..235, U and V 0..255 / 16..240 (full / limited).
 *   matrix / range    yoff    ay     rv      bu     gu     gv     yr     yg    yb     ur      ug     ub     vr      vg     vb
 *   BT.601 full          0  65536  91881  116130  22554  46802  19595  38470  7471  -11059  -21709  32768  32768  -27439  -5329
 *   BT.601 limited      16  76309 104597  132201  25675  53279  16829  33039  6416   -9714  -19071  28784  28784  -24103  -4681
 *   BT.709 full          0  65536 103206  121609  12276  30679  13933  46871  4732   -7509  -25259  32768  32768  -29763  -3005
 *   BT.709 limited      16  76309 117489  138438  13975  34925  11966  40254  4064   -6596  -22189  28784  28784  -26145  -2639
 * (round(c * 65536) of the ITU definitions; BT.601 full range keeps libjpeg's table, so it equals the JPEG decoder's and encoder's colour
 * functions bit for bit.)  Every channel is within 1 level of the float64 definition rounded half up.
 * Each call is ONE launch and nothing synchronises.  A thread owns 2-row x 16-column patches, so chroma is read (or averaged) once and no
 * thread needs another's pixels; only bytes inside [row * pitch, row * pitch + row bytes) are written, pitch padding stays untouched.
 * A frame whose plane pointers, BGR pointer and three pitches are ALL multiples of 16 takes 16-byte accesses on its full patches
 * (sp_yuv420_wide_path says so); its tail columns, the last row of an odd height, and every other frame go byte by byte: same bits. */
#define SP_YUV_NV12 0
#define SP_YUV_I420 1
#define SP_YUV_BT601 0
#define SP_YUV_BT709 1
#define SP_YUV_LIMITED 0
#define SP_YUV_FULL 1
typedef struct sp_yuv_ref {                 /* one frame; read from DEVICE memory by the _images entry points */
    unsigned char *y, *u, *v;               /* device pointers; NV12: u = the UV plane, v unused */
    unsigned char* bgr;                     /* [h, w, 3], pitch_bgr bytes per row */
    int32_t h, w, pitch_y, pitch_c, pitch_bgr;
    int32_t format, matrix, range;
} sp_yuv_ref;                               /* 64 bytes */
/* One frame, planes -> bgr.  Checked on the host (SP_EINVAL and a message, nothing launched): sizes, pitches below the row, the format /
 * matrix / range codes, NULL planes (v may be NULL for NV12), and bgr overlapping a plane. */
int sp_yuv420_to_bgr_u8c3(const unsigned char* y, const unsigned char* u, const unsigned char* v, int h, int w, int pitch_y, int pitch_c,
                          int format, int matrix, int range, unsigned char* bgr, int pitch_bgr, void* stream);
/* One frame, bgr -> planes; the same checks, with the planes as the outputs (they must not overlap bgr or each other). */
int sp_bgr_to_yuv420_u8c3(const unsigned char* bgr, int pitch_bgr, int h, int w, int format, int matrix, int range, unsigned char* y,
                          unsigned char* u, unsigned char* v, int pitch_y, int pitch_c, void* stream);
/* `count` frames of any sizes, formats and modes in one launch (count <= 65535; count == 0 launches nothing): frame i as frames_dev[i]
 * describes it, with the bits of the single-frame call on that frame (the same device functions).  max_h, max_w (1 .. 32767): bounds of the
 * frames' sizes, which size the grid.  The table's contents cannot be checked on the host: the caller guarantees valid pointers and what
 * the single-frame calls check; a frame whose sizes, pitches or codes those calls would refuse, or with a NULL plane, is skipped. */
int sp_yuv420_to_bgr_images_u8c3(const sp_yuv_ref* frames_dev, int count, int max_h, int max_w, void* stream);
int sp_bgr_to_yuv420_images_u8c3(const sp_yuv_ref* frames_dev, int count, int max_h, int max_w, void* stream);
/* 1 when a frame with these pointers and pitches takes the 16-byte path on its full patches, 0 when it goes byte by byte (the predicate
 * the kernels evaluate; v is not looked at for NV12).  Launches nothing. */
int sp_yuv420_wide_path(const void* y, const void* u, const void* v, const void* bgr, int pitch_y, int pitch_c, int pitch_bgr, int format);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLE_POSE_HIP_H */
