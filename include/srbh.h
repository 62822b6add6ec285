/*
 * srbh.h -- C ABI of libsrbh (MI355X / gfx950 native kernels for the SR building-height hot path).
 *
 * The reference (lauraset/Super-resolution-building-height-estimation) has NO native/FFI
 * interface: its boundary for this path is Python nn.Module duck typing + state_dict keys
 * (SURVEY.md 8b).  This header is therefore the build-defined C boundary that the Python mirror
 * modules (`super-resolution-building-height-estimation_amd/ *.py`) bind with ctypes; each entry
 * point names the reference call it stands in for (paths relative to /root/reference).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless stated;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - every function returns 0 on success, a negative srbh error or a positive hipError_t;
 *     srbh_last_error() returns a thread-local message for the last failure;
 *   - the library allocates nothing persistent: weights/workspaces are caller-owned buffers.
 *
 * Device data layouts (see DESIGN.md "Data layout in HBM")
 *   ACT16  : fp16 activations, chunk-planar, zero-bordered:  [B][C/32][H+2][W+2][32]
 *            (one 64-byte record per pixel per 32-channel chunk; the 1-pixel border is kept zero
 *             by construction so a 3x3 conv never bounds-checks)
 *   RES32  : fp32 residual stream, [B][H][W][64]
 *   NHWC32 : fp32 output, [B][H][W][C]  (== a torch channels_last (B,C,H,W) tensor)
 *   WPACK16: fp16 weights in MFMA A-fragment order: [Cin/32][tap 9][kstep 2][Cout/32][lane 64][8]
 */
#ifndef SRBH_H
#define SRBH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRBH_OK 0
#define SRBH_ERR_ARG (-1)        /* bad argument / unsupported shape (reference: assert / NotImplementedError) */
#define SRBH_ERR_WORKSPACE (-2)  /* workspace too small */

/* ---- library ------------------------------------------------------------------------------ */
int srbh_version(void);
const char* srbh_last_error(void);
/* Diagnostics: which form of the head entry points ran since the last reset (SURVEY 8b "no silent fallback": the choice between a
 * specialised persistent kernel and the general template, or one fused pass and two launches, depends on shapes / element types and is
 * invisible in the results).  out[i] for i < n in the order below; returns the number of counters. */
#define SRBH_PATH_HCONV16 0             /* srbh_hconv_h16 -> persistent 16 -> 16 3x3 kernel */
#define SRBH_PATH_HCONV_TEMPLATE 1      /* srbh_hconv_f32 / _h16 -> one-tile-per-workgroup template */
#define SRBH_PATH_ENTRY_FUSED 2         /* srbh_hconv_entry_h16 -> one pass */
#define SRBH_PATH_ENTRY_SPLIT 3         /* ... -> two template launches */
#define SRBH_PATH_WGRAD16 4             /* srbh_hconv_wgrad_b16 -> persistent 16 -> 16 kernel */
#define SRBH_PATH_WGRAD_B16_GENERIC 5
#define SRBH_PATH_WGRAD_F32 6
#define SRBH_PATH_WGRAD_ENTRY_FUSED 7   /* srbh_hconv_wgrad_entry_b16 -> one pass */
#define SRBH_PATH_WGRAD_ENTRY_SPLIT 8
#define SRBH_PATH_HCONV_UP 9             /* srbh_hconv_h16, pixelshuffle2 == 2 -> persistent Upsampler 16 -> 64 kernel */
#define SRBH_PATH_HBLOCK16 11            /* srbh_hblock16_eval: a plain BasicBlock of the inference head in one pass */
#define SRBH_PATH_HBWD16 10              /* srbh_hbwd16: BatchNorm apply + weight gradient + data gradient of a 16 -> 16 conv in one pass */
int srbh_path_counters(unsigned long long* out, int n, int reset);
/* Read-only: the workgroup cap in effect for the persistent tile walk of the kernel behind `path` (SRBH_PATH_HCONV16, _ENTRY_FUSED, _WGRAD16,
 * _HCONV_UP, _HBWD16, _HBLOCK16; the SRBH_*_WGS environment knobs, read once per process).  A walk over ntiles = B * (H/4) * (W/64) tiles
 * gives each of the 8 XCDs a contiguous run of tiles_per_xcd = ceil(ntiles / 8) and launches min(tiles_per_xcd, cap / 8) workgroups per XCD;
 * workgroup j of an XCD takes tiles j, j + that count, ... of its run.  SRBH_PATH_ENTRY_FUSED reports the chunked entry kernel's cap; the
 * whole-row form of the 64-channel fp16 source always runs 32 workgroups per XCD.  Returns -1 for a path without such a walk. */
int srbh_head_wgs_cap(int path);

/* ---- layout helpers (used by tests and by the Python mirror at module boundaries) ------------ */
/* bytes of an ACT16 buffer including the read slack the tiled kernels need */
size_t srbh_act16_bytes(int B, int C, int H, int W);
/* NCHW fp32 -> ACT16 (interior only; border must already be zero). C is padded up to a multiple of 32. */
int srbh_nchw32_to_act16(const float* src, void* dst, int B, int C, int H, int W, void* stream);
/* ACT16 -> NCHW fp32 (first C channels) */
int srbh_act16_to_nchw32(const void* src, float* dst, int B, int C, int H, int W, void* stream);

/* ---- weights ------------------------------------------------------------------------------ */
/* bytes of a WPACK16 image of an OIHW 3x3 weight (Cin, Cout padded up to multiples of 32) */
size_t srbh_wpack16_bytes(int cout, int cin);
/* OIHW fp32 [cout][cin][3][3] -> WPACK16.  Stands in for nn.Conv2d's weight tensor
 * (SR/rrdbnet_arch.py:125-129,197-204): same values, rounded to fp16, re-ordered once. */
int srbh_pack_conv3x3_f16(const float* w_oihw, int cout, int cin, void* packed, void* stream);

/* ---- generic fused 3x3 convolution (the hot kernel) ----------------------------------------
 * y = conv3x3(in, w) + bias, stride 1, zero pad 1  (nn.Conv2d(...,3,1,1): SR/rrdbnet_arch.py:125-129)
 * with the reference's surrounding elementwise ops fused into the epilogue:
 *   upsample2x : the input is read through F.interpolate(scale_factor=2, mode='nearest')
 *                (SR/rrdbnet_arch.py:236-237): in[y>>1][x>>1]; H,W below are the OUTPUT size
 *   res_scale  : y *= res_scale (0.2 of SR/rrdbnet_arch.py:143) before adding residuals
 *   res1       : y += res1 (RES32), then res1 := y when res1_update   (x5*0.2 + x, :143)
 *   res2       : y = y*res2_scale + res2 (RES32), res2 := y when res2_update (out*0.2 + x, :167)
 *   skip       : y += skip (RES32, read only)                    (feat + body_feat, :234)
 *   lrelu      : LeakyReLU(0.2)                                  (:131,206)
 *   out16      : store fp16 into chunks [out16_chunk0, +Cout/32) of an ACT16 buffer
 *   out32      : store fp32 NHWC with out32_c channels (only the first out32_c of Cout are stored)
 */
typedef struct srbh_conv3x3_args {
    const void* in;         /* ACT16, C_in = 32*in_chunks channels starting at chunk in_chunk0 */
    int in_chunks_total;    /* chunk planes per image in the `in` buffer */
    int in_chunk0;
    int in_chunks;          /* K = in_chunks*32*9 */
    const void* w;          /* WPACK16 for (cout, 32*in_chunks) */
    const float* bias;      /* [cout] fp32 or NULL */
    int cout;               /* 32 or 64 */
    int B, H, W;            /* output geometry (input is H/2 x W/2 when upsample2x) */
    int upsample2x;
    int lrelu;
    float res_scale;        /* multiplies (conv+bias) when res1 is given; ignored otherwise */
    float* res1;
    int res1_update;
    float res2_scale;
    float* res2;
    int res2_update;
    const float* skip;
    void* out16;            /* ACT16 or NULL */
    int out16_chunks_total;
    int out16_chunk0;
    float* out32;           /* NHWC32 or NULL */
    int out32_c;
    int out16_nhwc;         /* 1: `out16` is a dense fp16 NHWC tensor [B][H][W][32*out16_chunks_total] (no border), this conv's channels
                             * at chunk out16_chunk0 -- the hand-off format of the head's 16-bit kernels (SRBH_IO_SRC0_H16).  64 -> 64
                             * convs without residual epilogue only (the persistent tail kernel); anything else is an error */
} srbh_conv3x3_args;

int srbh_conv3x3_f16(const srbh_conv3x3_args* a, void* stream);

/* The same convolution on SPLIT fp16 operands (the "f16x2" precision mode of the up-sampler tail, SR/rrdbnet_arch.py:234-239's conv_body /
 * conv_up1 / conv_up2 / conv_hr): every fp32 value v is carried as hi = rne16(v) and lo' = rne16((v - hi) * 2^11), both fp16, weights
 * (srbh_pack_conv3x3_f16lo) and activations alike, and the conv is
 *     C = sum (w_hi * a_lo' + w_lo' * a_hi)     M = sum w_hi * a_hi     y = M + C * 2^-11 + bias      (fp32 accumulators, lo x lo dropped)
 * followed by `skip` and `lrelu` as above.  `a` describes the hi operands (a->in / a->w) and the outputs, `s` the lo' ones.  64 -> 64
 * channels (in_chunks == 2, cout == 64), no res1 / res2.  Outputs: out32 (fp32 NHWC, 64 channels); out16 as ACT16 planes = the hi planes of y
 * with its lo' planes in s->out16_lo (required then); out16 with out16_nhwc = rne16(y) as a dense fp16 NHWC tensor (no lo'). */
typedef struct srbh_conv3x3_split {
    const void* in_lo;          /* ACT16 buffer holding the lo' planes of the input, 2 planes from in_lo_chunk0 */
    int in_lo_chunks_total;
    int in_lo_chunk0;
    const void* w_lo;           /* WPACK16 of the weights' lo' parts */
    void* out16_lo;             /* ACT16 buffer for the lo' planes of the output, or NULL */
    int out16_lo_chunks_total;
    int out16_lo_chunk0;
} srbh_conv3x3_split;
int srbh_conv3x3_f16x2(const srbh_conv3x3_args* a, const srbh_conv3x3_split* s, void* stream);
/* OIHW fp32 -> WPACK16 of the lo' parts: rne16((w - rne16(w)) * 2^11) (the hi parts are srbh_pack_conv3x3_f16's pack) */
int srbh_pack_conv3x3_f16lo(const float* w_oihw, int cout, int cin, void* packed, void* stream);
/* lo' planes of an fp32 tensor whose hi planes exist: lo' = rne16((v - hi) * 2^11) for the 64 channels of v, hi read from planes
 * hi_chunk0.. of `hi`, written to planes lo_chunk0.. of `lo` (interior only; borders must be zero already).  v: NHWC fp32 (B,H,W,64), or
 * (fragment_order != 0, W == 64) the persistent trunk kernel's order of its output stream (see srbh_rrdbnet_trunk_out). */
int srbh_act16_split_lo(const float* v, int fragment_order, const void* hi, int hi_chunks_total, int hi_chunk0, void* lo, int lo_chunks_total,
                        int lo_chunk0, int B, int H, int W, void* stream);
/* The same convolution for the GRADIENT side of the RRDBNet training path (reference SR/rrdbnet_arch.py:538-592 differentiates the
 * generator; round 3, SURVEY 8f-4 second slice).  bf16 != 0: the ACT16 input / output planes and the WPACK16 weights hold bf16
 * (srbh_pack_conv3x3_b16; gradients need fp32's exponent range), products on v_mfma_f32_32x32x16_bf16.  mask16 != NULL: the output is
 * multiplied by the LeakyReLU derivative taken from the SAVED fp16 activation plane(s) -- chunks mask_chunk0.. of an ACT16 buffer with
 * mask_chunks_total planes: post-activation > 0 ? 1 : 0.2 (torch's leaky_relu backward) -- before the 16-bit / fp32 stores.  No
 * nearest-x2 read in these forms.  bf16 == 2: bf16 input planes and weights as bf16 == 1, but the 16-bit OUTPUT planes are rounded to
 * fp16 (RNE) -- the last conv5 of the bf16 inference trunk (srbh_rrdbnet_desc.rdb_b16), whose planes leave for conv_body's fp16 operands.
 * Any other nonzero value means 1.  All 16-bit roundings are round-to-nearest-even; out32 (if also requested) holds the unrounded fp32 values. */
int srbh_conv3x3_x16(const srbh_conv3x3_args* a, int bf16, const void* mask16, int mask_chunks_total, int mask_chunk0, void* stream);
int srbh_pack_conv3x3_b16(const float* w_oihw, int cout, int cin, void* packed, void* stream);
/* the same packs (SR/rrdbnet_arch.py:136-167's conv weights as WPACK16) for MANY convs in ONE launch: table_dev = n descriptors in DEVICE memory;
 * bias_dst != NULL also copies the conv's cout bias values (the padded bias table of srbh_rrdbnet_desc); max_elems = the largest
 * srbh_wpack16_bytes(cout, cin) / 2 among them.  (A generator in training repacks every conv each iteration: 351 + 345 launches otherwise.) */
typedef struct srbh_pack3x3_desc {
    const float* w;          /* OIHW fp32 [cout][cin][3][3] */
    void* packed;
    const float* bias_src;   /* or NULL */
    float* bias_dst;         /* or NULL */
    int cout, cin, bf16, pad_;  /* bf16: 0 = fp16 pack, 1 = bf16 pack, 2 = fp16 pack of the lo' parts (srbh_pack_conv3x3_f16lo) */
} srbh_pack3x3_desc;
int srbh_pack_conv3x3_many(const srbh_pack3x3_desc* table_dev, int n, long max_elems, void* stream);
/* NHWC fp32 [B][H][W][C] (C % 32 == 0) * scale -> chunk planes chunk0.. of an ACT16 buffer with chunks_total planes, as fp16 or bf16 */
int srbh_nhwc32_to_act16(const float* src, void* dst, int B, int C, int H, int W, int chunks_total, int chunk0, float scale, int bf16,
                         void* stream);
/* out[nchunk*32] = per-channel sums over (B,H,W) of nchunk ACT16 planes starting at chunk0 (bias gradients); fp16 or bf16 elements */
int srbh_act16_channel_sum(const void* src, int B, int H, int W, int chunks_total, int chunk0, int nchunk, int bf16, float* out,
                           void* stream);
/* weight gradient of a 3x3 conv on ACT16 tensors: x fp16 planes (channels 0..cin-1), dy bf16 planes (channels dy_ch0..+cout);
 * cin, cout, dy_ch0 multiples of 16, cout <= 64; dw OIHW fp32; ws = srbh_hwgrad_ws_bytes(cout, cin, 3) bytes (declared below) */
int srbh_act16_wgrad_b16(const void* x, int x_chunks_total, int cin, const void* dy, int dy_chunks_total, int dy_ch0, int cout,
                         int B, int H, int W, float* dw, float* ws, void* stream);
/* dst = a * x + b * y on fp32 vectors (y may be NULL; dst may alias x or y); n % 4 == 0 */
int srbh_axpby_f32(float* dst, float a, const float* x, float b, const float* y, long n, void* stream);
/* g *= (y > 0 ? 1 : slope), in place: the backward of F.leaky_relu (SR/rrdbnet_arch.py:234-239's activations) from the saved OUTPUT y; n % 4 == 0 */
int srbh_lrelu_bwd_f32(float* g, const float* y, float slope, long n, void* stream);
/* the adjoint of F.interpolate(scale_factor=2, mode='nearest') (SR/rrdbnet_arch.py:236-237) on an NHWC fp32 tensor: g [B][2Ho][2Wo][C] -> out [B][Ho][Wo][C],
 * the sum of each 2 x 2 block ((a + b) + (c + d)); C % 4 == 0 */
int srbh_up2_bwd_nhwc_f32(const float* g, float* out, int B, int Ho, int Wo, int C, void* stream);
/* F.interpolate(scale_factor=2, mode="bilinear", align_corners=False) on an NHWC fp32 tensor (UNetDiscriminatorSN, SR/rrdbnet_arch.py:285-297):
 * backward == 0: x [B][H][W][C] -> out [B][2H][2W][C]; backward != 0: x = the gradient [B][2H][2W][C] -> out = its adjoint [B][H][W][C] (a gather:
 * no atomics, fixed summation order).  C % 4 == 0. */
int srbh_bilinear2x_nhwc_f32(const float* x, float* out, int B, int H, int W, int C, int backward, void* stream);

/* conv_first (SR/rrdbnet_arch.py:197,232): 3x3 conv on the NCHW fp32 network input with few input
 * channels (3, 12 or 48), computed in fp32 on the vector ALUs.  Writes the 64-channel result to up to
 * three RES32 buffers (feat, rdb residual, rrdb residual) and as fp16 to chunks 0..1 of `out16`. */
int srbh_conv_first_f32(const float* x_nchw, const float* w_oihw, const float* bias, int B, int cin, int H, int W,
                        float* res_a, float* res_b, float* res_c, void* out16, int out16_chunks_total, void* stream);

/* ---- whole network: RRDBNet.forward_feature / forward (SR/rrdbnet_arch.py:208-240) -------------- */
typedef struct srbh_conv_w {
    const void* w;      /* WPACK16 */
    const float* bias;  /* fp32 [cout] */
} srbh_conv_w;

typedef struct srbh_rrdbnet_desc {
    int num_in_ch;              /* channels of x as seen by conv_first (after pixel_unshuffle) */
    int num_block;              /* RRDB blocks (23) */
    const float* conv_first_w;  /* OIHW fp32, used by srbh_conv_first_f32 */
    const float* conv_first_b;
    const srbh_conv_w* rdb;     /* [num_block*3*5] in body.{i}.rdb{r}.conv{k} order */
    srbh_conv_w conv_body, conv_up1, conv_up2, conv_hr;
    srbh_conv_w conv_last;      /* cout padded to 32; only used when want_forward */
    int num_out_ch;
    const srbh_conv_w* rdb_b16; /* NULL, or the same [num_block*3*5] convs as bf16 packs (srbh_pack_conv3x3_b16; bias pointers as in `rdb`):
                                 * srbh_rrdbnet_forward then runs the dense blocks on bf16 operands -- bf16 planes, v_mfma_f32_32x32x16_bf16,
                                 * fp32 RRDB streams as before, the trunk's output planes rounded to fp16 for conv_body, which with the
                                 * up-sampler tail keeps its fp16 operands.  Environment SRBH_TRUNK_BF16=0 restores the fp16 trunk (A/B).
                                 * The training entry points below always use `rdb`. */
    int tail_f16x2;             /* 0: the tail convs run on fp16 operands (everything above).  1: the "f16x2" mode -- conv_body, conv_up1,
                                 * conv_up2 and conv_hr on split fp16 operands (srbh_conv3x3_f16x2), conv_body's lo' planes taken from the
                                 * trunk's fp32 output stream; needs the lo' packs below and a workspace of
                                 * srbh_rrdbnet_workspace_bytes_f16x2(); want_forward 0 and 2 only.  The trunk is untouched. */
    const void* conv_body_lo;   /* srbh_pack_conv3x3_f16lo packs of the tail convs (biases as above); NULL unless tail_f16x2 */
    const void* conv_up1_lo;
    const void* conv_up2_lo;
    const void* conv_hr_lo;
} srbh_rrdbnet_desc;

size_t srbh_rrdbnet_workspace_bytes(int B, int H, int W, int want_forward);
/* the workspace of the f16x2 mode (srbh_rrdbnet_desc.tail_f16x2): the layout above with the lo' planes of the up-sampled activations behind
 * it, so srbh_rrdbnet_last_status / srbh_rrdbnet_trunk_out work on it unchanged and a forward in the default mode may use it too */
size_t srbh_rrdbnet_workspace_bytes_f16x2(int B, int H, int W, int want_forward);
/* x: NCHW fp32 (B,num_in_ch,H,W).  out: NHWC32 (B,4H,4W,64) for forward_feature (want_forward=0,
 * no activation after conv_hr -- SR/rrdbnet_arch.py:238) or (B,4H,4W,num_out_ch) for forward
 * (want_forward=1, lrelu(conv_hr) then conv_last -- :221-222).  want_forward=2: forward_feature with `out` a dense fp16 NHWC
 * tensor (B,4H,4W,64) -- the same values rounded once (RNE) in conv_hr's epilogue: what the head's fp16-operand kernels would make
 * of the fp32 tensor while staging it, so the height maps of the fp16 head mode are bit-identical and conv_hr writes / the block
 * entry reads half the bytes (harness paths only; the nn.Module API returns fp32).
 * ws: srbh_rrdbnet_workspace_bytes() bytes that were ZERO when first handed to this (B,H,W) geometry
 * (the kernels never write the zero borders, so the same workspace can be reused across calls). */
int srbh_rrdbnet_forward(const srbh_rrdbnet_desc* d, const float* x, float* out, int B, int H, int W,
                         int want_forward, void* ws, size_t ws_bytes, void* stream);


/* Training path of the 3 * num_block dense blocks (SR/rrdbnet_arch.py:538-592 differentiates the generator), the launch
 * loops of rrdbnet_autograd.py's "fast" mode on the device side of the C ABI.
 * forward: xr and xrr hold (copies of) conv_first's output (B,H,W,64) fp32 on entry and the trunk output on return; dense_all = 3 *
 * num_block + 1 zero-bordered ACT16 buffers of 6 planes, dense_stride bytes apart: buffer i keeps [x | x1 | x2 | x3 | x4] of RDB i.
 * backward: g_a = gradient of the trunk output on entry, g_b / g_c scratch of the same size, *g_out = which of the three holds the
 * gradient of the trunk input; packs = per RDB the five bf16 gradient-conv packs (srbh_pack_conv3x3_b16 of the stacked transposed +
 * flipped weight slices, at pack_off[0..4] inside a pack_stride-byte record); G = zero-bordered 6-plane ACT16 buffer(s) for the bf16
 * gradients [g5 | g4 | g3 | g2 | g1]: g_stride > 0 = two of them, g_stride bytes apart -- the weight / bias gradients of an RDB then
 * run on an internal side stream next to the gradient convs of the RDB below (joined before the call returns control of `stream`); dw_all = per RDB 239 616 floats (conv1..conv5, OIHW each), db_all = per RDB 192 floats in G's
 * channel order; wgrad_ws = srbh_rrdbnet_trunk_wgrad_ws_bytes() bytes. */
int srbh_rrdbnet_trunk_train_forward(const srbh_rrdbnet_desc* d, float* xr, float* xrr, void* dense_all, size_t dense_stride, int B, int H,
                                     int W, void* stream);
/* the same forward as ONE launch of the persistent trunk kernel (SR/rrdbnet_arch.py:136-167 x 69, as the inference trunk runs it) over a row
 * of dense buffers, every plane stored whole for the backward, the fp32 output in xr (pixel order); bit-identical to the per-layer call.
 * aux = srbh_rrdbnet_trunk_train_aux_bytes(B, H, W) bytes of scratch (0: geometry not taken); *used = 0: nothing ran, use the call above. */
size_t srbh_rrdbnet_trunk_train_aux_bytes(int B, int H, int W);
int srbh_rrdbnet_trunk_train_forward_persistent(const srbh_rrdbnet_desc* d, float* xr, float* xrr, void* dense_all, size_t dense_stride, int B, int H,
                                                int W, void* aux, void* stream, int* used);
size_t srbh_rrdbnet_trunk_wgrad_ws_bytes(void);   /* size of wgrad_ws below: the five weight-gradient workspaces of a dense block side by side (their reduces run as one pair of launches) */
int srbh_rrdbnet_trunk_train_backward(int num_block, const void* dense_all, size_t dense_stride, const void* packs, size_t pack_stride,
                                      const size_t* pack_off, float* g_a, float* g_b, float* g_c, float** g_out, void* G, size_t g_stride,
                                      float* dw_all, float* db_all, float* wgrad_ws, int B, int H, int W, void* stream);
/* the same backward (SR/rrdbnet_arch.py:538-592's l_g_total.backward() through the 69 dense blocks, SR/rrdbnet_arch.py:136-167) with the 345
 * data-gradient convs as ONE launch of the persistent trunk kernel's bf16 form: G_all = a ROW of num_block * 3 + 1 zero-bordered gradient buffers
 * g_stride bytes apart (buffer k = the k-th RDB from the end), the saved forward planes as LeakyReLU masks; the weight / bias gradients follow on
 * two streams (wgrad_ws = TWO workspaces of srbh_rrdbnet_trunk_wgrad_ws_bytes()) or, given trunk_wgrad_ws, as one launch (srbh_trunk_wgrad).  zero_bias = 64 zero floats; aux = the persistent forward's
 * scratch.  g_a is only read; *g_out is g_b or g_c.  Same operands and per-conv summation order as the call above, the fp32 streams agree with it
 * to the last bits.  *used = 0: nothing ran, use the call above. */
int srbh_rrdbnet_trunk_train_backward_persistent(int num_block, const void* dense_all, size_t dense_stride, const void* packs, size_t pack_stride,
                                                 const size_t* pack_off, const float* zero_bias, const float* g_a, float* g_b, float* g_c,
                                                 float** g_out, void* G_all, size_t g_stride, float* dw_all, float* db_all, float* wgrad_ws,
                                                 void* trunk_wgrad_ws, int B, int H, int W, void* aux, void* stream, int* used);
/* Weight and bias gradients of ALL dense blocks in one launch + one reduce (the gradients of SR/rrdbnet_arch.py:136-167's five convs w.r.t. their
 * parameters, for every RDB): dense_all = the forward's row of saved buffers (fp16 planes), G_all = the backward's row of gradient buffers (bf16
 * planes, buffer k = the k-th RDB from the end), dw_all / db_all as srbh_rrdbnet_trunk_train_backward; ws = srbh_trunk_wgrad_ws_bytes() bytes
 * (0: geometry not taken -- 64-pixel-wide images, H % 8 == 0).  bf16 operands (the saved planes rounded RNE while staged), fp32 accumulation,
 * fixed summation order.  trunk_wgrad_ws above = this workspace (NULL there = the general kernel, RDB by RDB). */
size_t srbh_trunk_wgrad_ws_bytes(int num_block, int B, int H, int W);
int srbh_trunk_wgrad(int num_block, const void* dense_all, size_t dense_stride, const void* G_all, size_t g_stride, int B, int H, int W, float* dw_all,
                     float* db_all, void* ws, void* stream);

/* Synchronises `stream` and returns 0 if the last srbh_rrdbnet_forward on this workspace completed normally, or a
 * negative code if the persistent trunk kernel gave up waiting for a neighbour workgroup (its spins are bounded so a
 * scheduling problem shows up as an error here instead of a hung GPU).  Set SRBH_PERSISTENT=0 to force per-layer launches (the same bits),
 * SRBH_TRUNK_BF16=0 to run the dense blocks on fp16 instead of bf16 operands (see srbh_rrdbnet_desc.rdb_b16). */
int srbh_rrdbnet_last_status(const void* ws, int B, int H, int W, int want_forward, void* stream);

/* Test / diagnosis accessor: the trunk's fp32 output (the RRDB-level residual stream behind the last RRDB, SR/rrdbnet_arch.py:167 x num_block --
 * what conv_body reads, before its rounding to fp16) of the LAST srbh_rrdbnet_forward on this workspace, copied to `out` as NHWC32
 * (B,H,W,64).  The up-sampler tail never writes that stream, so it survives the forward; the two launch forms keep it in different element
 * orders, and this call undoes the one the forward used: call it with the geometry, num_block and environment (SRBH_PERSISTENT) of that
 * forward.  `ws` is only read.  The error within the trunk is damped 25 x per RRDB on this stream and not yet hidden under the fp16
 * roundings of the tail: tests/test_gpu_trunk_parity.py compares it with a rounding-exact CPU emulation. */
int srbh_rrdbnet_trunk_out(const void* ws, size_t ws_bytes, int num_block, int B, int H, int W, int want_forward, float* out, void* stream);

/* Workgroups per launch of the persistent tail convs (conv_up1 / conv_up2 / conv_hr, SR/rrdbnet_arch.py:234-239) issued by the calling host
 * thread: 0 = one per CU (default), n = at most n.  Each workgroup holds a CU's whole LDS for its walk; a caller that runs the feature
 * extractor BESIDE other work (harness.TrainStep's prefetch stream) leaves CUs free with this.  Returns the previous value. */
int srbh_ptail_wgs_cap(int cap);

/* Which form of the persistent tail conv kernel the launches of the calling host thread took (same results, different speed -- counted like
 * srbh_path_counters, so a hot conv sliding back to the general form shows as a count).  counts[0]: the general form (ragged H / W, both
 * outputs at once); counts[1 + 4 * upsample2x + 2 * lrelu + k]: the full-tile form (H % 8 == 0 && W % 64 == 0) of that conv with only a 16-bit
 * output (k = 0: ACT16 planes or NHWC16) or only the fp32 NHWC output (k = 1).  Copies min(n, SRBH_PTAIL_FORMS) counters (counts may be NULL),
 * clears all of them when reset != 0, returns SRBH_PTAIL_FORMS. */
#define SRBH_PTAIL_FORMS 9
int srbh_ptail_form_counts(int* counts, int n, int reset);

/* Measurement hook used by bench.py: when on, srbh_rrdbnet_forward() brackets the persistent trunk kernel (the dominant
 * kernel: the 345 dense-block convs, reference SR/rrdbnet_arch.py:136-167) with HIP events on `stream`;
 * srbh_trunk_last_ms() synchronises on the closing event and returns that launch's duration in milliseconds. */
int srbh_trunk_timing(int on);
int srbh_trunk_last_ms(float* ms);
/* Name of the device kernel the last persistent-trunk launch of this process used ("none" before the first one):
 * lets bench.py label its roofline with the kernel that actually ran (it is what rocprofv3 lists). */
const char* srbh_trunk_kernel_name(void);

/* ==== head: HR feature / fusion / regression modules (SR/HRfuse.py), fp32 ==========================
 * Tensors are NHWC fp32 ([B][H][W][C]; a torch channels_last (B,C,H,W) tensor has exactly this memory).
 * HWPACK32: fp32 weights in v_mfma_f32_16x16x4_f32 A-fragment order [Cin/16][tap][4][Cout/16][lane 64]. */
size_t srbh_hpack_bytes(int cout, int cin, int ksize);
/* OIHW fp32 -> HWPACK32 (nn.Conv2d weight of conv3x3/conv1x1/default_conv, SR/HRfuse.py:11-14,95-109).
 * transpose_flip=1 packs the weight of the data-gradient convolution instead (cout/cin are then the
 * LOGICAL counts of that gradient conv: cout = original in_channels, cin = original out_channels). */
int srbh_hpack_conv_f32(const float* w_oihw, int cout, int cin, int ksize, int transpose_flip, float* packed, void* stream);

/* bytes of the per-channel sum / sum-of-squares partial buffer written by srbh_hconv_f32 (C = cout padded to 16) */
size_t srbh_bn_stats_bytes(int C);
/* 1 when srbh_hconv_h16 takes pixelshuffle2 == 2 at this input size (W % 64 == 0, H % 4 == 0) */
int srbh_hconv_up_supported(int H, int W);

/* y = conv_{ksize}(cat(pre(src0), src1)) + bias, stride 1, zero padding ksize/2
 *   pre(x) = relu?(x*pre_scale[c] + pre_shift[c])  -- BatchNorm(+ReLU) of the producer folded into this consumer
 *            (SR/HRfuse.py:146-148); pre_scale NULL = identity
 *   src1   : optional second source, concatenated after src0's channels (torch.cat, SR/HRfuse.py:187)
 *   pixelshuffle2: store through nn.PixelShuffle(2) (SR/HRfuse.py:23): out is [B][2H][2W][cout/4]
 *   stats  : if non-NULL (srbh_bn_stats_bytes), receives per-channel partial sums of y and y^2 over all
 *            B*H*W pixels (training-mode BatchNorm statistics); it is zeroed by this call */
typedef struct srbh_hconv_args {
    const float* src0; int c0;
    const float* pre_scale; const float* pre_shift; int pre_relu;
    const float* src1; int c1;
    const float* w;       /* HWPACK32 for (cout, c0+c1, ksize) */
    const float* bias;    /* [cout padded to 16] or NULL */
    int cout;             /* 1..32 or 49..64 */
    int ksize;            /* 3 or 1 */
    int B, H, W;
    int pixelshuffle2;    /* 1: PixelShuffle(2) store (SR/HRfuse.py:23), out = (B, cout/4, 2H, 2W) NHWC.  2 (srbh_hconv_h16, fp16 operands, 16 -> 64, 3x3, no
                           * pre / post ops, srbh_hconv_up_supported(H, W)): the same, with `w` / `bias` packed SUB-PIXEL-MAJOR -- row ob*16 + kk*4 + q of the
                           * pack (srbh_hpack_conv_h16 of the permuted weight) holds conv channel (kk*4 + ob)*4 + q -- for the persistent Upsampler kernel */
    float* out;
    double* stats;
    /* optional extensions (0 / NULL = off), used by the strict fp32 trunk: strided views into wider NHWC buffers,
     * LeakyReLU(0.2) and the two residual forms y*s1 + res1, (..)*s2 + res2 (SR/rrdbnet_arch.py:143,167) */
    int src0_ld, src1_ld;      /* floats between consecutive pixels of src0 / src1 (default c0 / c1) */
    int out_ld, out_coff;      /* pixel stride and first channel of the output view (default cout, 0) */
    int post_lrelu;
    const float* res1; int res1_ld; float res1_scale;
    const float* res2; int res2_ld; float res2_scale;
    /* inference-mode BasicBlock fusion (SR/HRfuse.py:146-157 with BatchNorm in eval mode): per-output-channel affine
     * y = y*post_scale[c] + post_shift[c] (applied after the bias, before res1) and a plain ReLU at the very end */
    const float* post_scale; const float* post_shift;   /* [cout padded to 16] or NULL */
    int post_relu;
    /* srbh_hconv_h16(bf16 = 0) only -- fp16 ACTIVATIONS in memory (inference: the producing epilogue rounds once, the consumer
     * stages the 8-byte channel quads as they are): bit 0 = src0 holds fp16, bit 1 = src1, bit 2 = res1, bit 3 = out is written as
     * fp16.  Such a tensor is NHWC with 2-byte elements; its *_ld stays in ELEMENTS.  An fp16 src0 takes no pre_scale / pre_relu (the
     * producer applied them), an fp16 out no PixelShuffle store and no statistics; channel counts and strides multiples of 4. */
    int io_h16;
    /* backward-statistics epilogue (srbh_hconv_h16, the persistent 16 -> 16 3x3 kernel only; SR/HRfuse.py:146-157 in reverse): the conv
     * output is the gradient da of a = relu(bn(c)).  With bstat_c (the BatchNorm input, NHWC fp32 [B][H][W][16]), the batch mean / invstd
     * and the folded affine (ms, mh: a > 0 <=> c*ms + mh > 0; both NULL = no ReLU) given, `stats` receives sum(dz) and sum(dz * xhat),
     * dz = da where the ReLU was active -- exactly what srbh_bn_bwd_reduce computes in a pass of its own (pass the same buffer to
     * srbh_bn_bwd_finalize).  No res1; cout == 16.  With a bf16 output (SRBH_IO_OUT_H16) the sums are taken from the fp32 accumulators
     * BEFORE the one rounding of the store, whereas the separate reduce pass (srbh_bn_bwd_reduce_io) sums the rounded tensor: dgamma /
     * dbeta / the mean terms of the two paths differ by bf16 rounding noise averaged over B*H*W elements (not bit-comparable;
     * tests/test_gpu_io16.py bounds it) -- fp16 also drops the out "no PixelShuffle" rule for the full 16 -> 64 conv (see pixelshuffle2). */
    const float* bstat_c; const float* bstat_mean; const float* bstat_invstd; const float* bstat_ms; const float* bstat_mh;
    /* nonzero: the caller guarantees that `stats` is all zero already (a buffer last consumed by srbh_bn_finalize_clear /
     * srbh_bn_bwd_finalize_clear, or freshly zeroed): this call then launches no zero fill of its own (round 5: 49 one-line fills per
     * training step sat as dependent launches in front of their convolutions) */
    int stats_clean;
} srbh_hconv_args;
#define SRBH_IO_SRC0_H16 1
#define SRBH_IO_SRC1_H16 2
#define SRBH_IO_RES1_H16 4
#define SRBH_IO_OUT_H16 8
int srbh_hconv_f32(const srbh_hconv_args* a, void* stream);
/* The same convolution with fp16 OPERANDS (staged activations and weights rounded to fp16, fp32 accumulate on
 * v_mfma_f32_16x16x16_f16; inputs / outputs / BatchNorm statistics stay fp32 in memory): 1/8 of the fp32 matrix-core time,
 * so the kernel runs at its HBM traffic (the head is HBM-bound; BASELINE configs[4] asks for fp16 MFMA).
 * `w` is the fp16 pack of srbh_hpack_conv_h16.  srbh_hconv_f32 remains the strict mode (<= 2e-5 against the reference). */
size_t srbh_hpack_h16_bytes(int cout, int cin, int ksize);
/* bf16 = 0: fp16 operands (forward: activations and weights are O(1));  bf16 = 1: bfloat16 operands on
 * v_mfma_f32_16x16x16_bf16 (data gradients: per-pixel gradients of a mean-reduced loss sit far below fp16's normal range,
 * bf16 keeps fp32's exponent).  The pack and the conv must use the same setting. */
int srbh_hpack_conv_h16(const float* w_oihw, int cout, int cin, int ksize, int transpose_flip, int bf16, void* packed, void* stream);
/* n such packs in ONE launch: table_dev[i] = the arguments of call i (w, cout, cin, ksize, transpose_flip, bf16, packed), in device memory;
 * max_elems = the largest srbh_hpack_h16_bytes(...) / 2 among them.  (hrfuse.py refreshes every registered head pack right behind
 * optimizer.step(): the weights the reference's torch.optim.Adam has just changed, train.py:256.) */
typedef struct srbh_hpack_desc {
    const float* w;
    void* out;
    int cout, cin, ksize, transpose_flip, bf16, pad_;
} srbh_hpack_desc;
int srbh_hpack_conv_h16_many(const srbh_hpack_desc* table_dev, int n, long max_elems, void* stream);
int srbh_hconv_h16(const srbh_hconv_args* a, int bf16, void* stream);
/* The entry of a BasicBlock with a downsample branch (SR/HRfuse.py:142-159): conv1 (3x3, `c1`) and downsample[0] (1x1, `ds`) read the
 * SAME input -- the widest tensor of each head.  One fused pass (the 1x1 is the centre tap with other weights) when both produce 16
 * channels from the same sources with 16-aligned channel counts, no pre-affine, W % 64 == 0, H % 4 == 0; otherwise exactly the two
 * srbh_hconv_h16 launches.  Same results either way (same operand rounding, fp32 accumulation). */
int srbh_hconv_entry_h16(const srbh_hconv_args* c1, const srbh_hconv_args* ds, int bf16, void* stream);

/* training-mode nn.BatchNorm2d statistics (SR/HRfuse.py:124,132,135): partial sums -> biased batch variance ->
 * scale = gamma/sqrt(var+eps), shift = beta - mean*scale; running stats updated with `momentum` and the unbiased
 * variance exactly as torch does; save_mean/save_invstd (optional) are kept for the backward pass. */
int srbh_bn_finalize(const double* stats, int C, double count, const float* gamma, const float* beta, float eps,
                     float momentum, float* running_mean, float* running_var, float* scale, float* shift,
                     float* save_mean, float* save_invstd, void* stream);
/* The same, and the partial-sum buffer is ZEROED behind the read (self-cleaning: the next producer may pass stats_clean = 1).  One
 * launch, one block: the zero fill is ordered behind this kernel's own reads of every slot. */
int srbh_bn_finalize_clear(double* stats, int C, double count, const float* gamma, const float* beta, float eps,
                           float momentum, float* running_mean, float* running_var, float* scale, float* shift,
                           float* save_mean, float* save_invstd, void* stream);
/* eval-mode BatchNorm folded to scale/shift from the running statistics */
int srbh_bn_eval_scale_shift(int C, const float* gamma, const float* beta, const float* running_mean,
                             const float* running_var, float eps, float* scale, float* shift, void* stream);
/* out = relu(a*a_scale + a_shift + (idt*i_scale + i_shift))   (BasicBlock tail, SR/HRfuse.py:150-157);
 * i_scale NULL = identity path without downsample.  C % 4 == 0; a, idt, out and the per-channel vectors are read as 4-channel groups:
 * 16-byte aligned (8 bytes for a tensor that holds fp16), anything else is refused. */
int srbh_bn_add_relu(const float* a, const float* a_scale, const float* a_shift, const float* idt,
                     const float* i_scale, const float* i_shift, float* out, long npix, int C, void* stream);
/* The same pass with fp16 tensors in memory (round 3: the training step keeps the block-internal activations c1 / c2 / downsample
 * output as fp16): io bit SRBH_BAR_A_H16 = `a` holds fp16 elements, SRBH_BAR_IDT_H16 = `idt` does; `out` stays fp32. */
#define SRBH_BAR_A_H16 1
#define SRBH_BAR_IDT_H16 2
int srbh_bn_add_relu_io(const void* a, const float* a_scale, const float* a_shift, const void* idt,
                        const float* i_scale, const float* i_shift, float* out, long npix, int C, int io, void* stream);
/* ... and ALSO writing the ReLU's activity pattern as bits (round 4): per 64 consecutive 4-channel groups four 64-bit words (word j bit l:
 * element j of group 64 k + l is > 0), srbh_relu_bits_bytes(npix, C) bytes, C % 4 == 0.  srbh_bn_bwd_reduce_io(SRBH_BN_REF_BITS) takes it
 * in place of the fp32 block output: the backward's reduce pass reads 1 bit per element instead of 4 bytes. */
size_t srbh_relu_bits_bytes(long npix, int C);
int srbh_bn_add_relu_bits(const void* a, const float* a_scale, const float* a_shift, const void* idt, const float* i_scale,
                          const float* i_shift, float* out, void* bits, long npix, int C, int io, void* stream);
/* aggregate_torch (aggregate_utils.py:29-41): data [N][H][W] fp32 -> out [N][H/step][W/step] */
int srbh_aggregate(const float* data, float* out, int N, int H, int W, int step, void* stream);
/* F.interpolate(scale_factor=2, mode='nearest') on NHWC fp32 (SR/rrdbnet_arch.py:236-237); H, W = output size */
int srbh_nearest2x_f32(const float* src, float* dst, int B, int H, int W, int C, void* stream);
/* NCHW fp32 -> NHWC fp32 */
int srbh_nchw_to_nhwc_f32(const float* src, float* dst, int B, int C, int H, int W, void* stream);

/* ---- head backward (training; the reference relies on torch autograd over SR/HRfuse.py, train.py:254-256) ---- */
/* dW[oc][ci][tap] = sum_px dy[px][oc] * X[px+tap][ci] with X = cat(pre(src0), src1) exactly as srbh_hconv_f32 reads it.
 * dw is OIHW fp32 [cout][c0+c1][ksize][ksize]; it is zeroed by this call. */
typedef struct srbh_hwgrad_args {
    const float* src0; int c0;
    const float* pre_scale; const float* pre_shift; int pre_relu;
    const float* src1; int c1;
    const float* dy;      /* NHWC [B][H][W][cout] */
    int cout; int ksize;
    int B, H, W;
    float* dw;            /* OIHW [cout][c0+c1][k][k], fully written (deterministic: fixed summation order) */
    float* ws;            /* scratch of srbh_hwgrad_ws_bytes(cout, c0 + c1, ksize) bytes: per-workgroup partial sums */
    int src0_ld, src1_ld; /* floats between consecutive pixels of src0 / src1 (0 = c0 / c1): strided views into wider NHWC
                           * buffers, e.g. the first 64 + 32k channels of a dense block's 192-channel buffer */
    int io;               /* srbh_hconv_wgrad_b16 only: SRBH_WG_SRC0_H16 = src0 holds fp16 elements (16 -> 16 3x3 form),
                           * SRBH_WG_DY_B16 = dy holds bf16 elements (its bits are the MFMA operand: no rounding) */
} srbh_hwgrad_args;
#define SRBH_WG_SRC0_H16 1
#define SRBH_WG_DY_B16 2
size_t srbh_hwgrad_ws_bytes(int cout, int cin, int ksize);
int srbh_hconv_wgrad_f32(const srbh_hwgrad_args* a, void* stream);
/* Mixed-precision form of the same gradient (torch.cuda.amp-style training; the reference itself trains in fp32,
 * train.py:254-256): X and dY are rounded to bf16 (RNE) while staged, products on v_mfma_f32_16x16x16_bf16, fp32 accumulation,
 * same workspace and fixed summation order.  Needs c0, c1, the pixel strides % 4 == 0, cout % 16 == 0 and 16-byte aligned
 * pointers; a layer outside that (the 1- / 7-channel output convs) is computed by the fp32 kernel. */
int srbh_hconv_wgrad_b16(const srbh_hwgrad_args* a, void* stream);
/* The two weight gradients of a BasicBlock ENTRY (SR/HRfuse.py:142-159: conv1 = 3x3, downsample[0] = 1x1, same input) in ONE pass over
 * that input: a3 / a1 = the arguments the two srbh_hconv_wgrad_b16 calls would take.  Fused when they describe the same sources, shape
 * and element types (cout a multiple of 16, 4-aligned channels); otherwise it runs the two calls.  Same results either way. */
int srbh_hconv_wgrad_entry_b16(const srbh_hwgrad_args* a3, const srbh_hwgrad_args* a1, void* stream);
/* The backward of ONE 3x3, 16 -> 16 convolution of a BasicBlock behind its BatchNorm, in one pass (round 5; reference graph:
 * SR/HRfuse.py:142-159 through torch autograd).  With y = bn(conv(x')), g = dL/dy and the constants of srbh_bn_bwd_finalize,
 *     dc = coef * (g' - k1 - xhat * k2),  g' = g where c*mask_scale + mask_shift > 0 (mask optional),  xhat = (c - mean) * invstd
 * is formed while the window is staged (rounded once to bf16, as srbh_bn_bwd_apply_io's bf16 store did) and feeds BOTH
 *     dw[oc][ci][tap] = sum_px dc[px][oc] * x'[px + tap][ci],   x' = relu?(x*pre_scale + pre_shift) rounded to bf16   (srbh_hconv_wgrad_b16)
 *     dx[px][ci]      = conv^T(dc, W) [+ res]                                                                          (srbh_hconv_h16, bf16)
 * without dc ever being written: 160 - 256 bytes per pixel instead of the 352 of apply + weight gradient + data gradient.
 * g / res: bf16 NHWC [B][H][W][16];  c / x / bstat_c: fp32 NHWC [B][H][W][16];  w: srbh_hpack_conv_h16(transpose_flip = 1, bf16 = 1);
 * dx: bf16 (dx_b16) or fp32;  dw: OIHW fp32 [16][16][3][3];  ws: srbh_hwgrad_ws_bytes(16, 16, 3).
 * stats (optional, srbh_bn_stats_bytes(16)): the BatchNorm-backward sums of dx as the gradient of relu?(bn'(bstat_c)) -- srbh_hconv_args'
 * bstat epilogue -- taken from the fp32 accumulators; no res then (but see relu_bits).  W % 64 == 0, H % 4 == 0 (srbh_hbwd16_supported). */
typedef struct srbh_hbwd16_args {
    const void* g; const float* c;
    const float* mean; const float* invstd; const float* coef; const float* k1; const float* k2;
    const float* mask_scale; const float* mask_shift;
    const float* x; const float* pre_scale; const float* pre_shift; int pre_relu;
    const void* w;
    int B, H, W;
    void* dx; int dx_b16;
    const void* res;
    const float* bstat_c; const float* bstat_mean; const float* bstat_invstd; const float* bstat_ms; const float* bstat_mh;
    double* stats; int stats_clean;
    float* dw; float* ws;
    /* optional (conv1's use inside a chain of blocks, hrfuse_autograd._BlockChainFn): dx (+ res) is the gradient of the PREVIOUS block's output
     * out' = relu(bn2'(c2') + idt').  With relu_bits (srbh_bn_add_relu_bits' buffer of that block) dx is masked with that ReLU, written as
     * bf16 (dx_b16 must be 1) and `stats` receives the BatchNorm-backward sums of bn2' (bstat_c = c2', bstat_mean / bstat_invstd its batch
     * statistics, no bstat_ms) over the rounded values: the previous block's srbh_bn_bwd_reduce_io pass, without the fp32 tensor. */
    const void* relu_bits;
} srbh_hbwd16_args;
int srbh_hbwd16_supported(int H, int W);
int srbh_hbwd16(const srbh_hbwd16_args* a, void* stream);

/* A whole PLAIN BasicBlock of the inference head in one pass (round 6; reference: SR/HRfuse.py:142-159 in eval mode):
 *     out = relu(bn2(conv2(relu(bn1(conv1(x))))) + x),   conv1 / conv2 = 3x3, 16 -> 16, no bias; bn folded to (scale, shift) per channel
 * with fp16 operands and the fp16 intermediate of the two-launch chain (srbh_hconv_h16 x 2: post_scale / post_relu / out fp16, then res1 = x)
 * kept inside the compute unit: 32 bytes read and 32 (out_h16) / 64 written per pixel instead of 160.  Bit-identical to that chain.
 * x: fp16 NHWC [B][H][W][16];  w1 / w2: srbh_hpack_conv_h16(ksize 3, transpose_flip 0, bf16 0);  out: fp16 (out_h16) or fp32 NHWC.
 * W % 64 == 0, H % 4 == 0 (srbh_hblock16_supported); 8-byte aligned x / fp16 out, 16-byte aligned fp32 out and packs. */
typedef struct srbh_hblock16_args {
    const void* x;
    const void* w1; const void* w2;
    const float* scale1; const float* shift1; const float* scale2; const float* shift2;
    void* out; int out_h16;
    int B, H, W;
} srbh_hblock16_args;
int srbh_hblock16_supported(int H, int W);
int srbh_hblock16_eval(const srbh_hblock16_args* a, void* stream);

/* Deferred weight-gradient reduces (round 5; hrfuse_autograd._BlockChainFn.backward).  The reference gets dW from torch autograd
 * (train.py:254-256); nothing reads it before the optimizer / the gradient all-reduce, so the ordered reduce of the per-workgroup partial sums
 * need not sit between the chip-filling kernels of the head's backward.  Between srbh_hwgrad_defer(1) and srbh_hwgrad_flush the entry points
 * srbh_hconv_wgrad_f32 / _b16 / _entry_b16 and srbh_hbwd16 launch their kernels but QUEUE that reduce (host thread local, any number of
 * jobs); srbh_hwgrad_flush(stream) runs all queued reduces as one pair of launches (same order of additions per element) and ends the
 * deferral.  The caller keeps every `ws` / `dw` of a queued job alive until the flush. */
int srbh_hwgrad_defer(int on);
int srbh_hwgrad_flush(void* stream);
/* out = g where ref > 0 else 0   (ReLU backward with the saved output, SR/HRfuse.py:157) */
int srbh_relu_mask_mul(const float* g, const float* ref, float* out, long n, void* stream);
int srbh_add_inplace(float* a, const float* b, long n, void* stream);
/* per-channel partial sums (into a srbh_bn_stats_bytes(C) buffer, zeroed here) of dy and dy*xhat,
 * dy = g * [c*mask_scale + mask_shift > 0] (mask optional), xhat = (c - mean)*invstd (c optional: bias gradients) */
int srbh_bn_bwd_reduce(const float* g, const float* c, const float* mean, const float* invstd, const float* mask_scale,
                       const float* mask_shift, long npix, int C, double* stats, void* stream);
/* The same reduction with the block-closing ReLU backward folded in (SR/HRfuse.py:157): dy = g where relu_ref > 0, else 0; dy is also
 * written to dz_out (may be NULL) for the skip / downsample branches.  C % 4 == 0, 16-byte aligned tensors. */
int srbh_bn_bwd_reduce_relu(const float* g, const float* relu_ref, float* dz_out, const float* c, const float* mean,
                            const float* invstd, long npix, int C, double* stats, void* stream);
/* dgamma = sum dy*xhat, dbeta = sum dy, and the constants of dc = coef*(dy - k1 - xhat*k2) (coef may be NULL) */
int srbh_bn_bwd_finalize(const double* stats, int C, double count, const float* gamma, const float* invstd,
                         float* dgamma, float* dbeta, float* coef, float* k1, float* k2, void* stream);
/* srbh_bn_bwd_finalize + zero fill of `stats` behind the read (see srbh_bn_finalize_clear) */
int srbh_bn_bwd_finalize_clear(double* stats, int C, double count, const float* gamma, const float* invstd,
                               float* dgamma, float* dbeta, float* coef, float* k1, float* k2, void* stream);
int srbh_bn_bwd_apply(const float* g, const float* c, const float* mean, const float* invstd, const float* mask_scale,
                      const float* mask_shift, const float* coef, const float* k1, const float* k2, float* out, long npix,
                      int C, void* stream);
/* The two BatchNorm-backward passes with 16-bit tensors in memory (round 3; vector form only: C % 4 == 0, 256 % (C/4) == 0): the
 * gradient tensors that live INSIDE one BasicBlock's backward are bf16 (SRBH_BN_G_B16: g; SRBH_BN_OUT_B16: dz_out / out -- their
 * consumers round their operands to bf16 anyway), the saved activation c is fp16 (SRBH_BN_C_H16); relu_ref stays fp32; the
 * arithmetic is fp32, and with a bf16 dz_out the sums are taken over the rounded values (what the consumers read).
 * srbh_bn_bwd_reduce_io: relu_ref / dz_out as srbh_bn_bwd_reduce_relu (may be NULL), mask_* as srbh_bn_bwd_reduce.
 * Without a dz_out nothing is rounded: the sums are those of the masked g.  srbh_bn_bwd_apply_io refuses tensors and per-channel
 * vectors that are not 16-byte aligned (8 bytes for a 16-bit tensor).  A refused call of any of these writes nothing, `stats` included. */
#define SRBH_BN_OUT_B16 1
#define SRBH_BN_C_H16 2
#define SRBH_BN_G_B16 4
#define SRBH_BN_REF_BITS 8   /* srbh_bn_bwd_reduce_io: relu_ref points at srbh_bn_add_relu_bits' bit buffer, not at an fp32 tensor */
#define SRBH_BN_STATS_CLEAN 16   /* srbh_bn_bwd_reduce_io: `stats` is all zero already (see srbh_hconv_args.stats_clean): no zero fill here */
int srbh_bn_bwd_reduce_io(const void* g, const float* relu_ref, void* dz_out, const void* c, const float* mean, const float* invstd,
                          const float* mask_scale, const float* mask_shift, long npix, int C, double* stats, int io, void* stream);
int srbh_bn_bwd_apply_io(const void* g, const void* c, const float* mean, const float* invstd, const float* mask_scale,
                         const float* mask_shift, const float* coef, const float* k1, const float* k2, void* out, long npix, int C,
                         int io, void* stream);
/* inverse of the PixelShuffle(2) store map: g_ps [B][2H][2W][C] -> g [B][H][W][4C] */
int srbh_ps2_inverse(const float* g_ps, float* g, int B, int H, int W, int C, void* stream);

/* ---- depthwise KxK convolution (K = 3|5, stride 1|2), fp32 NCHW, zero padding folded in (pad_t / pad_l given, bottom /
 * right implied by OH / OW): the EfficientNet encoder's `_depthwise_conv` (third-party efficientnet_pytorch called from
 * mymodels.py:242-248), for which MIOpen only has its naive fp32 kernels.  x [B][C][H][W], w [C][1][K][K],
 * y / dy [B][C][OH][OW]; bwd_weight sums in a fixed order (deterministic). */
int srbh_dwconv_fwd(const float* x, const float* w, float* y, int B, int C, int H, int W, int K, int stride, int pad_t,
                    int pad_l, int OH, int OW, void* stream);
int srbh_dwconv_bwd_data(const float* dy, const float* w, float* dx, int B, int C, int H, int W, int K, int stride,
                         int pad_t, int pad_l, int OH, int OW, void* stream);
/* ws: caller-provided scratch of srbh_dwconv_bwd_weight_splits(B, C) * C * K * K floats (per-batch-slice partial sums) */
int srbh_dwconv_bwd_weight_splits(int B, int C);
int srbh_dwconv_bwd_weight(const float* x, const float* dy, float* dw, float* ws, int B, int C, int H, int W, int K, int stride,
                           int pad_t, int pad_l, int OH, int OW, void* stream);

/* inference BatchNorm folded to a per-channel affine (srbh_bn_eval_scale_shift) + activation on NCHW fp32:
 * y = act(x * scale[c] + shift[c]), act 0 none | 1 SiLU | 2 ReLU; y may alias x. */
/* The encoder's stem at inference (round 6; smp EfficientNetEncoder.forward behind mymodels.py:276: _swish(_bn0(_conv_stem(x)))): a 3x3 conv with
 * stride `stride` and the static "same" zero padding (pt rows on top, pl columns on the left; whatever the window needs beyond the image on the
 * other sides is zero as well) + the folded BatchNorm (scale, shift per output channel) + activation (0 none, 1 SiLU, 2 ReLU) in ONE pass over
 * NCHW fp32 tensors.  w: OIHW fp32.  Cin <= 16, Cout in {32, 40, 48} (srbh_stem_conv_eval_supported: the stems of efficientnet-b0..b5; wider stems keep the stock conv). */
int srbh_stem_conv_eval_supported(int Cin, int Cout, int K);
int srbh_stem_conv_eval(const float* x, const float* w, const float* scale, const float* shift, float* y, int B, int Cin, int H, int W,
                        int Cout, int stride, int pt, int pl, int OH, int OW, int act, void* stream);
int srbh_affine_act_nchw(const float* x, const float* scale, const float* shift, float* y, int B, int C, int HW, int act,
                         void* stream);
/* y = act(x * scale[c] + shift[c]) + res: the closing BatchNorm of an MBConv block together with its skip connection
 * (efficientnet_pytorch MBConvBlock.forward: x = bn2(project_conv(x)); x = x + inputs), one pass instead of two. */
int srbh_affine_act_add_nchw(const float* x, const float* scale, const float* shift, const float* res, float* y, int B, int C, int HW,
                             int act, void* stream);

/* squeeze-and-excitation of an MBConv block at inference (efficientnet_pytorch MBConvBlock.forward, called through
 * mymodels.py:242-248): (1) affine + activation as above, also writing the per-plane mean pooled [B][C];
 * (2) hidden [B][SQ] = swish(b1 + w1 [SQ][C] . pooled); (3) y[plane (b,c)] *= sigmoid(b2[c] + w2 [C][SQ] . hidden[b]), in place. */
int srbh_affine_act_pool_nchw(const float* x, const float* scale, const float* shift, float* y, float* pooled, int B, int C,
                              int HW, int act, void* stream);
int srbh_se_hidden(const float* pooled, const float* w1, const float* b1, float* hidden, int B, int C, int SQ, void* stream);
int srbh_se_gate_scale(float* y, const float* hidden, const float* w2, const float* b2, int B, int C, int SQ, int HW,
                       void* stream);
/* (3') the gate on its own, gate [B][C] = sigmoid(b2[c] + w2 [C][SQ] . hidden[b]): the fused inference block hands it to the project conv
 * (srbh_pwconv_fwd_epi) instead of rewriting the expanded tensor. */
int srbh_se_gate(const float* hidden, const float* w2, const float* b2, float* gate, int B, int C, int SQ, void* stream);
/* MBConv middle at inference as ONE launch (efficientnet_pytorch MBConvBlock.forward through mymodels.py:242-248, eval mode):
 * y = swish(bn1(depthwise(swish(bn0(x))))) with both BatchNorms folded to (scale, shift) [C] (pre_scale / pre_shift null: the block has
 * no expand conv, x is used as it is), pooled [B][C] = per-plane mean of y.  Geometry as srbh_dwconv_fwd; _supported tells whether
 * the LDS-staged form takes the plane (else: the separate launches). */
int srbh_dwconv_eval_supported(int B, int C, int H, int W, int K, int stride, int pad_t, int pad_l, int OH, int OW);
int srbh_dwconv_eval_fwd(const float* x, const float* w, const float* pre_scale, const float* pre_shift, const float* scale,
                         const float* shift, float* y, float* pooled, int B, int C, int H, int W, int K, int stride, int pad_t,
                         int pad_l, int OH, int OW, void* stream);

/* ---- TRAINING-mode BatchNorm + activation and squeeze-and-excitation of the MBConv / U-Net decoder blocks (csrc/srbh_mbconv.hip) ----
 * Replaces, for the encoder / decoders the reference builds at mymodels.py:242-258 and runs at mymodels.py:276-287, the stock
 * F.batch_norm(training=True) + SiLU/ReLU (+ adaptive_avg_pool2d, + drop-connect multiply and skip add) launches and their autograd
 * backward.  fp32 NCHW; planes of HW = 1, 4, 16, 64 or 256 elements with B * max(64, HW) floats within LDS, or large planes
 * (srbh_bn_act_train_supported; anything else stays on the stock ops).
 *   forward :  mean / biased variance over (B, HW) in two passes, running statistics updated as nn.BatchNorm2d does (momentum, unbiased
 *              variance), y = act(gamma (x - mean) invstd + beta) [* drop[b]] [+ res],  pooled[b][c] = mean over the plane of y
 *   backward:  dy_eff = dy [* gate[b][c] + dpooled[b][c] / HW] [* drop[b]];  dz = dy_eff act'(z);  dbeta = sum dz;  dgamma = sum dz xhat;
 *              dx = gamma invstd (dz - mean(dz) - xhat mean(dz xhat))   (dx may be NULL: parameter gradients only)            */
typedef struct srbh_bnact_args {
    const float* x;            /* [B][C][HW] the convolution output */
    float* y;                  /* [B][C][HW] */
    const float* gamma;        /* [C] */
    const float* beta;         /* [C] */
    float* running_mean;       /* [C], updated in place; NULL (both) = no running statistics */
    float* running_var;
    float* save_mean;          /* [C] out: batch mean */
    float* save_invstd;        /* [C] out: 1 / sqrt(biased variance + eps) */
    float* pooled;             /* optional [B][C] out: plane means of y (the squeeze of squeeze-and-excitation) */
    const float* res;          /* optional [B][C][HW]: added after the activation (MBConv skip connection) */
    const float* drop;         /* optional [B]: per-sample drop-connect factor floor(keep + u) / keep, applied before `res` */
    float momentum, eps;
    int B, C, HW;
    int act;                   /* 0 none | 1 SiLU | 2 ReLU */
    void* ws;                  /* srbh_bn_act_train_ws_bytes(B, C, HW) bytes of scratch (large planes only; may be NULL when that is 0) */
} srbh_bnact_args;
typedef struct srbh_bnact_bwd_args {
    const float* dy;           /* [B][C][HW] gradient of the output */
    const float* x;            /* the forward's x */
    const float* gamma;
    const float* beta;
    const float* save_mean;
    const float* save_invstd;
    const float* gate;         /* optional [B][C] (with dpooled): the squeeze-excite gate the forward output was scaled by */
    const float* dpooled;      /* optional [B][C]: gradient of the plane means */
    const float* drop;         /* optional [B] */
    float* dx;                 /* [B][C][HW] or NULL */
    float* dgamma;             /* [C] */
    float* dbeta;              /* [C] */
    int B, C, HW;
    int act;
    void* ws;                  /* as in the forward */
} srbh_bnact_bwd_args;
/* 0 = not taken; 1 = small planes (one launch each way); 2 = large planes, HW a multiple of 4 from 256 up (two launches each way:
 * per-(channel, image subset) partial sums in double in fixed slots of `ws`, then one workgroup per plane) */
int srbh_bn_act_train_supported(int B, int C, int HW);
size_t srbh_bn_act_train_ws_bytes(int B, int C, int HW);
int srbh_bn_act_train_fwd(const srbh_bnact_args* a, void* stream);
int srbh_bn_act_train_bwd(const srbh_bnact_bwd_args* a, void* stream);
/* squeeze-and-excitation in training (efficientnet_pytorch MBConvBlock.forward: x_squeezed = avg_pool(x); se_expand(swish(se_reduce(.)));
 * x = sigmoid(.) * x): forward = hidden_pre [B][SQ] = b1 + w1 [SQ][C] . pooled, hidden = swish(hidden_pre), gate [B][C] =
 * sigmoid(b2 + w2 [C][SQ] . hidden), y[plane (b, c)] *= gate in place (two launches); the three extra outputs are what the backward reads.
 * backward (three launches; ws: srbh_se_train_bwd_ws_floats): from dout = gradient of the scaled output and the BatchNorm's saved x /
 * statistics (y = act(bn(x)) is recomputed, it was scaled in place) -> dpooled [B][C] (feed it with `gate` to srbh_bn_act_train_bwd) and the
 * gradients of the four squeeze-excite parameters, batch sums in a fixed order. */
int srbh_se_train_fwd(float* y, const float* pooled, const float* w1, const float* b1, const float* w2, const float* b2, float* hidden,
                      float* hidden_pre, float* gate, int B, int C, int SQ, int HW, void* stream);
int srbh_se_train_bwd(const float* dout, const float* x, const float* gamma, const float* beta, const float* save_mean,
                      const float* save_invstd, const float* pooled, const float* hidden, const float* hidden_pre, const float* gate,
                      const float* w1, const float* w2, float* ws, float* dpooled, float* dw1, float* db1, float* dw2, float* db2, int B,
                      int C, int SQ, int HW, int act, void* stream);
size_t srbh_se_train_bwd_ws_floats(int B, int C, int SQ);

/* U-Net decoder block entry (smp DecoderBlock.forward, reached through mymodels.py:279,287): out [B][Cx+Cs][2H][2W] =
 * cat(nearest-x2(x [B][Cx][H][W]), skip [B][Cs][2H][2W]) in one launch (skip may be NULL with Cs = 0); backward: dx = 2x2 sums of the first
 * Cx channels of dout, dskip = the remaining channels as a contiguous tensor (either output may be NULL).  fp32 NCHW, W even. */
int srbh_up2_cat_fwd(const float* x, const float* skip, float* out, int B, int Cx, int Cs, int H, int W, void* stream);
int srbh_up2_cat_bwd(const float* dout, float* dx, float* dskip, int B, int Cx, int Cs, int H, int W, void* stream);

/* ---- 1x1 convolutions of the MBConv blocks (expand / project: no bias, stride 1, no padding), fp32 NCHW (csrc/srbh_pwconv.hip) ----
 * What F.conv2d and its autograd do for efficientnet_pytorch's _expand_conv / _project_conv (reached through mymodels.py:276), as ONE launch
 * per product on the fp32 matrix unit (true fp32, fixed summation order):  x [B][Cin][HW], w [Cout][Cin], y [B][Cout][HW].
 * The weight gradient splits over images when its tile grid is small: partials in `ws` (srbh_pwconv_bwd_weight_ws_floats floats, 0 = not
 * needed) + one ordered reduce.  srbh_pwconv_supported: HW == 4 or a multiple of 16. */
int srbh_pwconv_supported(int B, int Cin, int Cout, int HW);
int srbh_pwconv_fwd(const float* x, const float* w, float* y, int B, int Cin, int Cout, int HW, void* stream);
/* the same forward reading W^T [Cin][Cout] (coalesced along Cout, as the input gradient reads W): 2x faster on the deep products.
 * srbh_transpose_many makes the transposed copies of a whole table of matrices (device-resident descriptors) in one launch. */
typedef struct srbh_transpose_desc {
    const float* src;          /* [rows][cols] */
    float* dst;                /* [cols][rows] */
    int rows, cols;
} srbh_transpose_desc;
int srbh_transpose_many(const srbh_transpose_desc* table_dev, int n, void* stream);
int srbh_pwconv_fwd_wt(const float* x, const float* wt, float* y, int B, int Cin, int Cout, int HW, void* stream);
/* forward with a fused prologue / epilogue (inference MBConv project conv): y = act((W . (x * gate)) * scale[co] + shift[co]) [+ res];
 * gate [B][Cin] (squeeze-excite, srbh_se_gate), scale / shift [Cout] (folded inference BatchNorm), res [B][Cout][HW] (skip connection):
 * each may be null.  w_transposed: w is W^T [Cin][Cout] as for srbh_pwconv_fwd_wt.  act 0 none | 1 SiLU | 2 ReLU. */
int srbh_pwconv_fwd_epi(const float* x, const float* w, int w_transposed, float* y, int B, int Cin, int Cout, int HW, const float* gate,
                        const float* scale, const float* shift, const float* res, int act, void* stream);
int srbh_pwconv_bwd_data(const float* dy, const float* w, float* dx, int B, int Cin, int Cout, int HW, void* stream);
/* the same with the gradient arriving over the MBConv block's skip connection (res: [B][Cin][HW], as dx) added in the store:
 * dX = W^T dY + res (efficientnet_pytorch MBConvBlock.forward's `x = x + inputs`, differentiated) */
int srbh_pwconv_bwd_data_res(const float* dy, const float* w, const float* res, float* dx, int B, int Cin, int Cout, int HW, void* stream);
size_t srbh_pwconv_bwd_weight_ws_floats(int B, int Cin, int Cout, int HW);
int srbh_pwconv_bwd_weight(const float* x, const float* dy, float* dw, float* ws, int B, int Cin, int Cout, int HW, void* stream);
/* Which kernel form the entry points above launch for a shape: host-only queries of the launchers' own rule, nothing is launched (tests
 * assert the form they mean to run, and that every form the production batches select is one they compare with a reference).
 * srbh_pwconv_gemm_plan: the forward (M = Cout, K = Cin; srbh_pwconv_fwd / _fwd_wt / _fwd_epi) and the data gradient (M = Cin, K = Cout;
 * srbh_pwconv_bwd_data / _bwd_data_res).  *family = 0 pw_gemm_kernel | 1 pw_gemm_lds_kernel; *form = the tile 0 16x16 | 1 16x32 | 2 32x32 of
 * family 0, or the LDS form 1 64x64 | 2 64x128 | 4 32x128; *kw = waves sharing one tile's K (1 | 4 | 16; 1 for every LDS form).
 * srbh_pwconv_wgrad_plan: *vec = 1 (2x2 planes, one K step per image) | 4 (float4 runs), *kw = waves per 16x16 tile (4 | 16), *nsplit =
 * image splits (1 ... 64; > 1 needs the workspace and runs the ordered reduce).  SRBH_OK, or an error (nothing stored) for a null pointer,
 * a dimension <= 0 or, for the weight gradient, a plane that is neither 4 nor a multiple of 16 elements. */
int srbh_pwconv_gemm_plan(int B, int M, int K, int HW, int* family, int* form, int* kw);
int srbh_pwconv_wgrad_plan(int B, int Cin, int Cout, int HW, int* vec, int* kw, int* nsplit);

/* ---- inference epilogue: quantise + integer mosaic (predict_realesanet_feature_globe.py:172-204) ------------------
 * accumulate: height [B][th][tw] fp32 (model output, C=1), build logits NHWC [B][th][tw][C] fp32, pos [B][4] int32
 *   = (xoff, yoff, xcount, ycount) already multiplied by 4 (predict...py:182); adds round(max(h,0)*10) and
 *   round(softmax*255) (both round-half-even, uint16 range) into uint32 mosaics [H][W], [C][H][W] and 1 into the
 *   weight mosaic, with atomics.  finalize: build class = argmax of the class sums (mod 2^16), height =
 *   round(sum/weight) where weight (mod 2^8) > 0 -- bit-identical to the reference's uint16/uint8 numpy arrays for any
 *   tile order or sharding (mosaics of different ranks add).
 * The contract in full (tests/test_gpu_mosaic_forms.py pins every line of it):
 *   accumulate  1 <= C <= 16 (the exponentials of a pixel are kept in registers), B, th, tw, H, W > 0, no null pointer; anything else
 *               is refused with nothing launched.  pos is in MOSAIC PIXELS.  Pixel (x, y) of tile b is added at (xoff + x, yoff + y) iff
 *               x < xcount, y < ycount and the target lies inside [0, W) x [0, H): counts beyond the tile are bounded by the tile,
 *               counts <= 0 and pixels off the city add nothing (the window arithmetic is 64-bit: no content of pos overflows it).
 *               The height quantum is rintf(fl32(max(h, 0) * 10)) mod 2^16 (h = -0.0 counts as 0), the class quantum
 *               rintf(e_c / s * 255) with e_c = expf(fl32(z_c - max z)), s = the fp32 sum of e in class order 0 .. C - 1.  The
 *               mosaics are added to, never cleared: whatever they hold (high bits included) stays in the sums.
 *   finalize    C >= 1 with NO upper limit (one pass over the class sums, nothing kept per class), H, W > 0, no null pointer.  Only
 *               res_height & 0xffff, res_build & 0xffff and res_weight & 0xff are read: the higher bits of the accumulators never
 *               reach an output.  build_out = the FIRST class holding the largest masked sum; height_out = rint(h16 / w8) in double
 *               (half to even) where w8 > 0, else h16 itself -- so a pixel covered by 256 tiles keeps its undivided (wrapped) sum, as
 *               the reference's uint8 weight does.  The three accumulators are not written. */
int srbh_mosaic_accumulate(const float* height, const float* build, int C, int B, int th, int tw, const int* pos,
                           unsigned* res_height, unsigned* res_build, unsigned* res_weight, int H, int W, void* stream);
int srbh_mosaic_finalize(const unsigned* res_height, const unsigned* res_build, const unsigned* res_weight, int C, int H,
                         int W, unsigned short* height_out, unsigned char* build_out, void* stream);

/* ---- loader-side tensor math (BH_loader.py:30-61,326-329,361-392) --------------------------------
 * label_prep: height uint8 [B][H][W] -> build (int64 class = buildhir_lut[height]), height as float,
 *   weight = class_weight[build], and per 4x4 cell height_aggre = aggregate_torch(height, 0.25),
 *   weight_aggre = class_weight[buildhir_lut[(long)height_aggre]]  ([B][H/4][W/4]).
 * normalize_clamp: dst = clip((src - mins[c]) / ranges[c], lo, hi) on NCHW fp32 (clip only when clamp != 0).
 * The contract in full (tests/test_gpu_loader_forms.py pins every line of it):
 *   label_prep       B, H, W > 0, H and W multiples of 4, no null pointer, `height` 4-byte aligned (it is read four labels at a time);
 *                    anything else is refused with nothing launched.  Every output is exact: a cell's sum of 16 uint8 labels is an
 *                    integer <= 4080, exact in fp32 in any order, and the divisor fl32(16 + 1e-10) IS 16, so height_aggre is the exact
 *                    quotient sum / 16 and (long)height_aggre its floor; class weights are copied bit for bit.
 *   normalize_clamp  every dimension > 0, no null pointer.  Two correctly rounded fp32 operations, so dst equals the IEEE value bit for
 *                    bit.  The clip is `v < lo ? lo : (v > hi ? hi : v)`, as img[img < lo] = lo; img[img > hi] = hi: NaN (0 / 0 of a band
 *                    with range 0, or NaN in src) stays NaN with or without the clip, -0.0 stays -0.0 under lo = 0, +-inf become hi / lo. */
int srbh_label_prep(const unsigned char* height, int B, int H, int W, const unsigned char* buildhir_lut,
                    const float* class_weight, long long* build, float* height_f, float* weight, float* height_aggre,
                    float* weight_aggre, void* stream);
int srbh_normalize_clamp(const float* src, float* dst, int B, int C, int H, int W, const float* mins, const float* ranges,
                         float lo, float hi, int clamp, void* stream);
/* Training augmentation of both datasets (BH_loader.py:356-359 in myImageFloder_S12_globe, :735-737 in myImageFloderLRHRglobe:
 * Compose([Flip, RandomGridShuffle(grid=(2, 2)), Rotate]), applied before the normalisation at :361-369 / :744-750, the x0.25
 * decimation at :365 and the label branch at :373-392).  The definition is DESIGN.md 3.x; the per-image parameters are device arrays
 * (Python: loader_math.Augment.to_device):
 *   flip   int32 [B]                  bit 0 reverses the columns, bit 1 the rows (only the low two bits are read);
 *   perm   int32 [B][4]               source cell of destination cell i, cells row-major (only the low two bits are read; 16-byte aligned);
 *   tables int32 [B][2 Wg + 2 Hg]     ax[Wg], bx[Wg], X0[Hg], Y0[Hg]: the inverse rotation in 2^-10 fixed point (16-byte aligned).
 * aug_image: src fp32 [B][C][Hs][Ws] holds the grid at 1/up (grid Hg x Wg = Hs up x Ws up, multiples of 8); dst fp32
 *   [B][C][Hg/step][Wg/step] is the bilinear REFLECT_101 sample of the augmented grid at (step j, step i), then
 *   clip((v - mins[c]) / ranges[c], lo, hi) as normalize_clamp (mins == ranges == NULL: no normalisation; clip only when clamp != 0).
 *   up 4 / step 4 is the LR tile (:353-365), up 1 / step 1 the SR stage's HR image (:735-750), up 4 / step 1 the augmented x4 image.
 * aug_label_prep: the nearest-sampled augmented uint8 label [B][H][W] fused with label_prep's five outputs; label_out (optional,
 *   4-byte aligned) receives the augmented label itself.
 * Refused with SRBH_ERR_ARG: null pointers, a grid side that is no multiple of 8 or above 32768, up or step < 1, a step that does not
 * divide the grid.  Flip codes and perms live on the device and are refused by the Python layer; the kernels mask them. */
int srbh_aug_image(const float* src, int B, int C, int Hs, int Ws, int up, float* dst, int step, const int* flip, const int* perm,
                   const int* tables, const float* mins, const float* ranges, float lo, float hi, int clamp, void* stream);
int srbh_aug_label_prep(const unsigned char* height, int B, int H, int W, const int* flip, const int* perm, const int* tables,
                        const unsigned char* buildhir_lut, const float* class_weight, long long* build, float* height_f,
                        float* weight, float* height_aggre, float* weight_aggre, unsigned char* label_out, void* stream);
/* Inference tiles cut and normalised from a city's device rasters (BH_loader.py:933-993, gridimgLoader.__getitem__: two window reads,
 * the band cut, the concatenate, the cast to float32 and (v - min) / (max - min) per band WITHOUT a clip -- one grid cell at a time
 * there, a batch of cells per launch here).
 *   srcA  [CA][H][W] of element type typeA (Sentinel-2), of which the first CA_used bands are taken (:958, :971);
 *   srcB  [CB][H][W] of element type typeB (Sentinel-1), all bands; NULL with CB = 0 for a tile of srcA's bands alone;
 *   pos   int32 [N][4] on the device: (xoff, yoff, xcount, ycount) in raster pixels;
 *   mins, ranges  fp32 [CA_used + CB] on the device (range = max - min, formed in float64 on the host as for normalize_clamp);
 *   dst   fp32 [N][CA_used + CB][tile][tile], 16-byte aligned; tile a multiple of 4, at most 256.
 * dst[n][c][j][i] = ((float)src_c[yoff + j][xoff + i] - mins[c]) / ranges[c]  where i < xcount, j < ycount AND the source pixel lies
 * inside the raster: normalize_clamp's two fp32 operations in its order (true division), the conversion to float exact for every type.
 * Everywhere else dst is +0.0f.  The zero fill is this project's own choice (the reference cannot batch a clipped window): it is the
 * zero padding predict_tiles gives a ragged batch, and the mosaic reads [:ycount, :xcount] of a tile's prediction only.  The
 * inside-the-raster test is part of the predicate, so no content of pos takes a load outside [0, C*H*W) of either source; offsets
 * are 64-bit (C*H*W of a large city exceeds 2^31).  Every element of dst is written, by one 16-byte store per four pixels.
 * Refused with SRBH_ERR_ARG: null srcA / pos / dst / mins / ranges; srcB and CB that disagree; an unknown type code; CA_used outside
 * 1..CA; N, H or W <= 0; tile < 4, no multiple of 4 or above 256; a dst that is not 16-byte aligned; too many workgroups.  The
 * windows live on the device: the Python layer (loader_math.check_windows) validates them. */
#define SRBH_GRID_F32 0
#define SRBH_GRID_U16 1
#define SRBH_GRID_I16 2
int srbh_grid_tiles(const void* srcA, int typeA, int CA, int CA_used, const void* srcB, int typeB, int CB, int H, int W,
                    const int* pos, int N, const float* mins, const float* ranges, float* dst, int tile, void* stream);

/* ---- loss and metric reductions ------------------------------------------------------------
 * Replace the elementwise / reduction passes of reference losses_pytorch/selfloss.py and metrics.py.  All outputs are
 * ACCUMULATED into caller-zeroed device buffers; fp64 accumulation.
 *
 * srbh_wmse_sum:  *out_sum += sum_i w_i (pred_i - target_i)^2      (selfloss.py:87-88; weight may be NULL, :75)
 * srbh_wmse_grad: grad_i = gscale[0] * 2 w_i (pred_i - target_i)   (gscale: device scalar, d loss / d sum)          */
int srbh_wmse_sum(const float* pred, const float* target, const float* weight, long n, double* out_sum, void* stream);
int srbh_wmse_grad(const float* pred, const float* target, const float* weight, long n, const float* gscale,
                   float* grad, void* stream);
/* srbh_cedice_sums: logits (B,C,HW) fp32 with element strides (b,c,p) -- NCHW and channels_last both work --,
 * labels (B*HW) int64 in [0,C), weight (B*HW) fp32 or NULL.  out4 += [ sum w*CE, sum pb*tb, sum pb, sum tb ] with
 * CE = -log softmax_y (selfloss.py:149,157), pb = softmax[1:].sum (:160-161), tb = (y > 0) (:162).
 * srbh_cedice_grad: dlogits (same strides) = g3[0]*d(sum w*CE) + g3[1]*d(sum pb*tb) + g3[2]*d(sum pb); elements between
 * the strided logits are not written.
 * A label outside [0,C) (the reference raises): srbh_cedice_sums makes out4[0] NaN and counts the pixel in out4[1..3] by
 * tb = (y > 0) alone; srbh_cedice_grad writes a FINITE gradient there, the softmax with no one-hot class:
 * dlogits_c = g3[0]*w*s_c + (g3[1]*tb + g3[2])*s_0*(s_c - [c == 0]).  The NaN of the sum is the signal, not the gradient. */
int srbh_cedice_sums(const float* logits, int B, int C, long HW, long b_stride, long c_stride, long p_stride,
                     const long long* labels, const float* weight, double* out4, void* stream);
int srbh_cedice_grad(const float* logits, int B, int C, long HW, long b_stride, long c_stride, long p_stride,
                     const long long* labels, const float* weight, const float* g3, float* dlogits, void* stream);
/* srbh_height_metric_sums: out[k*4 + {0,1,2,3}] += { sum d^2, sum |d|, sum d, count } over the pixels with cls == k,
 * d = pred - ref (metrics.py:186-200 computes rmse/mae/me per class from exactly these).
 * srbh_confusion_add: cm[label*num_class + pred] += 1 (metrics.py:71-73); *bad_flag = 1 if any value is out of range. */
int srbh_height_metric_sums(const float* pred, const float* ref, const long long* cls, long n, int num_class,
                            double* out, void* stream);
int srbh_confusion_add(const long long* pred, const long long* label, long n, int num_class,
                       unsigned long long* cm, int* bad_flag, void* stream);

/* ---- SR-stage quality metrics as one-read reductions (reference SR/psnr_ssim.py; csrc/srbh_sr_metrics.hip) ---------------------------
 * a, b: fp32 images of logical shape (B, C, H, W), C = 1 | 3, each with its own four ELEMENT strides {batch, channel, row, column} (host
 * array; non-negative): a channels_last network output, an NCHW target and a cropped view are all read in place.  y_only (C == 3): the
 * value used is the BT.601 luma of rgb2ycbcr_pt (psnr_ssim.py:122-144), computed in fp32 as there; the effective channel count Ce is then 1,
 * otherwise Ce = C.  Everything behind the fp32 values is float64.  Results are OVERWRITTEN (not accumulated) and bit-reproducible: an image's
 * numbers depend neither on the run nor on the batch it travels in (per-workgroup partial sums in fixed slots of `ws`, folded in a fixed
 * order; no floating-point atomics).  ws: srbh_*_ws_bytes bytes of device memory, no initialisation needed.  One launch + one small fold.
 *
 * srbh_sr_psnr_ssim_sums: per image i,  sq[i] = sum (a - b)^2 over Ce x H x W (calculate_psnr_pt :228-231 takes its mean), and
 *   ssim[i] = sum of the SSIM map over Ce x (H-10) x (W-10) (_ssim_pth :352-382: 11-tap Gaussian sigma 1.5, inputs * 255, C1 = (0.01*255)^2,
 *   C2 = (0.03*255)^2; run as a separable horizontal + vertical pass).  Either of sq / ssim may be NULL; with ssim NULL no window pass runs
 *   and H, W < 11 are allowed.
 * srbh_sr_cpsnr_sums: for calculate_cpsnr_pt (:443-490).  sd / sqd [B][Ce][81]: for offset index ro * 9 + co (ro, co in 0..8), the sums of
 *   d and d^2 over the (H-8) x (W-8) window, d = a[r+ro, c+co] - b[r+8-ro, c+8-co] (:473-476).  The bias-corrected MSE of :479-484 over a set
 *   of images is  sum_c [S(d^2) - S(d)^2 / N] / (Ce N)  with S the sums over the set and N its element count per channel. */
size_t srbh_sr_psnr_ssim_ws_bytes(int B, int H, int W);
int srbh_sr_psnr_ssim_sums(const float* a, const long* a_strides, const float* b, const long* b_strides, int B, int C, int H, int W,
                           int y_only, double* sq, double* ssim, void* ws, void* stream);
size_t srbh_sr_cpsnr_ws_bytes(int B, int C, int H, int W, int y_only);
int srbh_sr_cpsnr_sums(const float* a, const long* a_strides, const float* b, const long* b_strides, int B, int C, int H, int W,
                       int y_only, double* sd, double* sqd, void* ws, void* stream);

/* ---- Height-stage validation / test pass as one read of a batch (reference train.py:315-344 vtest_epoch, :427-486 vtest_epoch2,
 * metrics.py:67-74 genConfusionMatrix, :186-200 HeightMetric.addBatch; csrc/srbh_eval.hip) ---------------------------------------------
 * height fp32 (B, HW) with a batch ELEMENT stride (the model's (B,1,H,W) output, or a batch slice of it, is read in place); logits fp32
 * (B, C, HW) with batch / channel / pixel element strides as for srbh_cedice_sums (NCHW and channels_last are both read in place),
 * 2 <= C <= 16; ref fp32 (B, HW) and label (B, HW), int64 or (label_u8 != 0) uint8, both contiguous.  Per image b, OVERWRITTEN:
 *   sums[b][k][4] = { sum d^2, sum |d|, sum d, count } over the pixels with label k, d = (double)height - (double)ref (metrics.py:186-200
 *                   forms rmse / mae / me per class from exactly these; train.py:333-336, :444 take sqrt(mean d^2) over all pixels);
 *   cm[b][label * C + pred] = pixel counts, pred = argmax of the C logits as torch.argmax (train.py:446) takes it: the first index among
 *                   equal maxima, a NaN counts as the maximum and the first NaN wins (metrics.py:71-73).
 * *bad |= 1 if a label lies outside [0, C) (sticky: zeroed by the caller once, never cleared here); such a pixel is counted nowhere.
 * Optional (NULL: not produced) maps of every pixel, (B, HW) contiguous: q_height = np.round(max(height, 0) * 10) as uint16, half to even
 * (train.py:464-466), cls_map = the argmax as uint8 (train.py:476).
 * Bit-reproducible: the pixel -> workgroup map and every summation order depend on HW only (float64 partial sums in registers, one slot of
 * `ws` per workgroup, an ordered fold; no floating-point atomics), so an image's numbers depend neither on the run, nor on the batch it
 * travels in, nor on the logits layout.  ws: at least srbh_eval_ws_bytes(B, HW, C) bytes of device memory (0 for arguments the call would
 * refuse), no initialisation needed.  One launch + one small fold. */
typedef struct srbh_eval_args {
    const float* height; long height_bs;
    const float* logits; long logits_bs, logits_cs, logits_ps;
    const float* ref;
    const void* label; int label_u8;
    int B, C, HW;
    double* sums; long long* cm; int* bad;
    unsigned short* q_height; unsigned char* cls_map;
    void* ws; size_t ws_bytes;
} srbh_eval_args;
size_t srbh_eval_ws_bytes(int B, int HW, int C);
int srbh_eval_sums(const srbh_eval_args* a, void* stream);

/* ---- Dataset statistics where the data lies (reference stats_dataset_globe.py: main_stats :61-101, main_stats_buildingheight :133-159;
 * csrc/srbh_stats.hip) --------------------------------------------------------------------------------------------------------------
 * srbh_band_stats: src of logical shape (N, C, H, W) and element type `type` (SRBH_GRID_F32 / _U16 / _I16), read in place through the
 * three ELEMENT strides {image, band, row} of the host array `strides` (non-negative; the column stride is 1): a batch of tiles, a band
 * cut x[:, :6] and a crop raster[None, :, y0:y1, x0:x1] all work.  Offsets are 64-bit.  Per image n and band c, OVERWRITTEN:
 *   stats[n][c][4] = { min, max, mean, std } float64, GDAL's order (a row stats_s1[b][i, :] of the reference's table);
 *   count[n][c]    = the number of valid pixels, int64.
 * A pixel is valid unless it is NaN or equals *nodata (nodata: HOST pointer to a double, NULL = none).  std is the population form
 * sqrt(M2 / count).  count == 0 leaves four NaNs.  This is the project's own statement of what GDAL's ComputeStatistics(False) is
 * understood to return (an exact scan of every pixel); GDAL is not available where the project is built and tested, so no result of
 * GDAL itself has been compared.
 * Arithmetic: float64 behind the exact conversion of each value, corrected two-pass: pass 1 gives min, max, count and the sum (mean =
 * sum / count), pass 2 gives M2 = sum (x - mean)^2 - (sum (x - mean))^2 / count.  The error of the variance M2 / count is within
 * 2 [(n + 2) u var + (n u)^2 (mean^2 + var)], u = 2^-53, n = count (Chan, Golub & LeVeque 1983); the mean of an integer type is the
 * correctly rounded quotient of the exact sum.
 * One workgroup per (image, band); a band of at most 4096 pixels is read once (kept in registers between the passes), a larger one
 * twice.  The pixels are cut row-major into 16-byte groups, lane t of 256 adds the groups t, t + 256, ... in order, then the lanes of a
 * wave by a shuffle tree, then the waves in wave order.  Bit-reproducible: an image's numbers depend on that image alone -- not on the
 * run, the batch, N, or whether a group was fetched by one 16-byte load (base and strides multiples of 16 bytes) or element by element.
 * No floating-point atomics, no workspace, one launch.
 * Refused with SRBH_ERR_ARG: null src / strides / stats / count, an unknown type code, N, C, H or W <= 0, a negative stride,
 * N * C above 2^31 - 1 workgroups.
 *
 * srbh_label_hist: hist[256] int64, OVERWRITTEN, = the exact counts of the uint8 labels (N, HW), image n at labels + n * image_stride
 * (element stride, non-negative; a batch slice is read in place).  A workgroup counts 65536 consecutive labels of one image in 32 bits
 * (16 labels per lane and load where base and stride are multiples of 16; runs of equal neighbours are added once, into one LDS
 * sub-histogram per wave) and writes its slot of ws; a second kernel adds the slots into int64.  ws: srbh_label_hist_ws_bytes(N, HW)
 * bytes of device memory (0 for arguments the call would refuse), no initialisation needed.
 * Refused with SRBH_ERR_ARG: null labels / hist / ws, N or HW <= 0, a negative stride, more than 2^31 - 1 workgroups. */
int srbh_band_stats(const void* src, int type, const long* strides, int N, int C, int H, int W, const double* nodata,
                    double* stats, long long* count, void* stream);
size_t srbh_label_hist_ws_bytes(int N, long HW);
int srbh_label_hist(const unsigned char* labels, long image_stride, int N, long HW, long long* hist, void* ws, void* stream);

/* ---- Per-cell built-up counts of a city's grid (reference demo_preprocess_height_v2.py: Fishgrid_stats :1143-1186, compare_twotiff_valid
 * and compare_twotiff_valid_iou :740-933 -- one shapefile feature and two GDAL window reads at a time there, every window of a city in
 * one launch here; csrc/srbh_cells.hip) --------------------------------------------------------------------------------------------------
 * a, b: rasters of logical shape (H, W) and element type SRBH_GRID_U16 / _I16 / _U8, each read in place through its own ROW stride in
 * ELEMENTS (>= W; the column stride is 1): one band of a (C, H, W) raster and a cropped view both work.  b may be NULL (one raster).
 * pos int32 [N][4] on the device: (xoff, yoff, xcount, ycount) in raster pixels.  out int64 [N][4] on the device, OVERWRITTEN: per window
 *   out[n] = { n_a, n_b, n_and, count }
 * count = the window's pixels that lie inside the raster; n_a = those with f(a) > thr, n_b the same for b, n_and those where both hold
 * (b == NULL: n_b = n_and = 0).  f is the identity (wrap8 == 0) or the value's low eight bits as an unsigned number (wrap8 == 1): the
 * reference casts the window .astype(numpy.uint8) BEFORE it compares (:1172-1173, :790-791), so uint16 256 counts as 0 and int16 -1 as
 * 255.  From these: Fishgrid_stats' sum = n_a, compare_twotiff_valid's vrt_sum = n_b, absdiff = n_a + n_b - 2 n_and, and the union of
 * calculate_iou (:732-736) = n_a + n_b - n_and.  Integers only: exact, independent of any order, bit-equal between runs.
 * One workgroup of 256 lanes per window, windows of any size; rows are cut into 16-byte groups of a's ADDRESS, the alignment taken per
 * row; a group that lies wholly inside the raster's row is one 16-byte load with the pixels outside the window masked off, any other
 * group is read pixel by pixel.  Every pixel is predicated on the window AND the raster, so no load touches a byte outside the rows of
 * either raster, i.e. outside [a, a + ((H-1) * row_stride + W) * element size), whatever pos holds.  int32 partial counts per lane (hence
 * H * W < 2^31), a shuffle tree per wave, the four waves through LDS; no atomics, no workspace, no host synchronisation, one launch.
 * Refused with SRBH_ERR_ARG: null a / pos / out; float32 (the reference's cast of a float to uint8 is not defined outside 0..255) or an
 * unknown type code; N, H or W <= 0; a row stride below W; H * W >= 2^31; thr outside -32768..65535; wrap8 other than 0 / 1; a raster
 * that is not aligned to its element size.  The windows live on the device: the Python layer (city_grid.cell_counts) validates them. */
#define SRBH_GRID_U8 3
int srbh_cell_counts(const void* a, int typeA, long row_strideA, const void* b, int typeB, long row_strideB, int H, int W,
                     const int* pos, int N, int thr, int wrap8, long long* out, void* stream);

/* ---- A city's summary: exact integer sums of a value raster under a mask raster, per window, per block and as a histogram (the step
 * behind harness.predict_city's rasters: the reference's per-urban-centre mean and std of building height and its histogram of predicted
 * heights, gathered there one shapefile feature and one GDAL window read at a time; csrc/srbh_summary.hip) -------------------------------
 * v: the value raster of logical shape (H, W), element type SRBH_GRID_U16 or SRBH_GRID_U8; m: an optional mask raster (NULL: none) of
 * the same two types.  Each is read in place through its own ROW stride in ELEMENTS (>= W; the column stride is 1).  A pixel is SELECTED
 * when it lies inside the raster, v > vthr and (m == NULL or m > mthr); vthr and mthr lie in -1..65535 (-1 selects every value).
 * Integers only: exact, independent of any order, bit-equal between runs; no floating point, no host synchronisation.  Rows are cut into
 * 16-byte groups of v's ADDRESS, the alignment taken per row; a group wholly inside the raster's row is one 16-byte load with the pixels
 * outside the rectangle at hand masked off, any other group is read pixel by pixel; m's pixels of the same columns follow the same rule
 * with loads of element alignment.  Every load is predicated on the rectangle AND the raster: no byte outside
 * [v, v + ((H-1) * row_strideV + W) * element size) (and the same of m) is touched, whatever pos holds.
 * Overflow: a group's sum (16 values below 2^16) is 32-bit, everything kept across groups is 64-bit; v * v < 2^32 enters the sum of
 * squares through a 32 x 32 -> 64-bit multiply-add, and H * W < 2^31 keeps that sum below 2^63.
 *
 * srbh_window_sums: pos int32 [N][4] on the device, (xoff, yoff, xcount, ycount); out int64 [N][5] on the device, OVERWRITTEN:
 *   out[n] = { count, n, sum, sumsq, max }
 * count = the window's pixels inside the raster, n = the selected ones among them, sum / sumsq / max = the sum of v, of v * v and the
 * largest v over the selected pixels (all three 0 when n == 0).  Windows have any size and may overlap.  One workgroup of 256 lanes per
 * window, a shuffle tree per wave, the four waves through LDS; one launch, no atomics, no workspace.
 *
 * srbh_block_sums: the raster cut into block x block blocks from the top-left corner (block >= 1; edge blocks hold what lies inside the
 * raster), Hb = ceil(H / block), Wb = ceil(W / block); out int64 [4][Hb][Wb] on the device, planar, OVERWRITTEN: { n, sum, sumsq, max }
 * per block.  Every block has ONE owner -- a lane for block <= 8, a wave for block <= 64, a workgroup beyond --, so the raster is read
 * once whatever block is, nothing is added across owners, and there is no workspace.  A block larger than the raster is the raster.
 *
 * srbh_value_hist: hist int64 [nbins] on the device, OVERWRITTEN: the selected pixels counted by min(v / bin_width, nbins - 1), floor
 * division (exact: (v * M) >> 32 with M = floor(2^32 / bin_width) + 1 = srbh_value_hist_magic(bin_width) equals v / bin_width for every
 * uint16 v and every bin_width in 2..65535; bin_width 1, magic 0, takes v itself).  1 <= bin_width <= 65535, 1 <= nbins <= 4096.  At most
 * 2048 workgroups stride over the raster, each counts into its own LDS histogram (32-bit) and stores it to its slot of ws; a second
 * kernel adds the slots into int64 in slot order.  ws: srbh_value_hist_ws_bytes(H, W, nbins) bytes of device memory (0 for arguments the
 * call would refuse), no initialisation needed.
 *
 * Refused with SRBH_ERR_ARG, nothing launched: int16, float32 or unknown type codes; null v / pos / out / hist / ws; H, W or N <= 0; a
 * row stride below W; H * W >= 2^31; a raster not aligned to its element size; a threshold outside -1..65535; block < 1; bin_width or
 * nbins out of range.  The windows live on the device: the Python layer (city_summary.window_sums) validates host windows. */
int srbh_window_sums(const void* v, int typeV, long row_strideV, const void* m, int typeM, long row_strideM, int H, int W,
                     const int* pos, int N, int vthr, int mthr, long long* out, void* stream);
int srbh_block_sums(const void* v, int typeV, long row_strideV, const void* m, int typeM, long row_strideM, int H, int W,
                    int block, int vthr, int mthr, long long* out, void* stream);
unsigned srbh_value_hist_magic(int bin_width);
size_t srbh_value_hist_ws_bytes(int H, int W, int nbins);
int srbh_value_hist(const void* v, int typeV, long row_strideV, const void* m, int typeM, long row_strideM, int H, int W,
                    int vthr, int mthr, int bin_width, int nbins, long long* hist, void* ws, void* stream);

/* ---- Polygon zones over a city's rasters: the reference's "mean and std of building height in each urban center" (zonal_stats,
 * demo_preprocess_height_v2.py:450-570: one gdal.RasterizeLayer, one window read and one numpy.ma sum per feature there; every zone in
 * one call here, rasterised on the device with no zone raster ever stored; csrc/srbh_zones.hip) -------------------------------------------
 * v, m, the row strides, vthr and mthr: as for srbh_window_sums above.  A pixel is SELECTED when it is selected there AND lies in the zone.
 *
 * The zone rule (this project's own statement, modelled on RasterizeLayer without ALL_TOUCHED on the value raster's own grid: a pixel
 * belongs to a polygon when its centre does; no result of GDAL is compared).  Coordinates are raster pixels: the raster spans
 * [0, W] x [0, H], pixel (x, y) has its centre at (x + 1/2, y + 1/2); they are held as int32 fixed point with 8 fractional bits,
 * X = round_half_even(256 px), |X|, |Y| <= 2^29.  A zone is the set of the edges (X0, Y0, X1, Y1) of all rings of all its parts, closing
 * segments included; horizontal edges may be left out (they never cross a scanline and are skipped).  With cy = 256 y + 128 and
 * cx = 256 x + 128 an edge CROSSES row y when min(Y0, Y1) <= cy < max(Y0, Y1); its abscissa there is the rational
 * xc = X0 + (cy - Y0)(X1 - X0) / (Y1 - Y0); pixel (x, y) is IN THE ZONE iff the number of crossing edges with xc > cx is odd.  Even-odd
 * over all edges: exterior rings, holes and parts carry no flag, and where two parts overlap the overlap is outside.  A centre exactly on
 * a left or top boundary is in, on a right or bottom boundary out, so two zones that share an edge never both own a pixel and never
 * both miss it.  Integer form: oriented so that den = Y1 - Y0 > 0, with N = X0 den + (cy - Y0)(X1 - X0), a crossing toggles exactly the
 * pixels x < t, t = ceil((N - 128 den) / (256 den)).  Differences stay <= 2^30 and every product below 2^61: int64 holds them; no float
 * touches the rule.
 *
 * Tables, int32 on the device:
 *   edges    [E][4]   (X0, Y0, X1, Y1), aligned to 16 bytes; an edge with a coordinate beyond +-2^29 contributes nothing
 *   edge_off [Z + 1]  zone z owns edges[edge_off[z] .. edge_off[z + 1]); a range outside [0, E] is an empty zone
 *   items    [NI][5]  (zone, xoff, yoff, xcount, ycount): a band of a zone's bounding box in raster pixels, clipped to the raster like a
 *                     row of pos; a zone index outside [0, Z) does nothing.  A zone's items must not overlap and must cover every pixel
 *                     of it that is to count (city_zones.zone_items cuts them)
 *   item_off [Z + 1]  zone z's partials are those of items[item_off[z] .. item_off[z + 1]); a range outside [0, NI] gives zeros
 * One workgroup of 256 lanes per item.  Per batch of rows and segment of <= 8192 columns: the lanes take the zone's edges in turn, one
 * 16-byte load each; an edge toggles, in each row it crosses, one bit of an LDS bitmap (an LDS XOR atomic; t of the first row by one
 * 64-bit floor division, quotient and remainder stepped exactly from row to row); a suffix XOR along the rows turns toggles into the
 * in-zone mask; the batch is then walked in 16-byte groups as srbh_window_sums walks a window, the zone's bits ANDed into the selection,
 * a group without a pixel in the zone loading nothing.  Cost follows the items, not the raster.  Wrong tables may give wrong sums; they
 * never give a load outside the rasters' rows or the tables' own bytes, nor a store outside out / ws.  No global atomics, no host
 * synchronisation, integers only: exact and bit-equal between runs.
 *
 * srbh_zone_sums: out int64 [Z][5] on the device, OVERWRITTEN: { count, n, sum, sumsq, max } per zone -- count = the zone's pixels inside
 * the raster, the others over the selected pixels (0 when n == 0), overflow as for srbh_window_sums.  Each item's partials go to its slot
 * of ws (srbh_zone_sums_ws_bytes(NI) bytes, no initialisation needed); a second kernel adds each zone's slots in item order.  A zone
 * without items gives zeros.
 * srbh_zone_hist: hist int64 [Z][nbins], OVERWRITTEN: per zone the selected pixels counted by min(v / bin_width, nbins - 1) with
 * srbh_value_hist's multiply-shift; 1 <= bin_width <= 65535, 1 <= nbins <= 4096; a 32-bit LDS histogram per item goes to its slot of ws
 * (srbh_zone_hist_ws_bytes(NI, nbins) bytes), the second kernel adds the slots in item order.
 * The _ws_bytes queries are host only and return 0 for arguments the call would refuse.
 * Refused with SRBH_ERR_ARG, nothing launched: whatever srbh_window_sums refuses; a null table, out or ws; Z, E or NI <= 0; edges not
 * aligned to 16 bytes, out or ws not to 8; bin_width or nbins out of range. */
size_t srbh_zone_sums_ws_bytes(int NI);
size_t srbh_zone_hist_ws_bytes(int NI, int nbins);
int srbh_zone_sums(const void* v, int typeV, long row_strideV, const void* m, int typeM, long row_strideM, int H, int W,
                   const int* edges, const int* edge_off, int Z, int E, const int* items, const int* item_off, int NI, int vthr, int mthr,
                   long long* out, void* ws, void* stream);
int srbh_zone_hist(const void* v, int typeV, long row_strideV, const void* m, int typeM, long row_strideM, int H, int W,
                   const int* edges, const int* edge_off, int Z, int E, const int* items, const int* item_off, int NI, int vthr, int mthr,
                   int bin_width, int nbins, long long* hist, void* ws, void* stream);

/* ---- City validation: a predicted raster against a reference raster on the same grid, summed in exact integers (the reference's cal_rmse,
 * demo_preprocess_height_v2.py:1389-1406, its per-cell compare_twotiff_valid* family and, at city scale, vtest_epoch2's HeightMetric per
 * height class and SegmentationMetric of the class map; the exact rule below is this project's own; csrc/srbh_compare.hip) ------------------
 * p: the predicted raster, r: the reference raster, m: an optional third raster (NULL: none; the class raster) -- logical shape (H, W),
 * element type SRBH_GRID_U16 or SRBH_GRID_U8 each, read in place through its own ROW stride in ELEMENTS (>= W; the column stride is 1),
 * aligned to the element size only.  All values are raster units; nothing is scaled.  d = p - r, signed.
 * A pixel is COMPARED when it lies inside the raster (and inside the window, for srbh_pair_sums), the pair test of `mode` holds and
 * (m == NULL or m > mthr).  With P := p > pthr and R := r > rthr the pair test is
 *   SRBH_PAIR_ANY  P or R      SRBH_PAIR_BOTH  P and R      SRBH_PAIR_REF  R      SRBH_PAIR_PRED  P
 * pthr, rthr and mthr lie in -1..65535; -1 makes a test always true, so ANY with (-1, -1) compares every pixel.
 * Integers only: exact, independent of any order, bit-equal between runs; no floating point, no global atomics, no host synchronisation.
 * The rasters are walked as srbh_window_sums walks v and m (16-byte groups of p's ADDRESS, the alignment taken per row; r and m follow with
 * loads of element alignment; every load predicated on the rectangle AND the raster): no byte outside the rows of any of the three rasters
 * is touched, whatever pos holds.
 * Overflow: H * W < 2^31 and every value is below 2^16, so count and n stay below 2^31, the sums of p, r, |d| and |sum of d| below
 * 65535 * 2^31 < 2^47, and the sums of p^2, r^2, p r and d^2 below 65535^2 * (2^31 - 1) < 2^32 * 2^31 = 2^63: every sum fits int64.  A
 * group's sums of p, r, d and |d| (16 values below 2^16) are 32-bit, everything kept across groups is 64-bit; squares and products enter
 * through 32 x 32 -> 64-bit multiply-adds.
 *
 * srbh_pair_sums: pos int32 [N][4] on the device, (xoff, yoff, xcount, ycount), clipped to the raster; out int64 [N][10] on the device,
 * OVERWRITTEN:
 *   out[n] = { count, n, sd, sad, sdd, sp, sr, spp, srr, spr }
 * count = the window's pixels inside the raster (no test applies to it), n = the compared ones among them, and over the compared pixels
 * sd = sum d, sad = sum |d|, sdd = sum d^2, sp = sum p, sr = sum r, spp = sum p^2, srr = sum r^2, spr = sum p r (all 0 when n == 0).
 * One workgroup of 256 lanes per window, a shuffle tree per wave, the four waves through LDS; one launch, no atomics, no workspace.
 *
 * srbh_pair_class_sums: the whole raster (a sub-rectangle is a view).  edges: C int32 values ON THE HOST, strictly ascending,
 * edges[0] == 0, 2 <= C <= 16.  The class of a value v is the number of k in 1 .. C - 1 with v >= edges[k]: values at or beyond the last
 * edge fall in class C - 1.  For every compared pixel c = the class of r, pc = the value of m when m is given, else the class of p;
 * { n, sd, sad, sdd } of class c are updated and cm[c][pc] is incremented.  A compared pixel with m >= C is counted in the four sums, in
 * no column of cm, and in the counter bad.  out int64 [C * (4 + C) + 1] on the device, OVERWRITTEN: C rows
 *   { n, sd, sad, sdd, cm[c][0], ..., cm[c][C - 1] }   then   bad
 * (cm is [reference class][predicted class]).  With m as the class source mthr = -1 switches its masking off.  At most 2048 workgroups
 * stride over the raster; each keeps the table in LDS (64-bit LDS integer atomics; a group of one value throughout is one update, and a
 * lane carries the sums of its current class and the count of its current cm entry in registers and updates the table when they change) and
 * stores it to its slot of ws; a second kernel adds
 * the slots in slot order.  ws: srbh_pair_class_ws_bytes(H, W, C) bytes of device memory (0 for arguments the call would refuse), aligned
 * to 8 bytes, no initialisation needed.
 *
 * Refused with SRBH_ERR_ARG, nothing launched: a null p, r, pos, out, edges or ws; int16, float32 or unknown type codes; H, W or N <= 0; a
 * row stride below W; H * W >= 2^31; a raster not aligned to its element size; a threshold outside -1..65535; a mode outside 0..3; C
 * outside 2..16; edges[0] != 0 or edges not strictly ascending; out or ws not aligned to 8 bytes.  The windows live on the device: the
 * Python layer (city_compare.pair_sums) validates host windows and the size of a workspace. */
#define SRBH_PAIR_ANY 0
#define SRBH_PAIR_BOTH 1
#define SRBH_PAIR_REF 2
#define SRBH_PAIR_PRED 3
int srbh_pair_sums(const void* p, int typeP, long row_strideP, const void* r, int typeR, long row_strideR, const void* m, int typeM,
                   long row_strideM, int H, int W, const int* pos, int N, int mode, int pthr, int rthr, int mthr, long long* out,
                   void* stream);
size_t srbh_pair_class_ws_bytes(int H, int W, int C);
int srbh_pair_class_sums(const void* p, int typeP, long row_strideP, const void* r, int typeR, long row_strideR, const void* m, int typeM,
                         long row_strideM, int H, int W, const int* edges, int C, int mode, int pthr, int rthr, int mthr, long long* out,
                         void* ws, void* stream);

/* ---- Urban-centre validation: the pair sums above per POLYGON ZONE (the paper reports per urban centre; csrc/srbh_zone_compare.hip) -----
 * p, r, m, their types and row strides, mode, pthr, rthr, mthr: as for srbh_pair_sums.  edges, edge_off, Z, E, items, item_off, NI: the
 * device tables of srbh_zone_sums, unchanged (the same uploaded tables serve both).
 * The rule is the conjunction of the two rules above, each unchanged: a pixel enters the sums when it is IN THE ZONE (int32 fixed point
 * with 8 fractional bits, even-odd over all the zone's edges, the pixel's centre (x + 1/2, y + 1/2) decides, a centre on a left or top
 * boundary is in, on a right or bottom boundary out) AND COMPARED (inside the raster, the pair test of `mode` holds, and m == NULL or
 * m > mthr).  out int64 [Z][10] on the device, OVERWRITTEN:
 *   out[z] = { count, n, sd, sad, sdd, sp, sr, spp, srr, spr }
 * count = the zone's pixels inside the raster, as srbh_zone_sums defines it (no test of the comparison applies to it); n = the compared
 * ones among them; over those sd = sum d (d = p - r, signed), sad = sum |d|, sdd = sum d^2, sp = sum p, sr = sum r, spp = sum p^2,
 * srr = sum r^2, spr = sum p r (all 0 when n == 0).  A zone with no edge or no item gives zeros.
 * Overflow: the argument of srbh_pair_sums.  H * W < 2^31 and a zone's items do not overlap, so a zone holds fewer than 2^31 pixels, and
 * every value is below 2^16: count and n stay below 2^31, sp, sr, sad and |sd| below 65535 * 2^31 < 2^47, and spp, srr, spr and sdd below
 * 65535^2 * (2^31 - 1) < 2^32 * 2^31 = 2^63: every sum fits int64, in an item's slot and in the zone's row alike.  A group's sums of p, r,
 * d and |d| are 32-bit, everything kept across groups is 64-bit.
 * One workgroup of 256 lanes per item: the LDS bitmap of srbh_zone_sums (toggles, suffix XOR), the walk of srbh_pair_sums with p as the
 * raster that fixes the groups; a group's raster row is recovered once from its row pointer and addresses both the bitmap's row and m's;
 * a group without a pixel in the zone loads nothing, and m is loaded only where a pixel of the zone passed the pair test.  Ten int64 per
 * item go to its slot of ws (srbh_zone_pair_ws_bytes(NI) = NI * 10 * 8 bytes, 0 for NI <= 0; no initialisation needed), a second kernel
 * adds each zone's slots in item order.  Integers only, no global atomics, no host synchronisation: exact, bit-equal between runs and
 * independent of how the items are cut.  Wrong tables may give wrong sums; they never give a load outside the rasters' rows or the
 * tables' own bytes, nor a store outside out / ws.
 * Refused with SRBH_ERR_ARG, nothing launched, nothing written: a null p, r, table, out or ws; a type code that is not SRBH_GRID_U16 or
 * SRBH_GRID_U8; m given with typeM 0, or typeM given without m; H or W <= 0; H * W >= 2^31; a row stride below W; a raster not aligned to
 * its element size; edges not aligned to 16 bytes, another table not to 4, out or ws not to 8; Z, E or NI <= 0; a mode outside 0..3; a
 * threshold outside -1..65535. */
size_t srbh_zone_pair_ws_bytes(int NI);
int srbh_zone_pair_sums(const void* p, int typeP, long row_strideP, const void* r, int typeR, long row_strideR, const void* m, int typeM,
                        long row_strideM, int H, int W, const int* edges, const int* edge_off, int Z, int E, const int* items,
                        const int* item_off, int NI, int mode, int pthr, int rthr, int mthr, long long* out, void* ws, void* stream);

/* ---- City labels: building footprints burned into a raster (the reference's shp_to_tiff / shp2tif, demo_preprocess_height_v2.py:27-119
 * and main_shp2tif: one gdal.RasterizeLayer(..., options=["ATTRIBUTE=<field>"]) that paints every footprint, in feature order, with its
 * attribute value -- the reference height raster of the validation entries above and the training labels; csrc/srbh_burn.hip) -----------
 * out: a raster of logical shape (H, W), element type SRBH_GRID_U16 or SRBH_GRID_U8, WRITTEN in place through its ROW stride in ELEMENTS
 * (>= W; the column stride is 1), aligned to its element size only: an interior view of a larger raster works.
 *
 * The rule (this project's own, like the zone rule above; no result of GDAL is compared).  Feature f of Z is a zone in the sense of the
 * zone rule: all edges of all its rings, int32 fixed point with 8 fractional bits, |X|, |Y| <= 2^29, even-odd over its OWN edges, the pixel
 * centre (x + 1/2, y + 1/2) decides, a centre on a left or top boundary is in, on a right or bottom boundary out.  Each feature has one
 * value values[f], 0..65535 (0..255 for a uint8 raster; the kernel takes the low 16 / 8 bits).
 *   merge = SRBH_BURN_LAST (GDAL's replace): out[y][x] = values[f] of the LARGEST f whose zone holds the pixel.  A value of 0 burns like
 *                          any other.
 *   merge = SRBH_BURN_MAX:  the largest value among the features whose zones hold the pixel: independent of the order.
 * A pixel in no feature gets init; with keep != 0 it is not written at all and out keeps its contents there.  Overlap between two
 * features is resolved by merge; overlap of two parts of ONE feature is outside, as even-odd has always said.  Integers only: bit-equal
 * between runs and independent of how the host cuts the work.
 *
 * Tables, int32 on the device:
 *   edges, edge_off     exactly srbh_zone_sums' tables (the same uploaded tables serve both); edges aligned to 16 bytes; an edge with a
 *                       coordinate beyond +-2^29 contributes nothing; an edge range outside [0, E] is an empty feature
 *   values   [Z]        the value of each feature
 *   boxes    [Z][4]     (x0, y0, x1, y1), half open, in pixels: the rows y with Ymin <= 256 y + 128 < Ymax and the columns floor(Xmin / 256)
 *                       .. ceil(Xmax / 256) of the feature's edges, clipped to the raster (city_zones.zone_items' rows and columns).  Only
 *                       a filter: a wave skips a feature whose box misses its rectangle; a box that is too small loses pixels, one that
 *                       is too large costs time
 *   tile_off [NT + 1]   the raster is cut into tiles of srbh_burn_tile() = 64 x 64 pixels anchored at pixel (0, 0), NT = ceil(H / 64) *
 *                       ceil(W / 64) in row-major tile order; tile t walks tile_feat[tile_off[t] .. tile_off[t + 1]); a range outside
 *                       [0, NF] is an empty tile
 *   tile_feat [NF]      feature indices, ASCENDING within a tile (the order is the rule of SRBH_BURN_LAST); every feature whose box meets
 *                       the tile must be listed (city_burn.burn_tiles cuts them); an index outside [0, Z) does nothing.  NF = 0 is legal:
 *                       every tile is then empty (tile_feat must still be a valid pointer)
 * One workgroup of 256 lanes per tile, the grid is every tile of the raster; a tile without features stores init, or nothing under keep.
 * A wave owns 16 rows x 64 columns, a lane 16 consecutive pixels of one row, and the lane's values live in registers from the first
 * feature to the store: no LDS, no barrier, no atomic of any kind.  Per feature the box is tested against the wave's rectangle, per edge
 * its row range and right extent (both uniform across the wave); then each lane runs the crossing test for its row -- oriented so that
 * den = Y1 - Y0 > 0, with N as in the zone rule, pixel x is toggled iff cx den < N, cx = 256 x + 128; for the lane's run of 16 pixels that
 * is four compares of R = N - cx0 den against 8, 4, 2 and 1 times 256 den -- and XORs a 16-bit mask into its parity; after the feature's
 * last edge the lane replaces (or maxes) its values under the parity.  Overflow: |N| < 2^61 as in the zone rule; cx den stays inside int64
 * only because a pixel with cx > 2^29 cannot lie in any zone: the columns x >= 2^21 never burn, and a tile there walks no feature before
 * any product is formed, so |X0 - cx0| <= 2^30 and |R| < 2^61.
 * Stores: a lane's 16 pixels go out as aligned 16-byte vector stores when the run lies wholly inside the raster and its address is
 * 16-byte aligned (and, under keep, all 16 were burned), otherwise element by element, each store predicated on x < W && y < H.  No byte
 * outside out's rows [0, H) x [0, W) is written, whatever the tables hold: wrong tables give wrong pixels at worst, never a load outside
 * the tables' own bytes nor a store outside out.  No host synchronisation.
 *
 * Refused with SRBH_ERR_ARG, nothing launched, nothing written: a null out or table; a type other than SRBH_GRID_U16 / SRBH_GRID_U8; H, W,
 * Z or E <= 0, or NF < 0; H * W >= 2^31; a row stride below W; out not aligned to its element size; edges not aligned to 16 bytes, another
 * table not to 4; NT not equal to the tile count of H x W; merge outside 0..1; init outside the type's range. */
#define SRBH_BURN_LAST 0
#define SRBH_BURN_MAX 1
int srbh_burn_tile(void);    /* 64: the tile side the tables must be cut for; host only */
int srbh_burn(void* out, int typeO, long row_strideO, int H, int W,
              const int* edges, const int* edge_off, const int* values, const int* boxes, int Z, int E,
              const int* tile_off, const int* tile_feat, int NT, int NF,
              int merge, int keep, int init, void* stream);

/* ---- The middle of an MBConv block in ONE launch per direction (round 4; efficientnet_pytorch MBConvBlock.forward between the expand and
 * the project conv, run by smp's encoder at mymodels.py:276): BatchNorm0 (training) + SiLU -> depthwise KxK, stride 1, "same" zero padding ->
 * BatchNorm1 (training) + SiLU (+ the plane means squeeze-and-excitation pools).  fp32 NCHW, square planes 2x2 / 4x4 / 8x8, K = 3 | 5.
 * forward: reads e_pre (the expand conv's output), writes d_pre (the depthwise output, kept for the backward), y and pooled, both
 * BatchNorms' batch statistics and running statistics.  backward: dout = gradient of y * gate (the excite gate [B][C]), dpooled = gradient
 * of the plane means [B][C]; writes de_pre (may be NULL), the depthwise weight gradient [C][K][K] and the four affine gradients. */
typedef struct srbh_mbmid_args {
    const float* e_pre; const float* wdw;
    const float* gamma0; const float* beta0; float* running_mean0; float* running_var0; float* mean0; float* invstd0;
    const float* gamma1; const float* beta1; float* running_mean1; float* running_var1; float* mean1; float* invstd1;
    float* d_pre; float* y; float* pooled;
    float momentum0, eps0, momentum1, eps1;
    int B, C, H, W, K;
} srbh_mbmid_args;
typedef struct srbh_mbmid_bwd_args {
    const float* dout; const float* gate; const float* dpooled;
    const float* d_pre; const float* e_pre; const float* wdw;
    const float* gamma0; const float* beta0; const float* mean0; const float* invstd0;
    const float* gamma1; const float* beta1; const float* mean1; const float* invstd1;
    float* de_pre; float* dwdw; float* dgamma0; float* dbeta0; float* dgamma1; float* dbeta1;
    int B, C, H, W, K;
} srbh_mbmid_bwd_args;
int srbh_mbconv_mid_supported(int B, int C, int H, int W, int K, int stride);
int srbh_mbconv_mid_fwd(const srbh_mbmid_args* a, void* stream);
int srbh_mbconv_mid_bwd(const srbh_mbmid_bwd_args* a, void* stream);

/* ---- 3x3 convolutions of the two U-Net decoders (mymodels.py:245-258 builds them, :279 / :287 call them; smp UnetDecoder blocks:
 * nearest x2 -> concat skip -> [Conv3x3 (no bias) + BatchNorm + ReLU] x 2) on NCHW fp32 tensors, square planes 4x4 ... 64x64, 16-bit
 * matrix-core operands, fp32 accumulation (csrc/srbh_dconv.hip).  Weights: srbh_hpack_conv_h16(w, Cout, Cin, 3, transpose_flip, bf16, ...).
 *   srbh_dconv_fwd(bf16 = 0): y = conv3x3(x, w), fp16 operands;
 *   srbh_dconv_fwd(bf16 = 1) with the transposed + flipped pack (hpack cout := forward Cin, cin := forward Cout): dX = conv^T(dY, W);
 *   srbh_dconv_wgrad: dW = sum_pixels dY (x) shifted X, bf16 operands, deterministic (ws: srbh_dconv_wgrad_ws_floats floats). */
typedef struct srbh_dconv_pack_desc {
    const float* w;      /* OIHW fp32 (cout, cin, 3, 3) */
    void* fwd;           /* fp16 image for srbh_dconv_fwd(bf16 = 0) */
    void* bwd;           /* bf16 transposed + flipped image for the data gradient */
    int cout, cin;
} srbh_dconv_pack_desc;
/* both images of n weights in ONE launch (table in device memory); each image = srbh_hpack_h16_bytes(cout, cin, 3) bytes */
int srbh_dconv_pack_many(const srbh_dconv_pack_desc* table, int n, void* stream);
int srbh_dconv_supported(int B, int Cin, int Cout, int H, int W);
int srbh_dconv_fwd(const float* x, const void* wpack, float* y, int B, int Cin, int Cout, int H, int W, int bf16, void* stream);
/* the same conv with y = act(conv * scale[co] + shift[co]) in its store: a decoder block's inference BatchNorm (folded, srbh_bn_eval_scale_shift)
 * and ReLU (act 2; 0 = none) without a pass of their own (smp DecoderBlock's Conv2dReLU, mymodels.py:245-258 in eval mode) */
int srbh_dconv_fwd_epi(const float* x, const void* wpack, float* y, int B, int Cin, int Cout, int H, int W, int bf16, const float* scale,
                       const float* shift, int act, void* stream);
size_t srbh_dconv_wgrad_ws_floats(int B, int Cin, int Cout, int H, int W);
int srbh_dconv_wgrad(const float* x, const float* dy, float* dw, float* ws, int B, int Cin, int Cout, int H, int W, void* stream);
/* Which kernel form the entry points above launch for a shape: host-only queries of the launchers' own planning rule, nothing is launched
 * (tests assert the form they mean to run, and that every form the production batches select is one they compare with a reference).
 * srbh_dconv_fwd_plan: *npx = pixels per workgroup tile (64 | 256), *mb = 16-channel output blocks per workgroup (1 | 2) of srbh_dconv_fwd /
 * srbh_dconv_fwd_epi; chosen from (B, Cout, W) alone -- for the data gradient Cout is the forward Cin.  srbh_dconv_wgrad_plan: *mo = 16-channel
 * output blocks per workgroup (1 | 2), *nsplit = workgroups sharing the pixels of one dW block.  SRBH_OK, or an error (nothing stored) for a
 * null pointer or a geometry srbh_dconv_supported refuses. */
int srbh_dconv_fwd_plan(int B, int Cout, int W, int* npx, int* mb);
int srbh_dconv_wgrad_plan(int B, int Cin, int Cout, int W, int* mo, int* nsplit);

/* ---- Adam (train.py:170-179,254-256: torch.optim.Adam over the network's parameters + the loss log_vars) as ONE launch over every parameter
 * tensor (csrc/srbh_optim.hip).  `table` (device memory): one entry per tensor -- p, m (exp_avg), v (exp_avg_sq) updated in place from the
 * gradient g (NULL: the tensor is skipped this step), n elements, the tensor's learning rate and (L2) weight decay.  `chunks` (device memory,
 * nchunks x 2 ints): (table index, slice) pairs, slice s covering elements [s * srbh_adam_chunk(), ...) of that tensor.  Arithmetic of
 * torch/optim/adam.py (amsgrad = maximize = False): g += wd * p; m = lerp(m, g, 1 - beta1); v = beta2 v + (1 - beta2) g^2;
 * p -= lr / bias_correction1 * m / (sqrt(v) / sqrt(bias_correction2) + eps), the bias corrections 1 - beta^t per tensor in the table. */
typedef struct srbh_adam_entry {
    float* p; const float* g; float* m; float* v;
    long n;
    float lr, wd;
    float inv_bc1, inv_sqrt_bc2;     /* 1 / (1 - beta1^t), 1 / sqrt(1 - beta2^t) with t = THIS tensor's step count (torch counts steps per parameter) */
} srbh_adam_entry;
int srbh_adam_chunk(void);
int srbh_adam_step(const srbh_adam_entry* table, const int* chunks, int nchunks, double beta1, double beta2, double eps, void* stream);

/* ---- VGG19 perceptual loss on ACT16 planes (reference SR/srloss.py:61-105 VGGFeatureExtractor, :108-143 PerceptualLoss; wired at
 * SR/rrdbnet_arch.py:496-498, used at :559-562).  srgan.PerceptualLoss.libsrbh = "f16" runs the feature stack, the loss and its input
 * gradient on the entry points below.  Arithmetic contract (restated in DESIGN.md 4):
 *   forward   x_n = (x [+1)/2] - mean) / std in fp32 (each operation rounded as torch's), rounded RNE to fp16: 3 channels of a 32-channel
 *             plane, the rest zero.  Each conv z = conv(a, w): fp16 operands (srbh_pack_conv3x3_f16's pack), exact products, fp32
 *             accumulation, fp32 bias.  The plane of a conv that is a cut (a feature) holds rne16(z), the plane of any other conv
 *             rne16(relu(z)).  The next conv reads relu(plane), behind a pool the 2x2 / stride-2 maximum of it (floor on odd sizes).  ReLU and
 *             max commute with the rounding: one fp16 rounding per conv defines the whole forward.
 *   loss      per cut i: w_i * mean |f_i(x) - f_i(gt)| (squared difference for "l2") on the fp16 planes, float64 sums in a fixed order
 *             (bit-reproducible); the same read writes the loss gradient w_i / N_i * sign(d) (sign(0) = 0; 2 d for l2) as bf16 planes.
 *   backward  bf16 gradient planes, transposed + flipped weights packed once as bf16 (srbh_pack_conv3x3_b16), fp32 accumulation, each plane
 *             rounded once to bf16.  At a conv's pre-activation  g_z = [loss gradient of this cut] + (saved plane > 0 ? 1 : 0) *
 *             pool_backward(g from above);  pool_backward sends the gradient to the FIRST maximum of the window in row-major order (torch's
 *             tie rule).  dloss/dx leaves as fp32 NCHW, divided by std (and by 2 with the range map), times grad_output.
 *
 * srbh_wconv3x3: the wide form of the trunk-family conv (SR/srloss.py:8-48 lists the stack: every conv 3x3 / stride 1 / pad 1, 64..512
 * channels).  One launch covers all output channels: workgroup = (8 x 64 tile, 64-channel output slice; one 32-channel slice when
 * cout == 32).  in: 16-bit ACT16 planes, any in_chunks >= 1; w: the ordinary WPACK16 of the whole (cout, 32 * in_chunks) weight
 * (srbh_pack_conv3x3_f16, or _b16 with bf16 != 0: bf16 input planes, weights and 16-bit outputs); bias: fp32, cout rounded up to 32
 * floats, or NULL.  Epilogue, in this order: + bias; mask16 != NULL: v = saved fp16 plane > 0 ? v : 0 (ReLU backward); add16 != NULL:
 * v += planes of the OUTPUT's 16-bit format (the cut's loss gradient); relu: v = max(v, 0).  out16: ACT16 planes, RNE, interior only;
 * out32: fp32 NHWC with out32_c <= cout channels per pixel (the unrounded values).  cout: 32 or a multiple of 64. */
typedef struct srbh_wconv3x3_args {
    const void* in; int in_chunks_total, in_chunk0, in_chunks;
    const void* w; const float* bias; int cout;
    int B, H, W;
    int bf16, relu;
    const void* mask16; int mask_chunks_total, mask_chunk0;
    const void* add16; int add_chunks_total, add_chunk0;
    void* out16; int out16_chunks_total, out16_chunk0;
    float* out32; int out32_c;
} srbh_wconv3x3_args;
int srbh_wconv3x3(const srbh_wconv3x3_args* a, void* stream);
/* SR/srloss.py:97-100 (range map, input normalisation): x fp32 NCHW (B, 3, H, W) -> one fp16 ACT16 plane (channels 3..31 zero), interior only.
 * mean / std: 3 host floats each, or both NULL (no normalisation); range_norm != 0: (x + 1) / 2 first. */
int srbh_vgg_input_f16(const float* x, void* plane, int B, int H, int W, const float* mean, const float* std_, int range_norm, void* stream);
/* SR/srloss.py:101-105 runs nn.ReLU / nn.MaxPool2d(2, 2) between the convs: out = relu(in), or (pool != 0) the 2x2 / stride-2 maximum of
 * relu(in) on (H / 2) x (W / 2) planes (floor).  fp16 ACT16 planes, `chunks` of them per image in both buffers, interior only. */
int srbh_vgg_relu_pool_f16(const void* in, void* out, int B, int chunks, int H, int W, int pool, void* stream);
/* the backward of the above at a conv's pre-activation (autograd of SR/srloss.py:135-141's loss through :101-105):
 *   out = [add] + (saved > 0 ? 1 : 0) * route(g),   route = identity (pool == 0, g on H x W planes) or the max-pool backward (pool != 0, g on
 * (H / 2) x (W / 2) planes): the gradient of a window goes to its first maximum of relu(saved) in row-major order; pixels outside every window
 * (odd sizes) get none.  g, add (may be NULL), out: bf16 planes; saved: the fp16 plane the forward stored; fp32 sum, one RNE rounding. */
int srbh_vgg_relu_pool_bwd_b16(const void* g, const void* saved, const void* add, void* out, int B, int chunks, int H, int W, int pool, void* stream);
/* SR/srloss.py:135-141, one cut: d = fx - fg on fp16 planes (B, 32 * chunks, H, W).  acc[0] = (accumulate ? acc[0] : 0) + coef * S with
 * S = sum |d| (l2: sum d^2) in float64, fixed order (per-workgroup slots of ws, then an ordered fold; no atomics).  grad != NULL: bf16
 * planes of gscale * sign(d) (l2: gscale * d, d = fx - fg in fp32; pass gscale = 2 w / N), gscale rounded to fp32 by the caller.
 * ws: srbh_vgg_dist_ws_bytes bytes of device memory, no initialisation needed. */
size_t srbh_vgg_dist_ws_bytes(int B, int chunks, int H, int W);
int srbh_vgg_dist(const void* fx, const void* fg, int B, int chunks, int H, int W, int l2, double coef, int accumulate, double* acc, float gscale,
                  void* grad, void* ws, void* stream);
/* the last step of the input gradient: g fp32 NHWC (B, H, W, 3) (srbh_wconv3x3's out32 of the first conv's data gradient) -> dx fp32 NCHW,
 * dx = g / std[c] (/ 2 with range_norm) * *grad_output (a DEVICE scalar).  std_: 3 host floats or NULL. */
int srbh_vgg_dx_nchw(const float* g, float* dx, int B, int H, int W, const float* std_, int range_norm, const float* grad_output, void* stream);

/* ---- the discriminator's 4x4 / stride 2 / pad 1 convolutions (SR/rrdbnet_arch.py:262-264 conv1..conv3, used at :277-279) on ACT16 planes:
 * srgan.UNetDiscriminatorSN.libsrbh_s2 = "f16" (csrc/srbh_disc.hip).  With xpad = x (C, H, W; C % 32 == 0, H and W even) in a
 * zero ring of 1, the conv is a 2x2-tap VALID conv over the space-to-depth image of xpad -- no tap wasted, no strided read:
 *   S[(2p+q) C + c][u][v]     = xpad[c][2u+p][2v+q]                   4C channels, (H/2+1) x (W/2+1)
 *   W2[o][(2p+q) C + c][a][b] = w[o][c][2a+p][2b+q]                   a, b in {0, 1}
 *   y[o][i][j]   = sum_{k,a,b} W2[o][k][a][b] S[k][i+a][j+b]          Ho x Wo = H/2 x W/2
 *   dS[k][u][v]  = sum_{o,a,b} Wt[k][o][a][b] gpad[o][u+a][v+b]       Wt[k][o][a][b] = W2[o][k][1-a][1-b]; gpad = g in a zero ring of 1
 *   dx           = depth-to-space(dS) with the ring cropped
 *   dW2[o][k][a][b] = sum_{n,i,j} g[n][o][i][j] S[n][k][i+a][j+b]     (dw[o][c][2a+p][2b+q] = dW2[o][(2p+q) C + c][a][b])
 * Arithmetic contract (rne16 = round to nearest even to fp16, bf16 likewise; every product of two 16-bit operands is exact in fp32, fp32
 * accumulation in any order, fp32 results unrounded):
 *   forward          y  = conv(rne16(x), rne16(w))
 *   data gradient    dx = conv^T(bf16(g), bf16(w))
 *   weight gradient  dw = sum bf16(g) * bf16(rne16(x))    fixed summation order, no atomics: two calls on the same input are bit-equal
 * No entry below launches anything when an argument check fails. */
/* x fp32 NHWC (B, H, W, C) -> the 4C / 32 chunk planes of S (phase (p, q) fills the C / 32 planes from (2p+q) C / 32 on), fp16 or (bf16 != 0)
 * bf16, RNE.  The whole (H/2+1) x (W/2+1) interior is written, the pad-derived zeros included; plane borders and read slack are those of
 * srbh_act16_bytes(B, 4 C, H/2+1, W/2+1) (zeroed once by whoever allocates the buffer). */
int srbh_s2d_nhwc32_to_act16(const float* x, void* planes, int B, int C, int H, int W, int bf16, void* stream);
/* g fp32 NHWC (B, H, W, C) -> C / 32 chunk planes with interior (H+2) x (W+2): the data at (1, 1), the ring written as zeros (gpad above);
 * buffer: srbh_act16_bytes(B, C, H+2, W+2). */
int srbh_nhwc32_to_act16_framed(const float* x, void* planes, int B, int C, int H, int W, int bf16, void* stream);
/* the weight packs of the 2x2-tap form: [input chunk][tap a*2+b][k-step][cout / 32][lane][8], 8 KiB per (chunk, 32 output channels).
 * srbh_pack_conv4x4s2: w fp32 OIHW [O][C][4][4]; transpose_flip = 0: W2, a (cout = O, cin = 4C) pack; 1: Wt, a (cout = 4C, cin = O) pack; RNE to
 * fp16 or (bf16 != 0) bf16.  Both have srbh_wpack2x2_bytes(O, 4 C) bytes.  _pair: W2 in fp16 and Wt in bf16 in one launch (spectral norm
 * rewrites the weight on every training forward). */
size_t srbh_wpack2x2_bytes(int cout, int cin);
int srbh_pack_conv4x4s2(const float* w, int O, int C, int transpose_flip, int bf16, void* packed, void* stream);
int srbh_pack_conv4x4s2_pair(const float* w, int O, int C, void* w2_f16, void* wt_b16, void* stream);
/* the 2x2-tap VALID form of srbh_wconv3x3 (same kernel body, taps dy, dx in {1, 2} of its pad-1 indexing; 8 weight fragments per chunk and
 * 32 output channels instead of 18): out32[n][i][j][o] = sum_{k,a,b} W[o][k][a][b] in[n][k][i+a][j+b] for i < H, j < W from planes whose
 * interior is (H+1) x (W+1) (buffer geometry of srbh_act16_bytes(B, 32 in_chunks_total, H+1, W+1)).  a->w: a srbh_pack_conv4x4s2 pack of
 * (cout, 32 in_chunks); bf16 selects the operand format of planes and pack.  cout % 64 == 0, in_chunks >= 1, out32_c == cout; bias, relu,
 * mask16, add16 and out16 must be 0 / NULL (the module applies LeakyReLU outside). */
int srbh_wconv2x2(const srbh_wconv3x3_args* a, void* stream);
/* ds fp32 NHWC (B, H/2+1, W/2+1, 4C) -> dx fp32 NHWC (B, H, W, C): dx[y][x][c] = ds[(y+1)/2][(x+1)/2][(2 ((y+1)%2) + (x+1)%2) C + c], the
 * exact inverse permutation of S with the ring dropped. */
int srbh_d2s_nhwc32(const float* ds, float* dx, int B, int C, int H, int W, void* stream);
/* dw fp32 OIHW [O][C][4][4] from the saved fp16 planes of S (srbh_s2d_nhwc32_to_act16 of the (B, 2 Ho, 2 Wo, C) input) and the framed bf16
 * planes of g (srbh_nhwc32_to_act16_framed of (B, Ho, Wo, O)); S is re-rounded fp16 -> bf16 while staged, as srbh_act16_wgrad_b16 does.
 * O % 64 == 0, C % 32 == 0.  ws: srbh_wgrad4x4s2_ws_bytes bytes, no initialisation needed. */
size_t srbh_wgrad4x4s2_ws_bytes(int O, int C, int B, int Ho, int Wo);
int srbh_wgrad4x4s2_b16(const void* s_planes, const void* g_planes, int B, int C, int O, int Ho, int Wo, float* dw, void* ws, void* stream);

/* ---- the discriminator's wide 3x3 / stride 1 / pad 1 convolutions with LeakyReLU (SR/rrdbnet_arch.py:265-269 conv4..conv8, used at :285-300:
 * act(conv_k(t)), bias-free, slope 0.2) on ACT16 planes: srgan.UNetDiscriminatorSN.libsrbh_wide = "f16" (csrc/srbh_disc3.hip).
 *   z  = conv(x, w)                 y = z >= 0 ? z : 0.2 z
 *   g' = g * (y > 0 ? 1 : 0.2)      (torch's leaky_relu backward rule on the saved output)
 *   dx[c][i][j]    = sum_{o,a,b} Wt[c][o][a][b] g'[o][i+a-1][j+b-1]       Wt[c][o][a][b] = w[o][c][2-a][2-b]
 *   dw[o][c][a][b] = sum_{n,i,j} g'[n][o][i][j] x[n][c][i+a-1][j+b-1]     (zero outside the image)
 * Arithmetic contract, that of the 4x4 stride-2 block above (rne16 = round to nearest even to fp16, bf16 likewise; every product of two 16-bit
 * operands is exact in fp32, fp32 accumulation in any order, fp32 results unrounded):
 *   forward          y  = lrelu(conv(rne16(x), rne16(w))), the one product of the LeakyReLU rounded in fp32
 *   staged gradient  g' = bf16(g * (y > 0 ? 1 : slope)), the product formed in fp32
 *   data gradient    dx = conv(g', bf16(Wt))
 *   weight gradient  dw = sum g' * bf16(rne16(x))      fixed summation order, no atomics: two calls on the same input (and the same walker
 *                                                       count) are bit-equal
 * No entry below launches anything when an argument check fails. */
/* srbh_wconv3x3 with the forward LeakyReLU (slope 0.2, v >= 0 ? v : v * 0.2f in fp32) as the last step of the epilogue, in front of the 16-bit
 * and fp32 stores: the same kernel body, one more compile-time form.  bias, relu, mask16 and add16 must be 0 / NULL; everything else as
 * srbh_wconv3x3 (cout 32 or a multiple of 64, out16 and / or out32, bf16 selects the operand format). */
int srbh_wconv3x3_lrelu(const srbh_wconv3x3_args* a, void* stream);
/* g, y fp32 NHWC (B, H, W, C), y the saved output of the forward -> the C / 32 chunk planes of rne(g * (y > 0 ? 1 : slope)) as bf16 (bf16 != 0)
 * or fp16; interior only: the zero border of a buffer of srbh_act16_bytes(B, C, H, W) (zeroed once by whoever allocates it) is kept.
 * C % 32 == 0; one read of each input. */
int srbh_nhwc32_to_act16_lrelu_bwd(const float* g, const float* y, void* planes, int B, int C, int H, int W, float slope, int bf16, void* stream);
/* both packs of one weight in one launch (spectral norm rewrites the weight on every training forward): w fp32 OIHW [cout][cin][3][3];
 * w_f16 = the WPACK16 of w in fp16, the bits of srbh_pack_conv3x3_f16(w, cout, cin); wt_b16 = the WPACK16 of Wt (above) in bf16, the bits of
 * srbh_pack_conv3x3_b16(Wt, cin, cout).  cout % 32 == 0, cin % 32 == 0: both packs have srbh_wpack16_bytes(cout, cin) bytes. */
int srbh_pack_conv3x3_pair(const float* w_oihw, int cout, int cin, void* w_f16, void* wt_b16, void* stream);
/* dw fp32 OIHW [cout][cin][3][3] from the fp16 planes the forward staged (x: chunk planes 0 .. cin / 32 - 1 of a buffer of x_chunks_total
 * planes, re-rounded fp16 -> bf16 (RNE) while staged, as srbh_act16_wgrad_b16 and srbh_wgrad4x4s2_b16 do; the planes' zero border is the padding)
 * and the bf16 planes of g' (srbh_nhwc32_to_act16_lrelu_bwd).  One launch covers all output channels: a workgroup owns a 64 (o) x 32 (c) x 9
 * block and walks the 8 x 64 tiles blockIdx.x, + walkers, ...; its partial sums go to its own slot of ws, a second kernel folds the slots in
 * walker order.  cin % 32 == 0; cout 32 or a multiple of 64.  ws: srbh_wgrad3x3_ws_bytes bytes (0 for a shape the entry refuses), no
 * initialisation needed.  Nothing outside the planes' borders is read. */
size_t srbh_wgrad3x3_ws_bytes(int cout, int cin, int B, int H, int W);
int srbh_wgrad3x3_b16(const void* x_planes, int x_chunks_total, int cin, const void* g_planes, int g_chunks_total, int cout, int B, int H, int W,
                      float* dw, void* ws, void* stream);
/* test hook: at most `cap` walkers per block in srbh_wgrad3x3_b16 / _ws_bytes from now on (process-wide); 0 restores the default (one workgroup
 * per compute unit over all blocks).  Returns the previous value.  Small shapes need it to give a workgroup more than one tile. */
int srbh_wgrad3x3_walkers_cap(int cap);

#ifdef __cplusplus
}
#endif
#endif /* SRBH_H */
