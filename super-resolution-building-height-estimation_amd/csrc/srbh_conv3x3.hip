// srbh_conv3x3.hip -- fused 3x3 convolution for gfx950 (MI355X), fp16 operands / fp32 accumulate.
//
// Stands in for every nn.Conv2d(.., 3, 1, 1) of the RRDBNet trunk and upsampler
// (reference SR/rrdbnet_arch.py:125-143,197-204,232-238) with the surrounding elementwise ops
// (bias, LeakyReLU 0.2, x5*0.2+x, out*0.2+x, feat+body_feat, nearest-x2 read) fused in.
//
// Formulation: implicit GEMM on the matrix cores, D[oc][px] = sum_k W[oc][k] * X[k][px], with
//   A (32 rows)  = 32 output channels x 16 input channels of one filter tap  (WPACK16 fragment, 1 KiB)
//   B (32 cols)  = 32 consecutive output pixels of one row x the same 16 input channels
//   v_mfma_f32_32x32x16_f16, K loop = (input chunk of 32 ch) x (9 taps) x (2 k-steps)
// The im2col is never materialised: the input tile (+1 pixel halo, zero border kept in HBM by the
// ACT16 layout) is staged once per 32-channel chunk into LDS by LDS-DMA (global_load_lds_dwordx4)
// and every tap is just a different LDS address of the same tile.
//
// Workgroup = 256 threads = 4 waves (one per SIMD) -> 8 rows x 64 cols of output, all `cout` channels.
//   wave (wr, wc) owns rows wr*4..+3, cols wc*32..+31: 4 (x cout/32) accumulators of 32x32.
//   per (k-step, dx): 6 pixel fragments (rows -1..4) + 3 weight fragments feed 12 (x cout/32) MFMAs.
// LDS: 2 stages x (input tile 10x66x64 B + weight chunk 18 KiB x cout/32), double buffered, one barrier per chunk.
// LDS bank conflicts: pixel records are 64 B, so the 16-B k-slot inside a record is XOR-swizzled with
// (pixel_col>>2)&3; the swizzle is applied on the *source* address of the LDS-DMA (LDS-DMA writes are
// lane-linear) and on the ds_read_b128 address -- same involution on both sides.
#include "srbh_wconv_host.h"

using namespace srbh;
using namespace srbh_k;

static int conv3x3_impl(const srbh_conv3x3_args* a, const int bf16, const void* mask16, const int mask_chunks_total, const int mask_chunk0,
                        void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const bool ext = bf16 || mask16;
    SRBH_REQUIRE(a != nullptr, "srbh_conv3x3_f16: null args");
    SRBH_REQUIRE(a->in && a->w, "srbh_conv3x3_f16: null input/weight pointer");
    SRBH_REQUIRE(a->cout == 32 || a->cout == 64, "srbh_conv3x3_f16: cout must be 32 or 64 (got %d)", a->cout);
    SRBH_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0, "srbh_conv3x3_f16: bad geometry B=%d H=%d W=%d", a->B, a->H, a->W);
    SRBH_REQUIRE(a->in_chunks >= 1 && a->in_chunk0 >= 0 && a->in_chunk0 + a->in_chunks <= a->in_chunks_total,
                 "srbh_conv3x3_f16: input chunk range [%d,+%d) outside %d planes", a->in_chunk0, a->in_chunks,
                 a->in_chunks_total);
    SRBH_REQUIRE(!a->upsample2x || (a->H % 2 == 0 && a->W % 2 == 0), "srbh_conv3x3_f16: upsample2x needs even H,W");
    SRBH_REQUIRE(a->out16 || a->out32, "srbh_conv3x3_f16: no output requested");
    SRBH_REQUIRE(!a->out16 || (a->out16_chunk0 >= 0 && a->out16_chunk0 + a->cout / 32 <= a->out16_chunks_total),
                 "srbh_conv3x3_f16: output chunk range outside buffer");
    SRBH_REQUIRE(!a->out32 || (a->out32_c >= 1 && a->out32_c <= a->cout), "srbh_conv3x3_f16: out32_c=%d invalid",
                 a->out32_c);
    SRBH_REQUIRE(!(a->res2 && !a->res1), "srbh_conv3x3_f16: res2 requires res1");
    SRBH_REQUIRE(!(a->res1 || a->res2 || a->skip) || a->cout == 64,
                 "srbh_conv3x3_f16: residual/skip epilogues need cout == 64");

    if (!ext) {   // many-tile 64 -> 64 convs (the up-sampler tail) have a persistent form, see srbh_ptail.hip
        int used = 0;
        const int rc = ptail_run(a, stream, &used);
        if (rc != SRBH_OK || used) return rc;
    }
    SRBH_REQUIRE(!a->out16_nhwc, "srbh_conv3x3_f16: out16_nhwc (dense fp16 NHWC output) exists for 64 -> 64 convs without residual / skip "
                                 "epilogue and without an fp32 output only (the persistent tail kernel)");
    SRBH_REQUIRE(!ext || !a->upsample2x, "srbh_conv3x3_x16: the gradient forms have no nearest-x2 read");
    SRBH_REQUIRE(!mask16 || (mask_chunk0 >= 0 && mask_chunk0 + a->cout / 32 <= mask_chunks_total), "srbh_conv3x3_x16: mask chunk range outside its buffer");

    KParams p{};
    conv_params_common(p, a, a->upsample2x ? a->H / 2 : a->H, a->upsample2x ? a->W / 2 : a->W);
    p.nblocks = p.tiles_per_img * a->B;
    p.lrelu = a->lrelu;
    p.res_scale = a->res_scale;
    p.res2_scale = a->res2_scale;
    p.res1 = a->res1;
    p.res2 = a->res2;
    p.skip = a->skip;
    p.res1_update = a->res1_update;
    p.res2_update = a->res2_update;
    plane_arg(p.mask16, p.mask_img_b, p.mask_plane_b, p.mask_row_b, mask16, a->B, mask_chunks_total, mask_chunk0, a->H, a->W);
    const int form = bf16 ? 1 + bf16 : a->upsample2x ? 1 : 0;      // (UPS, BF) = (0, 0), (1, 0), (0, 1), (0, 2)
    return with_const<4>(form, [&](auto f) {
        constexpr int UPS = decltype(f)::value == 1, BF = decltype(f)::value > 1 ? decltype(f)::value - 1 : 0;
        return a->cout == 64 ? launch<conv3x3_f16_kernel<2, UPS, 0, BF>, true>(dim3(p.nblocks), lds_bytes<2, UPS>(), stream, p)
                             : launch<conv3x3_f16_kernel<1, UPS, 0, BF>, true>(dim3(p.nblocks), lds_bytes<1, UPS>(), stream, p);
    });
}

extern "C" int srbh_conv3x3_f16(const srbh_conv3x3_args* a, void* stream) { return conv3x3_impl(a, 0, nullptr, 0, 0, stream); }

/* The same convolution for the GRADIENT side of the RRDBNet training path (SR/rrdbnet_arch.py:538-592 differentiates the generator):
 * bf16 != 0: the ACT16 input / output planes and the WPACK16 weights hold bf16 (srbh_pack_conv3x3_b16), products on
 * v_mfma_f32_32x32x16_bf16; mask16 != NULL: the output is multiplied by the LeakyReLU derivative taken from the SAVED fp16
 * activation plane(s) mask16[chunk mask_chunk0 ..] (post-activation > 0 ? 1 : 0.2), before the 16-bit / fp32 stores.
 * bf16 == 2: bf16 operands, the 16-bit output rounded to fp16 (the last conv5 of the bf16 inference trunk, conv3x3_trunk_b16(out_f16 = 1)). */
extern "C" int srbh_conv3x3_x16(const srbh_conv3x3_args* a, int bf16, const void* mask16, int mask_chunks_total, int mask_chunk0,
                                void* stream) {
    return conv3x3_impl(a, bf16 == 2 ? 2 : bf16 ? 1 : 0, mask16, mask_chunks_total, mask_chunk0, stream);
}

// ---- the wide form: 32..512 channels on either side, one launch per conv (include/srbh.h, srbh_wconv3x3) ---------------------------------
// The trunk's conv_tile (staging, swizzle, MFMA body, transposing epilogue) per (8 x 64 tile, 64-channel output slice); the slices of a tile
// are neighbours in the XCD-remapped grid order, so the input tile they all stage comes out of L2 after the first.  Every wait in the body
// is the full vmcnt(0) of conv_tile.
extern "C" int srbh_wconv3x3(const srbh_wconv3x3_args* a, void* stream) {
    static constexpr WideForm form = {"srbh_wconv3x3", 3, 0, true, true, true, false};
    if (const int rc = wide_validate(a, form)) return rc;
    const WKParams p = wide_params(a, form);
    return with_const<2>(a->bf16 != 0, [&](auto bf) {
        constexpr int BF = decltype(bf)::value;
        return a->cout == 32 ? launch<wconv3x3_kernel<1, BF>, true>(dim3(p.nblocks), lds_bytes<1, 0>(), (hipStream_t)stream, p)
                             : launch<wconv3x3_kernel<2, BF>, true>(dim3(p.nblocks), lds_bytes<2, 0>(), (hipStream_t)stream, p);
    });
}

int srbh::conv3x3_trunk_b16(const srbh_conv3x3_args* a, const int out_f16, void* stream) {
    return conv3x3_impl(a, out_f16 ? 2 : 1, nullptr, 0, 0, stream);
}
