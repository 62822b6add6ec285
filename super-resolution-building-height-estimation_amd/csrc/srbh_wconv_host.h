// srbh_wconv_host.h -- host path of the conv_tile entry points (srbh_conv3x3_kernel.h): the parameter fields srbh_conv3x3_f16 / _x16 and the
// wide entry points fill alike, and for the three wide forms (srbh_wconv3x3, srbh_wconv2x2, srbh_wconv3x3_lrelu) one description, one argument
// check and one WKParams filler.  An entry point is: form, wide_validate, wide_params, launch<kernel form, true>.
#pragma once
#include "srbh_conv3x3_kernel.h"

namespace srbh_k {

// chunk planes chunk0.. of a `chunks_total`-plane ACT16 buffer with interior H x W as a kernel argument (pointer + three strides); a null
// buffer leaves the zeros of the zero-initialised parameter struct
template <class Ptr>
inline void plane_arg(Ptr& ptr, long& img_b, int& plane_b, int& row_b, const void* base, int B, int chunks_total, int chunk0, int H, int W) {
    if (!base) return;
    const Act16Geo g = act16_geo(B, chunks_total, H, W);
    ptr = (Ptr)((const char*)base + (long)chunk0 * g.plane_b);
    img_b = g.img_b;
    plane_b = g.plane_b;
    row_b = g.row_b;
}

// The KParams fields that srbh_conv3x3_args and srbh_wconv3x3_args name alike: input planes (interior inH x inW), weights, bias, the tile grid
// of the H x W output and both outputs.  p is zero-initialised (KParams p{} / WKParams p{}): what a caller does not set stays 0 / null.
template <class P, class A>
inline void conv_params_common(P& p, const A* a, int inH, int inW) {
    plane_arg(p.in, p.in_img_b, p.in_plane_b, p.in_row_b, a->in, a->B, a->in_chunks_total, a->in_chunk0, inH, inW);
    p.nchunk = a->in_chunks;
    p.w = (const char*)a->w;
    p.bias = a->bias;
    p.H = a->H;
    p.W = a->W;
    p.tiles_x = (a->W + TILE_W - 1) / TILE_W;
    p.tiles_per_img = p.tiles_x * ((a->H + TILE_H - 1) / TILE_H);
    plane_arg(p.out16, p.out16_img_b, p.out16_plane_b, p.out16_row_b, a->out16, a->B, a->out16_chunks_total, a->out16_chunk0, a->H, a->W);
    p.out32 = a->out32;
    p.out32_c = a->out32_c;
}

// One wide entry point: what it takes of srbh_wconv3x3_args.
struct WideForm {
    const char* name;   // in front of every error text
    int taps;           // per axis: 3, or 2 (the VALID form: conv_tile<.., T2 = 1>)
    int grow;           // the input interior is (H + grow) x (W + grow)
    bool cout32;        // cout == 32 allowed (else multiples of 64 only)
    bool epilogue;      // bias / relu / mask16 / add16 allowed
    bool out16;         // out16 allowed
    bool out32_all;     // out32 required, with out32_c == cout
};

// The checks of a wide entry point in the order it has always made them, the texts as they were (spacing included: callers match them).
inline int wide_validate(const srbh_wconv3x3_args* a, const WideForm& f) {
    SRBH_REQUIRE(a != nullptr, "%s: null args", f.name);
    if (f.out32_all) SRBH_REQUIRE(a->in && a->w && a->out32, "%s: null input / weight / out32 pointer", f.name);
    else SRBH_REQUIRE(a->in && a->w, f.epilogue ? "%s: null input/weight pointer" : "%s: null input / weight pointer", f.name);
    if (f.cout32) SRBH_REQUIRE(a->cout == 32 || (a->cout >= 64 && a->cout % 64 == 0), "%s: cout must be 32 or a multiple of 64 (got %d)", f.name, a->cout);
    else SRBH_REQUIRE(a->cout >= 64 && a->cout % 64 == 0, "%s: cout must be a multiple of 64 (got %d)", f.name, a->cout);
    SRBH_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0, "%s: bad geometry B=%d H=%d W=%d", f.name, a->B, a->H, a->W);
    SRBH_REQUIRE(a->in_chunks >= 1 && a->in_chunk0 >= 0 && a->in_chunk0 + a->in_chunks <= a->in_chunks_total,
                 "%s: input chunk range [%d,+%d) outside %d planes", f.name, a->in_chunk0, a->in_chunks, a->in_chunks_total);
    if (!f.epilogue)
        SRBH_REQUIRE(!a->bias && !a->relu && !a->mask16 && !a->add16 && (f.out16 || !a->out16),
                     f.out16 ? "%s: no bias / relu / mask16 / add16 in this form" : "%s: no bias / relu / mask16 / add16 / out16 in this form", f.name);
    const int nmb = a->cout / 32;
    if (f.out32_all) {
        SRBH_REQUIRE(a->out32_c == a->cout, "%s: out32_c=%d must equal cout=%d", f.name, a->out32_c, a->cout);
    } else {
        SRBH_REQUIRE(a->out16 || a->out32, "%s: no output requested", f.name);
        SRBH_REQUIRE(!a->out16 || (a->out16_chunk0 >= 0 && a->out16_chunk0 + nmb <= a->out16_chunks_total), "%s: output chunk range outside its buffer", f.name);
        SRBH_REQUIRE(!a->mask16 || (a->mask_chunk0 >= 0 && a->mask_chunk0 + nmb <= a->mask_chunks_total), "%s: mask chunk range outside its buffer", f.name);
        SRBH_REQUIRE(!a->add16 || (a->add_chunk0 >= 0 && a->add_chunk0 + nmb <= a->add_chunks_total), "%s: addend chunk range outside its buffer", f.name);
        SRBH_REQUIRE(!a->out32 || (a->out32_c >= 1 && a->out32_c <= a->cout), "%s: out32_c=%d invalid", f.name, a->out32_c);
    }
    const long tiles = (long)((a->W + TILE_W - 1) / TILE_W) * ((a->H + TILE_H - 1) / TILE_H) * a->B;
    SRBH_REQUIRE(tiles * (nmb / (a->cout == 32 ? 1 : 2)) < (1l << 30), "%s: too many workgroups", f.name);
    return SRBH_OK;
}

// The kernel parameters of validated arguments: one workgroup per (tile, output slice of 64 channels, or the 32 of cout == 32).
inline WKParams wide_params(const srbh_wconv3x3_args* a, const WideForm& f) {
    WKParams p{};
    conv_params_common(p, a, a->H + f.grow, a->W + f.grow);
    const int nmb = a->cout / 32;
    p.nslice = nmb / (a->cout == 32 ? 1 : 2);
    p.nblocks = p.tiles_per_img * a->B * p.nslice;
    plane_arg(p.mask16, p.mask_img_b, p.mask_plane_b, p.mask_row_b, a->mask16, a->B, a->mask_chunks_total, a->mask_chunk0, a->H, a->W);
    plane_arg(p.add16, p.add_img_b, p.add_plane_b, p.add_row_b, a->add16, a->B, a->add_chunks_total, a->add_chunk0, a->H, a->W);
    p.w_nmb = nmb;
    p.w_chunk_b = 2 * f.taps * f.taps * 1024 * nmb;      // 18 or 8 KiB per 32 output channels
    p.relu = a->relu;
    return p;
}

}  // namespace srbh_k
