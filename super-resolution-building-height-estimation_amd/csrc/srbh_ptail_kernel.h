// srbh_ptail_kernel.h -- what the persistent tail kernels ptail_kernel (srbh_ptail.hip, fp16 operands) and ptail_split_kernel
// (srbh_ptail_split.hip, split fp16 operands, "f16x2") share, each piece written once: the LDS-DMA instruction, the tile walk's origin, the
// 16-byte store of a 16-bit channel-group pair, the descriptors of the 16-bit planes they read and write with their host-side fillers, and
// the grid sizing.  Only pieces that leave both kernels' instruction streams as they were live here (profiles/ptail_shared_core_isa_compare.txt);
// the per-lane set-up, the staging loops and the 288-MFMA pass stay written out in each kernel: behind a function boundary their address
// arithmetic is optimised once more after inlining and comes out different.
#pragma once
#include <stdlib.h>
#include "srbh_conv3x3_kernel.h"

namespace srbh_k {

constexpr int TAIL_W_B = 2 * 36 * 1024;       // resident weights of both input chunks
template <int UPS>
constexpr int TAIL_LDS_B = TAIL_W_B + 2 * TileGeo<UPS>::UNITS * 16;   // [weights 72 KiB][input chunk 0][input chunk 1], the input tiles exact

// 16-bit planes a kernel reads: ACT16, the first of two consecutive chunk planes
struct In16 {
    const char* base;
    long img_b;
    int plane_b, row_b;
};
// 16-bit records a kernel writes.  ACT16: 64-byte pixel records behind a 1-pixel border, two chunk planes.  NHWC16
// (srbh_conv3x3_args::out16_nhwc): dense fp16 [B][H][W][C] records of pix_b bytes, no border, "plane" = 64 bytes (the next 32 channels).
struct Out16 {
    char* base;                 // nullptr: no such output
    long img_b;
    int plane_b, row_b, pix_b, border;
};


// 16 B per lane LDS-DMA under an explicit EXEC mask (see srbh_ptrunk.hip)
__device__ __forceinline__ void dma16(const char* gaddr, const unsigned lds_off_v, const unsigned long long mask) {
    unsigned long long sv;
    const unsigned lds_off = __builtin_amdgcn_readfirstlane(lds_off_v);
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %1\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %3, off\n\ts_mov_b64 exec, %0"
                 : "=&s"(sv) : "s"(mask), "s"(lds_off), "v"(gaddr) : "memory", "m0");
}

__device__ __forceinline__ void tile_origin(const int t, const int tiles_per_img, const int tiles_x, int& img, int& Y0, int& X0) {
    img = t / tiles_per_img;
    const int trem = t - img * tiles_per_img;
    const int ty = trem / tiles_x;
    Y0 = ty * TILE_H;
    X0 = (trem - ty * tiles_x) * TILE_W;
}

typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

// channel groups 2m and 2m + 1 of a pixel (MFMA D layout: 4 + 4 fp16 values per lane, two dwords each) -> after the half-wave swap every lane
// holds 8 consecutive channels of its pixel: the 16 bytes at m * 32 + hi * 16 of the pixel's record
__device__ __forceinline__ uintx4 pair16(const unsigned (&ga)[2], const unsigned (&gb)[2]) {
    auto s0 = __builtin_amdgcn_permlane32_swap(ga[0], gb[0], false, false);
    auto s1 = __builtin_amdgcn_permlane32_swap(ga[1], gb[1], false, false);
    return uintx4{s0[0], s1[0], s0[1], s1[1]};
}

// channel groups 2m and 2m + 1 of block mb of pixel (Y, X): one 16-byte store into the pixel's record
__device__ __forceinline__ void store16_pair(const Out16& o, const bool valid, const int img, const int mb, const int Y, const int X, const int m, const int hi,
                                             const unsigned (&ga)[2], const unsigned (&gb)[2]) {
    const uintx4 raw = pair16(ga, gb);
    if (valid)
        *(uintx4*)(o.base + (long)img * o.img_b + (long)mb * o.plane_b + (long)(Y + o.border) * o.row_b + (X + o.border) * o.pix_b + m * 32 + hi * 16) = raw;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// the two planes from chunk0 of the `chunks_total`-plane ACT16 buffer `buf` that conv `a` reads (behind the nearest-x2 read: at half size)
inline In16 tail_in16(const srbh_conv3x3_args* a, const void* buf, const int chunks_total, const int chunk0) {
    const Act16Geo g = act16_geo(a->B, chunks_total, a->upsample2x ? a->H / 2 : a->H, a->upsample2x ? a->W / 2 : a->W);
    return In16{(const char*)buf + (long)chunk0 * g.plane_b, g.img_b, g.plane_b, g.row_b};
}

// the 16-bit output of conv `a` in `buf` (nullptr: none), ACT16 planes or NHWC16 records as a->out16_nhwc says, from chunk0 of chunks_total
inline Out16 tail_out16(const srbh_conv3x3_args* a, void* buf, const int chunks_total, const int chunk0) {
    if (!buf) return Out16{};
    if (a->out16_nhwc) {
        const int C = chunks_total * 32;
        return Out16{(char*)buf + (long)chunk0 * 64, (long)a->H * a->W * C * 2, 64, a->W * C * 2, C * 2, 0};
    }
    const Act16Geo g = act16_geo(a->B, chunks_total, a->H, a->W);
    return Out16{(char*)buf + (long)chunk0 * g.plane_b, g.img_b, g.plane_b, g.row_b, PIX_B, 1};
}

// ntiles tiles over at most one workgroup per CU, each walking a contiguous range.  Fewer workgroups than CUs on request: a workgroup of
// these kernels holds a whole CU's LDS for its entire walk, so a full grid lets no kernel of another stream in while it runs
// (srbh_ptail_wgs_cap, the harness knob, like SRBH_PT_IMAGES).
inline int tail_grid(const int ntiles, int* tiles_per_wg, int* grid) {
    static int ncu_of[64] = {0};   // CU count per device (queried once each)
    int dev = 0;
    SRBH_HIP(hipGetDevice(&dev));
    if (!ncu_of[dev & 63]) SRBH_HIP(hipDeviceGetAttribute(&ncu_of[dev & 63], hipDeviceAttributeMultiprocessorCount, dev));
    int ncu = ncu_of[dev & 63];
    const int cap = ptail_wgs_cap();
    if (cap > 0 && cap < ncu) ncu = cap;
    if (const char* we = getenv("SRBH_PTAIL_WGS")) {          // (developer A/B aid: overrides the caller's cap)
        const int ecap = atoi(we);
        if (ecap > 0 && ecap < ncu_of[dev & 63]) ncu = ecap;
    }
    const int nwg = ntiles < ncu ? ntiles : ncu;
    *tiles_per_wg = (ntiles + nwg - 1) / nwg;
    *grid = (ntiles + *tiles_per_wg - 1) / *tiles_per_wg;
    return SRBH_OK;
}

}  // namespace srbh_k
