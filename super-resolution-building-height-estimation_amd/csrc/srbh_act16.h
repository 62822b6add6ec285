// srbh_act16.h -- what the plane kernels around the wide convs share (srbh_vgg.hip, srbh_disc.hip, srbh_disc3.hip; the pack kernels of
// srbh_aux.hip): the geometry of a chunk-plane buffer as a kernel argument, the address of a record in it, one-thread-per-unit launch sizes,
// the 8-value roundings and loads of the staging kernels and the index decode of a WPACK16 element.  Not part of the C ABI.
#pragma once
#include "srbh_internal.h"

namespace srbh {

struct PlaneGeo {
    int row_b, plane_b;
    long img_b;
};
inline PlaneGeo plane_geo(int B, int chunks, int H, int W) {
    const Act16Geo g = act16_geo(B, chunks, H, W);
    return PlaneGeo{g.row_b, g.plane_b, g.img_b};
}
// one thread per unit, 256 per workgroup
inline unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }
inline bool fits(long units) { return units > 0 && units < (1l << 31) * 256; }

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
typedef unsigned uint4w __attribute__((ext_vector_type(4)));

// byte offset of octet `oct` (8 channels, 16 bytes) of the record of interior pixel (y, x) in chunk plane `ch` of image b
__device__ __forceinline__ long rec_off(const PlaneGeo& g, int b, int ch, int y, int x, int oct) {
    return (long)b * g.img_b + (long)ch * g.plane_b + (long)(y + 1) * g.row_b + (x + 1) * PIX_B + oct * 16;
}

// 8 fp32 -> 8 x 16 bit (RNE), fp16 or bf16
template <int BF>
__device__ __forceinline__ uint4w round8(const float (&v)[8]) {
    if constexpr (BF) {
        return uint4w{bf16x2_rne(v[0], v[1]), bf16x2_rne(v[2], v[3]), bf16x2_rne(v[4], v[5]), bf16x2_rne(v[6], v[7])};
    } else {
        typedef _Float16 h8 __attribute__((ext_vector_type(8)));
        h8 h;
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = (_Float16)v[j];
        return __builtin_bit_cast(uint4w, h);
    }
}

// octet o8 of pixel (y, xx) of an fp32 NHWC (B, H, W, C) tensor as two 16-byte loads; eight zeros for a pixel outside the image
__device__ __forceinline__ void load8_or_zero(const float* x, int H, int W, int C, int b, int y, int xx, int o8, float (&val)[8]) {
    typedef float f4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int j = 0; j < 8; ++j) val[j] = 0.f;
    if (y >= 0 && y < H && xx >= 0 && xx < W) {
        const float* s = x + (((long)b * H + y) * W + xx) * C + o8 * 8;
        const f4 a0 = *(const f4*)s, a1 = *(const f4*)(s + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { val[j] = a0[j]; val[4 + j] = a1[j]; }
    }
}

// element idx of a WPACK16 pack [chunk][tap][k-step][mb][lane][8] of nmb 32-channel output blocks and ntaps taps -> the weight it holds:
// output channel, input channel, tap
struct WpackElem {
    int oc, ic, tap;
};
__device__ __forceinline__ WpackElem wpack_decode(long idx, int nmb, int ntaps) {
    const int j = (int)(idx & 7), lane = (int)((idx >> 3) & 63);
    unsigned long f = (unsigned long)idx >> 9;      // (idx >= 0, nmb > 0: unsigned division is the shorter sequence)
    const int mb = (int)(f % (unsigned)nmb); f /= (unsigned)nmb;
    const int ks = (int)(f & 1); f >>= 1;
    const int tap = (int)(f % (unsigned)ntaps), chunk = (int)(f / (unsigned)ntaps);
    return WpackElem{mb * 32 + (lane & 31), chunk * 32 + ks * 16 + (lane >> 5) * 8 + j, tap};
}
// one weight -> its 16-bit slot: fp16, or bf16 by the integer RNE sequence (not bf16x2_rne: the packs keep their bits for every input)
__device__ __forceinline__ unsigned short to16(float v, int bf) {
    if (bf) {
        const unsigned u = __builtin_bit_cast(unsigned, v);
        return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
    const _Float16 h = (_Float16)v;
    return __builtin_bit_cast(unsigned short, h);
}
#endif
}  // namespace srbh
