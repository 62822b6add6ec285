// srbh_ptail_split.hip -- the 64 -> 64 channel 3x3 convs behind the trunk (conv_body, conv_up1, conv_up2, conv_hr; reference
// SR/rrdbnet_arch.py:234-239) on SPLIT fp16 operands: the "f16x2" precision mode.
//
// Every fp32 value v travels as two fp16 numbers, hi = rne16(v) and lo' = rne16((v - hi) * 2^11); weights are split the same way when
// they are packed.  A conv is three matrix products on the fp16 matrix cores with fp32 accumulation,
//     C = sum (w_hi * a_lo' + w_lo' * a_hi)      M = sum w_hi * a_hi      y = M + C * 2^-11 + bias
// (lo x lo dropped), then the usual epilogue, then the fp32 result is split again for the next conv.  The 2^11 scale keeps the low parts
// normal fp16 numbers (unscaled, 98 % of the weights' low parts are fp16 subnormals), so nothing hangs on how the MFMA treats those.
//
// Schedule.  The persistent fp16 form (srbh_ptail.hip) keeps 72 KiB of weights and both input chunks of a tile (2 x 42 KiB) in LDS; two
// weight sets and four input chunks do not fit.  Here the LDS holds ONE weight set and ONE pair of input chunks at a time and a tile is three
// passes of srbh_ptail.hip's barrier-free 288-MFMA loop over the same accumulators:
//     pass 0:  w_hi  x a_lo'         (w_hi is still resident from the previous tile; a_lo' was requested under its epilogue)
//     pass 1:  w_lo' x a_hi          then the accumulators (= C) are multiplied by 2^-11 once
//     pass 2:  w_hi  x a_hi          M on top; a_hi stays where pass 1 put it, only the weights are re-staged
// i.e. per tile 144 KiB of weights (L2 hits: every workgroup reads the same two packs) and 168 KiB of input go through the LDS-DMA, each
// behind a full wait + barrier.  Every wait is s_waitcnt vmcnt(0): no counted waits, so none of their hazards.
// A workgroup walks a contiguous range of tiles; a launch with fewer tiles than CUs (conv_body at B x 64 x 64) runs one tile per workgroup.
#include "srbh_ptail_kernel.h"

namespace {
using namespace srbh;
using namespace srbh_k;

struct SParams {
    const char* in_hi;          // first hi plane (ACT16)
    const char* in_lo;          // first lo' plane
    long in_hi_img_b, in_lo_img_b;
    int in_plane_b, in_row_b;   // same plane geometry for both
    const char* w_hi;           // WPACK16, 2 chunks x 36 KiB
    const char* w_lo;
    const float* bias;
    const float* skip;          // fp32 NHWC (64 channels) added before the activation, or nullptr
    int H, W;                   // OUTPUT geometry
    int tiles_x, tiles_per_img, ntiles, tiles_per_wg;
    int lrelu;
    char* out_hi;               // ACT16 hi planes, or the dense fp16 NHWC tensor (nhwc), or nullptr
    char* out_lo;               // ACT16 lo' planes or nullptr (nhwc: none -- the hand-off is rne16(y))
    long out_hi_img_b, out_lo_img_b;
    int out_plane_b, out_row_b, out_pix_b, out_border;
    float* out32;               // fp32 NHWC (64 channels) output or nullptr
};

constexpr float LO_SCALE = 2048.f, LO_UNSCALE = 1.f / 2048.f;

template <int UPS>
__global__ __launch_bounds__(256, 1) void ptail_split_kernel(const SParams p) {
    using G = TileGeo<UPS>;
    constexpr int IN_EX = G::UNITS * 16;
    constexpr int CB = 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [weights 72 KiB][input chunk 0][input chunk 1]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;

    int goff[G::NJ];
#pragma unroll
    for (int j = 0; j < G::NJ; ++j) {
        const int u0 = j * 256 + tid;
        const int u = u0 < G::UNITS ? u0 : 0;
        const int trow = u / (G::COLS * 4);
        const int rem = u - trow * (G::COLS * 4);
        const int pc = rem >> 2, ps = rem & 3;
        goff[j] = trow * p.in_row_b + pc * PIX_B + ((ps ^ ((pc >> 2) & 3)) << 4);
    }
    const unsigned long long tail_mask = __builtin_amdgcn_ballot_w64((G::NJ - 1) * 256 + tid < G::UNITS);
    int aoff[3][2];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
        const int pc = UPS ? (((wc * 32 + l31 + dx - 1) >> 1) + 1) : (wc * 32 + l31 + dx);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            aoff[dx][ks] = wr * (UPS ? 2 : 4) * G::ROW_B + pc * PIX_B + (((ks * 2 + hi) ^ ((pc >> 2) & 3)) << 4);
    }

    auto stage_inputs = [&](int t, const char* base, long img_b) {
        int img, Y0, X0;
        tile_origin(t, p.tiles_per_img, p.tiles_x, img, Y0, X0);
        const char* src0 = base + (long)img * img_b + (long)(UPS ? (Y0 >> 1) : Y0) * p.in_row_b + (UPS ? (X0 >> 1) : X0) * PIX_B;
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int j = 0; j < G::NJ; ++j)
                dma16(src0 + (long)c * p.in_plane_b + goff[j], TAIL_W_B + c * IN_EX + (j * 256 + wave * 64) * 16,
                      j < G::NJ - 1 ? ~0ull : tail_mask);
    };
    auto stage_weights = [&](const char* w) {     // 72 fragments of 1 KiB, 18 per wave
#pragma unroll
        for (int k = 0; k < 18; ++k) dma16(w + (wave + 4 * k) * 1024 + lane * 16, (wave + 4 * k) * 1024, ~0ull);
    };

    const Out16 out_hi{p.out_hi, p.out_hi_img_b, p.out_plane_b, p.out_row_b, p.out_pix_b, p.out_border};
    const Out16 out_lo{p.out_lo, p.out_lo_img_b, p.out_plane_b, p.out_row_b, p.out_pix_b, p.out_border};
    const int t0 = blockIdx.x * p.tiles_per_wg;
    const int t1 = (t0 + p.tiles_per_wg < p.ntiles) ? t0 + p.tiles_per_wg : p.ntiles;
    if (t0 >= t1) return;
    stage_weights(p.w_hi);
    stage_inputs(t0, p.in_lo, p.in_lo_img_b);
    floatx4 bias4[CB][4];
#pragma unroll
    for (int mb = 0; mb < CB; ++mb)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            bias4[mb][g] = p.bias ? *(const floatx4*)(p.bias + mb * 32 + g * 8 + hi * 4) : floatx4{0.f, 0.f, 0.f, 0.f};

    for (int t = t0; t < t1; ++t) {
        int img, Y0, X0;
        tile_origin(t, p.tiles_per_img, p.tiles_x, img, Y0, X0);
        floatx16 acc[CB][4];
#pragma unroll
        for (int mb = 0; mb < CB; ++mb)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mb][i][r] = 0.f;
        constexpr int NREAD = G::NP + 3 * CB, NMFMA = 12 * CB;
        // the three passes are unrolled: straight-line code, the accumulators never cross a loop edge (as a runtime loop the kernel spilled)
#pragma unroll
        for (int pass = 0; pass < 3; ++pass) {
            if (pass == 1) {          // (behind the barrier that closed pass 0: nobody reads the LDS any more)
                stage_weights(p.w_lo);
                stage_inputs(t, p.in_hi, p.in_hi_img_b);
            } else if (pass == 2) {
                stage_weights(p.w_hi);
#pragma unroll
                for (int mb = 0; mb < CB; ++mb)      // C -> C * 2^-11, once, while the weights fly
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[mb][i] *= LO_UNSCALE;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // this pass's operands landed (and the previous tile's stores are out) ...
            __syncthreads();                                    // ... on every wave
            __builtin_amdgcn_sched_barrier(0);                  // (one scheduling region per pass: the compile time of the group pipeline below grows faster than its length)
            half8 P[2][G::NP];
            half8 A[2][3][CB];
            auto load_group = [&](int q, int set) {   // q = chunk * 6 + (ks * 3 + dx)
                const int c = q / 6, g = q - c * 6;
                const int ks = g / 3, dx = g - ks * 3;
                const char* sbi = smem + TAIL_W_B + c * IN_EX;
                const char* sbw = smem + c * (36 * 1024) + lane * 16;
#pragma unroll
                for (int r = 0; r < G::NP; ++r) P[set][r] = *(const half8*)(sbi + aoff[dx][ks] + r * G::ROW_B);
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int mb = 0; mb < CB; ++mb)
                        A[set][dy][mb] = *(const half8*)(sbw + ((((dy * 3 + dx) * 2 + ks) * CB + mb) << 10));
            };
            load_group(0, 0);
#pragma unroll
            for (int q = 0; q < 12; ++q) {
                if (q + 1 < 12) load_group(q + 1, (q + 1) & 1);
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int pr = UPS ? (((i + dy - 1) >> 1) + 1) : (i + dy);
#pragma unroll
                        for (int mb = 0; mb < CB; ++mb)
                            acc[mb][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[q & 1][dy][mb], P[q & 1][pr], acc[mb][i], 0, 0, 0);
                    }
                if (q == 0) __builtin_amdgcn_sched_group_barrier(0x100, NREAD, 0);
                if (q + 1 < 12) {
#pragma unroll
                    for (int k = 0; k < NREAD; ++k) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    }
                    __builtin_amdgcn_sched_group_barrier(0x008, NMFMA - NREAD, 0);
                } else {
                    __builtin_amdgcn_sched_group_barrier(0x008, NMFMA, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();                       // every wave is done reading this pass's operands
        }
        // w_hi stays for the next tile's pass 0; its lo' planes fly under this tile's epilogue
        if (t + 1 < t1) stage_inputs(t + 1, p.in_lo, p.in_lo_img_b);

        // ---- epilogue, straight from the MFMA D layout: lane (l31, hi) holds for row i and channel group g the 4
        // consecutive channels 8g + 4hi + (0..3) of pixel l31
        const int X = X0 + wc * 32 + l31;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int Y = Y0 + wr * 4 + i;
            const bool valid = (Y < p.H) && (X < p.W);
            const long pix = ((long)img * p.H + Y) * p.W + X;
#pragma unroll
            for (int mb = 0; mb < CB; ++mb) {
                unsigned hp[4][2], lp[4][2];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    floatx4 v;
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = acc[mb][i][g * 4 + q];
                    v += bias4[mb][g];
                    if (p.skip && valid) v += *(const floatx4*)(p.skip + pix * 64 + mb * 32 + g * 8 + hi * 4);
                    if (p.lrelu) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) v[q] = v[q] >= 0.f ? v[q] : v[q] * 0.2f;
                    }
                    if (p.out32 && valid) *(floatx4*)(p.out32 + pix * 64 + mb * 32 + g * 8 + hi * 4) = v;
                    half4 h4, l4;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        h4[q] = (_Float16)v[q];
                        l4[q] = (_Float16)((v[q] - (float)h4[q]) * LO_SCALE);
                    }
                    const uint2 u = __builtin_bit_cast(uint2, h4), ul = __builtin_bit_cast(uint2, l4);
                    hp[g][0] = u.x;
                    hp[g][1] = u.y;
                    lp[g][0] = ul.x;
                    lp[g][1] = ul.y;
                }
                if (p.out_hi) {
#pragma unroll
                    for (int m = 0; m < 2; ++m) store16_pair(out_hi, valid, img, mb, Y, X, m, hi, hp[2 * m], hp[2 * m + 1]);
                }
                if (p.out_lo) {
#pragma unroll
                    for (int m = 0; m < 2; ++m) store16_pair(out_lo, valid, img, mb, Y, X, m, hi, lp[2 * m], lp[2 * m + 1]);
                }
            }
        }
    }
}

// lo' planes of conv_body's input: lo' = rne16((v - hi) * 2^11) from the trunk's fp32 output stream v and the fp16 planes hi the trunk wrote.
// One thread per (pixel, 8-channel octet).  fragment != 0: v is in the persistent trunk kernel's order (W == 64; per image row float4 number
// wc * 512 + mb * 256 + g * 64 + lane = channels mb * 32 + g * 8 + (lane >> 5) * 4 .. + 3 of pixel wc * 32 + (lane & 31), as
// trunk_out_pixel_order_kernel in srbh_rrdbnet.hip undoes it); else NHWC.
__global__ __launch_bounds__(256) void split_lo_kernel(const float* __restrict__ v, const int fragment, const char* __restrict__ hi_planes,
                                                       char* __restrict__ lo_planes, const long hi_img_b, const long lo_img_b, const int plane_b,
                                                       const int row_b, const int B, const int H, const int W) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * H * W * 8) return;
    const int o8 = (int)(idx & 7);
    long r = idx >> 3;
    const int x = (int)(r % W);
    r /= W;                               // r = b * H + y
    const int y = (int)(r % H), b = (int)(r / H);
    floatx4 a0, a1;
    if (fragment) {
        const floatx4* s = (const floatx4*)v + r * 1024 + (x >> 5) * 512 + (o8 >> 2) * 256 + (o8 & 3) * 64 + (x & 31);
        a0 = s[0];
        a1 = s[32];
    } else {
        const floatx4* s = (const floatx4*)(v + (r * W + x) * 64 + o8 * 8);
        a0 = s[0];
        a1 = s[1];
    }
    const long off = (long)(o8 >> 2) * plane_b + (long)(y + 1) * row_b + (x + 1) * PIX_B + (o8 & 3) * 16;
    const half8 h = *(const half8*)(hi_planes + b * hi_img_b + off);
    half8 l;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        l[q] = (_Float16)((a0[q] - (float)h[q]) * LO_SCALE);
        l[4 + q] = (_Float16)((a1[q] - (float)h[4 + q]) * LO_SCALE);
    }
    *(half8*)(lo_planes + b * lo_img_b + off) = l;
}

template <int UPS>
int launch(const SParams& p0, hipStream_t stream) {
    constexpr int LDS_B = TAIL_LDS_B<UPS>;
    static_assert(LDS_B <= 163840, "one weight set + one pair of input chunks must fit the 160 KiB LDS");
    SRBH_ONCE_PER_DEVICE(SRBH_HIP(hipFuncSetAttribute((const void*)ptail_split_kernel<UPS>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_B)));
    SParams p = p0;
    int grid = 0;
    if (const int rc = tail_grid(p.ntiles, &p.tiles_per_wg, &grid)) return rc;      // (the caller's srbh_ptail_wgs_cap holds here too)
    hipLaunchKernelGGL(ptail_split_kernel<UPS>, dim3(grid), dim3(256), LDS_B, stream, p);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

}  // namespace

extern "C" int srbh_conv3x3_f16x2(const srbh_conv3x3_args* a, const srbh_conv3x3_split* s, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SRBH_REQUIRE(a && s, "srbh_conv3x3_f16x2: null args");
    SRBH_REQUIRE(a->in && a->w && s->in_lo && s->w_lo, "srbh_conv3x3_f16x2: null input / weight pointer (hi and lo' of both are needed)");
    SRBH_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0, "srbh_conv3x3_f16x2: bad geometry B=%d H=%d W=%d", a->B, a->H, a->W);
    SRBH_REQUIRE(a->cout == 64 && a->in_chunks == 2, "srbh_conv3x3_f16x2: 64 -> 64 channel convs only (cout=%d, in_chunks=%d)", a->cout, a->in_chunks);
    SRBH_REQUIRE(!a->res1 && !a->res2, "srbh_conv3x3_f16x2: no residual epilogue (skip only)");
    SRBH_REQUIRE(a->in_chunk0 >= 0 && a->in_chunk0 + 2 <= a->in_chunks_total && s->in_lo_chunk0 >= 0 && s->in_lo_chunk0 + 2 <= s->in_lo_chunks_total,
                 "srbh_conv3x3_f16x2: input chunk range outside its buffer");
    SRBH_REQUIRE(!a->upsample2x || (a->H % 2 == 0 && a->W % 2 == 0), "srbh_conv3x3_f16x2: upsample2x needs even H,W");
    SRBH_REQUIRE(a->out16 || a->out32, "srbh_conv3x3_f16x2: no output requested");
    SRBH_REQUIRE(!a->out32 || a->out32_c == 64, "srbh_conv3x3_f16x2: out32_c must be 64");
    SRBH_REQUIRE(!a->out16 || (a->out16_chunk0 >= 0 && a->out16_chunk0 + 2 <= a->out16_chunks_total), "srbh_conv3x3_f16x2: output chunk range outside buffer");
    SRBH_REQUIRE(!a->out16 || a->out16_nhwc || (s->out16_lo && s->out16_lo_chunk0 >= 0 && s->out16_lo_chunk0 + 2 <= s->out16_lo_chunks_total),
                 "srbh_conv3x3_f16x2: an ACT16 output needs its lo' planes (out16_lo)");
    SRBH_REQUIRE(!a->out16_nhwc || (a->out16 && !a->out32), "srbh_conv3x3_f16x2: out16_nhwc excludes an fp32 output");
    const int tiles_x = (a->W + TILE_W - 1) / TILE_W, tiles_y = (a->H + TILE_H - 1) / TILE_H;
    const In16 ih = tail_in16(a, a->in, a->in_chunks_total, a->in_chunk0), il = tail_in16(a, s->in_lo, s->in_lo_chunks_total, s->in_lo_chunk0);
    SParams p{};
    p.in_hi = ih.base;
    p.in_lo = il.base;
    p.in_hi_img_b = ih.img_b;
    p.in_lo_img_b = il.img_b;
    p.in_plane_b = ih.plane_b;
    p.in_row_b = ih.row_b;
    p.w_hi = (const char*)a->w;
    p.w_lo = (const char*)s->w_lo;
    p.bias = a->bias;
    p.skip = a->skip;
    p.H = a->H;
    p.W = a->W;
    p.tiles_x = tiles_x;
    p.tiles_per_img = tiles_x * tiles_y;
    p.ntiles = p.tiles_per_img * a->B;
    p.lrelu = a->lrelu;
    const Out16 oh = tail_out16(a, a->out16, a->out16_chunks_total, a->out16_chunk0);
    p.out_hi = oh.base;
    p.out_hi_img_b = oh.img_b;
    p.out_plane_b = oh.plane_b;
    p.out_row_b = oh.row_b;
    p.out_pix_b = oh.pix_b;
    p.out_border = oh.border;
    if (a->out16 && !a->out16_nhwc) {
        const Out16 ol = tail_out16(a, s->out16_lo, s->out16_lo_chunks_total, s->out16_lo_chunk0);
        p.out_lo = ol.base;
        p.out_lo_img_b = ol.img_b;
    }
    p.out32 = a->out32;
    return a->upsample2x ? launch<1>(p, stream) : launch<0>(p, stream);
}

extern "C" int srbh_act16_split_lo(const float* v, int fragment_order, const void* hi, int hi_chunks_total, int hi_chunk0, void* lo, int lo_chunks_total,
                                   int lo_chunk0, int B, int H, int W, void* stream) {
    SRBH_REQUIRE(v && hi && lo && B > 0 && H > 0 && W > 0, "srbh_act16_split_lo: bad arguments");
    SRBH_REQUIRE(hi_chunk0 >= 0 && hi_chunk0 + 2 <= hi_chunks_total && lo_chunk0 >= 0 && lo_chunk0 + 2 <= lo_chunks_total,
                 "srbh_act16_split_lo: chunk range outside its buffer");
    SRBH_REQUIRE(!fragment_order || W == TILE_W, "srbh_act16_split_lo: the fragment order exists for 64-pixel-wide images only (W=%d)", W);
    const Act16Geo gh = act16_geo(B, hi_chunks_total, H, W), gl = act16_geo(B, lo_chunks_total, H, W);
    const long total = (long)B * H * W * 8;
    hipLaunchKernelGGL(split_lo_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v, fragment_order,
                       (const char*)hi + (long)hi_chunk0 * gh.plane_b, (char*)lo + (long)lo_chunk0 * gl.plane_b, gh.img_b, gl.img_b, gh.plane_b, gh.row_b,
                       B, H, W);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
