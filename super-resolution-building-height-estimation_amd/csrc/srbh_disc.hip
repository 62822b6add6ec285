// srbh_disc.hip -- the discriminator's 4x4 / stride 2 / pad 1 convolutions (reference SR/rrdbnet_arch.py:262-264, used at :277-279) as
// 2x2-tap VALID convolutions over the space-to-depth image of the zero-padded input.  With xpad = x in a zero ring of 1:
//     S[(2p+q) C + c][u][v]  = xpad[c][2u+p][2v+q]                 4C channels, (H/2+1) x (W/2+1)
//     W2[o][(2p+q) C + c][a][b] = w[o][c][2a+p][2b+q]              a, b in {0, 1}
//     y[o][i][j]  = sum_{k,a,b} W2[o][k][a][b] S[k][i+a][j+b]
//     dS[k][u][v] = sum_{o,a,b} Wt[k][o][a][b] gpad[o][u+a][v+b]   Wt[k][o][a][b] = W2[o][k][1-a][1-b], gpad = g in a zero ring of 1
//     dx = depth-to-space(dS), ring cropped
//     dW2[o][k][a][b] = sum_{n,i,j} g[n][o][i][j] S[n][k][i+a][j+b]
// No tap is wasted and no operand read is strided.  This file holds the plane staging (space-to-depth, framed gradient), the two weight packs,
// depth-to-space, the entry point of the 2x2-tap form of the wide conv kernel (conv_tile<.., T2 = 1>, srbh_conv3x3_kernel.h) and the weight
// gradient (a GEMM over pixels on v_mfma_f32_16x16x16_bf16, the construction of hwgrad_b16_kernel with two taps per axis and no halo).
// Arithmetic contract: include/srbh.h, DESIGN.md 4.  No atomics anywhere: every result is bit-reproducible.
#include "srbh_act16.h"
#include "srbh_wconv_host.h"

namespace {
using namespace srbh;
using namespace srbh_k;

typedef unsigned uint2w __attribute__((ext_vector_type(2)));
typedef short short4w __attribute__((ext_vector_type(4)));

// ---- space-to-depth staging: fp32 NHWC (B, H, W, C) -> the planes of S.  One thread per (b, phase, u, v, octet): every record of the interior
// is written, the pad-derived zeros (row 0 of the phases p = 0, row H/2 of p = 1, likewise the columns) included.
template <int BF>
__global__ __launch_bounds__(256) void s2d_kernel(const float* __restrict__ x, char* planes, int B, int C, int H, int W, PlaneGeo g) {
    const int Hs = H / 2 + 1, Ws = W / 2 + 1, oct = C / 8;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * 4 * Hs * Ws * oct) return;
    const int o8 = (int)(idx % oct);
    long r = idx / oct;
    const int v = (int)(r % Ws); r /= Ws;
    const int u = (int)(r % Hs); r /= Hs;
    const int ph = (int)(r & 3), b = (int)(r >> 2);
    const int y = 2 * u + (ph >> 1) - 1, xx = 2 * v + (ph & 1) - 1;
    float val[8];
    load8_or_zero(x, H, W, C, b, y, xx, o8, val);
    // (rec_off written out: through the helper the sum is associated differently and this kernel takes 20 VGPRs for 18)
    char* o = planes + (long)b * g.img_b + (long)(ph * (C / 32) + (o8 >> 2)) * g.plane_b + (long)(u + 1) * g.row_b + (v + 1) * PIX_B + (o8 & 3) * 16;
    *(uint4w*)o = round8<BF>(val);
}

// ---- framed staging: fp32 NHWC (B, H, W, C) -> planes with interior (H+2) x (W+2), the data at (1, 1), the ring written as zeros
template <int BF>
__global__ __launch_bounds__(256) void framed_kernel(const float* __restrict__ x, char* planes, int B, int C, int H, int W, PlaneGeo g) {
    const int Hf = H + 2, Wf = W + 2, oct = C / 8;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * Hf * Wf * oct) return;
    const int o8 = (int)(idx % oct);
    long r = idx / oct;
    const int v = (int)(r % Wf); r /= Wf;
    const int u = (int)(r % Hf);
    const int b = (int)(r / Hf);
    float val[8];
    load8_or_zero(x, H, W, C, b, u - 1, v - 1, o8, val);
    *(uint4w*)(planes + rec_off(g, b, o8 >> 2, u, v, o8 & 3)) = round8<BF>(val);
}

// ---- OIHW [O][C][4][4] fp32 -> the 2x2 pack [chunk][tap a*2+b][k-step][mb][lane][8] of a (cout, cin) weight; one thread per packed element.
// TF = 0: W2 (cout = O, cin = 4C);  TF = 1: Wt (cout = 4C, cin = O)
__device__ __forceinline__ void pack2x2_elem(const float* __restrict__ w, unsigned short* __restrict__ out, const int O, const int C, const int tf,
                                             const int bf, const long idx) {
    const int cout = tf ? 4 * C : O, cin = tf ? O : 4 * C;
    const WpackElem e = wpack_decode(idx, cout / 32, 4);
    const int a = e.tap >> 1, b = e.tap & 1;
    float v = 0.f;
    if (e.ic < cin) {
        const int k = tf ? e.oc : e.ic, o = tf ? e.ic : e.oc;
        const int ph = k / C, c = k - ph * C;
        const int ky = 2 * (tf ? 1 - a : a) + (ph >> 1), kx = 2 * (tf ? 1 - b : b) + (ph & 1);
        v = w[(((long)o * C + c) * 4 + ky) * 4 + kx];
    }
    out[idx] = to16(v, bf);
}
__global__ __launch_bounds__(256) void pack2x2_kernel(const float* __restrict__ w, unsigned short* out, int O, int C, int tf, int bf, long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < total) pack2x2_elem(w, out, O, C, tf, bf, idx);
}
// both packs of one weight in one launch: W2 in fp16 and Wt in bf16 (spectral norm rewrites the weight on every training forward)
__global__ __launch_bounds__(256) void pack2x2_pair_kernel(const float* __restrict__ w, unsigned short* w2, unsigned short* wt, int O, int C, long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    if (blockIdx.y == 0) pack2x2_elem(w, w2, O, C, 0, 0, idx);
    else pack2x2_elem(w, wt, O, C, 1, 1, idx);
}

// ---- depth-to-space: fp32 NHWC (B, H/2+1, W/2+1, 4C) -> fp32 NHWC (B, H, W, C), ring cropped; one thread per 4 channels
__global__ __launch_bounds__(256) void d2s_kernel(const float* __restrict__ ds, float* __restrict__ dx, int B, int C, int H, int W) {
    const int q4 = C / 4, Hs = H / 2 + 1, Ws = W / 2 + 1;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * H * W * q4) return;
    const int c4 = (int)(idx % q4);
    long r = idx / q4;
    const int xx = (int)(r % W); r /= W;
    const int y = (int)(r % H);
    const int b = (int)(r / H);
    const int u = (y + 1) >> 1, p = (y + 1) & 1, v = (xx + 1) >> 1, q = (xx + 1) & 1;
    *(floatx4*)(dx + idx * 4) = *(const floatx4*)(ds + (((long)b * Hs + u) * Ws + v) * 4 * C + (2 * p + q) * C + c4 * 4);
}

// ---- weight gradient --------------------------------------------------------------------------------------------------------------------
// dW2[o][k][a][b] = sum over (n, i, j) of g[n][o][i][j] S[n][k][i+a][j+b] as a GEMM over pixels on v_mfma_f32_16x16x16_bf16: a workgroup owns a
// 16 (o) x 16 (k) block (blockIdx.y, blockIdx.z) and walks the 8 x 64 tiles blockIdx.x, + gridDim.x, ...; its four waves take two rows of a tile
// each.  K of the MFMA is the pixel axis, so both operands are staged channel-major ([channel][row][pixel], two pixels per dword; channel stride
// = 4 mod 64 dwords: conflict-free 8-byte fragment reads); the tap b = 1 fragment is funnel-shifted out of the aligned quad and the first dword
// of its neighbour.  S is fp16 in memory and re-rounded to bf16 (RNE) while staged; g's bf16 bits are the operand.  The four taps' partial sums
// go to the workgroup's workspace slot (waves added in the order 0..3), a second kernel adds the slots in the order of blockIdx.x and writes OIHW.
constexpr int WG_ROWS = TILE_H + 1;            // staged S rows: Y0 .. Y0+8
constexpr int WG_QX = 17;                      // staged 4-pixel groups per S row: columns X0 .. X0+67
constexpr int WG_SX = 324;                     // dwords per staged S channel (>= 9 * 17 * 2, = 4 mod 64)
constexpr int WG_SD = 260;                     // dwords per staged g channel (8 * 64 / 2 + 4)
constexpr int WG_NIX = (WG_ROWS * WG_QX * 4 + 255) / 256;
constexpr int WG_NID = TILE_H * 16 * 4 / 256;
constexpr int WG_LDS_B = (16 * WG_SX + 16 * WG_SD) * 4;
static_assert(WG_LDS_B >= 4 * 4 * 256 * 4, "flush buffer must fit");

struct WG2Params {
    const char* s;          // fp16 planes of S: interior (H+1) x (W+1)
    PlaneGeo gs;
    const char* g;          // bf16 framed planes of g: interior (H+2) x (W+2), the data at (1, 1)
    PlaneGeo gg;
    int H, W;               // of g
    int tiles_x, tiles_per_img, ntiles;
    float* ws;
};

__device__ __forceinline__ unsigned field_pair(const uint2w a, const uint2w b, const int j) {
    const unsigned ua = (j & 1) ? (a[j >> 1] >> 16) : (a[j >> 1] & 0xffffu);
    const unsigned ub = (j & 1) ? (b[j >> 1] & 0xffff0000u) : (b[j >> 1] << 16);
    return ua | ub;
}

__global__ __launch_bounds__(256) void wgrad2x2_kernel(const WG2Params p) {
    extern __shared__ __attribute__((aligned(16))) float wsm[];
    unsigned* s_x = (unsigned*)wsm;                 // [16 k][WG_SX]
    unsigned* s_dy = s_x + 16 * WG_SX;              // [16 o][WG_SD]
    float* s_red = wsm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kk = lane >> 4;
    const int ob = blockIdx.y, c = blockIdx.z;
    floatx4 acc[4];
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) acc[tp] = floatx4{0.f, 0.f, 0.f, 0.f};
    for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
        const int img = t / p.tiles_per_img;
        const int trem = t - img * p.tiles_per_img;
        const int ty = trem / p.tiles_x, tx = trem - ty * p.tiles_x;
        const int Y0 = ty * TILE_H, X0 = tx * TILE_W;
        uint2w lx[WG_NIX][4], ld[WG_NID][4];
#pragma unroll
        for (int it = 0; it < WG_NIX; ++it) {
            const int u = tid + it * 256;
            const int cg = u & 3, q = u >> 2;
            const int r = q / WG_QX, qc = q - r * WG_QX;
            const int y = Y0 + r, x0 = X0 + qc * 4;
            const int ch = c * 16 + cg * 4;
            const bool rowok = u < WG_ROWS * WG_QX * 4 && y <= p.H;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uint2w a = {0u, 0u};
                if (rowok && x0 + i <= p.W)
                    a = *(const uint2w*)(p.s + (long)img * p.gs.img_b + (long)(ch >> 5) * p.gs.plane_b + (long)(y + 1) * p.gs.row_b + (x0 + i + 1) * PIX_B +
                                         (ch & 31) * 2);
                lx[it][i] = a;
            }
        }
#pragma unroll
        for (int it = 0; it < WG_NID; ++it) {
            const int u = tid + it * 256;
            const int cg = u & 3, q = u >> 2;
            const int y = Y0 + (q >> 4), x0 = X0 + (q & 15) * 4;
            const int dch = ob * 16 + cg * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uint2w a = {0u, 0u};
                if (y < p.H && x0 + i < p.W)
                    a = *(const uint2w*)(p.g + (long)img * p.gg.img_b + (long)(dch >> 5) * p.gg.plane_b + (long)(y + 2) * p.gg.row_b + (x0 + i + 2) * PIX_B +
                                         (dch & 31) * 2);
                ld[it][i] = a;
            }
        }
        __syncthreads();                       // the previous tile's fragment reads are done
#pragma unroll
        for (int it = 0; it < WG_NIX; ++it) {
            const int u = tid + it * 256;
            if (u < WG_ROWS * WG_QX * 4) {
                const int cg = u & 3, q = u >> 2;
                float f[4][4];                 // [pixel][channel]: fp16 -> fp32 (exact), then bf16 RNE
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const half4 h = __builtin_bit_cast(half4, lx[it][i]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) f[i][j] = (float)h[j];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    *(uint2w*)(s_x + (cg * 4 + j) * WG_SX + q * 2) = uint2w{bf16x2_rne(f[0][j], f[1][j]), bf16x2_rne(f[2][j], f[3][j])};
            }
        }
#pragma unroll
        for (int it = 0; it < WG_NID; ++it) {
            const int u = tid + it * 256;
            const int cg = u & 3, q = u >> 2;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *(uint2w*)(s_dy + (cg * 4 + j) * WG_SD + q * 2) = uint2w{field_pair(ld[it][0], ld[it][1], j), field_pair(ld[it][2], ld[it][3], j)};
        }
        __syncthreads();
        // ---- 2 rows x 4 groups of 16 pixels per wave
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const int row = wave * 2 + (ks >> 2), g = ks & 3;
            const short4w a = __builtin_bit_cast(short4w, *(const uint2w*)(s_dy + l15 * WG_SD + (row * 16 + g * 4 + kk) * 2));
            const unsigned* bp = s_x + l15 * WG_SX + (row * WG_QX + g * 4 + kk) * 2;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const unsigned* rp = bp + dy * WG_QX * 2;
                const uint2w cur = *(const uint2w*)rp;
                const unsigned nx = rp[2];
                const uint2w b1 = {__builtin_amdgcn_alignbit(cur[1], cur[0], 16), __builtin_amdgcn_alignbit(nx, cur[1], 16)};
                acc[dy * 2 + 0] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, __builtin_bit_cast(short4w, cur), acc[dy * 2 + 0], 0, 0, 0);
                acc[dy * 2 + 1] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, __builtin_bit_cast(short4w, b1), acc[dy * 2 + 1], 0, 0, 0);
            }
        }
    }
    // flush: D[row = o = kk*4 + r][col = k = l15] of each wave, the waves added in the order 0, 1, 2, 3
    __syncthreads();
#pragma unroll
    for (int tp = 0; tp < 4; ++tp)
#pragma unroll
        for (int r = 0; r < 4; ++r) s_red[((wave * 4 + tp) * 16 + kk * 4 + r) * 16 + l15] = acc[tp][r];
    __syncthreads();
    const long slot = ((long)blockIdx.x * gridDim.y + ob) * gridDim.z + c;
    for (int u = tid; u < 1024; u += 256) p.ws[slot * 1024 + u] = s_red[u] + s_red[1024 + u] + s_red[2048 + u] + s_red[3072 + u];
}

// dw[o][c][ky][kx] = the slots' sums in the order of the walkers; (ky, kx) = (2a+p, 2b+q), k = (2p+q) C + c
__global__ __launch_bounds__(256) void wgrad2x2_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int O, int C, int nwalk) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)O * C * 16) return;
    const int kx = (int)(idx & 3), ky = (int)((idx >> 2) & 3);
    const long oc = idx >> 4;
    const int c = (int)(oc % C), o = (int)(oc / C);
    const int k = (2 * (ky & 1) + (kx & 1)) * C + c, tap = (ky >> 1) * 2 + (kx >> 1);
    const int nob = O / 16, nchunk = 4 * C / 16;
    float s = 0.f;
    for (int w = 0; w < nwalk; ++w) s += ws[(((long)w * nob + (o >> 4)) * nchunk + (k >> 4)) * 1024 + tap * 256 + (o & 15) * 16 + (k & 15)];
    dw[idx] = s;
}

// walkers of the weight gradient: enough workgroups to fill the device, never more than tiles
inline int wgrad_walkers(int O, int C, int B, int Ho, int Wo) {
    const long ntiles = (long)((Wo + TILE_W - 1) / TILE_W) * ((Ho + TILE_H - 1) / TILE_H) * B;
    const long blocks = (long)(O / 16) * (4 * C / 16);
    long n = 4096 / blocks;
    if (n < 1) n = 1;
    return (int)(n < ntiles ? n : ntiles);
}

}  // namespace

extern "C" int srbh_s2d_nhwc32_to_act16(const float* x, void* planes, int B, int C, int H, int W, int bf16, void* stream) {
    SRBH_REQUIRE(x && planes, "srbh_s2d_nhwc32_to_act16: null pointer");
    SRBH_REQUIRE(B > 0 && C > 0 && (C & 31) == 0, "srbh_s2d_nhwc32_to_act16: C must be a positive multiple of 32 (got B=%d C=%d)", B, C);
    SRBH_REQUIRE(H > 0 && W > 0 && !(H & 1) && !(W & 1), "srbh_s2d_nhwc32_to_act16: H and W must be even (got %dx%d)", H, W);
    const int Hs = H / 2 + 1, Ws = W / 2 + 1;
    const long total = (long)B * 4 * Hs * Ws * (C / 8);
    SRBH_REQUIRE(fits(total), "srbh_s2d_nhwc32_to_act16: too large");
    const PlaneGeo g = plane_geo(B, 4 * C / 32, Hs, Ws);
    if (bf16) hipLaunchKernelGGL(s2d_kernel<1>, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, x, (char*)planes, B, C, H, W, g);
    else hipLaunchKernelGGL(s2d_kernel<0>, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, x, (char*)planes, B, C, H, W, g);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_nhwc32_to_act16_framed(const float* x, void* planes, int B, int C, int H, int W, int bf16, void* stream) {
    SRBH_REQUIRE(x && planes, "srbh_nhwc32_to_act16_framed: null pointer");
    SRBH_REQUIRE(B > 0 && C > 0 && (C & 31) == 0, "srbh_nhwc32_to_act16_framed: C must be a positive multiple of 32 (got B=%d C=%d)", B, C);
    SRBH_REQUIRE(H > 0 && W > 0, "srbh_nhwc32_to_act16_framed: bad geometry %dx%d", H, W);
    const long total = (long)B * (H + 2) * (W + 2) * (C / 8);
    SRBH_REQUIRE(fits(total), "srbh_nhwc32_to_act16_framed: too large");
    const PlaneGeo g = plane_geo(B, C / 32, H + 2, W + 2);
    if (bf16) hipLaunchKernelGGL(framed_kernel<1>, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, x, (char*)planes, B, C, H, W, g);
    else hipLaunchKernelGGL(framed_kernel<0>, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, x, (char*)planes, B, C, H, W, g);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" size_t srbh_wpack2x2_bytes(int cout, int cin) {
    if (cout <= 0 || cin <= 0) return 0;
    return (size_t)((cin + 31) / 32) * 8 * ((cout + 31) / 32) * 1024;
}

extern "C" int srbh_pack_conv4x4s2(const float* w, int O, int C, int transpose_flip, int bf16, void* packed, void* stream) {
    SRBH_REQUIRE(w && packed, "srbh_pack_conv4x4s2: null pointer");
    SRBH_REQUIRE(O > 0 && C > 0 && (C & 31) == 0 && (O & 31) == 0, "srbh_pack_conv4x4s2: O and C must be positive multiples of 32 (got O=%d C=%d)", O, C);
    const long total = (long)srbh_wpack2x2_bytes(O, 4 * C) / 2;      // (the same size either way round)
    SRBH_REQUIRE(fits(total), "srbh_pack_conv4x4s2: too large");
    hipLaunchKernelGGL(pack2x2_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, w, (unsigned short*)packed, O, C, transpose_flip != 0,
                       bf16 != 0, total);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_pack_conv4x4s2_pair(const float* w, int O, int C, void* w2_f16, void* wt_b16, void* stream) {
    SRBH_REQUIRE(w && w2_f16 && wt_b16, "srbh_pack_conv4x4s2_pair: null pointer");
    SRBH_REQUIRE(O > 0 && C > 0 && (C & 31) == 0 && (O & 31) == 0, "srbh_pack_conv4x4s2_pair: O and C must be positive multiples of 32 (got O=%d C=%d)", O, C);
    const long total = (long)srbh_wpack2x2_bytes(O, 4 * C) / 2;
    SRBH_REQUIRE(fits(total), "srbh_pack_conv4x4s2_pair: too large");
    hipLaunchKernelGGL(pack2x2_pair_kernel, dim3(blocks_of(total), 2), dim3(256), 0, (hipStream_t)stream, w, (unsigned short*)w2_f16, (unsigned short*)wt_b16,
                       O, C, total);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_d2s_nhwc32(const float* ds, float* dx, int B, int C, int H, int W, void* stream) {
    SRBH_REQUIRE(ds && dx, "srbh_d2s_nhwc32: null pointer");
    SRBH_REQUIRE(B > 0 && C > 0 && (C & 31) == 0, "srbh_d2s_nhwc32: C must be a positive multiple of 32 (got B=%d C=%d)", B, C);
    SRBH_REQUIRE(H > 0 && W > 0 && !(H & 1) && !(W & 1), "srbh_d2s_nhwc32: H and W must be even (got %dx%d)", H, W);
    const long total = (long)B * H * W * (C / 4);
    SRBH_REQUIRE(fits(total), "srbh_d2s_nhwc32: too large");
    hipLaunchKernelGGL(d2s_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, ds, dx, B, C, H, W);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

// the 2x2-tap VALID form of the wide conv: input interior (H+1) x (W+1), cout a multiple of 64, fp32 NHWC output of all channels only
extern "C" int srbh_wconv2x2(const srbh_wconv3x3_args* a, void* stream) {
    static constexpr WideForm form = {"srbh_wconv2x2", 2, 1, false, false, false, true};
    if (const int rc = wide_validate(a, form)) return rc;
    const WKParams p = wide_params(a, form);
    return with_const<2>(a->bf16 != 0, [&](auto bf) {
        return launch<wconv2x2_kernel<2, decltype(bf)::value>, true>(dim3(p.nblocks), lds_bytes<2, 0>(), (hipStream_t)stream, p);
    });
}

extern "C" size_t srbh_wgrad4x4s2_ws_bytes(int O, int C, int B, int Ho, int Wo) {
    if (O <= 0 || C <= 0 || B <= 0 || Ho <= 0 || Wo <= 0 || (O & 15) || (C & 31)) return 0;
    return (size_t)wgrad_walkers(O, C, B, Ho, Wo) * (O / 16) * (4 * C / 16) * 1024 * sizeof(float);
}

extern "C" int srbh_wgrad4x4s2_b16(const void* s_planes, const void* g_planes, int B, int C, int O, int Ho, int Wo, float* dw, void* ws, void* stream) {
    SRBH_REQUIRE(s_planes && g_planes && dw && ws, "srbh_wgrad4x4s2_b16: null pointer");
    SRBH_REQUIRE(B > 0 && C > 0 && (C & 31) == 0, "srbh_wgrad4x4s2_b16: C must be a positive multiple of 32 (got B=%d C=%d)", B, C);
    SRBH_REQUIRE(O >= 64 && O % 64 == 0, "srbh_wgrad4x4s2_b16: cout must be a multiple of 64 (got %d)", O);
    SRBH_REQUIRE(Ho > 0 && Wo > 0, "srbh_wgrad4x4s2_b16: bad geometry %dx%d", Ho, Wo);
    SRBH_REQUIRE(O / 16 <= 65535 && 4 * C / 16 <= 65535, "srbh_wgrad4x4s2_b16: too many channels");
    WG2Params p;
    p.s = (const char*)s_planes;
    p.gs = plane_geo(B, 4 * C / 32, Ho + 1, Wo + 1);
    p.g = (const char*)g_planes;
    p.gg = plane_geo(B, O / 32, Ho + 2, Wo + 2);
    p.H = Ho;
    p.W = Wo;
    p.tiles_x = (Wo + TILE_W - 1) / TILE_W;
    p.tiles_per_img = p.tiles_x * ((Ho + TILE_H - 1) / TILE_H);
    const long ntiles = (long)p.tiles_per_img * B;
    SRBH_REQUIRE(ntiles < (1l << 30), "srbh_wgrad4x4s2_b16: too many tiles");
    p.ntiles = (int)ntiles;
    p.ws = (float*)ws;
    const int nwalk = wgrad_walkers(O, C, B, Ho, Wo);
    hipLaunchKernelGGL(wgrad2x2_kernel, dim3(nwalk, O / 16, 4 * C / 16), dim3(256), WG_LDS_B, (hipStream_t)stream, p);
    SRBH_HIP(hipGetLastError());
    const long total = (long)O * C * 16;
    hipLaunchKernelGGL(wgrad2x2_reduce_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, (const float*)ws, dw, O, C, nwalk);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
