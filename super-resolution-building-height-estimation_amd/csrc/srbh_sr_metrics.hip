// srbh_sr_metrics.hip -- quality metrics of the SR stage as one-read reductions (reference SR/psnr_ssim.py).
//
// calculate_psnr_pt (:203-232), calculate_ssim_pt / _ssim_pth (:283-318, :352-382) and calculate_cpsnr_pt (:443-490) each read two images
// and return a few numbers.  The reference runs SSIM as five grouped 11x11 float64 convolutions plus ~15 elementwise passes and cPSNR as
// 81 offset iterations of ~8 passes each; here a workgroup stages a tile of both images (plus halo) in LDS once and produces partial SUMS:
//   srbh_sr_psnr_ssim_sums : sum (a-b)^2 and the sum of the SSIM map (separable 11-tap Gaussian: horizontal pass, then vertical pass)
//   srbh_sr_cpsnr_sums     : for each of the 81 offsets, sum d and sum d^2 of d = a[r+ro, c+co] - b[r+8-ro, c+8-co]
// The scalar arithmetic around the sums (mean, log10, bias-corrected MSE, best offset) stays with the caller (sr_metrics.py).
//
// Contract shared by both: fp32 images of logical shape (B, C, H, W), C in {1, 3}, each with its own four ELEMENT strides (channels_last
// outputs, NCHW targets and cropped views are read in place); y_only (C == 3): the staged value is the BT.601 luma of rgb2ycbcr_pt
// (:122-144) in fp32; everything behind the fp32 staging is float64 (a product of two fp32 values is exact there).  Bit-reproducible:
// the tile -> workgroup map and every summation order depend on (H, W) only, each workgroup writes its partial sums to its own slot of
// the caller's workspace, and one small fold kernel adds the slots of an image in a fixed order.  No floating-point atomics.
#include <math.h>
#include "srbh_internal.h"

namespace {
using namespace srbh;

struct Img {
    const float* p;
    long sb, sc, sr, sw;   // element strides: batch, channel, row, column
};

// BT.601 luma of rgb2ycbcr_pt(y_only=True): (65.481 r + 128.553 g + 24.966 b + 16) / 255 in fp32, left to right, no contraction (the
// reference's torch.matmul leaves the order of the three terms open; tests/test_gpu_sr_metrics.py bounds what that can change).  Plain
// operators under the pragma: the __fmul_rn / __fadd_rn wrappers are compiled with contraction allowed and fuse once inlined.
__device__ __forceinline__ float luma601(float r, float g, float b) {
#pragma clang fp contract(off)
    const float tr = 65.481f * r, tg = 128.553f * g, tb = 24.966f * b;
    const float s = ((tr + tg) + tb) + 16.0f;
    return s / 255.0f;      // correctly rounded (hipcc's default for fp32 division)
}

// the staged value of pixel (r, c) of effective channel ch of image b (in bounds)
template <bool Y>
__device__ __forceinline__ float load_px(const Img& m, int b, int ch, int r, int c) {
    const float* q = m.p + (long)b * m.sb + (long)r * m.sr + (long)c * m.sw;
    if (Y) return luma601(q[0], q[m.sc], q[2 * m.sc]);
    return q[(long)ch * m.sc];
}

// sum of v over the 256 threads, in a fixed order; the result is valid in thread 0.  red: 4 doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- PSNR / SSIM ---------------------------------------------------------------------------------------------------------------------
constexpr int PT_H = 16, PT_W = 32;            // pixels a workgroup owns (their (a-b)^2, and the SSIM positions whose top-left they are)
constexpr int SS_HALO = 10;                    // 11-tap window: 5 on each side
constexpr int SS_R = PT_H + SS_HALO, SS_C = PT_W + SS_HALO;
constexpr int SS_LD = SS_C + 1;

struct PsnrSsimParams {
    Img a, b;
    int B, C, Ce, H, W;      // C: channels in memory, Ce: effective channels (1 with y_only)
    int tiles_x, tiles;      // per image
    double g[11];            // normalised Gaussian, sigma 1.5
    double* ws;              // [B][tiles][2]: sq, ssim
};

// One workgroup = one PT_H x PT_W tile of one image, all effective channels.  SSIM: the tile plus a 10-pixel halo to the right and below is
// staged (fp32, the value the reference casts to float64), the five windowed quantities (a, b, a^2, b^2, ab of the inputs scaled by 255)
// go through the horizontal pass into `hb`, then each thread finishes two positions vertically and adds their map values.
template <bool SSIM, bool Y>
__global__ __launch_bounds__(256) void psnr_ssim_kernel(const PsnrSsimParams p) {
    constexpr int R = SSIM ? SS_R : PT_H, CW = SSIM ? SS_C : PT_W;
    __shared__ float sa[SSIM ? 3 * SS_R * SS_LD : 1], sb[SSIM ? 3 * SS_R * SS_LD : 1];
    __shared__ double hb[SSIM ? 5 * SS_R * PT_W : 1];
    __shared__ double red[4];
    const int t = threadIdx.x, img = blockIdx.z;
    const int ty = blockIdx.x / p.tiles_x, tx = blockIdx.x - ty * p.tiles_x;
    const int r0 = ty * PT_H, c0 = tx * PT_W;
    const int Ce = p.Ce;
    // channel fastest when that is the small stride (channels_last): neighbouring threads then read neighbouring addresses
    const bool ch_fast = !Y && Ce > 1 && p.a.sc < p.a.sw;
    double sq = 0.0;
    for (int i = t; i < Ce * R * CW; i += 256) {
        int ch, lr, lc;
        if (ch_fast) { ch = i % Ce; const int j = i / Ce; lc = j % CW; lr = j / CW; }
        else { lc = i % CW; const int j = i / CW; lr = j % R; ch = j / R; }
        const int r = r0 + lr, c = c0 + lc;
        float va = 0.f, vb = 0.f;
        if (r < p.H && c < p.W) {
            va = load_px<Y>(p.a, img, ch, r, c);
            vb = load_px<Y>(p.b, img, ch, r, c);
            if (lr < PT_H && lc < PT_W) {
                const double d = (double)va - (double)vb;
                sq += d * d;
            }
        }
        if (SSIM) {
            sa[(ch * SS_R + lr) * SS_LD + lc] = va;
            sb[(ch * SS_R + lr) * SS_LD + lc] = vb;
        }
    }
    double ss = 0.0;
    if (SSIM) {
        const double c1 = (0.01 * 255) * (0.01 * 255), c2 = (0.03 * 255) * (0.03 * 255);
        for (int ch = 0; ch < Ce; ++ch) {
            __syncthreads();      // staging (first channel) / the previous channel's vertical pass is done with hb
            for (int i = t; i < SS_R * PT_W; i += 256) {
                const int lr = i / PT_W, lc = i - lr * PT_W;
                const float* ra = sa + (ch * SS_R + lr) * SS_LD + lc;
                const float* rb = sb + (ch * SS_R + lr) * SS_LD + lc;
                double m1 = 0, m2 = 0, q1 = 0, q2 = 0, q12 = 0;
#pragma unroll
                for (int k = 0; k < 11; ++k) {
                    const double x = (double)ra[k] * 255.0, y = (double)rb[k] * 255.0, w = p.g[k];
                    m1 += w * x;
                    m2 += w * y;
                    q1 += w * (x * x);
                    q2 += w * (y * y);
                    q12 += w * (x * y);
                }
                double* h = hb + lr * PT_W + lc;
                h[0] = m1; h[SS_R * PT_W] = m2; h[2 * SS_R * PT_W] = q1; h[3 * SS_R * PT_W] = q2; h[4 * SS_R * PT_W] = q12;
            }
            __syncthreads();
            for (int i = t; i < PT_H * PT_W; i += 256) {
                const int lr = i / PT_W, lc = i - lr * PT_W;
                if (r0 + lr > p.H - 11 || c0 + lc > p.W - 11) continue;      // the window would leave the image
                const double* h = hb + lr * PT_W + lc;
                double v[5];
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    double s = 0;
#pragma unroll
                    for (int k = 0; k < 11; ++k) s += p.g[k] * h[q * SS_R * PT_W + k * PT_W];
                    v[q] = s;
                }
                const double mu1 = v[0], mu2 = v[1], mu11 = mu1 * mu1, mu22 = mu2 * mu2, mu12 = mu1 * mu2;
                const double s1 = v[2] - mu11, s2 = v[3] - mu22, s12 = v[4] - mu12;
                const double cs = (2 * s12 + c2) / (s1 + s2 + c2);
                ss += ((2 * mu12 + c1) / (mu11 + mu22 + c1)) * cs;
            }
        }
    }
    double* out = p.ws + ((long)img * p.tiles + blockIdx.x) * 2;
    const double tsq = block_sum(sq, red);
    if (t == 0) out[0] = tsq;
    const double tss = SSIM ? block_sum(ss, red) : 0.0;
    if (t == 0) out[1] = tss;
}

// out[img] = sum of the image's slots: thread t adds slots t, t + 256, ... in order, then a fixed tree.  One block per image.
__global__ __launch_bounds__(256) void psnr_ssim_fold_kernel(const double* __restrict__ ws, int tiles, double* sq, double* ssim) {
    __shared__ double red[4];
    const double* w = ws + (long)blockIdx.x * tiles * 2;
    double s0 = 0.0, s1 = 0.0;
    for (int k = threadIdx.x; k < tiles; k += 256) { s0 += w[2 * k]; s1 += w[2 * k + 1]; }
    const double a = block_sum(s0, red);
    if (threadIdx.x == 0 && sq) sq[blockIdx.x] = a;
    const double b = block_sum(s1, red);
    if (threadIdx.x == 0 && ssim) ssim[blockIdx.x] = b;
}

// ---- cPSNR ---------------------------------------------------------------------------------------------------------------------------
constexpr int CT = 32;                         // window positions per tile side
constexpr int CP_OFF = 8;                      // max_offset of calculate_cpsnr_pt
constexpr int CS = CT + CP_OFF, CS_LD = CS + 1;
constexpr int CP_NOFF = 81, CP_PER_WAVE = 21;  // 4 waves x 21 >= 81 offsets
constexpr int CP_MAX_WGS = 16;                 // workgroups per (image, channel): each walks tiles wg, wg + nwg, ...

struct CpsnrParams {
    Img a, b;
    int B, C, Ce, H, W;
    int tiles_x, tiles, nwg;
    double* ws;              // [B][Ce][nwg][81][2]
};

// One workgroup walks a fixed subset of the 32x32 tiles of one channel of one image.  Per tile both images are staged with an 8-pixel
// halo; wave w owns offsets 21 w .. 21 w + 20 and keeps their sum d / sum d^2 in registers over the whole walk (every wave visits every
// position); the lanes are folded once at the end.
template <bool Y>
__global__ __launch_bounds__(256) void cpsnr_kernel(const CpsnrParams p) {
    __shared__ float sa[CS * CS_LD], sb[CS * CS_LD];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int img = blockIdx.z, ch = blockIdx.y;
    const int Hw = p.H - CP_OFF, Ww = p.W - CP_OFF;       // the window
    double sd[CP_PER_WAVE], sq[CP_PER_WAVE];
#pragma unroll
    for (int k = 0; k < CP_PER_WAVE; ++k) sd[k] = sq[k] = 0.0;
    for (int tile = blockIdx.x; tile < p.tiles; tile += p.nwg) {
        const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
        const int r0 = ty * CT, c0 = tx * CT;
        __syncthreads();      // the previous tile's reads are done
        for (int i = t; i < CS * CS; i += 256) {
            const int lr = i / CS, lc = i - lr * CS;
            const int r = r0 + lr, c = c0 + lc;
            float va = 0.f, vb = 0.f;
            if (r < p.H && c < p.W) {
                va = load_px<Y>(p.a, img, ch, r, c);
                vb = load_px<Y>(p.b, img, ch, r, c);
            }
            sa[lr * CS_LD + lc] = va;
            sb[lr * CS_LD + lc] = vb;
        }
        __syncthreads();
        for (int i = lane; i < CT * CT; i += 64) {
            const int lr = i / CT, lc = i - lr * CT;
            if (r0 + lr >= Hw || c0 + lc >= Ww) continue;
            const float* pa = sa + lr * CS_LD + lc;
            const float* pb = sb + (lr + CP_OFF) * CS_LD + lc + CP_OFF;
#pragma unroll
            for (int k = 0; k < CP_PER_WAVE; ++k) {
                const int off = wave * CP_PER_WAVE + k;
                if (off < CP_NOFF) {      // wave-uniform
                    const int ro = off / 9, co = off - ro * 9;
                    const double d = (double)pa[ro * CS_LD + co] - (double)pb[-(ro * CS_LD + co)];
                    sd[k] += d;
                    sq[k] += d * d;
                }
            }
        }
    }
    double* out = p.ws + (((long)img * p.Ce + ch) * p.nwg + blockIdx.x) * (CP_NOFF * 2);
#pragma unroll
    for (int k = 0; k < CP_PER_WAVE; ++k) {
        double x = sd[k], y = sq[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { x += __shfl_down(x, o, 64); y += __shfl_down(y, o, 64); }
        const int off = wave * CP_PER_WAVE + k;
        if (lane == 0 && off < CP_NOFF) { out[off * 2] = x; out[off * 2 + 1] = y; }
    }
}

// one block per (image, channel): thread q < 162 adds its quantity over the nwg slots in order
__global__ __launch_bounds__(192) void cpsnr_fold_kernel(const double* __restrict__ ws, int nwg, double* sd, double* sqd) {
    const int q = threadIdx.x;
    if (q >= CP_NOFF * 2) return;
    const double* w = ws + (long)blockIdx.x * nwg * (CP_NOFF * 2);
    double s = 0.0;
    for (int k = 0; k < nwg; ++k) s += w[(long)k * (CP_NOFF * 2) + q];
    ((q & 1) ? sqd : sd)[(long)blockIdx.x * CP_NOFF + (q >> 1)] = s;
}

inline int psnr_tiles(int H, int W, int* tiles_x) {
    *tiles_x = (W + PT_W - 1) / PT_W;
    return *tiles_x * ((H + PT_H - 1) / PT_H);
}
inline int cpsnr_tiles(int H, int W, int* tiles_x) {
    *tiles_x = (W - CP_OFF + CT - 1) / CT;
    return *tiles_x * ((H - CP_OFF + CT - 1) / CT);
}
inline int cpsnr_nwg(int tiles) { return tiles < CP_MAX_WGS ? tiles : CP_MAX_WGS; }

// every address a kernel forms is b*sb + ch*sc + r*sr + c*sw with 0 <= b < B, ch < C, r < H, c < W: strides may not be negative
inline bool strides_ok(const long* s) { return s && s[0] >= 0 && s[1] >= 0 && s[2] >= 0 && s[3] >= 0; }

}  // namespace

extern "C" size_t srbh_sr_psnr_ssim_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    int tx;
    return (size_t)B * psnr_tiles(H, W, &tx) * 2 * sizeof(double);
}

extern "C" int srbh_sr_psnr_ssim_sums(const float* a, const long* a_strides, const float* b, const long* b_strides, int B, int C, int H,
                                      int W, int y_only, double* sq, double* ssim, void* ws, void* stream) {
    SRBH_REQUIRE(a && b && ws && (sq || ssim) && B > 0 && H > 0 && W > 0, "srbh_sr_psnr_ssim_sums: bad arguments");
    SRBH_REQUIRE(B <= 65535, "srbh_sr_psnr_ssim_sums: at most 65535 images per call (got %d)", B);
    SRBH_REQUIRE(C == 1 || C == 3, "srbh_sr_psnr_ssim_sums: 1 or 3 channels (got %d)", C);
    SRBH_REQUIRE(!y_only || C == 3, "srbh_sr_psnr_ssim_sums: y_only needs 3 channels (got %d)", C);
    SRBH_REQUIRE(strides_ok(a_strides) && strides_ok(b_strides), "srbh_sr_psnr_ssim_sums: strides must be given and non-negative");
    SRBH_REQUIRE(!ssim || (H >= 11 && W >= 11), "srbh_sr_psnr_ssim_sums: SSIM needs an 11x11 window (got %dx%d)", H, W);
    PsnrSsimParams p;
    p.a = Img{a, a_strides[0], a_strides[1], a_strides[2], a_strides[3]};
    p.b = Img{b, b_strides[0], b_strides[1], b_strides[2], b_strides[3]};
    p.B = B; p.C = C; p.Ce = y_only ? 1 : C; p.H = H; p.W = W;
    p.tiles = psnr_tiles(H, W, &p.tiles_x);
    double gs = 0.0;
    for (int k = 0; k < 11; ++k) { p.g[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5)); gs += p.g[k]; }
    for (int k = 0; k < 11; ++k) p.g[k] /= gs;
    p.ws = (double*)ws;
    const dim3 grid(p.tiles, 1, B);
    hipStream_t st = (hipStream_t)stream;
    if (ssim) {
        if (y_only) hipLaunchKernelGGL((psnr_ssim_kernel<true, true>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((psnr_ssim_kernel<true, false>), grid, dim3(256), 0, st, p);
    } else {
        if (y_only) hipLaunchKernelGGL((psnr_ssim_kernel<false, true>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((psnr_ssim_kernel<false, false>), grid, dim3(256), 0, st, p);
    }
    SRBH_HIP(hipGetLastError());
    hipLaunchKernelGGL(psnr_ssim_fold_kernel, dim3(B), dim3(256), 0, st, (const double*)ws, p.tiles, sq, ssim);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" size_t srbh_sr_cpsnr_ws_bytes(int B, int C, int H, int W, int y_only) {
    if (B <= 0 || (C != 1 && C != 3) || H < CP_OFF + 1 || W < CP_OFF + 1) return 0;
    int tx;
    return (size_t)B * (y_only ? 1 : C) * cpsnr_nwg(cpsnr_tiles(H, W, &tx)) * CP_NOFF * 2 * sizeof(double);
}

extern "C" int srbh_sr_cpsnr_sums(const float* a, const long* a_strides, const float* b, const long* b_strides, int B, int C, int H, int W,
                                  int y_only, double* sd, double* sqd, void* ws, void* stream) {
    SRBH_REQUIRE(a && b && ws && sd && sqd && B > 0, "srbh_sr_cpsnr_sums: bad arguments");
    SRBH_REQUIRE(B <= 65535, "srbh_sr_cpsnr_sums: at most 65535 images per call (got %d)", B);
    SRBH_REQUIRE(C == 1 || C == 3, "srbh_sr_cpsnr_sums: 1 or 3 channels (got %d)", C);
    SRBH_REQUIRE(!y_only || C == 3, "srbh_sr_cpsnr_sums: y_only needs 3 channels (got %d)", C);
    SRBH_REQUIRE(strides_ok(a_strides) && strides_ok(b_strides), "srbh_sr_cpsnr_sums: strides must be given and non-negative");
    SRBH_REQUIRE(H >= CP_OFF + 1 && W >= CP_OFF + 1, "srbh_sr_cpsnr_sums: the image must be at least 9x9 (got %dx%d)", H, W);
    CpsnrParams p;
    p.a = Img{a, a_strides[0], a_strides[1], a_strides[2], a_strides[3]};
    p.b = Img{b, b_strides[0], b_strides[1], b_strides[2], b_strides[3]};
    p.B = B; p.C = C; p.Ce = y_only ? 1 : C; p.H = H; p.W = W;
    p.tiles = cpsnr_tiles(H, W, &p.tiles_x);
    p.nwg = cpsnr_nwg(p.tiles);
    p.ws = (double*)ws;
    const dim3 grid(p.nwg, p.Ce, B);
    hipStream_t st = (hipStream_t)stream;
    if (y_only) hipLaunchKernelGGL(cpsnr_kernel<true>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(cpsnr_kernel<false>, grid, dim3(256), 0, st, p);
    SRBH_HIP(hipGetLastError());
    hipLaunchKernelGGL(cpsnr_fold_kernel, dim3(B * p.Ce), dim3(192), 0, st, (const double*)ws, p.nwg, sd, sqd);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
