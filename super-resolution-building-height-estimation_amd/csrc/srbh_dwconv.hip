// srbh_dwconv.hip -- depthwise KxK convolution (K = 3 or 5, stride 1 or 2), fp32 NCHW, forward / input gradient / weight
// gradient, with the zero padding folded in (top/left pad given; bottom/right implied by the output size), and the fused
// inference form of the MBConv middle.  (The encoder's other inference kernels: srbh_enc_eval.hip.)
//
// Why it exists: the EfficientNet-B4 encoder the reference instantiates (mymodels.py:242-248) is stock PyTorch ops in
// this build, but MIOpen has no fp32 solver for its 5x5 / strided depthwise convolutions and falls back
// to `naive_conv_ab_nonpacked_{fwd,bwd,wrw}` -- 10.7 % of the tiled-inference path and 5.6 ms of the 81 ms training step
// (profiles/r01e_*).  These are HBM-bound element-wise kernels: planes are at most 32x32, every tap re-read hits L1/L2.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "srbh.h"
#include "srbh_internal.h"

namespace {
using namespace srbh;

#include "srbh_dw_pieces.h"      // act_apply, wave_sum, DWLds, dw_stage, grid_for

struct DWParams {
    const float* x;     // [B][C][H][W]
    const float* w;     // [C][1][K][K]
    const float* dy;    // [B][C][OH][OW]
    float* out;         // y, dx or dw
    int B, C, H, W, OH, OW, stride, pad_t, pad_l;
};

// (What stays written out although it repeats -- profiles/dw_pieces_isa.txt, "tried and left out": the tap loops of every kernel, the
//  two-accumulator walk over LDS in dw_lds_kernel and dw_lds_eval_kernel included -- as a shared piece it cost dw_lds_kernel<5, *> 24 VGPRs
//  and three of its eight waves per SIMD; and the reduction tail of the two weight-gradient kernels -- as a shared piece
//  dw_bwd_weight_kernel<3> measured 0.4 % above the parent at 144 x 32 x 32, stride 2, and even wave_sum() inside it gives other code.)
template <int K>
__global__ __launch_bounds__(256) void dw_fwd_kernel(const DWParams p) {
    const long total = (long)p.B * p.C * p.OH * p.OW;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int ox = idx % p.OW;
        long r = idx / p.OW;
        const int oy = r % p.OH;
        r /= p.OH;                                  // r = b * C + c
        const int c = r % p.C;
        const float* xp = p.x + r * p.H * p.W;
        const float* wp = p.w + (long)c * K * K;
        const int y0 = oy * p.stride - p.pad_t, x0 = ox * p.stride - p.pad_l;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const int y = y0 + i;
            if (y < 0 || y >= p.H) continue;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const int x = x0 + j;
                if (x >= 0 && x < p.W) acc = fmaf(xp[y * p.W + x], wp[i * K + j], acc);
            }
        }
        p.out[idx] = acc;
    }
}

// dx[y][x] = sum over taps (i, j) with (y + pad_t - i) = s * oy, (x + pad_l - j) = s * ox of dy[oy][ox] * w[i][j]
template <int K>
__global__ __launch_bounds__(256) void dw_bwd_data_kernel(const DWParams p) {
    const long total = (long)p.B * p.C * p.H * p.W;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int x = idx % p.W;
        long r = idx / p.W;
        const int y = r % p.H;
        r /= p.H;
        const int c = r % p.C;
        const float* gp = p.dy + r * p.OH * p.OW;
        const float* wp = p.w + (long)c * K * K;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const int ty = y + p.pad_t - i;
            if (ty < 0 || ty % p.stride) continue;
            const int oy = ty / p.stride;
            if (oy >= p.OH) continue;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const int tx = x + p.pad_l - j;
                if (tx < 0 || tx % p.stride) continue;
                const int ox = tx / p.stride;
                if (ox < p.OW) acc = fmaf(gp[oy * p.OW + ox], wp[i * K + j], acc);
            }
        }
        p.out[idx] = acc;
    }
}

// dw[c][i][j] = sum over (b, oy, ox) of dy[b][c][oy][ox] * x[b][c][oy*s - pad_t + i][ox*s - pad_l + j]: workgroup (c, s)
// sums the images of batch slice s in a fixed tree (thread-strided partial sums -> wave shuffles -> LDS across the 4
// waves) into ws[s][c][..]; dw_reduce_kernel adds the slices in order: deterministic, and >= ~1000 workgroups even for the 144-channel layers
template <int K>
__global__ __launch_bounds__(256) void dw_bwd_weight_kernel(const DWParams p, float* __restrict__ ws, int splits) {
    const int c = blockIdx.x, sp = blockIdx.y;
    const int per_img = p.OH * p.OW;
    const int b0 = (int)((long)p.B * sp / splits), b1 = (int)((long)p.B * (sp + 1) / splits);
    const long n = (long)(b1 - b0) * per_img;
    float acc[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) acc[t] = 0.f;
    for (long e = threadIdx.x; e < n; e += 256) {
        const int b = b0 + (int)(e / per_img);
        const int q = (int)(e % per_img);
        const int oy = q / p.OW, ox = q - oy * p.OW;
        const float g = p.dy[((long)b * p.C + c) * per_img + q];
        const float* xp = p.x + ((long)b * p.C + c) * p.H * p.W;
        const int y0 = oy * p.stride - p.pad_t, x0 = ox * p.stride - p.pad_l;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const int y = y0 + i;
            if (y < 0 || y >= p.H) continue;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const int x = x0 + j;
                if (x >= 0 && x < p.W) acc[i * K + j] = fmaf(g, xp[y * p.W + x], acc[i * K + j]);
            }
        }
    }
    __shared__ float red[4][K * K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int t = 0; t < K * K; ++t) {
        float v = acc[t];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) red[wave][t] = v;
    }
    __syncthreads();
    if (threadIdx.x < K * K)
        ws[((long)sp * p.C + c) * K * K + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// forward (FLIP = 0) and input gradient (FLIP = 1) over staged planes: thread = one output, even and odd taps in two accumulators
template <int K, int FLIP>
__global__ __launch_bounds__(256) void dw_lds_kernel(const DWLds p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int plane_sz = p.PH * p.PW;
    float* wl = sm + p.P * plane_sz;
    const long p0 = (long)blockIdx.x * p.P;
    const int np = dw_stage<K, false>(p, sm, wl, p0, nullptr, nullptr);
    const int osz = p.OUTH * p.OUTW;
    float* op = p.out + p0 * osz;
    for (int e = threadIdx.x; e < np * osz; e += 256) {
        const int pl = e / osz, q = e - pl * osz, oy = q / p.OUTW, ox = q - oy * p.OUTW;
        const float* base = sm + pl * plane_sz + (oy * p.os + p.by) * p.PW + ox * p.os + p.bx;
        const float* wp = wl + pl * K * K;
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int i = 0; i < K; ++i)
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const float v = FLIP ? base[-(i * p.PW + j)] : base[i * p.PW + j];
                if ((i * K + j) & 1) a1 = fmaf(v, wp[i * K + j], a1);
                else a0 = fmaf(v, wp[i * K + j], a0);
            }
        op[e] = a0 + a1;
    }
}

// ---- MBConv middle at inference, ONE launch (round 4): y = swish(bn1(dw(swish(bn0(e))))) plus the per-plane mean squeeze-excite pools,
// with both inference BatchNorms folded to (scale, shift).  bn0 + swish is applied while the expand conv's output is staged (the zero
// padding is the padding of the ACTIVATED tensor, as in the module chain), bn1 + swish + the pool on the accumulators: the three
// elementwise passes of the unfused chain (affine_act, affine_act_pool over 6x-expanded tensors) and their two intermediates go away.
// G = 2^k threads share one plane (G = min(256, outputs per plane)); the pool is a fixed butterfly over those lanes (+ an ordered LDS sum
// across waves when G > 64): the same bits every run.
struct DWEval {
    const float* a0; const float* b0;      // bn0 folded (null: the block has no expand conv)
    const float* a1; const float* b1;      // bn1 folded
    float* pooled;                         // [planes] means of the activated output
    int G;
};
template <int K>
__global__ __launch_bounds__(256) void dw_lds_eval_kernel(const DWLds p, const DWEval q) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ float red[4];
    const int t = threadIdx.x, plane_sz = p.PH * p.PW;
    float* wl = sm + p.P * plane_sz;
    const long p0 = (long)blockIdx.x * p.P;
    const int np = dw_stage<K, true>(p, sm, wl, p0, q.a0, q.b0);
    const int osz = p.OUTH * p.OUTW, G = q.G, g = t & (G - 1), slot = t / G, R = 256 / G;
    float* op = p.out + p0 * osz;
    const float inv = 1.f / (float)osz;
    for (int pl0 = 0; pl0 < p.P; pl0 += R) {                       // (uniform trip count: the barriers below are taken by every thread)
        const int pl = pl0 + slot;
        const bool ok = pl < np;
        float sum = 0.f;
        if (ok) {
            const int ch = (int)((p0 + pl) % p.C);
            const float s = q.a1[ch], h = q.b1[ch];
            const float* wp = wl + pl * K * K;
            for (int o = g; o < osz; o += G) {
                const int oy = o / p.OUTW, ox = o - oy * p.OUTW;
                const float* base = sm + pl * plane_sz + (oy * p.os + p.by) * p.PW + ox * p.os + p.bx;
                float c0 = 0.f, c1 = 0.f;
#pragma unroll
                for (int i = 0; i < K; ++i)
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        if ((i * K + j) & 1) c1 = fmaf(base[i * p.PW + j], wp[i * K + j], c1);
                        else c0 = fmaf(base[i * p.PW + j], wp[i * K + j], c0);
                    }
                const float y = act_apply(fmaf(c0 + c1, s, h), 1);
                op[(long)pl * osz + o] = y;
                sum += y;
            }
        }
        for (int o = (G < 64 ? G : 64) >> 1; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (G <= 64) {
            if (ok && g == 0) q.pooled[p0 + pl] = sum * inv;
        } else {
            if ((t & 63) == 0) red[t >> 6] = sum;
            __syncthreads();
            if (ok && g == 0) {
                float tot = 0.f;
                for (int w = 0; w < G / 64; ++w) tot += red[(t >> 6) + w];
                q.pooled[p0 + pl] = tot * inv;
            }
            __syncthreads();
        }
    }
}

// weight gradient, LDS-staged: workgroup (c, slice) stages P images' zero-padded x planes and dy planes per round; thread = one output pixel
template <int K>
__global__ __launch_bounds__(256) void dw_lds_wgrad_kernel(const DWParams p, float* __restrict__ ws, int splits, int PH, int PW, int P) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int c = blockIdx.x, sp = blockIdx.y, t = threadIdx.x;
    const int per_img = p.OH * p.OW, plane_sz = PH * PW, xsz = p.H * p.W;
    float* dyl = sm + P * plane_sz;
    const int b0 = (int)((long)p.B * sp / splits), b1 = (int)((long)p.B * (sp + 1) / splits);
    float acc[K * K];
#pragma unroll
    for (int q = 0; q < K * K; ++q) acc[q] = 0.f;
    for (int e = t; e < P * plane_sz; e += 256) sm[e] = 0.f;          // the halo stays zero for every round
    for (int br = b0; br < b1; br += P) {
        const int np = b1 - br < P ? b1 - br : P;
        __syncthreads();                                               // previous round's reads are done
        for (int e = t; e < np * xsz; e += 256) {
            const int pl = e / xsz, q = e - pl * xsz, u = q / p.W, v = q - u * p.W;
            const int r = u + p.pad_t, cc = v + p.pad_l;
            if (r < PH && cc < PW) sm[pl * plane_sz + r * PW + cc] = p.x[((long)(br + pl) * p.C + c) * xsz + q];
        }
        for (int e = t; e < np * per_img; e += 256) {
            const int pl = e / per_img, q = e - pl * per_img;
            dyl[e] = p.dy[((long)(br + pl) * p.C + c) * per_img + q];
        }
        __syncthreads();
        for (int e = t; e < np * per_img; e += 256) {
            const int pl = e / per_img, q = e - pl * per_img, oy = q / p.OW, ox = q - oy * p.OW;
            const float g = dyl[e];
            const float* base = sm + pl * plane_sz + oy * p.stride * PW + ox * p.stride;
#pragma unroll
            for (int i = 0; i < K; ++i)
#pragma unroll
                for (int j = 0; j < K; ++j) acc[i * K + j] = fmaf(g, base[i * PW + j], acc[i * K + j]);
        }
    }
    __shared__ float red[4][K * K];
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int q = 0; q < K * K; ++q) {
        const float v = wave_sum(acc[q]);
        if (lane == 0) red[wave][q] = v;
    }
    __syncthreads();
    if (t < K * K) ws[((long)sp * p.C + c) * K * K + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}

__global__ void dw_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int n, int splits) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = 0.f;
    for (int s = 0; s < splits; ++s) v += ws[(long)s * n + i];
    dw[i] = v;
}

int check(const DWParams& p, int K, const char* what) {
    SRBH_REQUIRE(K == 3 || K == 5, "%s: kernel size must be 3 or 5", what);
    SRBH_REQUIRE(p.stride == 1 || p.stride == 2, "%s: stride must be 1 or 2", what);
    SRBH_REQUIRE(p.B > 0 && p.C > 0 && p.H > 0 && p.W > 0 && p.OH > 0 && p.OW > 0, "%s: bad shape", what);
    SRBH_REQUIRE(p.pad_t >= 0 && p.pad_l >= 0 && p.pad_t < K && p.pad_l < K, "%s: bad padding", what);
    // bottom/right padding implied by the output size must be a zero pad, not a crop
    SRBH_REQUIRE((p.OH - 1) * p.stride - p.pad_t + K >= p.H - (p.stride - 1) && (p.OW - 1) * p.stride - p.pad_l + K >= p.W - (p.stride - 1),
                 "%s: output size does not cover the input", what);
    return SRBH_OK;
}

constexpr size_t DW_LDS_MAX = 60 * 1024;
#ifndef DW_LDS_FORMS
#define DW_LDS_FORMS 1          // (0: the one-thread-per-output kernels, for same-box A/B builds)
#endif
// (round 6: up to 8 rounds of planes per workgroup at the tiled prediction's 49 152 planes -- fewer, longer workgroups -- measured: the encoder
//  graph 4.67 ms at one round, 4.57 at two, 4.61 at four, 4.76 at eight (profiles/r06ae_predict_parts.txt): not kept)
int lds_planes(int out_px) {     // planes a workgroup stages per round: ~256 outputs
    int P = 256 / (out_px > 0 ? out_px : 1);
    return P < 1 ? 1 : (P > 64 ? 64 : P);
}
// Geometry of a staged launch and its dynamic LDS bytes.  Forward placement: x at (pad_t, pad_l) of the padded plane, outputs step by the
// stride.  Data-gradient placement (dgrad): dy zero-upsampled at (K-1 + oy s, K-1 + ox s), dx steps by one and its taps walk backwards.
DWLds dw_geometry(const DWParams& p, int K, bool dgrad, size_t& lds) {
    const int s = p.stride;
    DWLds q;
    q.w = p.w; q.out = p.out; q.planes = (long)p.B * p.C; q.C = p.C;
    if (!dgrad) {
        q.src = p.x; q.SH = p.H; q.SW = p.W; q.OUTH = p.OH; q.OUTW = p.OW;
        q.PH = (p.OH - 1) * s + K; q.PW = (p.OW - 1) * s + K;
        q.ss = 1; q.soy = p.pad_t; q.sox = p.pad_l; q.os = s; q.by = 0; q.bx = 0;
    } else {
        q.src = p.dy; q.SH = p.OH; q.SW = p.OW; q.OUTH = p.H; q.OUTW = p.W;
        // (rows / columns of x that no output covers -- possible at stride 2 -- read the zero slack and get dx = 0)
        q.PH = (p.OH - 1) * s + 2 * (K - 1) + s + 1; q.PW = (p.OW - 1) * s + 2 * (K - 1) + s + 1;
        q.ss = s; q.soy = K - 1; q.sox = K - 1; q.os = 1; q.by = p.pad_t + K - 1; q.bx = p.pad_l + K - 1;
    }
    q.P = lds_planes(q.OUTH * q.OUTW);
    lds = (size_t)q.P * (q.PH * q.PW + K * K) * 4;
    return q;
}
dim3 lds_grid(const DWLds& q) { return dim3((unsigned)((q.planes + q.P - 1) / q.P)); }
// One 256-thread launch of the K = 3 or K = 5 instantiation of a kernel (check() has seen to K); pick(integral_constant<int, K>) names it.
template <class Pick, class... A>
int launch_k(int K, Pick pick, dim3 grid, size_t lds, void* stream, const A&... a) {
    return with_const<2>(K == 5, [&](auto k5) -> int {
        const auto kernel = pick(std::integral_constant<int, 3 + 2 * decltype(k5)::value>{});
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, (hipStream_t)stream, a...);
        SRBH_HIP(hipGetLastError());
        return SRBH_OK;
    });
}
}  // namespace

extern "C" int srbh_dwconv_fwd(const float* x, const float* w, float* y, int B, int C, int H, int W, int K, int stride, int pad_t,
                               int pad_l, int OH, int OW, void* stream) {
    SRBH_REQUIRE(x && w && y, "srbh_dwconv_fwd: null pointer");
    DWParams p{x, w, nullptr, y, B, C, H, W, OH, OW, stride, pad_t, pad_l};
    if (int rc = check(p, K, "srbh_dwconv_fwd")) return rc;
    size_t lds;
    const DWLds q = dw_geometry(p, K, false, lds);
    if (lds <= DW_LDS_MAX && DW_LDS_FORMS) return launch_k(K, [](auto k) { return dw_lds_kernel<decltype(k)::value, 0>; }, lds_grid(q), lds, stream, q);
    return launch_k(K, [](auto k) { return dw_fwd_kernel<decltype(k)::value>; }, dim3(grid_for((long)B * C * OH * OW)), 0, stream, p);
}

extern "C" int srbh_dwconv_eval_supported(int B, int C, int H, int W, int K, int stride, int pad_t, int pad_l, int OH, int OW) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || (stride != 1 && stride != 2)) return 0;
    size_t lds;
    dw_geometry(DWParams{nullptr, nullptr, nullptr, nullptr, B, C, H, W, OH, OW, stride, pad_t, pad_l}, K, false, lds);
    return lds <= DW_LDS_MAX && (K == 3 || K == 5);
}

extern "C" int srbh_dwconv_eval_fwd(const float* x, const float* w, const float* pre_scale, const float* pre_shift, const float* scale,
                                    const float* shift, float* y, float* pooled, int B, int C, int H, int W, int K, int stride, int pad_t,
                                    int pad_l, int OH, int OW, void* stream) {
    SRBH_REQUIRE(x && w && scale && shift && y && pooled, "srbh_dwconv_eval_fwd: null pointer");
    SRBH_REQUIRE((pre_scale == nullptr) == (pre_shift == nullptr), "srbh_dwconv_eval_fwd: pre_scale and pre_shift go together");
    DWParams p{x, w, nullptr, y, B, C, H, W, OH, OW, stride, pad_t, pad_l};
    if (int rc = check(p, K, "srbh_dwconv_eval_fwd")) return rc;
    size_t lds;
    const DWLds q = dw_geometry(p, K, false, lds);
    SRBH_REQUIRE(lds <= DW_LDS_MAX, "srbh_dwconv_eval_fwd: plane too large for the LDS-staged form (srbh_dwconv_eval_supported)");
    DWEval e{pre_scale, pre_shift, scale, shift, pooled, 1};
    while (e.G < OH * OW && e.G < 256) e.G <<= 1;
    return launch_k(K, [](auto k) { return dw_lds_eval_kernel<decltype(k)::value>; }, lds_grid(q), lds, stream, q, e);
}

extern "C" int srbh_dwconv_bwd_data(const float* dy, const float* w, float* dx, int B, int C, int H, int W, int K, int stride,
                                    int pad_t, int pad_l, int OH, int OW, void* stream) {
    SRBH_REQUIRE(dy && w && dx, "srbh_dwconv_bwd_data: null pointer");
    DWParams p{nullptr, w, dy, dx, B, C, H, W, OH, OW, stride, pad_t, pad_l};
    if (int rc = check(p, K, "srbh_dwconv_bwd_data")) return rc;
    size_t lds;
    const DWLds q = dw_geometry(p, K, true, lds);
    if (lds <= DW_LDS_MAX && DW_LDS_FORMS && H - 1 + pad_t + K - 1 < q.PH && W - 1 + pad_l + K - 1 < q.PW)
        return launch_k(K, [](auto k) { return dw_lds_kernel<decltype(k)::value, 1>; }, lds_grid(q), lds, stream, q);
    return launch_k(K, [](auto k) { return dw_bwd_data_kernel<decltype(k)::value>; }, dim3(grid_for((long)B * C * H * W)), 0, stream, p);
}

extern "C" int srbh_dwconv_bwd_weight_splits(int B, int C) {
    int s = (1024 + C - 1) / (C > 0 ? C : 1);
    if (s > B) s = B;
    return s < 1 ? 1 : s;
}

extern "C" int srbh_dwconv_bwd_weight(const float* x, const float* dy, float* dw, float* ws, int B, int C, int H, int W, int K,
                                      int stride, int pad_t, int pad_l, int OH, int OW, void* stream) {
    SRBH_REQUIRE(x && dy && dw && ws, "srbh_dwconv_bwd_weight: null pointer");
    DWParams p{x, nullptr, dy, dw, B, C, H, W, OH, OW, stride, pad_t, pad_l};
    if (int rc = check(p, K, "srbh_dwconv_bwd_weight")) return rc;
    const int splits = srbh_dwconv_bwd_weight_splits(B, C);
    const int PH = (OH - 1) * stride + K, PW = (OW - 1) * stride + K, P = lds_planes(OH * OW);
    const size_t lds = (size_t)P * (PH * PW + OH * OW) * 4;
    float* const part = splits == 1 ? dw : ws;                       // (one slice: its sums ARE the gradient, no reduce launch)
    // (the staged form pays for 5x5 and for small planes; a 3x3 over >= 256-pixel planes is as fast from L1: measured per shape)
    const int rc = lds <= DW_LDS_MAX && DW_LDS_FORMS && (K == 5 || OH * OW < 256)
                       ? launch_k(K, [](auto k) { return dw_lds_wgrad_kernel<decltype(k)::value>; }, dim3(C, splits), lds, stream, p, part, splits, PH, PW, P)
                       : launch_k(K, [](auto k) { return dw_bwd_weight_kernel<decltype(k)::value>; }, dim3(C, splits), 0, stream, p, part, splits);
    if (rc || splits == 1) return rc;
    const int n = C * K * K;
    hipLaunchKernelGGL(dw_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, ws, dw, n, splits);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
