// srbh_head_bwd.hip -- backward kernels of the HR feature / fusion head (training: SURVEY.md 3.1, train.py:254-256).
//
// The reference gets these from torch autograd over SR/HRfuse.py; here each is a hand-written gfx950 kernel:
//  * weight gradients of the 3x3 / 1x1 convs as a GEMM over pixels, dW[oc][ci][tap] = sum_px dY[px][oc] * X[px + tap][ci], X read with
//    the same concat / folded BN+ReLU transform as the forward conv:
//      - hwgrad_f32_kernel (here): fp32 matrix cores (v_mfma_f32_16x16x4_f32, K = 4 pixels), any channel counts;
//      - srbh_hwgrad_b16_kernel.h: the bf16-operand kernels on 8 x 64 tiles (hwgrad_b16_kernel, hwgrad_entry_b16_kernel,
//        hwgrad_ob_b16_kernel, hwgrad_entry64_b16_kernel) and the walk / staging / tap / flush pieces they share;
//      - srbh_hwgrad16_kernel.h: the double-buffered 16 -> 16 kernel; srbh_hbwd16_kernel.h: that layer's data and weight gradient
//        behind its BatchNorm backward in one pass;
//    every workgroup stores its partial sums, the reduce kernels here add them in a fixed order (now, or batched: srbh_hwgrad_defer);
//  * the host side of those: WGParams fillers, the kernel-form selection and launch of every weight-gradient entry point;
//  * data gradients reuse the forward conv kernel (srbh_hconv_f32) with transposed + flipped weights
//    (srbh_hpack_conv_f32(transpose_flip=1)).
//  * BatchNorm backward in three steps: per-channel reductions (sum dy, sum dy*xhat) -> per-channel constants ->
//    dc = gamma*invstd * (dy - mean(dy) - xhat * mean(dy*xhat)); the ReLU mask of the block is applied on the fly.
//  * small elementwise helpers: relu mask, in-place add, per-channel sum (bias grad), PixelShuffle(2) inverse.
#include "srbh_internal.h"
#include "srbh_head_walk.h"

#include <type_traits>
#include <vector>
#include <algorithm>

namespace {
using namespace srbh;

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float float2w __attribute__((ext_vector_type(2)));
typedef _Float16 half4w __attribute__((ext_vector_type(4)));
constexpr int HT_H = 8, HT_W = 64;
constexpr int NSLOT = 64;
constexpr int WS_SLOTS = 768;                  // per-workgroup partial-sum slots of the weight-gradient workspace (max grid.x)

struct WGParams {
    const float* src0; const float* src1;
    int c0, c1;
    const float* pre_scale; const float* pre_shift;
    int pre_relu;
    const float* dy;      // NHWC [B][H][W][cout_total]
    int cout_total;
    float* dw;            // OIHW fp32 [cout_total][cin][KS][KS]
    float* ws;            // [gridDim.x][nob][nchunk][TAPS*256] per-workgroup partial sums (hwgrad_reduce_kernel adds them)
    int B, H, W;
    int tiles_x, tiles_per_img, ntiles, tiles_per_xcd;
    int ld0, ld1;         // pixel strides (floats) of src0 / src1
    int io;               // SRBH_WG_SRC0_H16: src0 holds fp16 elements; SRBH_WG_DY_B16: dy holds bf16 elements (16-bit forms only)
    // ACT16 addressing (hwgrad_b16_kernel<.., XM = 1>, srbh_act16_wgrad_b16: the RRDBNet training path): src0 = fp16 chunk planes
    // [B][chunks][H+2][W+2][32] (channel ch lives in plane ch / 32), dy = bf16 chunk planes starting at channel dy_ch0
    long x_img_b, dy_img_b;
    int x_plane_b, x_row_b, dy_plane_b, dy_row_b, dy_ch0;
    int zchunk;           // 1: the 16-channel input chunk is blockIdx.z (few tiles per launch: one (tile set, oc block, chunk) per workgroup)
    // fused block-entry form (hwgrad_b16_kernel<3, DS, 0, 1>): the 1x1 downsample conv's dY over the SAME input -- one more accumulator on
    // the centre-tap fragment; its partial sums go to ws2 (layout of a ksize = 1 call)
    const float* dy2; float* ws2;
};

// 4 elements of a 16-bit tensor (raw bits in a float2w) -> fp32: fp16 activations / bf16 gradients
__device__ __forceinline__ floatx4 widen_h4(const float2w raw) {
    const half4w h = __builtin_bit_cast(half4w, raw);
    return floatx4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}
// (bit casts go through WHOLE vectors: __builtin_bit_cast of one ext-vector element -- bit_cast(unsigned, v[j]) -- returned element 0
//  for every j with this hipcc: every quad came back as (e0, e1, e0, e1).  Found by tools/io16_unit.py; now a test.)
typedef unsigned uint2q __attribute__((ext_vector_type(2)));
typedef unsigned uint4q __attribute__((ext_vector_type(4)));
__device__ __forceinline__ floatx4 widen_b4(const float2w raw) {
    const uint2q rw = __builtin_bit_cast(uint2q, raw);
    const unsigned lo = rw[0], hi = rw[1];
    return floatx4{__builtin_bit_cast(float, lo << 16), __builtin_bit_cast(float, lo & 0xffff0000u),
                   __builtin_bit_cast(float, hi << 16), __builtin_bit_cast(float, hi & 0xffff0000u)};
}
__device__ __forceinline__ float2w narrow_b4(const floatx4 v) {      // fp32 -> bf16 (RNE), 4 elements as raw bits
    const uint2q o = {bf16x2_rne(v[0], v[1]), bf16x2_rne(v[2], v[3])};
    return __builtin_bit_cast(float2w, o);
}
// the 16-bit element j (0..3) of two raw quads a, b -> one dword (a's element in the low half)
__device__ __forceinline__ unsigned b16_field_pair(const float2w a, const float2w b, const int j) {
    const uint2q ua = __builtin_bit_cast(uint2q, a), ub = __builtin_bit_cast(uint2q, b);
    const unsigned wa = ua[j >> 1], wb = ub[j >> 1];
    return (j & 1) ? ((wa >> 16) | (wb & 0xffff0000u)) : ((wa & 0xffffu) | (wb << 16));
}

#include "srbh_hwgrad_b16_kernel.h"

// One workgroup walks tiles t = blockIdx.x, +gridDim.x, ... and keeps the 16(oc) x 16(ci) x taps partial sums of
// one (oc block = blockIdx.y, ci chunk) in registers; flushed once per chunk through LDS with one atomic per value.
template <int KS>
__global__ __launch_bounds__(256) void hwgrad_f32_kernel(const WGParams p) {
    extern __shared__ __attribute__((aligned(16))) float wsm[];
    constexpr int TAPS = KS * KS, HALO = KS / 2;
    constexpr int ROWS = HT_H + 2 * HALO, COLS = HT_W + 2 * HALO;
    float* s_x = wsm;                          // [ROWS*COLS][16]
    float* s_dy = wsm + ROWS * COLS * 16;      // [8*64][16]
    float* s_red = s_dy;                       // reused for the cross-wave reduction at flush time
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kk = lane >> 4;
    const int cin = p.c0 + p.c1;
    const int nchunk = (cin + 15) / 16;
    const int ob = blockIdx.y;
    const bool vec0 = (p.c0 & 3) == 0 && (p.ld0 & 3) == 0, vec1 = p.c1 > 0 && (p.c1 & 3) == 0 && (p.c0 & 3) == 0 && (p.ld1 & 3) == 0;

    for (int c = 0; c < nchunk; ++c) {
        floatx4 acc[TAPS];
#pragma unroll
        for (int tp = 0; tp < TAPS; ++tp) acc[tp] = floatx4{0.f, 0.f, 0.f, 0.f};
        floatx4 acc2 = {0.f, 0.f, 0.f, 0.f};
        // XCD-aware walk (explained in srbh_head_walk.h; written out here: with head_walk / head_tile this kernel's instructions change,
        // profiles/head_launch_path_isa.txt)
        const int t_end = min((int)(blockIdx.x & 7) * p.tiles_per_xcd + p.tiles_per_xcd, p.ntiles);
        for (int t = (blockIdx.x & 7) * p.tiles_per_xcd + (blockIdx.x >> 3); t < t_end; t += gridDim.x >> 3) {
            const int img = t / p.tiles_per_img;
            const int trem = t - img * p.tiles_per_img;
            const int ty = trem / p.tiles_x, tx = trem - ty * p.tiles_x;
            const int Y0 = ty * HT_H, X0 = tx * HT_W;
            __syncthreads();
            // Fast path (all 4-channel groups are aligned 16-byte loads): every global load of the tile pair is issued
            // before the first LDS store; the one-load-per-iteration loops below expose one memory latency per
            // iteration (19 per tile) and made the kernel staging-latency bound.
            constexpr int NIX = (ROWS * COLS * 4 + 255) / 256, NID = HT_H * HT_W * 4 / 256;
            const bool fast = vec0 && (p.c1 == 0 || vec1) && (cin & 3) == 0 && (p.cout_total & 3) == 0 &&
                              ob * 16 + 15 < p.cout_total;
            if (fast) {
                floatx4 lx[NIX], ld[NID];
#pragma unroll
                for (int it = 0; it < NIX; ++it) {
                    const int u = tid + it * 256;
                    lx[it] = floatx4{0.f, 0.f, 0.f, 0.f};
                    if (u < ROWS * COLS * 4) {
                        const int cg = u & 3, pix = u >> 2;
                        const int r = pix / COLS, col = pix - r * COLS;
                        const int y = Y0 + r - HALO, x = X0 + col - HALO;
                        const int ch = c * 16 + cg * 4;
                        if (y >= 0 && y < p.H && x >= 0 && x < p.W && ch < cin) {
                            const long pixi = ((long)img * p.H + y) * p.W + x;
                            if (ch < p.c0) {
                                floatx4 a = *(const floatx4*)(p.src0 + pixi * p.ld0 + ch);
                                if (p.pre_scale) a = a * *(const floatx4*)(p.pre_scale + ch) + *(const floatx4*)(p.pre_shift + ch);
                                if (p.pre_relu) {
#pragma unroll
                                    for (int j = 0; j < 4; ++j) a[j] = fmaxf(a[j], 0.f);
                                }
                                lx[it] = a;
                            } else {
                                lx[it] = *(const floatx4*)(p.src1 + pixi * p.ld1 + (ch - p.c0));
                            }
                        }
                    }
                }
#pragma unroll
                for (int it = 0; it < NID; ++it) {
                    const int u = tid + it * 256;
                    const int cg = u & 3, pix = u >> 2;
                    const int y = Y0 + (pix >> 6), x = X0 + (pix & 63);
                    ld[it] = floatx4{0.f, 0.f, 0.f, 0.f};
                    if (y < p.H && x < p.W)
                        ld[it] = *(const floatx4*)(p.dy + (((long)img * p.H + y) * p.W + x) * p.cout_total + ob * 16 + cg * 4);
                }
#pragma unroll
                for (int it = 0; it < NIX; ++it) {
                    const int u = tid + it * 256;
                    if (u < ROWS * COLS * 4) *(floatx4*)(s_x + (u >> 2) * 16 + (u & 3) * 4) = lx[it];
                }
#pragma unroll
                for (int it = 0; it < NID; ++it) {
                    const int u = tid + it * 256;
                    *(floatx4*)(s_dy + (u >> 2) * 16 + (u & 3) * 4) = ld[it];
                }
            } else {
            for (int u = tid; u < ROWS * COLS * 4; u += 256) {   // X tile, pixel-major, 4 channels per thread
                const int cg = u & 3, pix = u >> 2;
                const int r = pix / COLS, col = pix - r * COLS;
                const int y = Y0 + r - HALO, x = X0 + col - HALO;
                const int ch = c * 16 + cg * 4;
                floatx4 v = {0.f, 0.f, 0.f, 0.f};
                if (y >= 0 && y < p.H && x >= 0 && x < p.W && ch < cin) {
                    const long pixi = ((long)img * p.H + y) * p.W + x;
                    if (vec0 && ch + 3 < p.c0) {
                        floatx4 a = *(const floatx4*)(p.src0 + pixi * p.ld0 + ch);
                        if (p.pre_scale) a = a * *(const floatx4*)(p.pre_scale + ch) + *(const floatx4*)(p.pre_shift + ch);
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = p.pre_relu ? fmaxf(a[j], 0.f) : a[j];
                    } else if (vec1 && ch >= p.c0 && ch + 3 < cin) {
                        v = *(const floatx4*)(p.src1 + pixi * p.ld1 + (ch - p.c0));
                    } else
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int cc = ch + j;
                        if (cc < p.c0) {
                            float a = p.src0[pixi * p.ld0 + cc];
                            if (p.pre_scale) a = a * p.pre_scale[cc] + p.pre_shift[cc];
                            if (p.pre_relu) a = fmaxf(a, 0.f);
                            v[j] = a;
                        } else if (cc < cin) {
                            v[j] = p.src1[pixi * p.ld1 + (cc - p.c0)];
                        }
                    }
                }
                *(floatx4*)(s_x + pix * 16 + cg * 4) = v;
            }
            for (int u = tid; u < HT_H * HT_W * 4; u += 256) {   // dY tile (16 channels of block `ob`)
                const int cg = u & 3, pix = u >> 2;
                const int r = pix >> 6, col = pix & 63;
                const int y = Y0 + r, x = X0 + col;
                floatx4 v = {0.f, 0.f, 0.f, 0.f};
                if (y < p.H && x < p.W) {
                    const float* s = p.dy + (((long)img * p.H + y) * p.W + x) * p.cout_total + ob * 16 + cg * 4;
                    if ((p.cout_total & 3) == 0 && ob * 16 + cg * 4 + 3 < p.cout_total) {
                        v = *(const floatx4*)s;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (ob * 16 + cg * 4 + j < p.cout_total) v[j] = s[j];
                    }
                }
                *(floatx4*)(s_dy + pix * 16 + cg * 4) = v;
            }
            }
            __syncthreads();
            // 2 rows x 16 groups of 4 pixels per wave; the operands of k-step ks+1 are read while the MFMAs of ks run
            float a_cur, b_cur[TAPS];
            auto fetch = [&](const int ks, float& a, float (&b)[TAPS]) {
                const int row = wave * 2 + (ks >> 4), col = (ks & 15) * 4 + kk;
                a = s_dy[(row * 64 + col) * 16 + l15];                     // A[oc = l15][k = kk]
                // one base address per k-step, the taps are immediate offsets of the LDS reads (left to the compiler, every
                // tap's address was rebuilt with 3 VALU instructions: 25 per 9 MFMAs)
                const float* bp = s_x + (row * COLS + col) * 16 + l15;
#pragma unroll
                for (int tp = 0; tp < TAPS; ++tp) {
                    const int dy = tp / KS, dx = tp - dy * KS;
                    b[tp] = bp[(dy * COLS + dx) * 16];                     // B[k = kk][ci = l15]
                }
            };
            fetch(0, a_cur, b_cur);
#pragma unroll 2
            for (int ks = 0; ks < 32; ++ks) {
                float a_nxt, b_nxt[TAPS];
                fetch(ks + 1 < 32 ? ks + 1 : ks, a_nxt, b_nxt);
#pragma unroll
                for (int tp = 0; tp < TAPS; ++tp) acc[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_cur, b_cur[tp], acc[tp], 0, 0, 0);
                a_cur = a_nxt;
#pragma unroll
                for (int tp = 0; tp < TAPS; ++tp) b_cur[tp] = b_nxt[tp];
            }
        }
        // flush: D[row = oc = kk*4 + r][col = ci = l15]
        __syncthreads();
#pragma unroll
        for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
            for (int r = 0; r < 4; ++r) s_red[((wave * TAPS + tp) * 16 + kk * 4 + r) * 16 + l15] = acc[tp][r];
        __syncthreads();
        for (int u = tid; u < TAPS * 256; u += 256) {
            const float v = s_red[u] + s_red[TAPS * 256 + u] + s_red[2 * TAPS * 256 + u] + s_red[3 * TAPS * 256 + u];
            // no atomics: 512 workgroups adding into the same 2 304 addresses cost 60 us of a 318 us layer (and made the
            // gradient order-dependent); every workgroup stores its partial, a second tiny kernel adds them in order
            p.ws[(((long)blockIdx.x * gridDim.y + ob) * nchunk + c) * (TAPS * 256) + u] = v;
        }
    }
}

#include "srbh_hwgrad16_kernel.h"
#include "srbh_hbwd16_kernel.h"

// Sum of the workgroups' partials in a fixed order (deterministic), two stages so that enough loads are in flight:
//   stage 1: tmp[s][u] = sum of the partials x in slice s (x = s*per .. s*per+per-1), grid (U/256, slices);
//   stage 2: dw[oc][ci][tap] = sum over s of tmp[s][u(oc, ci, tap)]
__global__ __launch_bounds__(256) void hwgrad_reduce1_kernel(const float* __restrict__ ws, float* __restrict__ tmp, long U, int gx, int per) {
    const long u = (long)blockIdx.x * 256 + threadIdx.x;
    if (u >= U) return;
    const int x0 = blockIdx.y * per;
    const int x1 = x0 + per < gx ? x0 + per : gx;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int x = x0;
    for (; x + 3 < x1; x += 4) {
        a0 += ws[(long)x * U + u];
        a1 += ws[(long)(x + 1) * U + u];
        a2 += ws[(long)(x + 2) * U + u];
        a3 += ws[(long)(x + 3) * U + u];
    }
    for (; x < x1; ++x) a0 += ws[(long)x * U + u];
    tmp[(long)blockIdx.y * U + u] = (a0 + a1) + (a2 + a3);
}

__global__ void hwgrad_reduce2_kernel(const float* __restrict__ tmp, float* __restrict__ dw, long U, int slices, int nchunk, int taps,
                                      int cout, int cin) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int total = cout * cin * taps;
    if (idx >= total) return;
    const int tp = idx % taps;
    const int ci = (idx / taps) % cin;
    const int oc = idx / (taps * cin);
    const long u = ((long)(oc >> 4) * nchunk + (ci >> 4)) * (taps * 256) + tp * 256 + (oc & 15) * 16 + (ci & 15);
    float v = 0.f;
    for (int sidx = 0; sidx < slices; ++sidx) v += tmp[(long)sidx * U + u];
    dw[idx] = v;
}

// ---- the same two stages for SEVERAL weight gradients in one launch each (round 5).  The partial sums of a weight gradient are not needed
// before the optimizer (or a gradient all-reduce) reads dW, so the producers of one autograd node's backward can queue their reduce jobs
// (srbh_hwgrad_defer) and ONE pair of launches does them all (srbh_hwgrad_flush): in the training step these 2 x 28 launches of ~6 us each sat
// between the chip-filling kernels of the head's backward.  Same order of additions per element as the per-gradient kernels.
struct RedJob {
    const float* ws; float* tmp; float* dw;
    long U;
    int gx, nchunk, taps, cout, cin, per;
};
constexpr int RED_MAX = 24;
struct RedMany { RedJob j[RED_MAX]; int n; };
__global__ __launch_bounds__(256) void hwgrad_reduce1_many_kernel(const RedMany m) {
    const RedJob& J = m.j[blockIdx.z];
    const long u = (long)blockIdx.x * 256 + threadIdx.x;
    if (u >= J.U) return;
    const int x0 = blockIdx.y * J.per;
    const int x1 = x0 + J.per < J.gx ? x0 + J.per : J.gx;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int x = x0;
    for (; x + 3 < x1; x += 4) {
        a0 += J.ws[(long)x * J.U + u];
        a1 += J.ws[(long)(x + 1) * J.U + u];
        a2 += J.ws[(long)(x + 2) * J.U + u];
        a3 += J.ws[(long)(x + 3) * J.U + u];
    }
    for (; x < x1; ++x) a0 += J.ws[(long)x * J.U + u];
    J.tmp[(long)blockIdx.y * J.U + u] = (a0 + a1) + (a2 + a3);
}
__global__ __launch_bounds__(256) void hwgrad_reduce2_many_kernel(const RedMany m, int slices) {
    const RedJob& J = m.j[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int total = J.cout * J.cin * J.taps;
    if (idx >= total) return;
    const int tp = idx % J.taps;
    const int ci = (idx / J.taps) % J.cin;
    const int oc = idx / (J.taps * J.cin);
    const long u = ((long)(oc >> 4) * J.nchunk + (ci >> 4)) * (J.taps * 256) + tp * 256 + (oc & 15) * 16 + (ci & 15);
    float v = 0.f;
    for (int sidx = 0; sidx < slices; ++sidx) v += J.tmp[(long)sidx * J.U + u];
    J.dw[idx] = v;
}
constexpr int RED_SLICES = 16;
thread_local bool g_red_defer = false;
thread_local std::vector<RedJob> g_red_queue;
int reduce_flush(hipStream_t st) {
    for (size_t b = 0; b < g_red_queue.size(); b += RED_MAX) {
        RedMany m = {};
        m.n = (int)std::min<size_t>(RED_MAX, g_red_queue.size() - b);
        long umax = 0;
        int tmax = 0;
        for (int k = 0; k < m.n; ++k) {
            m.j[k] = g_red_queue[b + k];
            umax = std::max(umax, m.j[k].U);
            tmax = std::max(tmax, m.j[k].cout * m.j[k].cin * m.j[k].taps);
        }
        hipLaunchKernelGGL(hwgrad_reduce1_many_kernel, dim3((unsigned)((umax + 255) / 256), RED_SLICES, m.n), dim3(256), 0, st, m);
        SRBH_HIP(hipGetLastError());
        hipLaunchKernelGGL(hwgrad_reduce2_many_kernel, dim3((tmax + 255) / 256, m.n), dim3(256), 0, st, m, RED_SLICES);
        SRBH_HIP(hipGetLastError());
    }
    g_red_queue.clear();
    return SRBH_OK;
}
// the two-stage ordered reduce of one weight gradient: now, or queued for srbh_hwgrad_flush
int reduce_partials(const float* ws, float* dw, long U, int gx, int nchunk, int taps, int cout, int cin, hipStream_t st) {
    float* tmp = (float*)ws + (long)WS_SLOTS * U;
    const int per = (gx + RED_SLICES - 1) / RED_SLICES;
    if (g_red_defer) {
        g_red_queue.push_back(RedJob{ws, tmp, dw, U, gx, nchunk, taps, cout, cin, per});
        return SRBH_OK;
    }
    hipLaunchKernelGGL(hwgrad_reduce1_kernel, dim3((unsigned)((U + 255) / 256), RED_SLICES), dim3(256), 0, st, ws, tmp, U, gx, per);
    SRBH_HIP(hipGetLastError());
    const int total = cout * cin * taps;
    hipLaunchKernelGGL(hwgrad_reduce2_kernel, dim3((total + 255) / 256), dim3(256), 0, st, tmp, dw, U, RED_SLICES, nchunk, taps, cout, cin);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

// one-stage form for few partial slots (gx <= 128: small batches, where the two-stage form is two launch latencies for 28 MB of L2 reads):
// dw[oc][ci][tap] = sum over x = 0 .. gx-1 of ws[x][u], in that fixed order
__global__ void hwgrad_reduce_direct_kernel(const float* __restrict__ ws, float* __restrict__ dw, long U, int gx, int nchunk, int taps, int cout,
                                            int cin) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int total = cout * cin * taps;
    if (idx >= total) return;
    const int tp = idx % taps;
    const int ci = (idx / taps) % cin;
    const int oc = idx / (taps * cin);
    const long u = ((long)(oc >> 4) * nchunk + (ci >> 4)) * (taps * 256) + tp * 256 + (oc & 15) * 16 + (ci & 15);
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // 8 loads in flight; the order of the additions is fixed all the same
    int x = 0;
    for (; x + 8 <= gx; x += 8) {
        float t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) t[k] = ws[(long)(x + k) * U + u];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] += t[k];
    }
    for (; x < gx; ++x) v[0] += ws[(long)x * U + u];
    dw[idx] = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}

// ---- elementwise / reduction helpers (NHWC fp32, C % 4 == 0 unless noted) ------------------------------------------
__global__ void relu_mask_mul_kernel(const floatx4* __restrict__ g, const floatx4* __restrict__ ref, floatx4* out, long n4) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    for (; i < n4; i += stride) {
        floatx4 a = g[i], r = ref[i];
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = r[q] > 0.f ? a[q] : 0.f;
        out[i] = a;
    }
}

__global__ void add_inplace_kernel(floatx4* a, const floatx4* __restrict__ b, long n4) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    for (; i < n4; i += stride) a[i] += b[i];
}

// per-channel sums of dy (and dy*xhat when c != nullptr); dy = g * [c*ms+mh > 0] when ms != nullptr.
// generic C (scalar loads); block = 256 threads over pixels, thread handles all channels of a pixel subset
__global__ void bn_bwd_reduce_kernel(const float* __restrict__ g, const float* __restrict__ c, const float* mean,
                                     const float* invstd, const float* ms, const float* mh, long npix, int C,
                                     double* stats /* [NSLOT][2][C] */) {
    extern __shared__ float red[];   // [2][C]
    for (int k = threadIdx.x; k < 2 * C; k += blockDim.x) red[k] = 0.f;
    __syncthreads();
    // thread layout: channel = threadIdx.x % C (C <= 64 divides 256 or not: use modulo walk over flat index)
    long total = npix * C;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    // stride is a multiple of C when C divides blockDim.x*gridDim.x; otherwise accumulate per element via LDS atomics
    const bool fixed = (stride % C) == 0;
    float s = 0.f, q = 0.f;
    int ch = (int)(i % C);
    for (; i < total; i += stride) {
        if (!fixed) ch = (int)(i % C);
        float dy = g[i];
        float cv = c ? c[i] : 0.f;
        if (ms && !(cv * ms[ch] + mh[ch] > 0.f)) dy = 0.f;
        const float xh = c ? (cv - mean[ch]) * invstd[ch] : 0.f;
        if (fixed) {
            s += dy;
            q += dy * xh;
        } else {
            atomicAdd(&red[ch], dy);
            atomicAdd(&red[C + ch], dy * xh);
        }
    }
    if (fixed) {
        atomicAdd(&red[ch], s);
        atomicAdd(&red[C + ch], q);
    }
    __syncthreads();
    double* slot = stats + (long)(blockIdx.x % NSLOT) * 2 * C;
    for (int k = threadIdx.x; k < 2 * C; k += blockDim.x) atomicAdd(slot + k, (double)red[k]);
}

// per-channel constants of the BatchNorm backward: dgamma, dbeta and (coef, k1, k2) with
// dc = coef * (dy - k1 - xhat * k2);   training: coef = gamma*invstd, k1 = sum(dy)/N, k2 = sum(dy*xhat)/N
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(double* stats, int C, double count, const float* gamma, const float* invstd,
                                       float* dgamma, float* dbeta, float* coef, float* k1, float* k2, int clear) {
    __shared__ double red[256];
    double s = 0, q = 0;
    srbh::fold_stat_slots(stats, C, clear, red, s, q);   // (one block of 256 threads, C <= 64; clear: the slots are zeroed behind the read)
    const int c = threadIdx.x;
    if (c >= C) return;
    if (dgamma) dgamma[c] = (float)q;
    if (dbeta) dbeta[c] = (float)s;
    if (coef) {
        coef[c] = (gamma ? gamma[c] : 1.f) * invstd[c];
        k1[c] = (float)(s / count);
        k2[c] = (float)(q / count);
    }
}

__global__ void bn_bwd_apply_kernel(const float* __restrict__ g, const float* __restrict__ c, const float* mean,
                                    const float* invstd, const float* ms, const float* mh, const float* coef,
                                    const float* k1, const float* k2, float* out, long total, int C) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        const int ch = (int)(i % C);
        float dy = g[i];
        const float cv = c[i];
        if (ms && !(cv * ms[ch] + mh[ch] > 0.f)) dy = 0.f;
        const float xh = (cv - mean[ch]) * invstd[ch];
        out[i] = coef[ch] * (dy - k1[ch] - xh * k2[ch]);
    }
}

// ---- 16-byte forms of the two BatchNorm-backward passes (C % 4 == 0: every head layer).  A thread owns the 4-channel group
// (flat index % (C/4)) of the pixels it walks, its per-channel constants live in registers, partial sums are flushed once per thread.
// `relu_ref` / `dz_out` fold the block-closing ReLU backward into the reduce pass (dz = g where ref > 0; it is written for the
// skip / downsample branches and read back by the apply pass): one 3-tensor elementwise launch per BasicBlock less.
// 16-bit tensors in memory (round 3; template flags): GB = g holds bf16 elements, CH = c holds fp16 elements, OB = dz_out / out is written
// as bf16.  One 4-channel group is then an 8-byte access; the arithmetic stays fp32.
template <int B16, typename T>
__device__ __forceinline__ floatx4 ld4(const T* base, const long i) {
    if constexpr (B16 == 0) return ((const floatx4*)base)[i];
    else if constexpr (B16 == 1) return widen_h4(((const float2w*)base)[i]);
    else return widen_b4(((const float2w*)base)[i]);
}
// RB = 1: relu_ref is the ReLU's activity bit pattern written by bn_add_relu (4 words per 64 groups) instead of the fp32 block output
template <int GB, int CH, int OB, int RB = 0>
__global__ __launch_bounds__(256) void bn_bwd_reduce4_kernel(const void* __restrict__ g, const void* __restrict__ c, const float* mean,
                                                              const float* invstd, const float* ms, const float* mh,
                                                              const floatx4* __restrict__ relu_ref, void* __restrict__ dz_out,
                                                              long n4, int C, double* stats /* [NSLOT][2][C] */) {
    extern __shared__ float red[];   // [2][C]
    for (int k = threadIdx.x; k < 2 * C; k += blockDim.x) red[k] = 0.f;
    __syncthreads();
    const int C4 = C >> 2;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;          // host: a multiple of C/4 -> the channel group is fixed per thread
    const int ch = (int)(i % C4) * 4;
    floatx4 mn = {0.f, 0.f, 0.f, 0.f}, is = mn, msv = mn, mhv = mn;
    if (c) { mn = *(const floatx4*)(mean + ch); is = *(const floatx4*)(invstd + ch); }
    if (ms) { msv = *(const floatx4*)(ms + ch); mhv = *(const floatx4*)(mh + ch); }
    floatx4 s = {0.f, 0.f, 0.f, 0.f}, q = s;
    for (; i < n4; i += stride) {
        floatx4 dy = ld4<GB ? 2 : 0>(g, i);
        if (relu_ref) {
            if constexpr (RB != 0) {
                const unsigned long long* mw = (const unsigned long long*)relu_ref + (i >> 6) * 4;
                const int sh = (int)(i & 63);
#pragma unroll
                for (int j = 0; j < 4; ++j) dy[j] = ((mw[j] >> sh) & 1ull) ? dy[j] : 0.f;
            } else {
                const floatx4 r = relu_ref[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) dy[j] = r[j] > 0.f ? dy[j] : 0.f;
            }
            if (dz_out) {
                if constexpr (OB != 0) {
                    const float2w nb = narrow_b4(dy);
                    ((float2w*)dz_out)[i] = nb;
                    dy = widen_b4(nb);          // the sums are taken over the values the consumers will read
                } else {
                    ((floatx4*)dz_out)[i] = dy;
                }
            }
        }
        if (c) {
            const floatx4 cv = ld4<CH ? 1 : 0>(c, i);
            if (ms) {
#pragma unroll
                for (int j = 0; j < 4; ++j) dy[j] = cv[j] * msv[j] + mhv[j] > 0.f ? dy[j] : 0.f;
            }
            q += dy * ((cv - mn) * is);
        }
        s += dy;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        atomicAdd(&red[ch + j], s[j]);
        atomicAdd(&red[C + ch + j], q[j]);
    }
    __syncthreads();
    double* slot = stats + (long)(blockIdx.x % NSLOT) * 2 * C;
    for (int k = threadIdx.x; k < 2 * C; k += blockDim.x) atomicAdd(slot + k, (double)red[k]);
}

template <int GB, int CH, int OB>
__global__ __launch_bounds__(256) void bn_bwd_apply4_kernel(const void* __restrict__ g, const void* __restrict__ c, const float* mean,
                                                             const float* invstd, const float* ms, const float* mh, const float* coef,
                                                             const float* k1, const float* k2, void* __restrict__ out, long n4, int C) {
    const int C4 = C >> 2;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    const int ch = (int)(i % C4) * 4;
    const floatx4 mn = *(const floatx4*)(mean + ch), is = *(const floatx4*)(invstd + ch), cf = *(const floatx4*)(coef + ch),
                  a1 = *(const floatx4*)(k1 + ch), a2 = *(const floatx4*)(k2 + ch);
    floatx4 msv = {0.f, 0.f, 0.f, 0.f}, mhv = msv;
    if (ms) { msv = *(const floatx4*)(ms + ch); mhv = *(const floatx4*)(mh + ch); }
    for (; i < n4; i += stride) {
        floatx4 dy = ld4<GB ? 2 : 0>(g, i);
        const floatx4 cv = ld4<CH ? 1 : 0>(c, i);
        if (ms) {
#pragma unroll
            for (int j = 0; j < 4; ++j) dy[j] = cv[j] * msv[j] + mhv[j] > 0.f ? dy[j] : 0.f;
        }
        const floatx4 r = cf * (dy - a1 - ((cv - mn) * is) * a2);
        if constexpr (OB != 0) ((float2w*)out)[i] = narrow_b4(r);
        else ((floatx4*)out)[i] = r;
    }
}

// grid for the 16-byte forms: a multiple of C/4 threads in total (blockDim 256, C/4 in {1, 2, 4, 8, 16} divides it)
int grid4_for(long n4) {
    long b = (n4 + 255) / 256;
    return (int)(b < 2048 ? (b > 0 ? b : 1) : 2048);
}

// PixelShuffle(2) inverse: g_ps [B][2H][2W][C] -> g [B][H][W][4C], channel 4c + 2i + j <- (2y+i, 2x+j, c)
__global__ void ps2_inverse_kernel(const float* __restrict__ gps, float* __restrict__ g, int B, int H, int W, int C) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)B * H * W * 4 * C;
    if (idx >= total) return;
    int oc = idx % (4 * C);
    long r = idx / (4 * C);
    int x = r % W; r /= W;
    int y = r % H;
    int b = r / H;
    int cc = oc >> 2, i = (oc >> 1) & 1, j = oc & 1;
    g[idx] = gps[(((long)b * 2 * H + 2 * y + i) * (2 * W) + 2 * x + j) * C + cc];
}

// the same permutation, 16 elements per thread (C % 4 == 0): a thread takes 4 channels of the 4 sub-pixels of one output pixel as four
// 16-byte loads, transposes 4x4 in registers and writes 16 consecutive output channels as four 16-byte stores (the one-element form
// spends ~30 integer instructions per 4 bytes: 226 us for 537 MB)
__global__ __launch_bounds__(256) void ps2_inverse4_kernel(const float* __restrict__ gps, float* __restrict__ g, long total, int H, int W, int C) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int C4 = C >> 2;
    const int cq = (int)(idx % C4);
    long r = idx / C4;
    const int x = (int)(r % W);
    r /= W;
    const int y = (int)(r % H);
    const long b = r / H;
    floatx4 v[4];
#pragma unroll
    for (int sub = 0; sub < 4; ++sub)
        v[sub] = *(const floatx4*)(gps + (((b * 2 * H + 2 * y + (sub >> 1)) * (2 * W) + 2 * x + (sub & 1)) * C + 4 * cq));
    float* o = g + (((b * H + y) * W + x) * 4L * C + 16 * cq);
#pragma unroll
    for (int k = 0; k < 4; ++k) *(floatx4*)(o + 4 * k) = floatx4{v[0][k], v[1][k], v[2][k], v[3][k]};
}

int grid_for(long n) {
    long b = (n + 255) / 256;
    return (int)(b < 2048 ? (b > 0 ? b : 1) : 2048);
}

}  // namespace

// workgroup caps of the two persistent gradient walks (srbh_internal.h; srbh_head_wgs_cap reports them)
namespace srbh {
int hwgrad16_wgs_cap() { static const int v = getenv("SRBH_HWGRAD16_WGS") ? atoi(getenv("SRBH_HWGRAD16_WGS")) : 768; return v; }
int hbwd16_wgs_cap() { static const int v = getenv("SRBH_HBWD16_WGS") ? atoi(getenv("SRBH_HBWD16_WGS")) : 512; return v; }
}  // namespace srbh

namespace {
// (tile geometry: head_set_tiles over HT_H x 64 tiles; 4 x 64 for hwgrad16_kernel)  workgroup columns (grid.x) of the 8 x 64 walks: a multiple of 8 (the same number of workgroups per XCD), at most 512
int wg_columns(const WGParams& p) { return p.ntiles < 512 ? (p.ntiles + 7) / 8 * 8 : 512; }
// sources, folded BN and dY of an NHWC call
void wg_set_tensors(WGParams& p, const srbh_hwgrad_args* a) {
    p.src0 = a->src0; p.src1 = a->src1; p.c0 = a->c0; p.c1 = a->c1;
    p.ld0 = a->src0_ld > 0 ? a->src0_ld : a->c0;
    p.ld1 = a->src1_ld > 0 ? a->src1_ld : a->c1;
    p.pre_scale = a->pre_scale; p.pre_shift = a->pre_shift; p.pre_relu = a->pre_relu;
    p.dy = a->dy; p.cout_total = a->cout; p.dw = a->dw; p.ws = a->ws;
    p.io = a->io;
    p.zchunk = 0;
}
// one launch of a weight-gradient kernel with lds_bytes of dynamic LDS (its limit is raised once per device and kernel form)
template <auto Kernel>
int launch_wg(dim3 grid, int lds_bytes, hipStream_t st, const WGParams& p) { return launch<Kernel, true>(grid, lds_bytes, st, p); }

int wgrad_impl(const srbh_hwgrad_args* a, void* stream, bool b16, const char* who) {
    SRBH_REQUIRE(a && a->src0 && a->dy && a->dw, "%s: null pointer", who);
    SRBH_REQUIRE(a->c0 > 0 && a->c1 >= 0 && (a->c1 == 0 || a->src1), "srbh_hconv_wgrad: bad channel split");
    SRBH_REQUIRE(a->ksize == 3 || a->ksize == 1, "srbh_hconv_wgrad: ksize must be 1 or 3");
    SRBH_REQUIRE(a->cout >= 1 && a->cout <= 64 && a->B > 0 && a->H > 0 && a->W > 0, "srbh_hconv_wgrad: bad shape");
    WGParams p = {};
    wg_set_tensors(p, a);
    SRBH_REQUIRE(a->ws, "srbh_hconv_wgrad: workspace missing (srbh_hwgrad_ws_bytes)");
    SRBH_REQUIRE((a->io & ~(SRBH_WG_SRC0_H16 | SRBH_WG_DY_B16)) == 0, "srbh_hconv_wgrad: unknown io bits");
    SRBH_REQUIRE(!a->io || b16, "srbh_hconv_wgrad_f32: 16-bit tensors in memory need the bf16-operand form (srbh_hconv_wgrad_b16)");
    const bool xs16 = (a->io & SRBH_WG_SRC0_H16) != 0, ds16 = (a->io & SRBH_WG_DY_B16) != 0;
    head_set_tiles(p, a->B, a->H, a->W, HT_H);
    hipStream_t st = (hipStream_t)stream;
    const int cin = a->c0 + a->c1;
    const int nob = (a->cout + 15) / 16;
    int gx = wg_columns(p);
    // the bf16 form moves whole 4-channel groups with 16-byte loads and whole 16-channel output blocks; the few layers outside
    // that (the 1- and 7-channel output convs) keep the fp32 kernel
    const bool can16 = (a->c0 & 3) == 0 && (a->c1 & 3) == 0 && (p.ld0 & 3) == 0 && (a->c1 == 0 || (p.ld1 & 3) == 0) && (a->cout & 15) == 0 &&
                       ((uintptr_t)a->src0 & 15) == 0 && ((uintptr_t)a->src1 & 15) == 0 && ((uintptr_t)a->dy & (ds16 ? 7 : 15)) == 0;
    // the dominant layer shape has its own double-buffered kernel (srbh_hwgrad16_kernel.h)
    const int k16_wgs = hwgrad16_wgs_cap();   // below 8 (0): not taken
    const bool narrow = a->cout < 16 && !ds16;          // conv_last (1 / 7 output channels): zero-padded to one 16-channel block while staged
    const bool k16 = b16 && k16_wgs >= 8 && k16_wgs <= WS_SLOTS && a->ksize == 3 && a->c0 == 16 && a->c1 == 0 && (a->cout == 16 || narrow) &&
                     (a->W & 63) == 0 && (a->H & 3) == 0 && (p.ld0 & 3) == 0 && ((uintptr_t)a->src0 & (xs16 ? 7 : 15)) == 0 &&
                     ((uintptr_t)a->dy & (narrow ? 3 : ds16 ? 7 : 15)) == 0;
    SRBH_REQUIRE(!xs16 || k16 || (b16 && can16 && ((uintptr_t)a->src0 & 7) == 0),
                 "srbh_hconv_wgrad_b16: an fp16 source tensor needs the bf16-operand forms (4-aligned channels, 16-channel output blocks)");
    SRBH_REQUIRE(!ds16 || k16 || can16, "srbh_hconv_wgrad_b16: a bf16 dY needs 4-aligned channels / 16-channel output blocks");
    count_path(k16 ? PATH_WGRAD16 : (b16 && can16) ? PATH_WGRAD_B16_GENERIC : PATH_WGRAD_F32);
    static const int ob_inner = getenv("SRBH_WGRAD_OB_INNER") ? atoi(getenv("SRBH_WGRAD_OB_INNER")) : 1;      // 0: grid.y = output blocks (A/B aid)
    int rc;
    if (k16) {
        head_set_tiles(p, a->B, a->H, a->W, 4);
        gx = head_walk_grid(p, k16_wgs);
        const dim3 grid(gx);
        constexpr int LDS_B = WG16T::LDS_B;
        if (narrow && xs16) rc = launch_wg<hwgrad16_kernel<1, 2>>(grid, LDS_B, st, p);
        else if (narrow) rc = launch_wg<hwgrad16_kernel<0, 2>>(grid, LDS_B, st, p);
        else if (xs16 && ds16) rc = launch_wg<hwgrad16_kernel<1, 1>>(grid, LDS_B, st, p);
        else if (xs16) rc = launch_wg<hwgrad16_kernel<1, 0>>(grid, LDS_B, st, p);
        else if (ds16) rc = launch_wg<hwgrad16_kernel<0, 1>>(grid, LDS_B, st, p);
        else rc = launch_wg<hwgrad16_kernel<0, 0>>(grid, LDS_B, st, p);
    } else if (b16 && can16 && a->ksize == 3 && a->c1 == 0 && cin <= 16 && nob == 4 && ob_inner) {
        // one input chunk, four output blocks (the Upsampler's 16 -> 64 convs): X staged once per tile, the dY blocks inside the walk
        if (ds16) rc = launch_wg<hwgrad_ob_b16_kernel<1, 4>>(dim3(gx), WG16<3>::LDS_B, st, p);
        else rc = launch_wg<hwgrad_ob_b16_kernel<0, 4>>(dim3(gx), WG16<3>::LDS_B, st, p);
    } else if (b16 && can16) {
        const dim3 grid(gx, nob);
        if (a->ksize == 3 && ds16) rc = launch_wg<hwgrad_b16_kernel<3, 1>>(grid, WG16<3>::LDS_B, st, p);
        else if (a->ksize == 3) rc = launch_wg<hwgrad_b16_kernel<3, 0>>(grid, WG16<3>::LDS_B, st, p);
        else if (ds16) rc = launch_wg<hwgrad_b16_kernel<1, 1>>(grid, WG16<1>::LDS_B, st, p);
        else rc = launch_wg<hwgrad_b16_kernel<1, 0>>(grid, WG16<1>::LDS_B, st, p);
    } else if (a->ksize == 3) {
        rc = launch_wg<hwgrad_f32_kernel<3>>(dim3(gx, nob), (10 * 66 * 16 + 4 * 9 * 256) * 4, st, p);   // X tile + max(dY tile, flush buffer)
    } else {
        rc = launch_wg<hwgrad_f32_kernel<1>>(dim3(gx, nob), (8 * 64 * 16 + 8 * 64 * 16) * 4, st, p);
    }
    if (rc) return rc;
    const int taps = a->ksize * a->ksize, nchunk = (cin + 15) / 16;
    const long U = (long)nob * nchunk * taps * 256;
    return reduce_partials(a->ws, a->dw, U, gx, nchunk, taps, a->cout, cin, st);
}
}  // namespace

/* Weight gradients of a BasicBlock ENTRY (SR/HRfuse.py:142-159: conv1 = 3x3 and downsample[0] = 1x1 over the same input) in one pass
 * over that input: a3 = the 3x3 call's arguments, a1 = the 1x1 call's (same sources, shape, cout, element types; its own dy / dw / ws).
 * bf16 operands.  Shapes the fused kernel does not take run as the two separate calls -- same results either way. */
extern "C" int srbh_hconv_wgrad_entry_b16(const srbh_hwgrad_args* a3, const srbh_hwgrad_args* a1, void* stream) {
    SRBH_REQUIRE(a3 && a1, "srbh_hconv_wgrad_entry_b16: null arguments");
    static const int fuse = getenv("SRBH_WGRAD_ENTRY_FUSE") ? atoi(getenv("SRBH_WGRAD_ENTRY_FUSE")) : 1;
    const int ld0 = a3->src0_ld > 0 ? a3->src0_ld : a3->c0, ld1 = a3->src1_ld > 0 ? a3->src1_ld : a3->c1;
    const int dld0 = a1->src0_ld > 0 ? a1->src0_ld : a1->c0, dld1 = a1->src1_ld > 0 ? a1->src1_ld : a1->c1;
    const bool ds16 = (a3->io & SRBH_WG_DY_B16) != 0;
    const bool same = a3->src0 == a1->src0 && a3->src1 == a1->src1 && a3->c0 == a1->c0 && a3->c1 == a1->c1 && ld0 == dld0 && ld1 == dld1 &&
                      a3->B == a1->B && a3->H == a1->H && a3->W == a1->W && a3->cout == a1->cout && a3->io == a1->io &&
                      a3->pre_scale == a1->pre_scale && a3->pre_shift == a1->pre_shift && a3->pre_relu == a1->pre_relu;
    const bool shape = a3->ksize == 3 && a1->ksize == 1 && a3->src0 && a3->dy && a1->dy && a3->dw && a1->dw && a3->ws && a1->ws &&
                       a3->c0 > 0 && (a3->c0 & 3) == 0 && (a3->c1 & 3) == 0 && (a3->c1 == 0 || a3->src1) && (ld0 & 3) == 0 && (a3->c1 == 0 || (ld1 & 3) == 0) &&
                       a3->cout > 0 && a3->cout <= 64 && (a3->cout & 15) == 0 && a3->B > 0 && a3->H > 0 && a3->W > 0 &&
                       !(a3->c0 == 16 && a3->c1 == 0) &&                /* (the 16 -> 16 layer has its own kernel) */
                       (a3->io & ~(SRBH_WG_SRC0_H16 | SRBH_WG_DY_B16)) == 0 &&
                       ((uintptr_t)a3->src0 & ((a3->io & SRBH_WG_SRC0_H16) ? 7 : 15)) == 0 && ((uintptr_t)a3->src1 & 15) == 0 &&
                       (((uintptr_t)a3->dy | (uintptr_t)a1->dy) & (ds16 ? 7 : 15)) == 0;
    if (!(fuse && same && shape)) {
        count_path(PATH_WGRAD_ENTRY_SPLIT);
        if (int rc = wgrad_impl(a3, stream, true, "srbh_hconv_wgrad_b16")) return rc;
        return wgrad_impl(a1, stream, true, "srbh_hconv_wgrad_b16");
    }
    count_path(PATH_WGRAD_ENTRY_FUSED);
    WGParams p = {};
    wg_set_tensors(p, a3);
    p.dy2 = a1->dy; p.ws2 = a1->ws;
    head_set_tiles(p, a3->B, a3->H, a3->W, HT_H);
    hipStream_t st = (hipStream_t)stream;
    const int cin = a3->c0 + a3->c1, nob = a3->cout / 16, nchunk = (cin + 15) / 16;
    const int gx = wg_columns(p);
    const dim3 grid(gx, nob);
    int rc;
    // (fuse == 2: the chunk-outer kernel also where the chunk-inner one applies; fuse == 3: without the whole-row 64-channel kernel -- same-box A/B aids)
    if ((fuse == 1) && a3->c0 == 64 && a3->c1 == 0 && ld0 == 64 && (a3->io & SRBH_WG_SRC0_H16) && !a3->pre_scale && !a3->pre_relu &&
        ((uintptr_t)a3->src0 & 15) == 0) {
        if (ds16) rc = launch_wg<hwgrad_entry64_b16_kernel<1>>(grid, WG64::LDS_B, st, p);
        else rc = launch_wg<hwgrad_entry64_b16_kernel<0>>(grid, WG64::LDS_B, st, p);
    } else if ((fuse == 1 || fuse == 3) && (nchunk == 2 || nchunk == 4)) {
        if (ds16 && nchunk == 4) rc = launch_wg<hwgrad_entry_b16_kernel<1, 4>>(grid, WG16<3>::LDS_B2, st, p);
        else if (ds16) rc = launch_wg<hwgrad_entry_b16_kernel<1, 2>>(grid, WG16<3>::LDS_B2, st, p);
        else if (nchunk == 4) rc = launch_wg<hwgrad_entry_b16_kernel<0, 4>>(grid, WG16<3>::LDS_B2, st, p);
        else rc = launch_wg<hwgrad_entry_b16_kernel<0, 2>>(grid, WG16<3>::LDS_B2, st, p);
    } else if (ds16) {
        rc = launch_wg<hwgrad_b16_kernel<3, 1, 0, 1>>(grid, WG16<3>::LDS_B2, st, p);
    } else {
        rc = launch_wg<hwgrad_b16_kernel<3, 0, 0, 1>>(grid, WG16<3>::LDS_B2, st, p);
    }
    if (rc) return rc;
    for (int k = 0; k < 2; ++k) {           // the two ordered reduces (3x3, then 1x1): as behind the separate calls
        const int taps = k == 0 ? 9 : 1;
        const srbh_hwgrad_args* a = k == 0 ? a3 : a1;
        const long U = (long)nob * nchunk * taps * 256;
        if (int rc = reduce_partials(a->ws, a->dw, U, gx, nchunk, taps, a->cout, cin, st)) return rc;
    }
    return SRBH_OK;
}

extern "C" int srbh_hconv_wgrad_f32(const srbh_hwgrad_args* a, void* stream) { return wgrad_impl(a, stream, false, "srbh_hconv_wgrad_f32"); }

extern "C" int srbh_hconv_wgrad_b16(const srbh_hwgrad_args* a, void* stream) { return wgrad_impl(a, stream, true, "srbh_hconv_wgrad_b16"); }

/* Weight gradient of a 3x3 conv of the RRDBNet training path on ACT16 tensors: x = fp16 chunk planes (the saved dense buffer: channels
 * 0 .. cin-1, cin % 16 == 0), dy = bf16 chunk planes (channels dy_ch0 .. dy_ch0 + cout - 1 of a dy_chunks_total-plane buffer, cout % 16 == 0);
 * dw OIHW fp32 [cout][cin][3][3]; ws as srbh_hwgrad_ws_bytes(cout, cin, 3).  bf16 operands (x rounded while staged), fp32 accumulate,
 * fixed summation order. */
extern "C" int srbh_act16_wgrad_b16(const void* x, int x_chunks_total, int cin, const void* dy, int dy_chunks_total, int dy_ch0, int cout,
                                    int B, int H, int W, float* dw, float* ws, void* stream) {
    SRBH_REQUIRE(x && dy && dw && ws && B > 0 && H > 0 && W > 0, "srbh_act16_wgrad_b16: bad arguments");
    SRBH_REQUIRE(cin > 0 && (cin & 15) == 0 && cin <= x_chunks_total * 32 && cout > 0 && (cout & 15) == 0 && cout <= 64 && (dy_ch0 & 15) == 0 &&
                 dy_ch0 + cout <= dy_chunks_total * 32, "srbh_act16_wgrad_b16: channel ranges (multiples of 16, inside the buffers)");
    WGParams p = {};
    p.src0 = (const float*)x; p.c0 = cin;
    p.dy = (const float*)dy; p.cout_total = cout; p.dw = dw; p.ws = ws;
    const Act16Geo gx_ = act16_geo(B, x_chunks_total, H, W), gd = act16_geo(B, dy_chunks_total, H, W);
    p.x_img_b = gx_.img_b; p.x_plane_b = gx_.plane_b; p.x_row_b = gx_.row_b;
    p.dy_img_b = gd.img_b; p.dy_plane_b = gd.plane_b; p.dy_row_b = gd.row_b; p.dy_ch0 = dy_ch0;
    head_set_tiles(p, B, H, W, HT_H);
    hipStream_t st = (hipStream_t)stream;
    const int nob = cout / 16;
    int gx = wg_columns(p);
    static const int zchunk_max = getenv("SRBH_WG_ZCHUNK_MAX") ? atoi(getenv("SRBH_WG_ZCHUNK_MAX")) : 256;
    p.zchunk = p.ntiles <= zchunk_max ? 1 : 0;
    if (p.zchunk) {
        // Every workgroup column (blockIdx.x) owns a full set of partial sums: with one column per tile the reduce reads gx * |dW| floats
        // -- 56 MB for the 192 -> 64 conv at batch 8, 13 us per call on the stream that bounds the backward.  The grid already has
        // nob * cin/16 workgroups per column, so columns walk several tiles each as long as ~768 workgroups remain (swept at batch 8: 22.5 ms per generator step with one column per tile, 22.1 / 20.7 / 21.1 / 22.2 at 1 536 / 768 / 512 / 256).
        static const int want_wgs = getenv("SRBH_WG_COLUMNS_WGS") ? atoi(getenv("SRBH_WG_COLUMNS_WGS")) : 768;
        const int per_col = nob * (cin / 16);
        int cols = ((want_wgs + per_col - 1) / per_col + 7) / 8 * 8;
        cols = cols < 8 ? 8 : cols;
        if (cols < gx) gx = cols;
    }
    if (int rc = launch_wg<hwgrad_b16_kernel<3, 1, 1>>(dim3(gx, nob, p.zchunk ? cin / 16 : 1), WG16<3>::LDS_B, st, p)) return rc;
    const int taps = 9, nchunk = cin / 16;
    const long U = (long)nob * nchunk * taps * 256;
    // few partial slots: the one-stage reduce; otherwise (and always under srbh_hwgrad_defer -- srbh_rrdbnet_trunk_train_backward batches a
    // dense block's five) the two-stage ordered reduce
    if (g_red_defer || gx > 128) return reduce_partials(ws, dw, U, gx, nchunk, taps, cout, cin, st);
    const int total = cout * cin * taps;
    hipLaunchKernelGGL(hwgrad_reduce_direct_kernel, dim3((total + 255) / 256), dim3(256), 0, st, ws, dw, U, gx, nchunk, taps, cout, cin);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_hbwd16_supported(int H, int W) { return H > 0 && W > 0 && (W & 63) == 0 && (H & 3) == 0; }

/* One pass for the backward of a 3x3, 16 -> 16 conv behind its BatchNorm (srbh_hbwd16_kernel.h): dc never reaches memory. */
extern "C" int srbh_hbwd16(const srbh_hbwd16_args* a, void* stream) {
    SRBH_REQUIRE(a && a->g && a->c && a->mean && a->invstd && a->coef && a->k1 && a->k2 && a->x && a->w && a->dx && a->dw && a->ws,
                 "srbh_hbwd16: null pointer");
    SRBH_REQUIRE(a->B > 0 && srbh_hbwd16_supported(a->H, a->W), "srbh_hbwd16: W %% 64 == 0 and H %% 4 == 0 (srbh_hbwd16_supported)");
    SRBH_REQUIRE((a->mask_scale == nullptr) == (a->mask_shift == nullptr) && (a->pre_scale == nullptr) == (a->pre_shift == nullptr),
                 "srbh_hbwd16: scale / shift come in pairs");
    SRBH_REQUIRE(!a->stats || (a->bstat_c && a->bstat_mean && a->bstat_invstd && (a->relu_bits || !a->res) && (a->bstat_ms == nullptr) == (a->bstat_mh == nullptr)),
                 "srbh_hbwd16: the statistics epilogue needs bstat_c / mean / invstd and takes no skip gradient (unless relu_bits)");
    SRBH_REQUIRE(!a->relu_bits || (a->stats && a->dx_b16 && !a->bstat_ms && ((uintptr_t)a->relu_bits & 7) == 0),
                 "srbh_hbwd16: relu_bits needs stats + bstat_c / mean / invstd of the previous block's bn2, a bf16 dx and no bstat mask");
    SRBH_REQUIRE((((uintptr_t)a->g | (uintptr_t)a->res) & 7) == 0 && (((uintptr_t)a->c | (uintptr_t)a->x | (uintptr_t)a->bstat_c | (uintptr_t)a->w) & 15) == 0 &&
                 ((uintptr_t)a->dx & (a->dx_b16 ? 7 : 15)) == 0, "srbh_hbwd16: misaligned tensor");
    hipStream_t st = (hipStream_t)stream;
    HBParams p;
    p.g = a->g; p.c = a->c; p.mean = a->mean; p.invstd = a->invstd; p.coef = a->coef; p.k1 = a->k1; p.k2 = a->k2;
    p.ms = a->mask_scale; p.mh = a->mask_shift;
    p.x = a->x; p.pre_scale = a->pre_scale; p.pre_shift = a->pre_shift; p.pre_relu = a->pre_relu;
    p.w = a->w; p.dx = a->dx; p.dx_b16 = a->dx_b16; p.res = a->res;
    p.bstat_c = a->bstat_c; p.bstat_mean = a->bstat_mean; p.bstat_invstd = a->bstat_invstd; p.bstat_ms = a->bstat_ms; p.bstat_mh = a->bstat_mh;
    p.stats = a->stats; p.ws = a->ws; p.relu_bits = (const unsigned long long*)a->relu_bits;
    head_set_tiles(p, a->B, a->H, a->W, 4);
    const int wgs = hbwd16_wgs_cap();
    SRBH_REQUIRE(wgs >= 8 && wgs <= WS_SLOTS, "SRBH_HBWD16_WGS must be 8 .. %d", WS_SLOTS);      // a cap below 8: an argument error
    const int gx = head_walk_grid(p, wgs);
    if (a->stats && !a->stats_clean) { if (int rc = zero_async(a->stats, (size_t)NSLOT * 2 * 16 * sizeof(double), st)) return rc; }
    // hbwd16_kernel<BS, MASK>: BS = 2 relu_bits form, 1 statistics epilogue, 0 none; MASK = the ReLU mask behind the BatchNorm
    const int rc = with_const<3>(a->relu_bits ? 2 : a->stats ? 1 : 0, [&](auto b) {
        return with_const<2>(a->mask_scale != nullptr, [&](auto m) {
            return launch<hbwd16_kernel<decltype(b)::value, decltype(m)::value>, true>(dim3(gx), HB16::LDS_B, st, p);
        });
    });
    if (rc) return rc;
    count_path(PATH_HBWD16);
    // the workgroups' weight-gradient partials -> dW (the ordered two-stage reduce of srbh_hconv_wgrad_b16; queued under srbh_hwgrad_defer)
    return reduce_partials(a->ws, a->dw, 9 * 256, gx, 1, 9, 16, 16, st);
}

/* Between srbh_hwgrad_defer(1) and srbh_hwgrad_flush the weight-gradient entry points above (srbh_hconv_wgrad_f32 / _b16 / _entry_b16,
 * srbh_hbwd16) run their kernels but QUEUE the ordered reduce of their partial sums; srbh_hwgrad_flush does every queued reduce in one pair
 * of launches and ends the deferral.  The caller keeps every `ws` (and `dw`) alive until the flush.  Per host thread. */
extern "C" int srbh_hwgrad_defer(int on) {
    SRBH_REQUIRE(on || g_red_queue.empty(), "srbh_hwgrad_defer(0) with queued reduce jobs: call srbh_hwgrad_flush");
    g_red_defer = on != 0;
    return SRBH_OK;
}
extern "C" int srbh_hwgrad_flush(void* stream) {
    g_red_defer = false;
    return reduce_flush((hipStream_t)stream);
}

extern "C" size_t srbh_hwgrad_ws_bytes(int cout, int cin, int ksize) {
    if (cout <= 0 || cin <= 0 || (ksize != 1 && ksize != 3)) return 0;
    return (size_t)(WS_SLOTS + 16) * ((cout + 15) / 16) * ((cin + 15) / 16) * ksize * ksize * 256 * sizeof(float);
}

extern "C" int srbh_relu_mask_mul(const float* g, const float* ref, float* out, long n, void* stream) {
    SRBH_REQUIRE(g && ref && out && n > 0 && n % 4 == 0, "srbh_relu_mask_mul: bad arguments");
    hipLaunchKernelGGL(relu_mask_mul_kernel, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, (const floatx4*)g,
                       (const floatx4*)ref, (floatx4*)out, n / 4);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_add_inplace(float* a, const float* b, long n, void* stream) {
    SRBH_REQUIRE(a && b && n > 0 && n % 4 == 0, "srbh_add_inplace: bad arguments");
    hipLaunchKernelGGL(add_inplace_kernel, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, (floatx4*)a,
                       (const floatx4*)b, n / 4);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

static int bn_bwd_reduce_impl(const void* g, const float* relu_ref, void* dz_out, const void* c, const float* mean, const float* invstd,
                              const float* mask_scale, const float* mask_shift, long npix, int C, double* stats, void* stream, int io = 0) {
    hipStream_t st = (hipStream_t)stream;
    const bool clean = (io & SRBH_BN_STATS_CLEAN) != 0;
    io &= ~SRBH_BN_STATS_CLEAN;
    const bool gb = (io & SRBH_BN_G_B16) != 0, ch = (io & SRBH_BN_C_H16) != 0, ob = (io & SRBH_BN_OUT_B16) != 0, rb = (io & SRBH_BN_REF_BITS) != 0;
    const bool v4 = (C & 3) == 0 && (256 % (C >> 2)) == 0 && ((uintptr_t)g & (gb ? 7 : 15)) == 0 && ((uintptr_t)c & (ch ? 7 : 15)) == 0 &&
                    ((uintptr_t)dz_out & (ob ? 7 : 15)) == 0 && ((uintptr_t)relu_ref & (rb ? 7 : 15)) == 0 && (((uintptr_t)mean | (uintptr_t)invstd |
                     (uintptr_t)mask_scale | (uintptr_t)mask_shift) & 15) == 0;
    SRBH_REQUIRE(!rb || (relu_ref && v4), "srbh_bn_bwd_reduce_io: SRBH_BN_REF_BITS needs relu_ref (the bit buffer) and the vector form");
    SRBH_REQUIRE(!io || v4, "srbh_bn_bwd_reduce: 16-bit tensors need the vector form (C %% 4 == 0, 256 %% (C/4) == 0, aligned)");
    SRBH_REQUIRE(!relu_ref || v4, "srbh_bn_bwd_reduce_relu: needs the 16-byte form (C %% 4 == 0, 256 %% (C/4) == 0, aligned)");
    // (the zero fill comes behind every refusal: a refused call writes nothing)
    if (!clean) { if (int rc = zero_async(stats, (size_t)NSLOT * 2 * C * sizeof(double), st)) return rc; }
    if (v4) {
        const long n4 = npix * (C >> 2);
#define SRBH_BNR(G_, C_, O_) hipLaunchKernelGGL((bn_bwd_reduce4_kernel<G_, C_, O_>), dim3(grid4_for(n4)), dim3(256), 2 * C * sizeof(float), st, \
                                                g, c, mean, invstd, mask_scale, mask_shift, (const floatx4*)relu_ref, dz_out, n4, C, stats)
        if (rb) {
#define SRBH_BNRB(G_, C_, O_) hipLaunchKernelGGL((bn_bwd_reduce4_kernel<G_, C_, O_, 1>), dim3(grid4_for(n4)), dim3(256), 2 * C * sizeof(float), st, \
                                                 g, c, mean, invstd, mask_scale, mask_shift, (const floatx4*)relu_ref, dz_out, n4, C, stats)
            switch ((gb ? 4 : 0) | (ch ? 2 : 0) | (ob ? 1 : 0)) {
                case 0: SRBH_BNRB(0, 0, 0); break; case 1: SRBH_BNRB(0, 0, 1); break; case 2: SRBH_BNRB(0, 1, 0); break; case 3: SRBH_BNRB(0, 1, 1); break;
                case 4: SRBH_BNRB(1, 0, 0); break; case 5: SRBH_BNRB(1, 0, 1); break; case 6: SRBH_BNRB(1, 1, 0); break; default: SRBH_BNRB(1, 1, 1); break;
            }
#undef SRBH_BNRB
        } else
        switch ((gb ? 4 : 0) | (ch ? 2 : 0) | (ob ? 1 : 0)) {
            case 0: SRBH_BNR(0, 0, 0); break; case 1: SRBH_BNR(0, 0, 1); break; case 2: SRBH_BNR(0, 1, 0); break; case 3: SRBH_BNR(0, 1, 1); break;
            case 4: SRBH_BNR(1, 0, 0); break; case 5: SRBH_BNR(1, 0, 1); break; case 6: SRBH_BNR(1, 1, 0); break; default: SRBH_BNR(1, 1, 1); break;
        }
#undef SRBH_BNR
    } else {
        // a block size that is a multiple of C keeps every thread on ONE channel (register partial sums); with 256 threads and e.g.
        // C = 7 (the bias gradient of the 7-class output conv) every element went through an LDS atomic: 295 us for 117 MB
        const int bd = (256 % C == 0) ? 256 : (256 / C) * C;
        hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(grid_for(npix * C)), dim3(bd), 2 * C * sizeof(float), st, (const float*)g, (const float*)c, mean,
                           invstd, mask_scale, mask_shift, npix, C, stats);
    }
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_bn_bwd_reduce(const float* g, const float* c, const float* mean, const float* invstd,
                                  const float* mask_scale, const float* mask_shift, long npix, int C, double* stats,
                                  void* stream) {
    SRBH_REQUIRE(g && stats && npix > 0 && C > 0 && C <= 64, "srbh_bn_bwd_reduce: bad arguments");
    SRBH_REQUIRE(!c || (mean && invstd), "srbh_bn_bwd_reduce: c needs mean/invstd");
    SRBH_REQUIRE(!mask_scale || (c && mask_shift), "srbh_bn_bwd_reduce: mask needs c and mask_shift");
    return bn_bwd_reduce_impl(g, nullptr, nullptr, c, mean, invstd, mask_scale, mask_shift, npix, C, stats, stream);
}

extern "C" int srbh_bn_bwd_reduce_relu(const float* g, const float* relu_ref, float* dz_out, const float* c, const float* mean,
                                       const float* invstd, long npix, int C, double* stats, void* stream) {
    SRBH_REQUIRE(g && relu_ref && stats && npix > 0 && C > 0 && C <= 64 && (C & 3) == 0, "srbh_bn_bwd_reduce_relu: bad arguments (C % 4 == 0)");
    SRBH_REQUIRE(!c || (mean && invstd), "srbh_bn_bwd_reduce_relu: c needs mean/invstd");
    SRBH_REQUIRE((((uintptr_t)g | (uintptr_t)relu_ref | (uintptr_t)dz_out | (uintptr_t)c) & 15) == 0, "srbh_bn_bwd_reduce_relu: 16-byte aligned tensors");
    return bn_bwd_reduce_impl(g, relu_ref, dz_out, c, mean, invstd, nullptr, nullptr, npix, C, stats, stream);
}

/* the same two reductions with 16-bit tensors in memory (io: SRBH_BN_G_B16 | SRBH_BN_C_H16 | SRBH_BN_OUT_B16); relu_ref / dz_out optional */
extern "C" int srbh_bn_bwd_reduce_io(const void* g, const float* relu_ref, void* dz_out, const void* c, const float* mean, const float* invstd,
                                     const float* mask_scale, const float* mask_shift, long npix, int C, double* stats, int io, void* stream) {
    SRBH_REQUIRE(g && stats && npix > 0 && C > 0 && C <= 64, "srbh_bn_bwd_reduce_io: bad arguments");
    SRBH_REQUIRE(!c || (mean && invstd), "srbh_bn_bwd_reduce_io: c needs mean/invstd");
    SRBH_REQUIRE(!mask_scale || (c && mask_shift), "srbh_bn_bwd_reduce_io: mask needs c and mask_shift");
    SRBH_REQUIRE(!(relu_ref && mask_scale), "srbh_bn_bwd_reduce_io: either the block-closing ReLU (relu_ref) or the bn1 mask");
    SRBH_REQUIRE((io & ~31) == 0, "srbh_bn_bwd_reduce_io: unknown io bits");
    return bn_bwd_reduce_impl(g, relu_ref, dz_out, c, mean, invstd, mask_scale, mask_shift, npix, C, stats, stream, io);
}

extern "C" int srbh_bn_bwd_apply_io(const void* g, const void* c, const float* mean, const float* invstd, const float* mask_scale,
                                    const float* mask_shift, const float* coef, const float* k1, const float* k2, void* out, long npix, int C,
                                    int io, void* stream) {
    SRBH_REQUIRE(g && c && mean && invstd && coef && k1 && k2 && out && npix > 0 && C > 0, "srbh_bn_bwd_apply_io: bad arguments");
    const bool gb = (io & SRBH_BN_G_B16) != 0, ch = (io & SRBH_BN_C_H16) != 0, ob = (io & SRBH_BN_OUT_B16) != 0;
    SRBH_REQUIRE((io & ~7) == 0 && (C & 3) == 0 && (256 % (C >> 2)) == 0 && ((uintptr_t)g & (gb ? 7 : 15)) == 0 && ((uintptr_t)c & (ch ? 7 : 15)) == 0 &&
                 ((uintptr_t)out & (ob ? 7 : 15)) == 0, "srbh_bn_bwd_apply_io: needs the vector form (C %% 4 == 0, 256 %% (C/4) == 0, aligned)");
    SRBH_REQUIRE(!mask_scale || mask_shift, "srbh_bn_bwd_apply_io: mask_scale needs mask_shift");
    SRBH_REQUIRE((((uintptr_t)mean | (uintptr_t)invstd | (uintptr_t)coef | (uintptr_t)k1 | (uintptr_t)k2 | (uintptr_t)mask_scale | (uintptr_t)mask_shift) & 15) == 0,
                 "srbh_bn_bwd_apply_io: 16-byte aligned per-channel vectors");
    const long n4 = npix * (C >> 2);
#define SRBH_BNA(G_, C_, O_) hipLaunchKernelGGL((bn_bwd_apply4_kernel<G_, C_, O_>), dim3(grid4_for(n4)), dim3(256), 0, (hipStream_t)stream, \
                                                g, c, mean, invstd, mask_scale, mask_shift, coef, k1, k2, out, n4, C)
    switch ((gb ? 4 : 0) | (ch ? 2 : 0) | (ob ? 1 : 0)) {
        case 0: SRBH_BNA(0, 0, 0); break; case 1: SRBH_BNA(0, 0, 1); break; case 2: SRBH_BNA(0, 1, 0); break; case 3: SRBH_BNA(0, 1, 1); break;
        case 4: SRBH_BNA(1, 0, 0); break; case 5: SRBH_BNA(1, 0, 1); break; case 6: SRBH_BNA(1, 1, 0); break; default: SRBH_BNA(1, 1, 1); break;
    }
#undef SRBH_BNA
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_bn_bwd_finalize(const double* stats, int C, double count, const float* gamma, const float* invstd,
                                    float* dgamma, float* dbeta, float* coef, float* k1, float* k2, void* stream) {
    SRBH_REQUIRE(stats && C > 0 && C <= 64 && count > 0, "srbh_bn_bwd_finalize: bad arguments");
    SRBH_REQUIRE(!coef || (invstd && k1 && k2), "srbh_bn_bwd_finalize: coef needs invstd, k1, k2");
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (double*)stats, C, count, gamma, invstd,
                       dgamma, dbeta, coef, k1, k2, 0);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_bn_bwd_finalize_clear(double* stats, int C, double count, const float* gamma, const float* invstd,
                                          float* dgamma, float* dbeta, float* coef, float* k1, float* k2, void* stream) {
    SRBH_REQUIRE(stats && C > 0 && C <= 64 && count > 0, "srbh_bn_bwd_finalize_clear: bad arguments");
    SRBH_REQUIRE(!coef || (invstd && k1 && k2), "srbh_bn_bwd_finalize_clear: coef needs invstd, k1, k2");
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, stats, C, count, gamma, invstd,
                       dgamma, dbeta, coef, k1, k2, 1);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_bn_bwd_apply(const float* g, const float* c, const float* mean, const float* invstd,
                                 const float* mask_scale, const float* mask_shift, const float* coef, const float* k1,
                                 const float* k2, float* out, long npix, int C, void* stream) {
    SRBH_REQUIRE(g && c && mean && invstd && coef && k1 && k2 && out && npix > 0 && C > 0, "srbh_bn_bwd_apply: bad arguments");
    if ((C & 3) == 0 && (256 % (C >> 2)) == 0 && (((uintptr_t)g | (uintptr_t)c | (uintptr_t)out | (uintptr_t)mean | (uintptr_t)invstd | (uintptr_t)coef |
                                                    (uintptr_t)k1 | (uintptr_t)k2 | (uintptr_t)mask_scale | (uintptr_t)mask_shift) & 15) == 0) {
        const long n4 = npix * (C >> 2);
        hipLaunchKernelGGL((bn_bwd_apply4_kernel<0, 0, 0>), dim3(grid4_for(n4)), dim3(256), 0, (hipStream_t)stream, (const void*)g, (const void*)c,
                           mean, invstd, mask_scale, mask_shift, coef, k1, k2, (void*)out, n4, C);
    } else
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_for(npix * C)), dim3(256), 0, (hipStream_t)stream, g, c, mean,
                       invstd, mask_scale, mask_shift, coef, k1, k2, out, npix * C, C);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_ps2_inverse(const float* g_ps, float* g, int B, int H, int W, int C, void* stream) {
    SRBH_REQUIRE(g_ps && g && B > 0 && H > 0 && W > 0 && C > 0, "srbh_ps2_inverse: bad arguments");
    long total = (long)B * H * W * 4 * C;
    if ((C & 3) == 0 && (((uintptr_t)g_ps | (uintptr_t)g) & 15) == 0) {
        const long n16 = total / 16;
        hipLaunchKernelGGL(ps2_inverse4_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g_ps, g, n16, H, W, C);
        SRBH_HIP(hipGetLastError());
        return SRBH_OK;
    }
    hipLaunchKernelGGL(ps2_inverse_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, g_ps, g, B, H, W, C);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
