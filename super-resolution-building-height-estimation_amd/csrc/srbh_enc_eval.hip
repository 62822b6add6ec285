// srbh_enc_eval.hip -- the EfficientNet encoder's element-wise inference kernels, fp32 NCHW: the folded BatchNorm + activation pass (+ skip
// connection, + per-plane mean), the squeeze-and-excitation layers of an MBConv block, and the stem conv.  (The depthwise conv and the fused
// MBConv middle: srbh_dwconv.hip.)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "srbh.h"
#include "srbh_internal.h"

namespace {
using namespace srbh;

#include "srbh_dw_pieces.h"      // floatx4, act_apply, gate_sigmoid, wave_sum, grid_for

// inference BatchNorm (+ activation) on NCHW fp32: y = act(x * scale[c] + shift[c]); act 0 none, 1 SiLU, 2 ReLU.  One pass,
// float4 when the plane size allows (MIOpen's inference-BatchNorm kernel takes ~39 us per call whatever the tensor size,
// 115 calls per batch in the encoder / decoders).
template <int VEC>
__global__ __launch_bounds__(256) void affine_act_nchw_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, const float* __restrict__ res,
                                                             float* __restrict__ y, long planes, int C, int hw, int act) {
    const int per = hw / VEC;
    const long total = planes * per;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long pl = idx / per;
        const int c = (int)(pl % C);
        const float s = scale[c], h = shift[c];
        float v[VEC];
        if (VEC == 4) {
            const floatx4 t = ((const floatx4*)x)[idx];
            v[0] = t[0]; v[1 % VEC] = t[1]; v[2 % VEC] = t[2]; v[3 % VEC] = t[3];
        } else {
            v[0] = x[idx];
        }
#pragma unroll
        for (int q = 0; q < VEC; ++q) v[q] = act_apply(fmaf(v[q], s, h), act);
        if (VEC == 4) {
            floatx4 t = {v[0], v[1 % VEC], v[2 % VEC], v[3 % VEC]};
            if (res) t += ((const floatx4*)res)[idx];          // the block's skip connection (MBConv: x = bn2(project(x)) + inputs)
            ((floatx4*)y)[idx] = t;
        } else {
            y[idx] = res ? v[0] + res[idx] : v[0];
        }
    }
}

// ---- the encoder's STEM at inference (round 6): conv3x3 stride 2 (static "same" padding) Cin <= 16 -> Cout <= 64 + the folded BatchNorm + SiLU in
// one pass on NCHW fp32 (smp EfficientNetEncoder.forward through mymodels.py:276: `_swish(_bn0(_conv_stem(x)))`).  MIOpen's solver search
// (benchmark mode of the tiled-inference path) settles on an asm kernel that takes ~0.6 ms per 128-tile batch for this 0.9-GFLOP layer
// (profiles/r05cd_predict_steady_kernel_stats.txt), followed by the affine pass.  Here: one thread per output pixel, all Cout accumulators
// in registers, the weights transposed into LDS as [ci][tap][co] and read as wave-uniform ds_read_b128 broadcasts, input taps straight from
// L1 (a 64 x 64 plane is 16 KB), outputs written plane by plane (coalesced along x).
template <int CO4>
__global__ __launch_bounds__(256) void stem_conv_eval_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, float* __restrict__ y, int B, int Cin, int H, int W,
                                                            int stride, int pt, int pl, int OH, int OW, int act) {
    constexpr int CO = CO4 * 4;
    extern __shared__ __attribute__((aligned(16))) float wl[];          // [Cin][9][CO]
    const int Cout = CO;
    for (int i = threadIdx.x; i < Cout * Cin * 9; i += 256) {
        const int co = i / (Cin * 9), r = i - co * Cin * 9;             // OIHW: r = ci * 9 + tap
        wl[r * CO + co] = w[i];
    }
    __syncthreads();
    const long total = (long)B * OH * OW;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ox = (int)(idx % OW);
    const long t = idx / OW;
    const int oy = (int)(t % OH), b = (int)(t / OH);
    floatx4 acc[CO4];
#pragma unroll
    for (int q = 0; q < CO4; ++q) acc[q] = floatx4{0.f, 0.f, 0.f, 0.f};
    const int iy0 = oy * stride - pt, ix0 = ox * stride - pl;
    const float* xb = x + (long)b * Cin * H * W;
    for (int ci = 0; ci < Cin; ++ci) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int iy = iy0 + tap / 3, ix = ix0 + tap % 3;
            float v = 0.f;
            if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) v = xb[((long)ci * H + iy) * W + ix];
            const floatx4* wq = (const floatx4*)(wl + (ci * 9 + tap) * CO);
#pragma unroll
            for (int q = 0; q < CO4; ++q) acc[q] += wq[q] * v;
        }
    }
    float* yb = y + ((long)b * Cout * OH + oy) * OW + ox;
#pragma unroll
    for (int q = 0; q < CO4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = q * 4 + j;
            yb[(long)co * OH * OW] = act_apply(fmaf(acc[q][j], scale[co], shift[co]), act);
        }
}

// ---- squeeze-and-excitation of an MBConv block at inference (efficientnet_pytorch MBConvBlock.forward: avg-pool -> 1x1
// reduce -> swish -> 1x1 expand -> sigmoid -> scale), three launches instead of ~11 stock-op ones per block:
//  (1) inference BatchNorm + SiLU of the depthwise output WITH the per-plane mean (one wave per (b, c) plane, <= 1024 px)
__global__ __launch_bounds__(256) void affine_act_pool_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, float* __restrict__ y,
                                                             float* __restrict__ pooled, long planes, int C, int hw, int act) {
    const int lane = threadIdx.x & 63;
    const long pl = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pl >= planes) return;
    const int c = (int)(pl % C);
    const float s = scale[c], h = shift[c];
    const float* xp = x + pl * hw;
    float* yp = y + pl * hw;
    float sum = 0.f;
    for (int i = lane; i < hw; i += 64) {
        const float u = act_apply(fmaf(xp[i], s, h), act);
        yp[i] = u;
        sum += u;
    }
    sum = wave_sum(sum);
    if (lane == 0) pooled[pl] = sum / (float)hw;
}

// small planes (hw = 1 .. 32, a power of two): a wave per plane would be mostly empty lanes (4 of 64 at 2x2, 172 k waves per call);
// planes are contiguous, so a wave takes 64 consecutive elements = 64 / hw whole planes and reduces inside hw-lane segments
__global__ __launch_bounds__(256) void affine_act_pool_small_kernel(const float* __restrict__ x, const float* __restrict__ scale,
                                                                   const float* __restrict__ shift, float* __restrict__ y,
                                                                   float* __restrict__ pooled, long planes, int C, int hw, int act) {
    const int lane = threadIdx.x & 63;
    const long idx = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64 + lane;
    const long pl = idx / hw;
    float u = 0.f;
    if (pl < planes) {
        const int c = (int)(pl % C);
        u = act_apply(fmaf(x[idx], scale[c], shift[c]), act);
        y[idx] = u;
    }
    for (int o = 1; o < hw; o <<= 1) u += __shfl_xor(u, o, 64);
    if (pl < planes && (lane & (hw - 1)) == 0) pooled[pl] = u / (float)hw;
}

//  (2) hidden[b][j] = swish(b1[j] + sum_c w1[j][c] * pooled[b][c]): one WAVE per (b, j) dot product (grid = B x SQ/4
//      workgroups: a per-b workgroup looping over j ran 63 us -- a serial chain of dependent global loads)
__global__ __launch_bounds__(256) void se_hidden_kernel(const float* __restrict__ pooled, const float* __restrict__ w1,
                                                       const float* __restrict__ b1, float* __restrict__ hidden, int C, int SQ) {
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (j >= SQ) return;
    const float* wr = w1 + (long)j * C;
    const float* pr = pooled + (long)b * C;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int c = lane;
    for (; c + 192 < C; c += 256) {
        a0 = fmaf(wr[c], pr[c], a0);
        a1 = fmaf(wr[c + 64], pr[c + 64], a1);
        a2 = fmaf(wr[c + 128], pr[c + 128], a2);
        a3 = fmaf(wr[c + 192], pr[c + 192], a3);
    }
    for (; c < C; c += 64) a0 = fmaf(wr[c], pr[c], a0);
    const float acc = wave_sum((a0 + a1) + (a2 + a3));
    if (lane == 0) hidden[(long)b * SQ + j] = act_apply(acc + b1[j], 1);
}

//  gate[b][c] = sigmoid(b2[c] + sum_j w2[c][j] * hidden[b][j]) on its own (the fused inference block multiplies it into the project conv's
//  operand instead of rewriting the expanded tensor).  16 lanes share one channel: a wave walks 4 contiguous rows of w2 (coalesced; one
//  thread per (b, c) read 64 different rows per load and ran 15 us), keeps its slice of the row in registers and loops over a chunk of
//  images; fixed butterfly over the 16 lanes.
constexpr int SE_GATE_IB = 8;          // images per workgroup row
__global__ __launch_bounds__(256) void se_gate_kernel(const float* __restrict__ hidden, const float* __restrict__ w2, const float* __restrict__ b2,
                                                     float* __restrict__ gate, int B, int C, int SQ) {
    const int t = threadIdx.x, sub = t & 15;
    const int c = blockIdx.x * 16 + (t >> 4);
    const bool ok = c < C;
    const float* wr = w2 + (long)(ok ? c : 0) * SQ;
    const int b0 = blockIdx.y * SE_GATE_IB, b1 = b0 + SE_GATE_IB < B ? b0 + SE_GATE_IB : B;
    const float bias = ok ? b2[c] : 0.f;
    if (SQ <= 128) {
        float wv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) wv[u] = (ok && sub + 16 * u < SQ) ? wr[sub + 16 * u] : 0.f;
        for (int b = b0; b < b1; ++b) {
            const float* hr = hidden + (long)b * SQ;
            float a0 = 0.f, a1 = 0.f;
#pragma unroll
            for (int u = 0; u < 8; u += 2) {
                a0 = fmaf(wv[u], sub + 16 * u < SQ ? hr[sub + 16 * u] : 0.f, a0);
                a1 = fmaf(wv[u + 1], sub + 16 * (u + 1) < SQ ? hr[sub + 16 * (u + 1)] : 0.f, a1);
            }
            float acc = a0 + a1;
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) acc += __shfl_xor(acc, o, 64);
            if (ok && sub == 0) gate[(long)b * C + c] = gate_sigmoid(acc + bias);
        }
    } else {
        for (int b = b0; b < b1; ++b) {
            const float* hr = hidden + (long)b * SQ;
            float acc = 0.f;
            if (ok)
                for (int j = sub; j < SQ; j += 16) acc = fmaf(wr[j], hr[j], acc);
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) acc += __shfl_xor(acc, o, 64);
            if (ok && sub == 0) gate[(long)b * C + c] = gate_sigmoid(acc + bias);
        }
    }
}

//  (3) y[plane] *= sigmoid(b2[c] + sum_j w2[c][j] * hidden[b][j]): one wave per (b, c) plane computes its own gate (row c of
//      the expand weight is read coalesced by the wave) and scales the plane in place
__global__ __launch_bounds__(256) void se_gate_scale_kernel(float* __restrict__ y, const float* __restrict__ hidden,
                                                           const float* __restrict__ w2, const float* __restrict__ b2, long planes,
                                                           int C, int SQ, int hw) {
    const int lane = threadIdx.x & 63;
    const long pl = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pl >= planes) return;
    const int c = (int)(pl % C);
    const long b = pl / C;
    const float* wr = w2 + (long)c * SQ;
    const float* hr = hidden + b * SQ;
    float acc = 0.f;
    for (int j = lane; j < SQ; j += 64) acc = fmaf(wr[j], hr[j], acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    const float g = gate_sigmoid(acc + b2[c]);
    float* yp = y + pl * hw;
    for (int i = lane; i < hw; i += 64) yp[i] *= g;
}

// gate + scale for planes of 4 / 16 / 64 / 256 elements: a workgroup takes 1024 consecutive elements (a float4 per thread); the hw / 4
// threads that hold one plane compute its gate together (same reason as affine_act_pool_small_kernel)
__global__ __launch_bounds__(256) void se_gate_scale_quad_kernel(float* __restrict__ y, const float* __restrict__ hidden,
                                                                const float* __restrict__ w2, const float* __restrict__ b2, long planes,
                                                                int C, int SQ, int hw) {
    const int t = threadIdx.x, G = hw >> 2, sub = t & (G - 1);
    const long e = (long)blockIdx.x * 1024 + 4 * t;
    const long pl = e / hw;
    const bool ok = pl < planes;
    const int c = ok ? (int)(pl % C) : 0;
    const long b = ok ? pl / C : 0;
    const float* wr = w2 + (long)c * SQ;
    const float* hr = hidden + b * SQ;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    int j = sub;
    for (; j + 3 * G < SQ; j += 4 * G) {
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = fmaf(wr[j + u * G], hr[j + u * G], a[u]);
    }
    for (; j < SQ; j += G) a[0] = fmaf(wr[j], hr[j], a[0]);
    float acc = (a[0] + a[1]) + (a[2] + a[3]);
    for (int o = 1; o < G; o <<= 1) acc += __shfl_xor(acc, o, 64);
    if (!ok) return;
    const float g = gate_sigmoid(acc + b2[c]);
    floatx4 v = *(floatx4*)(y + e);
    v *= g;
    *(floatx4*)(y + e) = v;
}

int affine_act_impl(const float* x, const float* scale, const float* shift, const float* res, float* y, int B, int C, int HW, int act,
                    void* stream) {
    SRBH_REQUIRE(x && scale && shift && y, "srbh_affine_act_nchw: null pointer");
    SRBH_REQUIRE(B > 0 && C > 0 && HW > 0 && act >= 0 && act <= 2, "srbh_affine_act_nchw: bad arguments");
    const long planes = (long)B * C;
    const bool v4 = (HW % 4 == 0) && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)res) % 16 == 0);
    const int g = grid_for(planes * (v4 ? HW / 4 : HW));
    if (v4)
        hipLaunchKernelGGL(affine_act_nchw_kernel<4>, dim3(g), dim3(256), 0, (hipStream_t)stream, x, scale, shift, res, y, planes, C, HW, act);
    else
        hipLaunchKernelGGL(affine_act_nchw_kernel<1>, dim3(g), dim3(256), 0, (hipStream_t)stream, x, scale, shift, res, y, planes, C, HW, act);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
}  // namespace

extern "C" int srbh_affine_act_nchw(const float* x, const float* scale, const float* shift, float* y, int B, int C, int HW, int act,
                                    void* stream) {
    return affine_act_impl(x, scale, shift, nullptr, y, B, C, HW, act, stream);
}

extern "C" int srbh_affine_act_add_nchw(const float* x, const float* scale, const float* shift, const float* res, float* y, int B, int C,
                                        int HW, int act, void* stream) {
    SRBH_REQUIRE(res, "srbh_affine_act_add_nchw: null residual");
    return affine_act_impl(x, scale, shift, res, y, B, C, HW, act, stream);
}

extern "C" int srbh_affine_act_pool_nchw(const float* x, const float* scale, const float* shift, float* y, float* pooled, int B, int C,
                                         int HW, int act, void* stream) {
    SRBH_REQUIRE(x && scale && shift && y && pooled, "srbh_affine_act_pool_nchw: null pointer");
    SRBH_REQUIRE(B > 0 && C > 0 && HW > 0 && act >= 0 && act <= 2, "srbh_affine_act_pool_nchw: bad arguments");
    const long planes = (long)B * C;
    if (HW < 64 && (HW & (HW - 1)) == 0)
        hipLaunchKernelGGL(affine_act_pool_small_kernel, dim3((unsigned)((planes * HW + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, scale,
                           shift, y, pooled, planes, C, HW, act);
    else
        hipLaunchKernelGGL(affine_act_pool_kernel, dim3((unsigned)((planes + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, scale, shift, y,
                           pooled, planes, C, HW, act);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_se_hidden(const float* pooled, const float* w1, const float* b1, float* hidden, int B, int C, int SQ,
                              void* stream) {
    SRBH_REQUIRE(pooled && w1 && b1 && hidden, "srbh_se_hidden: null pointer");
    SRBH_REQUIRE(B > 0 && C > 0 && SQ > 0 && SQ <= 65535 * 4, "srbh_se_hidden: bad shape");
    hipLaunchKernelGGL(se_hidden_kernel, dim3(B, (SQ + 3) / 4), dim3(256), 0, (hipStream_t)stream, pooled, w1, b1, hidden, C, SQ);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_se_gate(const float* hidden, const float* w2, const float* b2, float* gate, int B, int C, int SQ, void* stream) {
    SRBH_REQUIRE(hidden && w2 && b2 && gate, "srbh_se_gate: null pointer");
    SRBH_REQUIRE(B > 0 && C > 0 && SQ > 0, "srbh_se_gate: bad shape");
    SRBH_REQUIRE((B + SE_GATE_IB - 1) / SE_GATE_IB <= 65535, "srbh_se_gate: batch too large");
    hipLaunchKernelGGL(se_gate_kernel, dim3((unsigned)((C + 15) / 16), (unsigned)((B + SE_GATE_IB - 1) / SE_GATE_IB)), dim3(256), 0,
                       (hipStream_t)stream, hidden, w2, b2, gate, B, C, SQ);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_se_gate_scale(float* y, const float* hidden, const float* w2, const float* b2, int B, int C, int SQ, int HW,
                                  void* stream) {
    SRBH_REQUIRE(y && hidden && w2 && b2, "srbh_se_gate_scale: null pointer");
    SRBH_REQUIRE(B > 0 && C > 0 && SQ > 0 && HW > 0, "srbh_se_gate_scale: bad shape");
    const long planes = (long)B * C;
    if ((HW == 4 || HW == 16 || HW == 64 || HW == 256) && ((uintptr_t)y & 15) == 0)
        hipLaunchKernelGGL(se_gate_scale_quad_kernel, dim3((unsigned)((planes * HW + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, y, hidden,
                           w2, b2, planes, C, SQ, HW);
    else
        hipLaunchKernelGGL(se_gate_scale_kernel, dim3((unsigned)((planes + 3) / 4)), dim3(256), 0, (hipStream_t)stream, y, hidden, w2, b2,
                           planes, C, SQ, HW);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

// (56 / 64 output channels -- the stems of efficientnet-b6 / b7 -- would need a second accumulator pass: one thread holding 64 accumulators spills)
extern "C" int srbh_stem_conv_eval_supported(int Cin, int Cout, int K) { return K == 3 && Cin > 0 && Cin <= 16 && (Cout == 32 || Cout == 40 || Cout == 48); }

/* act(conv3x3(x, w, stride, static padding top = pt / left = pl, zeros beyond) * scale[c] + shift[c]) on NCHW fp32; w: OIHW; act 0 none / 1 SiLU / 2 ReLU */
extern "C" int srbh_stem_conv_eval(const float* x, const float* w, const float* scale, const float* shift, float* y, int B, int Cin, int H, int W,
                                   int Cout, int stride, int pt, int pl, int OH, int OW, int act, void* stream) {
    SRBH_REQUIRE(x && w && scale && shift && y, "srbh_stem_conv_eval: null pointer");
    SRBH_REQUIRE(B > 0 && H > 0 && W > 0 && OH > 0 && OW > 0 && stride >= 1 && pt >= 0 && pl >= 0 && act >= 0 && act <= 2 && srbh_stem_conv_eval_supported(Cin, Cout, 3),
                 "srbh_stem_conv_eval: bad arguments (3x3, Cin <= 16, Cout in {32, 40, 48})");
    const long total = (long)B * OH * OW;
    const dim3 grid((unsigned)((total + 255) / 256));
    const size_t lds = (size_t)Cin * 9 * Cout * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
#define SRBH_STEM(C4_) hipLaunchKernelGGL((stem_conv_eval_kernel<C4_>), grid, dim3(256), lds, st, x, w, scale, shift, y, B, Cin, H, W, stride, pt, pl, OH, OW, act)
    switch (Cout) { case 32: SRBH_STEM(8); break; case 40: SRBH_STEM(10); break; default: SRBH_STEM(12); }
#undef SRBH_STEM
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
