// srbh_vgg.hip -- the plane kernels of the VGG19 perceptual loss (reference SR/srloss.py:61-143) between the wide convs (srbh_wconv3x3):
// input normalisation into an fp16 plane, ReLU / ReLU + 2x2 max-pool plane -> plane and its backward from the saved plane, the one-read
// feature distance with its loss gradient, and the last step of the input gradient.  Contract: include/srbh.h, DESIGN.md 4.
//
// Every kernel owns one 16-byte octet (8 channels) of a pixel record per thread and touches the INTERIOR of its ACT16 planes only: the
// zero borders the convs rely on are written once by whoever allocates the buffers.  No atomics; the distance is bit-reproducible.
#include "srbh_act16.h"

namespace {
using namespace srbh;

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef unsigned uint4e __attribute__((ext_vector_type(4)));

// unit index -> (b, chunk, y, x, octet); octet fastest, so that 4 neighbouring threads cover one 64-byte record
__device__ __forceinline__ void unit_of(long idx, int chunks, int H, int W, int& b, int& ch, int& y, int& x, int& oct) {
    oct = (int)(idx & 3);
    long r = idx >> 2;
    x = (int)(r % W); r /= W;
    y = (int)(r % H); r /= H;
    ch = (int)(r % chunks);
    b = (int)(r / chunks);
}
__device__ __forceinline__ float bf16_lo(unsigned u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __builtin_bit_cast(float, u & 0xffff0000u); }

struct Norm3 {
    float mean[3], std_[3];
    int norm, range;
};

// SR/srloss.py:97-100.  One thread per pixel: the whole 64-byte record (3 values, 29 zeros).
__global__ __launch_bounds__(256) void vgg_input_kernel(const float* __restrict__ x, char* plane, int B, int H, int W, PlaneGeo g, Norm3 n) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * H * W) return;
    const int xx = (int)(idx % W);
    const long r = idx / W;
    const int yy = (int)(r % H), b = (int)(r / H);
    half8 h = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = x[(((long)b * 3 + c) * H + yy) * W + xx];
        if (n.range) v = (v + 1.0f) / 2.0f;
        if (n.norm) v = (v - n.mean[c]) / n.std_[c];      // correctly rounded division (hipcc's default for fp32)
        h[c] = (_Float16)v;
    }
    char* o = plane + rec_off(g, b, 0, yy, xx, 0);
    const half8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    *(half8*)o = h;
    *(half8*)(o + 16) = z;
    *(half8*)(o + 32) = z;
    *(half8*)(o + 48) = z;
}

__device__ __forceinline__ half8 relu8(half8 v) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)v[j] > 0.f ? v[j] : (_Float16)0;
    return v;
}

// out (Ho x Wo) = relu(in), or the 2x2 / stride-2 maximum of relu(in (H x W))
template <int POOL>
__global__ __launch_bounds__(256) void vgg_relu_pool_kernel(const char* __restrict__ in, char* out, int B, int chunks, int Ho, int Wo, PlaneGeo gi,
                                                            PlaneGeo go) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * chunks * Ho * Wo * 4) return;
    int b, ch, y, x, oct;
    unit_of(idx, chunks, Ho, Wo, b, ch, y, x, oct);
    half8 v;
    if (POOL) {
        const char* s = in + rec_off(gi, b, ch, 2 * y, 2 * x, oct);
        v = relu8(*(const half8*)s);
        const half8 v1 = relu8(*(const half8*)(s + PIX_B)), v2 = relu8(*(const half8*)(s + gi.row_b)), v3 = relu8(*(const half8*)(s + gi.row_b + PIX_B));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            _Float16 m = v[j];
            m = (float)v1[j] > (float)m ? v1[j] : m;
            m = (float)v2[j] > (float)m ? v2[j] : m;
            m = (float)v3[j] > (float)m ? v3[j] : m;
            v[j] = m;
        }
    } else {
        v = relu8(*(const half8*)(in + rec_off(gi, b, ch, y, x, oct)));
    }
    *(half8*)(out + rec_off(go, b, ch, y, x, oct)) = v;
}

// out (H x W, bf16) = [add] + (saved > 0) * route(g)
template <int POOL>
__global__ __launch_bounds__(256) void vgg_relu_pool_bwd_kernel(const char* __restrict__ gsrc, const char* __restrict__ saved, const char* __restrict__ add,
                                                                char* out, int B, int chunks, int H, int W, PlaneGeo gf, PlaneGeo gp) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * chunks * H * W * 4) return;
    int b, ch, y, x, oct;
    unit_of(idx, chunks, H, W, b, ch, y, x, oct);
    const half8 sv = *(const half8*)(saved + rec_off(gf, b, ch, y, x, oct));
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    if (POOL) {
        const int py = y >> 1, px = x >> 1;
        if (py < (H >> 1) && px < (W >> 1)) {          // inside a window (the last row / column of an odd size is in none)
            const uint4e gu = *(const uint4e*)(gsrc + rec_off(gp, b, ch, py, px, oct));
            const int k = (y & 1) * 2 + (x & 1);      // this pixel's place in the window, row-major
            half8 wv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                wv[q] = relu8(*(const half8*)(saved + rec_off(gf, b, ch, 2 * py + (q >> 1), 2 * px + (q & 1), oct)));
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float mine = (float)wv[k][j];
                bool first = true;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float o = (float)wv[q][j];
                    first = first && (q < k ? o < mine : o <= mine);
                }
                const float gv = (j & 1) ? bf16_hi(gu[j >> 1]) : bf16_lo(gu[j >> 1]);
                v[j] = (first && (float)sv[j] > 0.f) ? gv : 0.f;
            }
        }
    } else {
        const uint4e gu = *(const uint4e*)(gsrc + rec_off(gp, b, ch, y, x, oct));
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (float)sv[j] > 0.f ? ((j & 1) ? bf16_hi(gu[j >> 1]) : bf16_lo(gu[j >> 1])) : 0.f;
    }
    if (add) {
        const uint4e au = *(const uint4e*)(add + rec_off(gf, b, ch, y, x, oct));
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += (j & 1) ? bf16_hi(au[j >> 1]) : bf16_lo(au[j >> 1]);
    }
    *(uint4e*)(out + rec_off(gf, b, ch, y, x, oct)) = round8<1>(v);
}

// sum of v over the 256 threads in a fixed order; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

constexpr int DIST_UPT = 8;                      // units per thread
constexpr int DIST_UPW = 256 * DIST_UPT;         // units per workgroup

// workgroup w owns units [w * DIST_UPW, +DIST_UPW): thread t adds units t, t + 256, ... in order, then the fixed tree
template <int L2>
__global__ __launch_bounds__(256) void vgg_dist_kernel(const char* __restrict__ fx, const char* __restrict__ fg, char* grad, int B, int chunks, int H,
                                                       int W, PlaneGeo g, float gscale, double* ws) {
#pragma clang fp contract(off)
    __shared__ double red[4];
    const long total = (long)B * chunks * H * W * 4;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < DIST_UPT; ++k) {
        const long idx = (long)blockIdx.x * DIST_UPW + k * 256 + threadIdx.x;
        if (idx < total) {
            int b, ch, y, x, oct;
            unit_of(idx, chunks, H, W, b, ch, y, x, oct);
            const long off = rec_off(g, b, ch, y, x, oct);
            const half8 a = *(const half8*)(fx + off), c = *(const half8*)(fg + off);
            float gv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const double d = (double)a[j] - (double)c[j];      // exact
                if (L2) {
                    s += d * d;
                    gv[j] = gscale * ((float)a[j] - (float)c[j]);
                } else {
                    s += d < 0 ? -d : d;
                    gv[j] = d > 0 ? gscale : (d < 0 ? -gscale : 0.f);
                }
            }
            if (grad) *(uint4e*)(grad + off) = round8<1>(gv);
        }
    }
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) ws[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void vgg_dist_fold_kernel(const double* __restrict__ ws, int n, double coef, int accumulate, double* acc) {
    __shared__ double red[4];
    double s = 0.0;
    for (int k = threadIdx.x; k < n; k += 256) s += ws[k];
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) acc[0] = (accumulate ? acc[0] : 0.0) + coef * t;
}

struct DxScale {
    float std_[3];
    int norm, range;
};
__global__ __launch_bounds__(256) void vgg_dx_kernel(const float* __restrict__ g, float* __restrict__ dx, int B, int H, int W, DxScale sc,
                                                     const float* __restrict__ go) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)B * 3 * H * W) return;
    const int x = (int)(idx % W);
    long r = idx / W;
    const int y = (int)(r % H); r /= H;
    const int c = (int)(r % 3), b = (int)(r / 3);
    float v = g[(((long)b * H + y) * W + x) * 3 + c];
    if (sc.norm) v = v / sc.std_[c];
    if (sc.range) v = v / 2.0f;
    dx[idx] = v * go[0];
}

}  // namespace

extern "C" int srbh_vgg_input_f16(const float* x, void* plane, int B, int H, int W, const float* mean, const float* std_, int range_norm, void* stream) {
    SRBH_REQUIRE(x && plane && B > 0 && H > 0 && W > 0, "srbh_vgg_input_f16: bad arguments");
    SRBH_REQUIRE((mean == nullptr) == (std_ == nullptr), "srbh_vgg_input_f16: mean and std come together");
    Norm3 n;
    n.norm = mean != nullptr;
    n.range = range_norm != 0;
    for (int c = 0; c < 3; ++c) { n.mean[c] = mean ? mean[c] : 0.f; n.std_[c] = std_ ? std_[c] : 1.f; }
    const long total = (long)B * H * W;
    SRBH_REQUIRE(fits(total), "srbh_vgg_input_f16: too large");
    hipLaunchKernelGGL(vgg_input_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, x, (char*)plane, B, H, W, plane_geo(B, 1, H, W), n);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_vgg_relu_pool_f16(const void* in, void* out, int B, int chunks, int H, int W, int pool, void* stream) {
    SRBH_REQUIRE(in && out && B > 0 && chunks > 0 && H > 0 && W > 0, "srbh_vgg_relu_pool_f16: bad arguments");
    SRBH_REQUIRE(!pool || (H >= 2 && W >= 2), "srbh_vgg_relu_pool_f16: a pooled plane needs H, W >= 2 (got %dx%d)", H, W);
    const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
    const long total = (long)B * chunks * Ho * Wo * 4;
    SRBH_REQUIRE(fits(total), "srbh_vgg_relu_pool_f16: too large");
    const PlaneGeo gi = plane_geo(B, chunks, H, W), go = plane_geo(B, chunks, Ho, Wo);
    if (pool) hipLaunchKernelGGL(vgg_relu_pool_kernel<1>, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, (const char*)in, (char*)out, B, chunks, Ho, Wo, gi, go);
    else hipLaunchKernelGGL(vgg_relu_pool_kernel<0>, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, (const char*)in, (char*)out, B, chunks, Ho, Wo, gi, go);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_vgg_relu_pool_bwd_b16(const void* g, const void* saved, const void* add, void* out, int B, int chunks, int H, int W, int pool,
                                          void* stream) {
    SRBH_REQUIRE(g && saved && out && B > 0 && chunks > 0 && H > 0 && W > 0, "srbh_vgg_relu_pool_bwd_b16: bad arguments");
    SRBH_REQUIRE(!pool || (H >= 2 && W >= 2), "srbh_vgg_relu_pool_bwd_b16: a pooled plane needs H, W >= 2 (got %dx%d)", H, W);
    const long total = (long)B * chunks * H * W * 4;
    SRBH_REQUIRE(fits(total), "srbh_vgg_relu_pool_bwd_b16: too large");
    const PlaneGeo gf = plane_geo(B, chunks, H, W), gp = pool ? plane_geo(B, chunks, H / 2, W / 2) : gf;
    if (pool) hipLaunchKernelGGL(vgg_relu_pool_bwd_kernel<1>, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, (const char*)g, (const char*)saved, (const char*)add, (char*)out, B, chunks, H, W, gf, gp);
    else hipLaunchKernelGGL(vgg_relu_pool_bwd_kernel<0>, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, (const char*)g, (const char*)saved, (const char*)add, (char*)out, B, chunks, H, W, gf, gp);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" size_t srbh_vgg_dist_ws_bytes(int B, int chunks, int H, int W) {
    if (B <= 0 || chunks <= 0 || H <= 0 || W <= 0) return 0;
    const long total = (long)B * chunks * H * W * 4;
    return (size_t)((total + DIST_UPW - 1) / DIST_UPW) * sizeof(double);
}

extern "C" int srbh_vgg_dist(const void* fx, const void* fg, int B, int chunks, int H, int W, int l2, double coef, int accumulate, double* acc,
                             float gscale, void* grad, void* ws, void* stream) {
    SRBH_REQUIRE(fx && fg && acc && ws && B > 0 && chunks > 0 && H > 0 && W > 0, "srbh_vgg_dist: bad arguments");
    const long total = (long)B * chunks * H * W * 4;
    const long nwg = (total + DIST_UPW - 1) / DIST_UPW;
    SRBH_REQUIRE(nwg < (1l << 31), "srbh_vgg_dist: too large");
    const PlaneGeo g = plane_geo(B, chunks, H, W);
    hipStream_t st = (hipStream_t)stream;
    if (l2) hipLaunchKernelGGL(vgg_dist_kernel<1>, dim3((unsigned)nwg), dim3(256), 0, st, (const char*)fx, (const char*)fg, (char*)grad, B, chunks, H, W, g, gscale, (double*)ws);
    else hipLaunchKernelGGL(vgg_dist_kernel<0>, dim3((unsigned)nwg), dim3(256), 0, st, (const char*)fx, (const char*)fg, (char*)grad, B, chunks, H, W, g, gscale, (double*)ws);
    SRBH_HIP(hipGetLastError());
    hipLaunchKernelGGL(vgg_dist_fold_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, (int)nwg, coef, accumulate, acc);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_vgg_dx_nchw(const float* g, float* dx, int B, int H, int W, const float* std_, int range_norm, const float* grad_output,
                                void* stream) {
    SRBH_REQUIRE(g && dx && grad_output && B > 0 && H > 0 && W > 0, "srbh_vgg_dx_nchw: bad arguments");
    DxScale sc;
    sc.norm = std_ != nullptr;
    sc.range = range_norm != 0;
    for (int c = 0; c < 3; ++c) sc.std_[c] = std_ ? std_[c] : 1.f;
    const long total = (long)B * 3 * H * W;
    SRBH_REQUIRE(fits(total), "srbh_vgg_dx_nchw: too large");
    hipLaunchKernelGGL(vgg_dx_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, g, dx, B, H, W, sc, grad_output);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
