// srbh_loader.hip -- loader-side tensor math of the training tiles on the device.
//
// Stands in for the per-sample numpy/torch code of reference BH_loader.py:361-392 (myImageFloder_S12_globe.__getitem__):
//   normalise:  (img - min) / (max - min) per band, then clip to datarange      (:361-369; WITHOUT augmentation the nearest
//               x4 up / x0.25 down round trip at :353,365 is the identity for exact factors, and srbh_normalize_clamp does
//               not materialise it.  With `aug=True` (:356-359) it is not: behind a rotation LR pixel (i, j) is a bilinear
//               sample of the blocky up-sampled image at HR position (4i, 4j) -- that path is srbh_aug_image below)
//   labels   :  build = buildhir[height]; weight = heightweight[build]           (:373-375)
//               height_aggre = aggregate_torch(height, 0.25)                     (:386, aggregate_utils.py:29-41)
//               weight_aggre = heightweight[buildhir[height_aggre.long()]]       (:389-391)
// One thread per 4x4 label cell produces the 16 full-resolution outputs and the aggregated pair.
//
// Training augmentation (:356-359, :735-737: Compose([Flip, RandomGridShuffle(2x2), Rotate]), each with p = 0.5) as two gather
// kernels over an HR grid of Hg x Wg pixels (DESIGN.md 3.x holds the definition; it is this project's own, modelled on what
// albumentations / cv2 are understood to do and not tested against them).  Per destination pixel the chain runs backwards:
//   rotate's inverse map in fixed point (host-built int32 tables ax, bx, X0, Y0 per image) -> REFLECT_101 fold (general, period
//   2(N-1)) -> the grid shuffle's source cell -> the flip -> the source pixel; a band stored at 1/up of the grid is read at
//   (u / up, v / up), which IS the nearest x`up` up-sampling, never materialised.
// aug_image_kernel : one thread per destination pixel; the four corner offsets and weights are computed once and reused over the
//                    channels; consecutive lanes store consecutive x.  Bilinear, then (v - min) / range and the clip.
// aug_label_prep_kernel : one thread per 4x4 cell as label_prep_kernel, each label pixel a nearest sample.
// Every index is folded / masked on the device, so no content of the parameter arrays can take a read outside the source.
//
// Inference tiles (:933-993, gridimgLoader.__getitem__): grid_tiles_kernel cuts a batch of windows out of a city's two device rasters
// (uint16 / int16 / float32, channel-major), concatenates the bands and normalises as normalize_clamp_kernel does, without the clip;
// outside the window, and outside the raster, a tile is +0.0f.
#include "srbh_internal.h"

namespace {
using namespace srbh;

__global__ void label_prep_kernel(const unsigned char* __restrict__ height, int B, int H, int W,
                                  const unsigned char* __restrict__ lut, const float* __restrict__ cw,
                                  long long* build, float* height_f, float* weight, float* height_aggre,
                                  float* weight_aggre) {
    const int oh = H / 4, ow = W / 4;
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)B * oh * ow;
    if (idx >= total) return;
    const int ox = idx % ow;
    long r = idx / ow;
    const int oy = r % oh;
    const int b = r / oh;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long row = ((long)b * H + oy * 4 + i) * W + ox * 4;
        const uchar4 h4 = *(const uchar4*)(height + row);
        const unsigned char hv[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cls = lut[hv[j]];
            build[row + j] = cls;
            height_f[row + j] = (float)hv[j];
            weight[row + j] = cw[cls];
            s1 += (float)hv[j];
            s2 += 1.f;                       // (data >= 0) is always true for uint8 labels
        }
    }
    const float ha = s1 / (s2 + 1e-10f);
    height_aggre[idx] = ha;
    int hi = (int)ha;                         // .long(): truncation
    hi = hi < 0 ? 0 : (hi > 255 ? 255 : hi);
    weight_aggre[idx] = cw[lut[hi]];
}

__global__ void normalize_clamp_kernel(const float* __restrict__ src, float* __restrict__ dst, long n, int C, long hw,
                                       const float* __restrict__ mins, const float* __restrict__ ranges, float lo, float hi,
                                       int clamp) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const int c = (int)((i / hw) % C);
        float v = (src[i] - mins[c]) / ranges[c];
        if (clamp) v = v < lo ? lo : (v > hi ? hi : v);
        dst[i] = v;
    }
}

// ---- training augmentation ------------------------------------------------------------------------------------------------------
// REFLECT_101 of any integer into [0, n): period 2(n - 1), n >= 2.
__device__ __forceinline__ int fold101(int i, int n) {
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

// One image's flip code, shuffle and grid size.  src(u, v): the source pixel (after shuffle and flip) of HR grid pixel (u, v), both
// inside the grid.  perm is packed two bits per destination cell; both it and the flip code are masked, so any content stays in bounds.
struct AugCell {
    int Hg, Wg, hh, wh, flip, perm;
    __device__ __forceinline__ void src(int u, int v, int& su, int& sv) const {
        const int cx = u >= wh, cy = v >= hh;
        const int s = (perm >> (2 * (cy * 2 + cx))) & 3;
        su = u - cx * wh + (s & 1) * wh;
        sv = v - cy * hh + (s >> 1) * hh;
        if (flip & 1) su = Wg - 1 - su;
        if (flip & 2) sv = Hg - 1 - sv;
    }
};

__device__ __forceinline__ AugCell aug_cell(const int* __restrict__ flip, const int* __restrict__ perm, int b, int Hg, int Wg) {
    AugCell a;
    a.Hg = Hg, a.Wg = Wg, a.hh = Hg / 2, a.wh = Wg / 2;
    a.flip = flip[b] & 3;
    const int4 p = *(const int4*)(perm + 4 * (long)b);
    a.perm = (p.x & 3) | (p.y & 3) << 2 | (p.z & 3) << 4 | (p.w & 3) << 6;
    return a;
}

// (table sums in unsigned: wrap-around instead of undefined behaviour should a caller hand in tables of another grid)
__device__ __forceinline__ int tsum(int a, int b, int round) { return (int)((unsigned)a + (unsigned)b + (unsigned)round); }

__global__ void aug_image_kernel(const float* __restrict__ src, int B, int C, int Hs, int Ws, int up, float* __restrict__ dst,
                                 int step, const int* __restrict__ flip, const int* __restrict__ perm,
                                 const int* __restrict__ tables, const float* __restrict__ mins,
                                 const float* __restrict__ ranges, float lo, float hi, int clamp) {
    const int Hg = Hs * up, Wg = Ws * up, Hd = Hg / step, Wd = Wg / step;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)B * Hd * Wd) return;
    const int j = idx % Wd;
    const long r = idx / Wd;
    const int i = r % Hd;
    const int b = r / Hd;
    const int* t = tables + (long)b * (2 * Wg + 2 * Hg);      // ax[Wg], bx[Wg], X0[Hg], Y0[Hg]
    const int gx = j * step, gy = i * step;
    const int X = tsum(t[2 * Wg + gy], t[gx], 16) >> 5;
    const int Y = tsum(t[2 * Wg + Hg + gy], t[Wg + gx], 16) >> 5;
    const float fx = (float)(X & 31) * (1.f / 32.f), fy = (float)(Y & 31) * (1.f / 32.f);
    const int x0 = fold101(X >> 5, Wg), x1 = fold101((X >> 5) + 1, Wg);
    const int y0 = fold101(Y >> 5, Hg), y1 = fold101((Y >> 5) + 1, Hg);
    const AugCell cell = aug_cell(flip, perm, b, Hg, Wg);
    int off[4];
    {
        const int xs[2] = {x0, x1}, ys[2] = {y0, y1};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int su, sv;
            cell.src(xs[k & 1], ys[k >> 1], su, sv);
            off[k] = (sv / up) * Ws + su / up;
        }
    }
    const float w00 = (1.f - fx) * (1.f - fy), w01 = fx * (1.f - fy), w10 = (1.f - fx) * fy, w11 = fx * fy;     // exact: multiples of 2^-10
    const long plane_s = (long)Hs * Ws, plane_d = (long)Hd * Wd;
    const float* s = src + (long)b * C * plane_s;
    float* d = dst + (long)b * C * plane_d + (long)i * Wd + j;
    for (int c = 0; c < C; ++c, s += plane_s, d += plane_d) {
        float v = w00 * s[off[0]] + w01 * s[off[1]] + w10 * s[off[2]] + w11 * s[off[3]];
        if (mins) {
            v = (v - mins[c]) / ranges[c];
            if (clamp) v = v < lo ? lo : (v > hi ? hi : v);
        }
        *d = v;
    }
}

__global__ void aug_label_prep_kernel(const unsigned char* __restrict__ height, int B, int H, int W,
                                      const int* __restrict__ flip, const int* __restrict__ perm,
                                      const int* __restrict__ tables, const unsigned char* __restrict__ lut,
                                      const float* __restrict__ cw, long long* build, float* height_f, float* weight,
                                      float* height_aggre, float* weight_aggre, unsigned char* label_out) {
    const int oh = H / 4, ow = W / 4;
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)B * oh * ow;
    if (idx >= total) return;
    const int ox = idx % ow;
    long r = idx / ow;
    const int oy = r % oh;
    const int b = r / oh;
    const int* t = tables + (long)b * (2 * W + 2 * H);
    const AugCell cell = aug_cell(flip, perm, b, H, W);
    const unsigned char* img = height + (long)b * H * W;
    const int4 ax = *(const int4*)(t + ox * 4), bx = *(const int4*)(t + W + ox * 4);
    const int axv[4] = {ax.x, ax.y, ax.z, ax.w}, bxv[4] = {bx.x, bx.y, bx.z, bx.w};
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int y = oy * 4 + i;
        const long row = ((long)b * H + y) * W + ox * 4;
        const int X0 = t[2 * W + y], Y0 = t[2 * W + H + y];
        unsigned char hv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int su, sv;
            cell.src(fold101(tsum(X0, axv[j], 512) >> 10, W), fold101(tsum(Y0, bxv[j], 512) >> 10, H), su, sv);
            hv[j] = img[(long)sv * W + su];
        }
        if (label_out) *(uchar4*)(label_out + row) = make_uchar4(hv[0], hv[1], hv[2], hv[3]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cls = lut[hv[j]];
            build[row + j] = cls;
            height_f[row + j] = (float)hv[j];
            weight[row + j] = cw[cls];
            s1 += (float)hv[j];
            s2 += 1.f;
        }
    }
    const float ha = s1 / (s2 + 1e-10f);
    height_aggre[idx] = ha;
    int hi = (int)ha;
    hi = hi < 0 ? 0 : (hi > 255 ? 255 : hi);
    weight_aggre[idx] = cw[lut[hi]];
}

constexpr int AUG_MAX_GRID = 32768;      // |coordinate| * 1024 stays far inside int32 (the sampling position overshoots by < 1.5 N)

// ---- inference tiles from a city's rasters (BH_loader.py:933-993) ------------------------------------------------------------------
// One element of a raster as float: exact for all three types (16-bit integers fit fp32's 24-bit significand).
__device__ __forceinline__ float grid_load(const void* src, int type, long long o) {
    if (type == SRBH_GRID_U16) return (float)((const unsigned short*)src)[o];
    if (type == SRBH_GRID_I16) return (float)((const short*)src)[o];
    return ((const float*)src)[o];
}

// One thread: four consecutive pixels of one tile row, one 16-byte store (tile % 4 == 0: a store never straddles rows).  Consecutive
// lanes read consecutive groups of four source pixels of the same raster row.  A pixel is loaded only when it lies in the window AND in
// the raster -- whatever pos holds, no load leaves the source; the window arithmetic is 64-bit so that no content of pos overflows it.
__global__ void __launch_bounds__(256) grid_tiles_kernel(const void* __restrict__ srcA, int typeA, int CA_used,
                                                         const void* __restrict__ srcB, int typeB, int CB, int H, int W,
                                                         const int* __restrict__ pos, int N, const float* __restrict__ mins,
                                                         const float* __restrict__ ranges, float* __restrict__ dst, int tile) {
    const int q = tile / 4, C = CA_used + CB;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)N * C * tile * q) return;
    const int i0 = (int)(idx % q) * 4;
    long long r = idx / q;
    const int j = (int)(r % tile);
    r /= tile;
    const int c = (int)(r % C);
    const int* p = pos + 4 * (r / C);
    const int xoff = p[0], yoff = p[1], xcount = p[2], ycount = p[3];
    const long long y = (long long)yoff + j;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (j < ycount && y >= 0 && y < H) {
        const bool a = c < CA_used;
        const void* src = a ? srcA : srcB;
        const int type = a ? typeA : typeB;
        const long long row = ((long long)(a ? c : c - CA_used) * H + y) * W;
        const float mn = mins[c], rg = ranges[c];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long x = (long long)xoff + i0 + k;
            if (i0 + k < xcount && x >= 0 && x < W) v[k] = (grid_load(src, type, row + x) - mn) / rg;
        }
    }
    *(float4*)(dst + idx * 4) = make_float4(v[0], v[1], v[2], v[3]);
}

}  // namespace

extern "C" int srbh_grid_tiles(const void* srcA, int typeA, int CA, int CA_used, const void* srcB, int typeB, int CB, int H, int W,
                               const int* pos, int N, const float* mins, const float* ranges, float* dst, int tile, void* stream) {
    SRBH_REQUIRE(srcA && pos && dst && mins && ranges, "srbh_grid_tiles: null pointer");
    SRBH_REQUIRE(CB >= 0 && (srcB != nullptr) == (CB > 0), "srbh_grid_tiles: srcB and CB=%d must both be given or both be absent", CB);
    SRBH_REQUIRE(typeA >= SRBH_GRID_F32 && typeA <= SRBH_GRID_I16 && (!srcB || (typeB >= SRBH_GRID_F32 && typeB <= SRBH_GRID_I16)),
                 "srbh_grid_tiles: unknown element type typeA=%d typeB=%d (0 float32, 1 uint16, 2 int16)", typeA, typeB);
    SRBH_REQUIRE(CA_used >= 1 && CA_used <= CA, "srbh_grid_tiles: CA_used=%d must lie in 1..CA=%d", CA_used, CA);
    SRBH_REQUIRE(N > 0 && H > 0 && W > 0, "srbh_grid_tiles: bad geometry N=%d H=%d W=%d", N, H, W);
    SRBH_REQUIRE(tile >= 4 && tile % 4 == 0 && tile <= 256, "srbh_grid_tiles: tile=%d must be a multiple of 4 in 4..256", tile);
    SRBH_REQUIRE(((uintptr_t)dst & 15) == 0, "srbh_grid_tiles: dst must be 16-byte aligned");
    const long long per_tile = ((long long)CA_used + CB) * tile * (tile / 4);      // threads per tile: below 2^47
    SRBH_REQUIRE(N <= 0x7fffffffLL * 256 / per_tile, "srbh_grid_tiles: too many workgroups");
    const long long total = N * per_tile;
    hipLaunchKernelGGL(grid_tiles_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, srcA, typeA, CA_used,
                       srcB, typeB, CB, H, W, pos, N, mins, ranges, dst, tile);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_aug_image(const float* src, int B, int C, int Hs, int Ws, int up, float* dst, int step, const int* flip,
                              const int* perm, const int* tables, const float* mins, const float* ranges, float lo, float hi,
                              int clamp, void* stream) {
    SRBH_REQUIRE(src && dst && flip && perm && tables, "srbh_aug_image: null pointer");
    SRBH_REQUIRE((mins == nullptr) == (ranges == nullptr), "srbh_aug_image: mins and ranges go together");
    SRBH_REQUIRE(B > 0 && C > 0 && Hs > 0 && Ws > 0, "srbh_aug_image: bad geometry B=%d C=%d Hs=%d Ws=%d", B, C, Hs, Ws);
    SRBH_REQUIRE(up >= 1 && step >= 1 && Hs <= AUG_MAX_GRID / up && Ws <= AUG_MAX_GRID / up,
                 "srbh_aug_image: up=%d step=%d must be >= 1 and the grid at most %d a side", up, step, AUG_MAX_GRID);
    const int Hg = Hs * up, Wg = Ws * up;
    SRBH_REQUIRE(Hg % 8 == 0 && Wg % 8 == 0, "srbh_aug_image: grid %d x %d must be multiples of 8", Hg, Wg);
    SRBH_REQUIRE(Hg % step == 0 && Wg % step == 0, "srbh_aug_image: step=%d does not divide the grid %d x %d", step, Hg, Wg);
    SRBH_REQUIRE(((uintptr_t)perm & 15) == 0, "srbh_aug_image: perm must be 16-byte aligned");
    const long total = (long)B * (Hg / step) * (Wg / step);
    SRBH_REQUIRE((total + 255) / 256 <= 0x7fffffffL, "srbh_aug_image: too many workgroups");
    hipLaunchKernelGGL(aug_image_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, src, B, C, Hs, Ws, up, dst,
                       step, flip, perm, tables, mins, ranges, lo, hi, clamp);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_aug_label_prep(const unsigned char* height, int B, int H, int W, const int* flip, const int* perm,
                                   const int* tables, const unsigned char* buildhir_lut, const float* class_weight,
                                   long long* build, float* height_f, float* weight, float* height_aggre, float* weight_aggre,
                                   unsigned char* label_out, void* stream) {
    SRBH_REQUIRE(height && flip && perm && tables && buildhir_lut && class_weight && build && height_f && weight && height_aggre &&
                     weight_aggre,
                 "srbh_aug_label_prep: null pointer");
    SRBH_REQUIRE(B > 0 && H > 0 && W > 0 && H <= AUG_MAX_GRID && W <= AUG_MAX_GRID,
                 "srbh_aug_label_prep: bad geometry B=%d H=%d W=%d", B, H, W);
    SRBH_REQUIRE(H % 8 == 0 && W % 8 == 0, "srbh_aug_label_prep: H=%d, W=%d must be multiples of 8", H, W);
    SRBH_REQUIRE((((uintptr_t)perm | (uintptr_t)tables) & 15) == 0, "srbh_aug_label_prep: perm and tables must be 16-byte aligned");
    SRBH_REQUIRE(label_out == nullptr || ((uintptr_t)label_out & 3) == 0, "srbh_aug_label_prep: label_out must be 4-byte aligned");
    const long total = (long)B * (H / 4) * (W / 4);
    SRBH_REQUIRE((total + 255) / 256 <= 0x7fffffffL, "srbh_aug_label_prep: too many workgroups");
    hipLaunchKernelGGL(aug_label_prep_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, height, B, H, W, flip,
                       perm, tables, buildhir_lut, class_weight, build, height_f, weight, height_aggre, weight_aggre, label_out);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_label_prep(const unsigned char* height, int B, int H, int W, const unsigned char* buildhir_lut,
                               const float* class_weight, long long* build, float* height_f, float* weight,
                               float* height_aggre, float* weight_aggre, void* stream) {
    SRBH_REQUIRE(height && buildhir_lut && class_weight && build && height_f && weight && height_aggre && weight_aggre,
                 "srbh_label_prep: null pointer");
    SRBH_REQUIRE(B > 0 && H > 0 && W > 0 && H % 4 == 0 && W % 4 == 0, "srbh_label_prep: H, W must be multiples of 4");
    SRBH_REQUIRE(((uintptr_t)height & 3) == 0, "srbh_label_prep: height must be 4-byte aligned");      // read as uchar4
    long total = (long)B * (H / 4) * (W / 4);
    hipLaunchKernelGGL(label_prep_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, height, B, H, W,
                       buildhir_lut, class_weight, build, height_f, weight, height_aggre, weight_aggre);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_normalize_clamp(const float* src, float* dst, int B, int C, int H, int W, const float* mins,
                                    const float* ranges, float lo, float hi, int clamp, void* stream) {
    SRBH_REQUIRE(src && dst && mins && ranges && B > 0 && C > 0 && H > 0 && W > 0, "srbh_normalize_clamp: bad arguments");
    long n = (long)B * C * H * W;
    long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(normalize_clamp_kernel, dim3(blocks < 4096 ? blocks : 4096), dim3(256), 0, (hipStream_t)stream, src,
                       dst, n, C, (long)H * W, mins, ranges, lo, hi, clamp);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
