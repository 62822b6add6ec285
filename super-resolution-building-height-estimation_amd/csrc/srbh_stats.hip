// srbh_stats.hip -- the dataset statistics every loader starts from, computed where the data already lies (reference
// stats_dataset_globe.py: main_stats :61-101 asks GDAL for ComputeStatistics(False) per tile and band, main_stats_buildingheight :133-159
// counts every height label with np.unique).
//
// srbh_band_stats: per (image, band) {min, max, mean, std} and the count of valid pixels.  GDAL is not available where this project is
// built and tested, so the definition below is the PROJECT'S OWN statement of what ComputeStatistics(False) is understood to return (an
// exact scan, not the approximate overview form): every pixel that is neither NaN nor equal to the optional nodata value counts; std is
// the population form sqrt(M2 / count); a band without a valid pixel gives count 0 and four NaNs.
//
// Arithmetic: float64 behind the exact conversion of each value, the corrected two-pass form (Chan, Golub & LeVeque 1983):
//   pass 1   min, max, count, sum                 -> mean = sum / count
//   pass 2   s1 = sum (x - mean), s2 = sum (x - mean)^2   -> M2 = s2 - s1 * s1 / count
// A one-pass sum of squares loses every digit of the variance of a band such as {65534, 65535} or 1000 + 1e-3 * rand; this form does not.
//
// Form: ONE workgroup of 256 lanes per (image, band).  The band's H * W values are numbered row-major and cut into groups of 16 bytes (4
// floats, 8 sixteen-bit values); lane t owns the groups t, t + 256, ... and adds its values in that order (lane-strided partials), the 64
// lanes of a wave are folded by a shuffle tree, and the four waves are added in wave order through LDS.  That order depends on H, W and the
// element type alone: an image's numbers depend neither on the run, nor on the batch it travels in, nor on N -- and not on HOW a group was
// loaded: one 16-byte load where the base and the three strides allow it, element by element otherwise, the same values to the same lane
// in the same order.  A band of at most 4096 values (64 x 64: 16 per lane) stays in registers between the passes and is read once; a larger
// one is walked twice, the second walk out of the cache.  No floating-point atomics, no workspace.
//
// The kernel is bound by instruction issue, not by memory (a wave-instruction is four cycles on a 16-lane SIMD whatever its width), so
// pass 1 does in the element's own type what is exact there: min and max as float / int32, the sum of a 16-bit type as an integer (every
// partial sum of the float64 order is below 2^53, so the integer sum IS that sum), the count as a population count of the validity mask;
// and a wave whose group holds valid pixels only skips the masking.  Neither changes a bit: a masked-out pixel adds +0.0.
//
// srbh_label_hist: the exact 256-bin histogram of uint8 labels.  A workgroup takes LH_RANGE = 65536 consecutive labels of one image (so its
// 32-bit counters cannot wrap), 16 labels per lane and load.  Real labels are mostly 0, and 64 lanes adding to one LDS counter take turns:
//   * label 0 never goes to LDS: a lane counts the zero bytes of its 16 labels with a few bit operations into a register; the wave adds
//     its lanes' counts once, at the end;
//   * of the other labels a lane adds a RUN of equal values once (zeros in between do not end a run), into the sub-histogram of its own
//     wave (four copies in LDS);
//   * a wave whose 1024 labels are all one non-zero value adds them with a single LDS operation.
// The workgroup's counts go to its slot of the workspace; a second kernel adds the slots into int64.  Integer adds only: nothing here has
// an order.
#include <limits.h>
#include <string.h>
#include "srbh_internal.h"

namespace {
using namespace srbh;

constexpr int BS_REG = 16;                       // values a lane keeps in registers between the passes
constexpr long BS_SMALL = 256L * BS_REG;         // largest band that is read once

template <int TYPE> struct Elem;
template <> struct Elem<SRBH_GRID_F32> { typedef float T; };
template <> struct Elem<SRBH_GRID_U16> { typedef unsigned short T; };
template <> struct Elem<SRBH_GRID_I16> { typedef short T; };

struct BandParams {
    const void* src;
    long s_img, s_band, s_row;      // element strides; the column stride is 1
    int C, H, W;
    int vec;                        // 16-byte loads are allowed: base and strides are multiples of 16 bytes, and no group straddles a row end
    int flat;                       // s_row == W: a band is one contiguous run
    int has_nodata;                 // a nodata value was given AND the element type can hold it (no pixel equals any other value)
    int nodata_bits;                // that value in the element type: the bits of the float, or the integer
    double* stats;                  // [N][C][4]
    long long* count;               // [N][C]
};

__device__ __forceinline__ float lo(float a, float b) { return fminf(a, b); }      // (neither operand is ever a NaN here)
__device__ __forceinline__ float hi(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ int lo(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int hi(int a, int b) { return a > b ? a : b; }

// the V values of group g of a band; ok bit j: value j exists (inside the band), is no NaN and is not the nodata value.  A value outside the
// band is T(0).
template <class T, int V>
__device__ __forceinline__ unsigned load_group(const BandParams& p, const T* band, long g, long HW, T* raw) {
    typedef T vec_t __attribute__((ext_vector_type(V)));
    const long e0 = g * V;
    unsigned ok = 0;
    if (p.vec && e0 + V <= HW) {
        long off = e0;
        if (!p.flat) { const long r = e0 / p.W; off = r * p.s_row + (e0 - r * p.W); }
        const vec_t v = *reinterpret_cast<const vec_t*>(band + off);
#pragma unroll
        for (int j = 0; j < V; ++j) raw[j] = v[j];
        ok = (1u << V) - 1u;
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const long e = e0 + j;
            raw[j] = T(0);
            if (e < HW) {
                long off = e;
                if (!p.flat) { const long r = e / p.W; off = r * p.s_row + (e - r * p.W); }
                raw[j] = band[off];
                ok |= 1u << j;
            }
        }
    }
    if (std::is_floating_point<T>::value) {
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (raw[j] != raw[j]) ok &= ~(1u << j);
    }
    if (p.has_nodata) {                                               // uniform
        T nd;
        if (std::is_floating_point<T>::value) nd = (T)__int_as_float(p.nodata_bits);
        else nd = (T)p.nodata_bits;
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (raw[j] == nd) ok &= ~(1u << j);
    }
    return ok;
}

template <int TYPE, bool SMALL>
__global__ __launch_bounds__(256) void band_stats_kernel(const BandParams p) {
    typedef typename Elem<TYPE>::T T;
    constexpr bool FLT = TYPE == SRBH_GRID_F32;
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int NG = BS_REG / V;                                    // groups a lane holds in the read-once form
    constexpr unsigned FULL = (1u << V) - 1u;
    typedef typename std::conditional<FLT, float, int>::type M;       // min / max: exact in the element's own kind
    // a lane's sum: float64 for floats; for the 16-bit types an integer that cannot overflow (16 values in the read-once form, a wave's 1024
    // below 2^27; 64-bit otherwise) and equals the float64 sum of the same values in any order
    typedef typename std::conditional<FLT, double, typename std::conditional<SMALL, int, long long>::type>::type S;
    typedef typename std::conditional<SMALL, int, long long>::type N;
    __shared__ double red[2][4];
    __shared__ M red_mn[4], red_mx[4];
    __shared__ long long red_n[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long nc = blockIdx.x;                                       // n * C + c
    const long n = nc / p.C, c = nc - n * p.C;
    const T* band = (const T*)p.src + n * p.s_img + c * p.s_band;
    const long HW = (long)p.H * p.W, groups = (HW + V - 1) / V;

    M mn, mx;
    if (FLT) { mn = (M)__builtin_inff(); mx = (M)-__builtin_inff(); }
    else { mn = (M)INT_MAX; mx = (M)INT_MIN; }
    S sum = S(0);
    N cnt = 0;
    auto pass1 = [&](const T* raw, unsigned ok) {
        cnt += (N)__popc(ok);
        if (__all(ok == FULL)) {                                      // the whole wave's groups are valid: no masks
#pragma unroll
            for (int j = 0; j < V; ++j) { const M v = (M)raw[j]; mn = lo(mn, v); mx = hi(mx, v); sum += (S)raw[j]; }
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const bool k = (ok >> j) & 1u;
                const M v = (M)raw[j];
                mn = k ? lo(mn, v) : mn;
                mx = k ? hi(mx, v) : mx;
                sum += k ? (S)raw[j] : S(0);
            }
        }
    };
    T keep[SMALL ? BS_REG : 1];
    unsigned keep_ok[SMALL ? NG : 1];
    if (SMALL) {
#pragma unroll
        for (int k = 0; k < NG; ++k) keep_ok[k] = load_group<T, V>(p, band, t + 256L * k, HW, &keep[k * V]);
#pragma unroll
        for (int k = 0; k < NG; ++k) pass1(&keep[k * V], keep_ok[k]);
    } else {
        for (long g = t; g < groups; g += 256) {
            T raw[V];
            const unsigned ok = load_group<T, V>(p, band, g, HW, raw);
            pass1(raw, ok);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = lo(mn, __shfl_down(mn, o, 64));
        mx = hi(mx, __shfl_down(mx, o, 64));
        cnt += __shfl_down(cnt, o, 64);
        sum += __shfl_down(sum, o, 64);
    }
    if (lane == 0) { red_mn[wave] = mn; red_mx[wave] = mx; red_n[wave] = (long long)cnt; red[0][wave] = (double)sum; }
    __syncthreads();
    const long long count = ((red_n[0] + red_n[1]) + red_n[2]) + red_n[3];
    const double mean = (((red[0][0] + red[0][1]) + red[0][2]) + red[0][3]) / (double)count;

    double s1 = 0.0, s2 = 0.0;
    auto pass2 = [&](const T* raw, unsigned ok) {
        if (__all(ok == FULL)) {
#pragma unroll
            for (int j = 0; j < V; ++j) { const double d = (double)raw[j] - mean; s1 += d; s2 = fma(d, d, s2); }
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const double d = ((ok >> j) & 1u) ? (double)raw[j] - mean : 0.0;      // (+0.0: adds nothing)
                s1 += d;
                s2 = fma(d, d, s2);
            }
        }
    };
    if (count > 0) {                                                  // uniform
        if (SMALL) {
#pragma unroll
            for (int k = 0; k < NG; ++k) pass2(&keep[k * V], keep_ok[k]);
        } else {
            for (long g = t; g < groups; g += 256) {
                T raw[V];
                const unsigned ok = load_group<T, V>(p, band, g, HW, raw);
                pass2(raw, ok);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_down(s1, o, 64); s2 += __shfl_down(s2, o, 64); }
    __syncthreads();                                                  // (red[0] has been read by every lane)
    if (lane == 0) { red[0][wave] = s1; red[1][wave] = s2; }
    __syncthreads();
    if (t == 0) {
        double* o = p.stats + nc * 4;
        p.count[nc] = count;
        if (count > 0) {
            s1 = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
            s2 = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
            M m = red_mn[0], mm = red_mx[0];
#pragma unroll
            for (int w = 1; w < 4; ++w) { m = lo(m, red_mn[w]); mm = hi(mm, red_mx[w]); }
            double m2 = s2 - s1 * s1 / (double)count;
            m2 = m2 < 0.0 ? 0.0 : m2;
            o[0] = (double)m; o[1] = (double)mm; o[2] = mean; o[3] = sqrt(m2 / (double)count);
        } else {
            o[0] = o[1] = o[2] = o[3] = __builtin_nan("");
        }
    }
}

template <int TYPE>
inline void band_launch(bool small, long grid, hipStream_t st, const BandParams& p) {
    if (small) hipLaunchKernelGGL((band_stats_kernel<TYPE, true>), dim3((unsigned)grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((band_stats_kernel<TYPE, false>), dim3((unsigned)grid), dim3(256), 0, st, p);
}

// ---- label histogram ------------------------------------------------------------------------------------------------------------------
constexpr int LH_PF = 4;                               // 16-byte loads a lane has in flight
constexpr int LH_ITERS = 4;                            // such rounds per workgroup
constexpr long LH_RANGE = 256L * 16 * LH_PF * LH_ITERS;      // labels per workgroup: 65536
static_assert(LH_RANGE < (1LL << 32), "a workgroup counts in 32 bits: it must see fewer than 2^32 labels");
constexpr int LH_FOLD_BLOCKS = 16;                     // the fold: 16 bins per block, 16 groups of slots per block

inline long lh_slots(long HW) { return (HW + LH_RANGE - 1) / LH_RANGE; }

// how many of the four bytes of w are zero
__device__ __forceinline__ unsigned zero_bytes(unsigned w) {
    const unsigned t = (w & 0x7f7f7f7fu) + 0x7f7f7f7fu;               // bit 7 of a byte: its low seven bits are not all clear
    return __popc(~(t | w | 0x7f7f7f7fu));                           // bit 7 set exactly where the byte is 0
}

__global__ __launch_bounds__(256) void label_hist_kernel(const unsigned char* __restrict__ labels, long s_img, long HW, long slots, int vec,
                                                         unsigned* __restrict__ ws) {
    __shared__ unsigned hist[4][256];
    const int t = threadIdx.x, wave = t >> 6;
    for (int i = t; i < 4 * 256; i += 256) (&hist[0][0])[i] = 0u;
    __syncthreads();
    const long wg = blockIdx.x, n = wg / slots, slot = wg - n * slots;
    const unsigned char* img = labels + n * s_img;
    unsigned* h = hist[wave];
    unsigned zeros = 0;                                               // this lane's labels 0
    unsigned cur = 0, run = 0;                                        // the open run of a non-zero label
#pragma unroll 1
    for (int it = 0; it < LH_ITERS; ++it) {
        const long p0 = slot * LH_RANGE + (long)it * (256 * 16 * LH_PF);
        if (p0 >= HW) break;                                          // uniform
        uint4 q[LH_PF];
        int nv[LH_PF];                                                // labels of the group inside the image: 0 .. 16
#pragma unroll
        for (int i = 0; i < LH_PF; ++i) {
            const long e0 = p0 + ((long)i * 256 + t) * 16;
            const long left = HW - e0;
            nv[i] = left >= 16 ? 16 : (left > 0 ? (int)left : 0);
            if (vec && nv[i] == 16) {
                q[i] = *reinterpret_cast<const uint4*>(img + e0);
            } else {                                                  // (bytes outside the image stay 0)
                unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (j < nv[i]) w[j >> 2] |= (unsigned)img[e0 + j] << (8 * (j & 3));
                q[i] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
#pragma unroll
        for (int i = 0; i < LH_PF; ++i) {
            const unsigned w[4] = {q[i].x, q[i].y, q[i].z, q[i].w};
            const unsigned first = w[0] & 0xffu, rep = first * 0x01010101u;
            const bool one = nv[i] == 16 && w[0] == rep && w[1] == rep && w[2] == rep && w[3] == rep;
            // the whole wave holds 1024 copies of one non-zero value: one add
            if (__all(one && first != 0u && first == (unsigned)__shfl((int)first, 0, 64))) {
                if ((t & 63) == 0) atomicAdd(&h[first], 64u * 16u);
                continue;                                             // uniform
            }
            zeros += zero_bytes(w[0]) + zero_bytes(w[1]) + zero_bytes(w[2]) + zero_bytes(w[3]) - (unsigned)(16 - nv[i]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (w[k] == 0u) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned v = (w[k] >> (8 * j)) & 0xffu;
                    if (v != 0u) {
                        if (v != cur) {
                            if (run) atomicAdd(&h[cur], run);
                            cur = v;
                            run = 0;
                        }
                        ++run;
                    }
                }
            }
        }
    }
    if (run) atomicAdd(&h[cur], run);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) zeros += __shfl_down(zeros, o, 64);
    if ((t & 63) == 0 && zeros) atomicAdd(&h[0], zeros);
    __syncthreads();
    ws[wg * 256 + t] = (hist[0][t] + hist[1][t]) + (hist[2][t] + hist[3][t]);
}

// block b owns the bins 16 b .. 16 b + 15; thread t adds the slots (t >> 4), (t >> 4) + 16, ... of bin 16 b + (t & 15) (64-byte segments of
// the workspace), then the 16 partial counts of a bin are added through LDS
__global__ __launch_bounds__(256) void label_hist_fold_kernel(const unsigned* __restrict__ ws, long nwg, long long* __restrict__ hist) {
    __shared__ long long part[16][16];
    const int t = threadIdx.x, bin = blockIdx.x * 16 + (t & 15), grp = t >> 4;
    long long a = 0;
#pragma unroll 8
    for (long k = grp; k < nwg; k += 16) a += ws[k * 256 + bin];
    part[grp][t & 15] = a;
    __syncthreads();
    if (t < 16) {
        long long s = 0;
#pragma unroll
        for (int g = 0; g < 16; ++g) s += part[g][t];
        hist[blockIdx.x * 16 + t] = s;
    }
}

}  // namespace

extern "C" int srbh_band_stats(const void* src, int type, const long* strides, int N, int C, int H, int W, const double* nodata,
                               double* stats, long long* count, void* stream) {
    SRBH_REQUIRE(src && strides && stats && count, "srbh_band_stats: null pointer");
    SRBH_REQUIRE(type == SRBH_GRID_F32 || type == SRBH_GRID_U16 || type == SRBH_GRID_I16, "srbh_band_stats: unknown element type code %d", type);
    SRBH_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "srbh_band_stats: N, C, H, W must be positive (got %d, %d, %d, %d)", N, C, H, W);
    // every address the kernel forms is n * s_img + c * s_band + r * s_row + col with 0 <= n < N, c < C, r < H, col < W
    SRBH_REQUIRE(strides[0] >= 0 && strides[1] >= 0 && strides[2] >= 0, "srbh_band_stats: strides must not be negative");
    const long grid = (long)N * C;
    SRBH_REQUIRE(grid <= 0x7fffffffL, "srbh_band_stats: N * C = %ld workgroups are beyond the launch limit", grid);
    const int esz = type == SRBH_GRID_F32 ? 4 : 2, V = 16 / esz;
    BandParams p;
    p.src = src; p.s_img = strides[0]; p.s_band = strides[1]; p.s_row = strides[2];
    p.C = C; p.H = H; p.W = W;
    p.flat = (p.s_row == W || H == 1) ? 1 : 0;
    // a group of V values is one aligned 16-byte load when every band starts on a 16-byte boundary and either the band is one contiguous
    // run or every row starts on such a boundary and holds whole groups only
    p.vec = ((uintptr_t)src % 16 == 0 && p.s_img % V == 0 && p.s_band % V == 0 && (p.flat || (p.s_row % V == 0 && W % V == 0))) ? 1 : 0;
    // "equal to nodata" is a comparison of exact values: a nodata value the element type cannot hold equals no pixel
    p.has_nodata = 0;
    p.nodata_bits = 0;
    if (nodata) {
        const double nd = *nodata;
        if (type == SRBH_GRID_F32) {
            const float f = (float)nd;
            if ((double)f == nd) { p.has_nodata = 1; memcpy(&p.nodata_bits, &f, sizeof f); }
        } else {
            const double lo_v = type == SRBH_GRID_U16 ? 0.0 : -32768.0, hi_v = type == SRBH_GRID_U16 ? 65535.0 : 32767.0;
            if (nd >= lo_v && nd <= hi_v && (double)(int)nd == nd) { p.has_nodata = 1; p.nodata_bits = (int)nd; }
        }
    }
    p.stats = stats; p.count = count;
    hipStream_t st = (hipStream_t)stream;
    const bool small = (long)H * W <= BS_SMALL;
    if (type == SRBH_GRID_F32) band_launch<SRBH_GRID_F32>(small, grid, st, p);
    else if (type == SRBH_GRID_U16) band_launch<SRBH_GRID_U16>(small, grid, st, p);
    else band_launch<SRBH_GRID_I16>(small, grid, st, p);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" size_t srbh_label_hist_ws_bytes(int N, long HW) {
    if (N <= 0 || HW <= 0) return 0;
    const long nwg = (long)N * lh_slots(HW);
    if (nwg > 0x7fffffffL) return 0;
    return (size_t)nwg * 256 * sizeof(unsigned);
}

extern "C" int srbh_label_hist(const unsigned char* labels, long image_stride, int N, long HW, long long* hist, void* ws, void* stream) {
    SRBH_REQUIRE(labels && hist && ws, "srbh_label_hist: null pointer");
    SRBH_REQUIRE(N > 0 && HW > 0, "srbh_label_hist: N and HW must be positive (got %d, %ld)", N, HW);
    SRBH_REQUIRE(image_stride >= 0, "srbh_label_hist: the image stride must not be negative");
    const long slots = lh_slots(HW), nwg = (long)N * slots;
    SRBH_REQUIRE(nwg <= 0x7fffffffL, "srbh_label_hist: %ld workgroups are beyond the launch limit", nwg);
    const int vec = ((uintptr_t)labels % 16 == 0 && image_stride % 16 == 0) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(label_hist_kernel, dim3((unsigned)nwg), dim3(256), 0, st, labels, image_stride, HW, slots, vec, (unsigned*)ws);
    SRBH_HIP(hipGetLastError());
    hipLaunchKernelGGL(label_hist_fold_kernel, dim3(LH_FOLD_BLOCKS), dim3(256), 0, st, (const unsigned*)ws, nwg, hist);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
