// srbh_summary.hip -- the step behind a city's predicted rasters: the reference publishes "the mean and std of building height in each
// urban center" and the distribution of predicted heights (README "Testing on 301 urban centers"), gathered one shapefile feature and one
// GDAL window read at a time (demo_preprocess_height_v2.py: Fishgrid_stats :1143-1186, zonal_stats :450-570).  Here: exact integer sums
// of a value raster under a mask raster, per window, per non-overlapping block and as a binned histogram.
//
// A pixel is SELECTED when it lies inside the raster, v > vthr and (no mask or m > mthr).  v and m are uint16 or uint8 rasters, each read
// in place through its own row stride.  Everything is an integer: exact, no order, bit-equal between runs.  No floating point.
//
// One walk serves the three entries.  A rectangle [x0, x1) x [y0, y0 + rows) inside the raster is cut, row by row, into groups of
// P = 16 / sizeof(element of v) pixels that start on 16-byte boundaries of v's ADDRESS (the alignment is taken per row: an odd W, a
// cropped view and xoff = k * 56 give every row its own); a TEAM of lanes takes the (row, group) pairs in turn.  As in srbh_cells.hip:
//   * a group whose P pixels all lie inside the raster's row [0, W) is fetched by one aligned 16-byte load, and the pixels outside
//     [x0, x1) are masked off -- the head and the tail of a rectangle's row read raster pixels next to it, never anything else;
//   * any other group is fetched pixel by pixel, each load predicated on the rectangle, which lies inside the raster.
// The same P pixels of m are fetched by the same rule with a load of element alignment (m has its own element size, stride and
// alignment).  So no load touches a byte outside the rows' own bytes of either raster, whatever pos holds.
//
//   srbh_window_sums   TEAM = one workgroup of 256 lanes per window (windows overlap and have any size): {count, n, sum, sumsq, max}.
//   srbh_block_sums    every block x block cell of the raster has ONE owner, so nothing is added across owners and the raster is read
//                      once: a lane owns a block of side <= 8, a wave one of side <= 64, a workgroup a larger one.
//   srbh_value_hist    a fixed grid of workgroups strides over the whole raster; a workgroup counts into its own LDS histogram (32-bit:
//                      H * W < 2^31), stores it to its slot of the workspace, and a second kernel adds the slots into int64 in slot order.
//
// The source holds no floating-point operation; the only ones in the ISA are the compiler's own reciprocal sequence for the integer
// divisions of indices (tid / cpr, b / Wb), whose result is the exact quotient -- as in cell_counts_kernel.
//
// Overflow.  A group holds at most 16 values below 2^16: its sum stays below 2^20 and is formed in 32 bits; everything a lane keeps
// across groups is 64-bit.  v * v reaches (2^16 - 1)^2 < 2^32: the product is a 32 x 32 -> 64-bit multiply-add (one v_mad_u64_u32), so
// the sum of squares is 64-bit from the first add; H * W < 2^31 keeps it below 2^31 * 2^32 = 2^63.  Counts: int32, below H * W.
#include "srbh_internal.h"

namespace {
using namespace srbh;

struct SumParams {
    const unsigned char* v;
    const unsigned char* m;         // NULL: no mask
    long rsV, rsM;                  // row strides in elements
    int H, W;
    int vthr, mthr;
};

struct Acc {
    int n;
    unsigned mx;
    unsigned long long sum, sq;
};

// val[j] = pixel c0 + j of the row at `row` (its pixel 0) for every j of [lo, hi), a non-empty part of [0, P) whose pixels lie inside
// [0, W); the other entries hold raster pixels of the same row or 0.  ALIGNED: row + c0 * E is a 16-byte boundary whenever the wide
// load is taken (P * E == 16).
template <int E, int P, bool ALIGNED>
__device__ __forceinline__ void group_vals(const unsigned char* row, int c0, int W, int lo, int hi, unsigned* val) {
    constexpr int WORDS = P * E / 4;
    if (c0 >= 0 && c0 <= W - P) {
        unsigned w[WORDS];
        const unsigned char* src = row + (long)c0 * E;
        if (ALIGNED) {
            const uint4 q = *reinterpret_cast<const uint4*>(src);
            w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else {
            __builtin_memcpy(w, __builtin_assume_aligned(src, E), sizeof w);
        }
#pragma unroll
        for (int j = 0; j < P; ++j) val[j] = E == 1 ? (w[j >> 2] >> (8 * (j & 3))) & 0xffu : (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
    } else {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            val[j] = 0u;
            if (j >= lo && j < hi) val[j] = E == 1 ? (unsigned)row[c0 + j] : (unsigned)reinterpret_cast<const unsigned short*>(row)[c0 + j];
        }
    }
}

// The rectangle [x0, x1) x [y0, y0 + rows) -- inside the raster, not empty -- walked by `team` lanes, this one being lane `tid` of them:
// f(val, sel) once per (row, group) of this lane, val the P values of v, bit j of sel: pixel j of the group is selected.
template <int EV, int EM, class F>
__device__ __forceinline__ void walk(const SumParams& p, int x0, int x1, int y0, int rows, int tid, int team, F&& f) {
    constexpr int P = 16 / EV;
    // a row's groups: group k holds the pixels x0 - mis + k * P .. + P - 1, mis < P the pixels between the 16-byte boundary below the
    // row's first pixel and that pixel; at most cpr groups reach into [x0, x1)
    const int cpr = (int)(((long)(x1 - x0) + 2 * P - 2) / P);
    const int drow = team / cpr, dk = team - drow * cpr;             // (32-bit index divisions: team <= 2048 * 256)
    long row = tid / cpr;
    int k = tid - (int)row * cpr;
    while (row < rows) {
        const long y = y0 + row;
        const unsigned char* rowV = p.v + y * p.rsV * EV;
        const int mis = (int)(((uintptr_t)rowV + (uintptr_t)x0 * EV) & 15u) / EV;
        const long c0l = (long)x0 - mis + (long)k * P;
        if (c0l < x1) {
            const int c0 = (int)c0l;
            const int lo = x0 > c0 ? x0 - c0 : 0, hi = x1 - c0 < P ? x1 - c0 : P;      // the rectangle's pixels of this group: hi > lo
            unsigned val[P];
            group_vals<EV, P, true>(rowV, c0, p.W, lo, hi, val);
            unsigned sel = 0;
#pragma unroll
            for (int j = 0; j < P; ++j) sel |= ((int)val[j] > p.vthr ? 1u : 0u) << j;
            sel &= ((1u << (hi - lo)) - 1u) << lo;
            if (EM) {
                constexpr int EMM = EM ? EM : 1;
                unsigned mv[P];
                group_vals<EMM, P, false>(p.m + y * p.rsM * EMM, c0, p.W, lo, hi, mv);
                unsigned ms = 0;
#pragma unroll
                for (int j = 0; j < P; ++j) ms |= ((int)mv[j] > p.mthr ? 1u : 0u) << j;
                sel &= ms;
            }
            f(val, sel);
        }
        row += drow;
        k += dk;
        if (k >= cpr) { k -= cpr; ++row; }
    }
}

template <int P>
__device__ __forceinline__ void add_group(Acc& a, const unsigned* val, unsigned sel) {
    unsigned s32 = 0;                                                 // at most 16 values below 2^16
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const unsigned s = (sel >> j) & 1u ? val[j] : 0u;
        s32 += s;
        a.sq += (unsigned long long)s * s;                            // 32 x 32 -> 64
        a.mx = a.mx > s ? a.mx : s;
    }
    a.n += __popc(sel);
    a.sum += s32;
}

// the team's lanes folded into its lane 0.  TEAM: 1 (a lane), 64 (a wave), 256 (the workgroup; every lane of it calls)
template <int TEAM>
__device__ __forceinline__ void fold(Acc& a) {
    if (TEAM == 1) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a.n += __shfl_down(a.n, o, 64);
        a.sum += __shfl_down(a.sum, o, 64);
        a.sq += __shfl_down(a.sq, o, 64);
        const unsigned other = __shfl_down(a.mx, o, 64);
        a.mx = a.mx > other ? a.mx : other;
    }
    if (TEAM == 256) {
        __shared__ unsigned long long red[2][4];
        __shared__ int red_n[4];
        __shared__ unsigned red_mx[4];
        const int t = threadIdx.x, wave = t >> 6;
        if ((t & 63) == 0) { red[0][wave] = a.sum; red[1][wave] = a.sq; red_n[wave] = a.n; red_mx[wave] = a.mx; }
        __syncthreads();
        if (t == 0) {
            a.sum = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
            a.sq = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
            a.n = ((red_n[0] + red_n[1]) + red_n[2]) + red_n[3];
#pragma unroll
            for (int w = 1; w < 4; ++w) a.mx = a.mx > red_mx[w] ? a.mx : red_mx[w];
        }
    }
}

// EV, EM: element sizes of v and m in bytes (EM == 0: no mask)
template <int EV, int EM>
__global__ __launch_bounds__(256) void window_sums_kernel(const SumParams p, const int* __restrict__ pos, long long* __restrict__ out) {
    const int* q = pos + 4 * (long)blockIdx.x;
    const int xoff = q[0], yoff = q[1], xcount = q[2], ycount = q[3];
    // the window clipped to the raster, in 64 bits so that no content of pos overflows
    const long long X0 = xoff > 0 ? xoff : 0, Y0 = yoff > 0 ? yoff : 0;
    long long X1 = (long long)xoff + xcount, Y1 = (long long)yoff + ycount;
    X1 = X1 < p.W ? X1 : p.W;
    Y1 = Y1 < p.H ? Y1 : p.H;
    const bool any = xcount > 0 && ycount > 0 && X1 > X0 && Y1 > Y0;
    const int x0 = any ? (int)X0 : 0, x1 = any ? (int)X1 : 0, y0 = any ? (int)Y0 : 0, rows = any ? (int)(Y1 - Y0) : 0;
    Acc a = {0, 0u, 0ull, 0ull};
    if (any)                                                          // uniform
        walk<EV, EM>(p, x0, x1, y0, rows, threadIdx.x, 256, [&](const unsigned* val, unsigned sel) { add_group<16 / EV>(a, val, sel); });
    fold<256>(a);
    if (threadIdx.x == 0) {
        long long* o = out + 5 * (long)blockIdx.x;
        o[0] = (long long)(x1 - x0) * rows;
        o[1] = a.n;
        o[2] = (long long)a.sum;
        o[3] = (long long)a.sq;
        o[4] = a.mx;
    }
}

// TEAM lanes own block b = by * Wb + bx: 256 blocks per workgroup (TEAM 1), four (TEAM 64) or one (TEAM 256)
template <int EV, int EM, int TEAM>
__global__ __launch_bounds__(256) void block_sums_kernel(const SumParams p, int block, int Hb, int Wb, long long* __restrict__ out) {
    const long nb = (long)Hb * Wb;
    const int t = threadIdx.x;
    const long b = TEAM == 1 ? blockIdx.x * 256L + t : TEAM == 64 ? blockIdx.x * 4L + (t >> 6) : (long)blockIdx.x;
    const int tid = TEAM == 1 ? 0 : TEAM == 64 ? (t & 63) : t;
    Acc a = {0, 0u, 0ull, 0ull};
    if (b < nb) {                                                     // the same in every lane of a team
        const int by = (int)((unsigned)b / (unsigned)Wb), bx = (int)b - by * Wb;      // b < Hb * Wb < 2^31
        const int x0 = bx * block, y0 = by * block;                  // below W and H
        const long long X1 = (long long)x0 + block, Y1 = (long long)y0 + block;
        const int x1 = X1 < p.W ? (int)X1 : p.W, y1 = Y1 < p.H ? (int)Y1 : p.H;
        walk<EV, EM>(p, x0, x1, y0, y1 - y0, tid, TEAM, [&](const unsigned* val, unsigned sel) { add_group<16 / EV>(a, val, sel); });
    }
    fold<TEAM>(a);
    if (b < nb && tid == 0) {
        out[b] = a.n;
        out[nb + b] = (long long)a.sum;
        out[2 * nb + b] = (long long)a.sq;
        out[3 * nb + b] = a.mx;
    }
}

// ---- histogram ----------------------------------------------------------------------------------------------------------------------------
constexpr int VH_MAX_BINS = 4096;
constexpr int VH_MAX_WGS = 2048;
constexpr int VH_GROUPS_PER_LANE = 8;                  // a workgroup is worth launching for 256 * 8 groups of 16 bytes

// v / d for 0 <= v < 2^16, 2 <= d < 2^16 is (v * M) >> 32 with M = floor(2^32 / d) + 1: M d = 2^32 + e with 0 < e <= d, so
// v M / 2^32 = v / d + v e / (d 2^32), and v e <= (2^16 - 1)^2 < 2^32 adds less than 1 / d: the floor does not move.  d == 1 would need
// M = 2^32 + 1, which 32 bits do not hold: magic 0 stands for it, and the quotient is v.
inline unsigned vh_magic(int d) { return d >= 2 && d <= 65535 ? (unsigned)(0x100000000ull / (unsigned)d) + 1u : 0u; }
inline long vh_wgs(int H, int W) {
    const long groups = (long)H * (((long)W + 14) / 8 + 1);           // not below the (row, group) pairs of either element size
    const long wgs = (groups + 256L * VH_GROUPS_PER_LANE - 1) / (256L * VH_GROUPS_PER_LANE);
    return wgs < VH_MAX_WGS ? wgs : VH_MAX_WGS;
}

template <int EV, int EM>
__global__ __launch_bounds__(256) void value_hist_kernel(const SumParams p, unsigned magic, int nbins, unsigned* __restrict__ ws) {
    __shared__ unsigned hist[VH_MAX_BINS];
    const int t = threadIdx.x;
    for (int i = t; i < nbins; i += 256) hist[i] = 0u;
    __syncthreads();
    const unsigned last = (unsigned)nbins - 1u;
    walk<EV, EM>(p, 0, p.W, 0, p.H, (int)blockIdx.x * 256 + t, (int)gridDim.x * 256, [&](const unsigned* val, unsigned sel) {
#pragma unroll
        for (int j = 0; j < 16 / EV; ++j) {
            if ((sel >> j) & 1u) {
                const unsigned qv = magic ? __umulhi(val[j], magic) : val[j];
                atomicAdd(&hist[qv < last ? qv : last], 1u);
            }
        }
    });
    __syncthreads();
    for (int i = t; i < nbins; i += 256) ws[(long)blockIdx.x * nbins + i] = hist[i];
}

// block b owns the bins 16 b .. 16 b + 15; thread t adds the slots (t >> 4), (t >> 4) + 16, ... of bin 16 b + (t & 15), then the 16 partial
// counts of a bin are added through LDS in a fixed order
__global__ __launch_bounds__(256) void value_hist_fold_kernel(const unsigned* __restrict__ ws, int nwg, int nbins, long long* __restrict__ hist) {
    __shared__ long long part[16][16];
    const int t = threadIdx.x, bin = blockIdx.x * 16 + (t & 15), grp = t >> 4;
    long long a = 0;
    if (bin < nbins) {
#pragma unroll 4
        for (int k = grp; k < nwg; k += 16) a += ws[(long)k * nbins + bin];
    }
    part[grp][t & 15] = a;
    __syncthreads();
    if (t < 16 && bin < nbins) {
        long long s = 0;
#pragma unroll
        for (int g = 0; g < 16; ++g) s += part[g][t];
        hist[bin] = s;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
inline bool sum_type_ok(int type) { return type == SRBH_GRID_U16 || type == SRBH_GRID_U8; }
inline int sum_esz(int type) { return type == SRBH_GRID_U8 ? 1 : 2; }

// the checks common to the three entries; fills p.  SRBH_OK or SRBH_ERR_ARG (the error text is set)
int sum_params(const char* who, const void* v, int typeV, long rsV, const void* m, int typeM, long rsM, int H, int W, int vthr, int mthr,
               SumParams* p) {
    SRBH_REQUIRE(v, "%s: null value raster", who);
    SRBH_REQUIRE(sum_type_ok(typeV) && (!m || sum_type_ok(typeM)),
                 "%s: element type typeV=%d typeM=%d; the rasters are uint16 (1) or uint8 (3) -- int16, float32 and unknown codes are refused",
                 who, typeV, typeM);
    SRBH_REQUIRE(H > 0 && W > 0, "%s: bad geometry H=%d W=%d", who, H, W);
    SRBH_REQUIRE(rsV >= W && (!m || rsM >= W), "%s: a row stride (%ld, %ld) is below W=%d", who, rsV, m ? rsM : rsV, W);
    SRBH_REQUIRE((long)H * W < 0x80000000L, "%s: H * W = %ld must stay below 2^31", who, (long)H * W);
    SRBH_REQUIRE(vthr >= -1 && vthr <= 65535 && mthr >= -1 && mthr <= 65535, "%s: a threshold (vthr=%d, mthr=%d) outside -1..65535", who,
                 vthr, mthr);
    const int ev = sum_esz(typeV), em = m ? sum_esz(typeM) : 0;
    SRBH_REQUIRE((uintptr_t)v % ev == 0 && (!m || (uintptr_t)m % em == 0), "%s: a raster is not aligned to its element size", who);
    p->v = (const unsigned char*)v; p->m = (const unsigned char*)m;
    p->rsV = rsV; p->rsM = m ? rsM : 0;
    p->H = H; p->W = W; p->vthr = vthr; p->mthr = mthr;
    return SRBH_OK;
}

// f(integral_constant EV, integral_constant EM) for the element sizes of p's rasters
template <class F>
inline void with_sizes(int typeV, const void* m, int typeM, F&& f) {
    using std::integral_constant;
    const int ev = sum_esz(typeV), em = m ? sum_esz(typeM) : 0;
    if (ev == 1) {
        if (em == 0) f(integral_constant<int, 1>{}, integral_constant<int, 0>{});
        else if (em == 1) f(integral_constant<int, 1>{}, integral_constant<int, 1>{});
        else f(integral_constant<int, 1>{}, integral_constant<int, 2>{});
    } else {
        if (em == 0) f(integral_constant<int, 2>{}, integral_constant<int, 0>{});
        else if (em == 1) f(integral_constant<int, 2>{}, integral_constant<int, 1>{});
        else f(integral_constant<int, 2>{}, integral_constant<int, 2>{});
    }
}

}  // namespace

extern "C" int srbh_window_sums(const void* v, int typeV, long row_strideV, const void* m, int typeM, long row_strideM, int H, int W,
                                const int* pos, int N, int vthr, int mthr, long long* out, void* stream) {
    SRBH_REQUIRE(pos && out, "srbh_window_sums: null pointer");
    SRBH_REQUIRE(N > 0, "srbh_window_sums: N=%d must be positive", N);
    SumParams p;
    const int rc = sum_params("srbh_window_sums", v, typeV, row_strideV, m, typeM, row_strideM, H, W, vthr, mthr, &p);
    if (rc != SRBH_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    with_sizes(typeV, m, typeM, [&](auto ev, auto em) {
        hipLaunchKernelGGL((window_sums_kernel<decltype(ev)::value, decltype(em)::value>), dim3((unsigned)N), dim3(256), 0, st, p, pos, out);
    });
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_block_sums(const void* v, int typeV, long row_strideV, const void* m, int typeM, long row_strideM, int H, int W,
                               int block, int vthr, int mthr, long long* out, void* stream) {
    SRBH_REQUIRE(out, "srbh_block_sums: null pointer");
    SRBH_REQUIRE(block >= 1, "srbh_block_sums: block=%d must be at least 1", block);
    SumParams p;
    const int rc = sum_params("srbh_block_sums", v, typeV, row_strideV, m, typeM, row_strideM, H, W, vthr, mthr, &p);
    if (rc != SRBH_OK) return rc;
    const int side = H > W ? H : W, bl = block < side ? block : side;     // a block beyond the raster is the raster: one block either way
    const int Hb = (H + bl - 1) / bl, Wb = (W + bl - 1) / bl;
    const long nb = (long)Hb * Wb;                                        // <= H * W < 2^31
    hipStream_t st = (hipStream_t)stream;
    with_sizes(typeV, m, typeM, [&](auto ev, auto em) {
        if (bl <= 8)
            hipLaunchKernelGGL((block_sums_kernel<decltype(ev)::value, decltype(em)::value, 1>), dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, p, bl, Hb, Wb, out);
        else if (bl <= 64)
            hipLaunchKernelGGL((block_sums_kernel<decltype(ev)::value, decltype(em)::value, 64>), dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, st, p, bl, Hb, Wb, out);
        else
            hipLaunchKernelGGL((block_sums_kernel<decltype(ev)::value, decltype(em)::value, 256>), dim3((unsigned)nb), dim3(256), 0, st, p, bl, Hb, Wb, out);
    });
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" unsigned srbh_value_hist_magic(int bin_width) { return vh_magic(bin_width); }

extern "C" size_t srbh_value_hist_ws_bytes(int H, int W, int nbins) {
    if (H <= 0 || W <= 0 || nbins < 1 || nbins > VH_MAX_BINS || (long)H * W >= 0x80000000L) return 0;
    return (size_t)vh_wgs(H, W) * nbins * sizeof(unsigned);
}

extern "C" int srbh_value_hist(const void* v, int typeV, long row_strideV, const void* m, int typeM, long row_strideM, int H, int W,
                               int vthr, int mthr, int bin_width, int nbins, long long* hist, void* ws, void* stream) {
    SRBH_REQUIRE(hist && ws, "srbh_value_hist: null pointer");
    SRBH_REQUIRE(bin_width >= 1 && bin_width <= 65535, "srbh_value_hist: bin_width=%d outside 1..65535", bin_width);
    SRBH_REQUIRE(nbins >= 1 && nbins <= VH_MAX_BINS, "srbh_value_hist: nbins=%d outside 1..%d", nbins, VH_MAX_BINS);
    SumParams p;
    const int rc = sum_params("srbh_value_hist", v, typeV, row_strideV, m, typeM, row_strideM, H, W, vthr, mthr, &p);
    if (rc != SRBH_OK) return rc;
    const int nwg = (int)vh_wgs(H, W);
    const unsigned magic = vh_magic(bin_width);
    hipStream_t st = (hipStream_t)stream;
    with_sizes(typeV, m, typeM, [&](auto ev, auto em) {
        hipLaunchKernelGGL((value_hist_kernel<decltype(ev)::value, decltype(em)::value>), dim3((unsigned)nwg), dim3(256), 0, st, p, magic, nbins, (unsigned*)ws);
    });
    SRBH_HIP(hipGetLastError());
    hipLaunchKernelGGL(value_hist_fold_kernel, dim3((unsigned)((nbins + 15) / 16)), dim3(256), 0, st, (const unsigned*)ws, nwg, nbins, hist);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
