// srbh_summary.hip -- the step behind a city's predicted rasters: the reference publishes "the mean and std of building height in each
// urban center" and the distribution of predicted heights (README "Testing on 301 urban centers"), gathered one shapefile feature and one
// GDAL window read at a time (demo_preprocess_height_v2.py: Fishgrid_stats :1143-1186, zonal_stats :450-570).  Here: exact integer sums
// of a value raster under a mask raster, per window, per non-overlapping block and as a binned histogram.
//
// A pixel is SELECTED when it lies inside the raster, v > vthr and (no mask or m > mthr).  v and m are uint16 or uint8 rasters, each read
// in place through its own row stride.  Everything is an integer: exact, no order, bit-equal between runs.  No floating point.
//
// One walk serves the three entries (srbh_raster_walk.h: the walk in 16-byte groups of v's address by a TEAM of lanes, and why no load
// leaves a raster whatever pos holds):
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
#include "srbh_summary_select.h"

namespace {
using namespace srbh;

// the selected pixels of the rectangle [x0, x1) x [y0, y0 + rows) that lane `tid` of `team` walks, added to a
template <int EV, int EM>
__device__ __forceinline__ void sum_rect(const SumParams& p, int x0, int x1, int y0, int rows, int tid, int team, Acc& a) {
    using G = Group<EV, EM>;
    walk_rect<EV, EM>(p.r, x0, x1, y0, rows, tid, team, [&](const G& g) {
        unsigned wv[G::WORDS_A];
        const unsigned sel = select_group(p, g, wv);
        unsigned s32 = 0;                                             // at most 16 values below 2^16
#pragma unroll
        for (int j = 0; j < G::P; ++j) {
            const unsigned s = (sel >> j) & 1u ? group_pixel<EV>(wv, j) : 0u;
            s32 += s;
            a.sq += (unsigned long long)s * s;                        // 32 x 32 -> 64
            a.mx = a.mx > s ? a.mx : s;
        }
        a.n += __popc(sel);
        a.sum += s32;
    });
}

// EV, EM: element sizes of v and m in bytes (EM == 0: no mask)
template <int EV, int EM>
__global__ __launch_bounds__(256) void window_sums_kernel(const SumParams p, const int* __restrict__ pos, long long* __restrict__ out) {
    const Rect w = clip_window(pos + 4 * (long)blockIdx.x, p.r.H, p.r.W);
    Acc a = {0, 0u, 0ull, 0ull};
    if (w.any) sum_rect<EV, EM>(p, w.x0, w.x1, w.y0, w.rows, threadIdx.x, 256, a);      // uniform
    fold_team<256>(a);
    if (threadIdx.x == 0) {
        long long* o = out + 5 * (long)blockIdx.x;
        o[0] = (long long)(w.x1 - w.x0) * w.rows;
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
        const int x1 = X1 < p.r.W ? (int)X1 : p.r.W, y1 = Y1 < p.r.H ? (int)Y1 : p.r.H;
        sum_rect<EV, EM>(p, x0, x1, y0, y1 - y0, tid, TEAM, a);
    }
    fold_team<TEAM>(a);
    if (b < nb && tid == 0) {
        out[b] = a.n;
        out[nb + b] = (long long)a.sum;
        out[2 * nb + b] = (long long)a.sq;
        out[3 * nb + b] = a.mx;
    }
}

// ---- histogram ----------------------------------------------------------------------------------------------------------------------------
constexpr int VH_MAX_WGS = 2048;
constexpr int VH_GROUPS_PER_LANE = 8;                  // a workgroup is worth launching for 256 * 8 groups of 16 bytes

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
    walk_rect<EV, EM>(p.r, 0, p.r.W, 0, p.r.H, (int)blockIdx.x * 256 + t, (int)gridDim.x * 256, [&](const Group<EV, EM>& g) {
        unsigned wv[Group<EV, EM>::WORDS_A];
        const unsigned sel = select_group(p, g, wv);
#pragma unroll
        for (int j = 0; j < 16 / EV; ++j) {
            if ((sel >> j) & 1u) {
                const unsigned v = group_pixel<EV>(wv, j), qv = magic ? __umulhi(v, magic) : v;
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
