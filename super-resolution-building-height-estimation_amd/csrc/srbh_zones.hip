// srbh_zones.hip -- polygon zones over a city's rasters: the reference's "mean and std of building height in each urban center"
// (datasetglobe/urbanarea_meanstd.xls, README "Testing on 301 urban centers") is one gdal.RasterizeLayer into a scratch raster, one window
// read and one numpy.ma sum per feature (zonal_stats, demo_preprocess_height_v2.py:450-570).  Here the zones are rasterised on the device,
// row by row into an LDS bitmap that is never stored, and summed under the selection rule of srbh_summary.hip in exact integers.
//
// The rule (include/srbh.h states it in full).  Vertices are int32 fixed point with 8 fractional bits in raster pixel coordinates, a zone
// is the set of its non-horizontal edges (X0, Y0, X1, Y1).  With cy = 256 y + 128 and cx = 256 x + 128 an edge CROSSES row y when
// min(Y0, Y1) <= cy < max(Y0, Y1); pixel (x, y) is in the zone iff the number of crossing edges whose abscissa xc on the scanline is
// > cx is odd.  Oriented so that den = Y1 - Y0 > 0, a crossing toggles exactly the pixels x < t,
//   t = ceil((N - 128 den) / (256 den)) = floor((N + 128 den - 1) / (256 den)),   N = X0 den + (cy - Y0)(X1 - X0).
// |X|, |Y| <= 2^29: den and |X1 - X0| stay <= 2^30, |N| <= 2^59 + 2^60, everything fits int64.  No floating point touches the rule.
//
// Work is a list of ITEMS (zone, xoff, yoff, xcount, ycount): horizontal bands of a zone's bounding box, one workgroup of 256 lanes each.
// A band is done in batches of rows x segments of columns that fit the bitmap (BM_WORDS words; a row of a segment is wpr <= 256 words):
//   1. the lanes take the zone's edges in turn (one 16-byte load each); an edge walks the batch's rows it crosses -- t of its first row by
//      one 64-bit floor division, then quotient and remainder stepped row by row, exactly -- and toggles bit min(t, xe) - 1 - xs of the row
//      by an LDS XOR atomic (t <= xs toggles no pixel of the segment, t >= xe all of them);
//   2. an inclusive suffix XOR along each row turns the toggles into the in-zone mask: within a word by shifts, across words by the parity
//      of the popcounts to the right (a ballot per 64 words);
//   3. walk_rect walks the batch; a group's row is recovered from its row pointer (an exact division by the row stride: a multiplication
//      by the stride's inverse modulo 2^64), the zone's bits of its P columns are ANDed into the selection.  A group with no pixel in the
//      zone loads nothing.
// The three steps are zone_item_walk's (srbh_zone_bitmap.h), which srbh_zone_compare.hip walks too; the kernel here keeps what it does
// with a group that has a pixel in the zone.  Loads of the rasters are walk_rect's: the memory-safety argument of srbh_raster_walk.h
// carries over untouched; that of the bitmap and the tables is stated once, at zone_item_walk.  No global atomics, no host
// synchronisation; per-item partials go to ws and a second kernel adds each zone's items in item order.
#include "srbh_summary_select.h"
#include "srbh_zone_bitmap.h"

namespace {
using namespace srbh;

struct ZAcc {
    int cnt;
    Acc a;
    __device__ __forceinline__ ZAcc down(int o) const { return {__shfl_down(cnt, o, 64), a.down(o)}; }
    __device__ __forceinline__ void merge(const ZAcc& o) { cnt += o.cnt; a.merge(o.a); }
};

// One item.  HIST == false: {count, n, sum, sumsq, max} to ws int64 [NI][5]; HIST == true: the item's histogram to ws uint32 [NI][nbins].
template <int EV, int EM, bool HIST>
__global__ __launch_bounds__(256) void zone_item_kernel(const SumParams p, const ZoneTables z, unsigned magic, int nbins, void* __restrict__ ws) {
    using G = Group<EV, EM>;
    __shared__ unsigned bm[BM_WORDS + 1];
    __shared__ unsigned hist[HIST ? VH_MAX_BINS : 1];
    const int t = threadIdx.x;
    const long item = blockIdx.x;                                     // < NI
    if (HIST) {
        for (int i = t; i < nbins; i += 256) hist[i] = 0u;            // (a barrier follows before any lane counts: the walk's, or the one below)
    }
    ZAcc acc = {0, {0, 0u, 0ull, 0ull}};
    const unsigned last = (unsigned)nbins - 1u;
    zone_item_walk<EV, EM>(p.r, z, item, bm, [&](const G& g, long, unsigned zb) {
        unsigned wv[G::WORDS_A];
        const unsigned sel = select_group(p, g, wv) & zb;
        if (HIST) {
#pragma unroll
            for (int j = 0; j < G::P; ++j) {
                if ((sel >> j) & 1u) {
                    const unsigned v = group_pixel<EV>(wv, j), qv = magic ? __umulhi(v, magic) : v;
                    atomicAdd(&hist[qv < last ? qv : last], 1u);
                }
            }
        } else {
            acc.cnt += __popc(zb);
            add_group<EV>(acc.a, sel, wv);
        }
    });
    if (HIST) {
        __syncthreads();
        unsigned* o = (unsigned*)ws + item * nbins;
        for (int i = t; i < nbins; i += 256) o[i] = hist[i];
    } else {
        fold_team<256>(acc);
        if (t == 0) {
            long long* o = (long long*)ws + 5 * item;
            o[0] = acc.cnt;
            o[1] = acc.a.n;
            o[2] = (long long)acc.a.sum;
            o[3] = (long long)acc.a.sq;
            o[4] = acc.a.mx;
        }
    }
}

// block (zone, 256 bins): a lane per bin
__global__ __launch_bounds__(256) void zone_hist_fold_kernel(const ZoneTables z, int nbins, const unsigned* __restrict__ ws, long long* __restrict__ hist) {
    const int zone = blockIdx.x, bin = blockIdx.y * 256 + threadIdx.x;
    if (bin >= nbins) return;
    int i0, i1;
    zone_items(z, zone, &i0, &i1);
    long long s = 0;
    for (int i = i0; i < i1; ++i) s += ws[(long)i * nbins + bin];
    hist[(long)zone * nbins + bin] = s;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
template <bool HIST>
int zone_launch(const char* who, const void* v, int typeV, long rsV, const void* m, int typeM, long rsM, int H, int W, const int* edges,
                const int* edge_off, int Z, int E, const int* items, const int* item_off, int NI, int vthr, int mthr, int bin_width, int nbins,
                long long* out, void* ws, void* stream) {
    SRBH_REQUIRE(out && ws, "%s: null pointer", who);
    if (HIST) {
        SRBH_REQUIRE(bin_width >= 1 && bin_width <= 65535, "%s: bin_width=%d outside 1..65535", who, bin_width);
        SRBH_REQUIRE(nbins >= 1 && nbins <= VH_MAX_BINS, "%s: nbins=%d outside 1..%d", who, nbins, VH_MAX_BINS);
    }
    SumParams p;
    int rc = sum_params(who, v, typeV, rsV, m, typeM, rsM, H, W, vthr, mthr, &p);
    if (rc != SRBH_OK) return rc;
    ZoneTables z;
    rc = zone_tables(who, edges, edge_off, Z, E, items, item_off, NI, (unsigned long long)rsV * (unsigned)raster_esz(typeV), &z);
    if (rc != SRBH_OK) return rc;
    SRBH_REQUIRE((uintptr_t)ws % 8 == 0 && (uintptr_t)out % 8 == 0, "%s: out and ws must be aligned to 8 bytes", who);
    const unsigned magic = HIST ? vh_magic(bin_width) : 0u;
    hipStream_t st = (hipStream_t)stream;
    with_sizes(typeV, m, typeM, [&](auto ev, auto em) {
        hipLaunchKernelGGL((zone_item_kernel<decltype(ev)::value, decltype(em)::value, HIST>), dim3((unsigned)NI), dim3(256), 0, st, p, z, magic,
                           HIST ? nbins : 1, ws);
    });
    SRBH_HIP(hipGetLastError());
    if (HIST)
        hipLaunchKernelGGL(zone_hist_fold_kernel, dim3((unsigned)Z, (unsigned)((nbins + 255) / 256)), dim3(256), 0, st, z, nbins, (const unsigned*)ws, out);
    else
        hipLaunchKernelGGL((zone_fold_kernel<5, 4>), dim3((unsigned)((Z + 255L) / 256)), dim3(256), 0, st, z, (const long long*)ws, out);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

}  // namespace

extern "C" size_t srbh_zone_sums_ws_bytes(int NI) { return NI > 0 ? (size_t)NI * 5 * sizeof(long long) : 0; }

extern "C" size_t srbh_zone_hist_ws_bytes(int NI, int nbins) {
    return NI > 0 && nbins >= 1 && nbins <= VH_MAX_BINS ? (size_t)NI * nbins * sizeof(unsigned) : 0;
}

extern "C" int srbh_zone_sums(const void* v, int typeV, long row_strideV, const void* m, int typeM, long row_strideM, int H, int W,
                              const int* edges, const int* edge_off, int Z, int E, const int* items, const int* item_off, int NI, int vthr,
                              int mthr, long long* out, void* ws, void* stream) {
    return zone_launch<false>("srbh_zone_sums", v, typeV, row_strideV, m, typeM, row_strideM, H, W, edges, edge_off, Z, E, items, item_off, NI,
                              vthr, mthr, 1, 1, out, ws, stream);
}

extern "C" int srbh_zone_hist(const void* v, int typeV, long row_strideV, const void* m, int typeM, long row_strideM, int H, int W,
                              const int* edges, const int* edge_off, int Z, int E, const int* items, const int* item_off, int NI, int vthr,
                              int mthr, int bin_width, int nbins, long long* hist, void* ws, void* stream) {
    return zone_launch<true>("srbh_zone_hist", v, typeV, row_strideV, m, typeM, row_strideM, H, W, edges, edge_off, Z, E, items, item_off, NI,
                             vthr, mthr, bin_width, nbins, hist, ws, stream);
}
