// srbh_zone_compare.hip -- a predicted city against a reference height raster PER POLYGON ZONE: the paper reports per urban centre, and
// its table of 301 centres (datasetglobe/urbanarea_meanstd.xls) is what a predicted city is held against.  srbh_zones.hip gives a zone's
// own sums, srbh_compare.hip the pair sums of rectangular windows; here the zone's bits are applied to the pair selection, so one call
// gives [count, n, sd, sad, sdd, sp, sr, spp, srr, spr] of every zone.
//
// The rule is the conjunction of the two, each unchanged (include/srbh.h states both in full): a pixel enters the nine sums when it is IN
// THE ZONE (srbh_zones.hip: int32 fixed point with 8 fractional bits, even-odd over all edges, the pixel's centre decides, left / top
// boundaries in) and COMPARED (srbh_compare.hip: inside the raster, the pair test of `mode` on p > pthr and r > rthr, and no m or
// m > mthr).  count is the zone's pixels inside the raster: no test of the comparison applies to it.  d = p - r, signed.
//
// One workgroup of 256 lanes per item, on zone_item_kernel's walk (zone_item_walk, srbh_zone_bitmap.h: the bitmap is zeroed, the edges
// toggle it, the suffix XOR turns toggles into the in-zone mask, and walk_rect walks the batch) with p as raster a and r as raster b.
// The walk recovers a group's raster row ONCE from its row pointer (the exact division by p's row stride); it serves both the bitmap row
// and m's row.  A group with no pixel in the zone loads nothing; the pair test is srbh_pair_pieces.h's pair_test with the zone's bits in
// the place of the rectangle's, so m (third_test) is fetched only where a pixel of the zone passed it.  The partials are
// pair_sums_kernel's: 32-bit within a group, 64-bit across groups.  Ten int64 per item go to ws, zone_fold_kernel adds each zone's items
// in item order.  Integers only, no global atomics, no host synchronisation: exact and bit-equal between runs, however the items are cut.
//
// Overflow: as for srbh_pair_sums.  H W < 2^31 and a zone's items do not overlap, so a zone holds fewer than 2^31 pixels; every value is
// below 2^16: count, n < 2^31; sp, sr, sad, |sd| <= 65535 (2^31 - 1) < 2^47; spp, srr, spr, sdd <= 65535^2 (2^31 - 1) < 2^63.
//
// Memory safety.  The rasters p and r, the bitmap and the item and edge tables are read by zone_item_walk alone: its argument
// (srbh_zone_bitmap.h), which rests on srbh_raster_walk.h's, carries over untouched.  m is loaded by load_group under the same predicates
// (the same columns, [lo, hi) inside [0, W)) from the row y that the walk hands over, y in [0, H), through m's own stride, which the
// host checks to be >= W: srbh_compare.hip's argument.  The items of a zone are read through zone_items' checked range.  So no content
// of the tables leads outside them, the rasters' rows, ws or out; hostile tables give wrong sums at worst.  Stores: ten words to slot
// blockIdx of ws, ten words to row zone < Z of out.
#include "srbh_pair_pieces.h"
#include "srbh_zone_bitmap.h"

namespace {
using namespace srbh;

struct ZPAcc {
    int cnt;
    PAcc a;
    __device__ __forceinline__ ZPAcc down(int o) const { return {__shfl_down(cnt, o, 64), a.down(o)}; }
    __device__ __forceinline__ void merge(const ZPAcc& o) { cnt += o.cnt; a.merge(o.a); }
};

// One item: {count, n, sd, sad, sdd, sp, sr, spp, srr, spr} to ws int64 [NI][10].  EP, ER, EM: element sizes of p, r and m in bytes
// (EM == 0: no third raster)
template <int EP, int ER, int EM>
__global__ __launch_bounds__(256) void zone_pair_kernel(const PairParams q, const ZoneTables z, long long* __restrict__ ws) {
    using G = Group<EP, ER>;
    __shared__ unsigned bm[BM_WORDS + 1];
    const long item = blockIdx.x;                                     // < NI
    ZPAcc acc = {};
    zone_item_walk<EP, ER>(q.r, z, item, bm, [&](const G& g, long y, unsigned zb) {
        acc.cnt += __popc(zb);
        // the zone's bits in the place of the rectangle's: m is fetched only where a pixel of the zone passed the pair test
        unsigned wp[G::WORDS_A], wr[G::WORDS_B];
        g.load_a(wp);
        g.load_b(wr);
        unsigned sel = pair_test<EP, ER>(q, wp, wr) & zb;
        if (!sel) return;
        if (EM) {
            constexpr int EMM = EM ? EM : 1;
            unsigned wm[G::P * EMM / 4];
            sel &= third_test<EMM>(q, g, y, wm);
            if (!sel) return;
        }
        // pair_sums_kernel's loop (why it is no function of srbh_pair_pieces.h is said there, at PAcc)
        PAcc& a = acc.a;
        unsigned sp32 = 0, sr32 = 0, sad32 = 0;                       // at most 16 values below 2^16
        int sd32 = 0;
#pragma unroll
        for (int j = 0; j < G::P; ++j) {
            const bool on = (sel >> j) & 1u;
            const unsigned pv = on ? group_pixel<EP>(wp, j) : 0u, rv = on ? group_pixel<ER>(wr, j) : 0u;
            const int d = (int)pv - (int)rv;
            const unsigned ad = (unsigned)(d < 0 ? -d : d);
            sp32 += pv;
            sr32 += rv;
            sd32 += d;
            sad32 += ad;
            a.sdd += (unsigned long long)ad * ad;                     // 32 x 32 -> 64
            a.spp += (unsigned long long)pv * pv;
            a.srr += (unsigned long long)rv * rv;
            a.spr += (unsigned long long)pv * rv;
        }
        a.n += __popc(sel);
        a.sd += sd32;
        a.sad += sad32;
        a.sp += sp32;
        a.sr += sr32;
    });
    fold_team<256>(acc);
    if (threadIdx.x == 0) acc.a.store(ws + 10 * item, acc.cnt);
}

}  // namespace

extern "C" size_t srbh_zone_pair_ws_bytes(int NI) { return NI > 0 ? (size_t)NI * 10 * sizeof(long long) : 0; }

extern "C" int srbh_zone_pair_sums(const void* p, int typeP, long row_strideP, const void* r, int typeR, long row_strideR, const void* m,
                                   int typeM, long row_strideM, int H, int W, const int* edges, const int* edge_off, int Z, int E,
                                   const int* items, const int* item_off, int NI, int mode, int pthr, int rthr, int mthr, long long* out,
                                   void* ws, void* stream) {
    const char* who = "srbh_zone_pair_sums";
    SRBH_REQUIRE(out && ws, "%s: null pointer", who);
    SRBH_REQUIRE((m != nullptr) == (typeM != 0), "%s: m and typeM=%d must be given together (typeM 0: no third raster)", who, typeM);
    PairParams q;
    int rc = pair_params(who, p, typeP, row_strideP, r, typeR, row_strideR, m, typeM, row_strideM, H, W, mode, pthr, rthr, mthr, &q);
    if (rc != SRBH_OK) return rc;
    ZoneTables z;
    rc = zone_tables(who, edges, edge_off, Z, E, items, item_off, NI, (unsigned long long)row_strideP * (unsigned)raster_esz(typeP), &z);
    if (rc != SRBH_OK) return rc;
    SRBH_REQUIRE((uintptr_t)ws % 8 == 0 && (uintptr_t)out % 8 == 0, "%s: out and ws must be aligned to 8 bytes", who);
    hipStream_t st = (hipStream_t)stream;
    with_pair_sizes(typeP, typeR, m, typeM, [&](auto ep, auto er, auto em) {
        hipLaunchKernelGGL((zone_pair_kernel<decltype(ep)::value, decltype(er)::value, decltype(em)::value>), dim3((unsigned)NI), dim3(256), 0, st,
                           q, z, (long long*)ws);
    });
    SRBH_HIP(hipGetLastError());
    hipLaunchKernelGGL((zone_fold_kernel<10, -1>), dim3((unsigned)((Z + 255L) / 256)), dim3(256), 0, st, z, (const long long*)ws, out);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
