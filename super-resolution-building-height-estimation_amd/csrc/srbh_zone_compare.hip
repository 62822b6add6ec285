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
// One workgroup of 256 lanes per item, zone_item_kernel's batch and segment loop: the bitmap is zeroed, the edges toggle it, the suffix
// XOR turns toggles into the in-zone mask (srbh_zone_bitmap.h), and walk_rect walks the batch with p as raster a and r as raster b.  A
// group's raster row is recovered ONCE from its row pointer (the exact division by p's row stride) and serves both the bitmap row and
// m's row.  A group with no pixel in the zone loads nothing; m is fetched only where a pixel of the zone passed the pair test.  The
// partials are pair_sums_kernel's: 32-bit within a group, 64-bit across groups.  Ten int64 per item go to ws, a second kernel adds each
// zone's items in item order.  Integers only, no global atomics, no host synchronisation: exact and bit-equal between runs, however the
// items are cut.
//
// Overflow: as for srbh_pair_sums.  H W < 2^31 and a zone's items do not overlap, so a zone holds fewer than 2^31 pixels; every value is
// below 2^16: count, n < 2^31; sp, sr, sad, |sd| <= 65535 (2^31 - 1) < 2^47; spp, srr, spr, sdd <= 65535^2 (2^31 - 1) < 2^63.
//
// Memory safety.  The rasters p and r are loaded by walk_rect's groups only, over rectangles that clip_window has cut to the raster in 64
// bits whatever an item holds: srbh_raster_walk.h's argument carries over untouched.  m is loaded by load_group under the same predicates
// (the same columns, [lo, hi) inside [0, W)) from the row y that the group's own row pointer gives, y in [0, H), through m's own stride,
// which the host checks to be >= W: srbh_compare.hip's argument.  The bitmap row y - yb lies in [0, rb) and the word pair read lies
// inside BM_WORDS + 1 words: srbh_zones.hip's argument.  The tables are read through checked indices only -- the item by blockIdx < NI,
// the zone's edge range only where 0 <= zone < Z and 0 <= a <= b <= E, the items of a zone through zone_items' checked range -- so no
// content of theirs leads outside them, the rasters' rows, ws or out; hostile tables give wrong sums at worst.  Stores: ten words to slot
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
    __shared__ unsigned bm[BM_WORDS + 1];                             // (+ 1: a group's bits are read as a pair of words)
    const int t = threadIdx.x;
    const long item = blockIdx.x;                                     // < NI
    const int* it = z.items + 5 * item;
    const int zone = it[0];
    const Rect w = clip_window(it + 1, q.r.H, q.r.W);
    int e0 = 0, e1 = 0;
    if (zone >= 0 && zone < z.Z) {
        const int a = z.edge_off[zone], b = z.edge_off[zone + 1];
        if (a >= 0 && a <= b && b <= z.E) { e0 = a; e1 = b; }
    }
    if (t == 0) bm[BM_WORDS] = 0u;
    ZPAcc acc = {0, {0, 0ll, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull}};
    if (w.any && e1 > e0) {                                           // uniform
        const int width = w.x1 - w.x0;
        const int full = (int)(((long)width + 31) >> 5);
        const int wpr = full < BM_MAX_WPR ? full : BM_MAX_WPR, segw = wpr * 32, rbmax = BM_WORDS / wpr;
        for (long done = 0; done < w.rows; done += rbmax) {
            const int yb = w.y0 + (int)done, left = w.rows - (int)done, rb = left < rbmax ? left : rbmax;
            for (long xl = w.x0; xl < w.x1; xl += segw) {
                const int xs = (int)xl, xe = xl + segw < w.x1 ? (int)(xl + segw) : w.x1;
                __syncthreads();                                      // the walk before is done with bm
                for (int i = t; i < rb * wpr; i += 256) bm[i] = 0u;
                __syncthreads();
                toggle_edges(z.edges, e0, e1, yb, rb, xs, xe, wpr, bm);
                __syncthreads();
                suffix_xor_rows(bm, rb, wpr);
                __syncthreads();
                walk_rect<EP, ER>(q.r, xs, xe, yb, rb, t, 256, [&](const G& g) {
                    const long y = (long)((((unsigned long long)(g.rowA - q.r.a)) >> q.row_tz) * q.row_inv);      // the raster row, in [yb, yb + rb)
                    const unsigned* brow = bm + ((int)y - yb) * wpr;
                    const int off = g.c0 - xs;                        // in (-P, segw)
                    unsigned zb;
                    if (off >= 0) {
                        const unsigned long long pair = brow[off >> 5] | ((unsigned long long)brow[(off >> 5) + 1] << 32);
                        zb = (unsigned)(pair >> (off & 31));
                    } else {
                        zb = brow[0] << -off;
                    }
                    zb &= g.inside();                                 // (bits beyond xe belong to the next row or are the suffix's spill)
                    if (!zb) return;
                    acc.cnt += __popc(zb);
                    // pair_select's test with the zone's bits in the place of the rectangle's: m is fetched for a pixel of the zone only
                    unsigned wp[G::WORDS_A], wr[G::WORDS_B];
                    g.load_a(wp);
                    g.load_b(wr);
                    unsigned P = 0, R = 0;
#pragma unroll
                    for (int j = 0; j < G::P; ++j) {
                        P |= ((int)group_pixel<EP>(wp, j) > q.pthr ? 1u : 0u) << j;
                        R |= ((int)group_pixel<ER>(wr, j) > q.rthr ? 1u : 0u) << j;
                    }
                    unsigned sel = q.mode == SRBH_PAIR_ANY ? (P | R) : q.mode == SRBH_PAIR_BOTH ? (P & R) : q.mode == SRBH_PAIR_REF ? R : P;
                    sel &= zb;
                    if (!sel) return;
                    if (EM) {
                        constexpr int EMM = EM ? EM : 1;
                        unsigned wm[G::P * EMM / 4];
                        load_group<EMM, G::P, false>(q.m + y * q.rsM * EMM, g.c0, g.W, g.lo, g.hi, wm);
                        unsigned ms = 0;
#pragma unroll
                        for (int j = 0; j < G::P; ++j) ms |= ((int)group_pixel<EMM>(wm, j) > q.mthr ? 1u : 0u) << j;
                        sel &= ms;
                        if (!sel) return;
                    }
                    PAcc& a = acc.a;
                    unsigned sp32 = 0, sr32 = 0, sad32 = 0;            // at most 16 values below 2^16
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
                        a.sdd += (unsigned long long)ad * ad;          // 32 x 32 -> 64
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
            }
        }
    }
    fold_team<256>(acc);
    if (t == 0) {
        long long* o = ws + 10 * item;
        o[0] = acc.cnt;
        o[1] = acc.a.n;
        o[2] = acc.a.sd;
        o[3] = (long long)acc.a.sad;
        o[4] = (long long)acc.a.sdd;
        o[5] = (long long)acc.a.sp;
        o[6] = (long long)acc.a.sr;
        o[7] = (long long)acc.a.spp;
        o[8] = (long long)acc.a.srr;
        o[9] = (long long)acc.a.spr;
    }
}

// a lane per zone: its items' partials added in item order
__global__ __launch_bounds__(256) void zone_pair_fold_kernel(const ZoneTables z, const long long* __restrict__ ws, long long* __restrict__ out) {
    const long zone = blockIdx.x * 256L + threadIdx.x;
    if (zone >= z.Z) return;
    int i0, i1;
    zone_items(z, (int)zone, &i0, &i1);
    long long s[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = i0; i < i1; ++i) {
        const long long* a = ws + 10 * (long)i;
#pragma unroll
        for (int k = 0; k < 10; ++k) s[k] += a[k];
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) out[10 * zone + k] = s[k];
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
    SumParams rows;                                                   // (zone_tables reads the value raster's row stride only: p's)
    rows.r = q.r;
    rows.vthr = rows.mthr = 0;
    ZoneTables z;
    rc = zone_tables(who, edges, edge_off, Z, E, items, item_off, NI, rows, typeP, &z);
    if (rc != SRBH_OK) return rc;
    SRBH_REQUIRE((uintptr_t)ws % 8 == 0 && (uintptr_t)out % 8 == 0, "%s: out and ws must be aligned to 8 bytes", who);
    hipStream_t st = (hipStream_t)stream;
    with_pair_sizes(typeP, typeR, m, typeM, [&](auto ep, auto er, auto em) {
        hipLaunchKernelGGL((zone_pair_kernel<decltype(ep)::value, decltype(er)::value, decltype(em)::value>), dim3((unsigned)NI), dim3(256), 0, st,
                           q, z, (long long*)ws);
    });
    SRBH_HIP(hipGetLastError());
    hipLaunchKernelGGL(zone_pair_fold_kernel, dim3((unsigned)((Z + 255L) / 256)), dim3(256), 0, st, z, (const long long*)ws, out);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
