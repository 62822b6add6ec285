// srbh_zone_bitmap.h -- what the polygon-zone kernels (srbh_zones.hip, srbh_zone_compare.hip) share: the device tables of the zones, the
// LDS bitmap of a batch of rows (the edges' toggles, then the suffix XOR that turns them into the in-zone mask), the walk of one item
// that hands a client the groups with a pixel in the zone (zone_item_walk: the memory-safety argument of both files is stated there), the
// checked range of a zone's items, the kernel that adds each zone's items, and the host check of the tables.  The rule is stated in
// srbh_zones.hip and, in full, in include/srbh.h.
//
// Everything sits in the including file's own anonymous namespace, as it did in srbh_zones.hip: ZoneTables is a kernel parameter, and its
// name is part of the kernels' symbols.
#pragma once
#include "srbh_raster_walk.h"

namespace {
using namespace srbh;

constexpr int BM_WORDS = 2048;                          // the bitmap: 64 Ki pixels of a batch
constexpr int BM_MAX_WPR = 256;                         // words of a row of one segment: 8192 columns
constexpr int COORD_MAX = 1 << 29;

struct ZoneTables {
    const int4* edges;              // [E] (X0, Y0, X1, Y1)
    const int* edge_off;            // [Z + 1]
    const int* items;               // [NI][5] (zone, xoff, yoff, xcount, ycount)
    const int* item_off;            // [Z + 1]
    int Z, E, NI;
    RowDiv row;                     // of the row stride in bytes of the walk's raster a
};

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
// floor(a / b) for b > 0, the remainder in [0, b) to *r
__device__ __forceinline__ long long floor_div(long long a, long long b, long long* r) {
    long long q = a / b, m = a - q * b;
    if (m < 0) { m += b; --q; }
    *r = m;
    return q;
}

// step 1: the toggles of the zone's edges [e0, e1) in the rows [yb, yb + rb) and the columns [xs, xe); bm holds rb rows of wpr words, zeroed
__device__ __forceinline__ void toggle_edges(const int4* __restrict__ edges, int e0, int e1, int yb, int rb, int xs, int xe, int wpr, unsigned* bm) {
    for (int e = e0 + (int)threadIdx.x; e < e1; e += 256) {
        const int4 q = edges[e];
        int X0 = q.x, Y0 = q.y, X1 = q.z, Y1 = q.w;
        const bool ok = X0 >= -COORD_MAX && X0 <= COORD_MAX && X1 >= -COORD_MAX && X1 <= COORD_MAX && Y0 >= -COORD_MAX && Y0 <= COORD_MAX &&
                        Y1 >= -COORD_MAX && Y1 <= COORD_MAX;
        if (!ok || Y0 == Y1) continue;
        if (Y0 > Y1) { int s = X0; X0 = X1; X1 = s; s = Y0; Y0 = Y1; Y1 = s; }
        // the rows with Y0 <= 256 y + 128 < Y1
        int ya = (Y0 + 127) >> 8, ye = (Y1 + 127) >> 8;
        ya = ya > yb ? ya : yb;
        ye = ye < yb + rb ? ye : yb + rb;
        if (ya >= ye) continue;
        const long long den = (long long)Y1 - Y0, dx = (long long)X1 - X0, D = 256 * den;
        long long r, sr;
        long long t = floor_div(X0 * den + (256ll * ya + 128 - Y0) * dx + 128 * den - 1, D, &r);
        const long long st = floor_div(256 * dx, D, &sr);
        for (int y = ya; y < ye; ++y) {
            if (t > xs) {
                const int j = (int)(t < xe ? t : xe) - 1 - xs;
                atomicXor(&bm[(y - yb) * wpr + (j >> 5)], 1u << (j & 31));
            }
            t += st;
            r += sr;
            if (r >= D) { r -= D; ++t; }
        }
    }
}

// step 2: every row of bm (rb rows of wpr words) replaced by its inclusive suffix XOR: bit i = the XOR of the bits >= i of the row.  A wave
// takes 64 / G rows at a time, G = the power of two >= wpr (64 for wider rows, which go 64 words at a time from the right).
__device__ __forceinline__ void suffix_xor_rows(unsigned* bm, int rb, int wpr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int lg = 6;
    while (lg > 0 && (1 << (lg - 1)) >= wpr) --lg;
    const int G = 1 << lg, R = 64 >> lg, sub = lane >> lg, j = lane & (G - 1);
    const int chunks = (wpr + 63) >> 6;
    for (int r0 = wave * R; r0 < rb; r0 += 4 * R) {                   // uniform in a wave
        const int row = r0 + sub;
        unsigned carry = 0;
        for (int c = chunks - 1; c >= 0; --c) {
            const int w = c * 64 + j;
            const bool on = row < rb && w < wpr;
            unsigned v = on ? bm[row * wpr + w] : 0u;
            const unsigned long long par = __ballot(__popc(v) & 1);
            const unsigned long long mine = lg == 6 ? par : (par >> (sub * G)) & ((1ull << G) - 1ull);
            const unsigned right = (unsigned)__popcll((mine >> j) >> 1) & 1u;      // the words of this row to the right of w
            v ^= v >> 1; v ^= v >> 2; v ^= v >> 4; v ^= v >> 8; v ^= v >> 16;
            if (right ^ carry) v = ~v;
            if (on) bm[row * wpr + w] = v;
            carry ^= (unsigned)__popcll(mine) & 1u;
        }
    }
}

// the items [i0, i1) of zone z, or none where item_off does not lie inside [0, NI]
__device__ __forceinline__ void zone_items(const ZoneTables& z, int zone, int* i0, int* i1) {
    const int a = z.item_off[zone], b = z.item_off[zone + 1];
    const bool ok = a >= 0 && a <= b && b <= z.NI;
    *i0 = ok ? a : 0;
    *i1 = ok ? b : 0;
}

// One item, by its workgroup of 256 lanes (every lane calls): f(g, y, zb) once per (row, group) of this lane that has a pixel in the zone
// -- g the group of walk_rect<EA, EB> over r, y its raster row, bit j of zb: pixel j of the group lies in the zone and inside the raster.
// bm: BM_WORDS + 1 words of LDS (+ 1: a group's bits are read as a pair of words).  The item's band is done in batches of rows x segments
// of columns that fit the bitmap: zeroed, toggled by the zone's edges, turned into the in-zone mask by the suffix XOR, then walked.
//
// Memory safety.  The item is read at `item` < NI (the caller's blockIdx) and clip_window cuts it to the raster in 64 bits whatever it
// holds; the zone's edge range is used only where 0 <= zone < Z and 0 <= a <= b <= E, so no content of the tables leads outside them.
// walk_rect's groups lie in the rows [yb, yb + rb) of the batch, and the row y that a group's row pointer gives (an exact division, z.row
// being made from r's stride of a) is that row: the bitmap row y - yb lies in [0, rb), rb wpr <= BM_WORDS.  A group's first column lies
// in (xs - P, xs + segw), so the word pair read ends at word (rb - 1) wpr + (segw - 1) / 32 + 1 <= BM_WORDS at most: inside bm, whose
// last word is kept 0.  A group with no pixel in the zone loads nothing of the rasters.
template <int EA, int EB, class F>
__device__ __forceinline__ void zone_item_walk(const Rasters& r, const ZoneTables& z, long item, unsigned* bm, F&& f) {
    using G = Group<EA, EB>;
    const int t = threadIdx.x;
    if (t == 0) bm[BM_WORDS] = 0u;
    const int* q = z.items + 5 * item;
    const int zone = q[0];
    const Rect w = clip_window(q + 1, r.H, r.W);
    int e0 = 0, e1 = 0;
    if (zone >= 0 && zone < z.Z) {
        const int a = z.edge_off[zone], b = z.edge_off[zone + 1];
        if (a >= 0 && a <= b && b <= z.E) { e0 = a; e1 = b; }
    }
    if (!(w.any && e1 > e0)) return;                                  // uniform
    const int width = w.x1 - w.x0;
    const int full = (int)(((long)width + 31) >> 5);
    const int wpr = full < BM_MAX_WPR ? full : BM_MAX_WPR, segw = wpr * 32, rbmax = BM_WORDS / wpr;
    for (long done = 0; done < w.rows; done += rbmax) {
        const int yb = w.y0 + (int)done, left = w.rows - (int)done, rb = left < rbmax ? left : rbmax;
        for (long xl = w.x0; xl < w.x1; xl += segw) {
            const int xs = (int)xl, xe = xl + segw < w.x1 ? (int)(xl + segw) : w.x1;
            __syncthreads();                                          // the walk before is done with bm
            for (int i = t; i < rb * wpr; i += 256) bm[i] = 0u;
            __syncthreads();
            toggle_edges(z.edges, e0, e1, yb, rb, xs, xe, wpr, bm);
            __syncthreads();
            suffix_xor_rows(bm, rb, wpr);
            __syncthreads();
            walk_rect<EA, EB>(r, xs, xe, yb, rb, t, 256, [&](const G& g) {
                const long y = row_index(z.row, (unsigned long long)(g.rowA - r.a));      // the raster row, in [yb, yb + rb)
                const unsigned* brow = bm + ((int)y - yb) * wpr;
                const int off = g.c0 - xs;                            // in (-P, segw)
                unsigned zb;
                if (off >= 0) {
                    const unsigned long long pair = brow[off >> 5] | ((unsigned long long)brow[(off >> 5) + 1] << 32);
                    zb = (unsigned)(pair >> (off & 31));
                } else {
                    zb = brow[0] << -off;
                }
                zb &= g.inside();                                     // (bits beyond xe belong to the next row or are the suffix's spill)
                if (!zb) return;
                f(g, y, zb);
            });
        }
    }
}

// A lane per zone: its items' rows of K words in ws added in item order to row `zone` of out; column MAXCOL (-1: none) takes the largest
template <int K, int MAXCOL>
__global__ __launch_bounds__(256) void zone_fold_kernel(const ZoneTables z, const long long* __restrict__ ws, long long* __restrict__ out) {
    const long zone = blockIdx.x * 256L + threadIdx.x;
    if (zone >= z.Z) return;
    int i0, i1;
    zone_items(z, (int)zone, &i0, &i1);
    long long s[K] = {};
    for (int i = i0; i < i1; ++i) {
        const long long* a = ws + K * (long)i;
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] = k == MAXCOL ? (s[k] > a[k] ? s[k] : a[k]) : s[k] + a[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) out[K * zone + k] = s[k];
}
#endif

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
// the checks of the tables; fills z.  stride_bytes: the row stride of the raster that the item kernel walks as raster a (> 0)
int zone_tables(const char* who, const int* edges, const int* edge_off, int Z, int E, const int* items, const int* item_off, int NI,
                unsigned long long stride_bytes, ZoneTables* z) {
    SRBH_REQUIRE(edges && edge_off && items && item_off, "%s: null table", who);
    SRBH_REQUIRE(Z > 0 && E > 0 && NI > 0, "%s: Z=%d, E=%d and the item count %d must be positive", who, Z, E, NI);
    SRBH_REQUIRE((uintptr_t)edges % 16 == 0 && (uintptr_t)edge_off % 4 == 0 && (uintptr_t)items % 4 == 0 && (uintptr_t)item_off % 4 == 0,
                 "%s: edges must be aligned to 16 bytes, the other tables to 4", who);
    z->edges = (const int4*)edges; z->edge_off = edge_off; z->items = items; z->item_off = item_off;
    z->Z = Z; z->E = E; z->NI = NI;
    z->row = row_div(stride_bytes);
    return SRBH_OK;
}

}  // namespace
