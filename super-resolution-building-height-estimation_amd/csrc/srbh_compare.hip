// srbh_compare.hip -- how good a predicted city is against a reference height raster on the same grid: the reference answers that per
// file (cal_rmse, demo_preprocess_height_v2.py:1389-1406: a height product against the label, RMSE over the pixels where they differ),
// per shapefile feature (the compare_twotiff_valid* family, one GDAL window read per cell) and per float tile (vtest_epoch2, train.py:
// HeightMetric per height class, SegmentationMetric of the class map).  Here: exact integer sums over a pair of rasters, per window
// (srbh_pair_sums) and per height class of the reference with the confusion matrix of the classes (srbh_pair_class_sums).
//
// p is the predicted raster, r the reference, m an optional third raster (the class raster), d = p - r, signed.  A pixel is COMPARED when
// it lies inside the raster (and the window), the pair test of `mode` holds -- with P := p > pthr and R := r > rthr: ANY P or R, BOTH P
// and R, REF R, PRED P -- and (no m or m > mthr).  Thresholds lie in -1..65535; -1 makes a test always true.  All three rasters are uint16
// or uint8, each read in place through its own row stride.  Integers only: exact, no order, bit-equal between runs.  No floating point.
//
// The walk is srbh_raster_walk.h's (p is its raster a, r its raster b; why no load leaves a raster is argued there).  The third raster is
// not part of Rasters / Group: a group's row index is recovered from its row pointer (an exact division by p's row stride in bytes: a
// shift and a multiplication by the odd part's inverse modulo 2^64, srbh_raster_walk.h's RowDiv), and m's pixels of the same columns are
// fetched by load_group under the same predicates -- m's rows are addressed through its own stride, which the host checks to be >= W.
//
// Overflow.  H * W < 2^31 (the host requires it) and every value is below 2^16:
//   count, n                 < 2^31
//   sp, sr, sad, |sd|        <= 65535 * (2^31 - 1) < 2^47
//   spp, srr, spr, sdd       <= 65535^2 * (2^31 - 1) < 2^32 * 2^31 = 2^63
// so every sum fits int64.  Within a group (at most 16 pixels) the sums of p, r, d and |d| stay below 2^20 and are formed in 32 bits;
// squares and products enter 64-bit lane sums through 32 x 32 -> 64-bit multiply-adds.
#include "srbh_pair_pieces.h"

#ifndef SRBH_PAIR_CLASS_DIRECT
#define SRBH_PAIR_CLASS_DIRECT 0      // developer A/B only: 1 = one LDS update per pixel and table entry, no combining in registers
#endif

namespace {
using namespace srbh;

constexpr int PC_MAX_C = 16;
constexpr int PC_MAX_WGS = 2048;
constexpr int PC_GROUPS_PER_LANE = 8;                  // a workgroup is worth launching for 256 * 8 groups of 16 bytes

struct ClassParams {
    int C;
    int edges[PC_MAX_C];            // edges[k] for k >= C: INT_MAX, which no value reaches
};

// ---- device ---------------------------------------------------------------------------------------------------------------------------------
// EP, ER, EM: element sizes of p, r and m in bytes (EM == 0: no third raster)
template <int EP, int ER, int EM>
__global__ __launch_bounds__(256) void pair_sums_kernel(const PairParams q, const int* __restrict__ pos, long long* __restrict__ out) {
    using G = Group<EP, ER>;
    const Rect w = clip_window(pos + 4 * (long)blockIdx.x, q.r.H, q.r.W);
    PAcc a = {};
    if (w.any) {                                                      // uniform
        walk_rect<EP, ER>(q.r, w.x0, w.x1, w.y0, w.rows, threadIdx.x, 256, [&](const G& g) {
            unsigned wp[G::WORDS_A], wr[G::WORDS_B], wm[G::P * (EM ? EM : 1) / 4];
            const unsigned sel = pair_select<EP, ER, EM>(q, g, wp, wr, wm);
            if (!sel) return;
            unsigned sp32 = 0, sr32 = 0, sad32 = 0;                    // at most 16 values below 2^16
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
                a.sdd += (unsigned long long)ad * ad;                  // 32 x 32 -> 64
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
    fold_team<256>(a);
    if (threadIdx.x == 0) a.store(out + 10 * (long)blockIdx.x, (long long)(w.x1 - w.x0) * w.rows);
}

// ---- per class ------------------------------------------------------------------------------------------------------------------------------
// The class of v: the number of k in 1 .. C - 1 with v >= edges[k] (the unused edges are INT_MAX)
__device__ __forceinline__ int class_of(const ClassParams& c, unsigned v) {
    int k = 0;
#pragma unroll
    for (int i = 1; i < PC_MAX_C / 2; ++i) k += (int)v >= c.edges[i] ? 1 : 0;
    if (c.C > PC_MAX_C / 2) {                                         // uniform
#pragma unroll
        for (int i = PC_MAX_C / 2; i < PC_MAX_C; ++i) k += (int)v >= c.edges[i] ? 1 : 0;
    }
    return k;
}

// whether the n words of a group hold one value of E bytes throughout
template <int E, int N>
__device__ __forceinline__ bool one_value(const unsigned* w) {
    unsigned diff = E == 1 ? w[0] ^ ((w[0] & 0xffu) * 0x01010101u) : w[0] ^ ((w[0] & 0xffffu) * 0x00010001u);
#pragma unroll
    for (int i = 1; i < N; ++i) diff |= w[i] ^ w[0];
    return diff == 0u;
}

inline long pc_wgs(int H, int W) {
    const long groups = (long)H * (((long)W + 14) / 8 + 1);           // not below the (row, group) pairs of either element size
    const long wgs = (groups + 256L * PC_GROUPS_PER_LANE - 1) / (256L * PC_GROUPS_PER_LANE);
    return wgs < PC_MAX_WGS ? wgs : PC_MAX_WGS;
}

inline int pc_entries(int C) { return C * (4 + C) + 1; }

// The table of a workgroup, in out's layout: row c = { n, sd, sad, sdd, cm[c][0 .. C - 1] }, then bad.  64-bit LDS integer atomics: the
// result does not depend on their order.  The hazard is contention (a reference raster is mostly zeros: almost every lane hits class 0),
// so a lane combines on the way in: a group that holds one value of each raster throughout is one update, not P; and the lane carries
// the sums of its current class and the count of its current cm entry in registers and updates the table only when the class or the entry
// changes, and once at the end.
struct ClassCarry {
    int cls, n;                     // the class carried (-1: none) and its pixels
    long long sd;
    unsigned long long sad, sdd;
    int entry;                      // the table entry (a cm entry or bad) carried (-1: none) and its count
    unsigned cnt;
};

__device__ __forceinline__ void flush_class(unsigned long long* tab, int C, ClassCarry& k) {
    if (k.cls >= 0 && k.n) {
        unsigned long long* t = tab + k.cls * (4 + C);
        atomicAdd(t + 0, (unsigned long long)k.n);
        atomicAdd(t + 1, (unsigned long long)k.sd);                    // (two's complement: the sum of the addends modulo 2^64 is sd)
        atomicAdd(t + 2, k.sad);
        atomicAdd(t + 3, k.sdd);
    }
    k.n = 0; k.sd = 0; k.sad = 0; k.sdd = 0;
}

__device__ __forceinline__ void flush_entry(unsigned long long* tab, ClassCarry& k) {
    if (k.entry >= 0 && k.cnt) atomicAdd(tab + k.entry, (unsigned long long)k.cnt);
    k.cnt = 0;
}

template <int EP, int ER, int EM>
__global__ __launch_bounds__(256) void pair_class_kernel(const PairParams q, const ClassParams c, unsigned long long* __restrict__ ws) {
    using G = Group<EP, ER>;
    __shared__ unsigned long long tab[PC_MAX_C * (4 + PC_MAX_C) + 1];
    const int t = threadIdx.x, C = c.C, T = C * (4 + C) + 1;
    for (int i = t; i < T; i += 256) tab[i] = 0ull;
    __syncthreads();
    ClassCarry k = {-1, 0, 0ll, 0ull, 0ull, -1, 0u};
    walk_rect<EP, ER>(q.r, 0, q.r.W, 0, q.r.H, (int)blockIdx.x * 256 + t, (int)gridDim.x * 256, [&](const G& g) {
        constexpr int EMM = EM ? EM : 1, WORDS_M = G::P * EMM / 4;
        unsigned wp[G::WORDS_A], wr[G::WORDS_B], wm[WORDS_M];
        const unsigned sel = pair_select<EP, ER, EM>(q, g, wp, wr, wm);
        if (!sel) return;
        // `mult` compared pixels that hold the same (p, r, m): mult <= 16, so d * mult and |d| * mult stay below 2^20
        auto add = [&](unsigned pv, unsigned rv, unsigned mv, unsigned mult) {
            const int d = (int)pv - (int)rv;
            const unsigned ad = (unsigned)(d < 0 ? -d : d);
            const int cls = class_of(c, rv);
            const int pc = EM ? (int)mv : class_of(c, pv);
            const int entry = pc < C ? cls * (4 + C) + 4 + pc : C * (4 + C);          // a class beyond the table: bad
#if SRBH_PAIR_CLASS_DIRECT
            unsigned long long* tc = tab + cls * (4 + C);
            atomicAdd(tc + 0, (unsigned long long)mult);
            atomicAdd(tc + 1, (unsigned long long)(long long)(d * (int)mult));
            atomicAdd(tc + 2, (unsigned long long)(ad * mult));
            atomicAdd(tc + 3, (unsigned long long)(ad * mult) * ad);
            atomicAdd(tab + entry, (unsigned long long)mult);
#else
            if (cls != k.cls) { flush_class(tab, C, k); k.cls = cls; }
            if (entry != k.entry) { flush_entry(tab, k); k.entry = entry; }
            k.n += (int)mult;
            k.sd += d * (int)mult;
            k.sad += ad * mult;
            k.sdd += (unsigned long long)(ad * mult) * ad;                            // 32 x 32 -> 64
            k.cnt += mult;
#endif
        };
        // one update per group where the group holds one value of each raster throughout (a reference raster is mostly zeros, in runs far
        // longer than a group); the pixels outside the rectangle are raster pixels or 0, so the test can only miss, never misjudge
        if (!SRBH_PAIR_CLASS_DIRECT && one_value<EP, G::WORDS_A>(wp) && one_value<ER, G::WORDS_B>(wr) && (!EM || one_value<EMM, WORDS_M>(wm))) {
            add(group_pixel<EP>(wp, 0), group_pixel<ER>(wr, 0), EM ? group_pixel<EMM>(wm, 0) : 0u, (unsigned)__popc(sel));
            return;
        }
#pragma unroll
        for (int j = 0; j < G::P; ++j) {
            if ((sel >> j) & 1u) add(group_pixel<EP>(wp, j), group_pixel<ER>(wr, j), EM ? group_pixel<EMM>(wm, j) : 0u, 1u);
        }
    });
    flush_class(tab, C, k);
    flush_entry(tab, k);
    __syncthreads();
    for (int i = t; i < T; i += 256) ws[(long)blockIdx.x * T + i] = tab[i];
}

// block b owns the entries 16 b .. 16 b + 15; thread t adds the slots (t >> 4), (t >> 4) + 16, ... of entry 16 b + (t & 15), then the 16
// partial sums of an entry are added through LDS in a fixed order
__global__ __launch_bounds__(256) void pair_class_fold_kernel(const unsigned long long* __restrict__ ws, int nwg, int T, long long* __restrict__ out) {
    __shared__ unsigned long long part[16][16];
    const int t = threadIdx.x, e = blockIdx.x * 16 + (t & 15), grp = t >> 4;
    unsigned long long a = 0;
    if (e < T) {
#pragma unroll 4
        for (int s = grp; s < nwg; s += 16) a += ws[(long)s * T + e];
    }
    part[grp][t & 15] = a;
    __syncthreads();
    if (t < 16 && e < T) {
        unsigned long long s = 0;
#pragma unroll
        for (int g = 0; g < 16; ++g) s += part[g][t];
        out[e] = (long long)s;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
}  // namespace

extern "C" int srbh_pair_sums(const void* p, int typeP, long row_strideP, const void* r, int typeR, long row_strideR, const void* m, int typeM,
                              long row_strideM, int H, int W, const int* pos, int N, int mode, int pthr, int rthr, int mthr, long long* out,
                              void* stream) {
    SRBH_REQUIRE(pos && out, "srbh_pair_sums: null pointer");
    SRBH_REQUIRE(N > 0, "srbh_pair_sums: N=%d must be positive", N);
    PairParams q;
    const int rc = pair_params("srbh_pair_sums", p, typeP, row_strideP, r, typeR, row_strideR, m, typeM, row_strideM, H, W, mode, pthr, rthr,
                               mthr, &q);
    if (rc != SRBH_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    with_pair_sizes(typeP, typeR, m, typeM, [&](auto ep, auto er, auto em) {
        hipLaunchKernelGGL((pair_sums_kernel<decltype(ep)::value, decltype(er)::value, decltype(em)::value>), dim3((unsigned)N), dim3(256), 0, st,
                           q, pos, out);
    });
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" size_t srbh_pair_class_ws_bytes(int H, int W, int C) {
    if (H <= 0 || W <= 0 || C < 2 || C > PC_MAX_C || (long)H * W >= 0x80000000L) return 0;
    return (size_t)pc_wgs(H, W) * pc_entries(C) * sizeof(unsigned long long);
}

extern "C" int srbh_pair_class_sums(const void* p, int typeP, long row_strideP, const void* r, int typeR, long row_strideR, const void* m,
                                    int typeM, long row_strideM, int H, int W, const int* edges, int C, int mode, int pthr, int rthr, int mthr,
                                    long long* out, void* ws, void* stream) {
    SRBH_REQUIRE(out && ws && edges, "srbh_pair_class_sums: null pointer");
    SRBH_REQUIRE(C >= 2 && C <= PC_MAX_C, "srbh_pair_class_sums: C=%d outside 2..%d", C, PC_MAX_C);
    SRBH_REQUIRE(edges[0] == 0, "srbh_pair_class_sums: edges[0]=%d must be 0", edges[0]);
    ClassParams c;
    c.C = C;
    for (int k = 0; k < PC_MAX_C; ++k) {
        SRBH_REQUIRE(k == 0 || k >= C || edges[k] > edges[k - 1], "srbh_pair_class_sums: edges[%d]=%d is not above edges[%d]=%d", k, edges[k],
                     k - 1, edges[k - 1]);
        c.edges[k] = k < C ? edges[k] : 0x7fffffff;
    }
    SRBH_REQUIRE((uintptr_t)ws % 8 == 0 && (uintptr_t)out % 8 == 0, "srbh_pair_class_sums: out and ws must be aligned to 8 bytes");
    PairParams q;
    const int rc = pair_params("srbh_pair_class_sums", p, typeP, row_strideP, r, typeR, row_strideR, m, typeM, row_strideM, H, W, mode, pthr,
                               rthr, mthr, &q);
    if (rc != SRBH_OK) return rc;
    const int nwg = (int)pc_wgs(H, W), T = pc_entries(C);
    hipStream_t st = (hipStream_t)stream;
    with_pair_sizes(typeP, typeR, m, typeM, [&](auto ep, auto er, auto em) {
        hipLaunchKernelGGL((pair_class_kernel<decltype(ep)::value, decltype(er)::value, decltype(em)::value>), dim3((unsigned)nwg), dim3(256), 0, st,
                           q, c, (unsigned long long*)ws);
    });
    SRBH_HIP(hipGetLastError());
    hipLaunchKernelGGL(pair_class_fold_kernel, dim3((unsigned)((T + 15) / 16)), dim3(256), 0, st, (const unsigned long long*)ws, nwg, T, out);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
