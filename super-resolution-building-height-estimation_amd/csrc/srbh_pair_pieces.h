// srbh_pair_pieces.h -- what the pair kernels (srbh_compare.hip, srbh_zone_compare.hip) share: the parameters of the comparison of a
// predicted raster p with a reference r under an optional third raster m, the two parts of the COMPARED test on one group of a walk, the
// nine sums a lane keeps and the row they are stored as, and the host routine that checks the arguments and fills the parameters.  The
// rule and the overflow argument are stated in srbh_compare.hip and include/srbh.h.
//
// Everything sits in the including file's own anonymous namespace, as it did in srbh_compare.hip: PairParams is a kernel parameter, and
// its name is part of the kernels' symbols.
#pragma once
#include "srbh_raster_walk.h"

namespace {
using namespace srbh;

struct PairParams {
    Rasters r;                      // a: the predicted raster p, b: the reference r
    const unsigned char* m;         // NULL: no third raster
    long rsM;                       // its row stride in elements
    int mode, pthr, rthr, mthr;
    RowDiv row;                     // of p's row stride in bytes
};

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
// ---- device ---------------------------------------------------------------------------------------------------------------------------------
// The COMPARED test comes in two parts, so that a caller puts its own pixels (a rectangle's, a zone's) between them and the third raster
// is fetched only where one of those passed the first.  Part one, bit j: pixel j of the group passes the pair test of q.mode.  wp, wr:
// the group's words of p and r
template <int EP, int ER>
__device__ __forceinline__ unsigned pair_test(const PairParams& q, const unsigned* wp, const unsigned* wr) {
    unsigned P = 0, R = 0;
#pragma unroll
    for (int j = 0; j < 16 / EP; ++j) {
        P |= ((int)group_pixel<EP>(wp, j) > q.pthr ? 1u : 0u) << j;
        R |= ((int)group_pixel<ER>(wr, j) > q.rthr ? 1u : 0u) << j;
    }
    return q.mode == SRBH_PAIR_ANY ? (P | R) : q.mode == SRBH_PAIR_BOTH ? (P & R) : q.mode == SRBH_PAIR_REF ? R : P;
}

// Part two, bit j: m > mthr at pixel j of the group, which lies in raster row y (in [0, H)).  wm: the group's words of m
template <int EM, class G>
__device__ __forceinline__ unsigned third_test(const PairParams& q, const G& g, long y, unsigned* wm) {
    load_group<EM, G::P, false>(q.m + y * q.rsM * EM, g.c0, g.W, g.lo, g.hi, wm);
    unsigned ms = 0;
#pragma unroll
    for (int j = 0; j < G::P; ++j) ms |= ((int)group_pixel<EM>(wm, j) > q.mthr ? 1u : 0u) << j;
    return ms;
}

// both parts over a rectangle's group: bit j: pixel j of the group is compared.  wm is loaded only when a pixel passed the pair test
template <int EP, int ER, int EM>
__device__ __forceinline__ unsigned pair_select(const PairParams& q, const Group<EP, ER>& g, unsigned* wp, unsigned* wr, unsigned* wm) {
    g.load_a(wp);
    g.load_b(wr);
    unsigned sel = pair_test<EP, ER>(q, wp, wr) & g.inside();
    if (EM) {
        if (!sel) return 0u;
        sel &= third_test<(EM ? EM : 1)>(q, g, row_index(q.row, (unsigned long long)(g.rowA - q.r.a)), wm);
    }
    return sel;
}

// The nine sums of a lane; PAcc{} is their zero.  (The loop that adds a group's compared pixels -- 32 bits inside a group, 64 bits across
// groups -- stays in the lambdas of pair_sums_kernel and zone_pair_kernel: as a function of this header, whether free, a member, taking
// the words by pointer, by array reference or by value, it is simplified on its own before it is inlined, the sixteen selects then come
// first, and kernels of both files need up to 10 more vector registers; profiles/zone_item_walk_isa.txt has the figures.)
struct PAcc {
    int n;
    long long sd;
    unsigned long long sad, sdd, sp, sr, spp, srr, spr;
    __device__ __forceinline__ PAcc down(int o) const {
        return {__shfl_down(n, o, 64),   __shfl_down(sd, o, 64),  __shfl_down(sad, o, 64), __shfl_down(sdd, o, 64), __shfl_down(sp, o, 64),
                __shfl_down(sr, o, 64),  __shfl_down(spp, o, 64), __shfl_down(srr, o, 64), __shfl_down(spr, o, 64)};
    }
    __device__ __forceinline__ void merge(const PAcc& o) {
        n += o.n; sd += o.sd; sad += o.sad; sdd += o.sdd; sp += o.sp; sr += o.sr; spp += o.spp; srr += o.srr; spr += o.spr;
    }
    // the row [count, n, sd, sad, sdd, sp, sr, spp, srr, spr] of out and of a workspace slot
    __device__ __forceinline__ void store(long long* o, long long count) const {
        o[0] = count;
        o[1] = n;
        o[2] = sd;
        o[3] = (long long)sad;
        o[4] = (long long)sdd;
        o[5] = (long long)sp;
        o[6] = (long long)sr;
        o[7] = (long long)spp;
        o[8] = (long long)srr;
        o[9] = (long long)spr;
    }
};
#endif

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
inline bool pair_type_ok(int type) { return type == SRBH_GRID_U16 || type == SRBH_GRID_U8; }

// the checks common to the entries; fills q.  SRBH_OK or SRBH_ERR_ARG (the error text is set)
int pair_params(const char* who, const void* p, int typeP, long rsP, const void* r, int typeR, long rsR, const void* m, int typeM, long rsM,
                int H, int W, int mode, int pthr, int rthr, int mthr, PairParams* q) {
    SRBH_REQUIRE(p && r, "%s: null raster", who);
    SRBH_REQUIRE(pair_type_ok(typeP) && pair_type_ok(typeR) && (!m || pair_type_ok(typeM)),
                 "%s: element type typeP=%d typeR=%d typeM=%d; the rasters are uint16 (1) or uint8 (3) -- int16, float32 and unknown codes are "
                 "refused", who, typeP, typeR, typeM);
    SRBH_REQUIRE(mode >= SRBH_PAIR_ANY && mode <= SRBH_PAIR_PRED, "%s: mode=%d outside 0..3", who, mode);
    SRBH_REQUIRE(pthr >= -1 && pthr <= 65535 && rthr >= -1 && rthr <= 65535 && mthr >= -1 && mthr <= 65535,
                 "%s: a threshold (pthr=%d, rthr=%d, mthr=%d) outside -1..65535", who, pthr, rthr, mthr);
    const int rc = rasters_checked(who, p, typeP, rsP, r, typeR, rsR, H, W, &q->r);
    if (rc != SRBH_OK) return rc;
    SRBH_REQUIRE(!m || rsM >= W, "%s: the third raster's row stride %ld is below W=%d", who, rsM, W);
    SRBH_REQUIRE(!m || (uintptr_t)m % raster_esz(typeM) == 0, "%s: the third raster is not aligned to its element size", who);
    q->m = (const unsigned char*)m;
    q->rsM = m ? rsM : 0;
    q->mode = mode; q->pthr = pthr; q->rthr = rthr; q->mthr = mthr;
    q->row = row_div((unsigned long long)rsP * (unsigned)raster_esz(typeP));
    return SRBH_OK;
}

// f(integral_constant EP, ER, EM) for the element sizes of the three rasters (EM == 0: no m)
template <class F>
inline void with_pair_sizes(int typeP, int typeR, const void* m, int typeM, F&& f) {
    with_const<2>(raster_esz(typeP) - 1, [&](auto ep) {
        return with_const<2>(raster_esz(typeR) - 1, [&](auto er) {
            return with_const<3>(m ? raster_esz(typeM) : 0, [&](auto em) {
                return f(std::integral_constant<int, decltype(ep)::value + 1>{}, std::integral_constant<int, decltype(er)::value + 1>{}, em), 0;
            });
        });
    });
}

}  // namespace
