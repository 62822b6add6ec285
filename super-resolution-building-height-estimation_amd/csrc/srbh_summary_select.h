// srbh_summary_select.h -- what the city summary (srbh_summary.hip) and the polygon zones (srbh_zones.hip) share: the parameters of the
// selection rule, the rule on one group of a walk (srbh_raster_walk.h), the partials a lane keeps, the histogram's division, and the host
// checks of the entry points.  A pixel is SELECTED when it lies inside the raster, v > vthr and (no mask or m > mthr).
#pragma once
#include "srbh_raster_walk.h"

namespace srbh {

struct SumParams {
    Rasters r;                      // a: the values v, b: the mask m
    int vthr, mthr;
};

constexpr int VH_MAX_BINS = 4096;

// v / d for 0 <= v < 2^16, 2 <= d < 2^16 is (v * M) >> 32 with M = floor(2^32 / d) + 1: M d = 2^32 + e with 0 < e <= d, so
// v M / 2^32 = v / d + v e / (d 2^32), and v e <= (2^16 - 1)^2 < 2^32 adds less than 1 / d: the floor does not move.  d == 1 would need
// M = 2^32 + 1, which 32 bits do not hold: magic 0 stands for it, and the quotient is v.
inline unsigned vh_magic(int d) { return d >= 2 && d <= 65535 ? (unsigned)(0x100000000ull / (unsigned)d) + 1u : 0u; }

// ---- host -----------------------------------------------------------------------------------------------------------------------------------
inline bool sum_type_ok(int type) { return type == SRBH_GRID_U16 || type == SRBH_GRID_U8; }

// the checks common to the entries; fills p.  SRBH_OK or SRBH_ERR_ARG (the error text is set)
inline int sum_params(const char* who, const void* v, int typeV, long rsV, const void* m, int typeM, long rsM, int H, int W, int vthr, int mthr,
                      SumParams* p) {
    SRBH_REQUIRE(sum_type_ok(typeV) && (!m || sum_type_ok(typeM)),
                 "%s: element type typeV=%d typeM=%d; the rasters are uint16 (1) or uint8 (3) -- int16, float32 and unknown codes are refused",
                 who, typeV, typeM);
    SRBH_REQUIRE(vthr >= -1 && vthr <= 65535 && mthr >= -1 && mthr <= 65535, "%s: a threshold (vthr=%d, mthr=%d) outside -1..65535", who,
                 vthr, mthr);
    p->vthr = vthr; p->mthr = mthr;
    return rasters_checked(who, v, typeV, rsV, m, typeM, rsM, H, W, &p->r);
}

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
// ---- device ---------------------------------------------------------------------------------------------------------------------------------
struct Acc {
    int n;
    unsigned mx;
    unsigned long long sum, sq;
    __device__ __forceinline__ Acc down(int o) const { return {__shfl_down(n, o, 64), __shfl_down(mx, o, 64), __shfl_down(sum, o, 64), __shfl_down(sq, o, 64)}; }
    __device__ __forceinline__ void merge(const Acc& o) {
        n += o.n;
        sum += o.sum;
        sq += o.sq;
        mx = mx > o.mx ? mx : o.mx;
    }
};

// The selection rule on one group: wv = the words of its P values of v, and bit j of the result: pixel j of the group is selected.  The
// value group is thresholded before the mask group is loaded.
template <int EV, int EM>
__device__ __forceinline__ unsigned select_group(const SumParams& p, const Group<EV, EM>& g, unsigned* wv) {
    using G = Group<EV, EM>;
    g.load_a(wv);
    unsigned sel = 0;
#pragma unroll
    for (int j = 0; j < G::P; ++j) sel |= ((int)group_pixel<EV>(wv, j) > p.vthr ? 1u : 0u) << j;
    sel &= g.inside();
    if (EM) {
        unsigned wm[G::WORDS_B];
        g.load_b(wm);
        unsigned ms = 0;
#pragma unroll
        for (int j = 0; j < G::P; ++j) ms |= ((int)group_pixel<G::EBB>(wm, j) > p.mthr ? 1u : 0u) << j;
        sel &= ms;
    }
    return sel;
}

// the selected pixels of a group (sel, wv: select_group's) added to a.  (sum_rect of srbh_summary.hip keeps this loop in its own lambda:
// called from there the compiler schedules window_sums_kernel differently, and its code object is to stay as it was.)
template <int EV>
__device__ __forceinline__ void add_group(Acc& a, unsigned sel, const unsigned* wv) {
    unsigned s32 = 0;                                                 // at most 16 values below 2^16
#pragma unroll
    for (int j = 0; j < 16 / EV; ++j) {
        const unsigned s = (sel >> j) & 1u ? group_pixel<EV>(wv, j) : 0u;
        s32 += s;
        a.sq += (unsigned long long)s * s;                            // 32 x 32 -> 64
        a.mx = a.mx > s ? a.mx : s;
    }
    a.n += __popc(sel);
    a.sum += s32;
}
#endif

}  // namespace srbh
