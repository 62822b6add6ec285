// srbh_raster_walk.h -- how the city kernels (srbh_cells.hip, srbh_summary.hip, and the zone and pair kernels through their own headers)
// read a rectangle of one or two (H, W) integer rasters in place: the group loader, the walk of a rectangle by a team of lanes, the clip
// of a window to the raster, the fold of a team's partials, the row divisor that gives a group's row back from its row pointer, and the
// host checks and element-size dispatch of their entry points.
//
// The walk and why no load leaves a raster.  A rectangle [x0, x1) x [y0, y0 + rows) INSIDE the raster is cut, row by row, into groups of
// P = 16 / sizeof(element of a) pixels that start on 16-byte boundaries of a's ADDRESS: xoff = k * 56, an odd W and a cropped view give
// every row its own alignment, so the group grid is computed per row, from the address of the row's first pixel of the rectangle.  A lane
// of the team takes one (row, group) at a time:
//   * a group whose P pixels all lie inside the raster's row [0, W) is fetched by one aligned 16-byte load, and the caller masks off the
//     pixels outside [x0, x1) (Group::inside) -- the head and the tail of a rectangle's row read raster pixels next to it, never anything
//     else;
//   * any other group (it would start before the row's first byte or end behind its last) is fetched pixel by pixel, each load predicated
//     on the rectangle, which lies inside the raster.
// The same P pixels of the second raster b are fetched by the same rule; b has its own element size, stride and alignment, so its wide
// load is one of element alignment only.  Rows are addressed through each raster's own stride, which the host checks to be at least W.
// So no load touches a byte outside the rows' own bytes of either raster, whatever the windows hold: clip_window turns any content of
// pos into a rectangle inside the raster (or none) in 64 bits, and the block and histogram kernels form theirs from H and W.
#pragma once
#include "srbh_internal.h"

namespace srbh {

// two rasters on one H x W grid, each read in place; a's address fixes the group grid
struct Rasters {
    const unsigned char* a;
    const unsigned char* b;         // NULL: one raster
    long rsA, rsB;                  // row strides in elements
    int H, W;
};

// The exact division of a byte offset inside raster a by its row stride, for the kernels that recover a group's row from its row pointer:
// the stride in bytes is odd << tz, and inv * odd == 1 modulo 2^64.
struct RowDiv {
    int tz;
    unsigned long long inv;
};

// ---- host: what the entry points of both files check and choose alike -------------------------------------------------------------------
inline int raster_esz(int type) { return type == SRBH_GRID_U8 ? 1 : 2; }

inline RowDiv row_div(unsigned long long stride_bytes) {              // > 0
    const int tz = __builtin_ctzll(stride_bytes);
    const unsigned long long odd = stride_bytes >> tz;
    unsigned long long inv = odd;                                     // correct to 3 bits; each step doubles them
    for (int i = 0; i < 5; ++i) inv *= 2ull - odd * inv;
    return {tz, inv};
}

// The checks common to every entry, made after the entry has judged the type codes (the accepted sets differ); fills r.  SRBH_OK or
// SRBH_ERR_ARG (the error text is set, `who` in front).  b == NULL makes typeB and rsB irrelevant.
inline int rasters_checked(const char* who, const void* a, int typeA, long rsA, const void* b, int typeB, long rsB, int H, int W, Rasters* r) {
    SRBH_REQUIRE(a, "%s: null raster", who);
    SRBH_REQUIRE(H > 0 && W > 0, "%s: bad geometry H=%d W=%d", who, H, W);
    SRBH_REQUIRE(rsA >= W && (!b || rsB >= W), "%s: a row stride (%ld, %ld) is below W=%d", who, rsA, b ? rsB : rsA, W);
    // a rectangle's counts are formed in 32 bits; the windows live on the device, so the raster bounds them
    SRBH_REQUIRE((long)H * W < 0x80000000L, "%s: H * W = %ld must stay below 2^31", who, (long)H * W);
    SRBH_REQUIRE((uintptr_t)a % raster_esz(typeA) == 0 && (!b || (uintptr_t)b % raster_esz(typeB) == 0),
                 "%s: a raster is not aligned to its element size", who);
    r->a = (const unsigned char*)a; r->b = (const unsigned char*)b;
    r->rsA = rsA; r->rsB = b ? rsB : 0;
    r->H = H; r->W = W;
    return SRBH_OK;
}

// f(integral_constant EA, integral_constant EB) for the element sizes of the two rasters (EB == 0: no b)
template <class F>
inline void with_sizes(int typeA, const void* b, int typeB, F&& f) {
    with_const<2>(raster_esz(typeA) - 1, [&](auto ea) {
        return with_const<3>(b ? raster_esz(typeB) : 0, [&](auto eb) { return f(std::integral_constant<int, decltype(ea)::value + 1>{}, eb), 0; });
    });
}

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
// ---- device ---------------------------------------------------------------------------------------------------------------------------------
// A group in registers: its P elements of E bytes as they lie in memory, in P * E / 4 words -- both ways of loading it end in the same
// four registers (P values each would be sixteen across the join, and the compiler then keeps them as one vector that every predicated
// load copies: profiles/raster_walk_isa.txt).  Pixel j of the group:
template <int E>
__device__ __forceinline__ unsigned group_pixel(const unsigned* w, int j) {
    return E == 1 ? (w[j >> 2] >> (8 * (j & 3))) & 0xffu : (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
}

// w = the pixels c0 .. c0 + P - 1 of the row at `row` (its pixel 0): pixel j is the raster's for every j of [lo, hi), a non-empty part
// of [0, P) whose pixels lie inside [0, W); the other pixels are raster pixels of the same row or 0.  ALIGNED: row + c0 * E is a 16-byte
// boundary whenever the wide load is taken (P * E == 16).
template <int E, int P, bool ALIGNED>
__device__ __forceinline__ void load_group(const unsigned char* row, int c0, int W, int lo, int hi, unsigned* w) {
    constexpr int WORDS = P * E / 4;
    if (c0 >= 0 && c0 <= W - P) {
        const unsigned char* src = row + (long)c0 * E;
        if (ALIGNED) {
            const uint4 q = *reinterpret_cast<const uint4*>(src);
            w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else {
            __builtin_memcpy(w, __builtin_assume_aligned(src, E), WORDS * 4);
        }
    } else {
#pragma unroll
        for (int i = 0; i < WORDS; ++i) w[i] = 0u;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            if (j >= lo && j < hi) {
                const unsigned v = E == 1 ? (unsigned)row[c0 + j] : (unsigned)reinterpret_cast<const unsigned short*>(row)[c0 + j];
                w[j * E / 4] |= v << (8 * E * (j % (4 / E)));
            }
        }
    }
}

// the row whose first byte lies `bytes` behind the raster's: bytes is a whole multiple of the stride d was made from
__device__ __forceinline__ long row_index(const RowDiv& d, unsigned long long bytes) { return (long)((bytes >> d.tz) * d.inv); }

// One (row, group) of a walk, handed to its functor: nothing is loaded until the functor asks, so it decides when b's group is in
// registers (a client that thresholds a's group first keeps one group live, not two).
template <int EA, int EB>
struct Group {
    static constexpr int P = 16 / EA, EBB = EB ? EB : 1;
    static constexpr int WORDS_A = 4, WORDS_B = P * EBB / 4;       // of a group of a and of b
    const unsigned char* rowA;
    const unsigned char* rowB;      // of the same raster row; not read when EB == 0
    int c0, W;                      // the group's first pixel (it may lie outside [0, W))
    int lo, hi;                     // the rectangle's pixels of this group: [lo, hi) of [0, P), hi > lo
    __device__ __forceinline__ unsigned inside() const { return ((1u << (hi - lo)) - 1u) << lo; }      // bit j: pixel j is in the rectangle
    __device__ __forceinline__ void load_a(unsigned* w) const { load_group<EA, P, true>(rowA, c0, W, lo, hi, w); }
    __device__ __forceinline__ void load_b(unsigned* w) const { load_group<EBB, P, false>(rowB, c0, W, lo, hi, w); }
};

// The rectangle [x0, x1) x [y0, y0 + rows) -- inside the raster, not empty -- walked by `team` lanes, this one being lane `tid` of them:
// f(group) once per (row, group) of this lane.
template <int EA, int EB, class F>
__device__ __forceinline__ void walk_rect(const Rasters& r, int x0, int x1, int y0, int rows, int tid, int team, F&& f) {
    constexpr int P = 16 / EA;
    // a row's groups: group k holds the pixels x0 - mis + k * P .. + P - 1, mis < P the pixels between the 16-byte boundary below the
    // row's first pixel and that pixel; at most cpr groups reach into [x0, x1)
    const int cpr = (int)(((long)(x1 - x0) + 2 * P - 2) / P);
    const int drow = team / cpr, dk = team - drow * cpr;             // (32-bit index divisions: team <= 2048 * 256)
    long row = tid / cpr;
    int k = tid - (int)row * cpr;
    while (row < rows) {
        const long y = y0 + row;
        const unsigned char* rowA = r.a + y * r.rsA * EA;
        const int mis = (int)(((uintptr_t)rowA + (uintptr_t)x0 * EA) & 15u) / EA;
        const long c0l = (long)x0 - mis + (long)k * P;
        if (c0l < x1) {
            const int c0 = (int)c0l;
            f(Group<EA, EB>{rowA, EB ? r.b + y * r.rsB * EB : nullptr, c0, r.W, x0 > c0 ? x0 - c0 : 0, x1 - c0 < P ? x1 - c0 : P});
        }
        row += drow;
        k += dk;
        if (k >= cpr) { k -= cpr; ++row; }
    }
}

// row (xoff, yoff, xcount, ycount) of pos clipped to the raster, in 64 bits so that no content of pos overflows; all zero when nothing
// of the window lies inside
struct Rect {
    bool any;
    int x0, x1, y0, rows;
};
__device__ __forceinline__ Rect clip_window(const int* q, int H, int W) {
    const int xoff = q[0], yoff = q[1], xcount = q[2], ycount = q[3];
    const long long X0 = xoff > 0 ? xoff : 0, Y0 = yoff > 0 ? yoff : 0;
    long long X1 = (long long)xoff + xcount, Y1 = (long long)yoff + ycount;
    X1 = X1 < W ? X1 : W;
    Y1 = Y1 < H ? Y1 : H;
    const bool any = xcount > 0 && ycount > 0 && X1 > X0 && Y1 > Y0;
    return {any, any ? (int)X0 : 0, any ? (int)X1 : 0, any ? (int)Y0 : 0, any ? (int)(Y1 - Y0) : 0};
}

// The team's partials folded into its lane 0: down the wave by a shuffle tree, then the four waves through LDS in wave order.  TEAM: 1 (a
// lane), 64 (a wave), 256 (the workgroup; every lane of it calls).  T: integers with T::down(o), the partials of the lane o below
// (__shfl_down of every member), and T::merge(other).
template <int TEAM, class T>
__device__ __forceinline__ void fold_team(T& v) {
    if (TEAM == 1) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v.merge(v.down(o));
    if (TEAM == 256) {
        __shared__ T red[4];
        const int t = threadIdx.x;
        if ((t & 63) == 0) red[t >> 6] = v;
        __syncthreads();
        if (t == 0) {
#pragma unroll
            for (int w = 1; w < 4; ++w) v.merge(red[w]);
        }
    }
}
#endif

}  // namespace srbh
