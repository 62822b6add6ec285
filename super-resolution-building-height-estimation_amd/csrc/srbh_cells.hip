// srbh_cells.hip -- which cells of a city's grid are predicted at all, and how two footprint rasters agree cell by cell (reference
// demo_preprocess_height_v2.py: Fishgrid_stats :1143-1186 counts the World-Settlement-Footprint pixels > 0 of every grid cell,
// compare_twotiff_valid / compare_twotiff_valid_iou :740-933 count the pixels of a second raster, the differing pixels and the
// intersection over union; one shapefile feature and two GDAL window reads at a time there, every window of a city in one launch here).
//
// srbh_cell_counts: per window (xoff, yoff, xcount, ycount) the four integers [n_a, n_b, n_and, count]: the window's pixels inside the
// raster, and of those the ones with f(a) > thr, with f(b) > thr and with both.  f is the identity, or the value's low eight bits as an
// unsigned number (wrap8: the reference casts to uint8 BEFORE it compares, so uint16 256 counts as 0 and int16 -1 as 255).  Integers
// only: the result is exact and has no order.
//
// Form: ONE workgroup of 256 lanes per window; windows overlap (offset 56 under window 64), so neighbours re-read each other's rows out
// of the cache.  The window is clipped to the raster and walked in 16-byte groups of a's address (srbh_raster_walk.h: the walk, and why
// no load leaves a raster whatever pos holds).  A lane turns a group into two bit masks and counts them (popcount) into three int32
// partials -- a window holds fewer than 2^31 pixels --, which the workgroup folds.  No atomics, no workspace; lane 0 writes the four
// int64 results.
#include "srbh_raster_walk.h"

namespace {
using namespace srbh;

struct CellParams {
    Rasters r;
    const int* pos;                 // [N][4] on the device
    int thr;
    unsigned vmaskA, sxA;           // f(v) = ((v & vmask) ^ sx) - sx: vmask cuts to eight bits (wrap8), sx = 0x8000 sign-extends int16
    unsigned vmaskB, sxB;
    long long* out;                 // [N][4]
};

struct Counts {
    int a, b, both;
    __device__ __forceinline__ Counts down(int o) const { return {__shfl_down(a, o, 64), __shfl_down(b, o, 64), __shfl_down(both, o, 64)}; }
    __device__ __forceinline__ void merge(const Counts& o) { a += o.a; b += o.b; both += o.both; }
};

// bit j: f(pixel j) > thr, for the P pixels of E bytes in the words w
template <int E, int P>
__device__ __forceinline__ unsigned over_bits(const unsigned* w, unsigned vmask, unsigned sx, int thr) {
    unsigned bits = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int v = (int)((group_pixel<E>(w, j) & vmask) ^ sx) - (int)sx;
        bits |= (v > thr ? 1u : 0u) << j;
    }
    return bits;
}

// EA, EB: element sizes of a and b in bytes (EB == 0: no b)
template <int EA, int EB>
__global__ __launch_bounds__(256) void cell_counts_kernel(const CellParams p) {
    using G = Group<EA, EB>;
    constexpr int P = G::P;
    const Rect w = clip_window(p.pos + 4 * (long)blockIdx.x, p.r.H, p.r.W);
    Counts n = {0, 0, 0};
    if (w.any)                                                        // uniform
        walk_rect<EA, EB>(p.r, w.x0, w.x1, w.y0, w.rows, threadIdx.x, 256, [&](const G& g) {
            unsigned wa[G::WORDS_A];
            g.load_a(wa);
            const unsigned ma = over_bits<EA, P>(wa, p.vmaskA, p.sxA, p.thr) & g.inside();
            n.a += __popc(ma);
            if (EB) {
                unsigned wb[G::WORDS_B];
                g.load_b(wb);
                const unsigned mb = over_bits<G::EBB, P>(wb, p.vmaskB, p.sxB, p.thr) & g.inside();
                n.b += __popc(mb);
                n.both += __popc(ma & mb);
            }
        });
    fold_team<256>(n);
    if (threadIdx.x == 0) {
        long long* o = p.out + 4 * (long)blockIdx.x;
        o[0] = n.a;
        o[1] = n.b;
        o[2] = n.both;
        o[3] = (long long)(w.x1 - w.x0) * w.rows;
    }
}

inline bool cell_type_ok(int type) { return type == SRBH_GRID_U16 || type == SRBH_GRID_I16 || type == SRBH_GRID_U8; }
inline void cell_value_map(int type, int wrap8, unsigned* vmask, unsigned* sx) {
    *vmask = (wrap8 || type == SRBH_GRID_U8) ? 0xffu : 0xffffu;
    *sx = (!wrap8 && type == SRBH_GRID_I16) ? 0x8000u : 0u;
}

}  // namespace

extern "C" int srbh_cell_counts(const void* a, int typeA, long row_strideA, const void* b, int typeB, long row_strideB, int H, int W,
                                const int* pos, int N, int thr, int wrap8, long long* out, void* stream) {
    SRBH_REQUIRE(pos && out, "srbh_cell_counts: null pointer");
    SRBH_REQUIRE(N > 0, "srbh_cell_counts: N=%d must be positive", N);
    SRBH_REQUIRE(typeA != SRBH_GRID_F32 && (!b || typeB != SRBH_GRID_F32),
                 "srbh_cell_counts: float32 rasters are refused (the reference's cast of a float to uint8 is not defined outside 0..255)");
    SRBH_REQUIRE(cell_type_ok(typeA) && (!b || cell_type_ok(typeB)),
                 "srbh_cell_counts: unknown element type typeA=%d typeB=%d (1 uint16, 2 int16, 3 uint8)", typeA, typeB);
    SRBH_REQUIRE(thr >= -32768 && thr <= 65535, "srbh_cell_counts: thr=%d outside -32768..65535", thr);
    SRBH_REQUIRE(wrap8 == 0 || wrap8 == 1, "srbh_cell_counts: wrap8=%d must be 0 or 1", wrap8);
    CellParams p;
    const int rc = rasters_checked("srbh_cell_counts", a, typeA, row_strideA, b, typeB, row_strideB, H, W, &p.r);
    if (rc != SRBH_OK) return rc;
    p.pos = pos; p.thr = thr; p.out = out;
    cell_value_map(typeA, wrap8, &p.vmaskA, &p.sxA);
    cell_value_map(b ? typeB : typeA, wrap8, &p.vmaskB, &p.sxB);
    with_sizes(typeA, b, typeB, [&](auto ea, auto eb) {
        hipLaunchKernelGGL((cell_counts_kernel<decltype(ea)::value, decltype(eb)::value>), dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, p);
    });
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
