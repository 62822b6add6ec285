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
// of the cache.  A row of the window is cut into groups of P = 16 / sizeof(element of a) pixels that start on 16-byte boundaries of a's
// ADDRESS: xoff = k * 56, an odd W and a cropped view give every row its own alignment, so the group grid is computed per row, from
// the address of the row's first window pixel.  A lane takes one (row, group) at a time:
//   * a group whose P pixels all lie inside the raster's row [0, W) is fetched by one aligned 16-byte load and the pixels outside the
//     window [x0, x1) are masked off -- the head and the tail of a window row read raster pixels next to the window, never anything else;
//   * any other group (it would start before the row's first byte or end behind its last) is fetched pixel by pixel, each load predicated
//     on the window, which by then is clipped to the raster.
// So no load touches a byte outside the rows' own bytes of the raster, whatever pos holds.  The same P pixels of b are fetched by the same
// rule; b has its own element size, stride and alignment, so its wide load is one of element alignment only.
// A lane turns a group into two bit masks and counts them (popcount) into three int32 partials -- a window holds fewer than 2^31 pixels --,
// the 64 lanes of a wave are folded by a shuffle tree and the four waves through LDS.  No atomics, no workspace; lane 0 writes the four
// int64 results.
#include "srbh_internal.h"

namespace {
using namespace srbh;

struct CellParams {
    const unsigned char* a;
    const unsigned char* b;         // NULL: one raster
    long rsA, rsB;                  // row strides in elements
    int H, W;
    const int* pos;                 // [N][4] on the device
    int thr;
    unsigned vmaskA, sxA;           // f(v) = ((v & vmask) ^ sx) - sx: vmask cuts to eight bits (wrap8), sx = 0x8000 sign-extends int16
    unsigned vmaskB, sxB;
    long long* out;                 // [N][4]
};

// bit j: pixel c0 + j of the row at `row` (its pixel 0) lies in the window [x0, x1) and f(value) > thr.  [x0, x1) lies inside [0, W).
// ALIGNED: row + c0 * E is a 16-byte boundary whenever the wide load is taken (P * E == 16).
template <int E, int P, bool ALIGNED>
__device__ __forceinline__ unsigned group_bits(const unsigned char* row, int c0, int W, int x0, int x1, unsigned vmask, unsigned sx,
                                               int thr) {
    constexpr int WORDS = P * E / 4;
    const int lo = x0 > c0 ? x0 - c0 : 0, hi = x1 - c0 < P ? x1 - c0 : P;      // the window's pixels of this group: [lo, hi), hi > lo
    unsigned bits = 0;
    if (c0 >= 0 && c0 <= W - P) {
        unsigned w[WORDS];
        const unsigned char* src = row + (long)c0 * E;
        if (ALIGNED) {
            const uint4 q = *reinterpret_cast<const uint4*>(src);
            w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else {
            __builtin_memcpy(w, __builtin_assume_aligned(src, E), sizeof w);
        }
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const unsigned raw = E == 1 ? (w[j >> 2] >> (8 * (j & 3))) & 0xffu : (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
            const int v = (int)((raw & vmask) ^ sx) - (int)sx;
            bits |= (v > thr ? 1u : 0u) << j;
        }
        bits &= ((1u << (hi - lo)) - 1u) << lo;
    } else {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            if (j >= lo && j < hi) {
                const unsigned raw = E == 1 ? (unsigned)row[c0 + j] : (unsigned)reinterpret_cast<const unsigned short*>(row)[c0 + j];
                const int v = (int)((raw & vmask) ^ sx) - (int)sx;
                bits |= (v > thr ? 1u : 0u) << j;
            }
        }
    }
    return bits;
}

// EA, EB: element sizes of a and b in bytes (EB == 0: no b)
template <int EA, int EB>
__global__ __launch_bounds__(256) void cell_counts_kernel(const CellParams p) {
    constexpr int P = 16 / EA;
    __shared__ int red[3][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int* q = p.pos + 4 * (long)blockIdx.x;
    const int xoff = q[0], yoff = q[1], xcount = q[2], ycount = q[3];
    // the window clipped to the raster, in 64 bits so that no content of pos overflows
    const long long X0 = xoff > 0 ? xoff : 0, Y0 = yoff > 0 ? yoff : 0;
    long long X1 = (long long)xoff + xcount, Y1 = (long long)yoff + ycount;
    X1 = X1 < p.W ? X1 : p.W;
    Y1 = Y1 < p.H ? Y1 : p.H;
    const bool any = xcount > 0 && ycount > 0 && X1 > X0 && Y1 > Y0;
    const int x0 = any ? (int)X0 : 0, x1 = any ? (int)X1 : 0, y0 = any ? (int)Y0 : 0, rows = any ? (int)(Y1 - Y0) : 0;
    const int w = x1 - x0;
    int na = 0, nb = 0, nand = 0;
    if (any) {                                                        // uniform
        // a row's groups: group k holds the pixels x0 - mis + k * P .. + P - 1, mis < P the pixels between the 16-byte boundary below the
        // row's first window pixel and that pixel; at most cpr groups reach into [x0, x1)
        const int cpr = (int)(((long)w + 2 * P - 2) / P);
        const int drow = 256 / cpr, dk = 256 % cpr;
        long row = t / cpr;
        int k = t - (int)row * cpr;
        while (row < rows) {
            const long y = y0 + row;
            const unsigned char* rowA = p.a + y * p.rsA * EA;
            const int mis = (int)(((uintptr_t)rowA + (uintptr_t)x0 * EA) & 15u) / EA;
            const long c0l = (long)x0 - mis + (long)k * P;
            if (c0l < x1) {
                const int c0 = (int)c0l;
                const unsigned ma = group_bits<EA, P, true>(rowA, c0, p.W, x0, x1, p.vmaskA, p.sxA, p.thr);
                na += __popc(ma);
                if (EB) {
                    const unsigned char* rowB = p.b + y * p.rsB * (EB ? EB : 1);
                    const unsigned mb = group_bits<(EB ? EB : 1), P, false>(rowB, c0, p.W, x0, x1, p.vmaskB, p.sxB, p.thr);
                    nb += __popc(mb);
                    nand += __popc(ma & mb);
                }
            }
            row += drow;
            k += dk;
            if (k >= cpr) { k -= cpr; ++row; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        na += __shfl_down(na, o, 64);
        if (EB) { nb += __shfl_down(nb, o, 64); nand += __shfl_down(nand, o, 64); }
    }
    if (lane == 0) { red[0][wave] = na; red[1][wave] = nb; red[2][wave] = nand; }
    __syncthreads();
    if (t == 0) {
        long long* o = p.out + 4 * (long)blockIdx.x;
        o[0] = (long long)(((red[0][0] + red[0][1]) + red[0][2]) + red[0][3]);
        o[1] = (long long)(((red[1][0] + red[1][1]) + red[1][2]) + red[1][3]);
        o[2] = (long long)(((red[2][0] + red[2][1]) + red[2][2]) + red[2][3]);
        o[3] = (long long)w * rows;
    }
}

inline bool cell_type_ok(int type) { return type == SRBH_GRID_U16 || type == SRBH_GRID_I16 || type == SRBH_GRID_U8; }
inline int cell_esz(int type) { return type == SRBH_GRID_U8 ? 1 : 2; }
inline void cell_value_map(int type, int wrap8, unsigned* vmask, unsigned* sx) {
    *vmask = (wrap8 || type == SRBH_GRID_U8) ? 0xffu : 0xffffu;
    *sx = (!wrap8 && type == SRBH_GRID_I16) ? 0x8000u : 0u;
}

}  // namespace

extern "C" int srbh_cell_counts(const void* a, int typeA, long row_strideA, const void* b, int typeB, long row_strideB, int H, int W,
                                const int* pos, int N, int thr, int wrap8, long long* out, void* stream) {
    SRBH_REQUIRE(a && pos && out, "srbh_cell_counts: null pointer");
    SRBH_REQUIRE(typeA != SRBH_GRID_F32 && (!b || typeB != SRBH_GRID_F32),
                 "srbh_cell_counts: float32 rasters are refused (the reference's cast of a float to uint8 is not defined outside 0..255)");
    SRBH_REQUIRE(cell_type_ok(typeA) && (!b || cell_type_ok(typeB)),
                 "srbh_cell_counts: unknown element type typeA=%d typeB=%d (1 uint16, 2 int16, 3 uint8)", typeA, typeB);
    SRBH_REQUIRE(N > 0 && H > 0 && W > 0, "srbh_cell_counts: bad geometry N=%d H=%d W=%d", N, H, W);
    SRBH_REQUIRE(row_strideA >= W && (!b || row_strideB >= W), "srbh_cell_counts: a row stride (%ld, %ld) is below W=%d", row_strideA,
                 b ? row_strideB : row_strideA, W);
    // a window's counts are formed in 32 bits; the windows live on the device, so the raster bounds them
    SRBH_REQUIRE((long)H * W < 0x80000000L, "srbh_cell_counts: H * W = %ld must stay below 2^31", (long)H * W);
    SRBH_REQUIRE(thr >= -32768 && thr <= 65535, "srbh_cell_counts: thr=%d outside -32768..65535", thr);
    SRBH_REQUIRE(wrap8 == 0 || wrap8 == 1, "srbh_cell_counts: wrap8=%d must be 0 or 1", wrap8);
    const int ea = cell_esz(typeA), eb = b ? cell_esz(typeB) : 0;
    SRBH_REQUIRE((uintptr_t)a % ea == 0 && (!b || (uintptr_t)b % eb == 0), "srbh_cell_counts: a raster is not aligned to its element size");
    CellParams p;
    p.a = (const unsigned char*)a; p.b = (const unsigned char*)b;
    p.rsA = row_strideA; p.rsB = b ? row_strideB : 0;
    p.H = H; p.W = W; p.pos = pos; p.thr = thr; p.out = out;
    cell_value_map(typeA, wrap8, &p.vmaskA, &p.sxA);
    cell_value_map(b ? typeB : typeA, wrap8, &p.vmaskB, &p.sxB);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)N), block(256);
    if (ea == 1) {
        if (eb == 0) hipLaunchKernelGGL((cell_counts_kernel<1, 0>), grid, block, 0, st, p);
        else if (eb == 1) hipLaunchKernelGGL((cell_counts_kernel<1, 1>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((cell_counts_kernel<1, 2>), grid, block, 0, st, p);
    } else {
        if (eb == 0) hipLaunchKernelGGL((cell_counts_kernel<2, 0>), grid, block, 0, st, p);
        else if (eb == 1) hipLaunchKernelGGL((cell_counts_kernel<2, 1>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((cell_counts_kernel<2, 2>), grid, block, 0, st, p);
    }
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
