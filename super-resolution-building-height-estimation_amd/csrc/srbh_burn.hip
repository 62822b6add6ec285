// srbh_burn.hip -- building footprints burned into a raster: the reference's shp_to_tiff / shp2tif (demo_preprocess_height_v2.py:27-119,
// main_shp2tif) is one gdal.RasterizeLayer(..., options=["ATTRIBUTE=<field>"]) that paints every footprint, in feature order, with its
// attribute value -- the step that makes the training labels and the reference raster of every validation entry.  Here a list of
// features (zones in the sense of srbh_zones.hip, one value each) becomes a uint16 or uint8 raster on the device.
//
// The rule (include/srbh.h states it in full).  Feature f is a zone: all edges of all its rings, int32 fixed point with 8 fractional bits,
// even-odd over its own edges, the pixel centre (x + 1/2, y + 1/2) decides, a centre on a left or top boundary is in, on a right or bottom
// boundary out.  merge "last": out[y][x] = values[f] of the LARGEST f whose zone holds the pixel (a value of 0 burns like any other);
// merge "max": the largest value among the containing features.  A pixel in no feature gets init, or, under keep, is not written.
//
// Why the tile owns the loop.  A city has about a million footprints of a few pixels each, and where they overlap the feature order decides
// the pixel: a workgroup per feature would need global atomics or an owner raster.  So a workgroup of 256 lanes owns a tile of 64 x 64
// output pixels (tiles anchored at pixel (0, 0), the grid is every tile of the raster) and walks the tile's features in ascending index
// from a CSR list (tile_off, tile_feat).  A wave owns 16 rows x 64 columns, a lane 16 consecutive pixels of one row; the lane's 16 values
// and its 16-bit "burned" mask live in registers from the first feature to the store.  No LDS, no barrier, no atomic of any kind.
//   per feature: its pixel box against the wave's rectangle (uniform across the wave);
//   per edge:    its row range and its right extent against the wave's rectangle (uniform), then each lane's crossing test for its row,
//                which XORs a 16-bit toggle mask into the lane's parity;
//   after the feature's last edge: the lane replaces (or maxes) its values under the parity mask.
//
// The crossing test, division free.  Oriented so that den = Y1 - Y0 > 0, with cy = 256 y + 128 and cx = 256 x + 128, an edge that crosses
// row y (Y0 <= cy < Y1) toggles pixel x iff cx < xc = X0 + (cy - Y0)(X1 - X0) / den, that is iff cx den < N, N = X0 den + (cy - Y0)(X1 -
// X0) as in srbh.h.  With cx0 the centre of the lane's first pixel, R = N - cx0 den = (X0 - cx0) den + (cy - Y0)(X1 - X0) and D = 256 den,
// pixel k of the run is toggled iff k D < R: a prefix of the run.  R <= 0 toggles nothing; otherwise the largest such k in 0..15 is found
// by four compares (k = 8, 4, 2, 1 in turn, R stepped down by 8 D, 4 D, 2 D, D) and the mask is the bits 0..k.
// Overflow.  |X|, |Y| <= 2^29 (an edge beyond contributes nothing), so den and |X1 - X0| <= 2^30 and, for a crossing row, 0 <= cy - Y0 <
// den: |(cy - Y0)(X1 - X0)| < 2^60 and |N| < 2^59 + 2^60 < 2^61 as in srbh_zones.hip.  (X0 - cx0) den stays inside int64 only because
// cx0 <= 2^29: a pixel with cx > 2^29 cannot lie in any zone (xc <= 2^29), so the columns x >= 2^21 are out by construction, and a tile
// there (2^21 is a multiple of the tile) walks no feature BEFORE any product is formed.  Then |X0 - cx0| <= 2^30, |R| < 2^61, and 16 D <=
// 2^42: everything fits int64.  A lane whose row the edge does not cross forms its products with cy - Y0 replaced by 0.
//
// The known weak case.  A feature is culled per wave, by its box, never per edge: one large feature of many edges makes every wave of
// every tile in its box walk ALL its edges, one dependent scalar load after the other.  Cost is (tiles its box meets) x (its edges), not
// its pixels: a million footprints of four edges are what this is shaped for, one 1000-vertex zone over half a 12 000 x 16 000 raster
// takes 8.7 ms, three times the stock-torch form.  Per-tile-row edge lists cut on the host would settle it; not built.
//
// Stores.  A lane's 16 pixels go out as aligned 16-byte vector stores (two for uint16, one for uint8; for uint16 a wave writes whole
// 128-byte rows) when the run lies wholly inside the raster, its address is 16-byte aligned and, under keep, all 16 pixels were burned;
// otherwise element by element, each store predicated on x < W && y < H (and, under keep, on the pixel's burned bit).  out is written in
// place through its row stride.
//
// Memory safety.  tile is the caller's blockIdx < NT, and the host checks NT == ceil(H / 64) ceil(W / 64).  tile_off[tile], [tile + 1] are
// used only where 0 <= a <= b <= NF; a feature index only where 0 <= f < Z (boxes, values and edge_off are read at f and f + 1 only then);
// an edge range only where 0 <= a <= b <= E; an edge with a coordinate beyond +-2^29 contributes nothing; boxes are only a filter (they
// are compared, never added to or used as an index).  No table content enters an address of out: a store goes to row y < H and column
// x < W of the lane's own run.  So wrong tables give wrong pixels at worst, never a load outside the tables nor a store outside out's rows
// [0, H) x [0, W).
#include "srbh_internal.h"

namespace {
using namespace srbh;

constexpr int BURN_TILE = 64;                           // the tile side; a wave owns 16 of its rows, a lane 16 pixels of one row
constexpr int COORD_MAX = 1 << 29;
constexpr int X_LIMIT = 1 << 21;                        // cx = 256 x + 128 > 2^29 from this column on

struct BurnParams {
    unsigned char* out;
    long rs;                        // row stride in elements
    int H, W, tiles_x;
    const int4* edges;              // [E] (X0, Y0, X1, Y1)
    const int* edge_off;            // [Z + 1]
    const int* values;              // [Z]
    const int* boxes;               // [Z][4] (x0, y0, x1, y1), half open, pixels
    const int* tile_off;            // [NT + 1]
    const int* tile_feat;           // [NF]
    int Z, E, NF;
    int keep;
    unsigned init;
};

// ES: the element size of out (2: uint16, 1: uint8).  MAX: merge "max" (false: "last").
template <int ES, bool MAX>
__global__ __launch_bounds__(256) void burn_kernel(const BurnParams p) {
    constexpr unsigned VMAX = ES == 2 ? 0xffffu : 0xffu;
    const long tile = blockIdx.x;                                     // < NT
    const long ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    // the wave's rectangle [wx0, wx1) x [wy0, wy1) and the lane's run: the pixels x0 .. x0 + 15 of row y
    const long wx0 = tx * BURN_TILE, wx1 = wx0 + BURN_TILE, wy0 = ty * BURN_TILE + wave * 16, wy1 = wy0 + 16;
    const long x0 = wx0 + (lane & 3) * 16, y = wy0 + (lane >> 2);
    unsigned v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = 0u;
    unsigned burned = 0u;                                             // bit j: pixel j lies in a feature

    int a = p.tile_off[tile], b = p.tile_off[tile + 1];
    if (!(a >= 0 && a <= b && b <= p.NF) || wx0 >= X_LIMIT || wy0 >= p.H) a = b = 0;      // uniform; x >= 2^21: no product is formed
    const long long cy = 256ll * y + 128, cx0 = 256ll * x0 + 128, cxw = 256ll * wx0 + 128;
    for (int i = a; i < b; ++i) {
        const int f = p.tile_feat[i];
        if (f < 0 || f >= p.Z) continue;
        const int* bx = p.boxes + 4 * (long)f;
        if (!(bx[0] < wx1 && bx[2] > wx0 && bx[1] < wy1 && bx[3] > wy0)) continue;        // the feature's box misses the wave's rectangle
        const int e0 = p.edge_off[f], e1 = p.edge_off[f + 1];
        if (!(e0 >= 0 && e0 <= e1 && e1 <= p.E)) continue;
        unsigned par = 0u;
        for (int e = e0; e < e1; ++e) {
            const int4 q = p.edges[e];
            int X0 = q.x, Y0 = q.y, X1 = q.z, Y1 = q.w;
            const bool ok = X0 >= -COORD_MAX && X0 <= COORD_MAX && X1 >= -COORD_MAX && X1 <= COORD_MAX && Y0 >= -COORD_MAX && Y0 <= COORD_MAX &&
                            Y1 >= -COORD_MAX && Y1 <= COORD_MAX;
            if (!ok || Y0 == Y1) continue;
            if (Y0 > Y1) { int s = X0; X0 = X1; X1 = s; s = Y0; Y0 = Y1; Y1 = s; }
            // the rows with Y0 <= 256 y + 128 < Y1 against the wave's rows; an edge wholly at or left of the wave's first centre toggles
            // nothing (an edge wholly RIGHT of the wave toggles every pixel of a crossing row and goes on)
            if (((Y1 + 127) >> 8) <= wy0 || ((Y0 + 127) >> 8) >= wy1) continue;
            if ((X0 > X1 ? X0 : X1) <= cxw) continue;
            const long long den = (long long)Y1 - Y0, dx = (long long)X1 - X0, D = 256 * den;
            const bool cross = cy >= Y0 && cy < Y1;
            long long R = (X0 - cx0) * den + (cross ? cy - Y0 : 0ll) * dx;
            int k = 0;
            const bool any = cross && R > 0;
            if (R > 8 * D) { R -= 8 * D; k += 8; }
            if (R > 4 * D) { R -= 4 * D; k += 4; }
            if (R > 2 * D) { R -= 2 * D; k += 2; }
            if (R > D) k += 1;
            par ^= any ? (2u << k) - 1u : 0u;
        }
        const unsigned val = (unsigned)p.values[f] & VMAX;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if ((par >> j) & 1u) v[j] = MAX ? (v[j] > val ? v[j] : val) : val;
        }
        burned |= par;
    }

    // the store: nx of the run's pixels lie inside the raster's row
    if (y >= p.H || x0 >= p.W) return;
    const int nx = p.W - x0 < 16 ? (int)(p.W - x0) : 16;
    const unsigned write = p.keep ? burned : 0xffffu;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (!((burned >> j) & 1u)) v[j] = p.init;
    }
    unsigned char* dst = p.out + (y * p.rs + x0) * ES;
    if (nx == 16 && ((uintptr_t)dst & 15u) == 0 && write == 0xffffu) {
        if (ES == 2) {
            uint4* o = reinterpret_cast<uint4*>(dst);
            o[0] = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
            o[1] = make_uint4(v[8] | (v[9] << 16), v[10] | (v[11] << 16), v[12] | (v[13] << 16), v[14] | (v[15] << 16));
        } else {
            *reinterpret_cast<uint4*>(dst) = make_uint4(v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24), v[4] | (v[5] << 8) | (v[6] << 16) | (v[7] << 24),
                                                       v[8] | (v[9] << 8) | (v[10] << 16) | (v[11] << 24), v[12] | (v[13] << 8) | (v[14] << 16) | (v[15] << 24));
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j < nx && ((write >> j) & 1u)) {                       // x0 + j < W, y < H
                if (ES == 2) reinterpret_cast<unsigned short*>(dst)[j] = (unsigned short)v[j];
                else dst[j] = (unsigned char)v[j];
            }
        }
    }
}

}  // namespace

extern "C" int srbh_burn_tile(void) { return BURN_TILE; }

extern "C" int srbh_burn(void* out, int typeO, long row_strideO, int H, int W, const int* edges, const int* edge_off, const int* values,
                         const int* boxes, int Z, int E, const int* tile_off, const int* tile_feat, int NT, int NF, int merge, int keep,
                         int init, void* stream) {
    const char* who = "srbh_burn";
    SRBH_REQUIRE(out && edges && edge_off && values && boxes && tile_off && tile_feat, "%s: null pointer", who);
    SRBH_REQUIRE(typeO == SRBH_GRID_U16 || typeO == SRBH_GRID_U8, "%s: type code %d is neither SRBH_GRID_U16 nor SRBH_GRID_U8", who, typeO);
    const int es = typeO == SRBH_GRID_U8 ? 1 : 2;
    SRBH_REQUIRE(H > 0 && W > 0 && Z > 0 && E > 0 && NF >= 0, "%s: H=%d, W=%d, Z=%d and E=%d must be positive, NF=%d not negative", who, H, W, Z, E, NF);
    SRBH_REQUIRE((long)H * W < 0x80000000L, "%s: H * W = %ld must stay below 2^31", who, (long)H * W);
    SRBH_REQUIRE(row_strideO >= W, "%s: the row stride %ld is below W=%d", who, row_strideO, W);
    SRBH_REQUIRE((uintptr_t)out % es == 0, "%s: out is not aligned to its element size", who);
    SRBH_REQUIRE((uintptr_t)edges % 16 == 0 && (uintptr_t)edge_off % 4 == 0 && (uintptr_t)values % 4 == 0 && (uintptr_t)boxes % 4 == 0 &&
                     (uintptr_t)tile_off % 4 == 0 && (uintptr_t)tile_feat % 4 == 0,
                 "%s: edges must be aligned to 16 bytes, the other tables to 4", who);
    const long tiles_x = ((long)W + BURN_TILE - 1) / BURN_TILE, tiles_y = ((long)H + BURN_TILE - 1) / BURN_TILE;
    SRBH_REQUIRE(tiles_x * tiles_y == NT, "%s: NT=%d is not the tile count %ld x %ld of a %d x %d raster", who, NT, tiles_y, tiles_x, H, W);
    SRBH_REQUIRE(merge == SRBH_BURN_LAST || merge == SRBH_BURN_MAX, "%s: merge=%d outside 0..1", who, merge);
    SRBH_REQUIRE(init >= 0 && init <= (es == 2 ? 65535 : 255), "%s: init=%d outside the type's range", who, init);
    BurnParams p;
    p.out = (unsigned char*)out; p.rs = row_strideO; p.H = H; p.W = W; p.tiles_x = (int)tiles_x;
    p.edges = (const int4*)edges; p.edge_off = edge_off; p.values = values; p.boxes = boxes; p.tile_off = tile_off; p.tile_feat = tile_feat;
    p.Z = Z; p.E = E; p.NF = NF; p.keep = keep != 0; p.init = (unsigned)init;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)NT), block(256);
    if (es == 2) {
        if (merge == SRBH_BURN_MAX) hipLaunchKernelGGL((burn_kernel<2, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((burn_kernel<2, false>), grid, block, 0, st, p);
    } else {
        if (merge == SRBH_BURN_MAX) hipLaunchKernelGGL((burn_kernel<1, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((burn_kernel<1, false>), grid, block, 0, st, p);
    }
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
