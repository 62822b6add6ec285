// srbh_disc3.hip -- the discriminator's wide 3x3 / stride 1 / pad 1 convolutions with LeakyReLU (reference SR/rrdbnet_arch.py:265-269 conv4..conv8,
// used at :285-300) on ACT16 planes: srgan.UNetDiscriminatorSN.libsrbh_wide = "f16".
//     y  = lrelu(conv(x, w))                                  srbh_wconv3x3_lrelu: conv_tile<.., WIDE = 1, LR = 1> (srbh_conv3x3_kernel.h)
//     g' = g * (y > 0 ? 1 : 0.2)                              srbh_nhwc32_to_act16_lrelu_bwd: fp32 NHWC g, y -> bf16 planes of g'
//     dx = conv(g', Wt),  Wt[c][o][a][b] = w[o][c][2-a][2-b]  srbh_wconv3x3 (bf16) on the Wt pack of srbh_pack_conv3x3_pair
//     dw[o][c][a][b] = sum_{n,i,j} g'[n][o][i][j] x[n][c][i+a-1][j+b-1]          srbh_wgrad3x3_b16
// The weight gradient is a GEMM over pixels on v_mfma_f32_16x16x32_bf16: a workgroup owns a 64 (o) x 32 (c) x 9 taps block of dw and walks the
// 8 x 64 tiles blockIdx.x, + walkers, ...; each of its four waves owns 16 of the 64 output channels (72 accumulator registers), so the waves never
// meet and one staged tile (32 channels of x with a halo, 64 of g', both channel-major: K of the MFMA is the pixel axis) serves 1152 MFMAs.
// Arithmetic contract: include/srbh.h, DESIGN.md 4.  No atomics anywhere: every result is bit-reproducible.
#include "srbh_act16.h"
#include "srbh_wconv_host.h"

namespace {
using namespace srbh;
using namespace srbh_k;

typedef unsigned uint2w __attribute__((ext_vector_type(2)));
typedef _Float16 half8w __attribute__((ext_vector_type(8)));

// ---- masked gradient staging: fp32 NHWC g and the saved fp32 NHWC forward output y -> chunk planes of rne(g * (y > 0 ? 1 : slope)), the product
// in fp32 (torch's leaky_relu backward rule, srbh_lrelu_bwd_f32's).  One thread per (pixel, 8-channel octet): two 32-byte reads, one 16-byte write.
template <int BF>
__global__ __launch_bounds__(256) void lrelu_bwd_stage_kernel(const float* __restrict__ g, const float* __restrict__ y, char* planes, int B, int C, int H,
                                                              int W, float slope, PlaneGeo geo) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int oct = C / 8;
    if (idx >= (long)B * H * W * oct) return;
    const int o8 = (int)(idx % oct);
    long r = idx / oct;
    const int x = (int)(r % W); r /= W;
    const int yy = (int)(r % H);
    const int b = (int)(r / H);
    const long off = (((long)b * H + yy) * W + x) * C + o8 * 8;
    const floatx4 g0 = *(const floatx4*)(g + off), g1 = *(const floatx4*)(g + off + 4);
    const floatx4 y0 = *(const floatx4*)(y + off), y1 = *(const floatx4*)(y + off + 4);
    float v[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = y0[j] > 0.f ? g0[j] : g0[j] * slope;
        v[4 + j] = y1[j] > 0.f ? g1[j] : g1[j] * slope;
    }
    *(uint4w*)(planes + rec_off(geo, b, o8 >> 2, yy, x, o8 & 3)) = round8<BF>(v);
}

// ---- both packs of one weight in one launch: blockIdx.y = 0 the fp16 WPACK16 of w (cout, cin), 1 the bf16 WPACK16 of Wt (cin, cout).  The layout
// is pack_w_kernel's (srbh_aux.hip; wpack_decode): [chunk][tap][k-step][mb][lane][8]; with both channel counts multiples of 32 the packs have one size.
__global__ __launch_bounds__(256) void pack3x3_pair_kernel(const float* __restrict__ w, unsigned short* __restrict__ wf, unsigned short* __restrict__ wt,
                                                           int cout, int cin, long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int tf = blockIdx.y;
    const WpackElem e = wpack_decode(idx, (tf ? cin : cout) / 32, 9);
    if (tf) wt[idx] = to16(w[((long)e.ic * cin + e.oc) * 9 + (8 - e.tap)], 1);        // Wt[oc][ic][a][b] = w[ic][oc][2-a][2-b]
    else wf[idx] = to16(w[((long)e.oc * cin + e.ic) * 9 + e.tap], 0);
}

// ---- weight gradient --------------------------------------------------------------------------------------------------------------------
// LDS, channel-major, two pixels per dword.  x: 32 channels x 10 rows (image rows Y0-1 .. Y0+8) x 80 positions (image column X at position
// X - X0 + 8, so that a lane's eight pixels are one aligned 16-byte read; columns X0-4 .. X0+67 are staged).  g': 64 channels x 8 rows x 64.
// Channel strides are 4 * odd mod 64 dwords: the sixteen channels of a 16-lane group read 16 distinct 4-dword bank groups.
constexpr int W3_XROWS = TILE_H + 2;
constexpr int W3_XQ = 18;                                  // staged 4-pixel groups per x row
constexpr int W3_RS = 40;                                  // dwords per staged x row (80 positions)
constexpr int W3_SX = W3_XROWS * W3_RS + 4;                // 404 = 20 mod 64
constexpr int W3_SG = TILE_H * 32 + 4;                     // 260 = 4 mod 64
constexpr int W3_XUNITS = W3_XROWS * W3_XQ * 4;            // 720 units of (4 pixels x 8 channels)
constexpr int W3_NIX = (W3_XUNITS + 255) / 256;            // 3 per thread
constexpr int W3_NIG = TILE_H * 16 * 8 / 256;              // 4 per thread
constexpr int W3_LDS_B = (32 * W3_SX + 64 * W3_SG) * 4;    // 118 272 B
constexpr int W3_SLOT = 9 * 64 * 32;                       // floats per workspace slot: [tap][o][c]
static_assert(W3_LDS_B <= 160 * 1024, "LDS of one workgroup");

struct WG3Params {
    const char* x;          // fp16 planes of the forward's input: interior H x W, chunk plane blockIdx.z
    int x_row_b, x_plane_b;
    long x_img_b;
    const char* g;          // bf16 planes of g'
    int g_row_b, g_plane_b;
    long g_img_b;
    int cout;
    int H, W;
    int tiles_x, tiles_per_img, ntiles;
    float* ws;
};

__global__ __launch_bounds__(256) void wgrad3x3_kernel(const WG3Params p) {
    extern __shared__ __attribute__((aligned(16))) unsigned w3_lds[];
    unsigned* s_x = w3_lds;                         // [32 c][W3_SX]
    unsigned* s_g = w3_lds + 32 * W3_SX;            // [64 o][W3_SG]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kb = lane >> 4;
    const int ob = blockIdx.y, cb = blockIdx.z;
    const char* xpl = p.x + (long)cb * p.x_plane_b;
    floatx4 acc[9][2];
#pragma unroll
    for (int tp = 0; tp < 9; ++tp)
#pragma unroll
        for (int h = 0; h < 2; ++h) acc[tp][h] = floatx4{0.f, 0.f, 0.f, 0.f};

    uint4w lx[W3_NIX][4], lg[W3_NIG][4];
    // every staged position is loaded or set to zero: rows and columns outside the planes' zero border are never read
    auto load_tile = [&](const int t) {
        const int img = t / p.tiles_per_img;
        const int trem = t - img * p.tiles_per_img;
        const int ty = trem / p.tiles_x, tx = trem - ty * p.tiles_x;
        const int Y0 = ty * TILE_H, X0 = tx * TILE_W;
#pragma unroll
        for (int it = 0; it < W3_NIX; ++it) {
            const int u = tid + it * 256;
            const int c8 = u & 3, q = u >> 2;
            const int r = q / W3_XQ, qc = q - r * W3_XQ;
            const int y = Y0 - 1 + r, x0 = X0 - 4 + qc * 4;
            const bool rowok = u < W3_XUNITS && y <= p.H;                       // (y >= -1 always)
            const char* src = xpl + (long)img * p.x_img_b + (long)(y + 1) * p.x_row_b + (long)(x0 + 1) * PIX_B + c8 * 16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uint4w a = {0u, 0u, 0u, 0u};
                if (rowok && x0 + i >= -1 && x0 + i <= p.W) a = *(const uint4w*)(src + i * PIX_B);
                lx[it][i] = a;
            }
        }
#pragma unroll
        for (int it = 0; it < W3_NIG; ++it) {
            const int u = tid + it * 256;
            const int c8 = u & 7, q = u >> 3;
            const int y = Y0 + (q >> 4), x0 = X0 + (q & 15) * 4;
            const int och = ob * 64 + c8 * 8;
            const bool rowok = y < p.H && och < p.cout;
            const char* src = p.g + (long)img * p.g_img_b + (long)(och >> 5) * p.g_plane_b + (long)(y + 1) * p.g_row_b + (long)(x0 + 1) * PIX_B + (c8 & 3) * 16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uint4w a = {0u, 0u, 0u, 0u};
                if (rowok && x0 + i < p.W) a = *(const uint4w*)(src + i * PIX_B);
                lg[it][i] = a;
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int it = 0; it < W3_NIX; ++it) {
            const int u = tid + it * 256;
            if (u < W3_XUNITS) {
                const int c8 = u & 3, q = u >> 2;
                const int r = q / W3_XQ, qc = q - r * W3_XQ;
                half8w h[4];                       // fp16 -> fp32 (exact), then bf16 RNE
#pragma unroll
                for (int i = 0; i < 4; ++i) h[i] = __builtin_bit_cast(half8w, lx[it][i]);
                unsigned* o = s_x + (c8 * 8) * W3_SX + r * W3_RS + qc * 2 + 2;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    *(uint2w*)(o + j * W3_SX) = uint2w{bf16x2_rne((float)h[0][j], (float)h[1][j]), bf16x2_rne((float)h[2][j], (float)h[3][j])};
            }
        }
#pragma unroll
        for (int it = 0; it < W3_NIG; ++it) {
            const int u = tid + it * 256;
            const int c8 = u & 7, q = u >> 3;
            unsigned* o = s_g + (c8 * 8) * W3_SG + q * 2;                        // q = row * 16 + group: row * 32 + group * 2 dwords
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const unsigned sel = (j & 1) ? 0x07060302u : 0x05040100u;
                *(uint2w*)(o + j * W3_SG) = uint2w{__builtin_amdgcn_perm(lg[it][1][j >> 1], lg[it][0][j >> 1], sel),
                                                   __builtin_amdgcn_perm(lg[it][3][j >> 1], lg[it][2][j >> 1], sel)};
            }
        }
    };

    int t = blockIdx.x;
    if (t < p.ntiles) load_tile(t);
    for (; t < p.ntiles; t += gridDim.x) {
        __syncthreads();                           // the previous tile's fragment reads are done
        store_tile();
        __syncthreads();
        if (t + (int)gridDim.x < p.ntiles) load_tile(t + gridDim.x);      // in flight under the MFMAs
        // x row xr serves the g' rows xr - dy, dy = 0..2 (tap row dy); a lane's eight pixels and their two neighbour dwords give the three tap columns
        const unsigned* gp = s_g + (wave * 16 + l15) * W3_SG + kb * 4;
        const unsigned* xp = s_x + l15 * W3_SX + 4 + kb * 4;
#pragma unroll
        for (int pg = 0; pg < 2; ++pg) {
            bf16x8 a[TILE_H];
#pragma unroll
            for (int xr = 0; xr < W3_XROWS; ++xr) {
                if (xr < TILE_H) a[xr] = __builtin_bit_cast(bf16x8, *(const uint4w*)(gp + xr * 32 + pg * 16));
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const unsigned* rp = xp + h * 16 * W3_SX + xr * W3_RS + pg * 16;
                    const uint4w cur = *(const uint4w*)rp;
                    const unsigned pv = rp[-1], nx = rp[4];
                    const unsigned m1 = __builtin_amdgcn_alignbit(cur[1], cur[0], 16), m2 = __builtin_amdgcn_alignbit(cur[2], cur[1], 16),
                                   m3 = __builtin_amdgcn_alignbit(cur[3], cur[2], 16);
                    const bf16x8 b0 = __builtin_bit_cast(bf16x8, uint4w{__builtin_amdgcn_alignbit(cur[0], pv, 16), m1, m2, m3});
                    const bf16x8 b1 = __builtin_bit_cast(bf16x8, cur);
                    const bf16x8 b2 = __builtin_bit_cast(bf16x8, uint4w{m1, m2, m3, __builtin_amdgcn_alignbit(nx, cur[3], 16)});
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy) {
                        const int gr = xr - dy;
                        if (gr >= 0 && gr < TILE_H) {
                            acc[dy * 3 + 0][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[gr], b0, acc[dy * 3 + 0][h], 0, 0, 0);
                            acc[dy * 3 + 1][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[gr], b1, acc[dy * 3 + 1][h], 0, 0, 0);
                            acc[dy * 3 + 2][h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[gr], b2, acc[dy * 3 + 2][h], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }
    // flush: D[row = o = kb * 4 + r][col = c = l15] of each (tap, half) to the workgroup's slot [tap][o][c]; a workgroup without a tile writes zeros
    float* out = p.ws + (((long)blockIdx.x * gridDim.y + ob) * gridDim.z + cb) * W3_SLOT;
#pragma unroll
    for (int tp = 0; tp < 9; ++tp)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[tp * 2048 + (wave * 16 + kb * 4 + r) * 32 + h * 16 + l15] = acc[tp][h][r];
}

// dw[o][c][a][b] = the slots' sums in the order of the walkers
__global__ __launch_bounds__(256) void wgrad3x3_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int O, int C, int nwalk) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)O * C * 9) return;
    const int tap = (int)(idx % 9);
    const long oc = idx / 9;
    const int c = (int)(oc % C), o = (int)(oc / C);
    const int nob = (O + 63) / 64, ncb = C / 32;
    float s = 0.f;
    for (int w = 0; w < nwalk; ++w) s += ws[(((long)w * nob + (o >> 6)) * ncb + (c >> 5)) * W3_SLOT + tap * 2048 + (o & 63) * 32 + (c & 31)];
    dw[idx] = s;
}

int g_walkers_cap = 0;      // srbh_wgrad3x3_walkers_cap: 0 = the default

// walkers of the weight gradient: one workgroup per CU of the device's 256 over all blocks, never more than tiles
inline int wgrad3_walkers(int cout, int cin, int B, int H, int W) {
    const long ntiles = (long)((W + TILE_W - 1) / TILE_W) * ((H + TILE_H - 1) / TILE_H) * B;
    const long blocks = (long)((cout + 63) / 64) * (cin / 32);
    long n = 256 / blocks;
    if (n < 1) n = 1;
    if (g_walkers_cap > 0 && n > g_walkers_cap) n = g_walkers_cap;
    return (int)(n < ntiles ? n : ntiles);
}
inline bool wgrad3_shape_ok(int cout, int cin, int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 && cin > 0 && (cin & 31) == 0 && (cout == 32 || (cout >= 64 && cout % 64 == 0)) && cout / 64 <= 65535 && cin / 32 <= 65535;
}

}  // namespace

// the wide 3x3 conv with the forward LeakyReLU(0.2) in its epilogue: no bias / relu / mask16 / add16
extern "C" int srbh_wconv3x3_lrelu(const srbh_wconv3x3_args* a, void* stream) {
    static constexpr WideForm form = {"srbh_wconv3x3_lrelu", 3, 0, true, false, true, false};
    if (const int rc = wide_validate(a, form)) return rc;
    const WKParams p = wide_params(a, form);
    return with_const<2>(a->bf16 != 0, [&](auto bf) {
        constexpr int BF = decltype(bf)::value;
        return a->cout == 32 ? launch<wconv3x3_lrelu_kernel<1, BF>, true>(dim3(p.nblocks), lds_bytes<1, 0>(), (hipStream_t)stream, p)
                             : launch<wconv3x3_lrelu_kernel<2, BF>, true>(dim3(p.nblocks), lds_bytes<2, 0>(), (hipStream_t)stream, p);
    });
}

extern "C" int srbh_nhwc32_to_act16_lrelu_bwd(const float* g, const float* y, void* planes, int B, int C, int H, int W, float slope, int bf16, void* stream) {
    SRBH_REQUIRE(g && y && planes, "srbh_nhwc32_to_act16_lrelu_bwd: null pointer");
    SRBH_REQUIRE(B > 0 && C > 0 && (C & 31) == 0, "srbh_nhwc32_to_act16_lrelu_bwd: C must be a positive multiple of 32 (got B=%d C=%d)", B, C);
    SRBH_REQUIRE(H > 0 && W > 0, "srbh_nhwc32_to_act16_lrelu_bwd: bad geometry %dx%d", H, W);
    const long total = (long)B * H * W * (C / 8);
    SRBH_REQUIRE(fits(total), "srbh_nhwc32_to_act16_lrelu_bwd: too large");
    const PlaneGeo ge = plane_geo(B, C / 32, H, W);
    if (bf16) hipLaunchKernelGGL(lrelu_bwd_stage_kernel<1>, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, g, y, (char*)planes, B, C, H, W, slope, ge);
    else hipLaunchKernelGGL(lrelu_bwd_stage_kernel<0>, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, g, y, (char*)planes, B, C, H, W, slope, ge);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_pack_conv3x3_pair(const float* w, int cout, int cin, void* w_f16, void* wt_b16, void* stream) {
    SRBH_REQUIRE(w && w_f16 && wt_b16, "srbh_pack_conv3x3_pair: null pointer");
    SRBH_REQUIRE(cout > 0 && cin > 0 && (cout & 31) == 0 && (cin & 31) == 0,
                 "srbh_pack_conv3x3_pair: cout and cin must be positive multiples of 32 (got cout=%d cin=%d)", cout, cin);
    const long total = (long)(cin / 32) * 18 * (cout / 32) * 512;
    SRBH_REQUIRE(fits(total), "srbh_pack_conv3x3_pair: too large");
    hipLaunchKernelGGL(pack3x3_pair_kernel, dim3(blocks_of(total), 2), dim3(256), 0, (hipStream_t)stream, w, (unsigned short*)w_f16, (unsigned short*)wt_b16,
                       cout, cin, total);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_wgrad3x3_walkers_cap(int cap) {
    const int prev = g_walkers_cap;
    g_walkers_cap = cap > 0 ? cap : 0;
    return prev;
}

extern "C" size_t srbh_wgrad3x3_ws_bytes(int cout, int cin, int B, int H, int W) {
    if (!wgrad3_shape_ok(cout, cin, B, H, W)) return 0;
    return (size_t)wgrad3_walkers(cout, cin, B, H, W) * ((cout + 63) / 64) * (cin / 32) * W3_SLOT * sizeof(float);
}

extern "C" int srbh_wgrad3x3_b16(const void* x_planes, int x_chunks_total, int cin, const void* g_planes, int g_chunks_total, int cout, int B, int H, int W,
                                 float* dw, void* ws, void* stream) {
    SRBH_REQUIRE(x_planes && g_planes && dw && ws, "srbh_wgrad3x3_b16: null pointer");
    SRBH_REQUIRE(cin > 0 && (cin & 31) == 0, "srbh_wgrad3x3_b16: cin must be a positive multiple of 32 (got %d)", cin);
    SRBH_REQUIRE(cout == 32 || (cout >= 64 && cout % 64 == 0), "srbh_wgrad3x3_b16: cout must be 32 or a multiple of 64 (got %d)", cout);
    SRBH_REQUIRE(wgrad3_shape_ok(cout, cin, B, H, W), "srbh_wgrad3x3_b16: bad geometry B=%d H=%d W=%d cout=%d cin=%d", B, H, W, cout, cin);
    SRBH_REQUIRE(cin / 32 <= x_chunks_total && cout / 32 <= g_chunks_total, "srbh_wgrad3x3_b16: channel ranges outside the plane buffers (%d of %d, %d of %d planes)",
                 cin / 32, x_chunks_total, cout / 32, g_chunks_total);
    const Act16Geo gx = act16_geo(B, x_chunks_total, H, W), gg = act16_geo(B, g_chunks_total, H, W);
    WG3Params p;
    p.x = (const char*)x_planes; p.x_row_b = gx.row_b; p.x_plane_b = gx.plane_b; p.x_img_b = gx.img_b;
    p.g = (const char*)g_planes; p.g_row_b = gg.row_b; p.g_plane_b = gg.plane_b; p.g_img_b = gg.img_b;
    p.cout = cout;
    p.H = H;
    p.W = W;
    p.tiles_x = (W + TILE_W - 1) / TILE_W;
    p.tiles_per_img = p.tiles_x * ((H + TILE_H - 1) / TILE_H);
    const long ntiles = (long)p.tiles_per_img * B;
    SRBH_REQUIRE(ntiles < (1l << 30), "srbh_wgrad3x3_b16: too many tiles");
    p.ntiles = (int)ntiles;
    p.ws = (float*)ws;
    const int nwalk = wgrad3_walkers(cout, cin, B, H, W);
    SRBH_ONCE_PER_DEVICE(SRBH_HIP(hipFuncSetAttribute((const void*)wgrad3x3_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, W3_LDS_B)));
    hipLaunchKernelGGL(wgrad3x3_kernel, dim3(nwalk, (cout + 63) / 64, cin / 32), dim3(256), W3_LDS_B, (hipStream_t)stream, p);
    SRBH_HIP(hipGetLastError());
    const long total = (long)cout * cin * 9;
    hipLaunchKernelGGL(wgrad3x3_reduce_kernel, dim3(blocks_of(total)), dim3(256), 0, (hipStream_t)stream, (const float*)ws, dw, cout, cin, nwalk);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
