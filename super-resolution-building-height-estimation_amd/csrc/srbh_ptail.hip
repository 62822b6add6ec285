// srbh_ptail.hip -- persistent form of the 64 -> 64 channel 3x3 convs at up-sampled resolution
// (conv_up1 / conv_up2 behind the nearest-x2 read, conv_hr, conv_last's producer; reference SR/rrdbnet_arch.py:
// 234-239): 1 024 - 4 096 output tiles per launch, i.e. 4 - 16 per CU.
//
// The per-launch kernel (srbh_conv3x3_kernel.h) runs one tile per workgroup and one workgroup per CU (160 KiB LDS), so
// every tile pays a cold staging latency and its epilogue stores with idle matrix cores.  Here a workgroup walks a
// contiguous range of tiles:
//   * the two 36 KiB weight chunks are loaded ONCE per workgroup and stay resident (K = 64 input channels only);
//   * both input chunks of a tile are resident too, so the 288 MFMAs per wave of a tile run without any barrier or DMA (general form; the
//     full-tile forms below issue the next tile's input DMA among them);
//   * the epilogue stores straight from the MFMA D layout (v_permlane32_swap -> 16 B per lane, no LDS), which leaves
//     LDS free: the input tiles of the NEXT tile are DMA'd while the epilogue of the current one drains.
// Same arithmetic, same accumulation order as conv3x3_f16_kernel<2, UPS> (bit-identical results).
// (Round 6: the three phases of a tile run one after the other here -- ablation builds, profiles/r06ag_ptail_ablation.txt: of the 0.34 ms the
//  three tail convs take per 32 tiles the MFMAs are 0.11, the epilogue (800 VALU instructions + 48 KB of stores per wave) 0.12, the exposed part
//  of the input DMA 0.045.  A fully pipelined form was built: two accumulator sets, the epilogue of tile t - 1 interleaved unit by unit with the
//  MFMA groups of tile t's second chunk in one basic block, the input chunks requested half a tile ahead, counted waits; bit-identical, 45 tests.
//  It is 0.4 % faster on forward_feature and 0.6 % slower in the tiled prediction (profiles/r06ah_ab_ptail_pipe.txt): with the phases
//  overlapped the launch draws more power at once and the package clocks down -- the tail convs are energy-bound like the trunk,
//  not latency-bound.  Not kept.)
//
// Kernel forms (profiles/ptail_forms_*): ptail_kernel<UPS, LRELU, OUT, FULL>.  The general form <UPS, LRELU_RT, OUT_RT, 0> is the
// body described above, with LeakyReLU, both outputs and the store predicate as run-time values: per tile and wave 128 v_accvgpr_read, 64 packed
// adds, 64 packed multiplies, 128 compares + 128 selects, 64 fp16 conversions, 32 half-wave swaps and 48 stores, each under its own EXEC
// save / branch -- about 700 instructions behind the 288 MFMAs.  It serves ragged shapes and launches with both outputs.  Whole tiles
// (H % 8 == 0, W % 64 == 0) with ONE output take a full-tile form, which executes per tile and wave only what its conv needs:
//   conv_up1 / conv_up2 <1, 1, OUT_16, 1>: 128 reads, 64 packed adds, 64 packed multiplies + 128 v_max_f32 (LeakyReLU as max(v, 0.2 v)),
//                                          64 conversions, 32 swaps, 16 unpredicated stores;
//   conv_hr, fp32       <0, 0, OUT_32, 1>: 128 reads, 64 packed adds, 32 unpredicated stores in line order (four pointers, constant offsets);
//   conv_hr, NHWC16 / planes + LeakyReLU   <0, 0 / 1, OUT_16, 1>: as conv_up without / with the LeakyReLU.
// These forms also ask for the next tile's inputs earlier (see LDS_B below).  Same products, accumulation order and roundings in every form:
// bit-identical to each other and to the per-tile kernel (tests/test_gpu_ptail_forms.py); srbh_ptail_form_counts says which form a launch took.
#include "srbh_ptail_kernel.h"

namespace {
using namespace srbh;
using namespace srbh_k;

struct TParams {
    In16 in;                    // first input plane
    const char* w;              // WPACK16, 2 chunks x 36 KiB
    const float* bias;
    int H, W;                   // OUTPUT geometry
    int tiles_x, tiles_per_img, ntiles, tiles_per_wg;
    int lrelu;
    Out16 out16;                // ACT16 (2 planes) or NHWC16 output, or none
    float* out32;               // fp32 NHWC (64 channels) output or nullptr
};

// Epilogue forms (compile-time).  LRELU: 0 / 1, or LRELU_RT = p.lrelu at run time.  OUT: OUT_16 = 16-bit records only (ACT16 planes or NHWC16),
// OUT_32 = fp32 NHWC only, OUT_RT = whichever of p.out16 / p.out32 is set, both included.  FULL: H % 8 == 0 && W % 64 == 0, so every tile is
// whole and no store is predicated.  <UPS, LRELU_RT, OUT_RT, 0> is the general form; the FULL forms exist for LRELU 0 / 1 x OUT_16 / OUT_32.
constexpr int LRELU_RT = 2, OUT_16 = 1, OUT_32 = 2, OUT_RT = 3;
// The FULL forms also request the next tile's inputs earlier than the general form (which asks for both chunks behind the tile's last MFMA):
//   UPS = 1: an input chunk is 13 KiB, so a second pair of input areas fits (72 + 4 x 13 KiB) and tile t + 1 is requested at the top of tile t;
//   UPS = 0: LDS is full (72 + 2 x 41.25 KiB): chunk 0 of tile t + 1 is requested behind the chunk-0 MFMAs of tile t, chunk 1 behind the last MFMA.
template <int UPS, int FULL>
constexpr int LDS_B = TAIL_LDS_B<UPS> + (FULL && UPS ? 2 * TileGeo<UPS>::UNITS * 16 : 0);

template <int UPS, int LRELU, int OUT, int FULL>
__global__ __launch_bounds__(256, 1) void ptail_kernel(const TParams p) {
    static_assert(FULL ? (LRELU != LRELU_RT && OUT != OUT_RT) : (LRELU == LRELU_RT && OUT == OUT_RT), "one general form, the rest full-tile forms");
    using G = TileGeo<UPS>;
    constexpr int IN_EX = G::UNITS * 16;   // exact input tile bytes (tail lanes of the last DMA instruction are masked)
    constexpr int CB = 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [weights 72 KiB][input chunk 0][input chunk 1] ([chunk 0][chunk 1] once more: FULL && UPS)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;

    int goff[G::NJ];
#pragma unroll
    for (int j = 0; j < G::NJ; ++j) {
        const int u0 = j * 256 + tid;
        const int u = u0 < G::UNITS ? u0 : 0;
        const int trow = u / (G::COLS * 4);
        const int rem = u - trow * (G::COLS * 4);
        const int pc = rem >> 2, ps = rem & 3;
        goff[j] = trow * p.in.row_b + pc * PIX_B + ((ps ^ ((pc >> 2) & 3)) << 4);
    }
    const unsigned long long tail_mask = __builtin_amdgcn_ballot_w64((G::NJ - 1) * 256 + tid < G::UNITS);
    int aoff[3][2];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
        const int pc = UPS ? (((wc * 32 + l31 + dx - 1) >> 1) + 1) : (wc * 32 + l31 + dx);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            aoff[dx][ks] = wr * (UPS ? 2 : 4) * G::ROW_B + pc * PIX_B + (((ks * 2 + hi) ^ ((pc >> 2) & 3)) << 4);
    }

    auto stage_chunk = [&](int t, int c, int buf) {
        int img, Y0, X0;
        tile_origin(t, p.tiles_per_img, p.tiles_x, img, Y0, X0);
        const char* src0 = p.in.base + (long)img * p.in.img_b + (long)(UPS ? (Y0 >> 1) : Y0) * p.in.row_b + (UPS ? (X0 >> 1) : X0) * PIX_B;
#pragma unroll
        for (int j = 0; j < G::NJ; ++j)
            dma16(src0 + (long)c * p.in.plane_b + goff[j], TAIL_W_B + (buf * 2 + c) * IN_EX + (j * 256 + wave * 64) * 16,
                  j < G::NJ - 1 ? ~0ull : tail_mask);
    };
    auto stage_inputs = [&](int t, int buf = 0) {
        stage_chunk(t, 0, buf);
        stage_chunk(t, 1, buf);
    };

    // epilogue stores per wave and tile when every tile is full (no store predicated off): see the wait at the top of the tile loop.  A FULL
    // form issues exactly its own: 4 rows x 2 channel blocks x 4 groups = 32 (fp32 output) or 4 rows x 2 blocks x 2 group pairs = 16 (16-bit)
    const int nst = FULL ? (OUT == OUT_32 ? 32 : 16)
                         : ((p.H & (TILE_H - 1)) == 0 && (p.W & (TILE_W - 1)) == 0) ? (p.out32 ? 32 : 0) + (p.out16.base ? 16 : 0) : 0;
    const int t0 = blockIdx.x * p.tiles_per_wg;
    const int t1 = (t0 + p.tiles_per_wg < p.ntiles) ? t0 + p.tiles_per_wg : p.ntiles;
    if (t0 >= t1) return;
    // resident weights: 72 fragments of 1 KiB, 18 per wave
#pragma unroll
    for (int k = 0; k < 18; ++k) dma16(p.w + (wave + 4 * k) * 1024 + lane * 16, (wave + 4 * k) * 1024, ~0ull);
    stage_inputs(t0);
    floatx4 bias4[CB][4];
#pragma unroll
    for (int mb = 0; mb < CB; ++mb)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            bias4[mb][g] = p.bias ? *(const floatx4*)(p.bias + mb * 32 + g * 8 + hi * 4) : floatx4{0.f, 0.f, 0.f, 0.f};

    for (int t = t0; t < t1; ++t) {
        int img, Y0, X0;
        tile_origin(t, p.tiles_per_img, p.tiles_x, img, Y0, X0);
        // this tile's inputs (and, first time, the weights) landed ...  From the second tile on the only operations YOUNGER than that DMA are the
        // previous tile's epilogue stores (issued behind stage_inputs): full tiles issue a fixed number of them per wave -- 32 (fp32 output) and /
        // or 16 (16-bit output) -- so the wait leaves exactly those in flight instead of waiting for their acknowledgement as well
        if (t == t0 || nst == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if (nst == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        else if (nst == 32) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(48)" ::: "memory");
        __syncthreads();                                    // ... on every wave
        // FULL forms, earlier requests: wherever they are issued inside tile t, the DMA of tile t + 1 is OLDER than tile t's epilogue stores and
        // younger than nothing else, so the count above stays nst: the wait at the top of tile t + 1 leaves tile t's nst stores in flight, and all
        // input requests (and tile t - 1's stores) have landed.  UPS = 1: the other pair of areas was last read by tile t - 1's MFMAs, which
        // every wave finished before it arrived at the barrier above.
        const int buf = (FULL && UPS) ? (t - t0) & 1 : 0;
        if constexpr (FULL && UPS) {
            if (t + 1 < t1) stage_inputs(t + 1, buf ^ 1);
        }
        floatx16 acc[CB][4];
#pragma unroll
        for (int mb = 0; mb < CB; ++mb)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mb][i][r] = 0.f;
        constexpr int NREAD = G::NP + 3 * CB, NMFMA = 12 * CB;
        half8 P[2][G::NP];
        half8 A[2][3][CB];
        auto load_group = [&](int q, int set) {   // q = chunk * 6 + (ks * 3 + dx)
            const int c = q / 6, g = q - c * 6;
            const int ks = g / 3, dx = g - ks * 3;
            const char* sbi = smem + TAIL_W_B + (buf * 2 + c) * IN_EX;
            const char* sbw = smem + c * (36 * 1024) + lane * 16;
#pragma unroll
            for (int r = 0; r < G::NP; ++r) P[set][r] = *(const half8*)(sbi + aoff[dx][ks] + r * G::ROW_B);
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int mb = 0; mb < CB; ++mb)
                    A[set][dy][mb] = *(const half8*)(sbw + ((((dy * 3 + dx) * 2 + ks) * CB + mb) << 10));
        };
        load_group(0, 0);
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            if (q + 1 < 12) load_group(q + 1, (q + 1) & 1);
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int pr = UPS ? (((i + dy - 1) >> 1) + 1) : (i + dy);
#pragma unroll
                    for (int mb = 0; mb < CB; ++mb)
                        acc[mb][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[q & 1][dy][mb], P[q & 1][pr], acc[mb][i], 0, 0, 0);
                }
            if (q == 0) __builtin_amdgcn_sched_group_barrier(0x100, NREAD, 0);
            if (q + 1 < 12) {
#pragma unroll
                for (int k = 0; k < NREAD; ++k) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, NMFMA - NREAD, 0);
            } else {
                __builtin_amdgcn_sched_group_barrier(0x008, NMFMA, 0);
            }
            if constexpr (FULL && !UPS) {
                if (q == 5) {                      // groups 0..5 were chunk 0: its last reads are in registers (the barrier's lgkmcnt(0)) on every wave
                    __syncthreads();
                    if (t + 1 < t1) stage_chunk(t + 1, 0, 0);
                }
            }
        }
        if constexpr (!FULL) {
            __syncthreads();                       // every wave is done reading the input tiles
            if (t + 1 < t1) stage_inputs(t + 1);   // ... so the next tile's inputs fly under this tile's epilogue
        } else if constexpr (!UPS) {
            __syncthreads();                       // every wave is done reading chunk 1
            if (t + 1 < t1) stage_chunk(t + 1, 1, 0);
        }

        // ---- epilogue, straight from the MFMA D layout: lane (l31, hi) holds for row i and channel group g the 4
        // consecutive channels 8g + 4hi + (0..3) of pixel l31
        if constexpr (FULL) {
            // one output, whole tiles: nothing is computed for the output that does not exist, no store is predicated, and the 32 / 16 stores of
            // a lane go to one pointer per tile (wave-uniform tile origin + the lane's own offset) plus the row stride and constant offsets.
            // Same values as the general form below: the same bias add, and LeakyReLU as max(v, 0.2f * v), which equals
            // v >= 0 ? v : 0.2f * v for every non-NaN v (v > 0: 0.2f * v < v; v < 0: 0.2f * v > v; +-0 and +-inf: both operands are v itself)
            auto value = [&](const int mb, const int i, const int g) {
                floatx4 v;
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = acc[mb][i][g * 4 + q];
                v += bias4[mb][g];
                if constexpr (LRELU) {
                    const floatx4 vs = v * 0.2f;
#pragma unroll
                    for (int q = 0; q < 4; ++q) asm("v_max_f32 %0, %1, %2" : "=v"(v[q]) : "v"(v[q]), "v"(vs[q]));
                }
                return v;
            };
            if constexpr (OUT == OUT_32) {
                const long row32 = (long)p.W * 64;
                float* const o = p.out32 + (((long)img * p.H + Y0) * p.W + X0) * 64 + (wr * 4 * row32 + (wc * 32 + l31) * 64 + hi * 4);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int mb = 0; mb < CB; ++mb) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) *(floatx4*)(o + i * row32 + mb * 32 + g * 8) = value(mb, i, g);
                        // keep the four 32-byte pieces a wave writes into each 128-byte line next to each other: left to the scheduler they
                        // come out group-major across the rows, and conv_hr -- 537 MB of fp32 per batch-32 launch, bound by the memory system --
                        // ran 4 % SLOWER than the general form's predicated stores; in line order it runs 3.6 % faster
                        __builtin_amdgcn_sched_barrier(0);
                    }
            } else {
                const Out16& o16 = p.out16;
                char* const o = o16.base + (long)img * o16.img_b + (long)(Y0 + o16.border) * o16.row_b + (long)X0 * o16.pix_b +
                                ((long)wr * 4 * o16.row_b + (wc * 32 + l31 + o16.border) * o16.pix_b + hi * 16);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int mb = 0; mb < CB; ++mb) {
                        unsigned hp[4][2];
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const floatx4 v = value(mb, i, g);
                            half4 h4;
#pragma unroll
                            for (int q = 0; q < 4; ++q) h4[q] = (_Float16)v[q];
                            const uint2 u = __builtin_bit_cast(uint2, h4);
                            hp[g][0] = u.x;
                            hp[g][1] = u.y;
                        }
#pragma unroll
                        for (int m = 0; m < 2; ++m) *(uintx4*)(o + (long)i * o16.row_b + (long)mb * o16.plane_b + m * 32) = pair16(hp[2 * m], hp[2 * m + 1]);
                    }
            }
            continue;
        }
        const int X = X0 + wc * 32 + l31;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int Y = Y0 + wr * 4 + i;
            const bool valid = (Y < p.H) && (X < p.W);
            const long pix = ((long)img * p.H + Y) * p.W + X;
#pragma unroll
            for (int mb = 0; mb < CB; ++mb) {
                unsigned hp[4][2];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    floatx4 v;
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = acc[mb][i][g * 4 + q];
                    v += bias4[mb][g];
                    if (p.lrelu) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) v[q] = v[q] >= 0.f ? v[q] : v[q] * 0.2f;
                    }
                    if (p.out32 && valid) *(floatx4*)(p.out32 + pix * 64 + mb * 32 + g * 8 + hi * 4) = v;
                    half4 h4;
#pragma unroll
                    for (int q = 0; q < 4; ++q) h4[q] = (_Float16)v[q];
                    const uint2 u = __builtin_bit_cast(uint2, h4);
                    hp[g][0] = u.x;
                    hp[g][1] = u.y;
                }
                if (p.out16.base) {
#pragma unroll
                    for (int m = 0; m < 2; ++m) {
                        store16_pair(p.out16, valid, img, mb, Y, X, m, hi, hp[2 * m], hp[2 * m + 1]);
                    }
                }
            }
        }
    }
}

thread_local int g_ptail_wgs_cap = 0;      // srbh_ptail_wgs_cap: workgroups per launch (0: one per CU)

thread_local int g_ptail_form_counts[SRBH_PTAIL_FORMS] = {};      // srbh_ptail_form_counts: launches per kernel form

template <int UPS, int LRELU, int OUT, int FULL>
int launch(const TParams& p0, hipStream_t stream) {
    static_assert(LDS_B<UPS, FULL> <= 163840, "resident weights + the input chunks must fit the 160 KiB LDS");
    constexpr auto kernel = ptail_kernel<UPS, LRELU, OUT, FULL>;
    constexpr int lds_b = LDS_B<UPS, FULL>;
    SRBH_ONCE_PER_DEVICE(SRBH_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_b)));
    TParams p = p0;
    int grid = 0;
    if (const int rc = tail_grid(p.ntiles, &p.tiles_per_wg, &grid)) return rc;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds_b, stream, p);
    SRBH_HIP(hipGetLastError());
    ++g_ptail_form_counts[FULL ? 1 + 4 * UPS + 2 * LRELU + (OUT == OUT_32) : 0];
    return SRBH_OK;
}

}  // namespace

/* Workgroups per launch of the persistent tail convs (conv_up1 / conv_up2 / conv_hr of srbh_rrdbnet_forward) on the calling host thread: 0 = one
 * per CU (default), n = at most n.  A workgroup of this kernel holds its CU's whole LDS for the entire walk, so a full grid lets no kernel of
 * another stream in: harness.TrainStep caps it for the feature prefetch it runs beside the training step.  Returns the previous value. */
extern "C" int srbh_ptail_wgs_cap(int cap) {
    const int prev = g_ptail_wgs_cap;
    g_ptail_wgs_cap = cap > 0 ? cap : 0;
    return prev;
}

/* Launches per kernel form on the calling host thread (include/srbh.h: [0] general, [1 + 4 ups + 2 lrelu + fp32] the full-tile forms). */
extern "C" int srbh_ptail_form_counts(int* counts, int n, int reset) {
    for (int i = 0; counts && i < n && i < SRBH_PTAIL_FORMS; ++i) counts[i] = g_ptail_form_counts[i];
    if (reset) for (int i = 0; i < SRBH_PTAIL_FORMS; ++i) g_ptail_form_counts[i] = 0;
    return SRBH_PTAIL_FORMS;
}

namespace srbh {

int ptail_wgs_cap() { return g_ptail_wgs_cap; }

// *used = 1 when the persistent form ran (64 -> 64 channels, no residual / skip epilogue), 0 when the caller must launch
// the per-tile kernel
int ptail_run(const srbh_conv3x3_args* a, hipStream_t stream, int* used) {
    *used = 0;
    const char* e = getenv("SRBH_PTAIL");
    if (e && e[0] == '0') return SRBH_OK;
    if (a->in_chunks != 2 || a->cout != 64 || a->res1 || a->res2 || a->skip) return SRBH_OK;
    if (a->out32 && a->out32_c != 64) return SRBH_OK;
    const int tiles_x = (a->W + TILE_W - 1) / TILE_W, tiles_y = (a->H + TILE_H - 1) / TILE_H;
    if (a->out16_nhwc && (!a->out16 || a->out32)) return SRBH_OK;
    if ((long)tiles_x * tiles_y * a->B < 512 && !a->out16_nhwc) return SRBH_OK;   // too few tiles per CU to amortise the resident weights (the NHWC16 store exists only here)
    TParams p{};
    p.in = tail_in16(a, a->in, a->in_chunks_total, a->in_chunk0);
    p.w = (const char*)a->w;
    p.bias = a->bias;
    p.H = a->H;
    p.W = a->W;
    p.tiles_x = tiles_x;
    p.tiles_per_img = tiles_x * tiles_y;
    p.ntiles = p.tiles_per_img * a->B;
    p.lrelu = a->lrelu;
    p.out16 = tail_out16(a, a->out16, a->out16_chunks_total, a->out16_chunk0);
    p.out32 = a->out32;
    // the form: whole tiles and exactly one output -> that conv's full-tile form; anything else (ragged edge, both outputs) -> the general form
    const bool full = a->H % TILE_H == 0 && a->W % TILE_W == 0 && (p.out16.base != nullptr) != (p.out32 != nullptr);
    const int rc = with_const<2>(a->upsample2x != 0, [&](auto u) {
        constexpr int UPS = decltype(u)::value;
        if (!full) return launch<UPS, LRELU_RT, OUT_RT, 0>(p, stream);
        return with_const<2>(a->lrelu != 0, [&](auto l) {
            return with_const<2>(p.out32 != nullptr, [&](auto o) { return launch<UPS, decltype(l)::value, decltype(o)::value ? OUT_32 : OUT_16, 1>(p, stream); });
        });
    });
    if (rc == SRBH_OK) *used = 1;
    return rc;
}

}  // namespace srbh
