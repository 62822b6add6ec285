// srbh_hwgrad_b16_kernel.h -- the 16-bit-operand weight-gradient kernels of the head on 8 x 64 tiles and the walk, staging, tap and flush
// pieces they are built from (included by srbh_head_bwd.hip inside its anonymous namespace, after WGParams and the 16-bit widen / narrow
// helpers).  srbh_hwgrad16_kernel.h and srbh_hbwd16_kernel.h, included behind it, use the walk and tap pieces; hwgrad_f32_kernel uses none.
//
// ---- 16-bit-operand weight gradient (mixed-precision training: hrfuse.set_head_precision("f16")) ----------------------------------
// Same GEMM over pixels, same tile walk, workspace and deterministic two-stage reduction as hwgrad_f32_kernel, but the products run
// on v_mfma_f32_16x16x16_bf16 (K = 16 pixels per instruction; the fp32 form's K = 4 at 32 cycles made the fp32 kernel MFMA-bound at
// ~2x its HBM time).  Both operands are rounded to bf16 (RNE) while staged -- dY needs bf16's exponent range, see srbh_head.hip --
// and accumulated in fp32.  K is the pixel axis, so the 16-bit operands must be contiguous along PIXELS: the staging transposes
// 4 pixels x 4 channels in registers and writes channel-major rows ([channel][row][pixel], 2 pixels per dword; channel stride
// = 4 mod 64 dwords: the 8-byte fragment reads and the staging writes are bank-conflict free).  A tap's dx = -1/+1 fragments are
// funnel-shifted (v_alignbit) out of the aligned quad and one dword of its neighbour.
//
// The kernels differ in their LOOP STRUCTURE only (chunk-outer, chunk-inner, output-block-inner, whole-row prefetch); what they load,
// how they round and stage it, which products a wave forms and in which order the partial sums are added is written once, below:
// that is what makes their partial sums the same bit patterns.
typedef short short4w __attribute__((ext_vector_type(4)));
typedef unsigned uint2w __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned bf16_pair(float lo, float hi) { return bf16x2_rne(lo, hi); }

template <int KS>
struct WG16 {
    static constexpr int TAPS = KS * KS, HALO = KS / 2;
    static constexpr int ROWS = HT_H + 2 * HALO;
    static constexpr int QX = KS == 3 ? 18 : 16;       // staged 4-pixel groups per row: image columns X0-4 .. X0+67 (3x3) / X0 .. X0+63
    static constexpr int XOFF = KS == 3 ? 4 : 0;       // staged column of image column X0
    static constexpr int SX = KS == 3 ? 388 : 260;     // dwords per staged X channel (>= ROWS*QX*2, = 4 mod 64)
    static constexpr int SD = 260;                     // dwords per staged dY channel (8 rows x 64 pixels / 2 + 4)
    static constexpr int NIX = (ROWS * QX * 4 + 255) / 256;   // staging items (4 pixels x 4 channels) of the X tile per thread
    static constexpr int NID = HT_H * 16 * 4 / 256;           // ... of a dY tile
    static constexpr int LDS_B = (16 * SX + 16 * SD) * 4;   // >= the flush buffer (4 waves x TAPS x 256 floats)
    static constexpr int LDS_B2 = (16 * SX + 32 * SD) * 4;  // + the second dY tile of the fused block-entry form (>= 4 x (TAPS + 1) x 256 floats)
};

// ---- the shared pieces ------------------------------------------------------------------------------------------------------------
// (All forced inline.  The staging registers and accumulators are passed by reference; WGParams is passed BY VALUE: behind a reference to
//  the kernel argument the compiler spent up to 5 % more instructions on the addresses of the entry forms (6 056 instead of 5 784 in
//  hwgrad_entry_b16_kernel<0, 4>).  The flush takes the lane coordinates its kernel already holds.)
// XCD-aware walk: explained in srbh_head_walk.h, whose head_walk / head_tile are the same arithmetic behind a reference (this family stays
// on its own by-value pair: by reference four of its forms change).  Returns the workgroup's first tile; its next ones are wg_walk_step()
// apart, up to t_end.
__device__ __forceinline__ int wg_walk(const WGParams p, int& t_end) {
    t_end = min((int)(blockIdx.x & 7) * p.tiles_per_xcd + p.tiles_per_xcd, p.ntiles);
    return (blockIdx.x & 7) * p.tiles_per_xcd + (blockIdx.x >> 3);
}
__device__ __forceinline__ unsigned wg_walk_step() { return gridDim.x >> 3; }
// tile t -> image and the tile's first row / column (tiles of TH x 64 pixels)
template <int TH>
__device__ __forceinline__ void wg_tile(const WGParams p, const int t, int& img, int& Y0, int& X0) {
    img = t / p.tiles_per_img;
    const int trem = t - img * p.tiles_per_img;
    const int ty = trem / p.tiles_x, tx = trem - ty * p.tiles_x;
    Y0 = ty * TH;
    X0 = tx * HT_W;
}

// Global loads of the X tile's 16-channel chunk c: item u = tid + it * 256 is 4 pixels x 4 channels (fp32 in registers), with the forward
// conv's concat / folded BN + ReLU transform applied; outside the image, behind the last channel and behind the last item: zeros.
// XM = 1: ACT16 chunk planes (WGParams::x_*).  CAT = false: src0 is the only source (no src1 branch is compiled).
template <int KS, int XM, bool CAT = true>
__device__ __forceinline__ void wg_load_x(const WGParams p, const int img, const int Y0, const int X0, const int c,
                                          floatx4 (&lx)[WG16<KS>::NIX][4]) {
    using G = WG16<KS>;
    const int tid = threadIdx.x;
    const int cin = CAT ? p.c0 + p.c1 : p.c0;
#pragma unroll
    for (int it = 0; it < G::NIX; ++it) {
        const int u = tid + it * 256;
        const int cg = u & 3, q = u >> 2;
        const int r = q / G::QX, qc = q - r * G::QX;
        const int y = Y0 + r - G::HALO, x0 = X0 - G::XOFF + qc * 4;
        const int ch = c * 16 + cg * 4;
        const bool rowok = u < G::ROWS * G::QX * 4 && y >= 0 && y < p.H && ch < cin;
        const long rowbase = ((long)img * p.H + y) * p.W;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            floatx4 a = {0.f, 0.f, 0.f, 0.f};
            const int x = x0 + i;
            if (rowok && x >= 0 && x < p.W) {
                if constexpr (XM != 0) {
                    a = widen_h4(*(const float2w*)((const char*)p.src0 + (long)img * p.x_img_b + (long)(ch >> 5) * p.x_plane_b +
                                                  (long)(y + 1) * p.x_row_b + (x + 1) * 64 + (ch & 31) * 2));
                } else if (!CAT || ch < p.c0) {
                    if (p.io & SRBH_WG_SRC0_H16)     // (uniform: fp16 elements in memory, e.g. RRDBNet features handed over as fp16)
                        a = widen_h4(*(const float2w*)((const short*)p.src0 + (rowbase + x) * p.ld0 + ch));
                    else
                        a = *(const floatx4*)(p.src0 + (rowbase + x) * p.ld0 + ch);
                    if (p.pre_scale) a = a * *(const floatx4*)(p.pre_scale + ch) + *(const floatx4*)(p.pre_shift + ch);
                    if (p.pre_relu) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) a[j] = fmaxf(a[j], 0.f);
                    }
                } else {
                    a = *(const floatx4*)(p.src1 + (rowbase + x) * p.ld1 + (ch - p.c0));
                }
            }
            lx[it][i] = a;
        }
    }
}
// ... rounded to bf16 and transposed 4 x 4 in registers into the channel-major rows of s_x ([16 ci][SX])
template <int KS>
__device__ __forceinline__ void wg_store_x(unsigned* s_x, const floatx4 (&lx)[WG16<KS>::NIX][4]) {
    using G = WG16<KS>;
    const int tid = threadIdx.x;
#pragma unroll
    for (int it = 0; it < G::NIX; ++it) {
        const int u = tid + it * 256;
        if (u < G::ROWS * G::QX * 4) {
            const int cg = u & 3, q = u >> 2;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *(uint2w*)(s_x + (cg * 4 + j) * G::SX + q * 2) = uint2w{bf16_pair(lx[it][0][j], lx[it][1][j]), bf16_pair(lx[it][2][j], lx[it][3][j])};
        }
    }
}

// A staging item of dY: 4 channels of one pixel, fp32 (DS = 0) or raw bf16 bits (DS = 1: dY holds bf16 elements in memory -- an internal
// gradient tensor of the training step -- and its bits ARE the operand)
template <int DS>
using wg_dy_t = typename std::conditional<DS != 0, float2w, floatx4>::type;
// Global loads of the 8 x 64 dY tile of output block ob from `dy` (XM = 1: the ACT16 planes of p.dy).  TWO: also the same tile of `dy2`
// (the fused entry's 1x1 gradient: same shape and element type) under the same bounds test and byte offset -- as a second call the
// second tile cost the entry forms a second set of exec-mask regions (9 more spilled SGPRs, 4 % more instructions).
template <int DS, int XM, bool TWO>
__device__ __forceinline__ void wg_load_dy(const WGParams p, const float* dy, const int img, const int Y0, const int X0, const int ob,
                                           wg_dy_t<DS> (&ld)[WG16<3>::NID][4], const float* dy2, wg_dy_t<DS> (&ld2)[WG16<3>::NID][4]) {
    typedef wg_dy_t<DS> ldv_t;
    const int tid = threadIdx.x;
#pragma unroll
    for (int it = 0; it < WG16<3>::NID; ++it) {
        const int u = tid + it * 256;
        const int cg = u & 3, q = u >> 2;
        const int y = Y0 + (q >> 4), x0 = X0 + (q & 15) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ldv_t a = ldv_t{}, a2 = ldv_t{};
            if (y < p.H && x0 + i < p.W) {
                long off;
                if constexpr (XM != 0) {
                    const int dch = p.dy_ch0 + ob * 16 + cg * 4;
                    off = (long)img * p.dy_img_b + (long)(dch >> 5) * p.dy_plane_b + (long)(y + 1) * p.dy_row_b + (x0 + i + 1) * 64 + (dch & 31) * 2;
                } else {
                    off = ((((long)img * p.H + y) * p.W + x0 + i) * p.cout_total + ob * 16 + cg * 4) * (DS ? 2 : 4);
                }
                a = *(const ldv_t*)((const char*)dy + off);
                if constexpr (TWO) a2 = *(const ldv_t*)((const char*)dy2 + off);
            }
            ld[it][i] = a;
            if constexpr (TWO) ld2[it][i] = a2;
        }
    }
}
template <int DS, int XM>
__device__ __forceinline__ void wg_load_dy(const WGParams p, const float* dy, const int img, const int Y0, const int X0, const int ob,
                                           wg_dy_t<DS> (&ld)[WG16<3>::NID][4]) {
    wg_load_dy<DS, XM, false>(p, dy, img, Y0, X0, ob, ld, dy, ld);
}
// ... into the channel-major rows of s_dy ([16 oc][SD]): rounded to bf16 (DS = 0) or picked out of the raw quads (DS = 1)
template <int DS>
__device__ __forceinline__ void wg_store_dy(unsigned* s_dy, const wg_dy_t<DS> (&ld)[WG16<3>::NID][4]) {
    constexpr int SD = WG16<3>::SD;
    const int tid = threadIdx.x;
#pragma unroll
    for (int it = 0; it < WG16<3>::NID; ++it) {
        const int u = tid + it * 256;
        const int cg = u & 3, q = u >> 2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (DS != 0)
                *(uint2w*)(s_dy + (cg * 4 + j) * SD + q * 2) = uint2w{b16_field_pair(ld[it][0], ld[it][1], j), b16_field_pair(ld[it][2], ld[it][3], j)};
            else
                *(uint2w*)(s_dy + (cg * 4 + j) * SD + q * 2) = uint2w{bf16_pair(ld[it][0][j], ld[it][1][j]), bf16_pair(ld[it][2][j], ld[it][3][j])};
        }
    }
}

// The three dx taps of one staged row on one K group of 16 pixels: rp -> this lane's aligned quad of the channel row; a = the dY fragment.
// acc_l / acc_c / acc_r are the taps dx = -1 / 0 / +1.  Returns the aligned (centre-tap) fragment.
__device__ __forceinline__ short4w wg_row_taps(const unsigned* rp, const short4w a, floatx4& acc_l, floatx4& acc_c, floatx4& acc_r) {
    const uint2w cur = *(const uint2w*)rp;
    const unsigned pv = rp[-1], nx = rp[2];
    const unsigned mid = __builtin_amdgcn_alignbit(cur[1], cur[0], 16);
    const uint2w b0 = {__builtin_amdgcn_alignbit(cur[0], pv, 16), mid};
    const uint2w b2 = {mid, __builtin_amdgcn_alignbit(nx, cur[1], 16)};
    const short4w bc = __builtin_bit_cast(short4w, cur);
    acc_l = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, __builtin_bit_cast(short4w, b0), acc_l, 0, 0, 0);
    acc_c = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, bc, acc_c, 0, 0, 0);
    acc_r = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, __builtin_bit_cast(short4w, b2), acc_r, 0, 0, 0);
    return bc;
}
// a lane's 8-byte MFMA fragment (4 of a K group's 16 pixels) out of a staged channel row
__device__ __forceinline__ short4w wg_frag(const unsigned* q) { return __builtin_bit_cast(short4w, *(const uint2w*)q); }

// Flush of a workgroup's TAPS accumulators (D[row = oc = kk*4 + r][col = ci = l15] in each of the 4 waves) into its workspace slot of
// TAPS * 256 floats: through s_red, the waves added in the order 0, 1, 2, 3.  No atomics: 512 workgroups adding into the same 2 304
// addresses cost 60 us of a 318 us layer (and made the gradient order-dependent); every workgroup stores its partial, a second tiny
// kernel adds them in order.  s_red aliases the staging buffers: barriers before the waves' stores and before the sums; the caller
// puts one behind the flush if it stages again.
template <int TAPS>
__device__ __forceinline__ void wg_flush(float* s_red, const floatx4 (&acc)[TAPS], float* ws, const long slot, const int tid, const int wave, const int l15, const int kk) {
    __syncthreads();
#pragma unroll
    for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
        for (int r = 0; r < 4; ++r) s_red[((wave * TAPS + tp) * 16 + kk * 4 + r) * 16 + l15] = acc[tp][r];
    __syncthreads();
    for (int u = tid; u < TAPS * 256; u += 256) {
        const float v = s_red[u] + s_red[TAPS * 256 + u] + s_red[2 * TAPS * 256 + u] + s_red[3 * TAPS * 256 + u];
        ws[slot * (TAPS * 256) + u] = v;
    }
}
// the workspace slot of (workgroup column blockIdx.x, output block ob of nob, chunk c of nchunk)
__device__ __forceinline__ long wg_slot(const unsigned nob, const int ob, const int nchunk, const int c) {
    return ((long)blockIdx.x * nob + ob) * nchunk + c;
}

// ---- the kernels ------------------------------------------------------------------------------------------------------------------
// Chunk-outer form.  One workgroup walks its tiles once per 16-channel input chunk and keeps the 16(oc) x 16(ci) x taps partial sums
// of one (oc block = blockIdx.y, ci chunk) in registers.  It shares the walk and the tap products; its staging and flush stay written out:
// through wg_load_x the ACT16 form came out with 24 more instructions and measured 0.7 - 1 % slower (38.4 instead of 38.0 us for the
// 192 -> 64 conv of the RRDBNet training path), through wg_store_* / wg_flush the LDS accesses of three forms paired differently.  The
// bit-for-bit tests between the forms (tests/test_gpu_head_f16.py) hold the two texts together.
// DS = 1: dY holds bf16 elements in memory (an internal gradient tensor of the training step): its bits are the operand
// XM = 1: both tensors are ACT16 chunk planes (WGParams::x_* / dy_*): X fp16, dY bf16 (DS must be 1)
// D2 = 1 (KS = 3, XM = 0): fused BasicBlock entry (SR/HRfuse.py:142-159): conv1 (3x3) and downsample[0] (1x1) read the same input, so
//   their weight gradients share the staged X tile -- the 1x1 gradient is one more MFMA per K step on the centre-tap fragment with its
//   own dY (p.dy2, same element type and channel count as dy); what bounds these kernels is the X staging (fp32 / fp16 -> bf16, 4x4
//   register transposes into channel-major rows), which the separate 1x1 launch repeated in full.
template <int KS, int DS, int XM = 0, int D2 = 0>
__global__ __launch_bounds__(256) void hwgrad_b16_kernel(const WGParams p) {
    static_assert(D2 == 0 || (KS == 3 && XM == 0), "the fused entry form is the 3x3 NHWC kernel");
    extern __shared__ __attribute__((aligned(16))) float wsm[];
    using G = WG16<KS>;
    constexpr int TAPS = G::TAPS, HALO = G::HALO, ROWS = G::ROWS, QX = G::QX, SX = G::SX, SD = G::SD;
    static_assert(G::LDS_B >= 4 * TAPS * 256 * 4, "flush buffer must fit");
    unsigned* s_x = (unsigned*)wsm;                 // [16 ci][SX]
    unsigned* s_dy = s_x + 16 * SX;                 // [16 oc][SD]
    unsigned* s_dy2 = s_dy + 16 * SD;               // [16 oc][SD] (D2)
    float* s_red = wsm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kk = lane >> 4;
    const int cin = p.c0 + p.c1;
    const int nchunk = (cin + 15) / 16;
    const int ob = blockIdx.y;
    // (zchunk: with few tiles -- the RRDBNet training path at batch 8 has 64 -- the chunk loop is spread over blockIdx.z: a workgroup's
    //  chunk iterations are a serial load -> LDS -> MFMA chain of ~4 us each, 12 of them for a 192-channel conv on a quarter-filled GPU)
    const int c_lo = p.zchunk ? (int)blockIdx.z : 0, c_hi = p.zchunk ? (int)blockIdx.z + 1 : nchunk;

    for (int c = c_lo; c < c_hi; ++c) {
        floatx4 acc[TAPS];
#pragma unroll
        for (int tp = 0; tp < TAPS; ++tp) acc[tp] = floatx4{0.f, 0.f, 0.f, 0.f};
        floatx4 acc2 = {0.f, 0.f, 0.f, 0.f};
        int t_end;
        for (int t = wg_walk(p, t_end); t < t_end; t += wg_walk_step()) {
            int img, Y0, X0;
            wg_tile<HT_H>(p, t, img, Y0, X0);
            // ---- stage: every global load of the tile is issued before the first LDS store.  (Issuing the NEXT tile's loads before this
            // tile's MFMAs -- a software pipeline over the walk -- needs 281 registers, one workgroup per CU: 152 -> 232 us.)
            constexpr int NIX = (ROWS * QX * 4 + 255) / 256, NID = HT_H * 16 * 4 / 256;
            typedef typename std::conditional<DS != 0, float2w, floatx4>::type ldv_t;
            floatx4 lx[NIX][4];
            ldv_t ld[NID][4];
            ldv_t ld2[D2 ? NID : 1][4];
#pragma unroll
            for (int it = 0; it < NIX; ++it) {
                const int u = tid + it * 256;
                const int cg = u & 3, q = u >> 2;
                const int r = q / QX, qc = q - r * QX;
                const int y = Y0 + r - HALO, x0 = X0 - G::XOFF + qc * 4;
                const int ch = c * 16 + cg * 4;
                const bool rowok = u < ROWS * QX * 4 && y >= 0 && y < p.H && ch < cin;
                const long rowbase = ((long)img * p.H + y) * p.W;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    floatx4 a = {0.f, 0.f, 0.f, 0.f};
                    const int x = x0 + i;
                    if (rowok && x >= 0 && x < p.W) {
                        if constexpr (XM != 0) {
                            a = widen_h4(*(const float2w*)((const char*)p.src0 + (long)img * p.x_img_b + (long)(ch >> 5) * p.x_plane_b +
                                                          (long)(y + 1) * p.x_row_b + (x + 1) * 64 + (ch & 31) * 2));
                        } else if (ch < p.c0) {
                            if (p.io & SRBH_WG_SRC0_H16)     // (uniform: fp16 elements in memory, e.g. RRDBNet features handed over as fp16)
                                a = widen_h4(*(const float2w*)((const short*)p.src0 + (rowbase + x) * p.ld0 + ch));
                            else
                                a = *(const floatx4*)(p.src0 + (rowbase + x) * p.ld0 + ch);
                            if (p.pre_scale) a = a * *(const floatx4*)(p.pre_scale + ch) + *(const floatx4*)(p.pre_shift + ch);
                            if (p.pre_relu) {
#pragma unroll
                                for (int j = 0; j < 4; ++j) a[j] = fmaxf(a[j], 0.f);
                            }
                        } else {
                            a = *(const floatx4*)(p.src1 + (rowbase + x) * p.ld1 + (ch - p.c0));
                        }
                    }
                    lx[it][i] = a;
                }
            }
#pragma unroll
            for (int it = 0; it < NID; ++it) {
                const int u = tid + it * 256;
                const int cg = u & 3, q = u >> 2;
                const int y = Y0 + (q >> 4), x0 = X0 + (q & 15) * 4;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ldv_t a = ldv_t{};
                    if (y < p.H && x0 + i < p.W) {
                        if constexpr (XM != 0) {
                            const int dch = p.dy_ch0 + ob * 16 + cg * 4;
                            a = *(const ldv_t*)((const char*)p.dy + (long)img * p.dy_img_b + (long)(dch >> 5) * p.dy_plane_b + (long)(y + 1) * p.dy_row_b +
                                                (x0 + i + 1) * 64 + (dch & 31) * 2);
                        } else {
                            a = *(const ldv_t*)((const char*)p.dy + ((((long)img * p.H + y) * p.W + x0 + i) * p.cout_total + ob * 16 + cg * 4) * (DS ? 2 : 4));
                        }
                    }
                    ld[it][i] = a;
                    if constexpr (D2 != 0) {
                        ldv_t a2 = ldv_t{};
                        if (y < p.H && x0 + i < p.W)
                            a2 = *(const ldv_t*)((const char*)p.dy2 + ((((long)img * p.H + y) * p.W + x0 + i) * p.cout_total + ob * 16 + cg * 4) * (DS ? 2 : 4));
                        ld2[it][i] = a2;
                    }
                }
            }
            __syncthreads();                       // the previous tile's fragment reads are done
#pragma unroll
            for (int it = 0; it < NIX; ++it) {
                const int u = tid + it * 256;
                if (u < ROWS * QX * 4) {
                    const int cg = u & 3, q = u >> 2;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        *(uint2w*)(s_x + (cg * 4 + j) * SX + q * 2) =
                            uint2w{bf16_pair(lx[it][0][j], lx[it][1][j]), bf16_pair(lx[it][2][j], lx[it][3][j])};
                }
            }
#pragma unroll
            for (int it = 0; it < NID; ++it) {
                const int u = tid + it * 256;
                const int cg = u & 3, q = u >> 2;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (DS != 0)
                        *(uint2w*)(s_dy + (cg * 4 + j) * SD + q * 2) = uint2w{b16_field_pair(ld[it][0], ld[it][1], j), b16_field_pair(ld[it][2], ld[it][3], j)};
                    else
                        *(uint2w*)(s_dy + (cg * 4 + j) * SD + q * 2) =
                            uint2w{bf16_pair(ld[it][0][j], ld[it][1][j]), bf16_pair(ld[it][2][j], ld[it][3][j])};
                    if constexpr (D2 != 0) {
                        if constexpr (DS != 0)
                            *(uint2w*)(s_dy2 + (cg * 4 + j) * SD + q * 2) = uint2w{b16_field_pair(ld2[it][0], ld2[it][1], j), b16_field_pair(ld2[it][2], ld2[it][3], j)};
                        else
                            *(uint2w*)(s_dy2 + (cg * 4 + j) * SD + q * 2) =
                                uint2w{bf16_pair(ld2[it][0][j], ld2[it][1][j]), bf16_pair(ld2[it][2][j], ld2[it][3][j])};
                    }
                }
            }
            __syncthreads();
            // ---- 2 rows x 4 groups of 16 pixels per wave
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const int row = wave * 2 + (ks >> 2), g = ks & 3;
                const short4w a = wg_frag(s_dy + l15 * SD + (row * 16 + g * 4 + kk) * 2);
                const unsigned* bp = s_x + l15 * SX + (row * QX + (G::XOFF >> 2) + g * 4 + kk) * 2;
#pragma unroll
                for (int dy = 0; dy < KS; ++dy) {
                    const unsigned* rp = bp + dy * QX * 2;
                    if constexpr (KS == 3) {
                        const short4w cur = wg_row_taps(rp, a, acc[dy * 3 + 0], acc[dy * 3 + 1], acc[dy * 3 + 2]);
                        if constexpr (D2 != 0) {
                            if (dy == 1) acc2 = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(wg_frag(s_dy2 + l15 * SD + (row * 16 + g * 4 + kk) * 2), cur, acc2, 0, 0, 0);
                        }
                    } else {
                        acc[0] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, wg_frag(rp), acc[0], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
            for (int r = 0; r < 4; ++r) s_red[((wave * TAPS + tp) * 16 + kk * 4 + r) * 16 + l15] = acc[tp][r];
        __syncthreads();
        for (int u = tid; u < TAPS * 256; u += 256) {
            const float v = s_red[u] + s_red[TAPS * 256 + u] + s_red[2 * TAPS * 256 + u] + s_red[3 * TAPS * 256 + u];
            p.ws[(((long)blockIdx.x * gridDim.y + ob) * nchunk + c) * (TAPS * 256) + u] = v;
        }
        __syncthreads();                           // s_red aliases the staging buffers of the next chunk
        if constexpr (D2 != 0) {                   // the 1x1 gradient's partial sums, in the layout of a ksize = 1 call
#pragma unroll
            for (int r = 0; r < 4; ++r) s_red[(wave * 16 + kk * 4 + r) * 16 + l15] = acc2[r];
            __syncthreads();
            p.ws2[(((long)blockIdx.x * gridDim.y + ob) * nchunk + c) * 256 + tid] = s_red[tid] + s_red[256 + tid] + s_red[512 + tid] + s_red[768 + tid];
            __syncthreads();
        }
    }
}

// Fused BasicBlock-entry weight gradient with the CHUNK loop inside the tile walk (round 4).  hwgrad_b16_kernel<3, DS, 0, 1> walks all its
// tiles once per 16-channel chunk of the input: the 64-channel entry (HRfeature: cin = 64, fp16 features) re-staged both dY tiles four times
// and touched 32 bytes of every 128-byte pixel row per pass -- 891 us for 805 MB (0.11 of the HBM peak, profiles/r04p).  Here a tile's dY /
// dY2 are staged once, the NC chunks of X follow one another through the same LDS buffer (chunk c + 1's global loads are issued before
// chunk c's MFMAs: the rows' other three 32-byte quarters come out of L2 while they are hot), and NC x 10 accumulators stay in registers.
// Same tile walk, same wave -> row assignment, same flush: every partial sum is the bit pattern the chunk-outer kernel writes.
template <int DS, int NC>
__global__ __launch_bounds__(256) void hwgrad_entry_b16_kernel(const WGParams p) {
    extern __shared__ __attribute__((aligned(16))) float wsm[];
    using G = WG16<3>;
    constexpr int TAPS = G::TAPS, QX = G::QX, SX = G::SX, SD = G::SD;
    unsigned* s_x = (unsigned*)wsm;                 // [16 ci][SX]
    unsigned* s_dy = s_x + 16 * SX;                 // [16 oc][SD]
    unsigned* s_dy2 = s_dy + 16 * SD;               // [16 oc][SD]
    float* s_red = wsm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kk = lane >> 4;
    const int ob = blockIdx.y;
    floatx4 acc[NC][TAPS];
    floatx4 acc2[NC][1];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int tp = 0; tp < TAPS; ++tp) acc[c][tp] = floatx4{0.f, 0.f, 0.f, 0.f};
        acc2[c][0] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    int t_end;
    for (int t = wg_walk(p, t_end); t < t_end; t += wg_walk_step()) {
        int img, Y0, X0;
        wg_tile<HT_H>(p, t, img, Y0, X0);
        floatx4 lx[G::NIX][4];
        {
            wg_dy_t<DS> ld[G::NID][4], ld2[G::NID][4];
            wg_load_x<3, 0>(p, img, Y0, X0, 0, lx);
            wg_load_dy<DS, 0, true>(p, p.dy, img, Y0, X0, ob, ld, p.dy2, ld2);
            __syncthreads();                       // the previous tile's fragment reads are done
            wg_store_x<3>(s_x, lx);
            wg_store_dy<DS>(s_dy, ld);
            wg_store_dy<DS>(s_dy2, ld2);
            __syncthreads();
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (c + 1 < NC) wg_load_x<3, 0>(p, img, Y0, X0, c + 1, lx);      // (in flight under this chunk's MFMAs)
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const int row = wave * 2 + (ks >> 2), g = ks & 3;
                const short4w a = wg_frag(s_dy + l15 * SD + (row * 16 + g * 4 + kk) * 2);
                const unsigned* bp = s_x + l15 * SX + (row * QX + (G::XOFF >> 2) + g * 4 + kk) * 2;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const short4w cur = wg_row_taps(bp + dy * QX * 2, a, acc[c][dy * 3 + 0], acc[c][dy * 3 + 1], acc[c][dy * 3 + 2]);
                    if (dy == 1)
                        acc2[c][0] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(wg_frag(s_dy2 + l15 * SD + (row * 16 + g * 4 + kk) * 2), cur, acc2[c][0], 0, 0, 0);
                }
            }
            if (c + 1 < NC) {
                __syncthreads();                   // every wave has read chunk c's fragments
                wg_store_x<3>(s_x, lx);
                __syncthreads();
            }
        }
    }
    // flush, chunk by chunk, in the layout of the chunk-outer kernel
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        wg_flush<TAPS>(s_red, acc[c], p.ws, wg_slot(gridDim.y, ob, NC, c), tid, wave, l15, kk);
        wg_flush<1>(s_red, acc2[c], p.ws2, wg_slot(gridDim.y, ob, NC, c), tid, wave, l15, kk);
    }
}

// Weight gradient of a conv with ONE input chunk and NOB output blocks (the Upsampler's 16 -> 64 convs, SR/HRfuse.py:17-44: dY = the
// PixelShuffle-inverted gradient, 64 channels): hwgrad_b16_kernel runs grid.y = NOB workgroups per tile, each staging the same X tile
// (the fp32 -> bf16 4x4 register transposes that bound these kernels).  Here the X tile is staged once and the NOB dY blocks follow one
// another through the dY buffer (block ob + 1's loads issued before block ob's MFMAs), NOB x 9 accumulators in registers.  Same walk,
// wave -> row assignment, products and flush layout as the chunk-outer kernel with grid.y = NOB: bit-identical partial sums.
template <int DS, int NOB>
__global__ __launch_bounds__(256) void hwgrad_ob_b16_kernel(const WGParams p) {
    extern __shared__ __attribute__((aligned(16))) float wsm[];
    using G = WG16<3>;
    constexpr int TAPS = G::TAPS, QX = G::QX, SX = G::SX, SD = G::SD;
    unsigned* s_x = (unsigned*)wsm;                 // [16 ci][SX]
    unsigned* s_dy = s_x + 16 * SX;                 // [16 oc][SD]
    float* s_red = wsm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kk = lane >> 4;
    floatx4 acc[NOB][TAPS];
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
        for (int tp = 0; tp < TAPS; ++tp) acc[ob][tp] = floatx4{0.f, 0.f, 0.f, 0.f};
    int t_end;
    for (int t = wg_walk(p, t_end); t < t_end; t += wg_walk_step()) {
        int img, Y0, X0;
        wg_tile<HT_H>(p, t, img, Y0, X0);
        wg_dy_t<DS> ld[G::NID][4];
        {
            floatx4 lx[G::NIX][4];
            wg_load_x<3, 0, false>(p, img, Y0, X0, 0, lx);
            wg_load_dy<DS, 0>(p, p.dy, img, Y0, X0, 0, ld);
            __syncthreads();                       // the previous tile's fragment reads are done
            wg_store_x<3>(s_x, lx);
            wg_store_dy<DS>(s_dy, ld);
            __syncthreads();
        }
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob) {
            if (ob + 1 < NOB) wg_load_dy<DS, 0>(p, p.dy, img, Y0, X0, ob + 1, ld);      // (in flight under this block's MFMAs)
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const int row = wave * 2 + (ks >> 2), g = ks & 3;
                const short4w a = wg_frag(s_dy + l15 * SD + (row * 16 + g * 4 + kk) * 2);
                const unsigned* bp = s_x + l15 * SX + (row * QX + (G::XOFF >> 2) + g * 4 + kk) * 2;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) wg_row_taps(bp + dy * QX * 2, a, acc[ob][dy * 3 + 0], acc[ob][dy * 3 + 1], acc[ob][dy * 3 + 2]);
            }
            if (ob + 1 < NOB) {
                __syncthreads();                   // every wave has read block ob's dY fragments
                wg_store_dy<DS>(s_dy, ld);
                __syncthreads();
            }
        }
    }
#pragma unroll
    for (int ob = 0; ob < NOB; ++ob)               // (= the chunk-outer layout with grid.y = NOB, nchunk = 1)
        wg_flush<TAPS>(s_red, acc[ob], p.ws, wg_slot(NOB, ob, 1, 0), tid, wave, l15, kk);
}

// HRfeature's entry (cin = 64, the RRDBNet features handed over as fp16 NHWC: 128 bytes per pixel): the chunked kernels above read 32 bytes
// of every pixel row per pass -- each load instruction touches 16 different 128-byte lines -- and ran at 0.11 of the HBM peak.  Here a lane
// loads 16 bytes (8 channels) and 8 lanes cover a pixel's whole row, ALL FOUR chunks of a tile are staged at once (64 channel rows in LDS,
// 130 KB with the two dY tiles: one workgroup per CU), and the next tile's global loads are issued before this tile's MFMAs (register
// prefetch: 96 + 32 registers) -- the one workgroup per CU has nothing else to hide the load latency behind.  Same walk, wave -> row
// assignment, products and flush as hwgrad_entry_b16_kernel<DS, 4>: bit-identical partial sums.
struct WG64 {
    using G = WG16<3>;
    static constexpr int NIT = (G::ROWS * G::QX * 8 + 255) / 256;           // 16-byte units of the X tile per thread
    static constexpr int LDS_B = (64 * G::SX + 32 * G::SD) * 4;
};
typedef unsigned uint4w __attribute__((ext_vector_type(4)));
typedef _Float16 half8w __attribute__((ext_vector_type(8)));
template <int DS>
__global__ __launch_bounds__(256) void hwgrad_entry64_b16_kernel(const WGParams p) {
    extern __shared__ __attribute__((aligned(16))) float wsm[];
    using G = WG16<3>;
    constexpr int TAPS = G::TAPS, ROWS = G::ROWS, QX = G::QX, SX = G::SX, SD = G::SD, NIT = WG64::NIT, NC = 4;
    static_assert(WG64::LDS_B >= 4 * TAPS * 256 * 4, "flush buffer must fit");
    unsigned* s_x = (unsigned*)wsm;                 // [64 ci][SX]
    unsigned* s_dy = s_x + 64 * SX;                 // [16 oc][SD]
    unsigned* s_dy2 = s_dy + 16 * SD;
    float* s_red = wsm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kk = lane >> 4;
    const int ob = blockIdx.y;
    floatx4 acc[NC][TAPS];
    floatx4 acc2[NC][1];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int tp = 0; tp < TAPS; ++tp) acc[c][tp] = floatx4{0.f, 0.f, 0.f, 0.f};
        acc2[c][0] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    uint4w lx[NIT][4];
    wg_dy_t<DS> ld[G::NID][4], ld2[G::NID][4];
    auto load_tile = [&](const int t) {
        int img, Y0, X0;
        wg_tile<HT_H>(p, t, img, Y0, X0);
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int u = tid + it * 256;
            const int pc = u & 7, q = u >> 3;
            const int r = q / QX, qc = q - r * QX;
            const int y = Y0 + r - 1, x0 = X0 - G::XOFF + qc * 4;
            const bool rowok = u < ROWS * QX * 8 && y >= 0 && y < p.H;
            const short* rowp = (const short*)p.src0 + (((long)img * p.H + y) * p.W) * 64 + pc * 8;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uint4w a = {0u, 0u, 0u, 0u};
                const int x = x0 + i;
                if (rowok && x >= 0 && x < p.W) a = *(const uint4w*)(rowp + (long)x * 64);
                lx[it][i] = a;
            }
        }
        wg_load_dy<DS, 0, true>(p, p.dy, img, Y0, X0, ob, ld, p.dy2, ld2);
    };
    int t_end;
    const int t_step = wg_walk_step();
    int t = wg_walk(p, t_end);
    if (t < t_end) load_tile(t);
    for (; t < t_end; t += t_step) {
        __syncthreads();                           // the previous tile's fragment reads are done
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int u = tid + it * 256;
            if (u < ROWS * QX * 8) {
                const int pc = u & 7, q = u >> 3;
                const half8w h0 = __builtin_bit_cast(half8w, lx[it][0]), h1 = __builtin_bit_cast(half8w, lx[it][1]);
                const half8w h2 = __builtin_bit_cast(half8w, lx[it][2]), h3 = __builtin_bit_cast(half8w, lx[it][3]);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    *(uint2w*)(s_x + (pc * 8 + j) * SX + q * 2) =
                        uint2w{bf16_pair((float)h0[j], (float)h1[j]), bf16_pair((float)h2[j], (float)h3[j])};
            }
        }
        wg_store_dy<DS>(s_dy, ld);
        wg_store_dy<DS>(s_dy2, ld2);
        __syncthreads();
        if (t + t_step < t_end) load_tile(t + t_step);      // in flight under this tile's 4 x 80 MFMAs
#pragma unroll
        for (int c = 0; c < NC; ++c) {
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const int row = wave * 2 + (ks >> 2), g = ks & 3;
                const short4w a = wg_frag(s_dy + l15 * SD + (row * 16 + g * 4 + kk) * 2);
                const unsigned* bp = s_x + (c * 16 + l15) * SX + (row * QX + (G::XOFF >> 2) + g * 4 + kk) * 2;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const short4w cur = wg_row_taps(bp + dy * QX * 2, a, acc[c][dy * 3 + 0], acc[c][dy * 3 + 1], acc[c][dy * 3 + 2]);
                    if (dy == 1)
                        acc2[c][0] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(wg_frag(s_dy2 + l15 * SD + (row * 16 + g * 4 + kk) * 2), cur, acc2[c][0], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        wg_flush<TAPS>(s_red, acc[c], p.ws, wg_slot(gridDim.y, ob, NC, c), tid, wave, l15, kk);
        wg_flush<1>(s_red, acc2[c], p.ws2, wg_slot(gridDim.y, ob, NC, c), tid, wave, l15, kk);
    }
}
