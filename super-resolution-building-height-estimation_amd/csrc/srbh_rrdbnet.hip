// srbh_rrdbnet.hip -- host-side driver that runs RRDBNet.forward_feature / forward
// (reference SR/rrdbnet_arch.py:208-240) as a fixed sequence of libsrbh kernel launches on one stream.
//
// Dense-block concat is never materialised: one ACT16 buffer with 6 chunk planes per image holds
// [x | x1 | x2 | x3 | x4] (SR/rrdbnet_arch.py:137-141); conv_k reads planes 0..k and writes plane k+1;
// conv5 writes the next block's x into planes 0..1 of the other (ping-pong) buffer.  The fp32
// residual streams (x5*0.2+x at :143, out*0.2+x at :167, feat+body_feat at :234) live in three RES32 buffers.
#include <stdlib.h>
#include "srbh_internal.h"

using namespace srbh;

namespace {

struct WsLayout {
    size_t d0, d1, feat, xr, xrr, u2, u3, u4, aux, total;
    size_t u2lo, u3lo;      // f16x2 mode only: the lo' planes of conv_up1's / conv_up2's outputs, BEHIND everything else
    size_t dense_b;
};

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// The persistent trunk kernel needs every workgroup co-resident; if something else holds CUs / LDS its bounded spins
// time out, it sets an error word and drains, and the kernels behind it would run on stale activations.  This guard
// runs last in the forward: error word clear -> every workgroup returns at once; set -> the whole output becomes NaN,
// so a timed-out launch can never be mistaken for a result (features, mosaics and losses all turn NaN).  The host-side
// check (srbh_rrdbnet_last_status) stays the way to get the reason.
__global__ __launch_bounds__(256) void poison_on_error_kernel(const int* __restrict__ err, float* __restrict__ out, size_t n) {
    if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
    const float nan = __builtin_nanf("");
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = nan;
}

// The persistent trunk kernel keeps the RRDB-level stream `xrr` in conv5's accumulator ("fragment") order: per image row of 64 pixels x 64
// channels, float4 number wc * 512 + mb * 256 + g * 64 + lane holds channels mb * 32 + g * 8 + (lane >> 5) * 4 .. + 3 of pixel
// wc * 32 + (lane & 31) (srbh_ptrunk3_kernel.h, epi64).  This copies such a stream out in pixel order (NHWC); nquads = rows * 1024.
__global__ __launch_bounds__(256) void trunk_out_pixel_order_kernel(const float* __restrict__ src, float* __restrict__ dst, long nquads) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nquads; i += (long)gridDim.x * blockDim.x) {
        const long row = i >> 10;
        const int f = (int)(i & 1023);
        const int lane = f & 63, g = (f >> 6) & 3, mb = (f >> 8) & 1, wc = f >> 9;
        const int px = wc * 32 + (lane & 31);
        ((f4*)dst)[row * 1024 + px * 16 + mb * 8 + g * 2 + (lane >> 5)] = ((const f4*)src)[i];
    }
}

// Every environment switch of this file: on unless its value starts with '0'.  SRBH_PERSISTENT and SRBH_TRUNK_BF16 are A/B switches
// read on EVERY call (a plain env_off call); the SRBH_SR_* switches of the training path are read ONCE per process (a function-local
// `static const bool` at their use).
inline bool env_off(const char* name) {
    const char* env = getenv(name);
    return env && env[0] == '0';
}

inline int tiles_per_img(int H) { return (H + TILE_H - 1) / TILE_H; }

// the persistent trunk kernel's error word inside its scratch `aux`
inline const int* ptrunk_err_word(const void* aux, int B, int H) {
    return (const int*)((const char*)aux + ptrunk_err_offset(B, tiles_per_img(H)));
}

// poison_on_error_kernel behind a launch of the persistent trunk kernel: `n` floats of `out` turn NaN if `err` is set
inline int poison_on_error(const int* err, float* out, size_t n, unsigned wgs, hipStream_t st) {
    hipLaunchKernelGGL(poison_on_error_kernel, dim3(wgs), dim3(256), 0, st, err, out, n);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

// ---- the network's 3x3 convs, one description per shape -----------------------------------------------------------------------------
// `in_chunks` planes from plane 0 of an ACT16 buffer with `in_chunks_total` planes per image -> cout channels; outputs are the caller's
inline srbh_conv3x3_args conv_on(const void* in, int in_chunks_total, int in_chunks, const void* w, const float* bias, int cout, int B, int H, int W) {
    srbh_conv3x3_args a{};
    a.in = in; a.in_chunks_total = in_chunks_total; a.in_chunk0 = 0; a.in_chunks = in_chunks;
    a.w = w; a.bias = bias; a.cout = cout;
    a.B = B; a.H = H; a.W = W;
    return a;
}
inline void out_planes(srbh_conv3x3_args& a, void* out16, int chunks_total, int chunk0) {
    a.out16 = out16; a.out16_chunks_total = chunks_total; a.out16_chunk0 = chunk0;
}

// conv_{k+1}, k = 0..3, of a dense block on its 6-plane buffer: x_{k+1} = lrelu(conv(cat(x, x1..xk))) into plane 2 + k
inline srbh_conv3x3_args growth_conv(void* D, int k, const srbh_conv_w& cw, int B, int H, int W) {
    srbh_conv3x3_args a = conv_on(D, 6, 2 + k, cw.w, cw.bias, 32, B, H, W);
    a.lrelu = 1;
    out_planes(a, D, 6, 2 + k);
    return a;
}

// conv5 + x5*0.2 + x on the fp32 stream xr (+ out*0.2 + x_rrdb on xrr at the end of an RRDB; NULL elsewhere); the new x as planes 0..1 of `next`
inline srbh_conv3x3_args conv5(const void* D, void* next, float* xr, float* xrr, const srbh_conv_w& cw, int B, int H, int W) {
    srbh_conv3x3_args a = conv_on(D, 6, 6, cw.w, cw.bias, 64, B, H, W);
    a.res_scale = 0.2f; a.res1 = xr; a.res1_update = 1;
    if (xrr) { a.res2 = xrr; a.res2_scale = 0.2f; a.res2_update = 1; }
    out_planes(a, next, 6, 0);
    return a;
}

// a 64 -> 64 conv of the up-sampler tail on planes 0..1 of `in`; H, W: output geometry
inline srbh_conv3x3_args tail_conv(const void* in, int in_chunks_total, const srbh_conv_w& cw, int B, int H, int W, int upsample2x, int lrelu) {
    srbh_conv3x3_args a = conv_on(in, in_chunks_total, 2, cw.w, cw.bias, 64, B, H, W);
    a.upsample2x = upsample2x; a.lrelu = lrelu;
    return a;
}

// gradient conv j of a dense block on its G buffer [g5 (2 planes) | g4 | g3 | g2 | g1]: j = 0..3 gives g4..g1 in plane 2 + j (the caller
// passes the LeakyReLU mask); j = 4 is dx = conv(G) + skip as fp32 NHWC
inline srbh_conv3x3_args grad_conv(void* G, int j, const void* w, int B, int H, int W, const float* skip = nullptr, float* dx = nullptr) {
    srbh_conv3x3_args a = conv_on(G, 6, j < 4 ? 2 + j : 6, w, nullptr, j < 4 ? 32 : 64, B, H, W);
    if (j < 4) out_planes(a, G, 6, 2 + j);
    else { a.skip = skip; a.out32 = dx; a.out32_c = 64; }
    return a;
}

// The five launches of one residual dense block (SR/rrdbnet_arch.py:137-143) on buffer D, the next block's x into `next`.  fp16 operands
// (srbh_conv3x3_f16), or bf16 ones (conv3x3_trunk_b16) with conv5's planes rounded to fp16 when out_f16 (the trunk's last conv5).
int run_rdb(void* D, void* next, float* xr, float* xrr, const srbh_conv_w* cw, int B, int H, int W, bool bf16, bool out_f16, void* stream) {
    int rc;
    for (int k = 0; k < 4; ++k) {
        const srbh_conv3x3_args a = growth_conv(D, k, cw[k], B, H, W);
        if ((rc = bf16 ? conv3x3_trunk_b16(&a, 0, stream) : srbh_conv3x3_f16(&a, stream))) return rc;
    }
    const srbh_conv3x3_args a = conv5(D, next, xr, xrr, cw[4], B, H, W);
    return bf16 ? conv3x3_trunk_b16(&a, out_f16 ? 1 : 0, stream) : srbh_conv3x3_f16(&a, stream);
}

// One tail conv: `a` describes the (hi) operands and the outputs; when split, the lo' planes of its input (2 planes from in_lo_chunk0), the
// lo' pack and where the lo' planes of its output go (out_lo NULL: none) join it and the conv runs on split fp16 operands
int run_tail_conv(const srbh_conv3x3_args& a, bool split, const void* in_lo, int in_lo_chunks_total, int in_lo_chunk0, const void* w_lo,
                  void* out_lo, int out_lo_chunks_total, int out_lo_chunk0, void* stream) {
    if (!split) return srbh_conv3x3_f16(&a, stream);
    srbh_conv3x3_split s{};
    s.in_lo = in_lo; s.in_lo_chunks_total = in_lo_chunks_total; s.in_lo_chunk0 = in_lo_chunk0;
    s.w_lo = w_lo;
    s.out16_lo = out_lo; s.out16_lo_chunks_total = out_lo_chunks_total; s.out16_lo_chunk0 = out_lo_chunk0;
    return srbh_conv3x3_f16x2(&a, &s, stream);
}

WsLayout ws_layout(int B, int H, int W, int want_forward, bool f16x2 = false) {
    WsLayout L;
    size_t off = 0;
    L.dense_b = act16_geo(B, 6, H, W).total_b;
    L.d0 = off; off = align256(off + L.dense_b);
    L.d1 = off; off = align256(off + L.dense_b);
    size_t res_b = (size_t)B * H * W * 64 * sizeof(float);
    L.feat = off; off = align256(off + res_b);
    L.xr = off; off = align256(off + res_b);
    L.xrr = off; off = align256(off + res_b);
    L.u2 = off; off = align256(off + act16_geo(B, 2, 2 * H, 2 * W).total_b);
    L.u3 = off; off = align256(off + act16_geo(B, 2, 4 * H, 4 * W).total_b);
    L.u4 = off;
    if (want_forward == 1) off = align256(off + act16_geo(B, 2, 4 * H, 4 * W).total_b);      // (2 = forward_feature as fp16: no conv_last)
    L.aux = off;   // persistent-trunk layer table, progress counters, error word
    off = align256(off + ptrunk_aux_bytes(B, tiles_per_img(H)));
    L.u2lo = L.u3lo = off;
    if (f16x2) {      // every offset above is the default layout's: srbh_rrdbnet_last_status / srbh_rrdbnet_trunk_out need not know the mode
        L.u2lo = off; off = align256(off + act16_geo(B, 2, 2 * H, 2 * W).total_b);
        L.u3lo = off; off = align256(off + act16_geo(B, 2, 4 * H, 4 * W).total_b);
    }
    L.total = off;
    return L;
}

}  // namespace

extern "C" size_t srbh_rrdbnet_workspace_bytes(int B, int H, int W, int want_forward) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return ws_layout(B, H, W, want_forward).total;
}

extern "C" size_t srbh_rrdbnet_workspace_bytes_f16x2(int B, int H, int W, int want_forward) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return ws_layout(B, H, W, want_forward, true).total;
}

extern "C" int srbh_rrdbnet_forward(const srbh_rrdbnet_desc* d, const float* x, float* out, int B, int H, int W,
                                    int want_forward, void* ws, size_t ws_bytes, void* stream) {
    SRBH_REQUIRE(d && x && out && ws, "srbh_rrdbnet_forward: null pointer");
    SRBH_REQUIRE(B > 0 && H > 0 && W > 0, "srbh_rrdbnet_forward: bad geometry B=%d H=%d W=%d", B, H, W);
    SRBH_REQUIRE(d->num_block >= 0 && d->rdb != nullptr, "srbh_rrdbnet_forward: bad descriptor");
    const bool split = d->tail_f16x2 != 0;
    SRBH_REQUIRE(!split || (d->conv_body_lo && d->conv_up1_lo && d->conv_up2_lo && d->conv_hr_lo),
                 "srbh_rrdbnet_forward: the f16x2 mode needs the lo' packs of conv_body, conv_up1, conv_up2 and conv_hr");
    SRBH_REQUIRE(!split || want_forward != 1, "srbh_rrdbnet_forward: the f16x2 mode computes forward_feature only (want_forward 0 or 2)");
    const WsLayout L = ws_layout(B, H, W, want_forward, split);
    if (ws_bytes < L.total) {
        set_error("srbh_rrdbnet_forward: workspace %zu bytes < required %zu", ws_bytes, L.total);
        return SRBH_ERR_WORKSPACE;
    }
    char* base = (char*)ws;
    void* D[2] = {base + L.d0, base + L.d1};
    float* feat = (float*)(base + L.feat);
    float* xr = (float*)(base + L.xr);
    float* xrr = (float*)(base + L.xrr);
    void* U2 = base + L.u2;
    void* U3 = base + L.u3;
    void* U4 = base + L.u4;

    // The dense blocks run on bf16 operands when the descriptor carries bf16 packs of the trunk convs (d->rdb_b16) and SRBH_TRUNK_BF16 is not
    // "0".  conv_first writes the trunk's first planes as bf16, every dense-block conv rounds its 16-bit output to bf16, and the last conv5
    // rounds the trunk's output planes to fp16 (the fp32 RRDB streams are fp32 either way): conv_body onwards runs on exactly the fp16 path.
    // Persistent and per-layer forms compute the same bits in both precisions.
    const bool bf16 = d->rdb_b16 && d->num_block > 0 && !env_off("SRBH_TRUNK_BF16");
    int rc = conv_first_f32(x, d->conv_first_w, d->conv_first_b, B, d->num_in_ch, H, W, feat, xr, xrr, D[0], 6, bf16 ? 1 : 0, stream);
    if (rc) return rc;

    int cur = 0;
    int used_persistent = 0;
    if (!env_off("SRBH_PERSISTENT")) {
        srbh_rrdbnet_desc dt = *d;
        if (bf16) dt.rdb = d->rdb_b16;
        rc = ptrunk_run(&dt, D[0], D[1], xr, xrr, B, H, W, base + L.aux, (hipStream_t)stream, &used_persistent, &cur, 0, nullptr, 0, bf16);
        if (rc) return rc;
    }
    const int n_rdb = d->num_block * 3;
    for (int i = 0; !used_persistent && i < n_rdb; ++i) {      // per layer: the dense buffers ping-pong
        const srbh_conv_w* cw = (bf16 ? d->rdb_b16 : d->rdb) + i * 5;
        if ((rc = run_rdb(D[cur], D[cur ^ 1], xr, i % 3 == 2 ? xrr : nullptr, cw, B, H, W, bf16, i + 1 == n_rdb, stream))) return rc;
        cur ^= 1;
    }

    // The tail.  On split fp16 operands (the f16x2 mode, srbh_ptail_split.hip) the hi planes live where the default mode keeps its planes; lo'
    // planes: planes 2..3 of the dense buffers (x1 / x2 of the last dense block: dead behind the trunk) and the two buffers behind the default
    // layout.  conv_body's hi planes are the trunk's own fp16 output planes, its lo' planes what those leave of the fp32 stream xrr.
    void* U2lo = base + L.u2lo;
    void* U3lo = base + L.u3lo;
    if (split && (rc = srbh_act16_split_lo(xrr, used_persistent, D[cur], 6, 0, D[cur], 6, 2, B, H, W, stream))) return rc;
    srbh_conv3x3_args a = tail_conv(D[cur], 6, d->conv_body, B, H, W, 0, 0);      // conv_body + trunk skip
    a.skip = feat;
    out_planes(a, D[cur ^ 1], 6, 0);
    if ((rc = run_tail_conv(a, split, D[cur], 6, 2, d->conv_body_lo, D[cur ^ 1], 6, 2, stream))) return rc;
    a = tail_conv(D[cur ^ 1], 6, d->conv_up1, B, 2 * H, 2 * W, 1, 1);      // conv_up1 / conv_up2 read through the nearest-x2 index map
    out_planes(a, U2, 2, 0);
    if ((rc = run_tail_conv(a, split, D[cur ^ 1], 6, 2, d->conv_up1_lo, U2lo, 2, 0, stream))) return rc;
    a = tail_conv(U2, 2, d->conv_up2, B, 4 * H, 4 * W, 1, 1);
    out_planes(a, U3, 2, 0);
    if ((rc = run_tail_conv(a, split, U2lo, 2, 0, d->conv_up2_lo, U3lo, 2, 0, stream))) return rc;
    // conv_hr, in the form the caller asked for
    a = tail_conv(U3, 2, d->conv_hr, B, 4 * H, 4 * W, 0, 0);
    const bool full = want_forward && want_forward != 2 && !split;
    int out_c = 64;
    if (want_forward == 2) {      // forward_feature as a dense fp16 NHWC tensor (the 16-bit head kernels stage it verbatim), rounded once
        out_planes(a, out, 2, 0);
        a.out16_nhwc = 1;
        out_c = 32;               // (64 halves = 32 words per pixel)
    } else if (!full) {           // forward_feature, fp32 NHWC
        a.out32 = out; a.out32_c = 64;
    } else {                      // forward: lrelu(conv_hr) as 16-bit planes for conv_last
        a.lrelu = 1;
        out_planes(a, U4, 2, 0);
    }
    if ((rc = run_tail_conv(a, split, U3lo, 2, 0, d->conv_hr_lo, nullptr, 0, 0, stream))) return rc;
    if (full) {
        SRBH_REQUIRE(d->conv_last.w && d->num_out_ch >= 1 && d->num_out_ch <= 32,
                     "srbh_rrdbnet_forward: conv_last needs 1..32 output channels (got %d)", d->num_out_ch);
        a = conv_on(U4, 2, 2, d->conv_last.w, d->conv_last.bias, 32, B, 4 * H, 4 * W);
        a.out32 = out; a.out32_c = out_c = d->num_out_ch;
        if ((rc = srbh_conv3x3_f16(&a, stream))) return rc;
    }
    if (!used_persistent) return SRBH_OK;
    return poison_on_error(ptrunk_err_word(base + L.aux, B, H), out, (size_t)B * 16 * H * W * out_c, 1024, (hipStream_t)stream);
}

/* The trunk's fp32 output -- `xrr` behind the last RRDB, what conv_body's input planes are the fp16 rounding of -- copied out of a workspace
 * that srbh_rrdbnet_forward has just run on, as NHWC [B][H][W][64].  The tail never touches that stream, so it is still there; its ORDER
 * depends on the form that ran (per-layer: pixel order; persistent kernel: fragment order per image row), which is decided here exactly as
 * the forward decides it (SRBH_PERSISTENT read now, ptrunk_takes).  Read only on `ws`.  num_block == 0: conv_first's output. */
extern "C" int srbh_rrdbnet_trunk_out(const void* ws, size_t ws_bytes, int num_block, int B, int H, int W, int want_forward, float* out,
                                      void* stream) {
    SRBH_REQUIRE(ws && out && B > 0 && H > 0 && W > 0 && num_block >= 0, "srbh_rrdbnet_trunk_out: bad arguments");
    const WsLayout L = ws_layout(B, H, W, want_forward);
    if (ws_bytes < L.total) {
        set_error("srbh_rrdbnet_trunk_out: workspace %zu bytes < required %zu", ws_bytes, L.total);
        return SRBH_ERR_WORKSPACE;
    }
    const float* xrr = (const float*)((const char*)ws + L.xrr);
    const size_t n = (size_t)B * H * W * 64;
    int fragment = 0;
    if (!env_off("SRBH_PERSISTENT")) {
        if (int rc = ptrunk_takes(num_block, H, W, &fragment, nullptr)) return rc;
    }
    if (!fragment) {
        SRBH_HIP(hipMemcpyAsync(out, xrr, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return SRBH_OK;
    }
    const long nquads = (long)(n / 4);       // (W == 64 here: 1024 float4 per image row)
    hipLaunchKernelGGL(trunk_out_pixel_order_kernel, dim3((unsigned)((nquads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, xrr, out, nquads);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}

extern "C" int srbh_rrdbnet_last_status(const void* ws, int B, int H, int W, int want_forward, void* stream) {
    SRBH_REQUIRE(ws && B > 0 && H > 0 && W > 0, "srbh_rrdbnet_last_status: bad arguments");
    const WsLayout L = ws_layout(B, H, W, want_forward);
    SRBH_HIP(hipStreamSynchronize((hipStream_t)stream));
    int err = 0;
    SRBH_HIP(hipMemcpy(&err, ptrunk_err_word((const char*)ws + L.aux, B, H), sizeof(int), hipMemcpyDeviceToHost));
    if (err) set_error("persistent trunk kernel timed out waiting for a neighbour workgroup (err=%d)", err);
    return err ? -3 : SRBH_OK;
}


// ---- training path of the trunk (second slice; host mirror: rrdbnet_autograd.py "fast") -------------------------------
// The two loops below are the per-layer launch sequence above with every RDB's dense buffer KEPT (forward) and its mirror image on
// gradients (backward); they live here rather than in Python because at batch 8 a step is ~2 400 launches of a few microseconds each
// and the ctypes call overhead (~10 us) was the whole runtime.
extern "C" int srbh_rrdbnet_trunk_train_forward(const srbh_rrdbnet_desc* d, float* xr, float* xrr, void* dense_all, size_t dense_stride,
                                                int B, int H, int W, void* stream) {
    SRBH_REQUIRE(d && d->rdb && xr && xrr && dense_all && B > 0 && H > 0 && W > 0, "srbh_rrdbnet_trunk_train_forward: bad arguments");
    // xr == xrr == feat on entry (the caller's copies); dense buffer 0 receives feat as fp16 planes 0..1
    int rc = srbh_nhwc32_to_act16(xr, dense_all, B, 64, H, W, 6, 0, 1.0f, 0, stream);
    if (rc) return rc;
    const int n_rdb = d->num_block * 3;
    for (int i = 0; i < n_rdb; ++i) {      // a row of dense buffers: RDB i keeps its own
        char* D = (char*)dense_all + (size_t)i * dense_stride;
        if ((rc = run_rdb(D, D + dense_stride, xr, i % 3 == 2 ? xrr : nullptr, d->rdb + i * 5, B, H, W, false, false, stream))) return rc;
    }
    return SRBH_OK;
}

/* The same forward as ONE launch of the persistent trunk kernel (round 5): the inference trunk's ptrunk3_kernel walking a row of dense buffers
 * (RDB i in dense_all + i * dense_stride) with every plane stored whole, its fp32 output written to xr in pixel order.  Same arithmetic in the
 * same order as the per-layer sequence above: xr and every saved plane come out bit-identical (tests/test_sr_stage.py).  aux: scratch of
 * srbh_rrdbnet_trunk_train_aux_bytes(B, H, W) bytes (0 = this geometry is not the kernel's: 64-pixel-wide tiles, H %% 8 == 0).  *used = 0:
 * nothing was launched, call srbh_rrdbnet_trunk_train_forward.  A halo-exchange timeout (never seen) turns xr into NaN. */
extern "C" size_t srbh_rrdbnet_trunk_train_aux_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W != TILE_W || (H % TILE_H) != 0) return 0;
    return ptrunk_aux_bytes(B, tiles_per_img(H));
}
extern "C" int srbh_rrdbnet_trunk_train_forward_persistent(const srbh_rrdbnet_desc* d, float* xr, float* xrr, void* dense_all, size_t dense_stride,
                                                           int B, int H, int W, void* aux, void* stream, int* used) {
    SRBH_REQUIRE(d && d->rdb && xr && xrr && dense_all && aux && used && B > 0 && H > 0 && W > 0 && dense_stride > 0,
                 "srbh_rrdbnet_trunk_train_forward_persistent: bad arguments");
    *used = 0;
    static const bool off = env_off("SRBH_SR_PTRUNK");
    if (off || srbh_rrdbnet_trunk_train_aux_bytes(B, H, W) == 0) return SRBH_OK;
    int rc = srbh_nhwc32_to_act16(xr, dense_all, B, 64, H, W, 6, 0, 1.0f, 0, stream);      // dense buffer 0 <- feat as fp16 planes 0..1 (xr == xrr == feat)
    if (rc) return rc;
    int cur = 0;
    if ((rc = ptrunk_run(d, dense_all, nullptr, xr, xrr, B, H, W, aux, (hipStream_t)stream, used, &cur, (long)dense_stride))) return rc;
    if (!*used) return SRBH_OK;
    return poison_on_error(ptrunk_err_word(aux, B, H), xr, (size_t)B * H * W * 64, 256, (hipStream_t)stream);
}

namespace {
struct SideStream {
    hipStream_t s = nullptr;
    hipEvent_t ready[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
    int dev = -1;
};
SideStream g_side;
int side_init() {
    int dev = 0;
    SRBH_HIP(hipGetDevice(&dev));
    if (g_side.s && g_side.dev == dev) return SRBH_OK;
    SRBH_HIP(hipStreamCreateWithFlags(&g_side.s, hipStreamNonBlocking));
    for (int k = 0; k < 2; ++k) {
        SRBH_HIP(hipEventCreateWithFlags(&g_side.ready[k], hipEventDisableTiming));
        SRBH_HIP(hipEventCreateWithFlags(&g_side.done[k], hipEventDisableTiming));
    }
    g_side.dev = dev;
    return SRBH_OK;
}

// A dense block's convs on the gradient side, conv1..conv5: first channel of the conv's output gradient in the G buffer (and in the RDB's 192
// floats of db_all: G order [g5 (64) | g4 | g3 | g2 | g1]), its cout and cin, and where its OIHW weights start in the RDB's DW_RDB floats of dw_all
constexpr int CH0[5] = {160, 128, 96, 64, 0}, COUT[5] = {32, 32, 32, 32, 64}, CIN[5] = {64, 96, 128, 160, 192};
constexpr long DWOFF[5] = {0, 9L * 2048, 9L * (2048 + 3072), 9L * (2048 + 3072 + 4096), 9L * (2048 + 3072 + 4096 + 5120)};
constexpr long DW_RDB = 9L * 26624;

// The bias gradients (channel sums of G) and the five weight gradients of RDB i, from its saved buffer D and its complete G buffer.  defer: each
// weight gradient into its own slice of `ws`, their ordered reduces queued and done by ONE pair of launches (round 5: five reduce launches of
// ~9 us per block sat on the stream that bounds the backward); otherwise each reduce follows its launch and `ws` is reused.
int rdb_wgrad(int i, const void* D, const void* G, int B, int H, int W, float* dw_all, float* db_all, float* ws, bool defer, void* stream) {
    int rc;
    if ((rc = srbh_act16_channel_sum(G, B, H, W, 6, 0, 6, 1, db_all + (long)i * 192, stream))) return rc;
    if (defer && (rc = srbh_hwgrad_defer(1))) return rc;
    size_t woff = 0;
    for (int k = 0; k < 5; ++k) {
        rc = srbh_act16_wgrad_b16(D, 6, CIN[k], G, 6, CH0[k], COUT[k], B, H, W, dw_all + (long)i * DW_RDB + DWOFF[k], ws + woff, stream);
        if (rc) { if (defer) srbh_hwgrad_flush(stream); return rc; }
        if (defer) woff += srbh_hwgrad_ws_bytes(COUT[k], CIN[k], 3) / sizeof(float);
    }
    return defer ? srbh_hwgrad_flush(stream) : SRBH_OK;
}
}  // namespace

/* bytes of `wgrad_ws` for srbh_rrdbnet_trunk_train_backward: the partial-sum workspaces of a dense block's five weight gradients side by side */
extern "C" size_t srbh_rrdbnet_trunk_wgrad_ws_bytes(void) {
    size_t n = 0;
    for (int k = 0; k < 5; ++k) n += srbh_hwgrad_ws_bytes(COUT[k], CIN[k], 3);
    return n;
}

// g_a: gradient of the trunk output on entry (fp32 NHWC64); g_b, g_c: scratch of the same size.  Returns the gradient of the trunk
// input in *g_out (one of the three).  packs: per RDB `pack_stride` bytes, gradient conv j (dX4, dX3, dX2, dX1, dx) at pack_off[j].
// dw_all: per RDB 239 616 floats in conv1..conv5 order (OIHW each); db_all: per RDB 192 floats in G order [g5 (64) | g4 | g3 | g2 | g1].
// The weight / bias gradients of RDB i only READ what the gradient convs of RDB i produced (G) and the saved planes: they run on a
// side stream next to the gradient convs of RDB i-1 -- at small batch a conv launch fills a quarter of the chip (64 workgroups at
// batch 8), so the two chains overlap almost completely.  G is double buffered for that (G and G + g_stride).
extern "C" int srbh_rrdbnet_trunk_train_backward(int num_block, const void* dense_all, size_t dense_stride, const void* packs, size_t pack_stride,
                                                 const size_t* pack_off, float* g_a, float* g_b, float* g_c, float** g_out, void* G, size_t g_stride,
                                                 float* dw_all, float* db_all, float* wgrad_ws, int B, int H, int W, void* stream) {
    SRBH_REQUIRE(num_block > 0 && dense_all && packs && pack_off && g_a && g_b && g_c && g_out && G && dw_all && db_all && wgrad_ws,
                 "srbh_rrdbnet_trunk_train_backward: null pointer");
    const long n = (long)B * H * W * 64;
    static const bool overlap = !env_off("SRBH_SR_OVERLAP");
    static const bool batch_red = !env_off("SRBH_SR_BATCH_REDUCE");
    const bool two = overlap && g_stride > 0;
    hipStream_t st = (hipStream_t)stream;
    if (two) { if (int rc0 = side_init()) return rc0; }
    hipStream_t ws_st = two ? g_side.s : st;
    float* gout = g_a;            // gradient of the current RRDB's output
    float* cur = g_b;             // gradient flowing down the RDBs
    float* nxt = g_c;
    int rc;
    int i = num_block * 3;
    int used[2] = {0, 0};
    for (int blk = num_block - 1; blk >= 0; --blk) {
        if ((rc = srbh_axpby_f32(cur, 0.2f, gout, 0.f, nullptr, n, stream))) return rc;        // out = rdb3(.) * 0.2 + x_rrdb
        for (int r = 2; r >= 0; --r) {
            --i;
            const int gb = two ? (i & 1) : 0;
            char* Gi = (char*)G + (size_t)gb * g_stride;
            const char* D = (const char*)dense_all + (size_t)i * dense_stride;
            const char* pk = (const char*)packs + (size_t)i * pack_stride;
            if (two && used[gb]) SRBH_HIP(hipStreamWaitEvent(st, g_side.done[gb], 0));          // the side stream is done reading this G
            if ((rc = srbh_nhwc32_to_act16(cur, Gi, B, 64, H, W, 6, 0, 0.2f, 1, stream))) return rc;        // g5 = 0.2 g (bf16)
            for (int j = 0; j < 4; ++j) {          // g4 .. g1: masked by the saved planes X4 .. X1
                const srbh_conv3x3_args a = grad_conv(Gi, j, pk + pack_off[j], B, H, W);
                if ((rc = srbh_conv3x3_x16(&a, 1, D, 6, 5 - j, stream))) return rc;
            }
            // G of this RDB is complete.  One stream: dx, then the weight / bias gradients.  Two: those start on the side stream first and dx is
            // issued behind their launches, to run beside them.
            const srbh_conv3x3_args dx = grad_conv(Gi, 4, pk + pack_off[4], B, H, W, cur, nxt);
            if (!two && (rc = srbh_conv3x3_x16(&dx, 1, nullptr, 0, 0, stream))) return rc;
            if (two) {
                SRBH_HIP(hipEventRecord(g_side.ready[gb], st));
                SRBH_HIP(hipStreamWaitEvent(ws_st, g_side.ready[gb], 0));
            }
            if ((rc = rdb_wgrad(i, D, Gi, B, H, W, dw_all, db_all, wgrad_ws, batch_red, ws_st))) return rc;
            if (two) {
                SRBH_HIP(hipEventRecord(g_side.done[gb], ws_st));
                used[gb] = 1;
            }
            if (two && (rc = srbh_conv3x3_x16(&dx, 1, nullptr, 0, 0, stream))) return rc;
            float* t = cur; cur = nxt; nxt = t;
        }
        // the RRDB's skip connection: gradient of the RRDB input = cur + gout; it is the next (lower) RRDB's output gradient
        if ((rc = srbh_axpby_f32(nxt, 1.f, cur, 1.f, gout, n, stream))) return rc;
        float* t = gout; gout = nxt; nxt = t;
    }
    if (two)      // join: everything the side stream wrote (dw_all, db_all) is ordered before what follows on `stream`
        for (int k = 0; k < 2; ++k)
            if (used[k]) SRBH_HIP(hipStreamWaitEvent(st, g_side.done[k], 0));
    *g_out = gout;
    return SRBH_OK;
}

/* The same backward with the 345 data-gradient convs as ONE launch of the persistent trunk kernel (round 5; ptrunk3_kernel<., 1>): the gradient of a
 * dense block is a dense block on gradients, so the launch walks the RDBs in reverse over a ROW of G buffers (G_all + k * g_stride for the k-th RDB
 * from the end; n_rdb + 1 buffers, zero borders) with the saved forward buffers as LeakyReLU masks, and the weight / bias gradients of all RDBs
 * follow on two streams.  The kernel's residual recurrences are the forward's: it runs on x = 0.04 g (g = gradient of the trunk output), where
 *   x' = 0.2 conv5(G) + x         is  0.2 (dx + cur)  with  x = 0.2 cur  (cur = gradient entering the RDB: dx's `skip` above), and
 *   x  = 0.2 x + x_rrdb           is  the RRDB's skip  (cur + gout) / 25  with  x_rrdb = gout / 25,
 * so every g5 plane the weight gradients read comes out at its true scale and the result is 25 x the launch's output.  Same operands (bf16, RNE)
 * and the same accumulation order per conv as the per-layer form; the fp32 streams differ from it in the last bit (0.2 applied to conv5's sum,
 * not to the stream).  zero_bias: >= 64 zero floats.  wgrad_ws: TWO workspaces of srbh_rrdbnet_trunk_wgrad_ws_bytes(); trunk_wgrad_ws: srbh_trunk_wgrad_ws_bytes()
 * bytes (the one-launch weight gradients; NULL = the general kernel RDB by RDB through wgrad_ws).  aux: the scratch of the
 * persistent forward.  g_a is read, g_b / g_c are scratch; *g_out = the gradient of the trunk input (one of g_b, g_c).  *used = 0: nothing was
 * launched (geometry not the kernel's, or SRBH_SR_PTRUNK_BWD=0): call srbh_rrdbnet_trunk_train_backward. */
extern "C" int srbh_rrdbnet_trunk_train_backward_persistent(int num_block, const void* dense_all, size_t dense_stride, const void* packs, size_t pack_stride,
                                                            const size_t* pack_off, const float* zero_bias, const float* g_a, float* g_b, float* g_c,
                                                            float** g_out, void* G_all, size_t g_stride, float* dw_all, float* db_all, float* wgrad_ws,
                                                            void* trunk_wgrad_ws, int B, int H, int W, void* aux, void* stream, int* used) {
    SRBH_REQUIRE(num_block > 0 && dense_all && packs && pack_off && zero_bias && g_a && g_b && g_c && g_out && G_all && dw_all && db_all && wgrad_ws && aux && used &&
                 dense_stride > 0 && g_stride > 0, "srbh_rrdbnet_trunk_train_backward_persistent: bad arguments");
    *used = 0;
    static const bool off = env_off("SRBH_SR_PTRUNK_BWD");
    if (off || srbh_rrdbnet_trunk_train_aux_bytes(B, H, W) == 0) return SRBH_OK;
    const long n = (long)B * H * W * 64;
    const int n_rdb = num_block * 3;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = srbh_axpby_f32(g_b, 0.04f, g_a, 0.f, nullptr, n, stream))) return rc;
    if ((rc = srbh_axpby_f32(g_c, 0.04f, g_a, 0.f, nullptr, n, stream))) return rc;
    if ((rc = srbh_nhwc32_to_act16(g_a, G_all, B, 64, H, W, 6, 0, 0.04f, 1, stream))) return rc;      // g5 of the last RDB (bf16)
    std::vector<srbh_conv_w> cw((size_t)n_rdb * 5);
    for (int k = 0; k < n_rdb; ++k)
        for (int j = 0; j < 5; ++j) {
            cw[(size_t)k * 5 + j] = srbh_conv_w{};
            cw[(size_t)k * 5 + j].w = (const char*)packs + (size_t)(n_rdb - 1 - k) * pack_stride + pack_off[j];
            cw[(size_t)k * 5 + j].bias = zero_bias;
        }
    srbh_rrdbnet_desc dd = {};
    dd.num_block = num_block;
    dd.rdb = cw.data();
    int cur = 0;
    if ((rc = ptrunk_run(&dd, G_all, nullptr, g_b, g_c, B, H, W, aux, st, used, &cur, (long)g_stride,
                         (const char*)dense_all + (size_t)(n_rdb - 1) * dense_stride, -(long)dense_stride))) return rc;
    if (!*used) return SRBH_OK;
    if ((rc = poison_on_error(ptrunk_err_word(aux, B, H), g_b, (size_t)n, 256, st))) return rc;
    if ((rc = srbh_axpby_f32(g_c, 25.f, g_b, 0.f, nullptr, n, stream))) return rc;
    *g_out = g_c;
    // weight / bias gradients of all RDBs: one launch over (RDB, plane pair, tile range) + one reduce (srbh_trunk_wgrad.hip) ...
    static const bool one_launch = !env_off("SRBH_SR_TRUNK_WGRAD");
    if (trunk_wgrad_ws && one_launch) return srbh_trunk_wgrad(num_block, dense_all, dense_stride, G_all, g_stride, B, H, W, dw_all, db_all, trunk_wgrad_ws, stream);
    // ... or (no workspace given / SRBH_SR_TRUNK_WGRAD=0) RDB by RDB with the general kernel, alternating between the caller's stream and the side stream (a weight-gradient launch fills the chip; the
    // small reduces and plane sums of one RDB run beside the next RDB's)
    static const bool overlap = !env_off("SRBH_SR_OVERLAP");
    if (overlap) {
        if ((rc = side_init())) return rc;
        SRBH_HIP(hipEventRecord(g_side.ready[0], st));
        SRBH_HIP(hipStreamWaitEvent(g_side.s, g_side.ready[0], 0));
    }
    const size_t ws_floats = srbh_rrdbnet_trunk_wgrad_ws_bytes() / sizeof(float);
    for (int k = 0; k < n_rdb; ++k) {
        const int i = n_rdb - 1 - k;                 // forward index of the RDB whose gradients sit in G buffer k
        const bool on_side = overlap && (k & 1);
        if ((rc = rdb_wgrad(i, (const char*)dense_all + (size_t)i * dense_stride, (const char*)G_all + (size_t)k * g_stride, B, H, W, dw_all, db_all,
                            wgrad_ws + (on_side ? ws_floats : 0), true, on_side ? g_side.s : st))) return rc;
    }
    if (overlap) {
        SRBH_HIP(hipEventRecord(g_side.done[0], g_side.s));
        SRBH_HIP(hipStreamWaitEvent(st, g_side.done[0], 0));
    }
    return SRBH_OK;
}
