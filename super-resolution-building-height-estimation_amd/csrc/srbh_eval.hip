// srbh_eval.hip -- the validation / test pass of the height stage as ONE read of a batch (reference train.py:315-344 vtest_epoch,
// :427-486 vtest_epoch2, metrics.py:67-74 genConfusionMatrix, :186-200 HeightMetric.addBatch).
//
// The reference scores a batch in pieces: argmax to an int64 map, a bincount over two int64 maps, seven boolean-mask gathers with three
// reductions each, and two more reductions for the RMSE.  Here one kernel reads height, logits, reference height and label once and leaves,
// PER IMAGE (nothing is summed over the batch, so a caller can regroup the images into the reference loader's batches afterwards):
//   sums[b][k][4]  float64: sum d^2, sum |d|, sum d, count over the pixels of label class k, d = (double)pred - (double)ref
//   cm[b][label][pred] int64: pred = argmax of the pixel's C logits under torch's rule (first index among equal maxima; a NaN is the
//                  maximum, the first NaN wins)
//   bad            sticky int: a label outside [0, C) was seen (such a pixel is counted nowhere)
//   q_height       uint16 = np.round(max(h, 0) * 10), half to even (train.py:464-466; the arithmetic of srbh_mosaic.hip)   [optional]
//   cls_map        uint8  = the argmax (train.py:476)                                                                      [optional]
//
// Form: a workgroup of 256 threads owns EV_RANGE = 4096 consecutive pixels of one image and takes them in four rounds of 1024; in a round
// thread t takes pixels t, t + 256, t + 512, t + 768, so the 64 lanes of a wave read 64 consecutive pixels of every plane (NCHW: 256
// contiguous bytes per load and plane; channels_last: the wave's C loads together cover one contiguous run of 64 C floats).  All loads of
// a round are issued before the first use.  The float64 partial sums of a thread stay in registers, selected by class with an unrolled
// compare-and-add (no register is indexed dynamically); the lanes are folded once at the end (wave shuffles, then four LDS words per
// value) and the workgroup writes its slot of the caller's workspace; a small fold kernel adds an image's slots in slot order.  The confusion counts are an integer LDS histogram (integer
// sums have no order); the count of class k is the sum of row k of the matrix.  No floating-point atomics: the pixel -> workgroup map and
// every summation order depend on H*W only, so results are bit-identical from run to run, for an image alone or in any batch, and for
// either logits layout.
#include "srbh_internal.h"

namespace {
using namespace srbh;

constexpr int EV_PPT = 4;                      // pixels a thread has in flight: loaded together, then scored
constexpr int EV_ITERS = 4;                    // such rounds per workgroup
constexpr int EV_RANGE = 256 * EV_PPT * EV_ITERS;      // pixels per workgroup: 4096

struct EvalParams {
    const float* height; long height_bs;
    const float* logits; long lbs, lcs, lps;
    const float* ref;
    const void* label;
    int C, HW, nslots;
    double* ws_d;            // [B][nslots][C][3]
    unsigned* ws_i;          // [B][nslots][C*C]
    int* bad;
    unsigned short* q_height;
    unsigned char* cls_map;
};

template <int CMAX, bool U8>
__global__ __launch_bounds__(256) void eval_kernel(const EvalParams p) {
    __shared__ unsigned hist[CMAX * CMAX];
    __shared__ double red[4][CMAX * 3];
    __shared__ int sbad;
    const int t = threadIdx.x, b = blockIdx.y, slot = blockIdx.x, C = p.C;
    for (int i = t; i < CMAX * CMAX; i += 256) hist[i] = 0u;
    if (t == 0) sbad = 0;
    __syncthreads();

    const float* hp = p.height + (long)b * p.height_bs;
    const float* rp = p.ref + (long)b * p.HW;
    const float* lp = p.logits + (long)b * p.lbs;
    double s2[CMAX], s1[CMAX], s0[CMAX];
#pragma unroll
    for (int k = 0; k < CMAX; ++k) s2[k] = s1[k] = s0[k] = 0.0;
#pragma unroll 1
    for (int it = 0; it < EV_ITERS; ++it) {
        // (nslots * EV_RANGE < HW + EV_RANGE: no overflow for HW <= 2^30, checked by the host)
        const int p0 = slot * EV_RANGE + it * (256 * EV_PPT);
        if (p0 >= p.HW) break;      // uniform
        float hv[EV_PPT], rv[EV_PPT], lv[EV_PPT][CMAX];
        int lab[EV_PPT];
#pragma unroll
        for (int i = 0; i < EV_PPT; ++i) {
            const int px = p0 + i * 256 + t;
            const bool in = px < p.HW;
            hv[i] = in ? hp[px] : 0.f;
            rv[i] = in ? rp[px] : 0.f;
            long long l = -1;
            if (in) l = U8 ? (long long)((const unsigned char*)p.label)[(long)b * p.HW + px] : ((const long long*)p.label)[(long)b * p.HW + px];
            lab[i] = (l >= 0 && l < C) ? (int)l : -1;
            if (in && lab[i] < 0) sbad = 1;        // (every writer stores the same value)
            const float* q = lp + (long)px * p.lps;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) lv[i][c] = (in && c < C) ? q[(long)c * p.lcs] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < EV_PPT; ++i) {
            const int px = p0 + i * 256 + t;
            if (px >= p.HW) continue;
            // torch.argmax: the first maximum; a NaN beats every number and the first NaN stays
            float best = lv[i][0];
            int arg = 0;
#pragma unroll
            for (int c = 1; c < CMAX; ++c) {
                const float v = lv[i][c];
                if (c < C && best == best && (v > best || v != v)) { best = v; arg = c; }
            }
            if (p.cls_map) p.cls_map[(long)b * p.HW + px] = (unsigned char)arg;
            if (p.q_height) {
                float h = hv[i];
                h = h < 0.f ? 0.f : h;                                                  // tmp[tmp<0] = 0
                p.q_height[(long)b * p.HW + px] = (unsigned short)(((unsigned)rintf(h * 10.f)) & 0xffffu);   // np.round(tmp*10).astype('uint16')
            }
            const int l = lab[i];
            if (l < 0) continue;
            atomicAdd(&hist[l * C + arg], 1u);
            const double d = (double)hv[i] - (double)rv[i];
            const double dd = d * d, ad = fabs(d);
#pragma unroll
            for (int k = 0; k < CMAX; ++k) {
                const bool m = l == k;
                s2[k] += m ? dd : 0.0;
                s1[k] += m ? ad : 0.0;
                s0[k] += m ? d : 0.0;
            }
        }
    }

    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int k = 0; k < CMAX; ++k) {
        if (k < C) {      // uniform
            double x = s2[k], y = s1[k], z = s0[k];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { x += __shfl_down(x, o, 64); y += __shfl_down(y, o, 64); z += __shfl_down(z, o, 64); }
            if (lane == 0) { red[wave][k * 3] = x; red[wave][k * 3 + 1] = y; red[wave][k * 3 + 2] = z; }
        }
    }
    __syncthreads();
    const long s = (long)b * p.nslots + slot;
    if (t < C * 3) p.ws_d[s * (C * 3) + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    if (t < C * C) p.ws_i[s * (C * C) + t] = hist[t];
    if (t == 0 && sbad) atomicOr(p.bad, 1);
}

// one block per image: cm[b] = the sum of the image's histograms, sums[b][k] = its slots added in slot order, count = row sum of cm
__global__ __launch_bounds__(256) void eval_fold_kernel(const double* __restrict__ ws_d, const unsigned* __restrict__ ws_i, int nslots, int C,
                                                        double* sums, long long* cm) {
    __shared__ long long scm[256];
    const int t = threadIdx.x, b = blockIdx.x;
    const long s0 = (long)b * nslots;
    if (t < C * C) {
        long long a = 0;
#pragma unroll 8
        for (int k = 0; k < nslots; ++k) a += ws_i[(s0 + k) * (C * C) + t];
        cm[(long)b * C * C + t] = a;
        scm[t] = a;
    }
    __syncthreads();
    if (t < C * 4) {
        const int k = t >> 2, j = t & 3;
        double v = 0.0;
        if (j < 3) {
#pragma unroll 8
            for (int q = 0; q < nslots; ++q) v += ws_d[(s0 + q) * (C * 3) + k * 3 + j];
        } else {
            long long n = 0;
            for (int q = 0; q < C; ++q) n += scm[k * C + q];
            v = (double)n;
        }
        sums[((long)b * C + k) * 4 + j] = v;
    }
}

inline int eval_nslots(int HW) { return (int)(((long)HW + EV_RANGE - 1) / EV_RANGE); }

template <int CMAX>
inline void eval_launch(bool u8, dim3 grid, hipStream_t st, const EvalParams& p) {
    if (u8) hipLaunchKernelGGL((eval_kernel<CMAX, true>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((eval_kernel<CMAX, false>), grid, dim3(256), 0, st, p);
}

}  // namespace

extern "C" size_t srbh_eval_ws_bytes(int B, int HW, int C) {
    if (B <= 0 || HW <= 0 || C < 2 || C > 16) return 0;
    return (size_t)B * eval_nslots(HW) * ((size_t)C * 3 * sizeof(double) + (size_t)C * C * sizeof(unsigned));
}

extern "C" int srbh_eval_sums(const srbh_eval_args* a, void* stream) {
    SRBH_REQUIRE(a, "srbh_eval_sums: null argument struct");
    SRBH_REQUIRE(a->height && a->logits && a->ref && a->label && a->sums && a->cm && a->bad && a->ws, "srbh_eval_sums: null pointer");
    SRBH_REQUIRE(a->C >= 2 && a->C <= 16, "srbh_eval_sums: 2 to 16 classes (got %d)", a->C);
    SRBH_REQUIRE(a->B > 0 && a->B <= 65535, "srbh_eval_sums: 1 to 65535 images per call (got %d)", a->B);
    SRBH_REQUIRE(a->HW > 0 && a->HW <= (1 << 30), "srbh_eval_sums: 1 to 2^30 pixels per image (got %d)", a->HW);
    // every address a kernel forms is b * bs + c * cs + px * ps with 0 <= b < B, c < C, px < HW: strides may not be negative
    SRBH_REQUIRE(a->height_bs >= 0 && a->logits_bs >= 0 && a->logits_cs >= 0 && a->logits_ps >= 0, "srbh_eval_sums: strides must not be negative");
    const size_t need = srbh_eval_ws_bytes(a->B, a->HW, a->C);
    SRBH_REQUIRE(a->ws_bytes >= need, "srbh_eval_sums: workspace of %zu bytes, srbh_eval_ws_bytes asks for %zu", a->ws_bytes, need);
    EvalParams p;
    p.height = a->height; p.height_bs = a->height_bs;
    p.logits = a->logits; p.lbs = a->logits_bs; p.lcs = a->logits_cs; p.lps = a->logits_ps;
    p.ref = a->ref; p.label = a->label;
    p.C = a->C; p.HW = a->HW; p.nslots = eval_nslots(a->HW);
    p.ws_d = (double*)a->ws;
    p.ws_i = (unsigned*)((char*)a->ws + (size_t)a->B * p.nslots * a->C * 3 * sizeof(double));
    p.bad = a->bad; p.q_height = a->q_height; p.cls_map = a->cls_map;
    const dim3 grid(p.nslots, a->B);
    hipStream_t st = (hipStream_t)stream;
    if (a->C <= 7) eval_launch<7>(a->label_u8 != 0, grid, st, p);      // (7: the reference's hierarchy classes, train.py:55)
    else if (a->C <= 8) eval_launch<8>(a->label_u8 != 0, grid, st, p);
    else eval_launch<16>(a->label_u8 != 0, grid, st, p);
    SRBH_HIP(hipGetLastError());
    hipLaunchKernelGGL(eval_fold_kernel, dim3(a->B), dim3(256), 0, st, (const double*)p.ws_d, (const unsigned*)p.ws_i, p.nslots, a->C, a->sums, a->cm);
    SRBH_HIP(hipGetLastError());
    return SRBH_OK;
}
