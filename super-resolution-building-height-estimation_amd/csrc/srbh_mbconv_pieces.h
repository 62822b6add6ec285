// srbh_mbconv_pieces.h -- the device pieces the training-mode BatchNorm / MBConv-middle kernels of srbh_mbconv.hip are built from (included by it
// inside its anonymous namespace): activation, the per-channel reduction, the lane / channel geometry of the LDS-resident kernels, the forward
// statistics (batched load, two-pass variance, saved and running statistics), the backward through the activation (dz, the two channel sums and
// their coefficients, dx) and the reach test of the in-plane depthwise taps.  Every piece is the arithmetic of the kernels it came from, in their order: the
// kernels add in a fixed order with no atomics, and profiles/mbconv_shared_pieces_{bits,isa}.txt hold them to the bits and the instructions
// they had before.  Arguments go by value: the pieces are always inlined and the compiler then sees plain registers.

constexpr int NW = 16;               // waves per workgroup of the BatchNorm kernels (1024 threads)
constexpr int U = 4;                 // images per wave and round of global loads (16 waves x 4 = the whole batch of 64 in ONE round)

// (v_rcp_f32: 1 ulp; these kernels are bound by the instruction stream of one wave per SIMD, an IEEE division is ~10 instructions)
__device__ __forceinline__ float sigmoidf(float z) { return __builtin_amdgcn_rcpf(1.f + __expf(-z)); }
template <int ACT>
__device__ __forceinline__ float act_f(float z) {
    if (ACT == 1) return z * sigmoidf(z);
    if (ACT == 2) return fmaxf(z, 0.f);
    return z;
}
template <int ACT>
__device__ __forceinline__ float act_grad(float z) {
    if (ACT == 1) {
        const float s = sigmoidf(z);
        return s * (1.f + z * (1.f - s));
    }
    if (ACT == 2) return z > 0.f ? 1.f : 0.f;
    return 1.f;
}

typedef float floatx4 __attribute__((ext_vector_type(4)));
template <int VEC> struct Vt { float v[VEC]; };
template <int VEC> __device__ __forceinline__ Vt<VEC> ldv(const float* p) {
    Vt<VEC> r;
    if (VEC == 4) {
        const floatx4 t = *(const floatx4*)p;
        r.v[0] = t[0]; r.v[1 % VEC] = t[1]; r.v[2 % VEC] = t[2]; r.v[3 % VEC] = t[3];
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int VEC> __device__ __forceinline__ void stv(float* p, const Vt<VEC>& r) {
    if (VEC == 4) *(floatx4*)p = floatx4{r.v[0], r.v[1 % VEC], r.v[2 % VEC], r.v[3 % VEC]};
    else *p = r.v[0];
}
template <int VEC> __device__ __forceinline__ Vt<VEC> zerov() {
    Vt<VEC> r;
#pragma unroll
    for (int k = 0; k < VEC; ++k) r.v[k] = 0.f;
    return r;
}

// ---- geometry of the LDS-resident kernels.  A workgroup owns a run of 64 * VEC contiguous floats per image: VEC = 1 -- CPW = 64 / HW adjacent
// channels of HW <= 64 elements; VEC = 4 -- one channel of 256 elements, a float4 per lane (slot = 0, seg = 64).  Wave w takes the images w,
// w + NW, ...; a lane keeps the same position of the run for every image, and its element(s) of image b sit at cache[(b * 64 + lane) * VEC].
template <int VEC>
struct Geo {
    int lane, wave;
    int seg;             // lanes that share a channel: min(HW, 64), a power of two
    int slot, pos;       // channel of the lane within the workgroup; position within its channel's lanes
    int c0, c;           // first channel of the workgroup, channel of the lane
    bool cok;            // c < C (the last workgroup may be ragged)
    long off, bstride;   // global offset of the lane's element(s) in image 0; image stride
    float n, invN;       // elements per channel, B * HW, and its reciprocal
    __device__ __forceinline__ Geo(int B, int C, int HW) {
        lane = threadIdx.x & 63;
        wave = threadIdx.x >> 6;
        seg = (VEC == 4 || HW >= 64) ? 64 : HW;
        slot = VEC == 4 ? 0 : lane / HW;
        pos = lane & (seg - 1);
        c0 = blockIdx.x * (64 * VEC / HW);
        c = c0 + slot;
        cok = c < C;
        off = (long)c0 * HW + lane * VEC;
        bstride = (long)C * HW;
        n = (float)B * (float)HW;
        invN = 1.f / n;
    }
    __device__ __forceinline__ int at(int b) const { return (b * 64 + lane) * VEC; }       // LDS index of the lane's element(s) of image b
    __device__ __forceinline__ bool writer() const { return cok && wave == 0 && pos == 0; } // the one lane that stores its channel's results
};

// sum over the lanes that share a channel (a run of `seg` consecutive lanes), then over the NW waves through `red`; every thread returns the
// total of ITS channel.  VEC == 1: a wave spans the CPW channels of the workgroup; VEC == 4: the whole workgroup is one channel.  Fixed order.
template <int VEC>
__device__ __forceinline__ float channel_sum(const Geo<VEC> g, float v, float (*red)[64]) {
    for (int o = 1; o < g.seg; o <<= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                          // `red` may still be read from the previous reduction
    if (g.pos == 0) red[g.wave][g.slot] = v;
    __syncthreads();
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int w = 0; w < NW; w += 2) {
        a += red[w][g.slot];
        b += red[w + 1][g.slot];
    }
    return a + b;
}

// ---- forward statistics ----
// x -> cache for all B images, U images of a wave in flight at a time; returns the lane's share of the channel sum.
// These kernels are LATENCY chains, not bandwidth: a workgroup moves 16-64 KB.  Every global pass is therefore issued U images at a time (a
// plain loop leaves one load in flight per lane: measured 12-16 us per launch).
template <int VEC>
__device__ __forceinline__ float stage_sum(const Geo<VEC> g, const float* x, float* cache, int B) {
    float s = 0.f;
    for (int b0 = g.wave; b0 < B; b0 += NW * U) {
        Vt<VEC> v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int b = b0 + NW * u;
            v[u] = (g.cok && b < B) ? ldv<VEC>(x + b * g.bstride + g.off) : zerov<VEC>();
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int b = b0 + NW * u;
            if (b < B) stv<VEC>(cache + g.at(b), v[u]);
#pragma unroll
            for (int k = 0; k < VEC; ++k) s += v[u].v[k];
        }
    }
    return s;
}

// what nn.BatchNorm2d keeps in running_var: the unbiased variance (T = float, or double for the large planes' double partial sums)
template <class T>
__device__ __forceinline__ T unbiased_var(T var, T n) { return n > (T)1 ? var * n / (n - (T)1) : var; }

// where a BatchNorm's batch statistics go, and the running statistics as they were (requested early, before the reductions)
struct BnStatOut {
    float* save_mean; float* save_invstd;
    float* running_mean; float* running_var;       // may be null (both) where the caller says OPTIONAL_RUNNING
    float rm0, rv0, momentum;
};
// the running-statistics update of one channel (rm / rv point at its two values, rm0 / rv0 are what they held), by ONE thread.  `var` is the
// biased variance over `n` elements, T as unbiased_var.  a * b + c * d leaves it to the compiler which product an fma swallows, and it chose
// differently from one arrangement of the surrounding code to the next: the roundings are therefore spelled out -- the mean as two products
// and their sum, the variance as one fma onto the rounded momentum * unbiased variance (what every kernel here has always computed).
template <class T>
__device__ __forceinline__ void update_running(float* rm, float* rv, float rm0, float rv0, float momentum, float mean, T var, T n) {
#pragma clang fp contract(off)
    *rm = (1.f - momentum) * rm0 + momentum * mean;
    *rv = fmaf(1.f - momentum, rv0, momentum * (float)unbiased_var(var, n));
}
// save_mean / save_invstd and the running statistics of channel c, by ONE thread
template <bool OPTIONAL_RUNNING>
__device__ __forceinline__ void store_stats(const BnStatOut o, int c, float mean, float invstd, float var, float n) {
    o.save_mean[c] = mean;
    o.save_invstd[c] = invstd;
    if (!OPTIONAL_RUNNING || o.running_mean) update_running(o.running_mean + c, o.running_var + c, o.rm0, o.rv0, o.momentum, mean, var, n);
}

// exact two-pass statistics of the lane's channel over cache (s: the lane's share of the sum, from stage_sum or from whoever filled cache),
// stored through `o` by the channel's writer lane
struct BnStat { float mean, invstd; };
template <int VEC, bool OPTIONAL_RUNNING>
__device__ __forceinline__ BnStat bn_stats(const Geo<VEC> g, const float* cache, int B, float s, float eps, const BnStatOut o, float (*red)[64]) {
    BnStat st;
    st.mean = channel_sum(g, s, red) * g.invN;
    float q = 0.f;
    for (int b = g.wave; b < B; b += NW) {
        const Vt<VEC> v = ldv<VEC>(cache + g.at(b));
#pragma unroll
        for (int k = 0; k < VEC; ++k) q = fmaf(v.v[k] - st.mean, v.v[k] - st.mean, q);
    }
    const float var = channel_sum(g, q, red) * g.invN;       // biased, as F.batch_norm normalises
    st.invstd = 1.f / sqrtf(var + eps);
    if (g.writer()) store_stats<OPTIONAL_RUNNING>(o, g.c, st.mean, st.invstd, var, g.n);
    return st;
}

// ---- backward through the activation ----
struct BnNorm { float mean, invstd, g, be; };      // of the lane's channel: saved statistics, gamma, beta
__device__ __forceinline__ float bn_xhat(float x, const BnNorm m) { return (x - m.mean) * m.invstd; }
// dz of one element from its xhat and dy.  GATE: dy * gate + dpooled / HW (gt, dpo; the caller may have folded the drop-connect factor into
// both); DROP: * dr.  Compile-time, so that a kernel that never has one does not multiply by 1.
template <int ACT, bool GATE, bool DROP>
__device__ __forceinline__ float bn_dz(float xh, float dy, const BnNorm m, float gt, float dpo, float dr) {
    float d = GATE ? fmaf(dy, gt, dpo) : dy;
    if (DROP) d *= dr;
    return d * act_grad<ACT>(fmaf(xh, m.g, m.be));
}
// xhat and dz of a float4 from x and dy
template <int ACT, bool GATE, bool DROP>
__device__ __forceinline__ floatx4 bn_dz(const floatx4 x, const floatx4 dy, const BnNorm m, float gt, float dpo, float dr, floatx4& xh) {
    floatx4 dz;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        xh[k] = bn_xhat(x[k], m);
        dz[k] = bn_dz<ACT, GATE, DROP>(xh[k], dy[k], m, gt, dpo, dr);
    }
    return dz;
}
__device__ __forceinline__ void bn_bwd_accum(float dz, float xh, float& s1, float& s2) {
    s2 = fmaf(dz, xh, s2);
    s1 += dz;
}
// the two channel sums -> dbeta / dgamma (by the writer lane) -> the coefficients of dx
struct BnBwdK { float k1, k2, gi; };
template <int VEC>
__device__ __forceinline__ BnBwdK bn_bwd_sums(const Geo<VEC> g, float s1, float s2, float gamma, float invstd, float* dbeta, float* dgamma,
                                              float (*red)[64]) {
    const float sum_dz = channel_sum(g, s1, red);
    const float sum_dzx = channel_sum(g, s2, red);
    if (g.writer()) {
        dbeta[g.c] = sum_dz;
        dgamma[g.c] = sum_dzx;
    }
    return BnBwdK{sum_dz * g.invN, sum_dzx * g.invN, gamma * invstd};
}
__device__ __forceinline__ float bn_dx(float dz, float xh, const BnBwdK k) { return k.gi * (dz - k.k1 - xh * k.k2); }

// ---- depthwise K x K taps inside one W x W plane (stride 1, zero padding K / 2) ----
// false: tap row / column d (0 .. K-1) is further out than the plane is wide and never lands inside it (uniform -- 16 of the 25 taps at 2x2)
template <int K>
__device__ __forceinline__ bool tap_reaches(int d, int W) { return !(d - K / 2 >= W || K / 2 - d >= W); }
// (The two tap loops themselves stand three times in the mid kernels, for the forward, the weight gradient and the mirrored data gradient: one
//  walk that hands (tap, LDS offset) to a functor compiled to another branch structure and ran the K = 5 kernels 3 % slower, and a shared
//  bounds-test helper changed their instructions too -- profiles/mbconv_shared_pieces_isa.txt.)
