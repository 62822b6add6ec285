// srbh_dw_pieces.h -- the device pieces the depthwise kernels of srbh_dwconv.hip and the encoder's inference kernels of srbh_enc_eval.hip are
// built from (included by each inside its anonymous namespace): activation and gate, the wave sum, the LDS staging of the staged
// depthwise forms.  Every piece is the arithmetic of the kernels it came from, in their
// order: the kernels add in a fixed order with no atomics, and profiles/dw_pieces_{bits,isa}.txt hold them to the bits and the instruction
// counts they had before.  Arguments go by value or const reference: the pieces are always inlined and the compiler then sees plain registers.

typedef float floatx4 __attribute__((ext_vector_type(4)));

// act 0 none, 1 SiLU, 2 ReLU.  (The IEEE division on purpose: srbh_mbconv_pieces.h's v_rcp form gives other bits.)
__device__ __forceinline__ float act_apply(float u, int act) {
    if (act == 1) return u / (1.f + __expf(-u));
    if (act == 2) return fmaxf(u, 0.f);
    return u;
}
__device__ __forceinline__ float gate_sigmoid(float z) { return 1.f / (1.f + __expf(-z)); }
// the sum over the 64 lanes of a wave, in lane 0
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// ---- LDS-staged forms (round 3).  The one-thread-per-output kernels spend ~150 instructions per output on 25 predicated taps with 64-bit
// address arithmetic (13-25 us per call on tensors that take 3-5 us to stream); here a workgroup stages P whole planes ZERO-PADDED in LDS
// (coalesced reads of P contiguous planes), so every tap is one unconditional ds_read + fma.
//   forward        : out[oy][ox] = sum_ij xpad[oy s + i][ox s + j] w[i][j]                      (x placed at (pad_t, pad_l))
//   input gradient : dx[y][x]   = sum_ij dyup[y + pad_t + K-1 - i][x + pad_l + K-1 - j] w[i][j]  (dy placed at (K-1 + oy s, K-1 + ox s): zero-upsampled)
struct DWLds {
    const float* src; const float* w; float* out;
    long planes;
    int C, SH, SW, OUTH, OUTW, PH, PW, ss, soy, sox, os, by, bx, P;
};
// Stage the workgroup's planes p0 .. p0 + np - 1 in sm (P planes of PH x PW, halo zero) and their weight rows in wl; returns np.  PRE: the
// staged value is swish(x * a0[ch] + b0[ch]) where a0 is given (the zero padding is then the padding of the ACTIVATED tensor).
// (zero fill, then scatter the source elements: a single pass over the PADDED index space -- a division and a predicated gather per
//  padded element -- was measured slower on every shape)
template <int K, bool PRE>
__device__ __forceinline__ int dw_stage(const DWLds& p, float* sm, float* wl, const long p0, const float* a0, const float* b0) {
    const int t = threadIdx.x, plane_sz = p.PH * p.PW;
    const int np = (int)((p.planes - p0) < p.P ? (p.planes - p0) : p.P);
    for (int e = t; e < p.P * plane_sz; e += 256) sm[e] = 0.f;
    for (int e = t; e < np * K * K; e += 256) wl[e] = p.w[(long)((p0 + e / (K * K)) % p.C) * K * K + e % (K * K)];
    __syncthreads();
    const int ssz = p.SH * p.SW;
    const float* sp = p.src + p0 * ssz;
    for (int e = t; e < np * ssz; e += 256) {
        const int pl = e / ssz, q = e - pl * ssz, u = q / p.SW, v = q - u * p.SW;
        const int r = u * p.ss + p.soy, c = v * p.ss + p.sox;
        float x = sp[e];
        if (PRE && a0) {
            const int ch = (int)((p0 + pl) % p.C);
            x = act_apply(fmaf(x, a0[ch], b0[ch]), 1);
        }
        if (r < p.PH && c < p.PW) sm[pl * plane_sz + r * p.PW + c] = x;
    }
    __syncthreads();
    return np;
}
// host side: workgroups of a grid-stride launch over n items, 256 per workgroup, at most 8192
inline int grid_for(long n) {
    const long b = (n + 255) / 256;
    return (int)(b < 8192 ? (b > 0 ? b : 1) : 8192);
}
