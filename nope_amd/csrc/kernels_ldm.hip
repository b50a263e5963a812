// Token-space kernels of the LDM cross-attention U-Net variant (src/model/u_net/ldm/attention.py:149-277): LayerNorm over the
// channels of a token, GEGLU, softmax self-attention over the h*w tokens of a sample, and the per-sample broadcast add
// that the single-token cross-attention collapses to.  Activations are NHWC, i.e. already (sample, token, channel).
#include <cstdlib>

#include "nope_common.h"

namespace nope {

namespace {

constexpr int NT = 256;

// ---- LayerNorm(C) per token (attention.py:210-212, eps 1e-5): one wave per token, 16-byte vectors -----------------------
template <class T>
__global__ __launch_bounds__(NT) void layernorm_kernel(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, long long M, int C, float eps) {
    constexpr int VEC = Elt<T>::VEC;
    const int lane = threadIdx.x & 63;
    const long long tok = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (tok >= M) return;
    const T* xr = x + tok * C;
    T* yr = y + tok * C;
    const int nv = C / VEC;
    float s = 0.f, q = 0.f;
    for (int v = lane; v < nv; v += 64) {
        float t[VEC];
        Elt<T>::unpack(ld16(xr + v * VEC), t);
#pragma unroll
        for (int e = 0; e < VEC; ++e) { s += t[e]; q += t[e] * t[e]; }
    }
    s = wave_sum(s); q = wave_sum(q);
    const float mean = s / (float)C;
    float var = q / (float)C - mean * mean;
    var = var > 0.f ? var : 0.f;
    const float rstd = 1.0f / sqrtf(var + eps);
    for (int v = lane; v < nv; v += 64) {
        float t[VEC];
        Elt<T>::unpack(ld16(xr + v * VEC), t);
#pragma unroll
        for (int e = 0; e < VEC; ++e) t[e] = (t[e] - mean) * rstd * gamma[v * VEC + e] + beta[v * VEC + e];
        st16(yr + v * VEC, Elt<T>::pack(t));
    }
}

// ---- GEGLU (attention.py:37-44): in (M, 2*D) = [x | gate] -> out (M, D) = x * gelu(gate), exact (erf) GELU ---------------
// (IL: the columns of `in` are (x_j, gate_j) pairs -- the layout the runtime packs the projection's rows in for the fused epilogue)
template <class T, bool IL>
__global__ __launch_bounds__(NT) void geglu_kernel(const T* __restrict__ in, T* __restrict__ out, long long M, int D) {
    constexpr int VEC = Elt<T>::VEC;
    const int nv = D / VEC;
    const long long total = M * nv;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const long long m = i / nv;
        const int v = (int)(i - m * nv);
        float a[VEC], g[VEC];
        if (IL) {
            float lo[VEC], hi[VEC];
            Elt<T>::unpack(ld16(in + m * 2 * D + 2 * v * VEC), lo);
            Elt<T>::unpack(ld16(in + m * 2 * D + 2 * v * VEC + VEC), hi);
#pragma unroll
            for (int e = 0; e < VEC / 2; ++e) { a[e] = lo[2 * e]; g[e] = lo[2 * e + 1]; a[VEC / 2 + e] = hi[2 * e]; g[VEC / 2 + e] = hi[2 * e + 1]; }
        } else {
            Elt<T>::unpack(ld16(in + m * 2 * D + v * VEC), a);
            Elt<T>::unpack(ld16(in + m * 2 * D + D + v * VEC), g);
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] = geglu_f(a[e], g[e]);
        st16(out + m * D + v * VEC, Elt<T>::pack(a));
    }
}

// ---- y[s, t, :] = x[s, t, :] + u[s, :]: what cross-attention against ONE context token is (softmax over a single key == 1,
// so attn2(x, context) = to_out(to_v(context)) for every query token, attention.py:168-189 with j = 1) ------------------------
template <class T>
__global__ __launch_bounds__(NT) void add_rowvec_kernel(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ u,
                                                        long long M, int tokens, int C, int u_stride) {
    constexpr int VEC = Elt<T>::VEC;
    const int nv = C / VEC;
    const long long total = M * nv;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const long long m = i / nv;
        const int v = (int)(i - m * nv);
        const float* ur = u + (m / tokens) * u_stride + v * VEC;
        float t[VEC];
        Elt<T>::unpack(ld16(x + m * C + v * VEC), t);
#pragma unroll
        for (int e = 0; e < VEC; ++e) t[e] += ur[e];
        st16(y + m * C + v * VEC, Elt<T>::pack(t));
    }
}

// ---- softmax self-attention over the tokens of a sample (CrossAttention with context = x, attention.py:168-189) ------------
// qkv (S, N, 3*C): [q | k | v], head h = channels h*D .. h*D+D-1 (rearrange "b n (h d)"), D = 32, 64 or 128.  L = D / 32 adjacent lanes
// own one query, 32 channels each (q and the output accumulator in registers: 64 VGPRs whatever D is); a score is the lanes' partial
// dot products summed with an xor butterfly, so every lane of the group holds the same value bit for bit.  Keys / values of the
// (sample, head) stream through LDS in f32 chunks of 4096 / D keys that the threads read at L addresses per key (broadcast), with an
// online softmax.  f32 arithmetic throughout.  (At D = 32, L = 1: one thread per query, 128-key chunks, no exchange.)
// (A VALU kernel: at D = 32 this op is ~5 % of the variant's FLOPs; the convolutions and linears run on the MFMA kernels.)
constexpr int AD = 32;           // channels per lane (and the head width of the shipped configuration)
template <class T, int D>
__global__ __launch_bounds__(NT) void token_attn_kernel(const T* __restrict__ qkv, T* __restrict__ out, int N, int C, float scale) {
    constexpr int L = D / AD, QPB = NT / L, KCH = 128 * AD / D;
    __shared__ __attribute__((aligned(16))) float s_k[KCH][D];
    __shared__ __attribute__((aligned(16))) float s_v[KCH][D];
    const int tid = threadIdx.x;
    const int head = blockIdx.y, smp = blockIdx.z;
    const int qi = blockIdx.x * QPB + tid / L, part = tid % L;
    const T* base = qkv + (size_t)smp * N * 3 * C;
    float q[AD], o[AD];
    const bool qok = qi < N;
    {
        const T* qp = base + (size_t)(qok ? qi : 0) * 3 * C + head * D + part * AD;
        constexpr int VEC = Elt<T>::VEC;
#pragma unroll
        for (int v = 0; v < AD / VEC; ++v) {
            float t[VEC];
            Elt<T>::unpack(ld16(qp + v * VEC), t);
#pragma unroll
            for (int e = 0; e < VEC; ++e) q[v * VEC + e] = t[e] * scale;
        }
    }
#pragma unroll
    for (int d = 0; d < AD; ++d) o[d] = 0.f;
    float mx = -3.0e38f, den = 0.f;
    for (int k0 = 0; k0 < N; k0 += KCH) {
        __syncthreads();
        // stage KCH keys and values of this head as f32: thread -> (key, 16-byte vector)
        constexpr int VEC = Elt<T>::VEC;
        constexpr int VPK = D / VEC;
        for (int i = tid; i < KCH * VPK * 2; i += NT) {
            const int which = i / (KCH * VPK), r = i - which * (KCH * VPK);
            const int key = r / VPK, v = r - key * VPK;
            float t[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) t[e] = 0.f;
            if (k0 + key < N) Elt<T>::unpack(ld16(base + (size_t)(k0 + key) * 3 * C + (1 + which) * C + head * D + v * VEC), t);
            float* dst = which ? &s_v[key][v * VEC] : &s_k[key][v * VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) dst[e] = t[e];
        }
        __syncthreads();
        const int kn = N - k0 < KCH ? N - k0 : KCH;
        for (int j = 0; j < kn; ++j) {
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < AD; ++d) s += q[d] * s_k[j][part * AD + d];
#pragma unroll
            for (int m = 1; m < L; m <<= 1) s += __shfl_xor(s, m, 64);      // (a + b == b + a: the group's lanes agree exactly)
            const float nm = s > mx ? s : mx;
            const float corr = __expf(mx - nm), p = __expf(s - nm);
            den = den * corr + p;
#pragma unroll
            for (int d = 0; d < AD; ++d) o[d] = o[d] * corr + p * s_v[j][part * AD + d];
            mx = nm;
        }
    }
    if (qok) {
        const float inv = 1.0f / den;
        T* op = out + ((size_t)smp * N + qi) * C + head * D + part * AD;
        constexpr int VEC = Elt<T>::VEC;
#pragma unroll
        for (int v = 0; v < AD / VEC; ++v) {
            float t[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) t[e] = o[v * VEC + e] * inv;
            st16(op + v * VEC, Elt<T>::pack(t));
        }
    }
}

// ---- the same op on the matrix cores (16-bit storage: bf16, and -- round 6 -- f16) ---------------------------------------------------------------------
// One wave owns 32 queries of a (sample, head); a workgroup of four waves shares the key / value blocks (64 keys per
// iteration) through LDS.  Everything is computed TRANSPOSED, so that a lane's accumulator column is one query throughout:
//   S^T = K Q^T        (v_mfma_f32_32x32x16_bf16: A = 32 keys x 16 d from LDS, B = Q^T from registers, two per 32 keys)
//   online softmax     per query = per lane pair (l, l ^ 32): the 16 + 16 keys of a block a pair holds; max / sum exchanged with
//                      one cross-lane move; the running output is rescaled by one factor per lane
//   O^T += V^T P^T     the B operand P^T is the lane's OWN 16 exponentials rounded to bf16 -- no data crosses lanes: the MFMA's
//                      k slot (8 h + j) of step t is defined to be key 16 t + 8 (j >> 2) + 4 h + (j & 3), which is where the
//                      accumulator layout left it, and the A operand V^T (staged transposed, [d][key]) is read in that key order
//                      (two 8-byte LDS reads per step)
// P is rounded to bf16 before P V (as V is stored); scores, max, sums and the output accumulate in f32.
// D = 64 / 128: D / 16 MFMA steps per score block (Q^T fragments qf[D / 16]) and D / 32 output accumulators (V^T rows li + 32 dt); the
// softmax and the P^T fragments do not depend on D.  At D = 32 the instructions and their order are those of the 32-wide kernel.
constexpr int MQ = 128;          // queries per workgroup
constexpr int MK = 64;           // keys per iteration
constexpr int VT_LD = 68;        // 16-bit elements per staged V^T row (64 keys + pad: conflict-free 8-byte reads)
template <int D> constexpr int k_ld() { return D + 8; }        // per staged K row (D + pad: conflict-free 16-byte fragment reads)
template <class T, int D>      // bf16_t or f16_t (v_mfma_f32_32x32x16_bf16 / _f16; P rounded to the same 16-bit type as V is stored in)
__global__ __launch_bounds__(NT) void token_attn_mfma_kernel(const T* __restrict__ qkv, T* __restrict__ out, int N, int C, float scale_log2e) {
    constexpr bool F16 = Elt<T>::DT == NOPE_F16;
    constexpr int KS = D / 16, DT = D / 32, K_LD = k_ld<D>();
    auto mma = [](const u32x4& a, const u32x4& b, const __attribute__((ext_vector_type(16))) float& c) {
        if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
        else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    };
    typedef __attribute__((ext_vector_type(16))) float f32x16;
    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
    __shared__ __attribute__((aligned(16))) unsigned short s_k[MK][K_LD];          // (raw 16-bit elements of either type)
    __shared__ __attribute__((aligned(16))) unsigned short s_vt[D][VT_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int head = blockIdx.y, smp = blockIdx.z;
    const int h = lane >> 5, li = lane & 31;
    const T* base = qkv + (size_t)smp * N * 3 * C + head * D;
    const int q = blockIdx.x * MQ + wave * 32 + li;            // this lane's query (accumulator column)
    // Q^T fragments (B operand): column = query, k = d: 8 consecutive d at 8 h (+ 16 kk for step kk)
    u32x4 qf[KS];
    {
        const T* qp = base + (size_t)(q < N ? q : N - 1) * 3 * C + 8 * h;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) qf[kk] = ld16(qp + 16 * kk);
    }
    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float mx = -3.0e38f, den = 0.f;                              // (in log2 units; den: this lane's half of the row sum)
    // staging role: thread -> (key, 16-byte vectors 8 svec + 32 j of its K row and of its V row); the next block's loads fly under the MFMAs
    const int skey = tid >> 2, svec = tid & 3;
    u32x4 nk[DT], nv[DT];
    auto fetch = [&](int k0) {
        const int key = k0 + skey;
        const T* kp = base + (size_t)(key < N ? key : N - 1) * 3 * C + C + svec * 8;
#pragma unroll
        for (int j = 0; j < DT; ++j) { nk[j] = ld16(kp + 32 * j); nv[j] = ld16(kp + C + 32 * j); }
    };
    fetch(0);
    for (int k0 = 0; k0 < N; k0 += MK) {
        __syncthreads();                                         // everyone is done reading the previous block
#pragma unroll
        for (int j = 0; j < DT; ++j) {
            st16(&s_k[skey][svec * 8 + 32 * j], nk[j]);
#pragma unroll
            for (int e = 0; e < 8; ++e) {                        // V^T: [d][key]
                const unsigned w = nv[j][e >> 1];
                s_vt[svec * 8 + 32 * j + e][skey] = (unsigned short)((e & 1) ? (w >> 16) : (w & 0xffffu));
            }
        }
        __syncthreads();
        if (k0 + MK < N) fetch(k0 + MK);
        f32x16 sc[2];
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[sb][r] = 0.f;
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                const u32x4 kf = ld16(&s_k[sb * 32 + li][8 * h + 16 * kk]);
                sc[sb] = mma(kf, qf[kk], sc[sb]);
            }
        }
        // scores in log2 units; keys behind N (last block of a ragged N: a uniform branch, the other blocks pay no compare / select) drop out
        float bm = -3.0e38f;
        if (k0 + MK > N) {
#pragma unroll
            for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = k0 + sb * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
                    const float v = key < N ? sc[sb][r] * scale_log2e : -3.0e38f;
                    sc[sb][r] = v;
                    bm = fmaxf(bm, v);
                }
        } else {
#pragma unroll
            for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = sc[sb][r] * scale_log2e;
                    sc[sb][r] = v;
                    bm = fmaxf(bm, v);
                }
        }
        bm = fmaxf(bm, __shfl_xor(bm, 32, 64));                  // the other half of this query's keys
        const float nm = fmaxf(mx, bm);
        const float corr = __builtin_amdgcn_exp2f(mx - nm);
        mx = nm;
        float ps = 0.f;
        u32x4 pf[2][2];                                          // P^T fragments: [32-key block][MFMA step]
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float p0 = __builtin_amdgcn_exp2f(sc[sb][8 * t + 2 * j] - nm), p1 = __builtin_amdgcn_exp2f(sc[sb][8 * t + 2 * j + 1] - nm);
                    ps += p0 + p1;
                    pf[sb][t][j] = Elt<T>::cvt_pk_raw(p0, p1);
                }
        den = den * corr + ps;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] *= corr;
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int kb = sb * 32 + 16 * t + 4 * h;        // keys kb .. kb + 3 and kb + 8 .. kb + 11 are this lane's 8 k slots
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    const u32x2 v0 = *reinterpret_cast<const u32x2*>(&s_vt[32 * dt + li][kb]);
                    const u32x2 v1 = *reinterpret_cast<const u32x2*>(&s_vt[32 * dt + li][kb + 8]);
                    const u32x4 vf = {v0[0], v0[1], v1[0], v1[1]};
                    o[dt] = mma(vf, pf[sb][t], o[dt]);
                }
            }
    }
    den += __shfl_xor(den, 32, 64);
    if (q < N) {
        const float inv = 1.0f / den;
        T* op = out + ((size_t)smp * N + q) * C + head * D + 4 * h;       // rows of O^T this lane holds: d = 32 dt + 8 g + 4 h + (r & 3)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const unsigned long long lo = Elt<T>::cvt_pk(o[dt][4 * g] * inv, o[dt][4 * g + 1] * inv), hi = Elt<T>::cvt_pk(o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv);
                *reinterpret_cast<unsigned long long*>(op + 32 * dt + 8 * g) = lo | (hi << 32);
            }
    }
}

// ---- ... and for the f32 STORAGE of the split-precision compute modes (NOPE_BF16X3, and NOPE_F16X2 = NOPE_BF16X3 outside the 3x3 convs) ----
// Same schedule and operand order as token_attn_mfma_kernel; every matrix product is the three bf16 passes of Tile<f32s_t>
// (conv_gemm_common.h): x = hi + lo with hi = bf16(x), lo = bf16(x - hi), product = lo*hi + hi*lo + hi*hi accumulated in f32 (the
// small terms first), i.e. 2^-16 relative per product where one bf16 pass has 2^-8.  K and V are split once per block when they
// are staged (two LDS images each), Q once per wave, P = exp2(...) in registers right where the accumulator layout leaves it.
// Scores, max, sums and the output accumulate in f32; the row sum adds the UNSPLIT exponentials.  (The VALU kernel above was 18.7
// of the 63 ms of a 128-hypothesis NOPE_F16X2 forward of the shipped LDM size: profiles/r06t_timeline_ldm_128_f16x2_summary.txt.)
__device__ __forceinline__ void split8_bf16(const u32x4 a, const u32x4 b, u32x4& hi, u32x4& lo) {      // 8 f32 (a | b) -> 8 bf16 hi + 8 bf16 lo
    float x[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {      // (through a scalar: __builtin_bit_cast straight from a vector-element lvalue reads element 0)
        const unsigned u0 = a[e], u1 = b[e];
        x[e] = __builtin_bit_cast(float, u0); x[4 + e] = __builtin_bit_cast(float, u1);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const unsigned h = cvt_pk_bf16(x[2 * e], x[2 * e + 1]);
        const float h0 = __builtin_bit_cast(float, h << 16), h1 = __builtin_bit_cast(float, h & 0xffff0000u);
        hi[e] = h;
        lo[e] = cvt_pk_bf16(x[2 * e] - h0, x[2 * e + 1] - h1);
    }
}
template <int D>
__global__ __launch_bounds__(NT) void token_attn_mfma_x3_kernel(const float* __restrict__ qkv, float* __restrict__ out, int N, int C, float scale_log2e) {
    constexpr int KS = D / 16, DT = D / 32, K_LD = k_ld<D>();
    typedef __attribute__((ext_vector_type(16))) float f32x16;
    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
    __shared__ __attribute__((aligned(16))) bf16_t s_k[2][MK][K_LD];          // [hi | lo]
    __shared__ __attribute__((aligned(16))) bf16_t s_vt[2][D][VT_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int head = blockIdx.y, smp = blockIdx.z;
    const int h = lane >> 5, li = lane & 31;
    const float* base = qkv + (size_t)smp * N * 3 * C + head * D;
    const int q = blockIdx.x * MQ + wave * 32 + li;            // this lane's query (accumulator column)
    u32x4 qh[KS], ql[KS];                                      // Q^T fragments (B operand): column = query, k = d: 8 consecutive d at 8 h (+ 16 kk for step kk)
    {
        const float* qp = base + (size_t)(q < N ? q : N - 1) * 3 * C + 8 * h;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {                      // q * (scale log2 e) in f32, then split: the scores come out of the MFMAs in log2 units
            u32x4 a = ld16(qp + 16 * kk), b = ld16(qp + 16 * kk + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned ua = a[e], ub = b[e];
                a[e] = __builtin_bit_cast(unsigned, __builtin_bit_cast(float, ua) * scale_log2e);
                b[e] = __builtin_bit_cast(unsigned, __builtin_bit_cast(float, ub) * scale_log2e);
            }
            split8_bf16(a, b, qh[kk], ql[kk]);
        }
    }
    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float mx = -3.0e38f, den = 0.f;                              // (in log2 units; den: this lane's half of the row sum)
    // staging role: thread -> (key, channels 8 svec + 32 j .. + 7 of its K row and of its V row); the next block's loads fly under the MFMAs
    const int skey = tid >> 2, svec = tid & 3;
    u32x4 nk[DT][2], nv[DT][2];
    auto fetch = [&](int k0) {
        const int key = k0 + skey;
        const float* kp = base + (size_t)(key < N ? key : N - 1) * 3 * C + C + svec * 8;
#pragma unroll
        for (int j = 0; j < DT; ++j) {
            nk[j][0] = ld16(kp + 32 * j); nk[j][1] = ld16(kp + 32 * j + 4); nv[j][0] = ld16(kp + C + 32 * j); nv[j][1] = ld16(kp + C + 32 * j + 4);
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < N; k0 += MK) {
        __syncthreads();                                         // everyone is done reading the previous block
#pragma unroll
        for (int j = 0; j < DT; ++j) {
            u32x4 kh, kl, vh, vl;
            split8_bf16(nk[j][0], nk[j][1], kh, kl);
            split8_bf16(nv[j][0], nv[j][1], vh, vl);
            st16(&s_k[0][skey][svec * 8 + 32 * j], kh);
            st16(&s_k[1][skey][svec * 8 + 32 * j], kl);
#pragma unroll
            for (int e = 0; e < 8; ++e) {                        // V^T: [d][key]
                const unsigned wh = vh[e >> 1], wl = vl[e >> 1];
                s_vt[0][svec * 8 + 32 * j + e][skey] = (bf16_t)((e & 1) ? (wh >> 16) : (wh & 0xffffu));
                s_vt[1][svec * 8 + 32 * j + e][skey] = (bf16_t)((e & 1) ? (wl >> 16) : (wl & 0xffffu));
            }
        }
        __syncthreads();
        if (k0 + MK < N) fetch(k0 + MK);
        f32x16 sc[2];
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[sb][r] = 0.f;
#pragma unroll
        for (int t = 0; t < 3; ++t)                               // term outer: (lo, hi), (hi, lo), (hi, hi) -- MFMAs on one accumulator sit apart
#pragma unroll
            for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) {
                    const u32x4 kf = ld16(&s_k[t == 0 ? 1 : 0][sb * 32 + li][8 * h + 16 * kk]);
                    const u32x4 qf = t == 1 ? ql[kk] : qh[kk];
                    sc[sb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kf), __builtin_bit_cast(bf16x8, qf), sc[sb], 0, 0, 0);
                }
        // keys behind N (last block of a ragged N: a uniform branch) drop out
        float bm = -3.0e38f;
        if (k0 + MK > N) {
#pragma unroll
            for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = k0 + sb * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
                    if (key >= N) sc[sb][r] = -3.0e38f;
                }
        }
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int r = 0; r < 16; ++r) bm = fmaxf(bm, sc[sb][r]);
        bm = fmaxf(bm, __shfl_xor(bm, 32, 64));                  // the other half of this query's keys
        const float nm = fmaxf(mx, bm);
        const float corr = __builtin_amdgcn_exp2f(mx - nm);
        mx = nm;
        float ps = 0.f;
        u32x4 ph[2][2], pl[2][2];                                // P^T fragments: [32-key block][MFMA step], hi and lo
#pragma unroll
        for (int sb = 0; sb < 2; ++sb)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float p0 = __builtin_amdgcn_exp2f(sc[sb][8 * t + 2 * j] - nm), p1 = __builtin_amdgcn_exp2f(sc[sb][8 * t + 2 * j + 1] - nm);
                    ps += p0 + p1;
                    const unsigned hh = cvt_pk_bf16(p0, p1);
                    ph[sb][t][j] = hh;
                    pl[sb][t][j] = cvt_pk_bf16(p0 - __builtin_bit_cast(float, hh << 16), p1 - __builtin_bit_cast(float, hh & 0xffff0000u));
                }
        den = den * corr + ps;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] *= corr;
#pragma unroll
        for (int tm = 0; tm < 3; ++tm)
#pragma unroll
            for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int kb = sb * 32 + 16 * t + 4 * h;        // keys kb .. kb + 3 and kb + 8 .. kb + 11 are this lane's 8 k slots
                    const u32x4 pf = tm == 1 ? pl[sb][t] : ph[sb][t];
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) {
                        const bf16_t* vr = &s_vt[tm == 0 ? 1 : 0][32 * dt + li][kb];
                        const u32x2 v0 = *reinterpret_cast<const u32x2*>(vr);
                        const u32x2 v1 = *reinterpret_cast<const u32x2*>(vr + 8);
                        const u32x4 vf = {v0[0], v0[1], v1[0], v1[1]};
                        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, vf), __builtin_bit_cast(bf16x8, pf), o[dt], 0, 0, 0);
                    }
                }
    }
    den += __shfl_xor(den, 32, 64);
    if (q < N) {
        const float inv = 1.0f / den;
        float* op = out + ((size_t)smp * N + q) * C + head * D + 4 * h;        // rows of O^T this lane holds: d = 32 dt + 8 g + 4 h + (r & 3)
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float t4[4] = {o[dt][4 * g] * inv, o[dt][4 * g + 1] * inv, o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv};
                u32x4 w;
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = __builtin_bit_cast(unsigned, t4[e]);
                st16(op + 32 * dt + 8 * g, w);
            }
    }
}

// x (M, C) -> y (M, C2) [:, off .. off + C): concatenation of token tensors along the channel axis (th.cat of the skip,
// adapt_openaimodel.py:152: GroupNorm(32) groups of the ResBlock that follows may straddle the two sources)
template <class T>
__global__ __launch_bounds__(NT) void copy_cols_kernel(const T* __restrict__ x, T* __restrict__ y, long long M, int C, int C2, int off) {
    constexpr int VEC = Elt<T>::VEC;
    const int nv = C / VEC;
    const long long total = M * nv;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const long long m = i / nv;
        const int v = (int)(i - m * nv);
        st16(y + m * C2 + off + v * VEC, ld16(x + m * C + v * VEC));
    }
}

// ---- parameter-free resampling on NHWC activations (openaimodel.py:94-175, and ResBlock's h_upd / x_upd, :262-271) ----------------
// avg_pool2d(2): y[n, i, j, :] = (x[2i, 2j] + x[2i, 2j+1] + x[2i+1, 2j] + x[2i+1, 2j+1]) / 4, H and W even; thread -> (output pixel, 16 bytes)
template <class T>
__global__ __launch_bounds__(NT) void avg_pool2_kernel(const T* __restrict__ x, T* __restrict__ y, long long n, int Ho, int Wo, int C) {
    constexpr int VEC = Elt<T>::VEC;
    const int nv = C / VEC;
    const long long total = n * Ho * Wo * nv;
    const long long rs = (long long)2 * Wo * C;           // one input row
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const long long pix = i / nv;
        const int v = (int)(i - pix * nv);
        const long long s = pix / ((long long)Ho * Wo);
        const int r = (int)(pix - s * Ho * Wo), oi = r / Wo, oj = r - oi * Wo;
        const T* xp = x + ((s * 2 * Ho + 2 * oi) * 2 * Wo + 2 * oj) * C + v * VEC;
        float a[VEC], b[VEC], c[VEC], d[VEC];
        Elt<T>::unpack(ld16(xp), a);
        Elt<T>::unpack(ld16(xp + C), b);
        Elt<T>::unpack(ld16(xp + rs), c);
        Elt<T>::unpack(ld16(xp + rs + C), d);
#pragma unroll
        for (int e = 0; e < VEC; ++e) a[e] = ((a[e] + b[e]) + (c[e] + d[e])) * 0.25f;
        st16(y + pix * C + v * VEC, Elt<T>::pack(a));
    }
}

// nearest x2 (F.interpolate(scale_factor=2, mode="nearest")): y[n, i, j, :] = x[n, i / 2, j / 2, :]; thread -> (input pixel, 16 bytes), four stores
template <class T>
__global__ __launch_bounds__(NT) void nearest2_kernel(const T* __restrict__ x, T* __restrict__ y, long long n, int H, int W, int C) {
    constexpr int VEC = Elt<T>::VEC;
    const int nv = C / VEC;
    const long long total = n * H * W * nv;
    const long long rs = (long long)2 * W * C;            // one output row
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const long long pix = i / nv;
        const int v = (int)(i - pix * nv);
        const long long s = pix / ((long long)H * W);
        const int r = (int)(pix - s * H * W), ii = r / W, jj = r - ii * W;
        const u32x4 t = ld16(x + pix * C + v * VEC);
        T* yp = y + ((s * 2 * H + 2 * ii) * 2 * W + 2 * jj) * C + v * VEC;
        st16(yp, t); st16(yp + C, t); st16(yp + rs, t); st16(yp + rs + C, t);
    }
}

unsigned grid_for_ll(long long n) {
    long long b = (n + NT - 1) / NT;
    if (b > 65535 * 8) b = 65535 * 8;
    if (b < 1) b = 1;
    return (unsigned)b;
}

}  // namespace

int launch_layernorm(int dt, const void* x, void* y, const float* gamma, const float* beta, long long M, int C, float eps, hipStream_t s) {
    const int vec = dt_vec(dt);
    if (!x || !y || !gamma || !beta || M <= 0 || C <= 0 || C % vec) return NOPE_ERR_ARG;
    const dim3 grid((unsigned)((M + NT / 64 - 1) / (NT / 64)));
    NOPE_DISPATCH_T(dt, T, hipLaunchKernelGGL((layernorm_kernel<T>), grid, dim3(NT), 0, s, (const T*)x, (T*)y, gamma, beta, M, C, eps));
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_geglu(int dt, const void* in, void* out, long long M, int D, hipStream_t s, int interleaved) {
    const int vec = dt_vec(dt);
    if (!in || !out || M <= 0 || D <= 0 || D % vec) return NOPE_ERR_ARG;
    const dim3 grid(grid_for_ll(M * (D / vec)));
    if (interleaved) { NOPE_DISPATCH_T(dt, T, hipLaunchKernelGGL((geglu_kernel<T, true>), grid, dim3(NT), 0, s, (const T*)in, (T*)out, M, D)); }
    else { NOPE_DISPATCH_T(dt, T, hipLaunchKernelGGL((geglu_kernel<T, false>), grid, dim3(NT), 0, s, (const T*)in, (T*)out, M, D)); }
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_add_rowvec(int dt, const void* x, void* y, const float* u, long long M, int tokens, int C, hipStream_t s, int u_stride) {
    if (u_stride <= 0) u_stride = C;
    const int vec = dt_vec(dt);
    if (!x || !y || !u || M <= 0 || tokens <= 0 || C % vec) return NOPE_ERR_ARG;
    const dim3 grid(grid_for_ll(M * (C / vec)));
    NOPE_DISPATCH_T(dt, T, hipLaunchKernelGGL((add_rowvec_kernel<T>), grid, dim3(NT), 0, s, (const T*)x, (T*)y, u, M, tokens, C, u_stride));
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

namespace {

template <int D>
int launch_token_attention_d(int dt, bool mfma, const void* qkv, void* out, int nsmp, int N, int C, hipStream_t s) {
    const float scale = 1.0f / sqrtf((float)D);
    const dim3 g2((unsigned)cdiv(N, MQ), (unsigned)(C / D), (unsigned)nsmp);
    if (dt == NOPE_BF16 && mfma) {
        hipLaunchKernelGGL((token_attn_mfma_kernel<bf16_t, D>), g2, dim3(NT), 0, s, (const bf16_t*)qkv, (bf16_t*)out, N, C, scale * 1.4426950408889634f);
    } else if (dt == NOPE_F16 && mfma) {
        hipLaunchKernelGGL((token_attn_mfma_kernel<f16_t, D>), g2, dim3(NT), 0, s, (const f16_t*)qkv, (f16_t*)out, N, C, scale * 1.4426950408889634f);
    } else if ((dt == NOPE_BF16X3 || dt == NOPE_F16X2) && mfma) {
        hipLaunchKernelGGL((token_attn_mfma_x3_kernel<D>), g2, dim3(NT), 0, s, (const float*)qkv, (float*)out, N, C, scale * 1.4426950408889634f);
    } else {
        const int sdt = dt_storage(dt);
        const dim3 grid((unsigned)cdiv(N, NT / (D / AD)), (unsigned)(C / D), (unsigned)nsmp);
        NOPE_DISPATCH_T(sdt, T, hipLaunchKernelGGL((token_attn_kernel<T, D>), grid, dim3(NT), 0, s, (const T*)qkv, (T*)out, N, C, scale));
    }
    return NOPE_OK;
}

}  // namespace

int launch_token_attention(int dt, const void* qkv, void* out, int nsmp, int N, int C, int dim_head, hipStream_t s) {
    if (!qkv || !out || nsmp <= 0 || N <= 0 || C <= 0 || (dim_head != 32 && dim_head != 64 && dim_head != 128) || C % dim_head) return NOPE_ERR_ARG;
    // bf16 / f16: the matrix-core kernel (NOPE_LDM_ATTN=0 keeps the VALU one: the tests compare the two); f32 -- the parity mode -- stays
    // on the all-f32 VALU kernel; the compute tags NOPE_BF16X3 / NOPE_F16X2 (f32 storage): the same schedule on three bf16 passes per product.
    // Head widths 32 / 64 / 128 (dim_head, attention.py:149-166), each kernel instantiated per width
    const bool mfma = NOPE_ENV("NOPE_LDM_ATTN", -1) != 0;
    const int e = dim_head == 32 ? launch_token_attention_d<32>(dt, mfma, qkv, out, nsmp, N, C, s)
                : dim_head == 64 ? launch_token_attention_d<64>(dt, mfma, qkv, out, nsmp, N, C, s)
                                 : launch_token_attention_d<128>(dt, mfma, qkv, out, nsmp, N, C, s);
    if (e) return e;
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

// ONE head as wide as the channels, C = 256 / 512 (the Stable Diffusion VAE's mid-block AttnBlock, u_net/ldm/model.py:144-187): the VALU kernel above
// with the head split over C / 32 = 8 / 16 lanes (q and the output accumulator stay 64 VGPRs per lane; 16 / 8 keys per LDS chunk, 32 KiB).  Every
// compute mode runs it on its storage type, f32 arithmetic: the op is ~2.1 GFLOP per 1 024-token sample, under 1 % of the VAE decoder's work.
int launch_wide_attention(int dt, const void* qkv, void* out, int nsmp, int N, int C, hipStream_t s) {
    if (!qkv || !out || nsmp <= 0 || N <= 0 || (C != 256 && C != 512) || !dt_is_compute(dt)) return NOPE_ERR_ARG;
    const int sdt = dt_storage(dt);
    const float scale = 1.0f / sqrtf((float)C);
    const dim3 grid((unsigned)cdiv(N, NT / (C / AD)), 1u, (unsigned)nsmp);
    if (C == 256) { NOPE_DISPATCH_T(sdt, T, hipLaunchKernelGGL((token_attn_kernel<T, 256>), grid, dim3(NT), 0, s, (const T*)qkv, (T*)out, N, C, scale)); }
    else { NOPE_DISPATCH_T(sdt, T, hipLaunchKernelGGL((token_attn_kernel<T, 512>), grid, dim3(NT), 0, s, (const T*)qkv, (T*)out, N, C, scale)); }
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_avg_pool2(int dt, const void* x, void* y, long long n, int H, int W, int C, hipStream_t s) {
    const int vec = dt_vec(dt);
    if (!x || !y || n <= 0 || H <= 0 || W <= 0 || H % 2 || W % 2 || C <= 0 || C % vec) return NOPE_ERR_ARG;
    const dim3 grid(grid_for_ll(n * (H / 2) * (W / 2) * (C / vec)));
    NOPE_DISPATCH_T(dt, T, hipLaunchKernelGGL((avg_pool2_kernel<T>), grid, dim3(NT), 0, s, (const T*)x, (T*)y, n, H / 2, W / 2, C));
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_nearest2(int dt, const void* x, void* y, long long n, int H, int W, int C, hipStream_t s) {
    const int vec = dt_vec(dt);
    if (!x || !y || n <= 0 || H <= 0 || W <= 0 || C <= 0 || C % vec) return NOPE_ERR_ARG;
    const dim3 grid(grid_for_ll(n * H * W * (C / vec)));
    NOPE_DISPATCH_T(dt, T, hipLaunchKernelGGL((nearest2_kernel<T>), grid, dim3(NT), 0, s, (const T*)x, (T*)y, n, H, W, C));
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_copy_cols(int dt, const void* x, void* y, long long M, int C, int C2, int off, hipStream_t s) {
    const int vec = dt_vec(dt);
    if (!x || !y || M <= 0 || C % vec || C2 % vec || off % vec || off + C > C2) return NOPE_ERR_ARG;
    const dim3 grid(grid_for_ll(M * (C / vec)));
    NOPE_DISPATCH_T(dt, T, hipLaunchKernelGGL((copy_cols_kernel<T>), grid, dim3(NT), 0, s, (const T*)x, (T*)y, M, C, C2, off));
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

}  // namespace nope
