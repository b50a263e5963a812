// Multi-reference pose retrieval (no reference counterpart: the reference has one reference image per object,
// src/model/model.py:313,323).  Five entries:
//
//   multiref_prepare      per (query b, reference r, grid pose n): the relative pose the U-Net is asked for (first two rows of T[n] P[b, r]^T),
//                         the distance d[b, r, n] between T[n] and P[b, r] (kernels_search.hip's two kinds) and the blend weight w[b, r, n]
//                         (uniform / softmax over the references at temperature tau / nearest).  f64, one launch, no atomics: a thread owns
//                         one (b, n) and walks the references in ascending order; the status word is written by ONE thread of ONE
//                         workgroup, which looks at every reference pose and count itself.
//   multiref_similarity   the hot path: score[b, n] = - sum_p sqrt( sum_c (q - tbar)^4 ) against the blend of R banks,
//                         tbar = sum_r w[b, r, n] t[b, r, n, c, p], in ONE streaming pass -- the blend is never written anywhere.
//   multiref_fuse_scores  late fusion: score[b, n] = f32( sum_r f64(w) f64(s[b, r, n]) ).
//
//   multiref_select        per (query b, slot s): the M nearest references of grid pose s -- or of pose cand[b, s] --, their
//                         relative poses and blend weights; multiref_prepare's distance and row arithmetic, so the bits agree.
//   multiref_gather       out[b, j, :] = reference_feats[b, src[b, j], :]: the source embedding of every hypothesis, 16-byte copies.
//
// The scoring kernels follow kernels_retrieval.hip's sim_reg_kernel / sim_lds_kernel (same lane -> pixel-vector mapping, same reductions,
// same per-type square root), whose small load / unpack helpers are restated here: that file does not change, and neither do its kernels'
// registers.  What is new is the order of the loads.  Channel-outer, reference-inner: a lane blends the R planes of one channel into LV
// live registers, takes the quartic difference against its query registers and moves on, so the blend costs LV registers whatever R is.
// The loads in flight are a block of SLOTS = 8 planes -- CB = 8 / RT channels by RT references, RT = R rounded up to 1, 2, 4 or 8 -- in one
// register set of 8 raw vectors, kernels_retrieval.hip's budget: slot (cc, r) is refilled with channel c + CB of the same hypothesis group
// (or, behind the group's last channels, with the next group's channel cc) right after channel c was consumed, so every lane keeps up to 8
// sixteen-byte loads in flight across the reduction and the barrier, as the single-reference kernel does.
//
// The blend is t = 0.0f; for r ascending: if (w[r] != 0) t = muladd(w[r], float(bank), t) -- one fma on the device (nope_common.h: muladd;
// the interpreter build of tests/ multiplies and adds).  A zero weight is a select, never a product: whatever its plane holds, NaN and inf
// included, does not reach the sum.  NaN != 0: a NaN weight gives a NaN score.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "nope_common.h"

namespace nope {

namespace {

constexpr int NT = 256;
constexpr int MR_MAX_REFS = 8;
constexpr int SLOTS = 8;                  // raw vectors a lane keeps in flight

// ---- kernels_retrieval.hip's helpers, restated (a lane's share of one channel plane: LV consecutive pixels = W 32-bit words = 16 bytes) ----
template <int W> struct RawVec { unsigned w[W]; };

template <bool NTL> __device__ __forceinline__ RawVec<4> ld_stream(const void* p) {     // streaming: every bank byte is read once per launch
    RawVec<4> r;
    const u32x4 v = NTL ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)) : *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) r.w[i] = v[i];
    return r;
}

template <class T> __device__ __forceinline__ void unpack_words(const RawVec<4>& raw, float* t) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = __builtin_bit_cast(float, raw.w[i]);
    } else if constexpr (Elt<T>::DT == NOPE_BF16) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            t[2 * i] = __builtin_bit_cast(float, raw.w[i] << 16);
            t[2 * i + 1] = __builtin_bit_cast(float, raw.w[i] & 0xffff0000u);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            union { unsigned u; f16_t h[2]; } x; x.u = raw.w[i];
            t[2 * i] = (float)x.h[0];
            t[2 * i + 1] = (float)x.h[1];
        }
    }
}

// tbar += w * plane (a zero weight: nothing, whatever the plane holds)
template <class T, int LV> __device__ __forceinline__ void blend_plane(const RawVec<4>& raw, float w, float* tbar) {
    float t[LV];
    unpack_words<T>(raw, t);
#pragma unroll
    for (int e = 0; e < LV; ++e) tbar[e] = w != 0.f ? muladd(w, t[e], tbar[e]) : tbar[e];
}

template <int LV> __device__ __forceinline__ void accum_quartic(const float* tbar, const float* q, float* acc) {
#pragma unroll
    for (int e = 0; e < LV; ++e) {
        const float d = q[e] - tbar[e];
        const float d2 = d * d;
        acc[e] += d2 * d2;
    }
}

// Register-tile form.  A lane owns LV = 16 bytes' worth of consecutive pixels of every channel plane; P = HW / LV lanes make a hypothesis
// (P <= 256, 256 % P == 0); hpi = 256 / P hypotheses per iteration; workgroup (b, split) scores the groups split, split + nsplit, ... of
// sample b: kernels_retrieval.hip's walk.  RT: references per slot block (R <= RT); CMAX: the unrolled channel count (C <= CMAX).
template <class T, int CMAX, int RT>
__global__ __launch_bounds__(NT) void mr_reg_kernel(const float* __restrict__ q, const T* __restrict__ bank, const float* __restrict__ weights,
                                                    float* __restrict__ scores, int N, int R, int C, int HW, int score_ld, int nsplit) {
    constexpr int LV = 16 / (int)sizeof(T);
    constexpr int CB = SLOTS / RT;            // channels per slot block
    __shared__ float s_part[2][NT / 64];
    const int P = HW / LV;
    const int hpi = NT / P;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = tid / P, pv = tid - sub * P;
    const int b = blockIdx.x / nsplit, split = blockIdx.x - b * nsplit;
    const int groups = (N + hpi - 1) / hpi;
    const int g0 = split, g1 = groups, gs = nsplit;

    float qr[CMAX][LV];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        if (c < C) {
            const float* qp = q + ((size_t)b * C + c) * HW + (size_t)pv * LV;
#pragma unroll
            for (int v4 = 0; v4 < LV / 4; ++v4) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(qp + 4 * v4);
#pragma unroll
                for (int e = 0; e < 4; ++e) qr[c][4 * v4 + e] = x[e];
            }
        }
    }
    const size_t hyp_elems = (size_t)C * HW;
    const size_t ref_elems = (size_t)N * hyp_elems;                          // from reference r to r + 1 of the same sample and pose
    const T* bb = bank + (size_t)b * R * ref_elems + (size_t)pv * LV;
    const float* wb = weights + (size_t)b * R * N;
    int buf = 0;
    RawVec<4> raw[CB][RT];
    float wcur[RT], wnext[RT];
    auto hyp_of = [&](int g) { const int n = g * hpi + sub; return n < N ? n : 0; };      // (a ragged last group reads template 0 and writes nothing)
    if (g0 < g1) {
        const int n = hyp_of(g0);
        const T* tp = bb + (size_t)n * hyp_elems;
#pragma unroll
        for (int r = 0; r < RT; ++r) wcur[r] = r < R ? wb[(size_t)r * N + n] : 0.f;
#pragma unroll
        for (int cc = 0; cc < CB; ++cc)
#pragma unroll
            for (int r = 0; r < RT; ++r)
                if (cc < C && r < R) raw[cc][r] = ld_stream<true>(tp + (size_t)r * ref_elems + (size_t)cc * HW);
    }
    // (the last group is peeled, as in sim_reg_kernel: a runtime `if (more)` around the prefetch makes the compiler keep a second register set)
    auto body = [&](int g, auto more_tag) __attribute__((always_inline)) {
        constexpr bool MORE = decltype(more_tag)::value;
        const int n = g * hpi + sub;
        const T* tc = bb + (size_t)hyp_of(g) * hyp_elems;
        const T* tn = tc;
        if constexpr (MORE) {
            const int nn = hyp_of(g + gs);
            tn = bb + (size_t)nn * hyp_elems;
#pragma unroll
            for (int r = 0; r < RT; ++r) wnext[r] = r < R ? wb[(size_t)r * N + nn] : 0.f;
        }
        float acc[LV];
#pragma unroll
        for (int e = 0; e < LV; ++e) acc[e] = 0.f;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) {
                const int cc = c % CB;
                float tbar[LV];
#pragma unroll
                for (int e = 0; e < LV; ++e) tbar[e] = 0.f;
#pragma unroll
                for (int r = 0; r < RT; ++r)
                    if (r < R) {
                        blend_plane<T, LV>(raw[c % CB][r], wcur[r], tbar);
                        // refill the slot: channel c + CB of this group, or the next group's channel cc
                        if (c + CB < C) raw[c % CB][r] = ld_stream<true>(tc + (size_t)r * ref_elems + (size_t)(c + CB) * HW);
                        else if (MORE) raw[c % CB][r] = ld_stream<true>(tn + (size_t)r * ref_elems + (size_t)cc * HW);
                    }
                accum_quartic<LV>(tbar, qr[c], acc);
                __builtin_amdgcn_sched_barrier(0);      // (one channel at a time: unpacking the planes ahead costs registers)
            }
        if constexpr (MORE) {
#pragma unroll
            for (int r = 0; r < RT; ++r) wcur[r] = wnext[r];
        }
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < LV; ++e) s += sizeof(T) == 4 ? sqrtf(acc[e]) : __builtin_amdgcn_sqrtf(acc[e]);      // nope_similarity's choice per bank type
        if (P >= 64) {
            s = wave_sum(s);
            if (lane == 0) s_part[buf][wave] = s;
            __syncthreads();
            if (pv == 0 && n < N) {
                const int w0 = sub * (P / 64);
                float tot = 0.f;
                for (int w = 0; w < P / 64; ++w) tot += s_part[buf][w0 + w];
                scores[(size_t)b * score_ld + n] = -tot;
            }
            buf ^= 1;   // double-buffered partials: one barrier per iteration
        } else {
            for (int o = P >> 1; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
            if (pv == 0 && n < N) scores[(size_t)b * score_ld + n] = -s;
        }
    };
    int g = g0;
    for (; g + gs < g1; g += gs) body(g, BoolTag<true>{});
    if (g < g1) body(g, BoolTag<false>{});
}

// Generic shapes: one hypothesis per iteration, query tile in LDS (C * HW * 4 <= 64 KiB), sim_lds_kernel's walk.
template <class T>
__global__ __launch_bounds__(NT) void mr_lds_kernel(const float* __restrict__ q, const T* __restrict__ bank, const float* __restrict__ weights,
                                                    float* __restrict__ scores, int N, int R, int C, int HW, int score_ld, int nsplit) {
    constexpr int VEC = Elt<T>::VEC;
    __shared__ __attribute__((aligned(16))) float s_q[16384];
    __shared__ float s_part[NT / 64];
    const int P = HW / VEC;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / nsplit, split = blockIdx.x - b * nsplit;
    const int nper = (N + nsplit - 1) / nsplit;
    const int n0 = split * nper;
    const int n1 = (n0 + nper < N) ? n0 + nper : N;
    for (int i = tid; i < C * HW; i += NT) s_q[i] = q[(size_t)b * C * HW + i];
    __syncthreads();
    const size_t hyp_elems = (size_t)C * HW, ref_elems = (size_t)N * hyp_elems;
    const T* bb = bank + (size_t)b * R * ref_elems;
    const float* wb = weights + (size_t)b * R * N;
    for (int n = n0; n < n1; ++n) {
        const T* tp = bb + (size_t)n * hyp_elems;
        float s = 0.f;
        for (int pv = tid; pv < P; pv += NT) {
            float acc[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
            for (int c = 0; c < C; ++c) {
                float tbar[VEC];
#pragma unroll
                for (int e = 0; e < VEC; ++e) tbar[e] = 0.f;
                for (int r = 0; r < R; ++r)
                    blend_plane<T, VEC>(ld_stream<false>(tp + (size_t)r * ref_elems + (size_t)c * HW + (size_t)pv * VEC), wb[(size_t)r * N + n], tbar);
                accum_quartic<VEC>(tbar, &s_q[c * HW + pv * VEC], acc);
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) s += sqrtf(acc[e]);
        }
        s = wave_sum(s);
        if (lane == 0) s_part[wave] = s;
        __syncthreads();
        if (tid == 0) {
            float tot = 0.f;
#pragma unroll
            for (int w = 0; w < NT / 64; ++w) tot += s_part[w];
            scores[(size_t)b * score_ld + n] = -tot;
        }
        __syncthreads();
    }
}

// ---- prepare --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double clamped_acos(double c) {      // a NaN stays a NaN
    return acos(c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c));
}

// d(A, S): A, S 3 x 3 row-major; kernels_search.hip's c2f_distance
__device__ __forceinline__ double mr_distance(const double* A, const double* S, int kind) {
    if (kind == 0) {
        double tr = 0.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) tr += A[e] * S[e];
        return clamped_acos((tr - 1.0) * 0.5);
    }
    const double na = sqrt(A[6] * A[6] + A[7] * A[7] + A[8] * A[8]), ns = sqrt(S[6] * S[6] + S[7] * S[7] + S[8] * S[8]);
    const double fa = na > 1e-8 ? na : 1e-8, fs = ns > 1e-8 ? ns : 1e-8;
    return clamped_acos((A[6] * S[6] + A[7] * S[7] + A[8] * S[8]) / (fa * fs));
}

__device__ __forceinline__ bool finite_f64(double v) { return v - v == 0.0; }       // false for NaN and +-inf

// status bits of sample b: 1 = a valid reference pose holds a non-finite entry, 2 = n_refs[b] outside [1, R]
__device__ __forceinline__ int mr_sample_status(const double* __restrict__ ref_poses, const int* __restrict__ n_refs, int R, int b) {
    const int nr = n_refs ? n_refs[b] : R;
    if (nr < 1 || nr > R) return 2;
    int bits = 0;
    for (int i = 0; i < nr * 9; ++i)
        if (!finite_f64(ref_poses[(size_t)b * R * 9 + i])) bits = 1;
    return bits;
}

// grid (chunks of 256 poses, B); thread -> one (b, n), the references in ascending order
__global__ __launch_bounds__(NT) void multiref_prepare_kernel(const double* __restrict__ tpl, long long stride_b, int N, const double* __restrict__ ref_poses,
                                                              int R, const int* __restrict__ n_refs, int weighting, double tau, int kind,
                                                              float* __restrict__ rel, float* __restrict__ weights, double* __restrict__ dist,
                                                              int* __restrict__ status, int B) {
    __shared__ int s_bits[NT / 64];
    const int b = blockIdx.y, t = threadIdx.x, n = blockIdx.x * NT + t;
    if (blockIdx.x == 0 && blockIdx.y == 0) {         // the status word: one writer, a plain store
        int bits = 0;
        for (int s = t; s < B; s += NT) bits |= mr_sample_status(ref_poses, n_refs, R, s);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) bits |= __shfl_xor(bits, o, 64);
        if ((t & 63) == 0) s_bits[t >> 6] = bits;
        __syncthreads();
        if (t == 0) {
            int all = 0;
#pragma unroll
            for (int w = 0; w < NT / 64; ++w) all |= s_bits[w];
            *status = all;
        }
    }
    if (n >= N) return;
    const bool bad = mr_sample_status(ref_poses, n_refs, R, b) != 0;        // (uniform over the workgroup)
    const int nr = n_refs ? n_refs[b] : R;
    const double* Pb = ref_poses + (size_t)b * R * 9;
    double T[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) T[e] = tpl[(size_t)b * stride_b + (size_t)n * 9 + e];
    const double inf = (double)__builtin_huge_valf();
    const float qnan = __builtin_nanf("");

    double d[MR_MAX_REFS];
    double dmin = inf;
    int best = 0;
#pragma unroll
    for (int r = 0; r < MR_MAX_REFS; ++r) {
        d[r] = inf;
        if (r < R) {
            const bool valid = r < nr;
            const double* S = Pb + (size_t)(valid ? r : 0) * 9;       // a padded reference carries the rows of reference 0
            double Pr[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) Pr[e] = S[e];
            if (valid) {
                d[r] = mr_distance(T, Pr, kind);
                if (d[r] < dmin) { dmin = d[r]; best = r; }          // (strict: a tie keeps the lower r)
            }
            const size_t o = ((size_t)b * R + r) * N + n;
            if (dist) dist[o] = d[r];
            if (rel) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        rel[o * 6 + i * 3 + j] = (float)(T[i * 3] * Pr[j * 3] + T[i * 3 + 1] * Pr[j * 3 + 1] + T[i * 3 + 2] * Pr[j * 3 + 2]);
            }
        }
    }
    double e[MR_MAX_REFS], Z = 0.0;
    if (weighting == 1) {
#pragma unroll
        for (int r = 0; r < MR_MAX_REFS; ++r) {
            e[r] = 0.0;
            if (r < R && r < nr) { e[r] = exp(-(d[r] - dmin) / tau); Z += e[r]; }
        }
    }
#pragma unroll
    for (int r = 0; r < MR_MAX_REFS; ++r)
        if (r < R) {
            float w = 0.f;
            if (bad) w = qnan;
            else if (r < nr) w = weighting == 0 ? (float)(1.0 / (double)nr) : weighting == 1 ? (float)(e[r] / Z) : (r == best ? 1.f : 0.f);
            weights[((size_t)b * R + r) * N + n] = w;
        }
}

// late fusion; grid (chunks of 256 poses, B)
__global__ __launch_bounds__(NT) void multiref_fuse_kernel(const float* __restrict__ per_ref, const float* __restrict__ weights, float* __restrict__ scores,
                                                           int R, int N, long long score_ld) {
    const int b = blockIdx.y, n = blockIdx.x * NT + threadIdx.x;
    if (n >= N) return;
    double acc = 0.0;
    for (int r = 0; r < R; ++r) {
        const size_t o = ((size_t)b * R + r) * N + n;
        const float w = weights[o];
        if (w != 0.f) acc += (double)w * (double)per_ref[o];
    }
    scores[(size_t)b * score_ld + n] = (float)acc;
}

// ---- select: the M nearest references per (sample, slot) -----------------------------------------------------------------------------------
// (a, i) before (b, j) in the order "distance ascending, then index ascending, a NaN after every number"; i != j
__device__ __forceinline__ bool mr_before(double a, int i, double b, int j) {
    const bool an = a != a, bn = b != b;
    if (an || bn) return an == bn ? i < j : bn;
    return a < b || (a == b && i < j);
}

// first two rows of T P^T, f64 rounded once: multiref_prepare_kernel's expression, so the bits agree
__device__ __forceinline__ void mr_store_rows(const double* T, const double* Pr, float* __restrict__ rel) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            rel[i * 3 + j] = (float)(T[i * 3] * Pr[j * 3] + T[i * 3 + 1] * Pr[j * 3 + 1] + T[i * 3 + 2] * Pr[j * 3 + 2]);
}

// grid (chunks of 256 slots, B); thread -> one (b, slot): M rounds of "the smallest (d, r) not taken yet" over the references, every loop
// unrolled to MR_MAX_REFS and the taken references a bit mask, so d[] stays in registers
__global__ __launch_bounds__(NT) void multiref_select_kernel(const double* __restrict__ tpl, long long stride_b, int N, const double* __restrict__ ref_poses,
                                                             int R, const int* __restrict__ n_refs, const int* __restrict__ cand, int S, int M,
                                                             int weighting, double tau, int kind, int* __restrict__ src, float* __restrict__ rel,
                                                             float* __restrict__ weights, double* __restrict__ dist, int* __restrict__ status, int B) {
    __shared__ int s_bits[NT / 64];
    const int b = blockIdx.y, t = threadIdx.x, s = blockIdx.x * NT + t;
    if (blockIdx.x == 0 && blockIdx.y == 0) {         // the status word: one writer, a plain store
        int bits = 0;
        for (int i = t; i < B; i += NT) bits |= mr_sample_status(ref_poses, n_refs, R, i);
        if (cand)
            for (long long i = t; i < (long long)B * S; i += NT) {
                const int c = cand[i];
                if (c < -1 || c >= N) bits |= 4;
            }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) bits |= __shfl_xor(bits, o, 64);
        if ((t & 63) == 0) s_bits[t >> 6] = bits;
        __syncthreads();
        if (t == 0) {
            int all = 0;
#pragma unroll
            for (int w = 0; w < NT / 64; ++w) all |= s_bits[w];
            *status = all;
        }
    }
    if (s >= S) return;
    const bool bad = mr_sample_status(ref_poses, n_refs, R, b) != 0;
    int nr = n_refs ? n_refs[b] : R;
    nr = nr < 0 ? 0 : (nr > R ? R : nr);
    int p = cand ? cand[(size_t)b * S + s] : s;
    const bool pad = p < 0 || p >= N;                 // -1, or an entry out of range (status bit 2)
    if (pad) p = 0;
    const int Mv = pad ? 0 : (M < nr ? M : nr);
    const double* Pb = ref_poses + (size_t)b * R * 9;
    double T[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) T[e] = tpl[(size_t)b * stride_b + (size_t)p * 9 + e];
    const double inf = (double)__builtin_huge_valf();
    const float qnan = __builtin_nanf("");

    double d[MR_MAX_REFS];
#pragma unroll
    for (int r = 0; r < MR_MAX_REFS; ++r) {
        d[r] = inf;
        if (r < nr) {
            double Pr[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) Pr[e] = Pb[r * 9 + e];
            d[r] = mr_distance(T, Pr, kind);
        }
    }
    unsigned taken = 0;
    int first = 0;                                    // slot 0's reference: what the slots m >= Mv repeat
    double d0 = 0.0, e[MR_MAX_REFS], Z = 0.0;
#pragma unroll
    for (int m = 0; m < MR_MAX_REFS; ++m) {
        e[m] = 0.0;
        if (m < M) {
            int best = -1;
            double dbest = inf;
            if (m < Mv) {
#pragma unroll
                for (int r = 0; r < MR_MAX_REFS; ++r)
                    if (r < nr && !((taken >> r) & 1u) && (best < 0 || mr_before(d[r], r, dbest, best))) { best = r; dbest = d[r]; }
                taken |= 1u << best;
                if (m == 0) { first = best; d0 = dbest; }
                e[m] = weighting == 1 ? exp(-(dbest - d0) / tau) : 0.0;
                Z += e[m];
            } else {
                best = first;
            }
            const size_t o = ((size_t)b * M + m) * S + s;
            src[o] = best;
            if (dist) dist[o] = dbest;
            if (rel) {
                double Pr[9];
#pragma unroll
                for (int q = 0; q < 9; ++q) Pr[q] = Pb[best * 9 + q];
                mr_store_rows(T, Pr, rel + o * 6);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MR_MAX_REFS; ++m)
        if (m < M) {
            float w = 0.f;
            if (bad) w = qnan;
            else if (m < Mv) w = weighting == 0 ? (float)(1.0 / (double)Mv) : weighting == 1 ? (float)(e[m] / Z) : (m == 0 ? 1.f : 0.f);
            weights[((size_t)b * M + m) * S + s] = w;
        }
}

// gather: one workgroup per output row (b, j); 16-byte copies, bit for bit; a source outside [0, R) fills the row with NaN
__global__ __launch_bounds__(NT) void multiref_gather_kernel(const float* __restrict__ feats, const int* __restrict__ src, float* __restrict__ out, int R, int J,
                                                             int L4) {
    const size_t row = blockIdx.x;
    const int b = (int)(row / (size_t)J);
    const int r = src[row];
    u32x4* o = reinterpret_cast<u32x4*>(out) + row * (size_t)L4;
    if (r < 0 || r >= R) {
        const unsigned q = 0x7fc00000u;
        const u32x4 v = {q, q, q, q};
        for (int i = threadIdx.x; i < L4; i += NT) o[i] = v;
        return;
    }
    const u32x4* in = reinterpret_cast<const u32x4*>(feats) + ((size_t)b * R + r) * (size_t)L4;
    for (int i = threadIdx.x; i < L4; i += NT) o[i] = in[i];
}

}  // namespace

int launch_multiref_select(const double* template_poses, long long stride_b, int N, const double* ref_poses, int R, const int* n_refs, const int* cand,
                           int S, int M, int weighting, double tau_rad, int dist_kind, int* src, float* all_rel, float* weights, double* dist, int* status,
                           int B, hipStream_t s) {
    if (!template_poses || !ref_poses || !src || !weights || !status || B <= 0 || N < 1 || stride_b < 0) return NOPE_ERR_ARG;
    if (R < 1 || R > MR_MAX_REFS || M < 1 || M > R) return NOPE_ERR_ARG;
    if (weighting < 0 || weighting > 2 || (dist_kind != 0 && dist_kind != 1)) return NOPE_ERR_ARG;
    if (weighting == 1 && (!(tau_rad > 0.0) || !std::isfinite(tau_rad))) return NOPE_ERR_ARG;
    if (cand && S < 1) return NOPE_ERR_ARG;
    if (!cand) S = N;
    if (B > 65535) return NOPE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(multiref_select_kernel, dim3((unsigned)cdiv(S, NT), (unsigned)B), dim3(NT), 0, s, template_poses, stride_b, N, ref_poses, R, n_refs,
                       cand, S, M, weighting, tau_rad, dist_kind, src, all_rel, weights, dist, status, B);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_multiref_gather(const float* reference_feats, const int* src, float* out, int B, int R, int J, long long L, hipStream_t s) {
    if (!reference_feats || !src || !out || B < 1 || R < 1 || J < 1 || L < 1 || (L & 3)) return NOPE_ERR_ARG;
    if ((long long)B * J > 0x7fffffffLL || L / 4 > 0x7fffffffLL) return NOPE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(multiref_gather_kernel, dim3((unsigned)((long long)B * J)), dim3(NT), 0, s, reference_feats, src, out, R, J, (int)(L / 4));
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_multiref_prepare(const double* template_poses, long long stride_b, int N, const double* ref_poses, int R, const int* n_refs,
                            int weighting, double tau_rad, int dist_kind, float* all_rel, float* weights, double* dist, int* status, int B,
                            hipStream_t s) {
    if (!template_poses || !ref_poses || !weights || !status || B <= 0 || N < 1 || stride_b < 0) return NOPE_ERR_ARG;
    if (R < 1 || R > MR_MAX_REFS) return NOPE_ERR_ARG;
    if (weighting < 0 || weighting > 2 || (dist_kind != 0 && dist_kind != 1)) return NOPE_ERR_ARG;
    if (weighting == 1 && (!(tau_rad > 0.0) || !std::isfinite(tau_rad))) return NOPE_ERR_ARG;
    if (B > 65535) return NOPE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(multiref_prepare_kernel, dim3((unsigned)cdiv(N, NT), (unsigned)B), dim3(NT), 0, s, template_poses, stride_b, N, ref_poses, R,
                       n_refs, weighting, tau_rad, dist_kind, all_rel, weights, dist, status, B);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_multiref_fuse_scores(const float* per_ref, const float* weights, float* scores, int B, int R, int N, long long score_ld, hipStream_t s) {
    if (!per_ref || !weights || !scores || B <= 0 || N < 1 || R < 1 || R > MR_MAX_REFS || score_ld < N) return NOPE_ERR_ARG;
    if (B > 65535) return NOPE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(multiref_fuse_kernel, dim3((unsigned)cdiv(N, NT), (unsigned)B), dim3(NT), 0, s, per_ref, weights, scores, R, N, score_ld);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_multiref_similarity(const float* q, const void* bank, int bank_dt, const float* weights, float* scores, int B, int R, int N, int C, int HW,
                               int score_ld, hipStream_t s) {
    if (!q || !bank || !weights || !scores || B <= 0 || N <= 0 || C <= 0 || HW <= 0 || score_ld < N || R < 1 || R > MR_MAX_REFS) return NOPE_ERR_ARG;
    if (bank_dt != NOPE_F32 && bank_dt != NOPE_BF16 && bank_dt != NOPE_F16) return NOPE_ERR_UNSUPPORTED;
    const int vec = bank_dt == NOPE_F32 ? 4 : 8;
    if (HW % vec) return NOPE_ERR_UNSUPPORTED;
    const bool trace = NOPE_ENV_SET("NOPE_SIM_TRACE");      // test aid: one line per launch saying which form ran
    const char* const dt_name = bank_dt == NOPE_F32 ? "f32" : bank_dt == NOPE_BF16 ? "bf16" : "f16";
    const int P = HW / vec;
    const bool reg_ok = (P <= NT) && (NT % P == 0) && (C <= 16);
    int nsplit;
    if (reg_ok) {
        const int hpi = NT / P, groups = cdiv(N, hpi);
        const int rt = R == 1 ? 1 : R == 2 ? 2 : R <= 4 ? 4 : 8;
        // nsplit workgroups per sample, ~4096 in all, at least NOPE_SIM_MINGROUPS template groups each: nope_similarity's grid
        const int min_groups = NOPE_ENV("NOPE_SIM_MINGROUPS", 1);
        nsplit = 4096 / B;
        if (min_groups > 0 && nsplit > groups / min_groups) nsplit = groups / min_groups;
        if (nsplit > groups) nsplit = groups;
        if (nsplit < 1) nsplit = 1;
        if (trace) fprintf(stderr, "mrsim reg %s LV %d CMAX %d RT %d R %d P %d hpi %d groups %d nsplit %d\n", dt_name, vec, C <= 8 ? 8 : 16, rt, R, P, hpi,
                           groups, nsplit);
        const dim3 grid((unsigned)((long long)B * nsplit)), block(NT);
#define NOPE_MR_LAUNCH(T, CM, RTV)                                                                                                          \
        hipLaunchKernelGGL((mr_reg_kernel<T, CM, RTV>), grid, block, 0, s, q, (const T*)bank, weights, scores, N, R, C, HW, score_ld, nsplit)
#define NOPE_MR_RT(T, CM)                                                                                                                   \
        do {                                                                                                                                \
            if (rt == 1) NOPE_MR_LAUNCH(T, CM, 1); else if (rt == 2) NOPE_MR_LAUNCH(T, CM, 2); else if (rt == 4) NOPE_MR_LAUNCH(T, CM, 4);  \
            else NOPE_MR_LAUNCH(T, CM, 8);                                                                                                  \
        } while (0)
#define NOPE_MR_T(T)                                                                                                                        \
        do { if (C <= 8) NOPE_MR_RT(T, 8); else NOPE_MR_RT(T, 16); } while (0)
        if (bank_dt == NOPE_F32) NOPE_MR_T(float);
        else if (bank_dt == NOPE_BF16) NOPE_MR_T(bf16_t);
        else NOPE_MR_T(f16_t);
#undef NOPE_MR_T
#undef NOPE_MR_RT
#undef NOPE_MR_LAUNCH
    } else {
        if ((size_t)C * HW > 16384) return NOPE_ERR_UNSUPPORTED;
        nsplit = cdiv(4096, B);
        if (nsplit > N) nsplit = N;
        if (trace) fprintf(stderr, "mrsim lds %s LV %d CMAX 0 RT 0 R %d P %d hpi 1 groups %d nsplit %d\n", dt_name, vec, R, P, N, nsplit);
        const dim3 grid((unsigned)((long long)B * nsplit)), block(NT);
        if (bank_dt == NOPE_F32) hipLaunchKernelGGL((mr_lds_kernel<float>), grid, block, 0, s, q, (const float*)bank, weights, scores, N, R, C, HW, score_ld, nsplit);
        else if (bank_dt == NOPE_BF16) hipLaunchKernelGGL((mr_lds_kernel<bf16_t>), grid, block, 0, s, q, (const bf16_t*)bank, weights, scores, N, R, C, HW, score_ld, nsplit);
        else hipLaunchKernelGGL((mr_lds_kernel<f16_t>), grid, block, 0, s, q, (const f16_t*)bank, weights, scores, N, R, C, HW, score_ld, nsplit);
    }
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

}  // namespace nope
