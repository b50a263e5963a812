// Occlusion-robust template scoring (no reference counterpart: the reference scores every pixel of the latent map,
// src/model/model.py:257-262).  Three entries:
//
//   robust_similarity   score[b, n] = - (sum of the m smallest d[b, n, p] over the pixels p of the mask), d = sqrt(sum_c (q - t)^4),
//                       m = a - min(a - 1, floor(trim a)), a the number of mask pixels: a masked, least-trimmed form of nope_similarity.
//   residual_maps       the d planes of chosen hypotheses (f64 arithmetic, rounded once).
//   pool_mask           an image-resolution coverage plane -> the latent mask.
//
// The scoring kernels follow kernels_retrieval.hip's sim_reg_kernel / sim_lds_kernel (same lane -> pixel-vector mapping, same walk of the
// template groups, same depth-1 prefetch in one register set, same per-type square root), whose small load / unpack helpers are restated
// here: that file does not change, and neither do its kernels' registers.  What is new sits behind the channel loop, while the next
// group's C loads are in flight: a lane keeps its LV per-pixel d values as f32 bit patterns ("keys": d >= 0, so the patterns order as the
// values do) in the registers the accumulators lived in, and the P lanes of a hypothesis find the m-th smallest key exactly, one bit per
// round from bit 30 down: v is the largest x with count(key < x) < m.  A round's count is LV ballots and population counts per wave (scalar
// work; a hypothesis of fewer than 64 lanes masks the ballot to its own lanes), and above one wave per hypothesis one LDS exchange and one
// barrier on double-buffered partials.  The score is s_less + (m - c_less) v over the keys strictly below v, so equal values at the m-th
// position need no rule.  A pixel outside the mask and a NaN both carry the key 0xffffffff, above every number: the first is a select
// (nothing of it is ever multiplied), the second sets a flag that makes the score NaN whatever the trim.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "nope_common.h"

namespace nope {

namespace {

constexpr int NT = 256;
constexpr unsigned KEY_OUT = 0xffffffffu;            // a masked-out pixel or a NaN: above every d

// ---- kernels_retrieval.hip's helpers, restated (a lane's share of one channel plane: LV consecutive pixels = 4 32-bit words = 16 bytes) ----
struct RawVec { unsigned w[4]; };

template <bool NTL> __device__ __forceinline__ RawVec ld_stream(const void* p) {     // streaming: every bank byte is read once per launch
    RawVec r;
    const u32x4 v = NTL ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)) : *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) r.w[i] = v[i];
    return r;
}

template <class T> __device__ __forceinline__ void unpack_words(const RawVec& raw, float* t) {
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

template <class T, int LV> __device__ __forceinline__ void accum_quartic(const RawVec& raw, const float* q, float* acc) {
    float t[LV];
    unpack_words<T>(raw, t);
#pragma unroll
    for (int e = 0; e < LV; ++e) {
        const float d = q[e] - t[e];
        const float d2 = d * d;
        acc[e] += d2 * d2;
    }
}

// the number of kept terms: m = a - min(a - 1, floor(trim a)), one f32 product (a == 0: 1, and the caller writes NaN)
__device__ __forceinline__ int kept_terms(int a, float trim) {
    int t = (int)floorf(trim * (float)a);
    if (t > a - 1) t = a - 1;
    if (t < 0) t = 0;
    return a - t;
}

// Register-tile form: sim_reg_kernel's plan.  A lane owns LV = 16 bytes' worth of consecutive pixels of every channel plane; P = HW / LV lanes
// make a hypothesis (P <= 256, a power of two); hpi = 256 / P hypotheses per iteration; workgroup (b, split) scores the groups split,
// split + nsplit, ... of sample b.  CEXACT: C == CMAX, the per-channel guards fold away.  TRIM false: a plain masked sum, no selection.
template <class T, int CMAX, bool CEXACT, bool TRIM>
__global__ __launch_bounds__(NT) void rb_reg_kernel(const float* __restrict__ q, const T* __restrict__ bank, const unsigned char* __restrict__ mask,
                                                    float trim, float* __restrict__ scores, int N, int C, int HW, long long bank_stride_b,
                                                    int score_ld, int nsplit) {
    constexpr int LV = 16 / (int)sizeof(T);
    __shared__ float s_part[2][NT / 64];
    __shared__ int s_cnt[2][NT / 64];
    const int P = HW / LV;
    const int hpi = NT / P;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = tid / P, pv = tid - sub * P;
    const int b = blockIdx.x / nsplit, split = blockIdx.x - b * nsplit;
    const int groups = (N + hpi - 1) / hpi;
    const int g0 = split, g1 = groups, gs = nsplit;
    // the lanes of this lane's hypothesis inside its wave
    const unsigned long long submask = P >= 64 ? ~0ull : (((1ull << P) - 1ull) << ((lane / P) * P));
    int cbuf = 0;
    // pred(e), e < LV, over the P lanes of a hypothesis -> how many hold; every lane of the workgroup calls it (P > 64: a barrier)
    auto hyp_count = [&](auto pred) __attribute__((always_inline)) {
        int c = 0;
#pragma unroll
        for (int e = 0; e < LV; ++e) c += __builtin_popcountll(__ballot(pred(e)) & submask);
        if (P > 64) {
            if (lane == 0) s_cnt[cbuf][wave] = c;
            __syncthreads();
            const int w0 = sub * (P / 64);
            c = 0;
            for (int w = 0; w < P / 64; ++w) c += s_cnt[cbuf][w0 + w];
            cbuf ^= 1;      // double-buffered partials: one barrier per count
        }
        return c;
    };
    // the mask bytes of this lane's pixels: the FIRST load of the workgroup, consumed behind the first group's loads (they return in order)
    const bool mask_vec = (reinterpret_cast<size_t>(mask) & (size_t)(LV - 1)) == 0;          // LV bytes in one load (HW is a multiple of LV)
    unsigned mw[LV / 4];
#pragma unroll
    for (int i = 0; i < LV / 4; ++i) mw[i] = 0x01010101u;
    if (mask && mask_vec) {
#pragma unroll
        for (int i = 0; i < LV / 4; ++i) mw[i] = reinterpret_cast<const unsigned*>(mask + (size_t)b * HW + (size_t)pv * LV)[i];
    }

    float qr[CMAX][LV];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        if (CEXACT || c < C) {
            const float* qp = q + ((size_t)b * C + c) * HW + (size_t)pv * LV;
#pragma unroll
            for (int v4 = 0; v4 < LV / 4; ++v4) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(qp + 4 * v4);
#pragma unroll
                for (int e = 0; e < 4; ++e) qr[c][4 * v4 + e] = x[e];
            }
        }
    }
    const T* bb = bank + (size_t)b * bank_stride_b;
    const size_t hyp_elems = (size_t)C * HW;
    int buf = 0;
    RawVec raw[CMAX];
    auto plane_ptr = [&](int g) {
        const int n = g * hpi + sub;
        return bb + (size_t)(n < N ? n : 0) * hyp_elems + (size_t)pv * LV;      // (a ragged last group reads template 0 and writes nothing)
    };
    if (g0 < g1) {
        const T* tp = plane_ptr(g0);
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (CEXACT || c < C) raw[c] = ld_stream<true>(tp + (size_t)c * HW);
    }
    // bit e of mbits: pixel pv * LV + e is scored; a: the number of scored pixels
    if (mask && !mask_vec) {
        const unsigned char* mp = mask + (size_t)b * HW + (size_t)pv * LV;
#pragma unroll
        for (int e = 0; e < LV; ++e) mw[e >> 2] = (mw[e >> 2] & ~(0xffu << (8 * (e & 3)))) | ((unsigned)mp[e] << (8 * (e & 3)));
    }
    unsigned mbits = 0;
#pragma unroll
    for (int e = 0; e < LV; ++e) mbits |= (((mw[e >> 2] >> (8 * (e & 3))) & 0xffu) != 0 ? 1u : 0u) << e;
    const int a = hyp_count([&](int e) { return (int)((mbits >> e) & 1u); });
    const int m = TRIM ? kept_terms(a, trim) : a;
    // (the last group is peeled, as in sim_reg_kernel: a runtime `if (more)` around the prefetch makes the compiler keep a second register set)
    auto body = [&](int g, auto more_tag) __attribute__((always_inline)) {
        constexpr bool MORE = decltype(more_tag)::value;
        const T* tn = plane_ptr(MORE ? g + gs : g);
        const int n = g * hpi + sub;
        float acc[LV];
#pragma unroll
        for (int e = 0; e < LV; ++e) acc[e] = 0.f;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (CEXACT || c < C) {
                accum_quartic<T, LV>(raw[c], qr[c], acc);
                if constexpr (MORE) raw[c] = ld_stream<true>(tn + (size_t)c * HW);
                __builtin_amdgcn_sched_barrier(0);      // (one plane at a time: unpacking all C planes ahead costs registers)
            }
        float s = 0.f;
        float extra_v = 0.f;
        int rest = 0;
        if constexpr (!TRIM) {
#pragma unroll
            for (int e = 0; e < LV; ++e) {
                const float r = sizeof(T) == 4 ? sqrtf(acc[e]) : __builtin_amdgcn_sqrtf(acc[e]);      // nope_similarity's choice per bank type
                s += ((mbits >> e) & 1u) ? r : 0.f;                                                   // a select, never a product
            }
        } else {
            unsigned key[LV];
            bool has_nan = false;
#pragma unroll
            for (int e = 0; e < LV; ++e) {
                const float r = sizeof(T) == 4 ? sqrtf(acc[e]) : __builtin_amdgcn_sqrtf(acc[e]);
                const bool on = (mbits >> e) & 1u, isn = r != r;
                has_nan = has_nan || (on && isn);
                key[e] = (on && !isn) ? __builtin_bit_cast(unsigned, r) : KEY_OUT;
            }
            // v = the m-th smallest key = the largest x with count(key < x) < m, bit by bit (bit 31 is clear in every d).  (Two bits per round
            // -- three counts sharing one exchange, 16 rounds -- measured 1.2x slower: the compares and ballots cost, not the barriers.)
            unsigned v = 0;
            for (int bit = 30; bit >= 0; --bit) {
                const unsigned cand = v | (1u << bit);
                const int cnt = hyp_count([&](int e) { return (int)(key[e] < cand); });
                if (cnt < m) v = cand;
            }
            const int c_less = hyp_count([&](int e) { return (int)(key[e] < v); });
#pragma unroll
            for (int e = 0; e < LV; ++e) s += key[e] < v ? __builtin_bit_cast(float, key[e]) : 0.f;
            if (has_nan) s = __builtin_nanf("");
            rest = m - c_less;
            extra_v = __builtin_bit_cast(float, v);
        }
        // reduce over the P threads of this sub-hypothesis
        if (P >= 64) {
            s = wave_sum(s);
            if (lane == 0) s_part[buf][wave] = s;
            __syncthreads();
            if (pv == 0 && n < N) {
                const int w0 = sub * (P / 64);
                float tot = 0.f;
                for (int w = 0; w < P / 64; ++w) tot += s_part[buf][w0 + w];
                if (TRIM && rest > 0) tot += (float)rest * extra_v;
                scores[(size_t)b * score_ld + n] = a > 0 ? -tot : __builtin_nanf("");
            }
            buf ^= 1;   // double-buffered partials: one barrier per iteration
        } else {
            for (int o = P >> 1; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
            if (TRIM && rest > 0) s += (float)rest * extra_v;
            if (pv == 0 && n < N) scores[(size_t)b * score_ld + n] = a > 0 ? -s : __builtin_nanf("");
        }
    };
    int g = g0;
    for (; g + gs < g1; g += gs) body(g, BoolTag<true>{});
    if (g < g1) body(g, BoolTag<false>{});
}

// Generic shapes (sim_lds_kernel's walk): one hypothesis per iteration, its HW keys in LDS (HW <= 16384: 64 KiB), the query read through
// the caches.  Counts and sums are folded over the whole workgroup: wave butterfly, then the four wave partials in order.
template <class T>
__global__ __launch_bounds__(NT) void rb_gen_kernel(const float* __restrict__ q, const T* __restrict__ bank, const unsigned char* __restrict__ mask,
                                                    float trim, int do_trim, float* __restrict__ scores, int N, int C, int HW, long long bank_stride_b,
                                                    int score_ld, int nsplit) {
    constexpr int VEC = Elt<T>::VEC;
    __shared__ unsigned s_key[16384];
    __shared__ float s_part[2][NT / 64];
    __shared__ int s_cnt[2][NT / 64];
    const int P = HW / VEC;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / nsplit, split = blockIdx.x - b * nsplit;
    const int nper = (N + nsplit - 1) / nsplit;
    const int n0 = split * nper;
    const int n1 = (n0 + nper < N) ? n0 + nper : N;
    int cbuf = 0, buf = 0;
    auto block_count = [&](int c) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) s_cnt[cbuf][wave] = c;
        __syncthreads();
        c = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) c += s_cnt[cbuf][w];
        cbuf ^= 1;
        return c;
    };
    const unsigned char* mb = mask ? mask + (size_t)b * HW : nullptr;
    int mine = 0;
    for (int p = tid; p < HW; p += NT) mine += mb ? (mb[p] != 0 ? 1 : 0) : 1;
    const int a = block_count(mine);
    const int m = do_trim ? kept_terms(a, trim) : a;
    const T* bb = bank + (size_t)b * bank_stride_b;
    const float* qb = q + (size_t)b * C * HW;
    for (int n = n0; n < n1; ++n) {
        const T* tp = bb + (size_t)n * C * HW;
        bool has_nan = false;
        for (int pv = tid; pv < P; pv += NT) {
            float acc[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
            for (int c = 0; c < C; ++c)
                accum_quartic<T, VEC>(ld_stream<false>(tp + (size_t)c * HW + (size_t)pv * VEC), qb + (size_t)c * HW + (size_t)pv * VEC, acc);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float r = sqrtf(acc[e]);
                const int p = pv * VEC + e;
                const bool on = mb ? mb[p] != 0 : true, isn = r != r;
                has_nan = has_nan || (on && isn);
                s_key[p] = (on && !isn) ? __builtin_bit_cast(unsigned, r) : KEY_OUT;
            }
        }
        __syncthreads();
        unsigned v = KEY_OUT;          // no trim: every scored number lies below
        int c_less = m;
        if (do_trim) {
            v = 0;
            for (int bit = 30; bit >= 0; --bit) {
                const unsigned cand = v | (1u << bit);
                int c = 0;
                for (int p = tid; p < HW; p += NT) c += s_key[p] < cand ? 1 : 0;
                if (block_count(c) < m) v = cand;
            }
            int c = 0;
            for (int p = tid; p < HW; p += NT) c += s_key[p] < v ? 1 : 0;
            c_less = block_count(c);
        }
        float s = 0.f;
        for (int p = tid; p < HW; p += NT) {
            const unsigned k = s_key[p];
            s += k < v ? __builtin_bit_cast(float, k) : 0.f;
        }
        if (has_nan) s = __builtin_nanf("");
        s = wave_sum(s);
        if (lane == 0) s_part[buf][wave] = s;
        __syncthreads();               // (also: every read of s_key lies before it, the next hypothesis may overwrite the keys)
        if (tid == 0) {
            float tot = 0.f;
#pragma unroll
            for (int w = 0; w < NT / 64; ++w) tot += s_part[buf][w];
            if (do_trim && m - c_less > 0) tot += (float)(m - c_less) * __builtin_bit_cast(float, v);
            scores[(size_t)b * score_ld + n] = a > 0 ? -tot : __builtin_nanf("");
        }
        buf ^= 1;
    }
}

// ---- residual maps: one workgroup per (b, j) plane; f64 arithmetic, rounded once --------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(NT) void residual_maps_kernel(const float* __restrict__ q, const T* __restrict__ bank, const long long* __restrict__ idx,
                                                           float* __restrict__ out, int N, int k, int C, int HW, long long bank_stride_b) {
    const size_t row = blockIdx.x;
    const int b = (int)(row / (size_t)k), j = (int)(row - (size_t)b * k);
    const long long n = idx ? idx[row] : (long long)j;
    float* o = out + row * (size_t)HW;
    if (n < 0 || n >= N) {
        for (int p = threadIdx.x; p < HW; p += NT) o[p] = __builtin_nanf("");
        return;
    }
    const T* tp = bank + (size_t)b * bank_stride_b + (size_t)n * C * HW;
    const float* qb = q + (size_t)b * C * HW;
    for (int p = threadIdx.x; p < HW; p += NT) {
        double acc = 0.0;
        for (int c = 0; c < C; ++c) {
            const double d = (double)qb[(size_t)c * HW + p] - (double)Elt<T>::ld(tp + (size_t)c * HW + p);
            const double d2 = d * d;
            acc += d2 * d2;
        }
        o[p] = (float)sqrt(acc);
    }
}

// ---- pool mask: one thread per latent pixel -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void pool_mask_kernel(const void* __restrict__ cover, int is_u8, long long total, int Sh, int Sw, int H, int W,
                                                       long long min_sum_u8, float min_mean_f32, unsigned char* __restrict__ mask) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int w = (int)(i % W), h = (int)((i / W) % H);
    const long long b = i / ((long long)W * H);
    const int ch = Sh / H, cw = Sw / W;
    const size_t base = ((size_t)b * Sh + (size_t)h * ch) * Sw + (size_t)w * cw;
    bool on;
    if (is_u8) {
        const unsigned char* p = reinterpret_cast<const unsigned char*>(cover) + base;
        long long sum = 0;
        for (int y = 0; y < ch; ++y)
            for (int x = 0; x < cw; ++x) sum += p[(size_t)y * Sw + x];
        on = sum >= min_sum_u8;
    } else {
        const float* p = reinterpret_cast<const float*>(cover) + base;
        float sum = 0.f;
        for (int y = 0; y < ch; ++y)
            for (int x = 0; x < cw; ++x) sum += p[(size_t)y * Sw + x];
        on = sum / (float)(ch * cw) >= min_mean_f32;
    }
    mask[i] = on ? 1 : 0;
}

}  // namespace

int launch_robust_similarity(const float* q, const void* bank, int bank_dt, const unsigned char* mask, float trim, float* scores, int B, int N, int C,
                             int HW, long long bank_stride_b, int score_ld, hipStream_t s) {
    if (!q || !bank || !scores || B <= 0 || N <= 0 || C <= 0 || HW <= 0 || score_ld < N || bank_stride_b < 0) return NOPE_ERR_ARG;
    if (!(trim >= 0.f && trim < 1.f)) return NOPE_ERR_ARG;          // (a NaN fails both comparisons)
    if (bank_dt != NOPE_F32 && bank_dt != NOPE_BF16 && bank_dt != NOPE_F16) return NOPE_ERR_UNSUPPORTED;
    const int vec = bank_dt == NOPE_F32 ? 4 : 8;
    if (HW % vec) return NOPE_ERR_UNSUPPORTED;
    const bool trace = NOPE_ENV_SET("NOPE_SIM_TRACE");      // test aid: one line per launch saying which form ran
    const char* const dt_name = bank_dt == NOPE_F32 ? "f32" : bank_dt == NOPE_BF16 ? "bf16" : "f16";
    const bool do_trim = trim > 0.f;
    const int P = HW / vec;
    const bool reg_ok = (P <= NT) && (NT % P == 0) && (C <= 16);
    int nsplit;
    if (reg_ok) {
        const int hpi = NT / P, groups = cdiv(N, hpi);
        // nsplit workgroups per sample, ~4096 in all, at least NOPE_SIM_MINGROUPS template groups each: nope_similarity's grid
        const int min_groups = NOPE_ENV("NOPE_SIM_MINGROUPS", 1);
        nsplit = 4096 / B;
        if (min_groups > 0 && nsplit > groups / min_groups) nsplit = groups / min_groups;
        if (nsplit > groups) nsplit = groups;
        if (nsplit < 1) nsplit = 1;
        if (trace) fprintf(stderr, "rbsim reg %s LV %d CMAX %d CEXACT %d trim %d mask %d P %d hpi %d groups %d nsplit %d\n", dt_name, vec, C <= 8 ? 8 : 16,
                           (int)(C == 8 && !do_trim), (int)do_trim, (int)(mask != nullptr), P, hpi, groups, nsplit);
        const dim3 grid((unsigned)((long long)B * nsplit)), block(NT);
#define NOPE_RB_LAUNCH(T, CM, EX, TR)                                                                                                       \
        hipLaunchKernelGGL((rb_reg_kernel<T, CM, EX, TR>), grid, block, 0, s, q, (const T*)bank, mask, trim, scores, N, C, HW, bank_stride_b, score_ld, nsplit)
// (the selection form always takes the guarded channel loop: with C == CMAX folded the compiler keeps ~100 more registers live for the bf16 bank)
#define NOPE_RB_T(T)                                                                                                                        \
        do {                                                                                                                                \
            if (do_trim) { if (C <= 8) NOPE_RB_LAUNCH(T, 8, false, true); else NOPE_RB_LAUNCH(T, 16, false, true); }                        \
            else if (C == 8) NOPE_RB_LAUNCH(T, 8, true, false);                                                                             \
            else if (C < 8) NOPE_RB_LAUNCH(T, 8, false, false);                                                                             \
            else NOPE_RB_LAUNCH(T, 16, false, false);                                                                                       \
        } while (0)
        if (bank_dt == NOPE_F32) NOPE_RB_T(float);
        else if (bank_dt == NOPE_BF16) NOPE_RB_T(bf16_t);
        else NOPE_RB_T(f16_t);
#undef NOPE_RB_T
#undef NOPE_RB_LAUNCH
    } else {
        if ((size_t)C * HW > 16384) return NOPE_ERR_UNSUPPORTED;
        nsplit = cdiv(4096, B);
        if (nsplit > N) nsplit = N;
        if (trace) fprintf(stderr, "rbsim gen %s LV %d CMAX 0 CEXACT 0 trim %d mask %d P %d hpi 1 groups %d nsplit %d\n", dt_name, vec, (int)do_trim,
                           (int)(mask != nullptr), P, N, nsplit);
        const dim3 grid((unsigned)((long long)B * nsplit)), block(NT);
        if (bank_dt == NOPE_F32) hipLaunchKernelGGL((rb_gen_kernel<float>), grid, block, 0, s, q, (const float*)bank, mask, trim, (int)do_trim, scores, N, C, HW, bank_stride_b, score_ld, nsplit);
        else if (bank_dt == NOPE_BF16) hipLaunchKernelGGL((rb_gen_kernel<bf16_t>), grid, block, 0, s, q, (const bf16_t*)bank, mask, trim, (int)do_trim, scores, N, C, HW, bank_stride_b, score_ld, nsplit);
        else hipLaunchKernelGGL((rb_gen_kernel<f16_t>), grid, block, 0, s, q, (const f16_t*)bank, mask, trim, (int)do_trim, scores, N, C, HW, bank_stride_b, score_ld, nsplit);
    }
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_residual_maps(const float* q, const void* bank, int bank_dt, const long long* idx, float* out, int B, int N, int k, int C, int HW,
                         long long bank_stride_b, hipStream_t s) {
    if (!q || !bank || !out || B <= 0 || N <= 0 || k <= 0 || C <= 0 || HW <= 0 || bank_stride_b < 0) return NOPE_ERR_ARG;
    if (!idx && k > N) return NOPE_ERR_ARG;
    if (bank_dt != NOPE_F32 && bank_dt != NOPE_BF16 && bank_dt != NOPE_F16) return NOPE_ERR_UNSUPPORTED;
    if ((long long)B * k > 0x7fffffffLL) return NOPE_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((long long)B * k)), block(NT);
    if (bank_dt == NOPE_F32) hipLaunchKernelGGL((residual_maps_kernel<float>), grid, block, 0, s, q, (const float*)bank, idx, out, N, k, C, HW, bank_stride_b);
    else if (bank_dt == NOPE_BF16) hipLaunchKernelGGL((residual_maps_kernel<bf16_t>), grid, block, 0, s, q, (const bf16_t*)bank, idx, out, N, k, C, HW, bank_stride_b);
    else hipLaunchKernelGGL((residual_maps_kernel<f16_t>), grid, block, 0, s, q, (const f16_t*)bank, idx, out, N, k, C, HW, bank_stride_b);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_pool_mask(const void* cover, int is_u8, int B, int Sh, int Sw, int H, int W, long long min_sum_u8, float min_mean_f32, unsigned char* mask,
                     hipStream_t s) {
    if (!cover || !mask || B <= 0 || H <= 0 || W <= 0 || Sh <= 0 || Sw <= 0 || Sh % H || Sw % W) return NOPE_ERR_ARG;
    const long long total = (long long)B * H * W;
    if (total > 0x7fffffffLL * (long long)NT) return NOPE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pool_mask_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, s, cover, is_u8, total, Sh, Sw, H, W, min_sum_u8,
                       min_mean_f32, mask);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

}  // namespace nope
