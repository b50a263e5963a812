// Pose distribution and distinct pose modes from the retrieval scores (no reference counterpart: the
// reference stops at `similarity.topk(k=5)`, src/model/model.py:265, whose five entries are one grid vertex and four of its neighbours).
//
// Per query b (one workgroup), from its score row s[0..N) and the template grid:
//   p[n] = exp((s[n] - max s) / temperature) / Z,   entropy = -sum p ln p = ln Z - (sum e x) / Z   with x = (s - max) / temperature, e = exp(x)
// in f64 (a term with e = 0 contributes 0: -inf is an ordinary score), rounded once to the f32 outputs.  A row whose maximum is NaN or
// +-inf (a NaN or +inf anywhere, or -inf everywhere) is undefined: NaN prob / entropy, no modes, *status bit 0.
//   modes: greedy suppression.  All templates alive; the seed of slot m is the alive template with the highest score (ties -> lowest index,
//   nope_topk's rule); its members are the alive templates within radius_rad of it (the seed always, a NaN distance never); they leave.
//   left-over slots: empty (fill = 0) or the best templates not yet listed, nope_topk's order, with mass 0 and count 0 (fill = 1).
//
// The distance d is THIS op's, f64, over the three symmetry classes of nope_op_geodesic (kernels_metric.hip):
//   theta(A, B) = acos(clamp((tr(A B^T) - 1) / 2, -1, 1))
//   symmetry 0  theta(A, B);   symmetry 1  min(theta(A, B), theta(diag(-1, 1, -1) A, B));
//   symmetry 2  acos(clamp(cos)) between the viewing axes -inv(P)[2, :], norms floored at 1e-8
// It does NOT reproduce what the reported metric carries over from the reference: the f32 round trips of the flipped pose, pytorch3d's
// linear extrapolation of acos beyond +-(1 - 1e-4) (a self-distance of 0.0071 rad) and the unclamped acos of the circular branch (NaN
// between viewpoints of equal elevation).  That is right for a reported number and wrong for a membership decision; the two differ by
// <= 0.0071 rad, near 0 (and near pi) only.
//
// Layout.  Thread t owns the templates n = t (mod 256), in ascending order: every sweep over the row is a coalesced strided loop.  Its
// alive flags are bits of its OWN LDS words (s_alive[word * 256 + t]: no two threads share a word, so no atomics and no barrier guards
// them; 32 words per thread bound N at 256 * 32 * 32 = 262144, NOPE_ERR_UNSUPPORTED beyond).  A slot costs ONE sweep: removing the
// members of the current seed and finding the best survivor -- the next seed -- happen in the same pass.  Reductions have a fixed
// shape (wave xor-tree over int shuffles -- a double travels as two ints --, then the four wave results in wave order): no
// floating-point atomics, bit-identical from run to run.  Nothing is read by the host and there is no workspace.
#include <cmath>
#include <cstring>

#include "nope_common.h"

namespace nope {

namespace {

constexpr int NT = 256;
constexpr int ALIVE_WORDS = 32;                      // per thread
constexpr int MODES_MAX_N = NT * 32 * ALIVE_WORDS;
constexpr int MODES_MAX_SLOTS = 64;
constexpr int NONE = 0x7fffffff;

struct Red {          // what one sweep hands to the workgroup: two f64 sums, a count, and the best (score, index) candidate
    double a, b;
    int cnt;
    float bestv;
    int besti;        // NONE: no candidate (ranks behind every real one, a real -inf score included)
};

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__device__ __forceinline__ double shfl_xor_f64(double v, int o) {
    int w[2];
    memcpy(w, &v, 8);
    w[0] = __shfl_xor(w[0], o, 64);
    w[1] = __shfl_xor(w[1], o, 64);
    memcpy(&v, w, 8);
    return v;
}

// every thread returns the same, fully reduced value
__device__ __forceinline__ Red block_reduce(Red r) {
    __shared__ double s_a[NT / 64], s_b[NT / 64];
    __shared__ int s_cnt[NT / 64], s_bi[NT / 64];
    __shared__ float s_bv[NT / 64];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        r.a += shfl_xor_f64(r.a, o);
        r.b += shfl_xor_f64(r.b, o);
        r.cnt += __shfl_xor(r.cnt, o, 64);
        const float ov = __shfl_xor(r.bestv, o, 64);
        const int oi = __shfl_xor(r.besti, o, 64);
        if (better(ov, oi, r.bestv, r.besti)) { r.bestv = ov; r.besti = oi; }
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_a[wave] = r.a; s_b[wave] = r.b; s_cnt[wave] = r.cnt; s_bv[wave] = r.bestv; s_bi[wave] = r.besti; }
    __syncthreads();
    Red t = {s_a[0], s_b[0], s_cnt[0], s_bv[0], s_bi[0]};
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) {
        t.a += s_a[w]; t.b += s_b[w]; t.cnt += s_cnt[w];
        if (better(s_bv[w], s_bi[w], t.bestv, t.besti)) { t.bestv = s_bv[w]; t.besti = s_bi[w]; }
    }
    __syncthreads();          // (the next reduction writes the same words)
    return t;
}

__device__ __forceinline__ double clamped_acos(double c) {      // a NaN stays a NaN
    return acos(c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c));
}

// the viewing axis -inv(M)[2, :] (adjugate / determinant), as kernels_metric.hip's neg_inv_row2, scaled to unit length (norm floored at 1e-8)
__device__ __forceinline__ void view_axis(const double* M, double* r) {
    const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
    const double det = M[0] * c00 + M[1] * c01 + M[2] * c02;
    const double a20 = M[3] * M[7] - M[4] * M[6], a21 = M[1] * M[6] - M[0] * M[7], a22 = M[0] * M[4] - M[1] * M[3];
    r[0] = -(a20 / det); r[1] = -(a21 / det); r[2] = -(a22 / det);
    const double n = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    const double f = n > 1e-8 ? n : 1e-8;
    r[0] /= f; r[1] /= f; r[2] /= f;
}

// d(A, S) for the seed pose S (saxis: its viewing axis, read for symmetry 2 only)
__device__ __forceinline__ double mode_distance(const double* A, const double* S, const double* saxis, int sym) {
    if (sym == 0 || sym == 1) {
        const double r0 = A[0] * S[0] + A[1] * S[1] + A[2] * S[2], r1 = A[3] * S[3] + A[4] * S[4] + A[5] * S[5],
                     r2 = A[6] * S[6] + A[7] * S[7] + A[8] * S[8];
        const double d0 = clamped_acos((r0 + r1 + r2 - 1.0) * 0.5);
        if (sym == 0) return d0;
        const double d1 = clamped_acos((-r0 + r1 - r2 - 1.0) * 0.5);      // diag(-1, 1, -1) A: rows 0 and 2 negated
        return d1 < d0 ? d1 : d0;                                         // (a NaN in either is a NaN in both)
    }
    double a[3];
    view_axis(A, a);
    return clamped_acos(a[0] * saxis[0] + a[1] * saxis[1] + a[2] * saxis[2]);
}

__global__ __launch_bounds__(NT) void pose_modes_kernel(const float* __restrict__ sim, long long sim_ld, const double* __restrict__ poses,
                                                        long long stride_b, int N, const int* __restrict__ symmetry, double temperature,
                                                        double radius, int max_modes, int fill, float* __restrict__ prob, long long prob_ld,
                                                        float* __restrict__ entropy, long long* __restrict__ mode_idx,
                                                        float* __restrict__ mode_score, float* __restrict__ mode_mass,
                                                        int* __restrict__ mode_count, int* __restrict__ n_modes, int* __restrict__ status) {
    __shared__ unsigned s_alive[ALIVE_WORDS * NT];
    __shared__ int s_seed[MODES_MAX_SLOTS];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* s = sim + (size_t)b * sim_ld;
    const float ninf = -__builtin_huge_valf(), qnan = __builtin_nanf("");
    const size_t slot0 = (size_t)b * max_modes;

    // ---- the maximum (and the first seed), and whether the row is defined
    Red r = {0.0, 0.0, 0, ninf, NONE};
    for (int n = t; n < N; n += NT) {
        const float v = s[n];
        if (v != v || v == __builtin_huge_valf()) r.cnt = 1;
        if (v > r.bestv || r.besti == NONE) { r.bestv = v; r.besti = n; }
    }
    r = block_reduce(r);
    if (r.cnt > 0 || r.bestv == ninf) {
        if (prob) for (int n = t; n < N; n += NT) prob[(size_t)b * prob_ld + n] = qnan;
        for (int m = t; m < max_modes; m += NT) { mode_idx[slot0 + m] = -1; mode_score[slot0 + m] = qnan; mode_mass[slot0 + m] = 0.f; mode_count[slot0 + m] = 0; }
        if (t == 0) { entropy[b] = qnan; n_modes[b] = 0; atomicOr(status, 1); }
        return;
    }
    const double mx = (double)r.bestv;
    float seedv = r.bestv;
    int seed = r.besti;

    // ---- Z and the entropy
    r = {0.0, 0.0, 0, ninf, NONE};
    for (int n = t; n < N; n += NT) {
        const double x = ((double)s[n] - mx) / temperature, e = exp(x);
        r.a += e;
        if (e > 0.0) r.b += e * x;
    }
    r = block_reduce(r);
    const double Z = r.a;
    if (t == 0) entropy[b] = (float)(log(Z) - r.b / Z);
    if (prob) for (int n = t; n < N; n += NT) prob[(size_t)b * prob_ld + n] = (float)(exp(((double)s[n] - mx) / temperature) / Z);
    if (max_modes == 0) {
        if (t == 0) n_modes[b] = 0;
        return;
    }

    // ---- greedy suppression.  Bit (q & 31) of word (q >> 5) of thread t is template q * 256 + t.
    const int mine = t < N ? (N - t + NT - 1) / NT : 0, nwords = ((N + NT - 1) / NT + 31) >> 5;
    for (int w = 0; w < nwords; ++w) {
        const int left = mine - 32 * w;
        s_alive[w * NT + t] = left >= 32 ? 0xffffffffu : (left > 0 ? (1u << left) - 1u : 0u);
    }
    const double* P = poses + (size_t)b * stride_b;
    const int sym = symmetry ? symmetry[b] : 0;
    int filled = 0;
    for (; filled < max_modes;) {
        double S[9], saxis[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int e = 0; e < 9; ++e) S[e] = P[(size_t)seed * 9 + e];
        if (sym != 0 && sym != 1) view_axis(S, saxis);
        r = {0.0, 0.0, 0, ninf, NONE};
        for (int w = 0; w < nwords; ++w) {
            const unsigned word = s_alive[w * NT + t];
            unsigned keep = word;
            for (unsigned bits = word; bits; bits &= bits - 1) {
                const int bit = __builtin_ctz(bits), n = (32 * w + bit) * NT + t;
                double A[9];
#pragma unroll
                for (int e = 0; e < 9; ++e) A[e] = P[(size_t)n * 9 + e];
                const float v = s[n];
                if (n == seed || mode_distance(A, S, saxis, sym) <= radius) {
                    keep &= ~(1u << bit);
                    r.a += exp(((double)v - mx) / temperature) / Z;
                    r.cnt += 1;
                } else if (v > r.bestv || r.besti == NONE) { r.bestv = v; r.besti = n; }      // (n ascends within a thread: ties keep the lower index)
            }
            s_alive[w * NT + t] = keep;
        }
        r = block_reduce(r);
        if (t == 0) {
            mode_idx[slot0 + filled] = seed; mode_score[slot0 + filled] = seedv; mode_mass[slot0 + filled] = (float)r.a;
            mode_count[slot0 + filled] = r.cnt; s_seed[filled] = seed;
        }
        ++filled;
        if (r.besti == NONE) break;       // nothing is alive
        seedv = r.bestv; seed = r.besti;
    }
    if (t == 0) n_modes[b] = filled;
    if (filled == max_modes) return;
    if (!fill) {
        for (int m = filled + t; m < max_modes; m += NT) { mode_idx[slot0 + m] = -1; mode_score[slot0 + m] = ninf; mode_mass[slot0 + m] = 0.f; mode_count[slot0 + m] = 0; }
        return;
    }

    // ---- fill: everything but the seeds is a candidate again; each thread keeps the best of its own, and only the owner of a winner looks again
    __syncthreads();          // s_seed
    for (int w = 0; w < nwords; ++w) {
        const int left = mine - 32 * w;
        s_alive[w * NT + t] = left >= 32 ? 0xffffffffu : (left > 0 ? (1u << left) - 1u : 0u);
    }
    for (int j = 0; j < filled; ++j) {
        const int n = s_seed[j];
        if (n % NT == t) s_alive[((n / NT) >> 5) * NT + t] &= ~(1u << ((n / NT) & 31));
    }
    bool rescan = true;
    Red local = {0.0, 0.0, 0, ninf, NONE};
    for (int m = filled; m < max_modes; ++m) {         // (max_modes <= N: a candidate is always left)
        if (rescan) {
            local = {0.0, 0.0, 0, ninf, NONE};
            for (int w = 0; w < nwords; ++w)
                for (unsigned bits = s_alive[w * NT + t]; bits; bits &= bits - 1) {
                    const int n = (32 * w + __builtin_ctz(bits)) * NT + t;
                    const float v = s[n];
                    if (v > local.bestv || local.besti == NONE) { local.bestv = v; local.besti = n; }
                }
        }
        r = block_reduce(local);
        rescan = r.besti != NONE && r.besti % NT == t;
        if (rescan) s_alive[((r.besti / NT) >> 5) * NT + t] &= ~(1u << ((r.besti / NT) & 31));
        if (t == 0) { mode_idx[slot0 + m] = r.besti == NONE ? -1 : r.besti; mode_score[slot0 + m] = r.bestv; mode_mass[slot0 + m] = 0.f; mode_count[slot0 + m] = 0; }
    }
}

}  // namespace

int launch_pose_modes(const float* sim, long long sim_ld, const double* poses, long long stride_b, int N, const int* symmetry,
                      double temperature, double radius_rad, int max_modes, int fill, float* prob, long long prob_ld, float* entropy,
                      long long* mode_idx, float* mode_score, float* mode_mass, int* mode_count, int* n_modes, int* status, int B,
                      hipStream_t s) {
    if (!sim || !entropy || !n_modes || !status || B <= 0 || N < 1 || sim_ld < N || stride_b < 0) return NOPE_ERR_ARG;
    if (prob && prob_ld < N) return NOPE_ERR_ARG;
    if (!(temperature > 0.0) || !std::isfinite(temperature) || !(radius_rad >= 0.0)) return NOPE_ERR_ARG;
    if (max_modes < 0 || max_modes > MODES_MAX_SLOTS || (fill && max_modes > N)) return NOPE_ERR_ARG;
    if (max_modes > 0 && (!poses || !mode_idx || !mode_score || !mode_mass || !mode_count)) return NOPE_ERR_ARG;
    if (N > MODES_MAX_N) return NOPE_ERR_UNSUPPORTED;
    if (hipMemsetAsync(status, 0, sizeof(int), s) != hipSuccess) return NOPE_ERR_LAUNCH;
    hipLaunchKernelGGL(pose_modes_kernel, dim3((unsigned)B), dim3(NT), 0, s, sim, sim_ld, poses, stride_b, N, symmetry, temperature, radius_rad,
                       max_modes, fill ? 1 : 0, prob, prob_ld, entropy, mode_idx, mode_score, mode_mass, mode_count, n_modes, status);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

}  // namespace nope
