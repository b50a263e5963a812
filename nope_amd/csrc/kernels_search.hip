// Coarse-to-fine pose retrieval over nested viewpoint grids (no reference counterpart: the reference scores every
// pose of the grid, src/model/model.py:313,323).  Two entries; the loop around them is nope_amd/search.py.
//
//   c2f_expand  per query b (one workgroup): which poses get a score at this stage, and their 6-D pose rows for the U-Net.
//     A pose p is eligible when stage_of[p] <= max_stage and state[b, p] == 0.  n_seeds == 0 (stage 0): every eligible pose, ascending.
//     Otherwise, seed by seed in the given order: the eligible poses p != seed with d(poses[p], poses[seed]) <= radius (a NaN distance
//     never), ascending; a pose counts once, under the first seed that reaches it.  The first `capacity` poses of that sequence are
//     emitted (cand, rows, state = 1); the rest are dropped (state stays 0) and counted.  A seed outside [0, N) is skipped, *status bit 1.
//   c2f_commit  similarity[b, cand[b, j]] = scores[b, j] for every cand >= 0: the scores' bits.
//
// The distance is f64: kind 0 theta(A, B) = acos(clamp((tr(A B^T) - 1) / 2, -1, 1)), kernels_modes.hip's; kind 1 the clamped acos of the
// cosine between the third ROWS P[2, :] (the camera's optical axis in the object frame), norms floored at 1e-8.
//
// Layout.  Thread t owns the poses n = t (mod 256); a sweep takes them chunk by chunk (n = chunk * 256 + t, coalesced).  The slot of a
// candidate is fixed by its place in the sequence alone: per chunk a block-wide exclusive scan of the membership flags -- the wave's ballot
// gives the lane prefix, the four wave counts go through LDS in wave order -- on top of the running count of the chunks and seeds before.
// No thread timing enters, no atomics but the integer OR into *status.  "Reached by an earlier seed" is a bit of the thread's OWN LDS
// words, kernels_modes.hip's alive-flag layout (s_taken[word * 256 + t]: no two threads share a word; 32 words per thread bound N at
// 256 * 32 * 32 = 262144, NOPE_ERR_UNSUPPORTED beyond): a dropped pose must not be counted again under a later seed, and state cannot
// say so.  Nothing is read by the host, there is no workspace, and every store is a plain vector store.
#include <cmath>

#include "nope_common.h"

namespace nope {

namespace {

constexpr int NT = 256;
constexpr int TAKEN_WORDS = 32;                      // per thread
constexpr int C2F_MAX_N = NT * 32 * TAKEN_WORDS;
constexpr int C2F_MAX_SEEDS = 16;

__device__ __forceinline__ double clamped_acos(double c) {      // a NaN stays a NaN
    return acos(c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c));
}

// d(A, S): A, S 3 x 3 row-major
__device__ __forceinline__ double c2f_distance(const double* A, const double* S, int kind) {
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

// the exclusive prefix of `flag` over the workgroup in thread order, and (total) the workgroup's count; every thread calls it
__device__ __forceinline__ int block_scan(bool flag, int& total) {
    __shared__ int s_wave[NT / 64];
    const unsigned long long m = __ballot(flag ? 1 : 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int before = __builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wave] = __builtin_popcountll(m);
    __syncthreads();
    total = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        if (w < wave) before += s_wave[w];
        total += s_wave[w];
    }
    __syncthreads();          // (the next scan writes the same words)
    return before;
}

__global__ __launch_bounds__(NT) void c2f_expand_kernel(const double* __restrict__ poses, long long stride_b, int N, const int* __restrict__ stage_of,
                                                        int max_stage, unsigned char* __restrict__ state, const long long* __restrict__ seeds,
                                                        int n_seeds, double radius, int kind, const unsigned* __restrict__ all_rel, int M,
                                                        int* __restrict__ cand, int* __restrict__ n_cand, int* __restrict__ n_dropped,
                                                        unsigned* __restrict__ rows, int* __restrict__ status) {
    __shared__ unsigned s_taken[TAKEN_WORDS * NT];
    const int b = blockIdx.x, t = threadIdx.x;
    const double* P = poses + (size_t)b * stride_b;
    unsigned char* st = state + (size_t)b * N;
    const unsigned* rel = all_rel + (size_t)b * N * 6;
    int* cb = cand + (size_t)b * M;
    unsigned* rb = rows + (size_t)b * M * 6;
    const int nchunks = (N + NT - 1) / NT, nwords = (nchunks + 31) >> 5;
    for (int w = 0; w < nwords; ++w) s_taken[w * NT + t] = 0u;      // (its own words: no barrier)

    // the seeds (every thread reads the same <= 16 values): the first valid one pads, one outside the grid is reported
    int pad = 0;
    bool have_pad = false, bad_seed = false;
    for (int j = 0; j < n_seeds; ++j) {
        const long long sd = seeds[(size_t)b * n_seeds + j];
        if (sd < 0 || sd >= N) bad_seed = true;
        else if (!have_pad) { pad = (int)sd; have_pad = true; }
    }

    int count = 0;            // the length of the candidate sequence so far, dropped ones included; the same in every thread
    const int passes = n_seeds == 0 ? 1 : n_seeds;
    for (int j = 0; j < passes; ++j) {
        long long sd = -1;
        double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (n_seeds > 0) {
            sd = seeds[(size_t)b * n_seeds + j];
            if (sd < 0 || sd >= N) continue;          // (uniform over the workgroup)
#pragma unroll
            for (int e = 0; e < 9; ++e) S[e] = P[(size_t)sd * 9 + e];
        }
        for (int c = 0; c < nchunks; ++c) {
            const int n = c * NT + t;
            const unsigned bit = 1u << (c & 31);
            bool flag = false;
            if (n < N && !(s_taken[(c >> 5) * NT + t] & bit) && stage_of[n] <= max_stage && st[n] == 0) {
                if (n_seeds == 0) flag = true;
                else if (n != sd) {
                    double A[9];
#pragma unroll
                    for (int e = 0; e < 9; ++e) A[e] = P[(size_t)n * 9 + e];
                    flag = c2f_distance(A, S, kind) <= radius;
                }
            }
            int total;
            const int slot = count + block_scan(flag, total);
            if (flag) {
                s_taken[(c >> 5) * NT + t] |= bit;
                if (slot < M) {
                    cb[slot] = n;
#pragma unroll
                    for (int e = 0; e < 6; ++e) rb[(size_t)slot * 6 + e] = rel[(size_t)n * 6 + e];
                    st[n] = 1;
                }
            }
            count += total;
        }
    }

    const int kept = count < M ? count : M;
    for (int sl = kept + t; sl < M; sl += NT) {
        cb[sl] = -1;
#pragma unroll
        for (int e = 0; e < 6; ++e) rb[(size_t)sl * 6 + e] = rel[(size_t)pad * 6 + e];
    }
    if (t == 0) {
        n_cand[b] = kept;
        n_dropped[b] = count - kept;
        const int bits = (count > kept ? 1 : 0) | (bad_seed ? 2 : 0);
        if (bits) atomicOr(status, bits);
    }
}

__global__ __launch_bounds__(NT) void c2f_commit_kernel(const unsigned* __restrict__ scores, const int* __restrict__ cand, int M, int N,
                                                        unsigned* __restrict__ sim, long long sim_ld) {
    const int b = blockIdx.x;
    for (int j = threadIdx.x; j < M; j += NT) {
        const int n = cand[(size_t)b * M + j];
        if (n >= 0 && n < N) sim[(size_t)b * sim_ld + n] = scores[(size_t)b * M + j];
    }
}

}  // namespace

int launch_c2f_expand(const double* poses, long long stride_b, int N, const int* stage_of, int max_stage, unsigned char* state,
                      const long long* seeds, int n_seeds, double radius_rad, int dist_kind, const float* all_rel, int capacity, int* cand,
                      int* n_cand, int* n_dropped, float* rows, int* status, int B, hipStream_t s) {
    if (!poses || !stage_of || !state || !all_rel || !cand || !n_cand || !n_dropped || !rows || !status) return NOPE_ERR_ARG;
    if (B <= 0 || N < 1 || capacity < 1 || stride_b < 0 || n_seeds < 0 || n_seeds > C2F_MAX_SEEDS) return NOPE_ERR_ARG;
    if (n_seeds > 0 && (!seeds || !(radius_rad >= 0.0))) return NOPE_ERR_ARG;
    if (dist_kind != 0 && dist_kind != 1) return NOPE_ERR_ARG;
    if (N > C2F_MAX_N) return NOPE_ERR_UNSUPPORTED;
    if (hipMemsetAsync(status, 0, sizeof(int), s) != hipSuccess) return NOPE_ERR_LAUNCH;
    hipLaunchKernelGGL(c2f_expand_kernel, dim3((unsigned)B), dim3(NT), 0, s, poses, stride_b, N, stage_of, max_stage, state, seeds, n_seeds,
                       radius_rad, dist_kind, (const unsigned*)all_rel, capacity, cand, n_cand, n_dropped, (unsigned*)rows, status);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_c2f_commit(const float* scores, const int* cand, int capacity, int N, float* sim, long long sim_ld, int B, hipStream_t s) {
    if (!scores || !cand || !sim || B <= 0 || N < 1 || capacity < 1 || sim_ld < N) return NOPE_ERR_ARG;
    hipLaunchKernelGGL(c2f_commit_kernel, dim3((unsigned)B), dim3(NT), 0, s, (const unsigned*)scores, cand, capacity, N, (unsigned*)sim, sim_ld);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

}  // namespace nope
