// Sub-grid pose refinement: Gauss-Newton on SO(3) through the U-Net (no reference counterpart: the
// reference's answer is template_poses[nearest_idx], src/model/model.py:352-354, a vertex of the template grid).
//
// A candidate (b, j) carries a relative rotation dR, 3x3 row-major f64.  It starts at the Gram-Schmidt matrix of the 6-D row
// all_relativeR[b, nearest_idx[b, j]] (first two matrix rows, src/poses/rotation_conversions.py:490-503 and its inverse) and
// moves by left-multiplied tangent steps dR <- exp(w) dR.  Per iteration the caller runs the U-Net on the seven poses
//   [dR, exp(+h e_x) dR, exp(-h e_x) dR, exp(+h e_y) dR, exp(-h e_y) dR, exp(+h e_z) dR, exp(-h e_z) dR]
// (written here as 6-D f32 rows) and hands the seven maps back:
//   r = t0 - q,   J_a = (t_{+a} - t_{-a}) / 2h,   A = J^T J,   g = J^T r,   cost = r^T r           refine_normal_eq
//   (A + damping diag A) w = -g,  |w| clamped,  dR <- GramSchmidt(exp(w) dR)                        refine_step
// and after the last iteration compares the reference's score of the refined pose with the retrieval score
//   accept iff score_refined > score_grid (NaN never), order by final score                          refine_select
//
// The four 3x3 kernels run one thread per candidate (or per sample) in f64: a few dozen operations.  The normal equations stream
// 8 C h w f32 values per candidate (256 KB at the shipped size: launch-latency territory), as sim_reg_kernel does -- lane i owns
// pixel vector i (16 bytes) of every channel plane, the loads of a plane are coalesced 16-byte loads -- with differences,
// products and sums in f64, so the result does not depend on the summation order beyond ~1e-12 of its terms.  Reductions have a
// fixed shape (wave xor-tree, ordered LDS fold, ordered fold of the pixel slices): run-to-run deterministic.
#include <cmath>

#include "nope_common.h"

namespace nope {

namespace {

constexpr int NT = 256;
constexpr int SLICE_PIX = NT * 4;      // pixels of one workgroup: one 16-byte vector per lane and channel plane

// ---- 3x3 f64 helpers (row-major) ----------------------------------------------------------------------------------------
// rotation_6d_to_matrix: b1 = a1 / |a1|, b2 = (a2 - (b1 . a2) b1) / |.|, b3 = b1 x b2 (F.normalize's eps = 1e-12 on the norms)
__device__ __forceinline__ void gram_schmidt(const double* a, double* R) {
    double n1 = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    n1 = n1 > 1e-12 ? n1 : 1e-12;
    const double b1[3] = {a[0] / n1, a[1] / n1, a[2] / n1};
    const double d = b1[0] * a[3] + b1[1] * a[4] + b1[2] * a[5];
    double b2[3] = {a[3] - d * b1[0], a[4] - d * b1[1], a[5] - d * b1[2]};
    double n2 = sqrt(b2[0] * b2[0] + b2[1] * b2[1] + b2[2] * b2[2]);
    n2 = n2 > 1e-12 ? n2 : 1e-12;
    b2[0] /= n2; b2[1] /= n2; b2[2] /= n2;
    R[0] = b1[0]; R[1] = b1[1]; R[2] = b1[2];
    R[3] = b2[0]; R[4] = b2[1]; R[5] = b2[2];
    R[6] = b1[1] * b2[2] - b1[2] * b2[1];
    R[7] = b1[2] * b2[0] - b1[0] * b2[2];
    R[8] = b1[0] * b2[1] - b1[1] * b2[0];
}

// exp of the skew matrix W of w (Rodrigues): I + (sin t / t) W + ((1 - cos t) / t^2) W^2, t = |w|; the series below 1e-6
__device__ __forceinline__ void so3_exp(const double* w, double* E) {
    const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const double t = sqrt(t2);
    double a, b;
    if (t < 1e-6) { a = 1.0 - t2 / 6.0; b = 0.5 - t2 / 24.0; }
    else { a = sin(t) / t; b = (1.0 - cos(t)) / t2; }
    const double x = w[0], y = w[1], z = w[2];
    E[0] = 1.0 - b * (y * y + z * z); E[1] = -a * z + b * x * y;        E[2] = a * y + b * x * z;
    E[3] = a * z + b * x * y;         E[4] = 1.0 - b * (x * x + z * z); E[5] = -a * x + b * y * z;
    E[6] = -a * y + b * x * z;        E[7] = a * x + b * y * z;         E[8] = 1.0 - b * (x * x + y * y);
}

__device__ __forceinline__ void mat3_mul(const double* X, const double* Y, double* Z) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Z[3 * i + j] = X[3 * i] * Y[j] + X[3 * i + 1] * Y[3 + j] + X[3 * i + 2] * Y[6 + j];
}

// the seven poses of a candidate as 6-D f32 rows: row 0 = dR, rows 1 + 2a / 2 + 2a = exp(+h e_a) dR / exp(-h e_a) dR
__device__ __forceinline__ void emit_poses(const double* R, double h, float* __restrict__ out) {
#pragma unroll
    for (int e = 0; e < 6; ++e) out[e] = (float)R[e];
    for (int m = 0; m < 6; ++m) {
        double w[3] = {0.0, 0.0, 0.0};
        w[m >> 1] = (m & 1) ? -h : h;
        double E[9], P[9];
        so3_exp(w, E);
        mat3_mul(E, R, P);
#pragma unroll
        for (int e = 0; e < 6; ++e) out[(size_t)(m + 1) * 6 + e] = (float)P[e];
    }
}

__global__ __launch_bounds__(NT) void refine_init_kernel(const float* __restrict__ all_rel, long long N, const long long* __restrict__ idx,
                                                         double* __restrict__ dR, double* __restrict__ dR0, float* __restrict__ poses,
                                                         int* __restrict__ status, int B, int k, double h) {
    const int t = blockIdx.x * NT + threadIdx.x;
    if (t >= B * k) return;
    const int b = t / k;
    long long n = idx[t];
    int st = 0;
    if (n < 0 || n >= N) { st = NOPE_REFINE_BAD_INDEX; n = n < 0 ? 0 : N - 1; }      // (clamped: a bad index never reads out of bounds)
    double a[6], R[9];
#pragma unroll
    for (int e = 0; e < 6; ++e) a[e] = (double)all_rel[((size_t)b * N + (size_t)n) * 6 + e];
    gram_schmidt(a, R);
#pragma unroll
    for (int e = 0; e < 9; ++e) { dR[(size_t)t * 9 + e] = R[e]; dR0[(size_t)t * 9 + e] = R[e]; }
    emit_poses(R, h, poses + (size_t)t * 42);
    status[t] = st;
}

// ---- normal equations ----------------------------------------------------------------------------------------------------
// sums[0..5] = sum d_a d_b for (a, b) = (0,0) (0,1) (0,2) (1,1) (1,2) (2,2), sums[6..8] = sum d_a r, sums[9] = sum r r, with
// d_a = t_{+a} - t_{-a} and r = t0 - q in f64 (differences of f32 values: exact up to one rounding); the 1 / 2h factors are
// applied once, by the fold.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(NT) void refine_partial_kernel(const float* __restrict__ q, const float* __restrict__ maps, double* __restrict__ partial,
                                                            int k, int C, int HW, int nslice) {
    __shared__ double s_part[NT / 64][10];
    const int cand = blockIdx.x / nslice, slice = blockIdx.x - cand * nslice;
    const int b = cand / k;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pix = slice * SLICE_PIX + tid * 4;
    double acc[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) acc[i] = 0.0;
    if (pix < HW) {              // (HW % 4 == 0: a lane's four pixels are inside the plane or all outside)
        const float* qp = q + (size_t)b * C * HW + pix;
        const float* mp = maps + (size_t)cand * 7 * C * HW + pix;
        const size_t map_elems = (size_t)C * HW;
        for (int c = 0; c < C; ++c) {
            const f32x4 qv = *reinterpret_cast<const f32x4*>(qp + (size_t)c * HW);
            f32x4 tv[7];
#pragma unroll
            for (int m = 0; m < 7; ++m) tv[m] = *reinterpret_cast<const f32x4*>(mp + (size_t)m * map_elems + (size_t)c * HW);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double r = (double)tv[0][e] - (double)qv[e];
                const double d0 = (double)tv[1][e] - (double)tv[2][e];
                const double d1 = (double)tv[3][e] - (double)tv[4][e];
                const double d2 = (double)tv[5][e] - (double)tv[6][e];
                acc[0] += d0 * d0; acc[1] += d0 * d1; acc[2] += d0 * d2;
                acc[3] += d1 * d1; acc[4] += d1 * d2; acc[5] += d2 * d2;
                acc[6] += d0 * r;  acc[7] += d1 * r;  acc[8] += d2 * r;
                acc[9] += r * r;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const double s = wave_sum_f64(acc[i]);
        if (lane == 0) s_part[wave][i] = s;
    }
    __syncthreads();
    if (tid < 10) {
        double tot = 0.0;
        for (int w = 0; w < NT / 64; ++w) tot += s_part[w][tid];
        partial[(size_t)blockIdx.x * 10 + tid] = tot;
    }
}

__global__ __launch_bounds__(NT) void refine_fold_kernel(const double* __restrict__ partial, double* __restrict__ ne, int n_cand, int nslice, double h) {
    const int t = blockIdx.x * NT + threadIdx.x;
    if (t >= n_cand * 10) return;
    const int cand = t / 10, i = t - cand * 10;
    double tot = 0.0;
    for (int s = 0; s < nslice; ++s) tot += partial[((size_t)cand * nslice + s) * 10 + i];
    const double inv = 1.0 / (2.0 * h);
    ne[t] = i < 6 ? tot * (inv * inv) : i < 9 ? tot * inv : tot;
}

// ---- the step ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void refine_step_kernel(const double* __restrict__ ne, double* __restrict__ dR, float* __restrict__ poses,
                                                         int* __restrict__ status, int n_cand, double h, double max_step, double damping) {
    const int t = blockIdx.x * NT + threadIdx.x;
    if (t >= n_cand) return;
    double v[10], R[9];
#pragma unroll
    for (int i = 0; i < 10; ++i) v[i] = ne[(size_t)t * 10 + i];
#pragma unroll
    for (int e = 0; e < 9; ++e) R[e] = dR[(size_t)t * 9 + e];
    int st = 0;
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 10; ++i) finite = finite && __builtin_isfinite(v[i]);
    if (!finite) st = NOPE_REFINE_NONFINITE;
    double w[3] = {0.0, 0.0, 0.0};
    if (st == 0) {
        // M = A + damping diag A (symmetric); w = -M^-1 g by the adjugate
        const double m00 = v[0] + damping * v[0], m11 = v[3] + damping * v[3], m22 = v[5] + damping * v[5];
        const double m01 = v[1], m02 = v[2], m12 = v[4];
        const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
        const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
        const double det = m00 * c00 + m01 * c01 + m02 * c02;
        if (!(det > 0.0)) {
            st = NOPE_REFINE_SINGULAR;
        } else {
            w[0] = -(c00 * v[6] + c01 * v[7] + c02 * v[8]) / det;
            w[1] = -(c01 * v[6] + c11 * v[7] + c12 * v[8]) / det;
            w[2] = -(c02 * v[6] + c12 * v[7] + c22 * v[8]) / det;
            const double n = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
            if (!__builtin_isfinite(n)) st = NOPE_REFINE_NONFINITE;
            else if (n == 0.0) st = NOPE_REFINE_ZERO_STEP;
            else if (n > max_step) {
                const double sc = max_step / n;
                w[0] *= sc; w[1] *= sc; w[2] *= sc;
                st = NOPE_REFINE_CLAMPED;
            }
        }
    }
    if (st == 0 || st == NOPE_REFINE_CLAMPED) {      // every other status: no step, dR stays as it is, bit for bit
        double E[9], P[9];
        so3_exp(w, E);
        mat3_mul(E, R, P);
        gram_schmidt(P, R);
#pragma unroll
        for (int e = 0; e < 9; ++e) dR[(size_t)t * 9 + e] = R[e];
    }
    emit_poses(R, h, poses + (size_t)t * 42);
    status[t] = st;
}

// ---- accept / revert, order, predicted pose -------------------------------------------------------------------------------
constexpr int KMAX = 16;

__global__ __launch_bounds__(NT) void refine_select_kernel(const double* __restrict__ dR, const double* __restrict__ dR0, const float* __restrict__ score_new,
                                                           const float* __restrict__ sim, long long sim_ld, long long N, const long long* __restrict__ idx,
                                                           const double* __restrict__ tpl, long long tpl_stride_b, long long n_tpl,
                                                           double* __restrict__ out_R, float* __restrict__ out_6d, float* __restrict__ out_score,
                                                           float* __restrict__ out_score0, int* __restrict__ out_accepted, long long* __restrict__ out_order,
                                                           double* __restrict__ pred_R, int B, int k) {
    const int b = blockIdx.x * NT + threadIdx.x;
    if (b >= B) return;
    const float INF = __builtin_huge_valf();
    float fin[KMAX], old[KMAX];
    bool acc[KMAX];
    int ord[KMAX];
    for (int j = 0; j < k; ++j) {
        long long n = idx[(size_t)b * k + j];
        n = n < 0 ? 0 : n >= N ? N - 1 : n;
        old[j] = sim[(size_t)b * sim_ld + n];
        const float s = score_new[(size_t)b * k + j];
        acc[j] = s > old[j];                 // strictly better; false for a NaN on either side
        fin[j] = acc[j] ? s : old[j];
    }
    // descending final score, ties -> the lower retrieval rank (a stable insertion); a NaN ranks highest, as in nope_topk
    for (int j = 0; j < k; ++j) {
        const float kj = fin[j] != fin[j] ? INF : fin[j];
        int p = j;
        while (p > 0) {
            const int o = ord[p - 1];
            const float ko = fin[o] != fin[o] ? INF : fin[o];
            if (!(kj > ko)) break;
            ord[p] = o;
            --p;
        }
        ord[p] = j;
    }
    for (int r = 0; r < k; ++r) {
        const int j = ord[r];
        const size_t src = (size_t)b * k + j, dst = (size_t)b * k + r;
        const double* R = (acc[j] ? dR : dR0) + src * 9;
#pragma unroll
        for (int e = 0; e < 9; ++e) out_R[dst * 9 + e] = R[e];
#pragma unroll
        for (int e = 0; e < 6; ++e) out_6d[dst * 6 + e] = (float)R[e];
        out_score[dst] = fin[j];
        out_score0[dst] = old[j];
        out_accepted[dst] = acc[j] ? 1 : 0;
        out_order[dst] = j;
        if (pred_R) {
            long long n = idx[src];
            n = n < 0 ? 0 : n >= n_tpl ? n_tpl - 1 : n;
            const double* T = tpl + (size_t)b * tpl_stride_b + (size_t)n * 9;
            if (!acc[j]) {                   // reverted: the grid pose itself
#pragma unroll
                for (int e = 0; e < 9; ++e) pred_R[dst * 9 + e] = T[e];
            } else {                         // (dR dR0^T) T
                const double* R0 = dR0 + src * 9;
                double D[9], Tl[9], P[9];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c) D[3 * i + c] = R[3 * i] * R0[3 * c] + R[3 * i + 1] * R0[3 * c + 1] + R[3 * i + 2] * R0[3 * c + 2];
#pragma unroll
                for (int e = 0; e < 9; ++e) Tl[e] = T[e];
                mat3_mul(D, Tl, P);
#pragma unroll
                for (int e = 0; e < 9; ++e) pred_R[dst * 9 + e] = P[e];
            }
        }
    }
}

}  // namespace

int launch_refine_init(const float* all_rel, long long N, const long long* idx, double* dR, double* dR0, float* poses, int* status, int B, int k,
                       double h, hipStream_t s) {
    if (!all_rel || !idx || !dR || !dR0 || !poses || !status || B <= 0 || k <= 0 || N <= 0 || !(h > 0.0)) return NOPE_ERR_ARG;
    hipLaunchKernelGGL(refine_init_kernel, dim3((unsigned)cdiv(B * k, NT)), dim3(NT), 0, s, all_rel, N, idx, dR, dR0, poses, status, B, k, h);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

size_t refine_normal_eq_workspace_bytes(int B, int k, int HW) {
    if (B <= 0 || k <= 0 || HW <= 0) return 0;
    return (size_t)B * k * cdiv(HW, SLICE_PIX) * 10 * sizeof(double);
}

int launch_refine_normal_eq(const float* q, const float* maps, double* ne, int B, int k, int C, int HW, double h, void* ws, size_t ws_bytes,
                            hipStream_t s) {
    if (!q || !maps || !ne || !ws || B <= 0 || k <= 0 || C <= 0 || HW <= 0 || !(h > 0.0)) return NOPE_ERR_ARG;
    if (HW % 16) return NOPE_ERR_UNSUPPORTED;
    if (ws_bytes < refine_normal_eq_workspace_bytes(B, k, HW)) return NOPE_ERR_WORKSPACE;
    const int nslice = cdiv(HW, SLICE_PIX);
    if ((long long)B * k * nslice > 0x7fffffffLL / 10) return NOPE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(refine_partial_kernel, dim3((unsigned)(B * k * nslice)), dim3(NT), 0, s, q, maps, (double*)ws, k, C, HW, nslice);
    NOPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(refine_fold_kernel, dim3((unsigned)cdiv(B * k * 10, NT)), dim3(NT), 0, s, (const double*)ws, ne, B * k, nslice, h);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_refine_step(const double* ne, double* dR, float* poses, int* status, int B, int k, double h, double max_step_rad, double damping,
                       hipStream_t s) {
    if (!ne || !dR || !poses || !status || B <= 0 || k <= 0 || !(h > 0.0) || !(max_step_rad > 0.0) || !(damping >= 0.0)) return NOPE_ERR_ARG;
    hipLaunchKernelGGL(refine_step_kernel, dim3((unsigned)cdiv(B * k, NT)), dim3(NT), 0, s, ne, dR, poses, status, B * k, h, max_step_rad, damping);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_refine_select(const double* dR, const double* dR0, const float* score_new, const float* sim, long long sim_ld, long long N,
                         const long long* idx, const double* tpl, long long tpl_stride_b, long long n_tpl, double* out_R, float* out_6d,
                         float* out_score, float* out_score0, int* out_accepted, long long* out_order, double* pred_R, int B, int k, hipStream_t s) {
    if (!dR || !dR0 || !score_new || !sim || !idx || !out_R || !out_6d || !out_score || !out_score0 || !out_accepted || !out_order) return NOPE_ERR_ARG;
    if (B <= 0 || k <= 0 || k > KMAX || N <= 0 || sim_ld < N || (pred_R != nullptr) != (tpl != nullptr)) return NOPE_ERR_ARG;
    if (tpl && (n_tpl <= 0 || tpl_stride_b < 0)) return NOPE_ERR_ARG;
    hipLaunchKernelGGL(refine_select_kernel, dim3((unsigned)cdiv(B, NT)), dim3(NT), 0, s, dR, dR0, score_new, sim, sim_ld, N, idx, tpl, tpl_stride_b,
                       n_tpl, out_R, out_6d, out_score, out_score0, out_accepted, out_order, pred_R, B, k);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

}  // namespace nope
