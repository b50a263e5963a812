// Translation from a rotation, the model and a 2D box, and its correction from a depth image (nope_amd/bop.py: estimate_translation,
// refine_translation_depth).  No reference counterpart: the reference predicts no translation (src/poses/vsd.py:84-87 takes the ground
// truth's).  The contracts are restated in include/nope_hip.h; DESIGN.md section 4.16.
//   fit_kernel          one workgroup per pose.  A pass walks the pose's vertices (lane l takes i = l, l + 256, ...), rotates each one again
//                       (f64 on the f32-stored vertex, no contraction) and keeps per-lane extremes; the extremes go through the butterfly
//                       and the waves, and every lane reads the same reduced values, so every branch of the iteration is uniform over the
//                       workgroup.  Pass 0 gives the extremes of R x (the initial guess), every later pass the projected box and min Z
//                       under the current t.  Only minima and maxima cross lanes (nan_min / nan_max keep a NaN): no order dependence.
//   mask_box_kernel     one workgroup per image: integer min / max of the non-zero pixels' x and y, and their count.
//   dshift_kernel       one workgroup per (block of pixels, estimate, image): inlier count and the f64 sum of test - est, per lane in pixel
//                       order, then the butterfly / wave order of vsd_kernel; one partial per workgroup.
//   dshift_final_kernel one lane per (image, estimate): partials in block order, the mean.
// No floating-point atomics: the same bits on every run.
#include <cmath>

#include "nope_common.h"

namespace nope {

namespace {

constexpr int kFitThreads = NOPE_FIT_THREADS;
constexpr int kFitWaves = kFitThreads / 64;
constexpr int kPixThreads = 256;

__device__ __forceinline__ bool is_nan(double a) { return a != a; }
// max / min that keep a NaN of either operand (fmax / fmin return the other operand)
__device__ __forceinline__ double nan_max(double a, double b) { return is_nan(a) ? a : ((b > a || is_nan(b)) ? b : a); }
__device__ __forceinline__ double nan_min(double a, double b) { return is_nan(a) ? a : ((b < a || is_nan(b)) ? b : a); }
__device__ __forceinline__ bool finite_all(const double* __restrict__ p, int n) {
    bool ok = true;
    for (int i = 0; i < n; ++i) ok = ok && (fabs(p[i]) <= 1.79769313486231570815e308);      // false for NaN and inf
    return ok;
}
// a range [off, off + cnt) that is non-empty, within [0, n) and no longer than the host's `max`
__device__ __forceinline__ bool range_ok(int off, int cnt, int n, int max) {
    return cnt > 0 && cnt <= max && off >= 0 && (long long)off + cnt <= (long long)n;
}

// three minima (m[0 .. 3)) and two maxima (m[3 .. 5)) over the workgroup; every lane returns with the reduced values
constexpr int kExt = 5, kExtMin = 3;
__device__ __forceinline__ void block_extremes(double* m, double (*red)[kExt]) {
#pragma unroll
    for (int q = 0; q < kExt; ++q) {
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const double o = __shfl_xor(m[q], s);
            m[q] = q < kExtMin ? nan_min(m[q], o) : nan_max(m[q], o);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                 // (red may still be read from the pass before)
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < kExt; ++q) red[wave][q] = m[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kExt; ++q) {
        double r = red[0][q];
#pragma unroll
        for (int w = 1; w < kFitWaves; ++w) r = q < kExtMin ? nan_min(r, red[w][q]) : nan_max(r, red[w][q]);
        m[q] = r;
    }
}

__global__ __launch_bounds__(kFitThreads) void fit_kernel(const float* __restrict__ verts, int V, const int* __restrict__ vert_off,
                                                          const int* __restrict__ vert_cnt, int max_verts, const double* __restrict__ Rs,
                                                          const double* __restrict__ Ks, const double* __restrict__ boxes, int max_iters,
                                                          double tol_scale, double tol_px, double* __restrict__ t_out,
                                                          double* __restrict__ residual, int* __restrict__ iters, int* __restrict__ status) {
#pragma clang fp contract(off)
    __shared__ double red[kFitWaves][kExt];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int off = vert_off[p], cnt = vert_cnt[p];
    const double* Rp = Rs + (size_t)p * 9;
    const double* Kp = Ks + (size_t)p * 9;
    const double* bx = boxes + (size_t)p * 4;
    double r[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) r[q] = Rp[q];
    const double fx = Kp[0], cx = Kp[2], fy = Kp[4], cy = Kp[5];
    const double u0 = bx[0], v0 = bx[1], u1 = bx[2], v1 = bx[3];
    const double bw = u1 - u0, bh = v1 - v0, cu = 0.5 * (u0 + u1), cv = 0.5 * (v0 + v1);
    // ---- edge rules (every lane evaluates the same values: uniform) ----
    int st = 0;
    const bool box_finite = finite_all(bx, 4);
    if (!finite_all(Rp, 9) || !finite_all(Kp, 9) || !box_finite) st |= NOPE_FIT_NONFINITE;
    if (box_finite && (!(bw > 0.0) || !(bh > 0.0))) st |= NOPE_FIT_BAD_BOX;
    if (!range_ok(off, cnt, V, max_verts)) st |= NOPE_FIT_VERT_RANGE;
    double tx = NAN, ty = NAN, tz = NAN, res = NAN;
    int n = 0;
    if (st == 0) {
        const float* vp = verts + 3 * (size_t)off;
        // ---- pass 0: the extremes of y = R x, the initial guess ----
        double m[kExt] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY};      // min y.x, min y.y, (unused) | max y.x, max y.y
        for (int i = tid; i < cnt; i += kFitThreads) {
            const double x = vp[3 * (size_t)i], y = vp[3 * (size_t)i + 1], z = vp[3 * (size_t)i + 2];
            const double yx = r[0] * x + r[1] * y + r[2] * z;
            const double yy = r[3] * x + r[4] * y + r[5] * z;
            m[0] = nan_min(m[0], yx); m[1] = nan_min(m[1], yy);
            m[3] = nan_max(m[3], yx); m[4] = nan_max(m[4], yy);
        }
        block_extremes(m, red);
        {
            const double ax0 = m[0], ay0 = m[1], ax1 = m[3], ay1 = m[4];
            tz = 0.5 * ((fx * (ax1 - ax0)) / bw + (fy * (ay1 - ay0)) / bh);
            tx = ((cu - cx) / fx) * tz - 0.5 * (ax0 + ax1);
            ty = ((cv - cy) / fy) * tz - 0.5 * (ay0 + ay1);
        }
        // ---- the iteration: every condition below is on block-reduced values ----
        for (;;) {
            m[0] = INFINITY; m[1] = INFINITY; m[2] = INFINITY; m[3] = -INFINITY; m[4] = -INFINITY;      // min Z, pu0, pv0 | pu1, pv1
            for (int i = tid; i < cnt; i += kFitThreads) {
                const double x = vp[3 * (size_t)i], y = vp[3 * (size_t)i + 1], z = vp[3 * (size_t)i + 2];
                const double yx = r[0] * x + r[1] * y + r[2] * z;
                const double yy = r[3] * x + r[4] * y + r[5] * z;
                const double yz = r[6] * x + r[7] * y + r[8] * z;
                const double Z = yz + tz;
                const double u = fx * ((yx + tx) / Z) + cx;
                const double v = fy * ((yy + ty) / Z) + cy;
                m[0] = nan_min(m[0], Z);
                m[1] = nan_min(m[1], u); m[2] = nan_min(m[2], v);
                m[3] = nan_max(m[3], u); m[4] = nan_max(m[4], v);
            }
            block_extremes(m, red);
            if (!(m[0] > 0.0)) {
                st |= NOPE_FIT_BEHIND;
                tx = NAN; ty = NAN; tz = NAN; res = NAN;
                break;
            }
            const double pu0 = m[1], pv0 = m[2], pu1 = m[3], pv1 = m[4];
            const double s = 0.5 * ((pu1 - pu0) / bw + (pv1 - pv0) / bh);
            const double du = cu - 0.5 * (pu0 + pu1), dv = cv - 0.5 * (pv0 + pv1);
            res = nan_max(nan_max(nan_max(fabs(pu0 - u0), fabs(pu1 - u1)), fabs(pv0 - v0)), fabs(pv1 - v1));
            if (fabs(s - 1.0) <= tol_scale && fabs(du) <= tol_px && fabs(dv) <= tol_px) break;
            if (n == max_iters) { st |= NOPE_FIT_NOT_CONVERGED; break; }
            const double zn = tz * s;
            tx = tx * s + (du * zn) / fx;
            ty = ty * s + (dv * zn) / fy;
            tz = zn;
            ++n;
        }
    }
    if (tid == 0) {
        t_out[(size_t)p * 3] = tx; t_out[(size_t)p * 3 + 1] = ty; t_out[(size_t)p * 3 + 2] = tz;
        residual[p] = res;
        iters[p] = n;
        status[p] = st;
    }
}

// ---- mask boxes ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPixThreads) void mask_box_kernel(const unsigned char* __restrict__ mask, int H, int W, double* __restrict__ box,
                                                               int* __restrict__ count) {
    __shared__ int red[kPixThreads / 64][5];
    const int b = blockIdx.x, tid = threadIdx.x;
    const unsigned HW = (unsigned)H * (unsigned)W;          // (H W <= 2^30: 32-bit index arithmetic)
    const unsigned char* mp = mask + (size_t)b * HW;
    int x0 = W, y0 = H, x1 = -1, y1 = -1, c = 0;
    for (unsigned i = tid; i < HW; i += kPixThreads) {
        if (mp[i] == 0) continue;
        const int y = (int)(i / (unsigned)W), x = (int)(i - (unsigned)y * (unsigned)W);
        x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1;
        y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
        ++c;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const int a0 = __shfl_xor(x0, s), a1 = __shfl_xor(y0, s), a2 = __shfl_xor(x1, s), a3 = __shfl_xor(y1, s);
        x0 = a0 < x0 ? a0 : x0; y0 = a1 < y0 ? a1 : y0;
        x1 = a2 > x1 ? a2 : x1; y1 = a3 > y1 ? a3 : y1;
        c += __shfl_xor(c, s);
    }
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) { red[wave][0] = x0; red[wave][1] = y0; red[wave][2] = x1; red[wave][3] = y1; red[wave][4] = c; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kPixThreads / 64; ++w) {
            x0 = red[w][0] < x0 ? red[w][0] : x0; y0 = red[w][1] < y0 ? red[w][1] : y0;
            x1 = red[w][2] > x1 ? red[w][2] : x1; y1 = red[w][3] > y1 ? red[w][3] : y1;
            c += red[w][4];
        }
        double* o = box + (size_t)b * 4;
        if (c == 0) { o[0] = NAN; o[1] = NAN; o[2] = NAN; o[3] = NAN; }
        else { o[0] = (double)x0; o[1] = (double)y0; o[2] = (double)(x1 + 1); o[3] = (double)(y1 + 1); }
        count[b] = c;
    }
}

// ---- depth shift ---------------------------------------------------------------------------------------------------------------------
// part: (B, k, nblk, 2) f64: the sum and the inlier count (an integer below 2^30, exact) of each workgroup
__global__ __launch_bounds__(kPixThreads) void dshift_kernel(const float* __restrict__ dtest, const float* __restrict__ dest,
                                                             const unsigned char* __restrict__ mask, int k, int H, int W, int nblk, double tau,
                                                             double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double red[kPixThreads / 64][2];
    const int blk = blockIdx.x, j = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const size_t HW = (size_t)H * W;
    const float* T = dtest + (size_t)b * HW;
    const float* E = dest + ((size_t)b * k + j) * HW;
    const unsigned char* M = mask ? mask + (size_t)b * HW : nullptr;
    double sum = 0.0;
    int cnt = 0;
    for (size_t i = (size_t)blk * kPixThreads + tid; i < HW; i += (size_t)nblk * kPixThreads) {
        const float t = T[i], e = E[i];
        const double d = (double)t - (double)e;
        if (t > 0.0f && e > 0.0f && (!M || M[i] != 0) && fabs(d) <= tau) { sum += d; ++cnt; }
    }
    double c = (double)cnt;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        sum += __shfl_xor(sum, m);
        c += __shfl_xor(c, m);
    }
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) { red[wave][0] = sum; red[wave][1] = c; }
    __syncthreads();
    if (tid == 0) {
        double* o = part + (((size_t)b * k + j) * nblk + blk) * 2;
        o[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        o[1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    }
    static_assert(kPixThreads == 256, "the line above folds four waves");
}

__global__ __launch_bounds__(256) void dshift_final_kernel(const double* __restrict__ part, int n, int nblk, double* __restrict__ shift,
                                                           int* __restrict__ count) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    double sum = 0.0, c = 0.0;
    for (int blk = 0; blk < nblk; ++blk) {
        const double* o = part + ((size_t)t * nblk + blk) * 2;
        sum += o[0]; c += o[1];
    }
    shift[t] = c == 0.0 ? NAN : sum / c;
    count[t] = (int)c;
}

int dshift_blocks_per_image(int H, int W) {
    const size_t HW = (size_t)H * W, per_block = (size_t)kPixThreads * 4;      // ~4 pixels per lane
    const size_t n = (HW + per_block - 1) / per_block;
    return (int)(n < 1 ? 1 : (n > 1024 ? 1024 : n));
}

}  // namespace

int launch_fit_translation(const float* verts, int V, const int* vert_off, const int* vert_cnt, int max_verts, const double* R, const double* K,
                           const double* box, int P, int max_iters, double tol_scale, double tol_px, double* t, double* residual, int* iters,
                           int* status, hipStream_t s) {
    if (!verts || !vert_off || !vert_cnt || !R || !K || !box || !t || !residual || !iters || !status) return NOPE_ERR_ARG;
    if (V <= 0 || P <= 0 || max_verts <= 0 || max_iters < 0 || !(tol_scale >= 0.0) || !(tol_px >= 0.0)) return NOPE_ERR_ARG;
    hipLaunchKernelGGL(fit_kernel, dim3((unsigned)P), dim3(kFitThreads), 0, s, verts, V, vert_off, vert_cnt, max_verts, R, K, box, max_iters,
                       tol_scale, tol_px, t, residual, iters, status);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_mask_boxes(const unsigned char* mask, int B, int H, int W, double* box, int* count, hipStream_t s) {
    if (!mask || !box || !count) return NOPE_ERR_ARG;
    if (B <= 0 || H <= 0 || W <= 0 || (long long)H * W > (1ll << 30)) return NOPE_ERR_ARG;
    hipLaunchKernelGGL(mask_box_kernel, dim3((unsigned)B), dim3(kPixThreads), 0, s, mask, H, W, box, count);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

size_t depth_shift_workspace_bytes(int B, int k, int H, int W) {
    if (B <= 0 || k <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * k * dshift_blocks_per_image(H, W) * 2 * sizeof(double);
}

int launch_depth_shift(const float* dtest, const float* dest, const unsigned char* mask, int B, int k, int H, int W, double tau, double* shift,
                       int* count, void* ws, size_t ws_bytes, hipStream_t s) {
    if (!dtest || !dest || !shift || !count || !ws) return NOPE_ERR_ARG;
    if (B <= 0 || B > 65535 || k <= 0 || k > 16 || H <= 0 || W <= 0 || (long long)H * W > (1ll << 30) || !(tau >= 0.0)) return NOPE_ERR_ARG;
    if (ws_bytes < depth_shift_workspace_bytes(B, k, H, W)) return NOPE_ERR_WORKSPACE;
    const int nblk = dshift_blocks_per_image(H, W);
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(dshift_kernel, dim3((unsigned)nblk, (unsigned)k, (unsigned)B), dim3(kPixThreads), 0, s, dtest, dest, mask, k, H, W, nblk, tau,
                       part);
    NOPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(dshift_final_kernel, dim3((unsigned)cdiv(B * k, 256)), dim3(256), 0, s, part, B * k, nblk, shift, count);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

}  // namespace nope
