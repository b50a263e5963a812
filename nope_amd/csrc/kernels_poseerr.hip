// BOP pose errors on the device (nope_amd/bop.py): MSSD, MSPD, ADD, ADI (ADD-S) of P pose pairs, and mesh diameters.  No reference
// counterpart: the reference reads models_info.json (dataloader/baseBOP.py:284) and evaluates VSD alone; the definitions are those of
// the BOP toolkit's pose_error.py (mssd, mspd, add, adi), restated in include/nope_hip.h.
//
// A pose pair is an estimate and a ground truth (4x4 f64 object-to-camera, OpenCV axes, mm), K (3x3 f64), a range of the shared f32
// vertex buffer and a range of the shared (S_total, 4, 4) f64 symmetry buffer.  All arithmetic is f64 on the f32-stored vertices,
// without contraction: Xe_i = Re x_i + te, Xg_i^s = Rg (Rs x_i + ts) + tg, every 3-term dot product summed left to right.
//   pe_point_kernel<ADD, ADI>  one workgroup per (pose, block of kPtBlock vertices), kPts points per lane in registers.
//                      ADD: |Xe_i - (Rg x_i + tg)| per point.
//                      ADI: y_i = Rg^T (Xe_i - tg), the estimate's point in the ground truth's object frame; the object's vertices
//                      stream through an LDS tile of kTile vertices (f64, one array per coordinate: every lane reads the same
//                      vertex, so the reads are broadcasts and the 8-byte stores of the fill are conflict-free); each point keeps the
//                      running minimum of the squared distance and takes sqrt once.
//                      Both sums: per lane in point order, then the butterfly / wave order of vsd_kernel; one partial per
//                      (pose, block) goes to the workspace.
//   pe_sym_kernel      one workgroup per (pose, chunk of kSymChunk symmetries) walks the object's vertices once: per symmetry the
//                      maximum squared distance |Xe_i - Xg_i^s|^2 (MSSD) and the maximum squared pixel distance
//                      |pi(Xe_i) - pi(Xg_i^s)|^2 (MSPD), pi(X) = (K X)_{0,1} / (K X)_2 with the whole K.  The maxima keep a NaN
//                      (nan_max below; fmax would drop it).  A vertex at (K X)_2 <= 0 under either pose raises the chunk's flag.
//   pe_fold_kernel     one lane per pose: range and finiteness checks, partial sums in block order -> means, min over the symmetries
//                      of the per-symmetry maxima (nan_min), sqrt, status bits.  A pose whose ranges are bad reads no partial.
//   diam_kernel        the ADI tiling with a maximum: a block of points against every tile that is not wholly below it (the pair
//                      (i, j) and (j, i) give the same distance, so tiles that end before the block begins are skipped)
//   diam_fold_kernel   max over an object's blocks in block order, sqrt
// sqrt is monotone and correctly rounded, so sqrt(max d^2) = max sqrt(d^2) and sqrt(min d^2) = min sqrt(d^2) bit for bit.
// No floating-point atomics: the same bits on every run.
#include <cmath>

#include "nope_common.h"

namespace nope {

namespace {

constexpr int kPeThreads = 128;                  // pe_point_kernel, diam_kernel
constexpr int kPts = 4;                          // points per lane
constexpr int kPtBlock = kPeThreads * kPts;      // 512 points per workgroup
constexpr int kTile = NOPE_POSE_ERR_TILE;        // 1024 vertices per LDS tile (3 x 8 KiB)
constexpr int kSymThreads = 256;
constexpr int kSymChunk = NOPE_POSE_ERR_SYM_CHUNK;      // 8 symmetries per workgroup
static_assert(kPtBlock == NOPE_POSE_ERR_POINT_BLOCK, "include/nope_hip.h names the point block");

__device__ __forceinline__ bool is_nan(double a) { return a != a; }
// max / min that keep a NaN of either operand (fmax / fmin return the other operand)
__device__ __forceinline__ double nan_max(double a, double b) { return is_nan(a) ? a : ((b > a || is_nan(b)) ? b : a); }
__device__ __forceinline__ double nan_min(double a, double b) { return is_nan(a) ? a : ((b < a || is_nan(b)) ? b : a); }
__device__ __forceinline__ bool finite_all(const double* __restrict__ p, int n) {
    bool ok = true;
    for (int i = 0; i < n; ++i) ok = ok && (fabs(p[i]) <= 1.79769313486231570815e308);      // false for NaN and inf
    return ok;
}

// rows 0..2 of a 4x4 row-major transform applied to a point: (m0 x + m1 y) + m2 z + m3, no contraction
struct P3 { double x, y, z; };
__device__ __forceinline__ P3 xform(const double* __restrict__ T, double x, double y, double z) {
#pragma clang fp contract(off)
    P3 r;
    r.x = T[0] * x + T[1] * y + T[2] * z + T[3];
    r.y = T[4] * x + T[5] * y + T[6] * z + T[7];
    r.z = T[8] * x + T[9] * y + T[10] * z + T[11];
    return r;
}

// a range [off, off + cnt) that is non-empty, within [0, n) and no longer than the host's `max`
__device__ __forceinline__ bool range_ok(int off, int cnt, int n, int max) {
    return cnt > 0 && cnt <= max && off >= 0 && (long long)off + cnt <= (long long)n;
}

// sum over the workgroup in the fixed order of vsd_kernel: butterfly within a wave, waves left to right; valid in lane 0 of wave 0
template <int NW>
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma clang fp contract(off)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                 // (red may still be read from the call before)
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) s += red[w];
    return s;
}

template <int NW>
__device__ __forceinline__ double block_nan_max(double v, double* red) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = nan_max(v, __shfl_xor(v, m));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) s = nan_max(s, red[w]);
    return s;
}

// fill the LDS tile with vertices [v0 + t0, v0 + t0 + n) as f64; a NaN coordinate is reported (min / max compares drop it)
template <int NT>
__device__ __forceinline__ bool fill_tile(const float* __restrict__ verts, int first, int n, double* sx, double* sy, double* sz) {
    bool nan = false;
    for (int j = threadIdx.x; j < n; j += NT) {
        const float* v = verts + 3 * (size_t)(first + j);
        const double x = v[0], y = v[1], z = v[2];
        nan = nan || is_nan(x) || is_nan(y) || is_nan(z);
        sx[j] = x; sy[j] = y; sz[j] = z;
    }
    return nan;
}

template <bool ADD, bool ADI>
__global__ __launch_bounds__(kPeThreads) void pe_point_kernel(const float* __restrict__ verts, int V, const int* __restrict__ vert_off,
                                                              const int* __restrict__ vert_cnt, int max_verts,
                                                              const double* __restrict__ pose_est, const double* __restrict__ pose_gt,
                                                              int nblk, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double sx[ADI ? kTile : 1], sy[ADI ? kTile : 1], sz[ADI ? kTile : 1];
    __shared__ double red[kPeThreads / 64];
    const int p = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    const int off = vert_off[p], cnt = vert_cnt[p];
    if (!range_ok(off, cnt, V, max_verts) || blk * kPtBlock >= cnt) return;          // (uniform over the workgroup; the fold reads nothing of it)
    const double* Te = pose_est + (size_t)p * 16;
    const double* Tg = pose_gt + (size_t)p * 16;
    double yx[kPts], yy[kPts], yz[kPts], mn[kPts];
    bool live[kPts];
    double add_sum = 0.0;
#pragma unroll
    for (int m = 0; m < kPts; ++m) {
        const int i = blk * kPtBlock + m * kPeThreads + tid;
        live[m] = i < cnt;
        const float* v = verts + 3 * (size_t)(off + (live[m] ? i : 0));
        const double x = v[0], y = v[1], z = v[2];
        const P3 e = xform(Te, x, y, z);
        if (ADD) {
            const P3 g = xform(Tg, x, y, z);
            const double dx = e.x - g.x, dy = e.y - g.y, dz = e.z - g.z;
            const double d = sqrt(dx * dx + dy * dy + dz * dz);
            add_sum += live[m] ? d : 0.0;
        }
        // y = Rg^T (Xe - tg)
        const double ex = e.x - Tg[3], ey = e.y - Tg[7], ez = e.z - Tg[11];
        yx[m] = Tg[0] * ex + Tg[4] * ey + Tg[8] * ez;
        yy[m] = Tg[1] * ex + Tg[5] * ey + Tg[9] * ez;
        yz[m] = Tg[2] * ex + Tg[6] * ey + Tg[10] * ez;
        mn[m] = INFINITY;
    }
    if (ADD) {
        const double s = block_sum<kPeThreads / 64>(add_sum, red);
        if (tid == 0) part[((size_t)p * nblk + blk) * 2] = s;
    }
    if (ADI) {
        bool nan = false;
        for (int t0 = 0; t0 < cnt; t0 += kTile) {
            const int n = cnt - t0 < kTile ? cnt - t0 : kTile;
            __syncthreads();
            nan = fill_tile<kPeThreads>(verts, off + t0, n, sx, sy, sz) || nan;
            __syncthreads();
#pragma unroll 4
            for (int j = 0; j < n; ++j) {
                const double vx = sx[j], vy = sy[j], vz = sz[j];
#pragma unroll
                for (int m = 0; m < kPts; ++m) {
                    const double dx = yx[m] - vx, dy = yy[m] - vy, dz = yz[m] - vz;
                    const double d2 = dx * dx + dy * dy + dz * dz;
                    mn[m] = fmin(mn[m], d2);          // (one v_min_f64; it drops a NaN, which is put back below)
                }
            }
        }
        double adi_sum = 0.0;
#pragma unroll
        for (int m = 0; m < kPts; ++m) {
            // fmin drops the NaN distances of a NaN point and would leave +inf: the NaN is put back here
            const double d = is_nan(yx[m] + yy[m] + yz[m]) ? NAN : sqrt(mn[m]);
            adi_sum += live[m] ? d : 0.0;
        }
        if (nan) adi_sum = NAN;
        const double s = block_sum<kPeThreads / 64>(adi_sum, red);
        if (tid == 0) part[((size_t)p * nblk + blk) * 2 + 1] = s;
    }
}

// sym_part: (P, max_syms, 2) maxima of squared distances;  behind: (P, nchunk) 0 / 1
template <bool MSSD, bool MSPD>
__global__ __launch_bounds__(kSymThreads) void pe_sym_kernel(const float* __restrict__ verts, int V, const int* __restrict__ vert_off,
                                                             const int* __restrict__ vert_cnt, int max_verts, const double* __restrict__ syms,
                                                             int S_total, const int* __restrict__ sym_off, const int* __restrict__ sym_cnt,
                                                             int max_syms, const double* __restrict__ pose_est,
                                                             const double* __restrict__ pose_gt, const double* __restrict__ Ks, int nchunk,
                                                             double* __restrict__ sym_part, double* __restrict__ behind) {
#pragma clang fp contract(off)
    __shared__ double red[kSymChunk][kSymThreads / 64][3];
    const int p = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const int off = vert_off[p], cnt = vert_cnt[p], soff = sym_off[p], scnt = sym_cnt[p];
    if (!range_ok(off, cnt, V, max_verts) || !range_ok(soff, scnt, S_total, max_syms) || chunk * kSymChunk >= scnt) return;
    const int s0 = chunk * kSymChunk;
    const int ns = scnt - s0 < kSymChunk ? scnt - s0 : kSymChunk;
    const int lane = tid & 63, wave = tid >> 6;
    const double* Te = pose_est + (size_t)p * 16;
    const double* Tg = pose_gt + (size_t)p * 16;
    const double* K = Ks + (size_t)p * 9;
    double k[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) k[q] = K[q];
    // one symmetry at a time: its transform stays in registers, the estimate's point is recomputed (cheaper than a tile of them)
    for (int s = 0; s < ns; ++s) {
        const double* Ts = syms + (size_t)(soff + s0 + s) * 16;
        double m3 = 0.0, m2 = 0.0, bad = 0.0;
        for (int i = tid; i < cnt; i += kSymThreads) {
            const float* v = verts + 3 * (size_t)(off + i);
            const double x = v[0], y = v[1], z = v[2];
            const P3 e = xform(Te, x, y, z);
            const P3 o = xform(Ts, x, y, z);
            const P3 g = xform(Tg, o.x, o.y, o.z);
            if (MSSD) {
                const double dx = e.x - g.x, dy = e.y - g.y, dz = e.z - g.z;
                m3 = nan_max(m3, dx * dx + dy * dy + dz * dz);
            }
            if (MSPD) {
                const double we = k[6] * e.x + k[7] * e.y + k[8] * e.z;
                const double wg = k[6] * g.x + k[7] * g.y + k[8] * g.z;
                if (!(we > 0.0) || !(wg > 0.0)) bad = 1.0;
                const double du = (k[0] * e.x + k[1] * e.y + k[2] * e.z) / we - (k[0] * g.x + k[1] * g.y + k[2] * g.z) / wg;
                const double dv = (k[3] * e.x + k[4] * e.y + k[5] * e.z) / we - (k[3] * g.x + k[4] * g.y + k[5] * g.z) / wg;
                m2 = nan_max(m2, du * du + dv * dv);
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            m3 = nan_max(m3, __shfl_xor(m3, m));
            m2 = nan_max(m2, __shfl_xor(m2, m));
            bad = nan_max(bad, __shfl_xor(bad, m));
        }
        if (lane == 0) { red[s][wave][0] = m3; red[s][wave][1] = m2; red[s][wave][2] = bad; }
    }
    __syncthreads();
    if (tid < ns) {
        double r[3];
        for (int q = 0; q < 3; ++q) {
            r[q] = red[tid][0][q];
            for (int w = 1; w < kSymThreads / 64; ++w) r[q] = nan_max(r[q], red[tid][w][q]);
        }
        double* o = sym_part + ((size_t)p * max_syms + s0 + tid) * 2;
        if (MSSD) o[0] = r[0];
        if (MSPD) o[1] = r[1];
        red[tid][0][2] = r[2];
    }
    __syncthreads();
    if (MSPD && tid == 0) {
        double bh = 0.0;
        for (int s = 0; s < ns; ++s) bh = nan_max(bh, red[s][0][2]);
        behind[(size_t)p * nchunk + chunk] = bh;
    }
}

__global__ __launch_bounds__(256) void pe_fold_kernel(int V, const int* __restrict__ vert_off, const int* __restrict__ vert_cnt, int max_verts,
                                                      int S_total, const int* __restrict__ sym_off, const int* __restrict__ sym_cnt,
                                                      int max_syms, const double* __restrict__ pose_est, const double* __restrict__ pose_gt,
                                                      const double* __restrict__ Ks, int P, int nblk, int nchunk,
                                                      const double* __restrict__ part, const double* __restrict__ sym_part,
                                                      const double* __restrict__ behind, double* __restrict__ mssd, double* __restrict__ mspd,
                                                      double* __restrict__ add, double* __restrict__ adi, int* __restrict__ status) {
#pragma clang fp contract(off)
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int off = vert_off[p], cnt = vert_cnt[p], soff = sym_off[p], scnt = sym_cnt[p];
    int st = 0;
    if (!finite_all(pose_est + (size_t)p * 16, 16) || !finite_all(pose_gt + (size_t)p * 16, 16) || !finite_all(Ks + (size_t)p * 9, 9))
        st |= NOPE_POSE_ERR_NONFINITE;
    if (!range_ok(off, cnt, V, max_verts)) st |= NOPE_POSE_ERR_VERT_RANGE;
    if (!range_ok(soff, scnt, S_total, max_syms)) st |= NOPE_POSE_ERR_SYM_RANGE;
    double r_mssd = NAN, r_mspd = NAN, r_add = NAN, r_adi = NAN;
    if (st == 0) {
        if (add || adi) {
            double sa = 0.0, si = 0.0;
            const int nb = (cnt + kPtBlock - 1) / kPtBlock;
            for (int b = 0; b < nb; ++b) {
                const double* o = part + ((size_t)p * nblk + b) * 2;
                if (add) sa += o[0];
                if (adi) si += o[1];
            }
            r_add = sa / (double)cnt;
            r_adi = si / (double)cnt;
        }
        if (mssd || mspd) {
            double m3 = INFINITY, m2 = INFINITY;
            for (int s = 0; s < scnt; ++s) {
                const double* o = sym_part + ((size_t)p * max_syms + s) * 2;
                if (mssd) m3 = nan_min(m3, o[0]);
                if (mspd) m2 = nan_min(m2, o[1]);
            }
            r_mssd = sqrt(m3);
            r_mspd = sqrt(m2);
            if (mspd) {
                bool bh = false;
                const int nc = (scnt + kSymChunk - 1) / kSymChunk;
                for (int c = 0; c < nc; ++c) bh = bh || behind[(size_t)p * nchunk + c] != 0.0;
                if (bh) { st |= NOPE_POSE_ERR_BEHIND; r_mspd = NAN; }
            }
        }
    }
    if (mssd) mssd[p] = r_mssd;
    if (mspd) mspd[p] = r_mspd;
    if (add) add[p] = r_add;
    if (adi) adi[p] = r_adi;
    status[p] = st;
}

// ---- diameter ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPeThreads) void diam_kernel(const float* __restrict__ verts, int V, const int* __restrict__ vert_off,
                                                          const int* __restrict__ vert_cnt, int max_verts, int nblk,
                                                          double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double sx[kTile], sy[kTile], sz[kTile];
    __shared__ double red[kPeThreads / 64];
    const int o = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    const int off = vert_off[o], cnt = vert_cnt[o];
    if (!range_ok(off, cnt, V, max_verts) || blk * kPtBlock >= cnt) return;
    double px[kPts], py[kPts], pz[kPts], mx[kPts];
    bool nan = false;
#pragma unroll
    for (int m = 0; m < kPts; ++m) {
        const int i = blk * kPtBlock + m * kPeThreads + tid;
        const float* v = verts + 3 * (size_t)(off + (i < cnt ? i : 0));        // (a lane past the end repeats vertex 0: a real point of the object)
        px[m] = v[0]; py[m] = v[1]; pz[m] = v[2];
        nan = nan || is_nan(px[m]) || is_nan(py[m]) || is_nan(pz[m]);
        mx[m] = 0.0;
    }
    // tiles that end before this block begins hold only pairs (i, j) with j < i, which the blocks below have as (j, i)
    for (int t0 = (blk * kPtBlock) / kTile * kTile; t0 < cnt; t0 += kTile) {
        const int n = cnt - t0 < kTile ? cnt - t0 : kTile;
        __syncthreads();
        nan = fill_tile<kPeThreads>(verts, off + t0, n, sx, sy, sz) || nan;
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const double vx = sx[j], vy = sy[j], vz = sz[j];
#pragma unroll
            for (int m = 0; m < kPts; ++m) {
                const double dx = px[m] - vx, dy = py[m] - vy, dz = pz[m] - vz;
                const double d2 = dx * dx + dy * dy + dz * dz;
                mx[m] = fmax(mx[m], d2);          // (one v_max_f64; a NaN is put back below)
            }
        }
    }
    double r = nan ? NAN : fmax(fmax(mx[0], mx[1]), fmax(mx[2], mx[3]));
    static_assert(kPts == 4, "the line above folds four points");
    r = block_nan_max<kPeThreads / 64>(r, red);
    if (tid == 0) part[(size_t)o * nblk + blk] = r;
}

__global__ __launch_bounds__(256) void diam_fold_kernel(int V, const int* __restrict__ vert_off, const int* __restrict__ vert_cnt,
                                                        int max_verts, int n_obj, int nblk, const double* __restrict__ part,
                                                        double* __restrict__ diameter) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= n_obj) return;
    const int off = vert_off[o], cnt = vert_cnt[o];
    double r = NAN;
    if (range_ok(off, cnt, V, max_verts)) {
        r = 0.0;
        const int nb = (cnt + kPtBlock - 1) / kPtBlock;
        for (int b = 0; b < nb; ++b) r = nan_max(r, part[(size_t)o * nblk + b]);
        r = sqrt(r);
    }
    diameter[o] = r;
}

template <bool A, bool B>
void launch_point(dim3 grid, hipStream_t s, const float* verts, int V, const int* vert_off, const int* vert_cnt, int max_verts,
                  const double* pose_est, const double* pose_gt, int nblk, double* part) {
    hipLaunchKernelGGL((pe_point_kernel<A, B>), grid, dim3(kPeThreads), 0, s, verts, V, vert_off, vert_cnt, max_verts, pose_est, pose_gt, nblk, part);
}

template <bool A, bool B>
void launch_sym(dim3 grid, hipStream_t s, const float* verts, int V, const int* vert_off, const int* vert_cnt, int max_verts, const double* syms,
                int S_total, const int* sym_off, const int* sym_cnt, int max_syms, const double* pose_est, const double* pose_gt, const double* K,
                int nchunk, double* sym_part, double* behind) {
    hipLaunchKernelGGL((pe_sym_kernel<A, B>), grid, dim3(kSymThreads), 0, s, verts, V, vert_off, vert_cnt, max_verts, syms, S_total, sym_off,
                       sym_cnt, max_syms, pose_est, pose_gt, K, nchunk, sym_part, behind);
}

}  // namespace

size_t pose_errors_workspace_bytes(int P, int max_verts, int max_syms) {
    if (P <= 0 || max_verts <= 0 || max_syms <= 0) return 0;
    const size_t nblk = (size_t)cdiv(max_verts, kPtBlock), nchunk = (size_t)cdiv(max_syms, kSymChunk);
    return (size_t)P * (nblk * 2 + (size_t)max_syms * 2 + nchunk) * sizeof(double);
}

int launch_pose_errors(const float* verts, int V, const int* vert_off, const int* vert_cnt, int max_verts, const double* syms, int S_total,
                       const int* sym_off, const int* sym_cnt, int max_syms, const double* pose_est, const double* pose_gt, const double* K, int P,
                       double* mssd, double* mspd, double* add, double* adi, int* status, void* ws, size_t ws_bytes, hipStream_t s) {
    if (!verts || !vert_off || !vert_cnt || !syms || !sym_off || !sym_cnt || !pose_est || !pose_gt || !K || !status || !ws) return NOPE_ERR_ARG;
    if (!mssd && !mspd && !add && !adi) return NOPE_ERR_ARG;
    if (V <= 0 || S_total <= 0 || P <= 0 || P > 65535 || max_verts <= 0 || max_syms <= 0) return NOPE_ERR_ARG;
    if (ws_bytes < pose_errors_workspace_bytes(P, max_verts, max_syms)) return NOPE_ERR_WORKSPACE;
    const int nblk = cdiv(max_verts, kPtBlock), nchunk = cdiv(max_syms, kSymChunk);
    double* part = static_cast<double*>(ws);
    double* sym_part = part + (size_t)P * nblk * 2;
    double* behind = sym_part + (size_t)P * max_syms * 2;
    if (add || adi) {
        const dim3 grid((unsigned)nblk, (unsigned)P);
        if (add && adi) launch_point<true, true>(grid, s, verts, V, vert_off, vert_cnt, max_verts, pose_est, pose_gt, nblk, part);
        else if (adi) launch_point<false, true>(grid, s, verts, V, vert_off, vert_cnt, max_verts, pose_est, pose_gt, nblk, part);
        else launch_point<true, false>(grid, s, verts, V, vert_off, vert_cnt, max_verts, pose_est, pose_gt, nblk, part);
        NOPE_CHECK_LAUNCH();
    }
    if (mssd || mspd) {
        const dim3 grid((unsigned)nchunk, (unsigned)P);
        if (mssd && mspd)
            launch_sym<true, true>(grid, s, verts, V, vert_off, vert_cnt, max_verts, syms, S_total, sym_off, sym_cnt, max_syms, pose_est, pose_gt, K,
                                   nchunk, sym_part, behind);
        else if (mssd)
            launch_sym<true, false>(grid, s, verts, V, vert_off, vert_cnt, max_verts, syms, S_total, sym_off, sym_cnt, max_syms, pose_est, pose_gt, K,
                                    nchunk, sym_part, behind);
        else
            launch_sym<false, true>(grid, s, verts, V, vert_off, vert_cnt, max_verts, syms, S_total, sym_off, sym_cnt, max_syms, pose_est, pose_gt, K,
                                    nchunk, sym_part, behind);
        NOPE_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(pe_fold_kernel, dim3((unsigned)cdiv(P, 256)), dim3(256), 0, s, V, vert_off, vert_cnt, max_verts, S_total, sym_off, sym_cnt,
                       max_syms, pose_est, pose_gt, K, P, nblk, nchunk, part, sym_part, behind, mssd, mspd, add, adi, status);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

size_t mesh_diameter_workspace_bytes(int n_obj, int max_verts) {
    if (n_obj <= 0 || max_verts <= 0) return 0;
    return (size_t)n_obj * (size_t)cdiv(max_verts, kPtBlock) * sizeof(double);
}

int launch_mesh_diameter(const float* verts, int V, const int* vert_off, const int* vert_cnt, int n_obj, int max_verts, double* diameter, void* ws,
                         size_t ws_bytes, hipStream_t s) {
    if (!verts || !vert_off || !vert_cnt || !diameter || !ws) return NOPE_ERR_ARG;
    if (V <= 0 || n_obj <= 0 || n_obj > 65535 || max_verts <= 0) return NOPE_ERR_ARG;
    if (ws_bytes < mesh_diameter_workspace_bytes(n_obj, max_verts)) return NOPE_ERR_WORKSPACE;
    const int nblk = cdiv(max_verts, kPtBlock);
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(diam_kernel, dim3((unsigned)nblk, (unsigned)n_obj), dim3(kPeThreads), 0, s, verts, V, vert_off, vert_cnt, max_verts, nblk, part);
    NOPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(diam_fold_kernel, dim3((unsigned)cdiv(n_obj, 256)), dim3(256), 0, s, V, vert_off, vert_cnt, max_verts, n_obj, nblk, part,
                       diameter);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

}  // namespace nope
