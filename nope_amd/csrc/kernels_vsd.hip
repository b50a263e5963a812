// T-LESS evaluation on the device (nope_amd/vsd.py): replaces
//   pyrenderer -- pyrender's OffscreenRenderer, DEPTH_ONLY                  src/poses/vsd.py:25-54
//   vsd_obj's per-pose arithmetic                                          src/poses/vsd.py:57-132
//   depth_im_to_dist_im_fast, estimate_visib_mask_gt / _est (bop_toolkit)  src/poses/vsd_utils.py
//
// Depth rasteriser.  P poses of meshes in one shared vertex / face buffer, each pose its own face range, 4x4 object-to-camera
// pose (OpenCV axes) and K.  Pixel (x, y) samples the image point (x + 0.5, y + 0.5); depth is the camera-frame Z of the nearest
// surface, interpolated perspective-correctly (1/Z is affine in screen space), 0 where nothing is hit.  No face culling.  The
// z-buffer holds ~bits(Z) (0 = empty): for positive floats a larger complement is a nearer surface, so an unsigned atomic MAX
// keeps the nearest one whatever order the triangles land in -- the result is deterministic.  Set-up and coverage are f64.
// A triangle with a vertex at Z <= znear is not clipped: it is skipped and counted per pose (the binding raises).
//   raster_tri_kernel  one thread per (pose, face): set-up, and triangles whose pixel box holds <= kSmallArea pixels are drawn
//                      by that thread; larger ones are appended to a list
//   raster_big_kernel  the list: one workgroup per (triangle, band of rows), 16 x 16 pixel steps -- a triangle that covers the
//                      image runs on kBigSplit workgroups of 256 lanes, never on one lane
//   depth_final_kernel ~bits -> Z (0 stays 0)
//
// VSD.  One pass over (test, gt, k estimates) per image: test and gt pixels are read once for all k.  Distance images in f64
// from integer pixel coordinates (BOP convention; the rasteriser's +0.5 is the reference's own disagreement), the visibility
// test in f32, counts as integers, the tlinear sum per thread in pixel order, then a fixed butterfly / wave / block order:
// the same bits on every run.  vsd_final_kernel combines the per-block partials in block order.
#include <cmath>

#include "nope_common.h"

namespace nope {

namespace {

constexpr double kZnear = 0.05, kZfar = 100000.0;       // vsd.py:42-44
constexpr long long kSmallArea = 64;
constexpr int kBigBlocks = 256, kBigSplit = 8;

struct Tri {
    double x[3], y[3], iz[3], area;
    int x0, x1, y0, y1;
};

// 1: draw; 0: nothing to draw (degenerate, outside the image, bad index); -1: a vertex at Z <= znear
__device__ __forceinline__ int tri_setup(const float* __restrict__ verts, int V, const int* __restrict__ faces, int f,
                                         const double* __restrict__ T, const double* __restrict__ Kp, int H, int W, Tri& t) {
#pragma clang fp contract(off)
    const double fx = Kp[0], cx = Kp[2], fy = Kp[4], cy = Kp[5];
    bool near = false;
    for (int i = 0; i < 3; ++i) {
        const int vi = faces[3 * (size_t)f + i];
        if ((unsigned)vi >= (unsigned)V) return 0;
        const double vx = verts[3 * (size_t)vi], vy = verts[3 * (size_t)vi + 1], vz = verts[3 * (size_t)vi + 2];
        const double X = T[0] * vx + T[1] * vy + T[2] * vz + T[3];
        const double Y = T[4] * vx + T[5] * vy + T[6] * vz + T[7];
        const double Z = T[8] * vx + T[9] * vy + T[10] * vz + T[11];
        if (!(Z > kZnear)) near = true;
        t.x[i] = fx * X / Z + cx;
        t.y[i] = fy * Y / Z + cy;
        t.iz[i] = 1.0 / Z;
    }
    if (near) return -1;
    t.area = (t.x[1] - t.x[0]) * (t.y[2] - t.y[0]) - (t.x[2] - t.x[0]) * (t.y[1] - t.y[0]);
    const double aa = fabs(t.area);
    if (!(aa > 0.0 && aa < 1e300)) return 0;         // degenerate, or non-finite
    // pixels whose sample point x + 0.5 lies in [min, max]
    const double xa = fmax(ceil(fmin(fmin(t.x[0], t.x[1]), t.x[2]) - 0.5), 0.0);
    const double xb = fmin(floor(fmax(fmax(t.x[0], t.x[1]), t.x[2]) - 0.5), (double)(W - 1));
    const double ya = fmax(ceil(fmin(fmin(t.y[0], t.y[1]), t.y[2]) - 0.5), 0.0);
    const double yb = fmin(floor(fmax(fmax(t.y[0], t.y[1]), t.y[2]) - 0.5), (double)(H - 1));
    if (!(xa <= xb) || !(ya <= yb)) return 0;
    t.x0 = (int)xa; t.x1 = (int)xb; t.y0 = (int)ya; t.y1 = (int)yb;
    return 1;
}

__device__ __forceinline__ void shade(const Tri& t, int px, int py, int W, unsigned* __restrict__ zb) {
#pragma clang fp contract(off)
    const double sx = px + 0.5, sy = py + 0.5;
    // edge(a, b, p) = (b - a) x (p - a); w_i = the edge opposite vertex i, all of the sign of `area` inside
    double w0 = (t.x[2] - t.x[1]) * (sy - t.y[1]) - (t.y[2] - t.y[1]) * (sx - t.x[1]);
    double w1 = (t.x[0] - t.x[2]) * (sy - t.y[2]) - (t.y[0] - t.y[2]) * (sx - t.x[2]);
    double w2 = (t.x[1] - t.x[0]) * (sy - t.y[0]) - (t.y[1] - t.y[0]) * (sx - t.x[0]);
    if (t.area < 0.0) { w0 = -w0; w1 = -w1; w2 = -w2; }
    if (w0 < 0.0 || w1 < 0.0 || w2 < 0.0) return;
    const double a = t.area < 0.0 ? -t.area : t.area;
    const double iz = (w0 * t.iz[0] + w1 * t.iz[1] + w2 * t.iz[2]) / a;
    const double z = 1.0 / iz;
    if (!(z > kZnear) || z > kZfar) return;
    const unsigned bits = ~__builtin_bit_cast(unsigned, (float)z);
    atomicMax(zb + (size_t)py * W + px, bits);
}

__global__ __launch_bounds__(256) void raster_tri_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                         const int* __restrict__ face_off, const int* __restrict__ face_cnt, int max_faces,
                                                         const double* __restrict__ poses, const double* __restrict__ Ks, int H, int W,
                                                         unsigned* __restrict__ zbuf, unsigned* __restrict__ skipped,
                                                         int* __restrict__ big, unsigned* __restrict__ big_count) {
    const int p = blockIdx.y;
    const int fl = blockIdx.x * 256 + threadIdx.x;
    const int off = face_off[p], cnt = face_cnt[p];
    if (fl >= cnt || fl >= max_faces || off < 0 || (long long)off + fl >= F) return;      // (<= P * max_faces list entries)
    const int f = off + fl;
    Tri t;
    const int st = tri_setup(verts, V, faces, f, poses + (size_t)p * 16, Ks + (size_t)p * 9, H, W, t);
    if (st < 0) { atomicAdd(skipped + p, 1u); return; }
    if (st == 0) return;
    if ((long long)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) > kSmallArea) {
        const unsigned e = atomicAdd(big_count, 1u);        // capacity: one entry per launched (pose, face)
        big[2 * (size_t)e] = p;
        big[2 * (size_t)e + 1] = f;
        return;
    }
    unsigned* zb = zbuf + (size_t)p * H * W;
    for (int y = t.y0; y <= t.y1; ++y)
        for (int x = t.x0; x <= t.x1; ++x) shade(t, x, y, W, zb);
}

__global__ __launch_bounds__(256) void raster_big_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces,
                                                         const double* __restrict__ poses, const double* __restrict__ Ks, int H, int W,
                                                         unsigned* __restrict__ zbuf, const int* __restrict__ big,
                                                         const unsigned* __restrict__ big_count) {
    const unsigned n = *big_count;
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    for (unsigned e = blockIdx.x; e < n; e += gridDim.x) {
        const int p = big[2 * (size_t)e], f = big[2 * (size_t)e + 1];
        Tri t;
        if (tri_setup(verts, V, faces, f, poses + (size_t)p * 16, Ks + (size_t)p * 9, H, W, t) != 1) continue;
        unsigned* zb = zbuf + (size_t)p * H * W;
        for (int yb = t.y0 + 16 * (int)blockIdx.y; yb <= t.y1; yb += 16 * (int)gridDim.y) {
            const int y = yb + ly;
            for (int xb = t.x0; xb <= t.x1; xb += 16) {
                const int x = xb + lx;
                if (x <= t.x1 && y <= t.y1) shade(t, x, y, W, zb);
            }
        }
    }
}

__global__ __launch_bounds__(256) void depth_final_kernel(unsigned* __restrict__ zbuf, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned v = zbuf[i];
        zbuf[i] = v ? ~v : 0u;          // the f32 bits of Z, or +0
    }
}

// ---- VSD ---------------------------------------------------------------------------------------------------------------------

// depth_im_to_dist_im_fast: sqrt((pre_X d)^2 + (pre_Y d)^2 + d^2), numpy's evaluation order, no contraction
__device__ __forceinline__ double dist_of(double prex, double prey, double d) {
#pragma clang fp contract(off)
    if (d == 0.0) return 0.0;
    const double a = prex * d, b = prey * d;
    return sqrt(a * a + b * b + d * d);
}

// _estimate_visib_mask: d_diff = f32(d_model) - f32(d_test) <= delta in f32
__device__ __forceinline__ bool visible(double d_model, double d_test, float delta, bool bop18) {
    const float diff = (float)d_model - (float)d_test;
    if (bop18) return diff <= delta && d_test > 0.0 && d_model > 0.0;
    return (diff <= delta || d_test == 0.0) && d_model > 0.0;
}

struct alignas(16) F4 { float v[4]; };

template <int VW>
__device__ __forceinline__ void load_px(const float* __restrict__ p, size_t i, float* out) {
    if constexpr (VW == 4) {
        const F4 q = *reinterpret_cast<const F4*>(p + i);
#pragma unroll
        for (int v = 0; v < 4; ++v) out[v] = q.v[v];
    } else {
        out[0] = p[i];
    }
}

// per thread: groups of VW consecutive pixels (flat index) g = blk * 256 + tid, + nblk * 256, ...
template <int KC, int VW>
__global__ __launch_bounds__(256) void vsd_kernel(const float* __restrict__ dtest, const float* __restrict__ dgt,
                                                  const float* __restrict__ dest, const double* __restrict__ Ks, int k, int H, int W,
                                                  int nblk, double delta, double tau, int tlinear, int bop18, double* __restrict__ part) {
#pragma clang fp contract(off)
    const int b = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    const size_t HW = (size_t)H * W, groups = HW / VW;
    const double* Kp = Ks + (size_t)b * 9;
    const double fx = Kp[0], cx = Kp[2], fy = Kp[4], cy = Kp[5];
    const float delta_f = (float)delta;
    int n_inter[KC], n_union[KC];
    double cost[KC];
#pragma unroll
    for (int j = 0; j < KC; ++j) { n_inter[j] = 0; n_union[j] = 0; cost[j] = 0.0; }
    const float* T = dtest + (size_t)b * HW;
    const float* G = dgt + (size_t)b * HW;
    for (size_t g = (size_t)blk * 256 + tid; g < groups; g += (size_t)nblk * 256) {
        float t4[VW], g4[VW];
        load_px<VW>(T, g * VW, t4);
        load_px<VW>(G, g * VW, g4);
        double prex[VW], prey[VW], dt[VW], dg[VW];
        bool vg[VW];
#pragma unroll
        for (int v = 0; v < VW; ++v) {
            const unsigned i = (unsigned)(g * VW + v);                  // (H W <= 2^30: 32-bit index arithmetic)
            const int y = (int)(i / (unsigned)W), x = (int)(i - (unsigned)y * (unsigned)W);
            prex[v] = ((double)x - cx) / fx;
            prey[v] = ((double)y - cy) / fy;
            dt[v] = dist_of(prex[v], prey[v], (double)t4[v]);
            dg[v] = dist_of(prex[v], prey[v], (double)g4[v]);
            vg[v] = visible(dg[v], dt[v], delta_f, bop18);
        }
#pragma unroll
        for (int j = 0; j < KC; ++j) {
            if (j >= k) continue;
            float e4[VW];
            load_px<VW>(dest + ((size_t)b * k + j) * HW, g * VW, e4);
#pragma unroll
            for (int v = 0; v < VW; ++v) {
                const double de = dist_of(prex[v], prey[v], (double)e4[v]);
                const bool ve = visible(de, dt[v], delta_f, bop18) || (vg[v] && de > 0.0);
                n_union[j] += (vg[v] || ve) ? 1 : 0;
                if (vg[v] && ve) {
                    n_inter[j] += 1;
                    const double d = fabs(dg[v] - de);
                    if (tlinear) {
                        double c = d / tau;
                        if (c > 1.0) c = 1.0;
                        cost[j] += c;
                    } else {
                        cost[j] += d >= tau ? 1.0 : 0.0;
                    }
                }
            }
        }
    }
    __shared__ double red[4][KC][3];
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int j = 0; j < KC; ++j) {
        double a = (double)n_inter[j], u = (double)n_union[j], c = cost[j];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            a += __shfl_xor(a, m);
            u += __shfl_xor(u, m);
            c += __shfl_xor(c, m);
        }
        if (lane == 0) { red[wave][j][0] = a; red[wave][j][1] = u; red[wave][j][2] = c; }
    }
    __syncthreads();
    if (tid < k && tid < KC) {
        double s[3];
        for (int q = 0; q < 3; ++q) s[q] = ((red[0][tid][q] + red[1][tid][q]) + red[2][tid][q]) + red[3][tid][q];
        double* o = part + (((size_t)b * nblk + blk) * k + tid) * 3;
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
    }
}

__global__ __launch_bounds__(256) void vsd_final_kernel(const double* __restrict__ part, int B, int k, int nblk, double* __restrict__ err) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= B * k) return;
    const int b = t / k, j = t - b * k;
    double inter = 0.0, uni = 0.0, cost = 0.0;
    for (int blk = 0; blk < nblk; ++blk) {
        const double* o = part + (((size_t)b * nblk + blk) * k + j) * 3;
        inter += o[0]; uni += o[1]; cost += o[2];
    }
    // (np.sum(costs) + visib_comp_count) / float(visib_union_count), vsd.py:115-131
    err[t] = uni == 0.0 ? 1.0 : (cost + (uni - inter)) / uni;
}

int vsd_blocks_per_image(int H, int W) {
    const size_t HW = (size_t)H * W, groups = HW % 4 == 0 ? HW / 4 : HW;
    const size_t per_block = 256 * 4;      // ~4 pixel groups per thread
    const size_t n = (groups + per_block - 1) / per_block;
    return (int)(n < 1 ? 1 : (n > 4096 ? 4096 : n));
}

template <int KC, int VW>
void launch_vsd_kc(const float* t, const float* g, const float* e, const double* K, int B, int k, int H, int W, int nblk, double delta,
                   double tau, int tlinear, int bop18, double* part, hipStream_t s) {
    hipLaunchKernelGGL((vsd_kernel<KC, VW>), dim3((unsigned)nblk, (unsigned)B), dim3(256), 0, s, t, g, e, K, k, H, W, nblk, delta, tau, tlinear,
                       bop18, part);
}

template <int KC>
void launch_vsd_vw(bool v4, const float* t, const float* g, const float* e, const double* K, int B, int k, int H, int W, int nblk,
                   double delta, double tau, int tlinear, int bop18, double* part, hipStream_t s) {
    if (v4) launch_vsd_kc<KC, 4>(t, g, e, K, B, k, H, W, nblk, delta, tau, tlinear, bop18, part, s);
    else launch_vsd_kc<KC, 1>(t, g, e, K, B, k, H, W, nblk, delta, tau, tlinear, bop18, part, s);
}

}  // namespace

size_t render_depth_workspace_bytes(int P, int max_faces) {
    if (P <= 0 || max_faces < 0) return 0;
    return 256 + (size_t)P * (size_t)max_faces * 2 * sizeof(int);
}

int launch_render_depth(const float* verts, int V, const int* faces, int F, const int* face_off, const int* face_cnt, int max_faces,
                        const double* poses, const double* K, int P, int H, int W, float* depth, unsigned* skipped, void* ws,
                        size_t ws_bytes, hipStream_t s) {
    if (!verts || !faces || !face_off || !face_cnt || !poses || !K || !depth || !skipped || !ws) return NOPE_ERR_ARG;
    if (V <= 0 || F <= 0 || P <= 0 || P > 65535 || H <= 0 || W <= 0 || max_faces < 0 || (long long)H * W > (1ll << 30)) return NOPE_ERR_ARG;
    if (ws_bytes < render_depth_workspace_bytes(P, max_faces)) return NOPE_ERR_WORKSPACE;
    const size_t n = (size_t)P * H * W;
    unsigned* zb = reinterpret_cast<unsigned*>(depth);
    unsigned* big_count = static_cast<unsigned*>(ws);
    int* big = reinterpret_cast<int*>(static_cast<char*>(ws) + 256);
    if (hipMemsetAsync(zb, 0, n * sizeof(unsigned), s) != hipSuccess) return NOPE_ERR_LAUNCH;
    if (hipMemsetAsync(skipped, 0, (size_t)P * sizeof(unsigned), s) != hipSuccess) return NOPE_ERR_LAUNCH;
    if (hipMemsetAsync(big_count, 0, sizeof(unsigned), s) != hipSuccess) return NOPE_ERR_LAUNCH;
    if (max_faces > 0) {
        hipLaunchKernelGGL(raster_tri_kernel, dim3((unsigned)cdiv(max_faces, 256), (unsigned)P), dim3(256), 0, s, verts, V, faces, F, face_off,
                           face_cnt, max_faces, poses, K, H, W, zb, skipped, big, big_count);
        NOPE_CHECK_LAUNCH();
        hipLaunchKernelGGL(raster_big_kernel, dim3(kBigBlocks, kBigSplit), dim3(256), 0, s, verts, V, faces, poses, K, H, W, zb, big, big_count);
        NOPE_CHECK_LAUNCH();
    }
    const size_t nb = (n + 255) / 256;
    hipLaunchKernelGGL(depth_final_kernel, dim3((unsigned)(nb < 8192 ? nb : 8192)), dim3(256), 0, s, zb, n);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

size_t vsd_workspace_bytes(int B, int k, int H, int W) {
    if (B <= 0 || k <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)B * vsd_blocks_per_image(H, W) * k * 3 * sizeof(double);
}

int launch_vsd(const float* dtest, const float* dgt, const float* dest, const double* K, int B, int k, int H, int W, double delta, double tau,
               int cost_type, int visib_mode, double* err, void* ws, size_t ws_bytes, hipStream_t s) {
    if (!dtest || !dgt || !dest || !K || !err || !ws) return NOPE_ERR_ARG;
    if (B <= 0 || B > 65535 || k <= 0 || k > 16 || H <= 0 || W <= 0 || (long long)H * W > (1ll << 30)) return NOPE_ERR_ARG;
    if ((cost_type != NOPE_VSD_STEP && cost_type != NOPE_VSD_TLINEAR) || (visib_mode != NOPE_VISIB_BOP19 && visib_mode != NOPE_VISIB_BOP18))
        return NOPE_ERR_ARG;
    if (!(tau > 0.0)) return NOPE_ERR_ARG;
    if (ws_bytes < vsd_workspace_bytes(B, k, H, W)) return NOPE_ERR_WORKSPACE;
    const int nblk = vsd_blocks_per_image(H, W);
    // (4-pixel groups need HW % 4 == 0 and 16-byte aligned images; otherwise the scalar form walks 4x the groups on the same grid)
    const bool v4 = ((size_t)H * W) % 4 == 0 && ((uintptr_t)dtest | (uintptr_t)dgt | (uintptr_t)dest) % 16 == 0;
    double* part = static_cast<double*>(ws);
    const int tl = cost_type == NOPE_VSD_TLINEAR, b18 = visib_mode == NOPE_VISIB_BOP18;
    if (k == 1) launch_vsd_vw<1>(v4, dtest, dgt, dest, K, B, k, H, W, nblk, delta, tau, tl, b18, part, s);
    else if (k <= 5) launch_vsd_vw<5>(v4, dtest, dgt, dest, K, B, k, H, W, nblk, delta, tau, tl, b18, part, s);
    else launch_vsd_vw<16>(v4, dtest, dgt, dest, K, B, k, H, W, nblk, delta, tau, tl, b18, part, s);
    NOPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(vsd_final_kernel, dim3((unsigned)cdiv(B * k, 256)), dim3(256), 0, s, part, B, k, nblk, err);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

}  // namespace nope
