// Visualisation outputs on the device (nope_amd/vis.py): replaces, per picture,
//   unnormalize_to_zero_to_one                                             src/model/utils.py:12-15
//   put_image_to_grid (f16 cast, scatter into a zero grid, margin column)  src/utils/visualization_utils.py:43-57
//   clone + F.interpolate(..., (64, 64), bilinear, align_corners=False)    src/model/model.py:232-235, :298-301, :340-343
//   torchvision.utils.save_image: make_grid(nrow, padding 2, pad 0), then mul(255).add_(0.5).clamp_(0, 255).to(uint8) ON THE F16 GRID
//
// A picture is up to 8 columns of f32 NCHW image stacks read in place (nope_vis_column): image b * (n_cols + 1) + i of a frame is column i
// of sample b, image b * (n_cols + 1) + n_cols the zero margin.
//   vis_grid_kernel   the full-size f16 grid (what the reference saves as `vis_imgs`): flags in f32, one cast.  One lane per VW elements.
//   vis_sheet_kernel  the bytes of the PNG, (F, Hs, Ws, 3) u8.  Every step is defined on the f16 value the reference would hold there:
//                     flags in f32 -> f16 -> four taps, weights and the sum in f32 -> f16 -> * 255 -> f16 -> + 0.5 -> f16 -> clamp, truncate.
//                     One workgroup row per (sheet row, frame): everything that depends on y (cell row, tap rows, row weights) is uniform in
//                     the workgroup; consecutive lanes walk the row, each lane owns one ALIGNED dword of it -- at most two pixels -- and stores
//                     it whole; the up to three bytes in front of a row's first / behind its last whole dword are byte stores (rows and frames
//                     start at any byte offset: Ws * 3 is not a multiple of 4).
// No LDS, no atomics: a pure gather.  All arithmetic is written in float with explicit f16 casts, contraction off -- the same roundings
// from the device compiler and from the interpreter build.
#include "nope_common.h"

namespace nope {

namespace {

struct VisCols {
    nope_vis_column c[NOPE_VIS_MAX_COLS];
};

// the three planes of column `col`'s image for sample b, frame f (elements from col.data); a gathered column reads frame index[b * stride]
// clamped into [0, index_limit)
__device__ __forceinline__ const float* vis_image(const nope_vis_column& col, int b, int f) {
    long long fr = f;
    if (col.index) {
        fr = col.index[(long long)b * col.index_stride];
        fr = fr < 0 ? 0 : (fr >= col.index_limit ? col.index_limit - 1 : fr);
    }
    return col.data + (long long)b * col.stride_b + fr * col.stride_f;
}

__device__ __forceinline__ f16_t vis_flags(float v, int flags) {
#pragma clang fp contract(off)
    if (flags & NOPE_VIS_UNNORMALIZE) v = (v + 1.0f) * 0.5f;
    if (flags & NOPE_VIS_CLAMP) v = fminf(fmaxf(v, 0.0f), 1.0f);
    return (f16_t)v;
}

template <int VW>
__global__ __launch_bounds__(256) void vis_grid_kernel(VisCols cols, int n_cols, int plane3, f16_t* __restrict__ grid) {
    const int e = (blockIdx.x * 256 + threadIdx.x) * VW;        // element of the image's 3 * H * W
    if (e >= plane3) return;
    const int k = blockIdx.y, f = blockIdx.z, n_img = gridDim.y;
    const int b = k / (n_cols + 1), i = k - b * (n_cols + 1);
    f16_t* o = grid + ((long long)f * n_img + k) * plane3 + e;
    f16_t v[VW];
    if (i == n_cols) {
        for (int j = 0; j < VW; ++j) v[j] = (f16_t)0.0f;
    } else {
        const nope_vis_column& col = cols.c[i];
        const float* src = vis_image(col, b, f) + e;
        float x[VW];
        if (VW == 4) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(src);
            for (int j = 0; j < VW; ++j) x[j] = t[j];
        } else {
            for (int j = 0; j < VW; ++j) x[j] = src[j];
        }
        for (int j = 0; j < VW; ++j) v[j] = vis_flags(x[j], col.flags);
    }
    if (VW == 4) {
        union { f16_t h[4]; f32x2 w; } u;
        for (int j = 0; j < 4; ++j) u.h[j] = v[j];
        *reinterpret_cast<f32x2*>(o) = u.w;
    } else {
        for (int j = 0; j < VW; ++j) o[j] = v[j];
    }
}

// one axis of F.interpolate(bilinear, align_corners=False): output o of `tile` from `n` source samples
struct VisTap { int i0, i1; float l0, l1; };
__device__ __forceinline__ VisTap vis_tap(int o, float scale, int n) {
#pragma clang fp contract(off)
    const float src = fmaxf(scale * ((float)o + 0.5f) - 0.5f, 0.0f);
    VisTap t;
    t.i0 = (int)src < n - 1 ? (int)src : n - 1;
    t.i1 = t.i0 + 1 < n - 1 ? t.i0 + 1 : n - 1;
    t.l1 = src - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

// a sheet pixel: where its four taps are (plane 0; `live` false: padding, margin image or empty slot -> 0)
struct VisPixel { bool live; const float* p0; const float* p1; int x0, x1; float l0x, l1x; int flags; };

__device__ __forceinline__ VisPixel vis_pixel(const VisCols& cols, int n_cols, int n_img, int x, int f, int H, int W, int tile, int padding,
                                              int xmaps, int cy, bool row_live, const VisTap& ty, float scale_x, int Ws) {
    VisPixel p;
    p.live = false;
    const int cell = tile + padding;
    const int cx = x / cell, rx = x - cx * cell;
    if (!row_live || x >= Ws || cx >= xmaps || rx < padding) return p;
    const int k = cy * xmaps + cx;
    if (k >= n_img) return p;
    const int b = k / (n_cols + 1), i = k - b * (n_cols + 1);
    if (i == n_cols) return p;
    const nope_vis_column& col = cols.c[i];
    const float* img = vis_image(col, b, f);
    const VisTap tx = vis_tap(rx - padding, scale_x, W);
    p.live = true;
    p.p0 = img + (long long)ty.i0 * W;
    p.p1 = img + (long long)ty.i1 * W;
    p.x0 = tx.i0; p.x1 = tx.i1; p.l0x = tx.l0; p.l1x = tx.l1;
    p.flags = col.flags;
    return p;
}

__device__ __forceinline__ unsigned vis_byte(const VisPixel& p, int c, long long plane, const VisTap& ty) {
#pragma clang fp contract(off)
    if (!p.live) return 0u;
    const float* r0 = p.p0 + c * plane;
    const float* r1 = p.p1 + c * plane;
    const float a = (float)vis_flags(r0[p.x0], p.flags), b = (float)vis_flags(r0[p.x1], p.flags);
    const float cc = (float)vis_flags(r1[p.x0], p.flags), d = (float)vis_flags(r1[p.x1], p.flags);
    const f16_t v = (f16_t)(ty.l0 * (p.l0x * a + p.l1x * b) + ty.l1 * (p.l0x * cc + p.l1x * d));
    const f16_t s = (f16_t)((float)v * 255.0f);                  // mul(255) on the f16 grid
    const float q = (float)(f16_t)((float)s + 0.5f);             // add_(0.5)
    return (unsigned)(int)fminf(fmaxf(q, 0.0f), 255.0f);         // clamp_(0, 255).to(uint8)
}

__global__ __launch_bounds__(256) void vis_sheet_kernel(VisCols cols, int n_cols, int n_img, int H, int W, int tile, int nrow_bytes, int Ws,
                                                        int padding, int xmaps, int ymaps, unsigned char* __restrict__ sheet) {
    const int y = blockIdx.y, f = blockIdx.z, Hs = gridDim.y;
    unsigned char* row = sheet + ((long long)f * Hs + y) * nrow_bytes;
    const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 3);
    // lane t owns the aligned dword at row - mis + 4 t: row bytes [4 t - mis, 4 t - mis + 4) cut to [0, nrow_bytes)
    const int first = (blockIdx.x * 256 + threadIdx.x) * 4 - mis;
    const int lo = first < 0 ? 0 : first, hi = first + 4 < nrow_bytes ? first + 4 : nrow_bytes;
    if (lo >= hi) return;
    const int cell = tile + padding;
    const int cy = y / cell, ry = y - cy * cell;
    const bool row_live = cy < ymaps && ry >= padding;
    const float scale_y = (float)H / (float)tile, scale_x = (float)W / (float)tile;
    const VisTap ty = vis_tap(row_live ? ry - padding : 0, scale_y, H);
    const int x = lo / 3, c0 = lo - 3 * x;
    const VisPixel pa = vis_pixel(cols, n_cols, n_img, x, f, H, W, tile, padding, xmaps, cy, row_live, ty, scale_x, Ws);
    const VisPixel pb = vis_pixel(cols, n_cols, n_img, x + 1, f, H, W, tile, padding, xmaps, cy, row_live, ty, scale_x, Ws);
    const long long plane = (long long)H * W;
    unsigned word = 0;
    for (int j = 0; j < 4; ++j) {
        const int r = first + j;
        if (r < lo || r >= hi) continue;
        const int d = c0 + (r - lo);                // 0 .. 5: channel d of pixel x, or channel d - 3 of pixel x + 1
        const unsigned v = d < 3 ? vis_byte(pa, d, plane, ty) : vis_byte(pb, d - 3, plane, ty);
        word |= v << (8 * j);
    }
    if (hi - lo == 4) {
        *reinterpret_cast<unsigned*>(row + first) = word;
    } else {
        for (int j = 0; j < 4; ++j) {
            const int r = first + j;
            if (r >= lo && r < hi) row[r] = (unsigned char)(word >> (8 * j));
        }
    }
}

int vis_check(const nope_vis_column* cols, int n_cols, int B, int F, int H, int W) {
    if (n_cols < 1 || n_cols > NOPE_VIS_MAX_COLS || B <= 0 || H <= 0 || W <= 0 || F < 0) return NOPE_ERR_ARG;
    if (F > 65535 || (long long)B * (n_cols + 1) > (1 << 24) || (long long)H * W > (1ll << 28)) return NOPE_ERR_ARG;
    if (F == 0) return NOPE_OK;
    if (!cols) return NOPE_ERR_ARG;
    for (int i = 0; i < n_cols; ++i) {
        if (!cols[i].data) return NOPE_ERR_ARG;
        if (cols[i].index && cols[i].index_limit < 1) return NOPE_ERR_ARG;
    }
    return NOPE_OK;
}

}  // namespace

static int vis_sheet_size(int n_cols, int B, int tile, int nrow, int padding, int* Hs, int* Ws) {
    if (n_cols < 1 || n_cols > NOPE_VIS_MAX_COLS || B <= 0 || tile <= 0 || nrow <= 0 || padding < 0) return NOPE_ERR_ARG;
    const long long n_img = (long long)B * (n_cols + 1);
    const long long xmaps = nrow < n_img ? nrow : n_img, ymaps = (n_img + xmaps - 1) / xmaps;
    const long long hs = ((long long)tile + padding) * ymaps + padding, ws = ((long long)tile + padding) * xmaps + padding;
    if (hs > 65535 || ws * 3 > (1ll << 30)) return NOPE_ERR_ARG;
    *Hs = (int)hs; *Ws = (int)ws;
    return NOPE_OK;
}

int launch_vis_grid(const nope_vis_column* cols, int n_cols, int B, int F, int H, int W, f16_t* grid, hipStream_t s) {
    if (const int e = vis_check(cols, n_cols, B, F, H, W)) return e;
    if (F == 0) return NOPE_OK;
    const int n_img = B * (n_cols + 1);
    if (!grid || n_img > 65535) return NOPE_ERR_ARG;
    VisCols c = {};
    const long long plane3 = 3ll * H * W;
    // four elements per lane need every image to start on 16 bytes (f32 source) / 8 bytes (f16 grid)
    bool v4 = plane3 % 4 == 0 && reinterpret_cast<uintptr_t>(grid) % 8 == 0;
    for (int i = 0; i < n_cols; ++i) {
        c.c[i] = cols[i];
        v4 = v4 && reinterpret_cast<uintptr_t>(cols[i].data) % 16 == 0 && cols[i].stride_b % 4 == 0 && cols[i].stride_f % 4 == 0;
    }
    const dim3 g((unsigned)((plane3 / (v4 ? 4 : 1) + 255) / 256), (unsigned)n_img, (unsigned)F);
    if (v4) hipLaunchKernelGGL(vis_grid_kernel<4>, g, dim3(256), 0, s, c, n_cols, (int)plane3, grid);
    else hipLaunchKernelGGL(vis_grid_kernel<1>, g, dim3(256), 0, s, c, n_cols, (int)plane3, grid);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_vis_sheet(const nope_vis_column* cols, int n_cols, int B, int F, int H, int W, int tile, int nrow, int padding,
                     unsigned char* sheet, hipStream_t s) {
    if (const int e = vis_check(cols, n_cols, B, F, H, W)) return e;
    int Hs = 0, Ws = 0;
    if (const int e = vis_sheet_size(n_cols, B, tile, nrow, padding, &Hs, &Ws)) return e;
    if (F == 0) return NOPE_OK;
    if (!sheet) return NOPE_ERR_ARG;
    VisCols c = {};
    for (int i = 0; i < n_cols; ++i) c.c[i] = cols[i];
    const int n_img = B * (n_cols + 1);
    const int xmaps = nrow < n_img ? nrow : n_img, ymaps = (n_img + xmaps - 1) / xmaps;
    const int nrow_bytes = Ws * 3;
    // (+ 3: a row that starts inside a dword ends one dword later)
    const dim3 g((unsigned)(((nrow_bytes + 3 + 3) / 4 + 255) / 256), (unsigned)Hs, (unsigned)F);
    hipLaunchKernelGGL(vis_sheet_kernel, g, dim3(256), 0, s, c, n_cols, n_img, H, W, tile, nrow_bytes, Ws, padding, xmaps, ymaps, sheet);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

}  // namespace nope
