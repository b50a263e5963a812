// Small data-movement kernels around the U-Net: layout changes at the NCHW API boundary,
// one-time weight repacking, and the tiny f32 linears of the pose embedding path.
#include "nope_common.h"

namespace nope {

namespace {

constexpr int NT = 256;

// Store element i of a packed weight tensor whose rows hold Cin values along K.  For NOPE_BF16X3 a row is 4 Cin bytes of
// 32-byte groups [hi x 8 | lo x 8] bf16, hi = rn(v), lo = rn(v - hi): channel c of a row sits in group c / 8 (Tile<f32s_t>,
// conv_gemm_common.h).  Cin % 8 == 0 (checked by the launcher).
template <class T> __device__ __forceinline__ void st_w(T* out, size_t i, int Cin, float v) { (void)Cin; Elt<T>::st(out + i, v); }
template <> __device__ __forceinline__ void st_w<f32s_t>(f32s_t* out, size_t i, int Cin, float v) {
    const size_t row = i / (size_t)Cin;
    const int c = (int)(i - row * (size_t)Cin);
    bf16_t* o = reinterpret_cast<bf16_t*>(out) + row * 2 * (size_t)Cin + (size_t)(c >> 3) * 16 + (c & 7);
    const bf16_t hi = f32_to_bf16(v);
    o[0] = hi;
    o[8] = f32_to_bf16(v - bf16_to_f32(hi));
}

// (n, C, HW) f32 NCHW -> [n][HW][C] T.  C is small (8 latent channels) at this boundary.
// (Csrc < C: the source has fewer channels; channels Csrc .. C-1 of the output are zeros -- inputs padded to a whole 16-byte vector)
template <class T>
__global__ __launch_bounds__(NT) void nchw_to_nhwc_kernel(const float* __restrict__ x, T* __restrict__ y, int C, int HW, size_t total, int Csrc) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
        const int c = (int)(i % C);
        const size_t t = i / C;
        const int p = (int)(t % HW);
        const size_t b = t / HW;
        Elt<T>::st(y + i, c < Csrc ? x[(b * Csrc + c) * HW + p] : 0.f);
    }
}

template <class T>
__global__ __launch_bounds__(NT) void nhwc_to_nchw_kernel(const T* __restrict__ x, float* __restrict__ y, int C, int HW, size_t total) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
        const int p = (int)(i % HW);
        const size_t t = i / HW;
        const int c = (int)(t % C);
        const size_t b = t / C;
        y[i] = Elt<T>::ld(x + (b * HW + p) * C + c);
    }
}

// torch Conv2d weight [Cout][Cin_t][kh][kw] f32 -> packed [Cout][tap][Cin] T.
//   PLAIN / UP2: Cin_t = Cin, tap = kh*3 + kw (or the single 1x1 tap).
//   DOWN2: the conv is 1x1 over the space-to-depth tensor whose channel index is
//          c*4 + p1*2 + p2 (einops "b (c p1 p2) h w", model_utils.py:170); tap = p1*2 + p2.
template <class T>
__global__ __launch_bounds__(NT) void pack_conv_w_kernel(const float* __restrict__ w, T* __restrict__ out, int Cin, int ntaps, int mode,
                                                         size_t total, const float* __restrict__ cin_scale,
                                                         const float* __restrict__ cout_scale, int Csrc) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
        const int c = (int)(i % Cin);
        const size_t t = i / Cin;
        const int tap = (int)(t % ntaps);
        const size_t co = t / ntaps;
        size_t src;
        if (mode == NOPE_CONV_DOWN2) src = co * ((size_t)Csrc * 4) + (size_t)c * 4 + tap;
        else src = (co * Csrc + c) * ntaps + tap;
        float v = c < Csrc ? w[src] : 0.f;         // (Csrc < Cin: zero weights for the channels the input was padded with)
        if (cin_scale) v *= cin_scale[c];      // per-input-channel scale (PreNorm gamma)
        if (cout_scale) v *= cout_scale[co];   // per-output-channel scale (folded eval-mode BatchNorm)
        st_w<T>(out, i, Cin, v);
    }
}

// ---- NOPE_F16X2 weight layout (Tile<f16x2_t>, conv_gemm_common.h): rows of Cin channels in chunks of 32 = 128 bytes = eight 16-byte slots:
// slots 0..3 the f16 hi parts of the chunk's 32 channels (8 per slot); slot 4 + h the 16 e4m3 bytes of w * 2^sw over "channel set" h =
// channels 8 h .. 8 h + 7 and 16 + 8 h .. 16 + 8 h + 7 (what the lanes of half h hold for the two f16 MFMAs), slot 6 + h those of
// (w - hi) * 2^(sw + 11).  sw is the layer's power-of-two pre-scale, the largest that keeps max |w| * 2^sw below 256 (the format reaches
// 448); |w - hi| <= 2^-11 max |w|, so the second operand cannot overflow either.  Three launches: the f32 rows in GEMM order into the
// destination (pack_conv_w_kernel<float> and its phase-conv siblings: every conv mode, same row order as every other pack), max |w| of
// those rows into the tail of the buffer (bits of a non-negative float order like unsigned integers), then the rows are encoded IN PLACE
// -- a chunk is 128 bytes before and after, one thread owns it; the first thread also writes the E8M0 scale byte the conv kernel hands to
// the MFMA: 127 - 9 - sw (nope_common.h).
__global__ __launch_bounds__(NT) void absmax_bits_kernel(const float* __restrict__ w, size_t n, unsigned* __restrict__ out) {
    unsigned m = 0;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
        const float v = fabsf(w[i]);
        const unsigned b = __builtin_bit_cast(unsigned, v);
        if (v == v && b > m) m = b;                    // (a NaN weight does not decide the scale)
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const unsigned t = __shfl_xor(m, o, 64); m = t > m ? t : m; }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}
// ... of an activation tensor (the NOPE_F16X2 range tracking of tensors no gn_apply produced): 16-byte loads, four in flight per thread
__global__ __launch_bounds__(NT) void absmax_f32_kernel(const float* __restrict__ x, size_t nvec, size_t n, unsigned* __restrict__ out) {
    float m = 0.f;
    const size_t stride = (size_t)gridDim.x * NT;
    size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = reinterpret_cast<const f32x4*>(x)[i + u * stride];
#pragma unroll
        for (int u = 0; u < 4; ++u) m = amax4(m, v[u][0], v[u][1], v[u][2], v[u][3]);
    }
    for (; i < nvec; i += stride) { const f32x4 v = reinterpret_cast<const f32x4*>(x)[i]; m = amax4(m, v[0], v[1], v[2], v[3]); }
    if (blockIdx.x == 0) for (size_t k = nvec * 4 + threadIdx.x; k < n; k += NT) m = __builtin_fmaxf(m, __builtin_fabsf(x[k]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = __builtin_fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0 && m > 0.f) amax_publish(out, m, blockIdx.x * (NT / 64) + (threadIdx.x >> 6));
}
// compact[i] = max over the kX2Spread lines of range slot i, which are zeroed for the next round (one 64-thread block per slot)
__global__ __launch_bounds__(64) void amax_reduce_kernel(unsigned* __restrict__ slots, unsigned* __restrict__ compact) {
    unsigned* p = slots + (size_t)blockIdx.x * kX2SlotWords + (threadIdx.x & (kX2Spread - 1)) * 32;
    unsigned m = 0;
    if (threadIdx.x < kX2Spread) { m = *p; *p = 0u; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const unsigned t = __shfl_xor(m, o, 64); m = t > m ? t : m; }
    if (threadIdx.x == 0) compact[blockIdx.x] = m;
}
// The verdict of one forward (NOPE_F16X2 range tracking; one block, enqueued behind the forward's last kernel): fold every range slot (and
// zero it for the next forward), take each layer's largest input maximum through `tab` -- [layer] = {t, slot, slot, slot, slot}, slot -1 =
// none; a layer that ran no two-pass launch in this forward has no slots -- and judge it against the layer's window (nope_common.h: kX2*):
// out = the e4m3(a') operand saturated (max |a| 2^-t > 1792), has no full-precision element (< 2^-4), or the maximum is not finite.
// status[0] = layers out in THIS forward (read by x2_poison_kernel), status[1] = forwards judged, status[2] / [3] = out / non-finite layers
// since create.  `host` (mapped host memory, polled without a synchronisation: nope_unet_x2_poll): [0] = status[1], [1] = status[0],
// [2] = status[2], [3] = status[3], [4 + l] = bits of the maximum that put layer l out of or near the end of its window (the host
// re-centres t from it and clears the word), [4 + n + l] = bits of layer l's maximum in this forward.
__global__ __launch_bounds__(NT) void x2_verdict_kernel(unsigned* __restrict__ slots, int nslots, const int* __restrict__ tab, int n_layers,
                                                        unsigned* __restrict__ status, volatile unsigned* __restrict__ host) {
    __shared__ unsigned compact[512];
    __shared__ unsigned n_out, n_inf;
    if (threadIdx.x == 0) { n_out = 0; n_inf = 0; }
    // fold: 32 lanes per slot, one line each (the loads of a pass are independent: a 100-slot forward folds in ~13 round trips, not 3 200)
    for (int i0 = 0; i0 < nslots && i0 < 512; i0 += NT / kX2Spread) {
        const int i = i0 + (int)(threadIdx.x / kX2Spread);
        unsigned m = 0;
        if (i < nslots && i < 512) {
            unsigned* p = slots + (size_t)i * kX2SlotWords + (threadIdx.x % kX2Spread) * 32;
            m = *p;
            if (m) *p = 0u;
        }
#pragma unroll
        for (int o = kX2Spread / 2; o >= 1; o >>= 1) { const unsigned v = __shfl_xor(m, o, 64); m = v > m ? v : m; }
        if (i < nslots && i < 512 && threadIdx.x % kX2Spread == 0) compact[i] = m;
    }
    __syncthreads();
    for (int l = threadIdx.x; l < n_layers; l += NT) {
        const int t = tab[l * 5];
        unsigned b = 0;
#pragma unroll
        for (int k = 1; k < 5; ++k) { const int sl = tab[l * 5 + k]; if (sl >= 0 && sl < 512 && compact[sl] > b) b = compact[sl]; }
        host[4 + n_layers + l] = b;
        if (!b) continue;
        const float amax = __builtin_bit_cast(float, b);
        if (b >= 0x7f800000u) { atomicAdd(&n_out, 1u); atomicAdd(&n_inf, 1u); host[4 + l] = b; continue; }      // inf (a NaN never enters a slot)
        const float v = ldexpf(amax, -t);
        const bool out = v > kX2AMaxFull || v < 0.0625f, uneasy = v > 1024.f || v < 1.f;
        if (out) atomicAdd(&n_out, 1u);
        if (out || uneasy) host[4 + l] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        status[0] = n_out; status[1] += 1u; status[2] += n_out; status[3] += n_inf;
        host[1] = n_out; host[2] = status[2]; host[3] = status[3];
        __threadfence_system();
        host[0] = status[1];
    }
}
// ... and what an out-of-range forward leaves in its output: NaNs, so that no caller reads inaccurate values for accurate ones (status[0] == 0:
// every block returns at once)
__global__ __launch_bounds__(NT) void x2_poison_kernel(unsigned* __restrict__ out, size_t nwords, unsigned pattern, const unsigned* __restrict__ status) {
    if (status[0] == 0u) return;
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < nwords; i += (size_t)gridDim.x * NT) out[i] = pattern;
}
__device__ __forceinline__ int x2_weight_shift(unsigned maxbits) {
    const int e = (int)(maxbits >> 23) - 127;          // floor(log2 max |w|) (normal numbers; zero / subnormal maxima give e = -127)
    const int sw = 7 - e;                              // max |w| * 2^sw in [128, 256)
    return sw < -64 ? -64 : (sw > 100 ? 100 : sw);
}
__global__ __launch_bounds__(NT) void encode_w_x2_kernel(unsigned char* __restrict__ buf, size_t chunks, int* __restrict__ tail) {
    const int sw = x2_weight_shift((unsigned)tail[2]);
    if (blockIdx.x == 0 && threadIdx.x == 0) { tail[0] = 127 - kX2ALoShift - sw; tail[1] = sw; tail[3] = 0; }
    const float s8 = ldexpf(1.0f, sw), sl8 = ldexpf(1.0f, sw + kX2WLoExtra);
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < chunks; i += (size_t)gridDim.x * NT) {
        unsigned char* chunk = buf + i * 128;
        float v[32];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const u32x4 t = reinterpret_cast<const u32x4*>(chunk)[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) { const unsigned u = t[e]; v[4 * q + e] = __builtin_bit_cast(float, u); }
        }
        union { unsigned char b[128]; u32x4 q[8]; } o;
#pragma unroll
        for (int cc = 0; cc < 32; ++cc) {
            const f16_t hi = f32_to_f16_sat(v[cc]);
            const float lo = v[cc] - (float)hi;
            reinterpret_cast<f16_t*>(o.b)[cc] = hi;                                            // slots 0..3
            const int h = (cc >> 3) & 1, pos = (cc >> 4) * 8 + (cc & 7);
            o.b[(4 + h) * 16 + pos] = (unsigned char)(cvt_pk_e4m3(v[cc] * s8, 0.f) & 0xffu);
            o.b[(6 + h) * 16 + pos] = (unsigned char)(cvt_pk_e4m3(lo * sl8, 0.f) & 0xffu);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) reinterpret_cast<u32x4*>(chunk)[q] = o.q[q];
    }
}

// out[r] = sum_k packed[r][k] (f32 sum of the values as the GEMM will see them)
template <class T>
__global__ __launch_bounds__(NT) void rowsum_kernel(const T* __restrict__ a, float* __restrict__ out, int rows, int K) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * NT + threadIdx.x) >> 6;
    if (wave >= rows) return;
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s += Elt<T>::ld(a + (size_t)wave * K + k);
    s = wave_sum(s);
    if (lane == 0) out[wave] = s;
}

// HardUpsample 3x3 weight [Cout][Cin][3][3] -> four phase sets [py*2+px][Cout][ty*2+tx][Cin]:
// tap (ty, tx) of phase (py, px) reads source pixel (y + ty + py - 1, x + tx + px - 1) and carries the sum of
// the 3x3 taps that land on it: rows {0} | {1,2} for py = 0, {0,1} | {2} for py = 1 (same for columns).
template <class T>
__global__ __launch_bounds__(NT) void pack_up2p_w_kernel(const float* __restrict__ w, T* __restrict__ out, int Cout, int Cin, size_t total) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
        const int c = (int)(i % Cin);
        size_t t = i / Cin;
        const int tap = (int)(t % 4); t /= 4;
        const int co = (int)(t % Cout);
        const int ph = (int)(t / Cout);
        const int py = ph >> 1, px = ph & 1, ty = tap >> 1, tx = tap & 1;
        const int y0 = py == 0 ? (ty == 0 ? 0 : 1) : (ty == 0 ? 0 : 2), y1 = py == 0 ? (ty == 0 ? 0 : 2) : (ty == 0 ? 1 : 2);
        const int x0 = px == 0 ? (tx == 0 ? 0 : 1) : (tx == 0 ? 0 : 2), x1 = px == 0 ? (tx == 0 ? 0 : 2) : (tx == 0 ? 1 : 2);
        float a = 0.f;
        for (int yy = y0; yy <= y1; ++yy)
            for (int xx = x0; xx <= x1; ++xx) a += w[(((size_t)co * Cin + c) * 3 + yy) * 3 + xx];
        st_w<T>(out, i, Cin, a);
    }
}

// Upsample = ConvTranspose2d(4, stride 2, pad 1), weight [Cin][Cout][4][4] (model_utils.py:119-126), as the same four phase
// sets: output pixel (2y + py, 2x + px) receives source pixel (y + ty + py - 1, x + tx + px - 1) through kernel element
// (3 - py - 2 ty, 3 - px - 2 tx) -- two source rows per output row, exactly the footprint of the nearest-x2 + 3x3 phases.
template <class T>
__global__ __launch_bounds__(NT) void pack_convT4_w_kernel(const float* __restrict__ w, T* __restrict__ out, int Cout, int Cin, size_t total) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < total; i += (size_t)gridDim.x * NT) {
        const int c = (int)(i % Cin);
        size_t t = i / Cin;
        const int tap = (int)(t % 4); t /= 4;
        const int co = (int)(t % Cout);
        const int ph = (int)(t / Cout);
        const int ky = 3 - (ph >> 1) - 2 * (tap >> 1), kx = 3 - (ph & 1) - 2 * (tap & 1);
        st_w<T>(out, i, Cin, w[(((size_t)c * Cout + co) * 4 + ky) * 4 + kx]);
    }
}

template <class T>
__global__ __launch_bounds__(NT) void cast_kernel(const float* __restrict__ in, T* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) Elt<T>::st(out + i, in[i]);
}

__global__ __launch_bounds__(NT) void silu_f32_kernel(const float* __restrict__ in, float* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) out[i] = silu_f<false>(in[i]);
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }

// out[m][n] = sum_k act(in[m][k]) * w[n][k] + bias[n]; one wave per output element row-chunk:
// each wave owns (m, 64 consecutive n?) -- no: K is the contiguous axis of both operands, so a
// wave owns one (m, n) pair group: lane l accumulates k = l, l+64, ... and the wave reduces.
__global__ __launch_bounds__(NT) void linear_naive_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ out, int M, int N, int K,
                                                          int act_in, int ldo) {
    const int lane = threadIdx.x & 63;
    const size_t wave = ((size_t)blockIdx.x * NT + threadIdx.x) >> 6;
    const size_t nwaves = ((size_t)gridDim.x * NT) >> 6;
    for (size_t o = wave; o < (size_t)M * N; o += nwaves) {
        const int m = (int)(o / N), n = (int)(o % N);
        float a = 0.f;
        for (int k = lane; k < K; k += 64) {
            float x = in[(size_t)m * K + k];
            if (act_in == 1) x = silu_f<false>(x);
            else if (act_in == 2) x = gelu_erf(x);
            a += x * w[(size_t)n * K + k];
        }
        a = wave_sum(a);
        if (lane == 0) out[(size_t)m * ldo + n] = a + (bias ? bias[n] : 0.f);
    }
}

// out[cls][co][ci] = sum of w[co][ci][ky][kx] over the taps a zero-padded 3x3 conv has inside the map at a pixel of border class
// cls = cy * 3 + cx (c* = 0: first row / column, tap 0 outside; 2: last, tap 2 outside; 1: all three inside), in tap order.
__global__ __launch_bounds__(NT) void pack_conv_classes_kernel(const float* __restrict__ w, float* __restrict__ out, size_t rows) {
    for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < 9 * rows; i += (size_t)gridDim.x * NT) {
        const int cls = (int)(i / rows), cy = cls / 3, cx = cls % 3;
        const float* t = w + (i % rows) * 9;
        float a = 0.f;
        for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx)
                if (!(cy == 0 && ky == 0) && !(cy == 2 && ky == 2) && !(cx == 0 && kx == 0) && !(cx == 2 && kx == 2)) a += t[ky * 3 + kx];
        out[i] = a;
    }
}

inline unsigned grid_for(size_t n) {
    size_t g = (n + NT - 1) / NT;
    if (g > 8192) g = 8192;
    if (g < 1) g = 1;
    return (unsigned)g;
}

}  // namespace

int launch_nchw_to_nhwc(int dt, const float* x, void* y, int n, int C, int HW, hipStream_t s, int C_src) {
    if (!x || !y || n <= 0 || C <= 0 || HW <= 0 || C_src < 0 || C_src > C) return NOPE_ERR_ARG;
    const size_t total = (size_t)n * C * HW;
    const int cs = C_src ? C_src : C;
    NOPE_DISPATCH_T(dt, T, hipLaunchKernelGGL((nchw_to_nhwc_kernel<T>), dim3(grid_for(total)), dim3(NT), 0, s, x, (T*)y, C, HW, total, cs));
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_nhwc_to_nchw_f32(int dt, const void* x, float* y, int n, int C, int HW, hipStream_t s) {
    if (!x || !y || n <= 0 || C <= 0 || HW <= 0) return NOPE_ERR_ARG;
    const size_t total = (size_t)n * C * HW;
    NOPE_DISPATCH_T(dt, T, hipLaunchKernelGGL((nhwc_to_nchw_kernel<T>), dim3(grid_for(total)), dim3(NT), 0, s, (const T*)x, y, C, HW, total));
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_pack_conv_w(int dt, const float* w, void* out, int Cout, int Cin, int ntaps, int mode, hipStream_t s, const float* cin_scale,
                       const float* cout_scale, int Cin_src) {
    if (!w || !out || Cout <= 0 || Cin <= 0 || ntaps <= 0 || Cin_src < 0 || Cin_src > Cin) return NOPE_ERR_ARG;
    if (Cin_src && Cin_src != Cin && (mode == NOPE_CONV_UP2P || cin_scale)) return NOPE_ERR_ARG;
    const int csrc = Cin_src ? Cin_src : Cin;
    if (dt == NOPE_F16X2) {                                             // the f16 + MX-fp8 tile's layout (tap-resident and per-tap ping-pong kernels)
        if (cin_scale || cout_scale || csrc != Cin) return NOPE_ERR_UNSUPPORTED;
        return launch_pack_conv_w_x2(w, out, Cout, Cin, s, ntaps, mode);
    }
    if (mode == NOPE_CONV_DOWN2 && ntaps != 4) return NOPE_ERR_ARG;
    if (dt == NOPE_BF16X3 && Cin % 8) return NOPE_ERR_UNSUPPORTED;      // (hi, lo) groups of 8 channels
    if (mode == NOPE_CONV_UP2P && ntaps == 16) {     // source is a ConvTranspose2d(4, 2, 1) weight
        if (cin_scale || cout_scale) return NOPE_ERR_ARG;
        const size_t tot = (size_t)4 * Cout * 4 * Cin;
        NOPE_DISPATCH_W(dt, T, hipLaunchKernelGGL((pack_convT4_w_kernel<T>), dim3(grid_for(tot)), dim3(NT), 0, s, w, (T*)out, Cout, Cin, tot));
        NOPE_CHECK_LAUNCH();
        return NOPE_OK;
    }
    if (mode == NOPE_CONV_UP2P) {
        if (ntaps != 4 || cin_scale || cout_scale) return NOPE_ERR_ARG;
        const size_t tot = (size_t)4 * Cout * 4 * Cin;
        NOPE_DISPATCH_W(dt, T, hipLaunchKernelGGL((pack_up2p_w_kernel<T>), dim3(grid_for(tot)), dim3(NT), 0, s, w, (T*)out, Cout, Cin, tot));
        NOPE_CHECK_LAUNCH();
        return NOPE_OK;
    }
    const size_t total = (size_t)Cout * ntaps * Cin;
    NOPE_DISPATCH_W(dt, T, hipLaunchKernelGGL((pack_conv_w_kernel<T>), dim3(grid_for(total)), dim3(NT), 0, s, w, (T*)out, Cin, ntaps, mode, total, cin_scale, cout_scale, csrc));
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_pack_conv_classes(const float* w, float* out, int Cout, int Cin, hipStream_t s) {
    if (!w || !out || Cout <= 0 || Cin <= 0) return NOPE_ERR_ARG;
    const size_t rows = (size_t)Cout * Cin;
    hipLaunchKernelGGL(pack_conv_classes_kernel, dim3(grid_for(9 * rows)), dim3(NT), 0, s, w, out, rows);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

static size_t x2_rows(int Cout, int ntaps, int mode) { return mode == NOPE_CONV_UP2P ? (size_t)16 * Cout : (size_t)Cout * ntaps; }      // (four phases x four taps)
size_t conv_w_x2_bytes(int Cout, int Cin, int ntaps, int mode) { return x2_rows(Cout, ntaps, mode) * Cin * 4 + kX2TailBytes; }

int launch_x2_verdict(unsigned* slots, int nslots, const int* tab, int n_layers, unsigned* status, unsigned* host_mapped, hipStream_t s) {
    if (!slots || !tab || !status || !host_mapped || nslots <= 0 || nslots > 512 || n_layers <= 0) return NOPE_ERR_ARG;
    hipLaunchKernelGGL(x2_verdict_kernel, dim3(1), dim3(NT), 0, s, slots, nslots, tab, n_layers, status, (volatile unsigned*)host_mapped);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}
int launch_x2_poison(void* out, size_t bytes, int out_dt, const unsigned* status, hipStream_t s) {
    if (!out || !status || bytes % 4) return NOPE_ERR_ARG;
    const unsigned pattern = out_dt == NOPE_F32 ? 0x7fc00000u : out_dt == NOPE_F16 ? 0x7e007e00u : 0x7fc07fc0u;      // quiet NaNs of the output type
    const size_t nwords = bytes / 4;
    size_t blocks = (nwords + (size_t)NT * 16 - 1) / ((size_t)NT * 16);
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(x2_poison_kernel, dim3((unsigned)blocks), dim3(NT), 0, s, (unsigned*)out, nwords, pattern, status);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_amax_reduce(unsigned* slots, int nslots, unsigned* compact, hipStream_t s) {
    if (!slots || !compact || nslots <= 0) return NOPE_ERR_ARG;
    hipLaunchKernelGGL(amax_reduce_kernel, dim3((unsigned)nslots), dim3(64), 0, s, slots, compact);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_absmax_f32(const float* x, size_t n, unsigned* out, hipStream_t s) {
    if (!x || !out) return NOPE_ERR_ARG;
    if (n == 0) return NOPE_OK;
    const size_t nvec = n / 4;
    size_t blocks = (nvec + (size_t)NT * 8 - 1) / ((size_t)NT * 8);
    blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
    hipLaunchKernelGGL(absmax_f32_kernel, dim3((unsigned)blocks), dim3(NT), 0, s, x, nvec, n, out);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_pack_conv_w_x2(const float* w, void* out, int Cout, int Cin, hipStream_t s, int ntaps, int mode) {
    if (!w || !out || Cout <= 0 || Cin <= 0) return NOPE_ERR_ARG;
    if (Cin % 32) return NOPE_ERR_UNSUPPORTED;                          // whole 32-channel chunks
    if (mode != NOPE_CONV_PLAIN && mode != NOPE_CONV_DOWN2 && mode != NOPE_CONV_UP2P) return NOPE_ERR_UNSUPPORTED;      // the modes of the ping-pong kernels
    if (const int e = launch_pack_conv_w(NOPE_F32, w, out, Cout, Cin, ntaps, mode, s)) return e;
    const size_t total = x2_rows(Cout, ntaps, mode) * Cin;
    int* tail = reinterpret_cast<int*>((unsigned char*)out + total * 4);
    if (hipMemsetAsync(tail, 0, kX2TailBytes, s) != hipSuccess) return NOPE_ERR_LAUNCH;
    hipLaunchKernelGGL(absmax_bits_kernel, dim3(grid_for(total)), dim3(NT), 0, s, (const float*)out, total, reinterpret_cast<unsigned*>(tail) + 2);
    NOPE_CHECK_LAUNCH();
    hipLaunchKernelGGL(encode_w_x2_kernel, dim3(grid_for(total / 32)), dim3(NT), 0, s, (unsigned char*)out, total / 32, tail);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

// (NOPE_BF16X3: a packed row of K channels is 2 K bf16 values, hi and lo parts: their plain sum is the row sum the MFMAs see)
int launch_rowsum(int dt, const void* packed, float* out, int rows, int K, hipStream_t s) {
    if (!packed || !out || rows <= 0 || K <= 0) return NOPE_ERR_ARG;
    const unsigned blocks = (unsigned)((rows + 3) / 4);
    if (dt == NOPE_BF16X3) { dt = NOPE_BF16; K *= 2; }
    NOPE_DISPATCH_T(dt, T, hipLaunchKernelGGL((rowsum_kernel<T>), dim3(blocks), dim3(NT), 0, s, (const T*)packed, out, rows, K));
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_cast(int dt, const float* in, void* out, size_t n, hipStream_t s) {
    if (!in || !out) return NOPE_ERR_ARG;
    if (n == 0) return NOPE_OK;
    NOPE_DISPATCH_T(dt, T, hipLaunchKernelGGL((cast_kernel<T>), dim3(grid_for(n)), dim3(NT), 0, s, in, (T*)out, n));
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

// "posEncoding" pose embedding, src/model/utils.py:36-51 with dim = classes / pose_dim: out[b, i*half + j] = sin(pose[b,i] * f_j),
// out[b, classes/2 + i*half + j] = cos(pose[b,i] * f_j), f_j = exp(-j * ln(1e4) / (half - 1)) evaluated in f32 as torch does.
__global__ __launch_bounds__(NT) void pos_emb_kernel(const float* __restrict__ pose, float* __restrict__ out, int n, int pose_dim, int half) {
    const int per = pose_dim * half;
    const size_t total = (size_t)n * per;
    const float step = logf(10000.0f) / (float)(half - 1);
    for (size_t idx = (size_t)blockIdx.x * NT + threadIdx.x; idx < total; idx += (size_t)gridDim.x * NT) {
        const int b = (int)(idx / per), r = (int)(idx - (size_t)b * per);
        const int i = r / half, j = r - i * half;
        const float a = pose[(size_t)b * pose_dim + i] * expf((float)j * -step);
        out[(size_t)b * 2 * per + r] = sinf(a);
        out[(size_t)b * 2 * per + per + r] = cosf(a);
    }
}

int launch_pos_emb(const float* pose, float* out, int n, int pose_dim, int classes, hipStream_t s) {
    if (!pose || !out || n <= 0 || pose_dim <= 0 || classes % (2 * pose_dim) || classes / (2 * pose_dim) < 2) return NOPE_ERR_ARG;
    const int half = classes / (2 * pose_dim);
    hipLaunchKernelGGL(pos_emb_kernel, dim3(grid_for((size_t)n * pose_dim * half)), dim3(NT), 0, s, pose, out, n, pose_dim, half);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

// Perspective warp of the dataset-side crop (src/poses/utils.py:204-272: cv2.warpPerspective(img, M, (S, S)), bilinear, constant
// zero border) fused with the image transform of the loader (dataloader/shapeNet.py:64-69: /255, *2-1, HWC -> CHW):
//   dst[c, y, x] = scale * bilinear(src, Minv * (x, y, 1)) + shift,   src (Hs, Ws, C) uint8 or f32, dst (C, Hd, Wd) f32.
// Pixel centres sit on integer coordinates, as in OpenCV; samples outside the source contribute zeros tap by tap.
struct Mat3 { float m[9]; };
// ROUND_U8: the interpolated value is rounded to the nearest integer and clamped to [0, 255] before scale / shift, as a uint8
// destination image does (cv2.warpPerspective on uint8 frames, then ToTensor's / 255): outputs land on the reference loader's
// k / 255 grid.  OpenCV's own fixed-point interpolation weights (1/32 pixel) are not restated: parity unpinned (cv2 is absent).
// The arithmetic of one output pixel, shared by warp_perspective_kernel and crop_frames_kernel (same f32 operations in the same order):
// warp_taps = the source position of output pixel (x, y) under the inverse map m, its four taps, their weights and which of them lie
// inside the source (none when w == 0); warp_interp = the weighted sum of the taps a fetch(t) hands out, rounding / clamp, scale and shift.
// Which products are fused is spelled out (fmaf) and nothing else may be (contract(off)): left to the compiler, the choice differed from one
// kernel to the next (its vectoriser pairs the three projections differently), and two kernels that agree only to an ulp in the source
// position disagree by a grey level after round_u8.  The spelling is what warp_perspective_kernel has always computed on gfx950.
struct WarpTaps { int x0, y0; float wt[4]; bool in[4]; };
__device__ __forceinline__ WarpTaps warp_taps(const float* __restrict__ m, int x, int y, int Hs, int Ws) {
#pragma clang fp contract(off)
    WarpTaps tp;
    const float xf = (float)x, yf = (float)y;
    const float w = fmaf(m[7], yf, m[6] * xf) + m[8];
    const float sx = ((m[0] * xf + m[1] * yf) + m[2]) / w;
    const float sy = (fmaf(m[3], xf, m[4] * yf) + m[5]) / w;
    const float fx = floorf(sx), fy = floorf(sy);
    tp.x0 = (int)fx, tp.y0 = (int)fy;
    const float ax = sx - fx, ay = sy - fy;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int xx = tp.x0 + (t & 1), yy = tp.y0 + (t >> 1);
        tp.wt[t] = ((t & 1) ? ax : 1.f - ax) * ((t >> 1) ? ay : 1.f - ay);
        tp.in[t] = xx >= 0 && xx < Ws && yy >= 0 && yy < Hs && w != 0.f;
    }
    return tp;
}
template <bool ROUND_U8, class Fetch>
__device__ __forceinline__ float warp_interp(const WarpTaps& tp, float scale, float shift, Fetch fetch) {
#pragma clang fp contract(off)
    float v = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (tp.in[t]) v = fmaf(tp.wt[t], fetch(t), v);
    if (ROUND_U8) v = fminf(fmaxf(rintf(v), 0.f), 255.f);
    return fmaf(scale, v, shift);
}

template <class TIN, bool ROUND_U8>
__global__ __launch_bounds__(NT) void warp_perspective_kernel(const TIN* __restrict__ src, int Hs, int Ws, int C, Mat3 inv, float* __restrict__ dst,
                                                              int Hd, int Wd, float scale, float shift) {
    const int total = Hd * Wd;
    for (int i = blockIdx.x * NT + threadIdx.x; i < total; i += gridDim.x * NT) {
        const int y = i / Wd, x = i - y * Wd;
        const WarpTaps tp = warp_taps(inv.m, x, y, Hs, Ws);
        for (int c = 0; c < C; ++c)
            dst[(size_t)c * total + i] = warp_interp<ROUND_U8>(tp, scale, shift, [&](int t) {
                return (float)src[((size_t)(tp.y0 + (t >> 1)) * Ws + tp.x0 + (t & 1)) * C + c]; });
    }
}

int launch_warp_perspective(const void* src, int src_u8, int Hs, int Ws, int C, const float* minv9, float* dst, int Hd, int Wd, float scale,
                            float shift, hipStream_t s) {
    if (!src || !minv9 || !dst || Hs <= 0 || Ws <= 0 || C <= 0 || Hd <= 0 || Wd <= 0) return NOPE_ERR_ARG;
    Mat3 m;
    for (int i = 0; i < 9; ++i) m.m[i] = minv9[i];
    const dim3 grid(grid_for((size_t)Hd * Wd));
    if (src_u8 == 2) hipLaunchKernelGGL((warp_perspective_kernel<unsigned char, true>), grid, dim3(NT), 0, s, (const unsigned char*)src, Hs, Ws, C, m, dst, Hd, Wd, scale, shift);
    else if (src_u8) hipLaunchKernelGGL((warp_perspective_kernel<unsigned char, false>), grid, dim3(NT), 0, s, (const unsigned char*)src, Hs, Ws, C, m, dst, Hd, Wd, scale, shift);
    else hipLaunchKernelGGL((warp_perspective_kernel<float, false>), grid, dim3(NT), 0, s, (const float*)src, Hs, Ws, C, m, dst, Hd, Wd, scale, shift);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

// The loader's whole chain for a stack of decoded frames in one pass (dataloader/shapeNet.py:184-210,167-182,64-69; bop.py:212-232): paste on
// black through the alpha channel, crop_frame's warp, ToTensor, * 2 - 1.  frames (F, Hs, Ws, CS) uint8, CS = 3 (RGB) or 4 (RGBA); minv (F, 9): one
// inverse map per frame, on the device; dst (F, 3, Hd, Wd).  One thread per output pixel, blockIdx.y walks the frames.  The reference pastes first
// and warps the pasted image, so every tap is composited before it is weighted: round(c * a / 255) in integers, PIL's paste onto black (its
// MULDIV255; c * a / 255 never ends in .5, 255 being odd).  An RGBA tap is one 32-bit load serving the three colour planes.
template <int CS, bool ROUND_U8>
__global__ __launch_bounds__(NT) void crop_frames_kernel(const unsigned char* __restrict__ frames, int Hs, int Ws, const float* __restrict__ minv,
                                                         float* __restrict__ dst, int F, int Hd, int Wd, float scale, float shift) {
    const int total = Hd * Wd;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int y = i / Wd, x = i - y * Wd;
    for (int f = blockIdx.y; f < F; f += gridDim.y) {
        const unsigned char* __restrict__ src = frames + (size_t)f * Hs * Ws * CS;
        float* __restrict__ out = dst + (size_t)f * 3 * total + i;
        const WarpTaps tp = warp_taps(minv + (size_t)f * 9, x, y, Hs, Ws);
        if (CS == 4) {
            unsigned px[4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                px[t] = tp.in[t] ? ((const unsigned*)src)[(size_t)(tp.y0 + (t >> 1)) * Ws + tp.x0 + (t & 1)] : 0u;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                out[(size_t)c * total] = warp_interp<ROUND_U8>(tp, scale, shift, [&](int t) {
                    return (float)((2u * ((px[t] >> (8 * c)) & 255u) * (px[t] >> 24) + 255u) / 510u); });
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                out[(size_t)c * total] = warp_interp<ROUND_U8>(tp, scale, shift, [&](int t) {
                    return (float)src[((size_t)(tp.y0 + (t >> 1)) * Ws + tp.x0 + (t & 1)) * 3 + c]; });
        }
    }
}

int launch_crop_frames(const void* frames, int F, int Hs, int Ws, int Cs, const float* minv, float* dst, int Hd, int Wd, float scale, float shift,
                       int round_u8, hipStream_t s) {
    if (!frames || !minv || !dst || F <= 0 || Hs <= 0 || Ws <= 0 || Hd <= 0 || Wd <= 0) return NOPE_ERR_ARG;
    if (Cs != 3 && Cs != 4) return NOPE_ERR_UNSUPPORTED;
    if (((uintptr_t)frames & 3) && Cs == 4) return NOPE_ERR_ARG;       // the 32-bit tap loads
    const size_t total = (size_t)Hd * Wd;
    if (total > (size_t)0x7fffffff - NT) return NOPE_ERR_ARG;
    const dim3 grid((unsigned)((total + NT - 1) / NT), (unsigned)(F < 65535 ? F : 65535));
    const unsigned char* fr = (const unsigned char*)frames;
#define NOPE_CROP_LAUNCH(CS, R) hipLaunchKernelGGL((crop_frames_kernel<CS, R>), grid, dim3(NT), 0, s, fr, Hs, Ws, minv, dst, F, Hd, Wd, scale, shift)
    if (Cs == 4) { if (round_u8) NOPE_CROP_LAUNCH(4, true); else NOPE_CROP_LAUNCH(4, false); }
    else { if (round_u8) NOPE_CROP_LAUNCH(3, true); else NOPE_CROP_LAUNCH(3, false); }
#undef NOPE_CROP_LAUNCH
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_silu_f32(const float* in, float* out, size_t n, hipStream_t s) {
    if (!in || !out) return NOPE_ERR_ARG;
    if (n == 0) return NOPE_OK;
    hipLaunchKernelGGL(silu_f32_kernel, dim3(grid_for(n)), dim3(NT), 0, s, in, out, n);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

int launch_linear_naive(const float* in, const float* w, const float* bias, float* out, int M, int N, int K, int act_in, int ldo,
                        hipStream_t s) {
    if (!in || !w || !out || M <= 0 || N <= 0 || K <= 0) return NOPE_ERR_ARG;
    const size_t outs = (size_t)M * N;
    size_t blocks = (outs + 3) / 4;   // 4 waves per block, one output per wave per iteration
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(linear_naive_kernel, dim3((unsigned)blocks), dim3(NT), 0, s, in, w, bias, out, M, N, K, act_in, ldo);
    NOPE_CHECK_LAUNCH();
    return NOPE_OK;
}

}  // namespace nope
