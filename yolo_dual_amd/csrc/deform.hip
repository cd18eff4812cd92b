// Deformable convolution (torchvision.ops.deform_conv2d: DCNv1 without a mask, DCNv2 with one) for gfx950, NHWC.
// The op is evaluated in column form: a gather kernel writes the modulated bilinear samples of every (output pixel, kernel point,
// channel) into col[pix][k*C + c] (k-major, so the KRSC weight [Cout][kh*kw][C] IS the weight of a 1x1 GEMM over col), the existing
// implicit-GEMM entry points do the matrix products, and one backward kernel turns d col into grad_input, grad_offset and grad_mask.
// Sampling (torchvision's documented semantics): for output (ho, wo), kernel point k = i*kw + j and offset group g
//     y = ho*sh - ph + i*dh + offset[2*(g*K + k)],   x = wo*sw - pw + j*dw + offset[2*(g*K + k) + 1]      ((dy, dx) interleaved)
//     value = bilinear over the four corners (h0, w0) .. (h0+1, w0+1), h0 = floor(y), w0 = floor(x); a corner outside the image
//             counts as 0; times mask[g*K + k] when a mask is given.
// Border convention: validity is tested PER CORNER only.  The value equals the one with torchvision's outer "y <= -1 || y >= H ..."
// test everywhere; the coordinate gradient differs only for a point exactly on -1 (e.g. DCNv2's zero-initialised offsets put every
// border tap there): it keeps the one-sided slope towards pixel 0 (corner 0 is valid, its weight derivative is not zero).
// grad_input: f32 atomics in arrival order (not bitwise deterministic, like the DCNv3 op).  grad_offset / grad_mask: one owner
// lane segment per (pixel, kernel point, group), channel sums by DPP / lane shuffles, plain stores.
#include "common.h"
#include <stdlib.h>

static int g_deform_win = 1;      // ydl_debug_set key 20: 1 (default) LDS-window backward where it applies, 0 per-corner atomics
void ydl_deform_debug_set(int key, int val) { if (key == 20) g_deform_win = val; }

struct DfmArgs {
    const void* x; const void* off; const void* msk; void* col;
    const void* dcol; float* gin; float* goff; float* gmsk;
    int ldx, ldo, ldm, ldc, sig, ones;
    int N, H, W, C, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, G;
};

// VEC consecutive channels as floats (one 16-byte load on the vector path)
template <typename T, int VEC> __device__ __forceinline__ void ld_vec(const T* p, float* f) {
    if constexpr (VEC == ET<T>::V) unpack16<T>(*(const uint4*)p, f);
    else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) f[e] = ET<T>::ld(p + e);
    }
}
template <typename T, int VEC> __device__ __forceinline__ void st_vec(T* p, const float* f) {
    if constexpr (VEC == ET<T>::V) *(uint4*)p = pack16<T>(f);
    else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) ET<T>::st(p + e, f[e]);
    }
}

// sampling geometry of one (pixel, kernel point, group): corner weights, corner validity and the raw / applied mask
struct Tap {
    int h0, w0;
    float lh, lw, m, mraw;
    bool v00, v01, v10, v11;
};
template <typename T>
__device__ __forceinline__ Tap make_tap(const DfmArgs& a, long long pix, int ho, int wo, int i, int j, int g) {
    const int K = a.kh * a.kw, k = i * a.kw + j;
    const T* off = (const T*)a.off + pix * a.ldo + 2 * (g * K + k);
    const float y = (float)(ho * a.sh - a.ph + i * a.dh) + ET<T>::ld(off);
    const float x = (float)(wo * a.sw - a.pw + j * a.dw) + ET<T>::ld(off + 1);
    Tap t;
    const float fy = floorf(y), fx = floorf(x);
    t.h0 = (int)fy; t.w0 = (int)fx;
    t.lh = y - fy; t.lw = x - fx;
    // |position| beyond the int range: every corner is outside (the floats compare safely, the ints may not)
    const bool sane = fabsf(y) < 1e8f && fabsf(x) < 1e8f;
    const bool r0 = sane && t.h0 >= 0 && t.h0 < a.H, r1 = sane && t.h0 + 1 >= 0 && t.h0 + 1 < a.H;
    const bool c0 = sane && t.w0 >= 0 && t.w0 < a.W, c1 = sane && t.w0 + 1 >= 0 && t.w0 + 1 < a.W;
    t.v00 = r0 && c0; t.v01 = r0 && c1; t.v10 = r1 && c0; t.v11 = r1 && c1;
    t.mraw = 1.f; t.m = 1.f;
    if (a.msk) {
        t.mraw = ET<T>::ld((const T*)a.msk + pix * a.ldm + g * K + k);
        t.m = a.sig ? 1.f / (1.f + __expf(-t.mraw)) : t.mraw;
    }
    return t;
}

// ------------------------------------------------------------------------------------------------------
// forward gather: one thread per (pixel, kernel point, VEC-channel chunk), chunks fastest (coalesced col rows)
// ------------------------------------------------------------------------------------------------------
template <typename T, int VEC>
__global__ __launch_bounds__(256) void deform_gather_kernel(const DfmArgs a) {
    const int K = a.kh * a.kw, nch = a.C / VEC, Cg = a.C / a.G;
    const long long npix = (long long)a.N * a.Ho * a.Wo;
    const long long total = npix * K * nch;
    const T* x = (const T*)a.x;
    T* col = (T*)a.col;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int ch = (int)(idx % nch);
        const long long t = idx / nch;
        const int k = (int)(t % K);
        const long long pix = t / K;
        const int wo = (int)(pix % a.Wo), ho = (int)((pix / a.Wo) % a.Ho), n = (int)(pix / ((long long)a.Wo * a.Ho));
        const int c = ch * VEC;
        const Tap tp = make_tap<T>(a, pix, ho, wo, k / a.kw, k % a.kw, c / Cg);
        const float hh = 1.f - tp.lh, hw = 1.f - tp.lw;
        float acc[VEC], v[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
        const T* xb = x + (long long)n * a.H * a.W * a.ldx + c;
#define DFM_CORNER(valid, hh_, ww_, wt)                                                              \
        if (valid) {                                                                                 \
            ld_vec<T, VEC>(xb + ((long long)(hh_) * a.W + (ww_)) * a.ldx, v);                        \
            _Pragma("unroll") for (int e = 0; e < VEC; ++e) acc[e] += (wt) * v[e];                   \
        }
        DFM_CORNER(tp.v00, tp.h0, tp.w0, hh * hw)
        DFM_CORNER(tp.v01, tp.h0, tp.w0 + 1, hh * tp.lw)
        DFM_CORNER(tp.v10, tp.h0 + 1, tp.w0, tp.lh * hw)
        DFM_CORNER(tp.v11, tp.h0 + 1, tp.w0 + 1, tp.lh * tp.lw)
#undef DFM_CORNER
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] *= tp.m;
        T* row = col + pix * a.ldc;
        st_vec<T, VEC>(row + k * a.C + c, acc);
        if (k == 0 && ch == 0)                      // the tail of the row: the bias column (ones) and the zero padding
            for (int q = K * a.C; q < a.ldc; ++q) ET<T>::st(row + q, (a.ones && q == K * a.C) ? 1.f : 0.f);
    }
}

// ------------------------------------------------------------------------------------------------------
// backward pieces
// ------------------------------------------------------------------------------------------------------
// sum over an aligned power-of-two lane segment (seg <= 64); valid in every lane of the segment.  Up to 16 lanes the butterfly is
// DPP inside a row (quad_perm xor 1 / xor 2, half-row mirror, row mirror); the 32- and 64-lane steps cross rows with a shuffle.
__device__ __forceinline__ float seg_reduce(float v, int seg) {
    if (seg >= 2) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
    if (seg >= 4) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
    if (seg >= 8) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, false));   // row_half_mirror
    if (seg >= 16) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, false));  // row_mirror
    if (seg >= 32) v += __shfl_xor(v, 16, 64);
    if (seg >= 64) v += __shfl_xor(v, 32, 64);
    return v;
}

// one VEC-channel chunk of one tap: partial (d mask, d y, d x) sums and the four corner contributions d col * m * w_corner,
// handed to `scatter(corner, h, w, VEC values)`
template <typename T, int VEC, typename S>
__device__ __forceinline__ void tap_chunk_bwd(const DfmArgs& a, const Tap& tp, int n, long long pix, int k, int c, float& sm, float& sy,
                                              float& sx, S&& scatter) {
    float g[VEC], v00[VEC], v01[VEC], v10[VEC], v11[VEC];
    ld_vec<T, VEC>((const T*)a.dcol + pix * a.ldc + k * a.C + c, g);
    const T* xb = (const T*)a.x + (long long)n * a.H * a.W * a.ldx + c;
#pragma unroll
    for (int e = 0; e < VEC; ++e) { v00[e] = 0.f; v01[e] = 0.f; v10[e] = 0.f; v11[e] = 0.f; }
    if (tp.v00) ld_vec<T, VEC>(xb + ((long long)tp.h0 * a.W + tp.w0) * a.ldx, v00);
    if (tp.v01) ld_vec<T, VEC>(xb + ((long long)tp.h0 * a.W + tp.w0 + 1) * a.ldx, v01);
    if (tp.v10) ld_vec<T, VEC>(xb + ((long long)(tp.h0 + 1) * a.W + tp.w0) * a.ldx, v10);
    if (tp.v11) ld_vec<T, VEC>(xb + ((long long)(tp.h0 + 1) * a.W + tp.w0 + 1) * a.ldx, v11);
    const float hh = 1.f - tp.lh, hw = 1.f - tp.lw;
    const float w00 = hh * hw, w01 = hh * tp.lw, w10 = tp.lh * hw, w11 = tp.lh * tp.lw;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const float val = w00 * v00[e] + w01 * v01[e] + w10 * v10[e] + w11 * v11[e];
        sm += g[e] * val;
        sy += g[e] * (hw * (v10[e] - v00[e]) + tp.lw * (v11[e] - v01[e]));
        sx += g[e] * (hh * (v01[e] - v00[e]) + tp.lh * (v11[e] - v10[e]));
        g[e] *= tp.m;
    }
    if (a.gin) {
        float d[VEC];
#define DFM_SCAT(valid, q, hh_, ww_, wt)                                     \
        if (valid) {                                                         \
            _Pragma("unroll") for (int e = 0; e < VEC; ++e) d[e] = (wt) * g[e]; \
            scatter(q, hh_, ww_, d);                                         \
        }
        DFM_SCAT(tp.v00, 0, tp.h0, tp.w0, w00)
        DFM_SCAT(tp.v01, 1, tp.h0, tp.w0 + 1, w01)
        DFM_SCAT(tp.v10, 2, tp.h0 + 1, tp.w0, w10)
        DFM_SCAT(tp.v11, 3, tp.h0 + 1, tp.w0 + 1, w11)
#undef DFM_SCAT
    }
}

// grad_offset / grad_mask of one tap from its channel sums (applied mask m, raw mask logit when the kernel applies the sigmoid)
__device__ __forceinline__ void tap_store(const DfmArgs& a, const Tap& tp, long long pix, int g, int k, float sm, float sy, float sx) {
    const int K = a.kh * a.kw;
    if (a.goff) {
        float* o = a.goff + pix * (2ll * a.G * K) + 2 * (g * K + k);
        o[0] = tp.m * sy;
        o[1] = tp.m * sx;
    }
    if (a.gmsk && a.msk) a.gmsk[pix * (long long)(a.G * K) + g * K + k] = a.sig ? sm * tp.m * (1.f - tp.m) : sm;
}

// generic backward (any kernel size / stride / padding / dilation / offset size): a lane segment of `seg` lanes per (pixel, kernel
// point, group) item, lanes over the group's VEC-channel chunks; grad_input by direct f32 atomics
template <typename T, int VEC>
__global__ __launch_bounds__(256) void deform_bwd_atomic_kernel(const DfmArgs a, int seg) {
    const int K = a.kh * a.kw, Cg = a.C / a.G, nchg = Cg / VEC;
    const long long npix = (long long)a.N * a.Ho * a.Wo;
    const long long items = npix * K * a.G;
    const int lane = threadIdx.x & 63, cl = lane % seg;
    const long long gl = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / seg;      // first item of this segment
    const long long step = ((long long)gridDim.x * blockDim.x) / seg;
    const long long rounds = (items + step - 1) / step;
    for (long long r = 0; r < rounds; ++r) {
        const long long it = gl + r * step;
        if (it >= items) break;                     // uniform over the segment
        const int g = (int)(it % a.G);
        const long long t = it / a.G;
        const int k = (int)(t % K);
        const long long pix = t / K;
        const int wo = (int)(pix % a.Wo), ho = (int)((pix / a.Wo) % a.Ho), n = (int)(pix / ((long long)a.Wo * a.Ho));
        const Tap tp = make_tap<T>(a, pix, ho, wo, k / a.kw, k % a.kw, g);
        float sm = 0.f, sy = 0.f, sx = 0.f;
        float* gib = a.gin ? a.gin + (long long)n * a.H * a.W * a.C : nullptr;
        for (int ch = cl; ch < nchg; ch += seg) {
            const int c = g * Cg + ch * VEC;
            tap_chunk_bwd<T, VEC>(a, tp, n, pix, k, c, sm, sy, sx, [&](int, int h, int w, const float* d) {
                float* p = gib + ((long long)h * a.W + w) * a.C + c;
#pragma unroll
                for (int e = 0; e < VEC; ++e) atomicAdd(p + e, d[e]);
            });
        }
        sm = seg_reduce(sm, seg); sy = seg_reduce(sy, seg); sx = seg_reduce(sx, seg);
        if (cl == 0) tap_store(a, tp, pix, g, k, sm, sy, sx);
    }
}

// LDS-window backward for 3x3, stride 1, dilation 1: a CTA owns an 8 x 8 tile of output pixels of one image and group and the
// (10 + 2R)^2 window of input cells their taps reach with |offset| < R px.  The group's channels are walked in slices of CS: per slice
// the window is cleared, every (pixel, tap, chunk) item adds its corner gradients into it with LDS atomics (corners outside the window:
// direct global atomics), and the window is flushed with one global atomic per (cell, channel) — neighbouring tiles' windows overlap.
// The per-tap channel sums of the slices accumulate in LDS (one owner segment per item and slice: plain adds) and are stored at the end.
#define DW_T 8
#define DW_R 2
#define DW_E (DW_T + 2 + 2 * DW_R)          // 14: window edge
#define DW_CELLS (DW_E * DW_E)
template <typename T, int VEC>
__global__ __launch_bounds__(256) void deform_bwd_window_kernel(const DfmArgs a, int CS, int tiles_w, int tiles_hw) {
    extern __shared__ float lds[];
    float* win = lds;                                // [DW_CELLS][CS]
    float* red = lds + DW_CELLS * CS;                // [64 pixels][9 taps][3]
    const int Cg = a.C / a.G;
    int b = blockIdx.x;
    const int g = b % a.G; b /= a.G;
    const int tl = b % tiles_hw, n = b / tiles_hw;
    const int th = (tl / tiles_w) * DW_T, tw = (tl % tiles_w) * DW_T;
    const int wh0 = th - a.ph - DW_R, ww0 = tw - a.pw - DW_R;           // input cell of window cell (0, 0)
    const int nch = CS / VEC;                        // lanes per item (power of two, <= 16)
    const int items = DW_T * DW_T * 9;
    for (int q = threadIdx.x; q < items * 3; q += blockDim.x) red[q] = 0.f;
    float* gib = a.gin + (long long)n * a.H * a.W * a.C;
    for (int cs0 = 0; cs0 < Cg; cs0 += CS) {
        for (int q = threadIdx.x; q < DW_CELLS * CS; q += blockDim.x) win[q] = 0.f;
        __syncthreads();
        const int cbase = g * Cg + cs0;
        for (int L = threadIdx.x; L < items * nch; L += blockDim.x) {      // items*nch is a multiple of 64: segments never split
            const int it = L / nch, cl = L % nch;
            const int pl = it / 9, k = it % 9;
            const int ho = th + pl / DW_T, wo = tw + pl % DW_T;
            const bool live = ho < a.Ho && wo < a.Wo;                       // uniform over the segment
            if (!live) continue;
            const long long pix = ((long long)n * a.Ho + ho) * a.Wo + wo;
            const Tap tp = make_tap<T>(a, pix, ho, wo, k / 3, k % 3, g);
            float sm = 0.f, sy = 0.f, sx = 0.f;
            const int cw = cl * VEC;
            tap_chunk_bwd<T, VEC>(a, tp, n, pix, k, cbase + cw, sm, sy, sx, [&](int, int h, int w, const float* d) {
                const int r = h - wh0, s = w - ww0;
                if (r >= 0 && r < DW_E && s >= 0 && s < DW_E) {
                    float* p = win + (r * DW_E + s) * CS + cw;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) atomicAdd(p + e, d[e]);
                } else {
                    float* p = gib + ((long long)h * a.W + w) * a.C + cbase + cw;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) atomicAdd(p + e, d[e]);
                }
            });
            sm = seg_reduce(sm, nch); sy = seg_reduce(sy, nch); sx = seg_reduce(sx, nch);
            if (cl == 0) { red[it * 3] += sm; red[it * 3 + 1] += sy; red[it * 3 + 2] += sx; }
        }
        __syncthreads();
        for (int q = threadIdx.x; q < DW_CELLS * CS; q += blockDim.x) {
            const int cell = q / CS, c = q % CS;
            const int h = wh0 + cell / DW_E, w = ww0 + cell % DW_E;
            const float v = win[q];
            if (v != 0.f && h >= 0 && h < a.H && w >= 0 && w < a.W) atomicAdd(gib + ((long long)h * a.W + w) * a.C + cbase + c, v);
        }
        __syncthreads();
    }
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
        const int pl = it / 9, k = it % 9;
        const int ho = th + pl / DW_T, wo = tw + pl % DW_T;
        if (ho >= a.Ho || wo >= a.Wo) continue;
        const long long pix = ((long long)n * a.Ho + ho) * a.Wo + wo;
        const Tap tp = make_tap<T>(a, pix, ho, wo, k / 3, k % 3, g);
        tap_store(a, tp, pix, g, k, red[it * 3], red[it * 3 + 1], red[it * 3 + 2]);
    }
}

// ------------------------------------------------------------------------------------------------------
// host entry points
// ------------------------------------------------------------------------------------------------------
static int dfm_check(const DfmArgs& a, int dtype) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "dtype must be YDL_F32 or YDL_BF16");
    YDL_CHECK(a.x && a.off, "input and offset are required");
    YDL_CHECK(a.N > 0 && a.H > 0 && a.W > 0 && a.C > 0 && a.Ho > 0 && a.Wo > 0, "empty shape");
    YDL_CHECK(a.kh > 0 && a.kw > 0 && a.sh > 0 && a.sw > 0 && a.dh > 0 && a.dw > 0 && a.ph >= 0 && a.pw >= 0, "bad kernel geometry");
    YDL_CHECK(a.Ho == (a.H + 2 * a.ph - (a.dh * (a.kh - 1) + 1)) / a.sh + 1 && a.Wo == (a.W + 2 * a.pw - (a.dw * (a.kw - 1) + 1)) / a.sw + 1,
              "Ho / Wo do not match the geometry");
    YDL_CHECK(a.G > 0 && a.C % a.G == 0, "offset groups must divide the channels");
    YDL_CHECK(a.ldx >= a.C && a.ldo >= 2 * a.G * a.kh * a.kw && (!a.msk || a.ldm >= a.G * a.kh * a.kw), "row strides too small");
    YDL_CHECK(a.ldc >= a.kh * a.kw * a.C + (a.ones ? 1 : 0), "col row stride too small");
    return 0;
}

// vector path: 16-byte chunks never straddle an offset group and every row start is 16-byte aligned
static bool dfm_vec(const DfmArgs& a, int dtype, const void* colp) {
    const int V = dtype == YDL_F32 ? 4 : 8;
    return (a.C / a.G) % V == 0 && a.ldx % V == 0 && a.ldc % V == 0 && aligned16(a.x) && aligned16(colp);
}

static int dfm_grid(long long total) {
    long long b = (total + 255) / 256;
    const long long cap = 256ll * 32;
    return (int)(b < 1 ? 1 : b > cap ? cap : b);
}

extern "C" int ydl_deform_gather(int dtype, const void* x, int ldx, const void* offset, int ldo, const void* mask, int ldm, int mask_sigmoid,
                                 void* col, int ldc, int ones_column, int N, int H, int W, int C, int Ho, int Wo, int kh, int kw,
                                 int sh, int sw, int ph, int pw, int dh, int dw, int G, void* stream) {
    DfmArgs a = {x, offset, mask, col, nullptr, nullptr, nullptr, nullptr, ldx, ldo, ldm, ldc, mask_sigmoid, ones_column,
                 N, H, W, C, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, G};
    if (int rc = dfm_check(a, dtype)) return rc;
    YDL_CHECK(col, "col is required");
    hipStream_t st = (hipStream_t)stream;
    const bool vec = dfm_vec(a, dtype, col);
    const int V = vec ? (dtype == YDL_F32 ? 4 : 8) : 1;
    const int grid = dfm_grid((long long)N * Ho * Wo * kh * kw * (C / V));
    if (dtype == YDL_F32) {
        if (vec) { deform_gather_kernel<float, 4><<<grid, 256, 0, st>>>(a); ydl_note_kernel(5, "deform_gather_kernel<f32,4>"); }
        else { deform_gather_kernel<float, 1><<<grid, 256, 0, st>>>(a); ydl_note_kernel(5, "deform_gather_kernel<f32,1>"); }
    } else {
        if (vec) { deform_gather_kernel<bf16_t, 8><<<grid, 256, 0, st>>>(a); ydl_note_kernel(5, "deform_gather_kernel<bf16,8>"); }
        else { deform_gather_kernel<bf16_t, 1><<<grid, 256, 0, st>>>(a); ydl_note_kernel(5, "deform_gather_kernel<bf16,1>"); }
    }
    YDL_LAUNCH_CHECK();
    return 0;
}

template <typename T, int VEC>
static void dfm_bwd_launch(const DfmArgs& a, bool window, int CS, hipStream_t st, const char* wname, const char* aname) {
    if (window) {
        const int tiles_w = (a.Wo + DW_T - 1) / DW_T, tiles_hw = tiles_w * ((a.Ho + DW_T - 1) / DW_T);
        const size_t lds = (size_t)(DW_CELLS * CS + DW_T * DW_T * 9 * 3) * sizeof(float);
        deform_bwd_window_kernel<T, VEC><<<(int)((long long)a.N * tiles_hw * a.G), 256, lds, st>>>(a, CS, tiles_w, tiles_hw);
        ydl_note_kernel(4, wname);
        return;
    }
    const int nchg = (a.C / a.G) / VEC;
    int seg = 1;
    while (seg < nchg && seg < 64) seg <<= 1;
    const long long items = (long long)a.N * a.Ho * a.Wo * a.kh * a.kw * a.G;
    deform_bwd_atomic_kernel<T, VEC><<<dfm_grid(items * seg), 256, 0, st>>>(a, seg);
    ydl_note_kernel(4, aname);
}

extern "C" int ydl_deform_bwd(int dtype, const void* x, int ldx, const void* offset, int ldo, const void* mask, int ldm, int mask_sigmoid,
                              const void* dcol, int ldc, float* grad_input, float* grad_offset, float* grad_mask, int N, int H, int W, int C,
                              int Ho, int Wo, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int G, void* stream) {
    DfmArgs a = {x, offset, mask, nullptr, dcol, grad_input, grad_offset, grad_mask, ldx, ldo, ldm, ldc, mask_sigmoid, 0,
                 N, H, W, C, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, G};
    if (int rc = dfm_check(a, dtype)) return rc;
    YDL_CHECK(dcol, "dcol is required");
    hipStream_t st = (hipStream_t)stream;
    const bool vec = dfm_vec(a, dtype, dcol);
    const int V = vec ? (dtype == YDL_F32 ? 4 : 8) : 1;
    const int Cg = C / G;
    int CS = 0;                                     // window channel slice: the widest of 64/32/16/8/4 that divides the group
    for (int cs = 64; cs >= V; cs >>= 1)
        if (Cg % cs == 0 && cs / V <= 16) { CS = cs; break; }
    const bool window = g_deform_win && vec && grad_input && kh == 3 && kw == 3 && sh == 1 && sw == 1 && dh == 1 && dw == 1 && CS > 0;
    if (window) {
        const size_t lds = (size_t)(DW_CELLS * CS + DW_T * DW_T * 9 * 3) * sizeof(float);
        if (dtype == YDL_F32) YDL_SET_MAX_LDS((deform_bwd_window_kernel<float, 4>), lds);
        else YDL_SET_MAX_LDS((deform_bwd_window_kernel<bf16_t, 8>), lds);
    }
    if (dtype == YDL_F32) {
        if (vec) dfm_bwd_launch<float, 4>(a, window, CS, st, "deform_bwd_window_kernel<f32>", "deform_bwd_atomic_kernel<f32,4>");
        else dfm_bwd_launch<float, 1>(a, false, 0, st, "", "deform_bwd_atomic_kernel<f32,1>");
    } else {
        if (vec) dfm_bwd_launch<bf16_t, 8>(a, window, CS, st, "deform_bwd_window_kernel<bf16>", "deform_bwd_atomic_kernel<bf16,8>");
        else dfm_bwd_launch<bf16_t, 1>(a, false, 0, st, "", "deform_bwd_atomic_kernel<bf16,1>");
    }
    YDL_LAUNCH_CHECK();
    return 0;
}
