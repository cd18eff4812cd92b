// Dilated convolution (stride 1, odd k, padding d*(k-1)/2: output and input have the same size) in column form for gfx950, NHWC.
// The zero-offset case of the deformable gather (deform.hip): ydl_dilated_cols writes col[pix][tap*C + c] = x at tap (ky, kx) of the
// dilated window, tap = ky*k + kx (k-major, so the KRSC weight [Cout][k*k][C] IS the weight of a 1x1 GEMM over col), the implicit-GEMM
// entry points do the products, the BatchNorm statistics and the weight gradient, and ydl_dilated_cols_bwd turns d col into d x.
// Without offsets both directions are pure gathers: the forward is a copy (one load per element, bit-exact), the backward reads the
// k*k entries of d col that one input element fed, adds them in f32 registers in tap order and stores once: no atomics, no workspace,
// bitwise reproducible.
// Two paths each.  Vector (C % 8 == 0 and 16-byte aligned rows): one lane per (pixel, 16-byte channel chunk), chunks fastest, the lane
// walks the k*k taps — its pixel coordinates are computed once, every access is 16 bytes and consecutive lanes touch consecutive
// addresses on both sides.  Element (any C: a 16-byte chunk of col would straddle taps): one lane per element.
#include "common.h"
#include <limits.h>

struct DilArgs {
    const void* src; void* dst;
    int lds, ldd, ones, acc;
    int N, H, W, C, k, d;
};

template <typename T> __device__ __forceinline__ T dil_one();
template <> __device__ __forceinline__ float dil_one<float>() { return 1.f; }
template <> __device__ __forceinline__ bf16_t dil_one<bf16_t>() { return (bf16_t)0x3F80; }

// ------------------------------------------------------------------------------------------------------
// forward: x (rows of lds) -> col (rows of ldd)
// ------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void dilated_cols_vec_kernel(const DilArgs a) {
    constexpr int V = ET<T>::V;
    const int nch = a.C / V, r = a.k / 2, KK = a.k * a.k;
    const long long npix = (long long)a.N * a.H * a.W, total = npix * nch;
    const T* x = (const T*)a.src;
    T* col = (T*)a.dst;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int ch = (int)(idx % nch);
        const long long pix = idx / nch;
        const int w = (int)(pix % a.W), h = (int)((pix / a.W) % a.H);
        const long long img = pix - ((long long)h * a.W + w);          // first pixel of this image
        const int c = ch * V;
        T* row = col + pix * a.ldd + c;
        int tap = 0;
        for (int ky = 0; ky < a.k; ++ky) {
            const int hh = h + (ky - r) * a.d;
            const bool vh = hh >= 0 && hh < a.H;
            for (int kx = 0; kx < a.k; ++kx, ++tap) {
                const int ww = w + (kx - r) * a.d;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (vh && ww >= 0 && ww < a.W) v = *(const uint4*)(x + (img + (long long)hh * a.W + ww) * a.lds + c);
                *(uint4*)(row + (long long)tap * a.C) = v;
            }
        }
        if (ch == 0 && a.ones) {                    // K*C is a multiple of 8 here: the tail is the bias column and seven zeros
            T* t = col + pix * a.ldd + (long long)KK * a.C;
            t[0] = dil_one<T>();
#pragma unroll
            for (int q = 1; q < 8; ++q) t[q] = (T)0;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void dilated_cols_elem_kernel(const DilArgs a, int width) {
    const int r = a.k / 2, KC = a.k * a.k * a.C;
    const long long npix = (long long)a.N * a.H * a.W, total = npix * width;
    const T* x = (const T*)a.src;
    T* col = (T*)a.dst;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(idx % width);
        const long long pix = idx / width;
        T v = (T)0;
        if (j < KC) {
            const int tap = j / a.C, c = j - tap * a.C;
            const int w = (int)(pix % a.W), h = (int)((pix / a.W) % a.H);
            const int hh = h + (tap / a.k - r) * a.d, ww = w + (tap % a.k - r) * a.d;
            if (hh >= 0 && hh < a.H && ww >= 0 && ww < a.W)
                v = x[(pix + (long long)(hh - h) * a.W + (ww - w)) * a.lds + c];
        } else if (j == KC && a.ones) {
            v = dil_one<T>();
        }
        col[pix * a.ldd + j] = v;
    }
}

// ------------------------------------------------------------------------------------------------------
// backward: d col (rows of lds) -> d x (rows of ldd); the tap (ky, kx) of output pixel (h - (ky-r)d, w - (kx-r)d) read x[h, w]
// ------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void dilated_cols_bwd_vec_kernel(const DilArgs a) {
    constexpr int V = ET<T>::V;
    const int nch = a.C / V, r = a.k / 2;
    const long long npix = (long long)a.N * a.H * a.W, total = npix * nch;
    const T* dcol = (const T*)a.src;
    T* dx = (T*)a.dst;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int ch = (int)(idx % nch);
        const long long pix = idx / nch;
        const int w = (int)(pix % a.W), h = (int)((pix / a.W) % a.H);
        const long long img = pix - ((long long)h * a.W + w);
        const int c = ch * V;
        float s[V], f[V];
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] = 0.f;
        int tap = 0;
        for (int ky = 0; ky < a.k; ++ky) {
            const int hh = h - (ky - r) * a.d;
            const bool vh = hh >= 0 && hh < a.H;
            for (int kx = 0; kx < a.k; ++kx, ++tap) {
                const int ww = w - (kx - r) * a.d;
                if (vh && ww >= 0 && ww < a.W) {
                    unpack16<T>(*(const uint4*)(dcol + (img + (long long)hh * a.W + ww) * a.lds + (long long)tap * a.C + c), f);
#pragma unroll
                    for (int e = 0; e < V; ++e) s[e] += f[e];
                }
            }
        }
        T* o = dx + pix * a.ldd + c;
        if (a.acc) {
            unpack16<T>(*(const uint4*)o, f);
#pragma unroll
            for (int e = 0; e < V; ++e) s[e] = f[e] + s[e];
        }
        *(uint4*)o = pack16<T>(s);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void dilated_cols_bwd_elem_kernel(const DilArgs a) {
    const int r = a.k / 2;
    const long long npix = (long long)a.N * a.H * a.W, total = npix * a.C;
    const T* dcol = (const T*)a.src;
    T* dx = (T*)a.dst;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % a.C);
        const long long pix = idx / a.C;
        const int w = (int)(pix % a.W), h = (int)((pix / a.W) % a.H);
        const long long img = pix - ((long long)h * a.W + w);
        float s = 0.f;
        int tap = 0;
        for (int ky = 0; ky < a.k; ++ky) {
            const int hh = h - (ky - r) * a.d;
            const bool vh = hh >= 0 && hh < a.H;
            for (int kx = 0; kx < a.k; ++kx, ++tap) {
                const int ww = w - (kx - r) * a.d;
                if (vh && ww >= 0 && ww < a.W) s += ET<T>::ld(dcol + (img + (long long)hh * a.W + ww) * a.lds + (long long)tap * a.C + c);
            }
        }
        T* o = dx + pix * a.ldd + c;
        if (a.acc) s = ET<T>::ld(o) + s;
        ET<T>::st(o, s);
    }
}

// ------------------------------------------------------------------------------------------------------
// host entry points
// ------------------------------------------------------------------------------------------------------
static int dil_check(int dtype, const void* a, const void* b, int ldx, int ldc, int ones, int N, int H, int W, int C, int k, int d) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "dtype must be YDL_F32 or YDL_BF16");
    YDL_CHECK(a && b, "null buffer");
    YDL_CHECK(N > 0 && H > 0 && W > 0 && C > 0, "empty shape");
    YDL_CHECK(k > 0 && (k & 1) && d >= 1, "stride 1, odd k, dilation d >= 1 and padding d*(k-1)/2 are the supported geometry");
    YDL_CHECK((long long)k * k * C + 8 < INT_MAX && (long long)k * d < INT_MAX / 2, "kernel window too large");
    YDL_CHECK(ldx >= C, "x row stride too small");
    YDL_CHECK(ldc >= round_up(k * k * C + (ones ? 1 : 0), 8), "col row stride too small");
    return 0;
}

static bool dil_vec(int dtype, const void* x, int ldx, const void* col, int ldc, int C) {
    const int V = dtype == YDL_F32 ? 4 : 8;
    return C % 8 == 0 && ldx % V == 0 && ldc % V == 0 && aligned16(x) && aligned16(col);
}

static int dil_grid(long long total) {
    long long b = (total + 255) / 256;
    const long long cap = 256ll * 32;
    return (int)(b < 1 ? 1 : b > cap ? cap : b);
}

extern "C" int ydl_dilated_cols(int dtype, const void* x, int ldx, void* col, int ldc, int ones_col,
                                int N, int H, int W, int C, int k, int d, void* stream) {
    if (int rc = dil_check(dtype, x, col, ldx, ldc, ones_col, N, H, W, C, k, d)) return rc;
    const DilArgs a = {x, col, ldx, ldc, ones_col ? 1 : 0, 0, N, H, W, C, k, d};
    hipStream_t st = (hipStream_t)stream;
    const long long npix = (long long)N * H * W;
    if (dil_vec(dtype, x, ldx, col, ldc, C)) {
        const int grid = dil_grid(npix * (C / (dtype == YDL_F32 ? 4 : 8)));
        if (dtype == YDL_F32) dilated_cols_vec_kernel<float><<<grid, 256, 0, st>>>(a);
        else dilated_cols_vec_kernel<bf16_t><<<grid, 256, 0, st>>>(a);
    } else {
        const int width = round_up(k * k * C + a.ones, 8);      // written columns: taps, the bias column, zeros up to a multiple of 8
        const int grid = dil_grid(npix * width);
        if (dtype == YDL_F32) dilated_cols_elem_kernel<float><<<grid, 256, 0, st>>>(a, width);
        else dilated_cols_elem_kernel<bf16_t><<<grid, 256, 0, st>>>(a, width);
    }
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int ydl_dilated_cols_bwd(int dtype, const void* dcol, int ldc, void* dx, int lddx, int accumulate,
                                    int N, int H, int W, int C, int k, int d, void* stream) {
    if (int rc = dil_check(dtype, dcol, dx, lddx, ldc, 0, N, H, W, C, k, d)) return rc;
    const DilArgs a = {dcol, dx, ldc, lddx, 0, accumulate ? 1 : 0, N, H, W, C, k, d};
    hipStream_t st = (hipStream_t)stream;
    const long long npix = (long long)N * H * W;
    if (dil_vec(dtype, dx, lddx, dcol, ldc, C)) {
        const int grid = dil_grid(npix * (C / (dtype == YDL_F32 ? 4 : 8)));
        if (dtype == YDL_F32) dilated_cols_bwd_vec_kernel<float><<<grid, 256, 0, st>>>(a);
        else dilated_cols_bwd_vec_kernel<bf16_t><<<grid, 256, 0, st>>>(a);
    } else {
        const int grid = dil_grid(npix * C);
        if (dtype == YDL_F32) dilated_cols_bwd_elem_kernel<float><<<grid, 256, 0, st>>>(a);
        else dilated_cols_bwd_elem_kernel<bf16_t><<<grid, 256, 0, st>>>(a);
    }
    YDL_LAUNCH_CHECK();
    return 0;
}
