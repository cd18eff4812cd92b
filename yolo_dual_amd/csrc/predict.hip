// The test / predict path (include/ydl.h, "prediction path"): label maps from scores, their nearest resize, the confusion matrix
// and histogram of label maps, and the three pictures the reference draws from them.  One thread per pixel (the up-sampling form
// of ydl_softmax_resize_labels shares its source pixels through LDS); the only atomics are the LDS / global atomicAdd pair of
// confusion_kernel (loss.hip).
#include "common.h"

#define MAXC 32          // as in loss.hip
#define MAXBINS 4096     // ydl_label_bincount: LDS histogram of nbins + 1 words

// torch.argmax over `C` values handed in one by one: the first maximum wins, a NaN counts as the maximum and the first NaN wins
struct ArgMax {
    float best;
    int bi;
    __device__ __forceinline__ void first(float v) { best = v; bi = 0; }
    __device__ __forceinline__ void next(float v, int c) {
        if (best == best && (v > best || v != v)) { best = v; bi = c; }
    }
};

// VEC: sc == 1 and every row 16-byte aligned with room for whole chunks: the pixel's channels come as 16-byte vectors.
// WIDE: rep_w is 2 or 4 and every output row start is a multiple of it: one 2- / 4-byte store per replicated row.
template <typename T, bool VEC, bool WIDE>
__global__ __launch_bounds__(256) void argmax_labels_kernel(const T* __restrict__ x, long long sn, long long sc, long long sh,
                                                            long long sw, int N, int C, int H, int W, int rep_h, int rep_w,
                                                            uint8_t* __restrict__ labels, long long ldl_n, long long ldl_h) {
    const long long total = (long long)N * H * W;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int w = (int)(i % W);
    const long long t2 = i / W;
    const int h = (int)(t2 % H);
    const int n = (int)(t2 / H);
    const T* pp = x + n * sn + h * sh + w * sw;
    ArgMax am;
    if (VEC) {
        constexpr int V = ET<T>::V;
        float f[V];
        for (int c0 = 0; c0 < C; c0 += V) {
            unpack16<T>(*(const uint4*)(pp + c0), f);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                if (c0 + e == 0) am.first(f[0]);
                else if (c0 + e < C) am.next(f[e], c0 + e);
            }
        }
    } else {
        am.first(ET<T>::ld(pp));
        for (int c = 1; c < C; ++c) am.next(ET<T>::ld(pp + c * sc), c);
    }
    uint8_t* op = labels + n * ldl_n + (long long)h * rep_h * ldl_h + (long long)w * rep_w;
    const uint32_t four = (uint32_t)am.bi * 0x01010101u;
    for (int r = 0; r < rep_h; ++r, op += ldl_h) {
        if (WIDE) {
            if (rep_w == 4) *(uint32_t*)op = four;
            else *(uint16_t*)op = (uint16_t)four;
        } else {
            for (int q = 0; q < rep_w; ++q) op[q] = (uint8_t)am.bi;
        }
    }
}

static inline unsigned blocks256(long long total) { return (unsigned)((total + 255) / 256); }

extern "C" int ydl_argmax_labels(int dtype, const void* x, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int N, int C, int H, int W,
                                 int rep_h, int rep_w, uint8_t* labels, int64_t ldl_n, int64_t ldl_h, void* stream) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "scores are f32 or bf16");
    YDL_CHECK(x && labels && N >= 1 && H >= 1 && W >= 1 && rep_h >= 1 && rep_w >= 1, "bad arguments");
    YDL_CHECK(C >= 1 && C <= MAXC, "1 <= C <= 32");
    YDL_CHECK(sn >= 0 && sc >= 0 && sh >= 0 && sw >= 0, "negative strides");
    const long long LH = (long long)H * rep_h, LW = (long long)W * rep_w;
    YDL_CHECK(LH < (1ll << 31) && LW < (1ll << 31) && (long long)N * H * W < (1ll << 31), "too large");
    YDL_CHECK(ldl_h >= LW && (N == 1 || ldl_n >= (LH - 1) * ldl_h + LW), "label strides overlap");
    const int es = esize(dtype), V = 16 / es;
    const bool vec = sc == 1 && aligned16(x) && (sw * es) % 16 == 0 && (sh * es) % 16 == 0 && (sn * es) % 16 == 0 &&
                     sw >= round_up(C, V);
    const bool wide = (rep_w == 2 || rep_w == 4) && ((uintptr_t)labels) % rep_w == 0 && ldl_h % rep_w == 0 && ldl_n % rep_w == 0;
    const unsigned grid = blocks256((long long)N * H * W);
    hipStream_t st = (hipStream_t)stream;
#define YDL_ARGMAX(T, VEC, WIDE)                                                                                     \
    argmax_labels_kernel<T, VEC, WIDE><<<grid, 256, 0, st>>>((const T*)x, sn, sc, sh, sw, N, C, H, W, rep_h, rep_w, \
                                                             labels, ldl_n, ldl_h)
    if (dtype == YDL_F32) {
        if (vec) { if (wide) YDL_ARGMAX(float, true, true); else YDL_ARGMAX(float, true, false); }
        else     { if (wide) YDL_ARGMAX(float, false, true); else YDL_ARGMAX(float, false, false); }
    } else {
        if (vec) { if (wide) YDL_ARGMAX(bf16_t, true, true); else YDL_ARGMAX(bf16_t, true, false); }
        else     { if (wide) YDL_ARGMAX(bf16_t, false, true); else YDL_ARGMAX(bf16_t, false, false); }
    }
#undef YDL_ARGMAX
    YDL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// argmax of bilinear_resize(softmax(x)): the exit of a yaml model whose last Softmax is not at the output size (every Upsample of
// the v8 family emits 256 x 256, and the result is resized to img_size).  Neither the f32 probabilities nor their resized copy are
// written: a thread forms the softmax of its output pixel's four source pixels and blends them.  The arithmetic is that of
// softmax_fwd_kernel (loss.hip) followed by resize_fwd_kernel's bilinear branch (spatial.hip), expression for expression, so the
// blended f32 probabilities, and with them the labels, are the ones model(x) would have exported.
// ------------------------------------------------------------------------------------------------------
struct Lin { int i0, i1; float w0, w1; };
__device__ __forceinline__ Lin lin_src(int dst, float scale, int in) {       // align_corners = False, ATen's float arithmetic
    Lin L;
    float src = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f);
    if (src < 0.f) src = 0.f;
    L.i0 = (int)src;
    if (L.i0 > in - 1) L.i0 = in - 1;
    L.i1 = L.i0 + (L.i0 < in - 1 ? 1 : 0);
    L.w1 = __fsub_rn(src, (float)L.i0);
    L.w0 = __fsub_rn(1.f, L.w1);
    return L;
}

template <typename T, int MC>
__device__ __forceinline__ void softmax_row(const T* __restrict__ xp, int C, float* v) {
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < MC; ++c)
        if (c < C) { v[c] = ET<T>::ld(xp + c); mx = fmaxf(mx, v[c]); }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < MC; ++c)
        if (c < C) { v[c] = expf(v[c] - mx); s += v[c]; }
    float inv = 1.f / s;
#pragma unroll
    for (int c = 0; c < MC; ++c)
        if (c < C) v[c] = v[c] * inv;
}

template <typename T, int MC>
__global__ __launch_bounds__(256) void softmax_resize_labels_kernel(const T* __restrict__ x, int ldx, int N, int C, int Hi, int Wi,
                                                                    int Ho, int Wo, float sh, float sw, uint8_t* __restrict__ labels,
                                                                    long long ldl_n, long long ldl_h) {
    const long long total = (long long)N * Ho * Wo;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int wo = (int)(i % Wo);
    const long long t2 = i / Wo;
    const int ho = (int)(t2 % Ho);
    const int n = (int)(t2 / Ho);
    const Lin lh = lin_src(ho, sh, Hi), lw = lin_src(wo, sw, Wi);
    const T* xb = x + (size_t)n * Hi * Wi * ldx;
    float v00[MC], v01[MC], v10[MC], v11[MC];
    softmax_row<T, MC>(xb + ((size_t)lh.i0 * Wi + lw.i0) * ldx, C, v00);
    softmax_row<T, MC>(xb + ((size_t)lh.i0 * Wi + lw.i1) * ldx, C, v01);
    softmax_row<T, MC>(xb + ((size_t)lh.i1 * Wi + lw.i0) * ldx, C, v10);
    softmax_row<T, MC>(xb + ((size_t)lh.i1 * Wi + lw.i1) * ldx, C, v11);
    ArgMax am;
#pragma unroll
    for (int c = 0; c < MC; ++c)
        if (c < C) {
            const float o = lh.w0 * (lw.w0 * v00[c] + lw.w1 * v01[c]) + lh.w1 * (lw.w0 * v10[c] + lw.w1 * v11[c]);
            if (c == 0) am.first(o);
            else am.next(o, c);
        }
    labels[n * ldl_n + ho * ldl_h + wo] = (uint8_t)am.bi;
}

// Up-sampling form: a CTA owns a 16 x 16 tile of the output.  The source pixels the tile's bilinear taps can name form a small
// rectangle (at most SRL_TS rows and columns when the scale is at most 0.6): their softmax is computed ONCE into LDS and the 256
// threads blend from there, instead of 4 softmax evaluations (4 * C exponentials) per output pixel.  The per-element arithmetic is
// the kernel's above, so the two forms give the same labels.  A tile whose rectangle would not fit (never, for the scales the
// launcher sends here) falls back to the direct form per thread.
#define SRL_TS 12
template <typename T, int MC>
__global__ __launch_bounds__(256) void softmax_resize_labels_tiled_kernel(const T* __restrict__ x, int ldx, int N, int C, int Hi,
                                                                          int Wi, int Ho, int Wo, float sh, float sw,
                                                                          uint8_t* __restrict__ labels, long long ldl_n,
                                                                          long long ldl_h) {
    __shared__ float prob[SRL_TS * SRL_TS][MC + 1];
    const int n = blockIdx.z;
    const int ho0 = blockIdx.y * 16, wo0 = blockIdx.x * 16;
    const int ho1 = min(ho0 + 15, Ho - 1), wo1 = min(wo0 + 15, Wo - 1);
    const int r0 = lin_src(ho0, sh, Hi).i0, c0 = lin_src(wo0, sw, Wi).i0;          // source indices grow with the output index
    const int th = lin_src(ho1, sh, Hi).i1 - r0 + 1, tw = lin_src(wo1, sw, Wi).i1 - c0 + 1;
    const bool fits = th <= SRL_TS && tw <= SRL_TS;          // uniform over the CTA
    const T* xb = x + (size_t)n * Hi * Wi * ldx;
    if (fits) {
        for (int q = threadIdx.x; q < th * tw; q += 256) {
            const int r = q / tw, c = q - r * tw;
            float v[MC];
            softmax_row<T, MC>(xb + ((size_t)(r0 + r) * Wi + (c0 + c)) * ldx, C, v);
#pragma unroll
            for (int k = 0; k < MC; ++k)
                if (k < C) prob[q][k] = v[k];
        }
    }
    __syncthreads();
    const int ho = ho0 + (int)(threadIdx.x >> 4), wo = wo0 + (int)(threadIdx.x & 15);
    if (ho >= Ho || wo >= Wo) return;
    const Lin lh = lin_src(ho, sh, Hi), lw = lin_src(wo, sw, Wi);
    ArgMax am;
    if (fits) {
        const float* p00 = prob[(lh.i0 - r0) * tw + (lw.i0 - c0)];
        const float* p01 = prob[(lh.i0 - r0) * tw + (lw.i1 - c0)];
        const float* p10 = prob[(lh.i1 - r0) * tw + (lw.i0 - c0)];
        const float* p11 = prob[(lh.i1 - r0) * tw + (lw.i1 - c0)];
#pragma unroll
        for (int c = 0; c < MC; ++c)
            if (c < C) {
                const float o = lh.w0 * (lw.w0 * p00[c] + lw.w1 * p01[c]) + lh.w1 * (lw.w0 * p10[c] + lw.w1 * p11[c]);
                if (c == 0) am.first(o);
                else am.next(o, c);
            }
    } else {
        float v00[MC], v01[MC], v10[MC], v11[MC];
        softmax_row<T, MC>(xb + ((size_t)lh.i0 * Wi + lw.i0) * ldx, C, v00);
        softmax_row<T, MC>(xb + ((size_t)lh.i0 * Wi + lw.i1) * ldx, C, v01);
        softmax_row<T, MC>(xb + ((size_t)lh.i1 * Wi + lw.i0) * ldx, C, v10);
        softmax_row<T, MC>(xb + ((size_t)lh.i1 * Wi + lw.i1) * ldx, C, v11);
#pragma unroll
        for (int c = 0; c < MC; ++c)
            if (c < C) {
                const float o = lh.w0 * (lw.w0 * v00[c] + lw.w1 * v01[c]) + lh.w1 * (lw.w0 * v10[c] + lw.w1 * v11[c]);
                if (c == 0) am.first(o);
                else am.next(o, c);
            }
    }
    labels[n * ldl_n + ho * ldl_h + wo] = (uint8_t)am.bi;
}

extern "C" int ydl_softmax_resize_labels(int dtype, const void* x, int ldx, int N, int C, int Hi, int Wi, int Ho, int Wo,
                                         uint8_t* labels, int64_t ldl_n, int64_t ldl_h, void* stream) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "scores are f32 or bf16");
    YDL_CHECK(x && labels && N >= 1 && Hi >= 1 && Wi >= 1 && Ho >= 1 && Wo >= 1, "bad arguments");
    YDL_CHECK(C >= 1 && C <= MAXC && ldx >= C, "1 <= C <= 32, rows of at least C elements");
    YDL_CHECK((long long)N * Ho * Wo < (1ll << 31) && (long long)N * Hi * Wi < (1ll << 31) && Ho < (1 << 20) && Wo < (1 << 20),
              "too large");
    YDL_CHECK(ldl_h >= Wo && (N == 1 || ldl_n >= ((long long)Ho - 1) * ldl_h + Wo), "label strides overlap");
    const float sh = (float)Hi / (float)Ho, sw = (float)Wi / (float)Wo;        // axis_scale of ydl_resize_fwd, mode 1, no given scale
    const unsigned grid = (unsigned)(((long long)N * Ho * Wo + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    // 16 consecutive outputs span at most floor(15 * scale) + 3 source rows: SRL_TS = 12 of them up to a scale of 0.6
    const bool tiled = sh <= 0.6f && sw <= 0.6f && N <= 65535;
    const dim3 tgrid((unsigned)((Wo + 15) / 16), (unsigned)((Ho + 15) / 16), (unsigned)N);
#define YDL_SRL(T, MC)                                                                                                              \
    do {                                                                                                                            \
        if (tiled)                                                                                                                  \
            softmax_resize_labels_tiled_kernel<T, MC><<<tgrid, 256, 0, st>>>((const T*)x, ldx, N, C, Hi, Wi, Ho, Wo, sh, sw, labels, \
                                                                             ldl_n, ldl_h);                                         \
        else                                                                                                                        \
            softmax_resize_labels_kernel<T, MC><<<grid, 256, 0, st>>>((const T*)x, ldx, N, C, Hi, Wi, Ho, Wo, sh, sw, labels, ldl_n, \
                                                                      ldl_h);                                                       \
    } while (0)
    if (dtype == YDL_F32) { if (C <= 16) YDL_SRL(float, 16); else YDL_SRL(float, 32); }
    else                  { if (C <= 16) YDL_SRL(bf16_t, 16); else YDL_SRL(bf16_t, 32); }
#undef YDL_SRL
    YDL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// nearest resize of a crop box (ATen's rule: the scale is a float, the product one f32 multiplication)
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int nearest_src(int i, float scale, int n_in) {
    const int s = (int)floorf(__fmul_rn((float)i, scale));
    return s < n_in - 1 ? s : n_in - 1;
}

__global__ __launch_bounds__(256) void labels_resize_kernel(const uint8_t* __restrict__ src, long long lds_n, long long lds_h, int N,
                                                            int y0, int x0, int hc, int wc, uint8_t* __restrict__ dst,
                                                            long long ldd_n, long long ldd_h, int Ho, int Wo, float scale_h,
                                                            float scale_w) {
    const long long total = (long long)N * Ho * Wo;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int w = (int)(i % Wo);
    const long long t2 = i / Wo;
    const int h = (int)(t2 % Ho);
    const int n = (int)(t2 / Ho);
    const int sy = y0 + nearest_src(h, scale_h, hc), sx = x0 + nearest_src(w, scale_w, wc);
    dst[n * ldd_n + h * ldd_h + w] = src[n * lds_n + sy * lds_h + sx];
}

extern "C" int ydl_labels_resize(const uint8_t* src, int64_t lds_n, int64_t lds_h, int N, int y0, int x0, int hc, int wc,
                                 uint8_t* dst, int64_t ldd_n, int64_t ldd_h, int Ho, int Wo, void* stream) {
    YDL_CHECK(src && dst && N >= 1 && Ho >= 1 && Wo >= 1, "bad arguments");
    YDL_CHECK(y0 >= 0 && x0 >= 0 && hc >= 1 && wc >= 1, "bad crop box");
    YDL_CHECK((long long)x0 + wc <= lds_h && (N == 1 || ((long long)y0 + hc - 1) * lds_h + x0 + wc <= lds_n),
              "crop box leaves the source row or image");
    YDL_CHECK(ldd_h >= Wo && (N == 1 || ldd_n >= ((long long)Ho - 1) * ldd_h + Wo), "destination strides overlap");
    YDL_CHECK((long long)N * Ho * Wo < (1ll << 31), "too large");
    const float scale_h = (float)hc / (float)Ho, scale_w = (float)wc / (float)Wo;
    labels_resize_kernel<<<blocks256((long long)N * Ho * Wo), 256, 0, (hipStream_t)stream>>>(src, lds_n, lds_h, N, y0, x0, hc, wc, dst,
                                                                                             ldd_n, ldd_h, Ho, Wo, scale_h, scale_w);
    YDL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// confusion matrix of two label maps (rows = target, cols = prediction) and the histogram of one
// ------------------------------------------------------------------------------------------------------
template <typename TT>
__global__ __launch_bounds__(256) void confusion_labels_kernel(const uint8_t* __restrict__ pred, long long ldp_n, long long ldp_h,
                                                               const TT* __restrict__ target, long long ldt_n, long long ldt_h, int N,
                                                               int H, int W, int C, int ignore,
                                                               unsigned long long* __restrict__ matrix) {
    __shared__ unsigned int hist[MAXC * MAXC];
    for (int i = threadIdx.x; i < C * C; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    const long long total = (long long)N * H * W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int w = (int)(i % W);
        const long long t2 = i / W;
        const int h = (int)(t2 % H);
        const int n = (int)(t2 / H);
        const long long t = (long long)target[n * ldt_n + h * ldt_h + w];
        const int p = pred[n * ldp_n + h * ldp_h + w];
        if (t < 0 || t >= C || t == ignore || p >= C) continue;
        atomicAdd(&hist[(int)t * C + p], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += blockDim.x)
        if (hist[i]) atomicAdd(&matrix[i], (unsigned long long)hist[i]);
}

static inline int hist_grid(long long total) {
    long long g = (total + 255) / 256;
    return (int)(g > 1024 ? 1024 : g);
}

extern "C" int ydl_confusion_labels(const uint8_t* pred, int64_t ldp_n, int64_t ldp_h, const void* target, int target_is_i64,
                                    int64_t ldt_n, int64_t ldt_h, int N, int H, int W, int C, int ignore_index, int64_t* matrix,
                                    void* stream) {
    YDL_CHECK(pred && target && matrix && N >= 1 && H >= 1 && W >= 1, "bad arguments");
    YDL_CHECK(C >= 1 && C <= MAXC, "1 <= C <= 32");
    YDL_CHECK(ldp_h >= W && ldt_h >= W && ldp_n >= 0 && ldt_n >= 0, "row strides shorter than a row");
    const long long total = (long long)N * H * W;
    hipStream_t st = (hipStream_t)stream;
    if (target_is_i64)
        confusion_labels_kernel<int64_t><<<hist_grid(total), 256, 0, st>>>(pred, ldp_n, ldp_h, (const int64_t*)target, ldt_n, ldt_h, N, H,
                                                                           W, C, ignore_index, (unsigned long long*)matrix);
    else
        confusion_labels_kernel<uint8_t><<<hist_grid(total), 256, 0, st>>>(pred, ldp_n, ldp_h, (const uint8_t*)target, ldt_n, ldt_h, N, H,
                                                                           W, C, ignore_index, (unsigned long long*)matrix);
    YDL_LAUNCH_CHECK();
    return 0;
}

template <typename TT>
__global__ __launch_bounds__(256) void label_bincount_kernel(const TT* __restrict__ labels, long long n, int nbins,
                                                             unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned int bins[];
    for (int i = threadIdx.x; i <= nbins; i += blockDim.x) bins[i] = 0;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long v = (long long)labels[i];
        atomicAdd(&bins[(v < 0 || v >= nbins) ? nbins : (int)v], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i <= nbins; i += blockDim.x)
        if (bins[i]) atomicAdd(&counts[i], (unsigned long long)bins[i]);
}

extern "C" int ydl_label_bincount(const void* labels, int is_i64, int64_t n, int nbins, int64_t* counts, void* stream) {
    YDL_CHECK(labels && counts && n >= 0, "bad arguments");
    YDL_CHECK(nbins >= 1 && nbins <= MAXBINS, "1 <= nbins <= 4096");
    if (n == 0) return 0;
    const size_t lds = (size_t)(nbins + 1) * sizeof(unsigned int);
    hipStream_t st = (hipStream_t)stream;
    if (is_i64)
        label_bincount_kernel<int64_t><<<hist_grid(n), 256, lds, st>>>((const int64_t*)labels, n, nbins, (unsigned long long*)counts);
    else
        label_bincount_kernel<uint8_t><<<hist_grid(n), 256, lds, st>>>((const uint8_t*)labels, n, nbins, (unsigned long long*)counts);
    YDL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// pictures: colour, difference, overlay
// ------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void labels_render_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ target,
                                                            const float* __restrict__ img, const uint8_t* __restrict__ palette,
                                                            int npal, uint8_t* __restrict__ out, int N, long long HW, int bgr) {
    const long long total = (long long)N * HW;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int p = pred[i];
    int c0 = 0, c1 = 0, c2 = 0;
    if (p < npal) { c0 = palette[3 * p]; c1 = palette[3 * p + 1]; c2 = palette[3 * p + 2]; }
    if (MODE == 1 && p != (int)target[i]) { c0 = 255; c1 = 0; c2 = 255; }
    if (MODE == 2) {
        const long long n = i / HW, q = i - n * HW;
        const float* ip = img + n * 3 * HW + q;
        int b[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = __fmul_rn(ip[k * HW], 255.f);
            b[k] = (int)fminf(fmaxf(v, 0.f), 255.f);        // uint8 by truncation (a value outside [0, 255] saturates; NaN gives 0)
        }
        if (bgr) { const int t = b[0]; b[0] = b[2]; b[2] = t; }
        // 0.5 * base + 0.5 * colour is exact in f32; rintf rounds half to even; the sum of two bytes' halves never leaves [0, 255]
        c0 = (int)rintf(0.5f * (float)b[0] + 0.5f * (float)c0);
        c1 = (int)rintf(0.5f * (float)b[1] + 0.5f * (float)c1);
        c2 = (int)rintf(0.5f * (float)b[2] + 0.5f * (float)c2);
    }
    uint8_t* o = out + 3 * i;
    o[0] = (uint8_t)c0;
    o[1] = (uint8_t)c1;
    o[2] = (uint8_t)c2;
}

extern "C" int ydl_labels_render(int mode, const uint8_t* pred, const uint8_t* target, const float* img, const uint8_t* palette,
                                 int npal, uint8_t* out, int N, int H, int W, int bgr, void* stream) {
    YDL_CHECK(mode >= 0 && mode <= 2, "mode is 0 (colour), 1 (difference) or 2 (overlay)");
    YDL_CHECK(pred && palette && out && N >= 1 && H >= 1 && W >= 1 && npal >= 1 && npal <= 256, "bad arguments");
    YDL_CHECK(mode != 1 || target, "the difference picture needs the target labels");
    YDL_CHECK(mode != 2 || img, "the overlay needs the image");
    const long long HW = (long long)H * W, total = HW * N;
    YDL_CHECK(total < (1ll << 31), "too large");
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = blocks256(total);
    if (mode == 0) labels_render_kernel<0><<<grid, 256, 0, st>>>(pred, target, img, palette, npal, out, N, HW, bgr);
    else if (mode == 1) labels_render_kernel<1><<<grid, 256, 0, st>>>(pred, target, img, palette, npal, out, N, HW, bgr);
    else labels_render_kernel<2><<<grid, 256, 0, st>>>(pred, target, img, palette, npal, out, N, HW, bgr);
    YDL_LAUNCH_CHECK();
    return 0;
}
