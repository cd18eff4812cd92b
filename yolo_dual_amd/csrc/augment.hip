// The reference dataset's seven random augmentations (unet-lite/yolo5-seg/seg_diceloss_yolov5.py:75-185) on decoded uint8 arrays:
// image [h][w][3], label map [h][w], same size out.  Bit-exact with Pillow 12 for 8-bit images: every kernel restates the arithmetic
// of the Pillow routine the reference's class ends up in (Geometry.c, Blend.c, BoxBlur.c, Resample.c); what Pillow computes once per
// call in Python or in double on the host (rotation matrix, box weights, resampling tables) arrives as arguments (yolo_dual_amd/data.py).
// Streaming byte work: one thread per output byte or pixel, consecutive threads write consecutive bytes.
//
// Pillow's x86-64 build rounds after every multiply and every add; hipcc would contract a + b*c into one FMA (the library is built
// with -ffp-contract=on).  The whole file is compiled WITHOUT contraction by the pragma below: it covers the affine source
// coordinates and the lerps of the rotation and the brightness / contrast blend.
#pragma clang fp contract(off)
#include <algorithm>

#include "common.h"

#define PIL_PRECISION_BITS 22

static inline unsigned aug_blocks(long long n) { return (unsigned)((n + 255) / 256); }

// ---- mirror / flip: ImageOps.mirror / ImageOps.flip ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void aug_flip_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int h,
                                                       int w, int c, int horizontal) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int rowb = w * c;
    if (i >= (long long)h * rowb) return;
    const int y = (int)(i / rowb), b = (int)(i - (long long)y * rowb);
    const int x = b / c, ch = b - x * c;
    const size_t s = horizontal ? ((size_t)y * w + (w - 1 - x)) * c + ch : ((size_t)(h - 1 - y) * w + x) * c + ch;
    dst[i] = src[s];
}

// ---- rotation, image: Geometry.c affine_transform + bilinear_filter32RGB (double, truncating store, 0 outside) -----------------
__global__ __launch_bounds__(256) void aug_rotate_image_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                               int h, int w, double a0, double a1, double a2, double a3, double a4,
                                                               double a5) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)h * w) return;
    const int oy = (int)(i / w), ox = (int)(i - (long long)oy * w);
    const double px = ox + 0.5, py = oy + 0.5;
    double xin = a0 * px + a1 * py + a2;
    double yin = a3 * px + a4 * py + a5;
    unsigned char* o = dst + (size_t)i * 3;
    if (xin < 0.0 || xin >= (double)w || yin < 0.0 || yin >= (double)h) {
        o[0] = 0; o[1] = 0; o[2] = 0;
        return;
    }
    xin -= 0.5;
    yin -= 0.5;
    const int x = (int)floor(xin), y = (int)floor(yin);
    const double dx = xin - x, dy = yin - y;
    const int x0 = min(max(x, 0), w - 1), x1 = min(max(x + 1, 0), w - 1), y0 = min(max(y, 0), h - 1);
    const unsigned char* r0 = src + (size_t)y0 * w * 3;
    const bool second = y + 1 >= 0 && y + 1 < h;
    const unsigned char* r1 = src + (size_t)(second ? y + 1 : y0) * w * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double p = r0[x0 * 3 + c], q = r0[x1 * 3 + c];
        const double v1 = p + (q - p) * dx;
        double v2 = v1;
        if (second) {
            const double p2 = r1[x0 * 3 + c], q2 = r1[x1 * 3 + c];
            v2 = p2 + (q2 - p2) * dx;
        }
        o[c] = (unsigned char)(int)(v1 + (v2 - v1) * dy);
    }
}

// ---- rotation, label map: Geometry.c affine_fixed (16.16 fixed point, nearest, 0 outside) ---------------------------------------
__global__ __launch_bounds__(256) void aug_rotate_mask_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                              int h, int w, long long a0, long long a1, long long a2, long long a3,
                                                              long long a4, long long a5) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)h * w) return;
    const int y = (int)(i / w), x = (int)(i - (long long)y * w);
    const long long xin = (a2 + a1 * y + a0 * x) >> 16, yin = (a5 + a4 * y + a3 * x) >> 16;
    unsigned char v = 0;
    if (xin >= 0 && xin < w && yin >= 0 && yin < h) v = src[(size_t)yin * w + xin];
    dst[i] = v;
}

// ---- brightness / contrast: ImageEnhance -> Image.blend(degenerate, image, factor) (Blend.c, single precision) -----------------
__device__ __forceinline__ unsigned char aug_blend8(int d, int px, float f) {
    const float v = (float)d + f * (float)(px - d);
    return v <= 0.0f ? 0 : (v >= 255.0f ? 255 : (unsigned char)(int)v);
}

__global__ __launch_bounds__(256) void aug_brightness_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                             long long n, float f) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = aug_blend8(0, src[i], f);
}

// image.convert("L") summed over the image (ImageStat: exact integer sum); one atomic per wave
__global__ __launch_bounds__(256) void aug_luma_sum_kernel(const unsigned char* __restrict__ src, long long npix,
                                                           unsigned long long* __restrict__ sum) {
    unsigned int acc = 0;                       // at most 255 per pixel: a thread would need 2^24 pixels to overflow
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x) {
        const unsigned char* p = src + (size_t)i * 3;
        acc += (19595u * p[0] + 38470u * p[1] + 7471u * p[2] + 0x8000u) >> 16;
    }
    unsigned long long t = acc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    if ((threadIdx.x & 63) == 0 && t) atomicAdd(sum, t);
}

// d = int(ImageStat.mean[0] + 0.5), formed once on the device (an IEEE double division): ws[0] = the sum, ws[1] = d
__global__ void aug_contrast_mean_kernel(unsigned long long* __restrict__ ws, long long npix) {
    ws[1] = (unsigned long long)(int)((double)ws[0] / (double)npix + 0.5);
}

__global__ __launch_bounds__(256) void aug_contrast_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                           long long n, float f, const unsigned long long* __restrict__ ws) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    dst[i] = aug_blend8((int)ws[1], src[i], f);
}

// ---- Gaussian blur: one pass of BoxBlur.c ImagingLineBoxBlur32 along x (or along y), 32-bit unsigned arithmetic ------------------
__global__ __launch_bounds__(256) void aug_box_blur_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int h,
                                                           int w, int vertical, int R, unsigned int ww, unsigned int fw) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)h * w) return;
    const int y = (int)(i / w), x = (int)(i - (long long)y * w);
    const int pos = vertical ? y : x, len = vertical ? h : w;
    const size_t step = vertical ? (size_t)w * 3 : 3;
    const unsigned char* line = src + (vertical ? (size_t)x * 3 : (size_t)y * w * 3);
    unsigned int s0 = 0, s1 = 0, s2 = 0;
    for (int k = -R; k <= R; ++k) {
        const unsigned char* p = line + (size_t)min(max(pos + k, 0), len - 1) * step;
        s0 += p[0]; s1 += p[1]; s2 += p[2];
    }
    const unsigned char* pa = line + (size_t)min(max(pos - R - 1, 0), len - 1) * step;
    const unsigned char* pb = line + (size_t)min(max(pos + R + 1, 0), len - 1) * step;
    unsigned char* o = dst + (size_t)i * 3;
    o[0] = (unsigned char)((s0 * ww + ((unsigned int)pa[0] + pb[0]) * fw + (1u << 23)) >> 24);
    o[1] = (unsigned char)((s1 * ww + ((unsigned int)pa[1] + pb[1]) * fw + (1u << 23)) >> 24);
    o[2] = (unsigned char)((s2 * ww + ((unsigned int)pa[2] + pb[2]) * fw + (1u << 23)) >> 24);
}

// ---- crop + resize back: Resample.c on a sub-rectangle (the crop is a fresh image to Pillow: no tap leaves the box) ----------------
__device__ __forceinline__ unsigned char aug_clip8(int ss) {
    const int v = ss >> PIL_PRECISION_BITS;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// horizontal pass: rows of the box (src points at its first pixel, `pitch` pixels per source row) -> tmp [ch][w][3]
__global__ __launch_bounds__(256) void aug_crop_h_kernel(const unsigned char* __restrict__ src, int pitch, int ch,
                                                         unsigned char* __restrict__ tmp, int w, const int* __restrict__ xb,
                                                         const int* __restrict__ xk, int ksize) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)ch * w) return;
    const int y = (int)(i / w), xx = (int)(i - (long long)y * w);
    const int x0 = xb[2 * xx], n = xb[2 * xx + 1];
    const int* k = xk + (size_t)xx * ksize;
    const unsigned char* row = src + ((size_t)y * pitch + x0) * 3;
    int s0 = 1 << (PIL_PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < n; ++t) {
        const int c = k[t];
        s0 += (int)row[3 * t + 0] * c;
        s1 += (int)row[3 * t + 1] * c;
        s2 += (int)row[3 * t + 2] * c;
    }
    unsigned char* o = tmp + (size_t)i * 3;
    o[0] = aug_clip8(s0); o[1] = aug_clip8(s1); o[2] = aug_clip8(s2);
}

// vertical pass (or a plain copy when the height does not change): mid [ch][.][3] with `pitch` pixels per row -> dst [h][w][3]
__global__ __launch_bounds__(256) void aug_crop_v_kernel(const unsigned char* __restrict__ mid, int pitch, unsigned char* __restrict__ dst,
                                                         int h, int w, const int* __restrict__ yb, const int* __restrict__ yk, int ksize,
                                                         int vertical) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)h * w) return;
    const int y = (int)(i / w), x = (int)(i - (long long)y * w);
    unsigned char* o = dst + (size_t)i * 3;
    if (!vertical) {
        const unsigned char* p = mid + ((size_t)y * pitch + x) * 3;
        o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
        return;
    }
    const int y0 = yb[2 * y], n = yb[2 * y + 1];
    const int* k = yk + (size_t)y * ksize;
    int s0 = 1 << (PIL_PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < n; ++t) {
        const unsigned char* p = mid + ((size_t)(y0 + t) * pitch + x) * 3;
        const int c = k[t];
        s0 += (int)p[0] * c; s1 += (int)p[1] * c; s2 += (int)p[2] * c;
    }
    o[0] = aug_clip8(s0); o[1] = aug_clip8(s1); o[2] = aug_clip8(s2);
}

__global__ __launch_bounds__(256) void aug_crop_mask_kernel(const unsigned char* __restrict__ src, int pitch,
                                                            unsigned char* __restrict__ dst, int h, int w, const int* __restrict__ xtab,
                                                            const int* __restrict__ ytab) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)h * w) return;
    const int y = (int)(i / w), x = (int)(i - (long long)y * w);
    dst[i] = src[(size_t)ytab[y] * pitch + xtab[x]];
}

// ---- entry points -----------------------------------------------------------------------------------------------------------
#define AUG_MAX_SIDE 32768          // Pillow switches code paths at this size (Geometry.c): not restated

#define AUG_CHECK_SIZE(src, dst, h, w)                                                                  \
    YDL_CHECK((src) && (dst) && (src) != (dst), "source and destination must be two distinct buffers"); \
    YDL_CHECK((h) > 0 && (w) > 0 && (h) < AUG_MAX_SIDE && (w) < AUG_MAX_SIDE, "bad image size")

extern "C" int ydl_aug_flip(const void* src, void* dst, int h, int w, int channels, int horizontal, void* stream) {
    AUG_CHECK_SIZE(src, dst, h, w);
    YDL_CHECK(channels == 1 || channels == 3, "1 (label map) or 3 (RGB) channels");
    const long long n = (long long)h * w * channels;
    aug_flip_kernel<<<aug_blocks(n), 256, 0, (hipStream_t)stream>>>((const unsigned char*)src, (unsigned char*)dst, h, w, channels,
                                                                   horizontal ? 1 : 0);
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int ydl_aug_rotate_image(const void* src, void* dst, int h, int w, double a0, double a1, double a2, double a3, double a4,
                                    double a5, void* stream) {
    AUG_CHECK_SIZE(src, dst, h, w);
    aug_rotate_image_kernel<<<aug_blocks((long long)h * w), 256, 0, (hipStream_t)stream>>>((const unsigned char*)src, (unsigned char*)dst,
                                                                                          h, w, a0, a1, a2, a3, a4, a5);
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int ydl_aug_rotate_mask(const void* src, void* dst, int h, int w, int64_t a0, int64_t a1, int64_t a2, int64_t a3, int64_t a4,
                                   int64_t a5, void* stream) {
    AUG_CHECK_SIZE(src, dst, h, w);
    aug_rotate_mask_kernel<<<aug_blocks((long long)h * w), 256, 0, (hipStream_t)stream>>>((const unsigned char*)src, (unsigned char*)dst,
                                                                                         h, w, a0, a1, a2, a3, a4, a5);
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int ydl_aug_brightness(const void* src, void* dst, int h, int w, float factor, void* stream) {
    AUG_CHECK_SIZE(src, dst, h, w);
    const long long n = (long long)h * w * 3;
    aug_brightness_kernel<<<aug_blocks(n), 256, 0, (hipStream_t)stream>>>((const unsigned char*)src, (unsigned char*)dst, n, factor);
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int ydl_aug_contrast(const void* src, void* dst, int h, int w, float factor, void* sum_ws, void* stream) {
    AUG_CHECK_SIZE(src, dst, h, w);
    YDL_CHECK(sum_ws && (((uintptr_t)sum_ws) & 7u) == 0, "the luminance sum and mean need 16 bytes of workspace, 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long npix = (long long)h * w, n = npix * 3;
    if (hipMemsetAsync(sum_ws, 0, 16, st) != hipSuccess) {
        ydl_set_error("ydl_aug_contrast: hipMemsetAsync failed");
        return 2;
    }
    const unsigned blocks = (unsigned)std::min<long long>((npix + 255) / 256, 1024);
    aug_luma_sum_kernel<<<blocks, 256, 0, st>>>((const unsigned char*)src, npix, (unsigned long long*)sum_ws);
    aug_contrast_mean_kernel<<<1, 1, 0, st>>>((unsigned long long*)sum_ws, npix);
    aug_contrast_kernel<<<aug_blocks(n), 256, 0, st>>>((const unsigned char*)src, (unsigned char*)dst, n, factor,
                                                      (const unsigned long long*)sum_ws);
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int ydl_aug_box_blur(const void* src, void* dst, int h, int w, int vertical, int radius, int ww, int fw, void* stream) {
    AUG_CHECK_SIZE(src, dst, h, w);
    YDL_CHECK(radius >= 0 && radius < AUG_MAX_SIDE && ww >= 0 && fw >= 0, "bad box weights");
    aug_box_blur_kernel<<<aug_blocks((long long)h * w), 256, 0, (hipStream_t)stream>>>((const unsigned char*)src, (unsigned char*)dst, h, w,
                                                                                      vertical ? 1 : 0, radius, (unsigned)ww, (unsigned)fw);
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int ydl_aug_crop_image(const void* src, int h, int w, int x1, int y1, int cw, int ch, void* tmp, void* dst,
                                  const int* xbounds, const int* xcoef, int xksize, const int* ybounds, const int* ycoef, int yksize,
                                  void* stream) {
    AUG_CHECK_SIZE(src, dst, h, w);
    YDL_CHECK(x1 >= 0 && y1 >= 0 && cw > 0 && ch > 0 && x1 + cw <= w && y1 + ch <= h, "the crop box leaves the image");
    const bool horiz = cw != w, vert = ch != h;
    YDL_CHECK(!horiz || (tmp && tmp != src && tmp != dst && xbounds && xcoef && xksize > 0),
              "horizontal pass needs tmp and its coefficient tables");
    YDL_CHECK(!vert || (ybounds && ycoef && yksize > 0), "vertical pass needs its coefficient tables");
    hipStream_t st = (hipStream_t)stream;
    const unsigned char* mid = (const unsigned char*)src + ((size_t)y1 * w + x1) * 3;
    int pitch = w;
    if (horiz) {
        aug_crop_h_kernel<<<aug_blocks((long long)ch * w), 256, 0, st>>>(mid, w, ch, (unsigned char*)tmp, w, xbounds, xcoef, xksize);
        mid = (const unsigned char*)tmp;
    }
    aug_crop_v_kernel<<<aug_blocks((long long)h * w), 256, 0, st>>>(mid, pitch, (unsigned char*)dst, h, w, ybounds, ycoef, yksize,
                                                                   vert ? 1 : 0);
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int ydl_aug_crop_mask(const void* src, int h, int w, int x1, int y1, int cw, int ch, void* dst, const int* xtab,
                                 const int* ytab, void* stream) {
    AUG_CHECK_SIZE(src, dst, h, w);
    YDL_CHECK(x1 >= 0 && y1 >= 0 && cw > 0 && ch > 0 && x1 + cw <= w && y1 + ch <= h, "the crop box leaves the image");
    YDL_CHECK(xtab && ytab, "nearest-neighbour index tables missing");
    aug_crop_mask_kernel<<<aug_blocks((long long)h * w), 256, 0, (hipStream_t)stream>>>(
        (const unsigned char*)src + (size_t)y1 * w + x1, w, (unsigned char*)dst, h, w, xtab, ytab);
    YDL_LAUNCH_CHECK();
    return 0;
}
