// Space-to-depth / depth-to-space on interior NHWC tensors (ydl_space_to_depth / ydl_depth_to_space): Focus, Contract and Expand of
// models/common.py:241-250, :282-307.  Pure byte movers; each entry point is the other's backward.
//
// Both directions are one index map between a FINE tensor (N, Hc*s, Wc*s, C) and a COARSE tensor (N, Hc, Wc, s*s*C):
//   coarse[n, hc, wc, blk(sy, sx)*C + c]  <->  fine[n, hc*s + sy, wc*s + sx, c],   blk = sy*s + sx (order 0) or sx*s + sy (order 1)
// Work is enumerated in the COARSE tensor's order, one coarse row (n, hc) per blockIdx.y step: consecutive lanes walk the s*s*C
// channels of a coarse pixel and then the next pixel of the row, so the coarse side is one contiguous run per pixel row and, on the
// fine side, each group of C/V lanes covers the whole channel row of one fine pixel.  No lane strides by a pixel.  The vector form
// moves 16-byte chunks (C, both row strides and both base pointers whole chunks); the element form serves everything else (C = 3
// under Focus, C = 12 where the blocks start at 24-byte offsets in bf16).  Every output element has exactly one source: no atomics,
// the same launch in throughput and deterministic mode.  accumulate adds in f32 with one rounding.
#include "common.h"

template <typename T, bool VEC, bool S2D>
__global__ __launch_bounds__(256) void s2d_kernel(const T* __restrict__ x, int ldx, T* __restrict__ y, int ldy, int rows, int Wc,
                                                  int C, int s, int order, int accumulate) {
    constexpr int V = VEC ? ET<T>::V : 1;
    const unsigned cpc = (unsigned)(C / V);           // chunks per block of C channels
    const unsigned ss = (unsigned)(s * s);
    const unsigned rowlen = (unsigned)Wc * ss * cpc;   // checked by the launcher to fit 31 bits
    const int ldf = S2D ? ldx : ldy, ldc = S2D ? ldy : ldx;
    const long long Wf = (long long)Wc * s;
    for (int r = blockIdx.y; r < rows; r += gridDim.y) {              // r = n * Hc + hc; the fine rows r*s .. r*s + s-1 belong to it
        for (unsigned j = blockIdx.x * 256u + threadIdx.x; j < rowlen; j += gridDim.x * 256u) {
            const unsigned q = j % cpc, t = j / cpc;
            const unsigned blk = t % ss, wc = t / ss;
            const unsigned hi = blk / (unsigned)s, lo = blk - hi * (unsigned)s;
            const unsigned sy = order ? lo : hi, sx = order ? hi : lo;
            const size_t co = ((size_t)r * Wc + wc) * (size_t)ldc + (size_t)blk * C + (size_t)q * V;
            const size_t fo = (((size_t)r * s + sy) * (size_t)Wf + (size_t)wc * s + sx) * (size_t)ldf + (size_t)q * V;
            const T* src = x + (S2D ? fo : co);
            T* dst = y + (S2D ? co : fo);
            if (VEC) {
                uint4 v = *(const uint4*)src;
                if (accumulate) {
                    float a[ET<T>::V], b[ET<T>::V];
                    unpack16<T>(v, a);
                    unpack16<T>(*(const uint4*)dst, b);
#pragma unroll
                    for (int e = 0; e < ET<T>::V; ++e) a[e] += b[e];
                    v = pack16<T>(a);
                }
                *(uint4*)dst = v;
            } else if (accumulate) {
                ET<T>::st(dst, ET<T>::ld(src) + ET<T>::ld(dst));
            } else {
                *dst = *src;
            }
        }
    }
}

template <bool S2D>
static int s2d_launch(const char* who, int dtype, const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, int s, int order,
                      int accumulate, void* stream) {
    // H and W are x's size, C the width of one channel block: x is (N, H, W, C) for space-to-depth, (N, H, W, s*s*C) for depth-to-space
    const long long ss = (long long)s * s;
    const int Hc = S2D ? H / s : H, Wc = S2D ? W / s : W;
    const int V = dtype == YDL_F32 ? 4 : 8;
    const bool vec = C % V == 0 && ldx % V == 0 && ldy % V == 0 && aligned16(x) && aligned16(y);
    const long long rowlen = (long long)Wc * ss * (vec ? C / V : C);
    const long long rows = (long long)N * Hc;
    if (rowlen >= (1ll << 31) || rows >= (1ll << 31)) {
        ydl_set_error(std::string(who) + ": tensor too large (a coarse row or the row count exceeds 31 bits)");
        return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    long long gx = (rowlen + 255) / 256, gy = rows;
    if (gx > 4096) gx = 4096;
    if (gy > 65535) gy = 65535;
    dim3 grid((unsigned)gx, (unsigned)gy);
#define YDL_S2D_GO(T, VEC) s2d_kernel<T, VEC, S2D><<<grid, 256, 0, st>>>((const T*)x, ldx, (T*)y, ldy, (int)rows, Wc, C, s, order, accumulate)
    if (dtype == YDL_F32) { if (vec) YDL_S2D_GO(float, true); else YDL_S2D_GO(float, false); }
    else { if (vec) YDL_S2D_GO(bf16_t, true); else YDL_S2D_GO(bf16_t, false); }
#undef YDL_S2D_GO
    hipError_t e_ = hipGetLastError();
    if (e_ != hipSuccess) {
        ydl_set_error(std::string(who) + ": launch failed: " + hipGetErrorString(e_));
        return 2;
    }
    return 0;
}

extern "C" int ydl_space_to_depth(int dtype, const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, int s, int order,
                                  int accumulate, void* stream) {
    YDL_CHECK((dtype == YDL_F32 || dtype == YDL_BF16) && x && y && N >= 1 && H >= 1 && W >= 1 && C >= 1, "bad arguments");
    YDL_CHECK(s >= 1 && s <= 64, "the block size s must be in 1..64");
    YDL_CHECK(order == 0 || order == 1, "order must be 0 (sy*s + sx) or 1 (sx*s + sy)");
    YDL_CHECK(H % s == 0 && W % s == 0, "H and W must be multiples of s");
    YDL_CHECK((long long)s * s * C < (1ll << 31), "s*s*C exceeds 31 bits");
    YDL_CHECK(ldx >= C && ldy >= s * s * C, "row strides must cover C (x) and s*s*C (y)");
    return s2d_launch<true>(__func__, dtype, x, ldx, y, ldy, N, H, W, C, s, order, accumulate, stream);
}

extern "C" int ydl_depth_to_space(int dtype, const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, int s, int order,
                                  int accumulate, void* stream) {
    YDL_CHECK((dtype == YDL_F32 || dtype == YDL_BF16) && x && y && N >= 1 && H >= 1 && W >= 1 && C >= 1, "bad arguments");
    YDL_CHECK(s >= 1 && s <= 64, "the block size s must be in 1..64");
    YDL_CHECK(order == 0 || order == 1, "order must be 0 (sy*s + sx) or 1 (sx*s + sy)");
    YDL_CHECK((long long)s * s * C < (1ll << 31), "s*s*C exceeds 31 bits");
    YDL_CHECK(ldx >= s * s * C && ldy >= C, "row strides must cover s*s*C (x) and C (y)");
    return s2d_launch<false>(__func__, dtype, x, ldx, y, ldy, N, H, W, C, s, order, accumulate, stream);
}
