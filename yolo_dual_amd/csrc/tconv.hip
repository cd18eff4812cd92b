// Depth-wise transposed convolution, stride 2 (DWConvTranspose2d, models/common.py:73-76), NHWC, in the three forms that double
// the map exactly: (k, p, output_padding) in {(2,0,0), (4,1,0), (3,1,1)} => Ho = 2H, Wo = 2W.  VALU kernels in the style of
// dwconv.hip: a thread owns one 16-byte channel chunk, the f32 master weight [C][k*k] is read directly (staged once per CTA in LDS,
// transposed to [tap][channel] so a thread reads its chunk's taps as contiguous floats), f32 accumulation, any pixel strides (the
// tensors may be channel slices of wider buffers).  HBM-bound: the forward reads x once (each input pixel feeds k*k outputs, but
// neighbouring outputs of a CTA's rows share them in L1/L2) and writes y once.
//   y [n,oh,ow,c] = b[c] + sum_{r,t} x[n,(oh+p-r)/2,(ow+p-t)/2,c] * w[c][r*k+t]     taps with exact quotients inside the input
//   dx[n,i,j,c]   = sum_{r,t} dy[n,2i-p+r,2j-p+t,c] * w[c][r*k+t]                   taps inside the output
//   dw[c][r*k+t] += sum_{n,i,j} x[n,i,j,c] * dy[n,2i-p+r,2j-p+t,c]
#include "common.h"

#define DWT_CPB 32           // 16-byte channel chunks per CTA (LDS weight tile: 16 taps x 32 chunks x 8 channels x 4 B = 16 KiB)
#define DWT_WG_BLOCKS 512    // partial rows of the weight gradient

extern "C" int ydl_dwtconv_supported(int C, int k, int s, int p, int op) {
    if (C <= 0 || C % 8 != 0 || s != 2) return 0;
    return (k == 2 && p == 0 && op == 0) || (k == 4 && p == 1 && op == 0) || (k == 3 && p == 1 && op == 1);
}

// the CTA's weight tile: wl[tap][cl] = w[(cbase + cl)][tap] for cl < chs (zero beyond C)
template <int K>
__device__ __forceinline__ void dwt_stage_weights(float* wl, const float* __restrict__ w, int cbase, int chs, int C) {
    for (int idx = threadIdx.x; idx < K * K * chs; idx += 256) {
        const int tap = idx / chs, c = cbase + idx % chs;
        wl[idx] = c < C ? w[(size_t)c * (K * K) + tap] : 0.f;
    }
    __syncthreads();
}

// forward: a CTA walks whole output rows (n, oh); thread = (chunk, output column lane).  The row's parity picks the kernel rows
// r = ((oh + p) & 1) + 2 rr, the column's parity the kernel columns: ceil(K/2)^2 taps per output at most, added r then t ascending
// onto the bias.
template <typename T, int K>
__global__ __launch_bounds__(256) void dwt_fwd_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ w,
                                                      const float* __restrict__ bias, T* __restrict__ y, int ldy, int H, int W, int C,
                                                      int cpp, int cpb, int nrows) {
    constexpr int V = ET<T>::V, P = K == 2 ? 0 : 1, HK = (K + 1) / 2;
    __shared__ __attribute__((aligned(16))) float wl[16 * DWT_CPB * 8];
    const int R = 256 / cpb, chs = cpb * V;
    const int cq = threadIdx.x % cpb, pl = threadIdx.x / cpb;
    const int chunk = blockIdx.y * cpb + cq;
    dwt_stage_weights<K>(wl, w, blockIdx.y * chs, chs, C);
    if (!(pl < R && chunk < cpp)) return;
    const int c0 = chunk * V, Ho = 2 * H, Wo = 2 * W;
    float bv[V];
#pragma unroll
    for (int e = 0; e < V; ++e) bv[e] = bias ? bias[c0 + e] : 0.f;
    const float* wc = wl + cq * V;
    for (int row = blockIdx.x; row < nrows; row += gridDim.x) {
        const int n = row / Ho, oh = row - n * Ho;
        const T* xb = x + (size_t)n * H * W * ldx + c0;
        T* yrow = y + (size_t)row * Wo * ldy + c0;
        const int r0 = (oh + P) & 1;
        for (int ow = pl; ow < Wo; ow += R) {
            const int t0 = (ow + P) & 1;
            float acc[V];
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] = bv[e];
#pragma unroll
            for (int rr = 0; rr < HK; ++rr) {
                const int r = r0 + 2 * rr, th = oh + P - r;
                if (r >= K || th < 0 || (th >> 1) >= H) continue;
                const T* xr = xb + (size_t)(th >> 1) * W * ldx;
#pragma unroll
                for (int tt = 0; tt < HK; ++tt) {
                    const int t = t0 + 2 * tt, tw = ow + P - t;
                    if (t >= K || tw < 0 || (tw >> 1) >= W) continue;
                    float v[V];
                    unpack16<T>(*(const uint4*)(xr + (size_t)(tw >> 1) * ldx), v);
                    const float* wt = wc + (r * K + t) * chs;
#pragma unroll
                    for (int e = 0; e < V; ++e) acc[e] = fmaf(v[e], wt[e], acc[e]);
                }
            }
            *(uint4*)(yrow + (size_t)ow * ldy) = pack16<T>(acc);
        }
    }
}

// input gradient: a CTA walks whole input rows (n, i); dx = the stride-2 depth-wise convolution of dy, in-range taps only, added
// r then t ascending; the previous contents of dx are added last (accumulate)
template <typename T, int K>
__global__ __launch_bounds__(256) void dwt_dgrad_kernel(const T* __restrict__ dy, int lddy, const float* __restrict__ w, T* __restrict__ dx,
                                                        int lddx, int accumulate, int H, int W, int C, int cpp, int cpb, int nrows) {
    constexpr int V = ET<T>::V, P = K == 2 ? 0 : 1;
    __shared__ __attribute__((aligned(16))) float wl[16 * DWT_CPB * 8];
    const int R = 256 / cpb, chs = cpb * V;
    const int cq = threadIdx.x % cpb, pl = threadIdx.x / cpb;
    const int chunk = blockIdx.y * cpb + cq;
    dwt_stage_weights<K>(wl, w, blockIdx.y * chs, chs, C);
    if (!(pl < R && chunk < cpp)) return;
    const int c0 = chunk * V, Ho = 2 * H, Wo = 2 * W;
    const float* wc = wl + cq * V;
    for (int row = blockIdx.x; row < nrows; row += gridDim.x) {
        const int n = row / H, i = row - n * H;
        const T* db = dy + (size_t)n * Ho * Wo * lddy + c0;
        T* xrow = dx + (size_t)row * W * lddx + c0;
        for (int j = pl; j < W; j += R) {
            float acc[V];
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e] = 0.f;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int oh = 2 * i - P + r;
                if ((unsigned)oh >= (unsigned)Ho) continue;
                const T* dr = db + (size_t)oh * Wo * lddy;
#pragma unroll
                for (int t = 0; t < K; ++t) {
                    const int ow = 2 * j - P + t;
                    if ((unsigned)ow >= (unsigned)Wo) continue;
                    float v[V];
                    unpack16<T>(*(const uint4*)(dr + (size_t)ow * lddy), v);
                    const float* wt = wc + (r * K + t) * chs;
#pragma unroll
                    for (int e = 0; e < V; ++e) acc[e] = fmaf(v[e], wt[e], acc[e]);
                }
            }
            T* dst = xrow + (size_t)j * lddx;
            if (accumulate) {
                float o[V];
                unpack16<T>(*(const uint4*)dst, o);
#pragma unroll
                for (int e = 0; e < V; ++e) acc[e] += o[e];
            }
            *(uint4*)dst = pack16<T>(acc);
        }
    }
}

// weight gradient, the dw2_wgrad_kernel form with the roles of the two tensors exchanged: thread = (chunk, kernel row r, pixel lane),
// K x V accumulators; CTA b walks the INPUT pixels b*RL + lane, + gridDim.x*RL, ...; the lanes are folded through LDS in lane order
// into part[b][c][tap]; dwt_wgrad_merge_kernel adds the partials in CTA order => bitwise reproducible.
template <typename T, int K>
__global__ __launch_bounds__(256) void dwt_wgrad_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ dy, int lddy,
                                                        float* __restrict__ part, int N, int H, int W, int C, int cpp, int cpb, int RL) {
    constexpr int V = ET<T>::V, P = K == 2 ? 0 : 1;
    const int tid = threadIdx.x;
    const int cq = tid % cpb, rr = (tid / cpb) % K, pl = tid / (cpb * K);
    const int chunk = blockIdx.y * cpb + cq;
    const bool live = pl < RL && chunk < cpp;
    const int c0 = chunk * V, Ho = 2 * H, Wo = 2 * W;
    const long long npix = (long long)N * H * W;
    float acc[K][V];
#pragma unroll
    for (int t = 0; t < K; ++t)
#pragma unroll
        for (int e = 0; e < V; ++e) acc[t][e] = 0.f;
    if (live) {
        for (long long pix = (long long)blockIdx.x * RL + pl; pix < npix; pix += (long long)gridDim.x * RL) {
            const int j = (int)(pix % W);
            const long long t2 = pix / W;
            const int i = (int)(t2 % H);
            const int n = (int)(t2 / H);
            const int oh = 2 * i - P + rr;
            if ((unsigned)oh >= (unsigned)Ho) continue;
            float xv[V];
            unpack16<T>(*(const uint4*)(x + (size_t)pix * ldx + c0), xv);
            const T* row = dy + ((size_t)n * Ho + oh) * Wo * lddy + c0;
#pragma unroll
            for (int t = 0; t < K; ++t) {
                const int ow = 2 * j - P + t;
                const bool ok = (unsigned)ow < (unsigned)Wo;
                float g[V];
                unpack16<T>(ok ? *(const uint4*)(row + (size_t)ow * lddy) : make_uint4(0u, 0u, 0u, 0u), g);
#pragma unroll
                for (int e = 0; e < V; ++e) acc[t][e] = fmaf(xv[e], g[e], acc[t][e]);
            }
        }
    }
    __shared__ float red[256 * 8];
#pragma unroll
    for (int t = 0; t < K; ++t) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < V; ++e) red[tid * V + e] = acc[t][e];
        __syncthreads();
        if (pl == 0 && chunk < cpp) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float a = 0.f;
                for (int l = 0; l < RL; ++l) a += red[((l * K + rr) * cpb + cq) * V + e];
                const int c = c0 + e;
                if (c < C) part[((size_t)blockIdx.x * C + c) * (K * K) + rr * K + t] = a;
            }
        }
    }
}

__global__ __launch_bounds__(256) void dwt_wgrad_merge_kernel(const float* __restrict__ part, float* __restrict__ dw, int nblk, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
#pragma unroll 16
    for (int b = 0; b < nblk; ++b) s += part[(size_t)b * n + i];          // (unrolled: the loads of 16 partials are in flight together; the order of the additions stays b ascending)
    dw[i] += s;
}

// a, c: the two activation tensors (lda the stride of the (H, W) one, ldc of the (2H, 2W) one); b: the f32 weight or its gradient
static int dwt_check(int dtype, const void* a, const void* b, const void* c, int lda, int ldc, int N, int H, int W, int C, int k, int p,
                     int op) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "bad dtype");
    YDL_CHECK(a && b && c, "null pointer");
    YDL_CHECK(N > 0 && H > 0 && W > 0, "empty tensor");
    YDL_CHECK(ydl_dwtconv_supported(C, k, 2, p, op), "depth-wise transposed conv: stride 2, (k, p, output_padding) in {(2,0,0), (4,1,0), (3,1,1)}, C a multiple of 8");
    const int V = dtype == YDL_F32 ? 4 : 8;
    YDL_CHECK(lda >= C && ldc >= C && lda % V == 0 && ldc % V == 0, "pixel strides must cover C and be multiples of a 16-byte chunk");
    YDL_CHECK(aligned16(a) && aligned16(c), "16-byte alignment");
    YDL_CHECK((long long)N * H < (1ll << 29), "too many rows");
    return 0;
}

#define DWT_BY_K(CALL)                 \
    do {                               \
        if (k == 2) { CALL(2); }       \
        else if (k == 3) { CALL(3); }  \
        else { CALL(4); }              \
    } while (0)

static inline dim3 dwt_row_grid(int nrows, int cpp, int cpb) {
    return dim3((unsigned)(nrows < 4096 ? nrows : 4096), (unsigned)((cpp + cpb - 1) / cpb));
}

extern "C" int ydl_dwtconv_fwd(int dtype, const void* x, int ldx, const float* w, const float* bias, void* y, int ldy, int N, int H, int W,
                               int C, int k, int p, int op, void* stream) {
    if (int e = dwt_check(dtype, x, w, y, ldx, ldy, N, H, W, C, k, p, op)) return e;
    hipStream_t st = (hipStream_t)stream;
    const int V = dtype == YDL_F32 ? 4 : 8, cpp = C / V, cpb = cpp < DWT_CPB ? cpp : DWT_CPB, nrows = N * 2 * H;
    const dim3 grid = dwt_row_grid(nrows, cpp, cpb);
#define DWT_FWD(KK)                                                                                                                  \
    if (dtype == YDL_F32) dwt_fwd_kernel<float, KK><<<grid, 256, 0, st>>>((const float*)x, ldx, w, bias, (float*)y, ldy, H, W, C, cpp, cpb, nrows); \
    else dwt_fwd_kernel<bf16_t, KK><<<grid, 256, 0, st>>>((const bf16_t*)x, ldx, w, bias, (bf16_t*)y, ldy, H, W, C, cpp, cpb, nrows)
    DWT_BY_K(DWT_FWD);
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int ydl_dwtconv_dgrad(int dtype, const void* dy, int lddy, const float* w, void* dx, int lddx, int accumulate, int N, int H,
                                 int W, int C, int k, int p, int op, void* stream) {
    if (int e = dwt_check(dtype, dx, w, dy, lddx, lddy, N, H, W, C, k, p, op)) return e;
    hipStream_t st = (hipStream_t)stream;
    const int V = dtype == YDL_F32 ? 4 : 8, cpp = C / V, cpb = cpp < DWT_CPB ? cpp : DWT_CPB, nrows = N * H;
    const dim3 grid = dwt_row_grid(nrows, cpp, cpb);
#define DWT_DG(KK)                                                                                                                   \
    if (dtype == YDL_F32) dwt_dgrad_kernel<float, KK><<<grid, 256, 0, st>>>((const float*)dy, lddy, w, (float*)dx, lddx, accumulate, H, W, C, cpp, cpb, nrows); \
    else dwt_dgrad_kernel<bf16_t, KK><<<grid, 256, 0, st>>>((const bf16_t*)dy, lddy, w, (bf16_t*)dx, lddx, accumulate, H, W, C, cpp, cpb, nrows)
    DWT_BY_K(DWT_DG);
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t ydl_dwtconv_wgrad_ws_bytes(int C, int k) { return (int64_t)DWT_WG_BLOCKS * C * k * k * (int64_t)sizeof(float); }
extern "C" int ydl_dwtconv_wgrad(int dtype, const void* x, int ldx, const void* dy, int lddy, float* dw, float* ws, int N, int H, int W,
                                 int C, int k, int p, int op, void* stream) {
    if (int e = dwt_check(dtype, x, dw, dy, ldx, lddy, N, H, W, C, k, p, op)) return e;
    YDL_CHECK(ws != nullptr, "workspace of ydl_dwtconv_wgrad_ws_bytes() required");
    hipStream_t st = (hipStream_t)stream;
    const int V = dtype == YDL_F32 ? 4 : 8, cpp = C / V, cpb = cpp < DWT_CPB ? cpp : DWT_CPB;
    const int RL = 256 / (cpb * k);
    const long long npix = (long long)N * H * W;
    long long gx = (npix + RL - 1) / RL;
    if (gx > DWT_WG_BLOCKS) gx = DWT_WG_BLOCKS;
    const dim3 grid((unsigned)gx, (unsigned)((cpp + cpb - 1) / cpb));
#define DWT_WG(KK)                                                                                                                   \
    if (dtype == YDL_F32) dwt_wgrad_kernel<float, KK><<<grid, 256, 0, st>>>((const float*)x, ldx, (const float*)dy, lddy, ws, N, H, W, C, cpp, cpb, RL); \
    else dwt_wgrad_kernel<bf16_t, KK><<<grid, 256, 0, st>>>((const bf16_t*)x, ldx, (const bf16_t*)dy, lddy, ws, N, H, W, C, cpp, cpb, RL)
    DWT_BY_K(DWT_WG);
    const int n = C * k * k;
    dwt_wgrad_merge_kernel<<<(n + 255) / 256, 256, 0, st>>>(ws, dw, (int)gx, n);
    YDL_LAUNCH_CHECK();
    return 0;
}
