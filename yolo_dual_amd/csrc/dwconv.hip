// Strided depth-wise convolution for the Ghost blocks (models/common.py:67-70 DWConv, :253-279 GhostConv / GhostBottleneck):
//   * forward, stride 1 or 2, with the BatchNorm partial statistics of the output from the same launch
//   * input gradient in gather form (no atomics)
//   * deterministic weight gradient (per-CTA partials, merged in a fixed order)
// NHWC, f32 / bf16 storage, f32 accumulation; w is the f32 master weight [C][k*k]; k in {1,3,5,7}, p = k/2.
// The stride-1 entry points of dcn_blocks.hip (ydl_dwconv_*) stay as they are: at s = 1 these kernels reproduce them bit for bit
// (same (r, s) tap order, one fmaf per tap), which is what tests/test_gpu_dwconv_strided.py holds them to.
#include "common.h"

#define DW2_RUN 4            // consecutive output pixels per thread: the k input columns they share are loaded once per kernel row
#define DW2_BLOCK_M 64       // pixels per statistics row; must equal ydl_bn_stats_block_m()
#define DW2_WG_BLOCKS 512

// ------------------------------------------------------------------------------------------------------
// forward.  A CTA owns PPC = (256 / cpc) * DW2_RUN consecutive output pixels (a whole number of statistics blocks) for cpc
// 16-byte channel chunks; thread = (run of DW2_RUN consecutive pixels, chunk).  A run inside one output row keeps its
// (DW2_RUN-1)*S + K input columns of a kernel row in registers; a run that crosses a row end takes the tap-by-tap form.
// The weights of the CTA's channels sit in LDS as [tap][channel].  With a statistics workspace the stored (rounded) results go to
// LDS too and one thread per (statistics block, channel) reduces them in pixel order: first the sum, then the fmaf pass about the
// block mean — the arithmetic of bn_stats_kernel, so the rows equal ydl_bn_stats of the stored tensor.
// ------------------------------------------------------------------------------------------------------
template <typename T, int K, int S, bool CHK>
__device__ __forceinline__ void dw2_row_taps(float (&acc)[DW2_RUN][ET<T>::V], const float (&col)[(DW2_RUN - 1) * S + K][ET<T>::V],
                                             const bool (&ok)[(DW2_RUN - 1) * S + K], const float* __restrict__ wrow, int chs) {
    constexpr int V = ET<T>::V;
#pragma unroll
    for (int s = 0; s < K; ++s) {
        float wv[V];
#pragma unroll
        for (int e = 0; e < V; e += 4) *(float4*)(wv + e) = *(const float4*)(wrow + s * chs + e);
#pragma unroll
        for (int o = 0; o < DW2_RUN; ++o) {
            if (CHK && !ok[o * S + s]) continue;
#pragma unroll
            for (int e = 0; e < V; ++e) acc[o][e] = fmaf(wv[e], col[o * S + s][e], acc[o][e]);
        }
    }
}

template <typename T, int K, int S>
__global__ __launch_bounds__(256) void dw2_fwd_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ w, T* __restrict__ y,
                                                      int ldy, float* __restrict__ part, int ldp, int N, int H, int W, int Ho, int Wo,
                                                      int C, int cpp, int cpc) {
    constexpr int V = ET<T>::V, R = DW2_RUN, P = K / 2, NCOL = (R - 1) * S + K, KK = K * K;
    extern __shared__ float smem[];
    const int chs = cpc * V;                       // channels of this CTA
    float* wl = smem;                              // [KK][chs]
    float* yl = smem + KK * chs;                   // [PPC + PPC/64][chs]: one spare row per statistics block spreads the LDS banks
    const int tid = threadIdx.x;
    const int cbase = blockIdx.y * chs;
    for (int i = tid; i < KK * chs; i += 256) {
        const int tap = i / chs, c = cbase + i % chs;
        wl[i] = c < C ? w[(size_t)c * KK + tap] : 0.f;
    }
    __syncthreads();
    const int cq = tid % cpc, run = tid / cpc;
    const int chunk = blockIdx.y * cpc + cq;
    const int c0 = chunk * V, cl0 = cq * V;
    const int ppc = (256 / cpc) * R;
    const long long npix = (long long)N * Ho * Wo;
    const long long q0 = (long long)blockIdx.x * ppc + (long long)run * R;
    if (chunk < cpp && q0 < npix) {
        float acc[R][V];
#pragma unroll
        for (int o = 0; o < R; ++o)
#pragma unroll
            for (int e = 0; e < V; ++e) acc[o][e] = 0.f;
        const int wo = (int)(q0 % Wo);
        const long long t2 = q0 / Wo;
        const int ho = (int)(t2 % Ho);
        const int n = (int)(t2 / Ho);
        if (wo + R <= Wo) {
            const int iw0 = wo * S - P;
            const bool inner = iw0 >= 0 && iw0 + NCOL <= W;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int ih = ho * S + r - P;
                if ((unsigned)ih >= (unsigned)H) continue;
                const T* row = x + ((size_t)n * H + ih) * W * ldx + c0;
                float col[NCOL][V];
                bool ok[NCOL];
#pragma unroll
                for (int j = 0; j < NCOL; ++j) {
                    const int iw = iw0 + j;
                    ok[j] = (unsigned)iw < (unsigned)W;
                    const uint4 u = ok[j] ? *(const uint4*)(row + (size_t)iw * ldx) : make_uint4(0u, 0u, 0u, 0u);
                    unpack16<T>(u, col[j]);
                }
                if (inner) dw2_row_taps<T, K, S, false>(acc, col, ok, wl + r * K * chs + cl0, chs);
                else dw2_row_taps<T, K, S, true>(acc, col, ok, wl + r * K * chs + cl0, chs);
            }
        } else {
#pragma unroll
            for (int o = 0; o < R; ++o) {
                const long long q = q0 + o;
                if (q >= npix) break;
                const int wo2 = (int)(q % Wo);
                const long long t3 = q / Wo;
                const int ho2 = (int)(t3 % Ho);
                const int n2 = (int)(t3 / Ho);
                for (int r = 0; r < K; ++r) {
                    const int ih = ho2 * S + r - P;
                    if ((unsigned)ih >= (unsigned)H) continue;
                    for (int s = 0; s < K; ++s) {
                        const int iw = wo2 * S + s - P;
                        if ((unsigned)iw >= (unsigned)W) continue;
                        float v[V];
                        unpack16<T>(*(const uint4*)(x + (((size_t)n2 * H + ih) * W + iw) * ldx + c0), v);
                        const float* wt = wl + (r * K + s) * chs + cl0;
#pragma unroll
                        for (int e = 0; e < V; ++e) acc[o][e] = fmaf(wt[e], v[e], acc[o][e]);
                    }
                }
            }
        }
#pragma unroll
        for (int o = 0; o < R; ++o) {
            const long long q = q0 + o;
            if (q >= npix) break;
            const uint4 u = pack16<T>(acc[o]);
            T* dst = y + (size_t)q * ldy + c0;
            if (c0 + V <= C) {
                *(uint4*)dst = u;
            } else {                                // last chunk of a C that is no multiple of the chunk: the padding stays untouched
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (c0 + e < C) ET<T>::st(dst + e, acc[o][e]);
            }
            if (part) {                             // the values as stored
                float vr[V];
                unpack16<T>(u, vr);
                const int pl = run * R + o;
                float* d = yl + (size_t)(pl + (pl >> 6)) * chs + cl0;
#pragma unroll
                for (int e = 0; e < V; e += 4) *(float4*)(d + e) = *(const float4*)(vr + e);
            }
        }
    }
    if (!part) return;
    __syncthreads();
    const int nbc = ppc / DW2_BLOCK_M;
    for (int i = tid; i < nbc * chs; i += 256) {
        const int b = i / chs, cl = i % chs, c = cbase + cl;
        const long long gb = (long long)blockIdx.x * nbc + b;
        const long long p0 = gb * DW2_BLOCK_M;
        if (c >= C || p0 >= npix) continue;
        long long p1 = p0 + DW2_BLOCK_M;
        if (p1 > npix) p1 = npix;
        const int cnt = (int)(p1 - p0);
        const float inv = 1.f / (float)(p1 - p0);
        const float* src = yl + (size_t)(b * DW2_BLOCK_M + b) * chs + cl;
        float s = 0.f;
        for (int j = 0; j < cnt; ++j) s += src[j * chs];
        const float mu = s * inv;
        float q = 0.f;
        for (int j = 0; j < cnt; ++j) {
            const float d = src[j * chs] - mu;
            q = fmaf(d, d, q);
        }
        part[((size_t)gb * 2) * ldp + c] = s;
        part[((size_t)gb * 2 + 1) * ldp + c] = q;
    }
}

// a, c: the two activation tensors (16-byte aligned chunks); b: the f32 weight or its gradient
static int dw2_check(int dtype, const void* a, const void* b, const void* c, int lda, int ldc, int N, int H, int W, int C, int k, int s) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "bad dtype");
    YDL_CHECK(a && b && c, "null pointer");
    YDL_CHECK(N > 0 && H > 0 && W > 0 && C > 0, "empty tensor");
    YDL_CHECK(k == 1 || k == 3 || k == 5 || k == 7, "depth-wise conv: k in {1,3,5,7} (padding k/2)");
    YDL_CHECK(s == 1 || s == 2, "depth-wise conv: stride s in {1,2}");
    const int V = dtype == YDL_F32 ? 4 : 8;
    YDL_CHECK(lda >= round_up(C, V) && ldc >= round_up(C, V), "pixel strides must cover C rounded up to a 16-byte chunk");
    YDL_CHECK(lda % V == 0 && ldc % V == 0, "pixel strides must be multiples of a 16-byte chunk");
    YDL_CHECK(aligned16(a) && aligned16(c), "16-byte alignment");
    return 0;
}
static inline int dw2_out(int H, int k, int s) { return (H + 2 * (k / 2) - k) / s + 1; }

template <typename T, int K>
static void dw2_fwd_launch(const void* x, int ldx, const float* w, void* y, int ldy, float* part, int N, int H, int W, int C, int s,
                           hipStream_t st) {
    constexpr int V = ET<T>::V;
    const int Ho = dw2_out(H, K, s), Wo = dw2_out(W, K, s);
    const int cpp = round_up(C, V) / V;
    const int cpc = cpp >= 3 ? 4 : cpp;                      // 1, 2 or 4: the CTA's pixel count stays a multiple of 64
    const int ppc = (256 / cpc) * DW2_RUN;
    const long long npix = (long long)N * Ho * Wo;
    const int chs = cpc * V;
    const size_t lds = sizeof(float) * ((size_t)K * K * chs + (part ? (size_t)(ppc + ppc / DW2_BLOCK_M) * chs : 0));
    dim3 grid((unsigned)((npix + ppc - 1) / ppc), (unsigned)((cpp + cpc - 1) / cpc));
    if (s == 1)
        dw2_fwd_kernel<T, K, 1><<<grid, 256, lds, st>>>((const T*)x, ldx, w, (T*)y, ldy, part, round_up(C, 8), N, H, W, Ho, Wo, C, cpp, cpc);
    else
        dw2_fwd_kernel<T, K, 2><<<grid, 256, lds, st>>>((const T*)x, ldx, w, (T*)y, ldy, part, round_up(C, 8), N, H, W, Ho, Wo, C, cpp, cpc);
}

extern "C" int ydl_dwconv2_fwd(int dtype, const void* x, int ldx, const float* w, void* y, int ldy, float* stats_ws, int N, int H, int W,
                               int C, int k, int s, void* stream) {
    if (int e = dw2_check(dtype, x, w, y, ldx, ldy, N, H, W, C, k, s)) return e;
    YDL_CHECK(DW2_BLOCK_M == ydl_bn_stats_block_m(), "statistics block size");
    hipStream_t st = (hipStream_t)stream;
#define DW2_FWD(KK)                                                                                                        \
    do {                                                                                                                   \
        if (dtype == YDL_F32) dw2_fwd_launch<float, KK>(x, ldx, w, y, ldy, stats_ws, N, H, W, C, s, st);                  \
        else dw2_fwd_launch<bf16_t, KK>(x, ldx, w, y, ldy, stats_ws, N, H, W, C, s, st);                                  \
    } while (0)
    if (k == 1) DW2_FWD(1);
    else if (k == 3) DW2_FWD(3);
    else if (k == 5) DW2_FWD(5);
    else DW2_FWD(7);
    YDL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// input gradient, gather form: dx[n,h,w,c] = sum_{r,t} w[c][r*k+t] * dy[n, (h+p-r)/s, (w+p-t)/s, c] over the taps whose two
// quotients are exact and inside the output.  (H, W) is the INPUT size; thread = one 16-byte chunk of one input pixel.
// ------------------------------------------------------------------------------------------------------
template <typename T, int S>
__global__ __launch_bounds__(256) void dw2_dgrad_kernel(const T* __restrict__ dy, int lddy, const float* __restrict__ w, T* __restrict__ dx,
                                                        int lddx, int accumulate, int N, int H, int W, int Ho, int Wo, int Cp, int C, int k,
                                                        int p) {
    constexpr int V = ET<T>::V;
    const int cpp = Cp / V;
    const long long total = (long long)N * H * W * cpp;
    const int kk = k * k;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int cq = (int)(i % cpp);
        const long long pix = i / cpp;
        const int wx = (int)(pix % W);
        const long long t2 = pix / W;
        const int hy = (int)(t2 % H);
        const int n = (int)(t2 / H);
        const int c0 = cq * V;
        float acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0.f;
        for (int r = 0; r < k; ++r) {
            const int th = hy - r + p;
            if (th < 0 || th % S != 0) continue;
            const int oh = th / S;
            if (oh >= Ho) continue;
            for (int t = 0; t < k; ++t) {
                const int tw = wx - t + p;
                if (tw < 0 || tw % S != 0) continue;
                const int ow = tw / S;
                if (ow >= Wo) continue;
                float v[V];
                unpack16<T>(*(const uint4*)(dy + (((size_t)n * Ho + oh) * Wo + ow) * lddy + c0), v);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float wv = (c0 + e) < C ? w[(size_t)(c0 + e) * kk + r * k + t] : 0.f;
                    acc[e] = fmaf(wv, v[e], acc[e]);
                }
            }
        }
        T* dst = dx + (size_t)pix * lddx + c0;
        if (c0 + V <= C) {
            if (accumulate) {
                float o[V];
                unpack16<T>(*(const uint4*)dst, o);
#pragma unroll
                for (int e = 0; e < V; ++e) acc[e] += o[e];
            }
            *(uint4*)dst = pack16<T>(acc);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (c0 + e < C) {
                    if (accumulate) acc[e] += ET<T>::ld(dst + e);
                    ET<T>::st(dst + e, acc[e]);
                }
        }
    }
}

extern "C" int ydl_dwconv2_dgrad(int dtype, const void* dy, int lddy, const float* w, void* dx, int lddx, int accumulate, int N, int H,
                                 int W, int C, int k, int s, void* stream) {
    if (int e = dw2_check(dtype, dy, w, dx, lddy, lddx, N, H, W, C, k, s)) return e;
    const int V = dtype == YDL_F32 ? 4 : 8, Cp = round_up(C, V), p = k / 2;
    const int Ho = dw2_out(H, k, s), Wo = dw2_out(W, k, s);
    hipStream_t st = (hipStream_t)stream;
    long long blocks = ((long long)N * H * W * (Cp / V) + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    const int grid = (int)blocks;
#define DW2_DG(TT, SS)                                                                                                            \
    dw2_dgrad_kernel<TT, SS><<<grid, 256, 0, st>>>((const TT*)dy, lddy, w, (TT*)dx, lddx, accumulate, N, H, W, Ho, Wo, Cp, C, k, p)
    if (dtype == YDL_F32) {
        if (s == 1) DW2_DG(float, 1);
        else DW2_DG(float, 2);
    } else {
        if (s == 1) DW2_DG(bf16_t, 1);
        else DW2_DG(bf16_t, 2);
    }
    YDL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// weight gradient: dw[c][r*k+t] += sum_{n,ho,wo} dy[n,ho,wo,c] * x[n, ho*s+r-p, wo*s+t-p, c].  Thread = (16-byte channel chunk,
// kernel row r, pixel lane): K x V accumulators.  CTA b walks the output pixels b*RL + lane, + gridDim.x*RL, ...; the lanes are folded
// through LDS in lane order, one tap column at a time, into part[b][c][tap]; dw2_wgrad_merge_kernel adds the partials in CTA order.
// ------------------------------------------------------------------------------------------------------
template <typename T, int K, int S>
__global__ __launch_bounds__(256) void dw2_wgrad_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ dy, int lddy,
                                                        float* __restrict__ part, int N, int H, int W, int Ho, int Wo, int C, int cpp,
                                                        int cpb, int RL) {
    constexpr int V = ET<T>::V, P = K / 2;
    const int tid = threadIdx.x;
    const int cq = tid % cpb, rr = (tid / cpb) % K, pl = tid / (cpb * K);
    const int chunk = blockIdx.y * cpb + cq;
    const bool live = pl < RL && chunk < cpp;
    const int c0 = chunk * V;
    const long long npix = (long long)N * Ho * Wo;
    float acc[K][V];
#pragma unroll
    for (int t = 0; t < K; ++t)
#pragma unroll
        for (int e = 0; e < V; ++e) acc[t][e] = 0.f;
    if (live) {
        for (long long pix = (long long)blockIdx.x * RL + pl; pix < npix; pix += (long long)gridDim.x * RL) {
            const int wo = (int)(pix % Wo);
            const long long t2 = pix / Wo;
            const int ho = (int)(t2 % Ho);
            const int n = (int)(t2 / Ho);
            const int ih = ho * S + rr - P;
            if ((unsigned)ih >= (unsigned)H) continue;
            float g[V];
            unpack16<T>(*(const uint4*)(dy + (size_t)pix * lddy + c0), g);
            const T* row = x + ((size_t)n * H + ih) * W * ldx + c0;
#pragma unroll
            for (int t = 0; t < K; ++t) {
                const int iw = wo * S + t - P;
                const bool ok = (unsigned)iw < (unsigned)W;
                float xv[V];
                unpack16<T>(ok ? *(const uint4*)(row + (size_t)iw * ldx) : make_uint4(0u, 0u, 0u, 0u), xv);
#pragma unroll
                for (int e = 0; e < V; ++e) acc[t][e] = fmaf(g[e], xv[e], acc[t][e]);
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

__global__ __launch_bounds__(256) void dw2_wgrad_merge_kernel(const float* __restrict__ part, float* __restrict__ dw, int nblk, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int b = 0; b < nblk; ++b) s += part[(size_t)b * n + i];
    dw[i] += s;
}

template <typename T, int K>
static int dw2_wgrad_launch(const void* x, int ldx, const void* dy, int lddy, float* ws, int N, int H, int W, int C, int s, hipStream_t st) {
    constexpr int V = ET<T>::V;
    const int Ho = dw2_out(H, K, s), Wo = dw2_out(W, K, s);
    const int cpp = round_up(C, V) / V;
    const int cpb = cpp < 32 ? cpp : 32;
    const int RL = 256 / (cpb * K);
    const long long npix = (long long)N * Ho * Wo;
    long long gx = (npix + RL - 1) / RL;
    if (gx > DW2_WG_BLOCKS) gx = DW2_WG_BLOCKS;
    dim3 grid((unsigned)gx, (unsigned)((cpp + cpb - 1) / cpb));
    if (s == 1) dw2_wgrad_kernel<T, K, 1><<<grid, 256, 0, st>>>((const T*)x, ldx, (const T*)dy, lddy, ws, N, H, W, Ho, Wo, C, cpp, cpb, RL);
    else dw2_wgrad_kernel<T, K, 2><<<grid, 256, 0, st>>>((const T*)x, ldx, (const T*)dy, lddy, ws, N, H, W, Ho, Wo, C, cpp, cpb, RL);
    return (int)gx;
}

extern "C" int64_t ydl_dwconv2_wgrad_ws_bytes(int C, int k) { return (int64_t)DW2_WG_BLOCKS * C * k * k * (int64_t)sizeof(float); }
extern "C" int ydl_dwconv2_wgrad(int dtype, const void* x, int ldx, const void* dy, int lddy, float* dw, float* ws, int N, int H, int W,
                                 int C, int k, int s, void* stream) {
    if (int e = dw2_check(dtype, x, dw, dy, ldx, lddy, N, H, W, C, k, s)) return e;
    YDL_CHECK(ws != nullptr, "workspace of ydl_dwconv2_wgrad_ws_bytes() required");
    hipStream_t st = (hipStream_t)stream;
    int nblk = 0;
#define DW2_WG(KK)                                                                                                   \
    do {                                                                                                             \
        if (dtype == YDL_F32) nblk = dw2_wgrad_launch<float, KK>(x, ldx, dy, lddy, ws, N, H, W, C, s, st);          \
        else nblk = dw2_wgrad_launch<bf16_t, KK>(x, ldx, dy, lddy, ws, N, H, W, C, s, st);                          \
    } while (0)
    if (k == 1) DW2_WG(1);
    else if (k == 3) DW2_WG(3);
    else if (k == 5) DW2_WG(5);
    else DW2_WG(7);
    const int n = C * k * k;
    dw2_wgrad_merge_kernel<<<(n + 255) / 256, 256, 0, st>>>(ws, dw, nblk, n);
    YDL_LAUNCH_CHECK();
    return 0;
}
