// Grouped convolution (1 < groups < channels) as implicit GEMM on MFMA: models/common.py:1451-1468 SPPCSPC_group, and every
// Conv / Bottleneck / C3 / C2f built with g > 1.  NHWC, f32 or bf16 storage, f32 accumulation, no atomics anywhere.
//
// Served set (ydl_gconv_supported): groups >= 2, Cin/groups and Cout/groups multiples of 16 (a 16-column MFMA tile and a 16-channel
// K piece never straddle a group, no weight padding exists), k in {1, 3}, s = 1, p = k/2, ldw = 0.
//
// Structure: plain LDS-staged tile kernels, ONE launch for all groups — the group is part of blockIdx.y.
//   * forward / input gradient (gconv_kernel): a CTA owns 64 pixels x 16*NT output channels of one group.  K = k*k*(channels per
//     group) is walked in stages of 128 bytes per row: 16-byte pieces of the im2col row (pixels) and of the weight row go global ->
//     registers -> LDS (the next stage's loads are in flight while this stage's MFMAs run), fragments come back as ds_read_b128.
//     The weight tile is the MFMA A operand and the pixel tile the B operand, so a lane ends up with FOUR CONSECUTIVE CHANNELS of
//     one pixel: an 8- or 16-byte store.  The input gradient is the same kernel on (dy, wt) with the taps mirrored.
//   * weight gradient (gconv_wgrad_kernel): a CTA owns (pixel split, group, tap, <=64 x <=64 channel tile); dy and the shifted x
//     are transposed on their way into LDS ([channel][pixel]) so that the pixel index is the MFMA K; every CTA stores its partial
//     tile into the workspace and gconv_merge_kernel adds the splits into dw in a fixed order.
#include "conv_common.h"

#define GC_BM 64                 // pixels per CTA = pixels per BatchNorm statistics row
#define GC_KB 128                // bytes of K per row and stage: two 64-byte MFMA chunks (2 x 32 bf16, 2 x 16 f32)
#define GC_ROW (GC_KB + 16)      // LDS row stride: one 16-byte slot of padding spreads the rows over the banks
#define GW_PB 64                 // weight gradient: pixels per step
#define GW_MAX_SPLITS 64

struct GcPix { int n, h, w, ok; };

// ------------------------------------------------------------------------------------------------------
// forward (DGRAD = false): dst[pix][grp*Cdg + c] = sum_{tap, cs} src[pix + tap][grp*Csg + cs] * w[grp*Cdg + c][tap][cs]
// input gradient (DGRAD = true): the same sum over mirrored taps with w = wt [Cin][k*k][Cout/groups]
// ------------------------------------------------------------------------------------------------------
template <typename T, int NT, bool DGRAD>
__global__ __launch_bounds__(256) void gconv_kernel(const T* __restrict__ src, int lds_, const T* __restrict__ w, T* __restrict__ dst,
                                                    int ldd, float* __restrict__ part, int ldp, int npix, int H, int W, int k, int Csg,
                                                    int Cdg, int accumulate) {
    constexpr int ES = sizeof(T), BN = 16 * NT;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * GC_BM * GC_ROW];
    unsigned char* Ps = smem;                         // [64 pixels][GC_ROW]
    unsigned char* Ws = smem + GC_BM * GC_ROW;        // [BN weight rows][GC_ROW]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int chunks = Cdg / BN;
    const int grp = blockIdx.y / chunks, chunk = blockIdx.y - grp * chunks;
    const int col0 = grp * Cdg + chunk * BN;          // first destination channel of this CTA
    const int K = k * k * Csg, p = k >> 1;
    const int nst = (K * ES + GC_KB - 1) / GC_KB;
    const int pc = tid & 7, r0 = tid >> 3;            // this thread stages piece pc of rows r0 and r0 + 32

    GcPix px[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long long q = (long long)blockIdx.x * GC_BM + r0 + 32 * i;
        px[i].ok = q < npix;
        const long long qq = px[i].ok ? q : 0;
        px[i].w = (int)(qq % W);
        const long long t = qq / W;
        px[i].h = (int)(t % H);
        px[i].n = (int)(t / H);
    }
    const T* sbase = src + (size_t)grp * Csg;

    uint4 rp[2], rw[2];
    auto load = [&](int st) {
        const int kidx = (st * GC_KB + pc * 16) / ES;
        const bool valid = kidx < K;                  // the tail of the last stage is zero on both sides
        const int tap = valid ? kidx / Csg : 0;
        const int c = kidx - tap * Csg;
        const int tr = tap / k, ts = tap - tr * k;
        const int dr = DGRAD ? p - tr : tr - p, dc = DGRAD ? p - ts : ts - p;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int ih = px[i].h + dr, iw = px[i].w + dc;
            rp[i] = make_uint4(0u, 0u, 0u, 0u);
            if (valid && px[i].ok && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W)
                rp[i] = *(const uint4*)(sbase + ((size_t)((size_t)px[i].n * H + ih) * W + iw) * lds_ + c);
            const int row = r0 + 32 * i;
            rw[i] = make_uint4(0u, 0u, 0u, 0u);
            if (valid && row < BN) rw[i] = *(const uint4*)(w + (size_t)(col0 + row) * K + kidx);
        }
    };

    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    load(0);
    for (int st = 0; st < nst; ++st) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = r0 + 32 * i;
            *(uint4*)(Ps + row * GC_ROW + pc * 16) = rp[i];
            if (row < BN) *(uint4*)(Ws + row * GC_ROW + pc * 16) = rw[i];
        }
        __syncthreads();
        if (st + 1 < nst) load(st + 1);
#pragma unroll
        for (int kc = 0; kc < GC_KB / 64; ++kc) {
            if (st * GC_KB + kc * 64 < K * ES) {      // block-uniform: a 64-byte chunk wholly behind K is skipped
                const uint4 b = *(const uint4*)(Ps + (wv * 16 + lr) * GC_ROW + kc * 64 + lq * 16);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const uint4 a = *(const uint4*)(Ws + (nt * 16 + lr) * GC_ROW + kc * 64 + lq * 16);
                    Mma<T>::run(a, b, acc[nt]);
                }
            }
        }
        __syncthreads();
    }

    // acc[nt][r] = result of pixel (wv*16 + lr), channel nt*16 + lq*4 + r of the CTA's columns
    const int pl = wv * 16 + lr;
    const long long pix = (long long)blockIdx.x * GC_BM + pl;
    float* sl = (float*)smem;                         // [64][BN + 1] stored values, for the statistics (the staging tiles are dead)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int cl = nt * 16 + lq * 4;
        float v[4] = {acc[nt][0], acc[nt][1], acc[nt][2], acc[nt][3]};
        if (pix < npix) {
            T* d = dst + (size_t)pix * ldd + col0 + cl;
            if (accumulate) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += ET<T>::ld(d + e);
            }
            if constexpr (ES == 4) {
                *(float4*)d = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                uint2 u;
                u.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
                u.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
                *(uint2*)d = u;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = bf2f(f2bf(v[e]));       // the values as stored
            }
        }
        if (part) {
#pragma unroll
            for (int e = 0; e < 4; ++e) sl[pl * (BN + 1) + cl + e] = v[e];
        }
    }
    if (!part) return;
    __syncthreads();
    if (tid < BN) {                                   // one thread per channel, pixels in order: sum, then M2 about the block mean
        const long long left = (long long)npix - (long long)blockIdx.x * GC_BM;
        const int cnt = left < GC_BM ? (int)left : GC_BM;
        const float inv = 1.f / (float)cnt;
        float s = 0.f;
        for (int j = 0; j < cnt; ++j) s += sl[j * (BN + 1) + tid];
        const float mu = s * inv;
        float m2 = 0.f;
        for (int j = 0; j < cnt; ++j) {
            const float d = sl[j * (BN + 1) + tid] - mu;
            m2 = fmaf(d, d, m2);
        }
        part[((size_t)blockIdx.x * 2) * ldp + col0 + tid] = s;
        part[((size_t)blockIdx.x * 2 + 1) * ldp + col0 + tid] = m2;
    }
}

// ------------------------------------------------------------------------------------------------------
// weight gradient: ws[split][co][tap][ci] = sum over the split's pixels of dy[pix][co] * x[pix + tap][grp*Cig + ci]
// ------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void gconv_wgrad_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ dy, int lddy,
                                                          float* __restrict__ ws, int npix, int H, int W, int k, int Cig, int Cog,
                                                          int nMc, int nNc, int per, int steps, long long total) {
    constexpr int ES = sizeof(T), V = 16 / ES, ROWB = GW_PB * ES + 16, NP = 64 / V / 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 64 * ROWB];
    unsigned char* Ds = smem;                         // dy^T: [64 output channels][GW_PB pixels]
    unsigned char* Xs = smem + 64 * ROWB;             // x^T:  [64 input channels][GW_PB pixels]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int kk = k * k, p = k >> 1;
    int idx = blockIdx.y;
    const int nc = idx % nNc; idx /= nNc;
    const int mc = idx % nMc; idx /= nMc;
    const int tap = idx % kk;
    const int grp = idx / kk;
    const int mrows = min(64, Cog - mc * 64), nrows = min(64, Cig - nc * 64);
    const int co0 = grp * Cog + mc * 64, ci0 = grp * Cig + nc * 64;
    const int tr = tap / k, dr = tr - p, dc = tap - tr * k - p;
    const int s0 = blockIdx.x * per, s1 = min(steps, s0 + per);

    f32x4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int step = s0; step < s1; ++step) {
        const long long q = (long long)step * GW_PB + lane;      // this thread stages pixel `lane`, 16-byte chunks wv, wv + 4, ...
        uint4 rd[NP], rx[NP];
        const bool ok = q < npix;
        const long long qq = ok ? q : 0;
        const int pw = (int)(qq % W);
        const long long t = qq / W;
        const int ih = (int)(t % H) + dr, iw = pw + dc;
        const bool xok = ok && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
        const size_t xpix = xok ? ((size_t)(t / H) * H + ih) * W + iw : 0;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int c = (wv + 4 * i) * V;
            rd[i] = make_uint4(0u, 0u, 0u, 0u);
            rx[i] = make_uint4(0u, 0u, 0u, 0u);
            if (ok && c < mrows) rd[i] = *(const uint4*)(dy + (size_t)q * lddy + co0 + c);
            if (xok && c < nrows) rx[i] = *(const uint4*)(x + xpix * ldx + ci0 + c);
        }
        __syncthreads();                              // the previous step's fragments have been read
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int c = (wv + 4 * i) * V;
            const T* ed = (const T*)&rd[i];
            const T* ex = (const T*)&rx[i];
#pragma unroll
            for (int e = 0; e < V; ++e) {
                *(T*)(Ds + (c + e) * ROWB + lane * ES) = ed[e];
                *(T*)(Xs + (c + e) * ROWB + lane * ES) = ex[e];
            }
        }
        __syncthreads();
        if (wv * 16 < mrows) {
#pragma unroll
            for (int kc = 0; kc < GW_PB * ES / 64; ++kc) {
                const uint4 a = *(const uint4*)(Ds + (wv * 16 + lr) * ROWB + kc * 64 + lq * 16);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    if (nt * 16 < nrows) {
                        const uint4 b = *(const uint4*)(Xs + (nt * 16 + lr) * ROWB + kc * 64 + lq * 16);
                        Mma<T>::run(a, b, acc[nt]);
                    }
                }
            }
        }
    }
    if (wv * 16 >= mrows) return;
    // acc[nt][r]: output channel co0 + wv*16 + lq*4 + r, input channel (of the group) nc*64 + nt*16 + lr
    float* out = ws + (size_t)blockIdx.x * total;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        if (nt * 16 >= nrows) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int co = co0 + wv * 16 + lq * 4 + r;
            out[((size_t)co * kk + tap) * Cig + nc * 64 + nt * 16 + lr] = acc[nt][r];
        }
    }
}

__global__ __launch_bounds__(256) void gconv_merge_kernel(const float* __restrict__ ws, float* __restrict__ dw, long long total, int splits) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float s = 0.f;
    for (int sp = 0; sp < splits; ++sp) s += ws[(size_t)sp * total + i];
    dw[i] += s;
}

// master [Cout][kk][Cig] f32 -> w (same shape, compute dtype) and wt [Cin][kk][Cog]: wt[grp*Cig + ci][tap][col] = w[grp*Cog + col][tap][ci]
template <typename T>
__global__ __launch_bounds__(256) void gconv_prep_kernel(const float* __restrict__ master, T* __restrict__ w, T* __restrict__ wt, long long total,
                                                         int kk, int Cig, int Cog) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const float v = master[i];
    ET<T>::st(w + i, v);
    const int ci = (int)(i % Cig);
    const long long t = i / Cig;
    const int tap = (int)(t % kk);
    const int co = (int)(t / kk);
    const int grp = co / Cog, col = co - grp * Cog;
    ET<T>::st(wt + ((size_t)(grp * Cig + ci) * kk + tap) * Cog + col, v);
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
static int gconv_check(const ydl_conv_geom* g, int groups, int dtype) {
    if (int e = check_geom(g, dtype)) return e;
    YDL_CHECK(groups >= 2, "grouped conv: groups >= 2 (groups = 1 is ydl_conv_fwd)");
    YDL_CHECK(g->Cin % groups == 0 && g->Cout % groups == 0, "grouped conv: groups must divide Cin and Cout");
    YDL_CHECK((g->Cin / groups) % 16 == 0 && (g->Cout / groups) % 16 == 0,
              "grouped conv: Cin/groups and Cout/groups must be multiples of 16");
    YDL_CHECK((g->k == 1 || g->k == 3) && g->s == 1 && g->p == g->k / 2, "grouped conv: k in {1,3}, s = 1, p = k/2");
    YDL_CHECK(g->ldw == 0, "grouped conv: ldw must be 0 (dense weights)");
    return 0;
}
extern "C" int ydl_gconv_supported(const ydl_conv_geom* g, int groups, int dtype) { return gconv_check(g, groups, dtype) == 0 ? 1 : 0; }
extern "C" int ydl_gconv_fwd_block_m(const ydl_conv_geom* g, int groups, int dtype) { return gconv_check(g, groups, dtype) == 0 ? GC_BM : 0; }
extern "C" int64_t ydl_gconv_fwd_stats_ws_bytes(const ydl_conv_geom* g, int groups, int dtype) {
    if (gconv_check(g, groups, dtype)) return 0;
    const int64_t rows = cdiv64((int64_t)g->N * g->Ho * g->Wo, GC_BM);
    return (rows + rows / 64 + 2) * 2 * round_up(g->Cout, 8) * (int64_t)sizeof(float);      // + room for ydl_bn_finalize's level-1 rows
}

template <typename T, bool DGRAD>
static void gconv_launch(const void* src, int lds_, const void* w, void* dst, int ldd, float* part, int ldp, int npix, int H, int W, int k,
                         int Csg, int Cdg, int groups, int accumulate, hipStream_t st) {
    const int tiles = Cdg / 16;
    const int nt = tiles % 4 == 0 ? 4 : tiles % 2 == 0 ? 2 : 1;
    dim3 grid((unsigned)((npix + GC_BM - 1) / GC_BM), (unsigned)(groups * (tiles / nt)));
#define GC_GO(NT_)                                                                                                               \
    gconv_kernel<T, NT_, DGRAD><<<grid, 256, 0, st>>>((const T*)src, lds_, (const T*)w, (T*)dst, ldd, part, ldp, npix, H, W, k, Csg, \
                                                     Cdg, accumulate)
    if (nt == 4) GC_GO(4);
    else if (nt == 2) GC_GO(2);
    else GC_GO(1);
#undef GC_GO
}

extern "C" int ydl_gconv_fwd(const ydl_conv_geom* g, int groups, int dtype, const void* x, const void* w, void* y, float* stats_ws,
                             void* stream) {
    if (int e = gconv_check(g, groups, dtype)) return e;
    YDL_CHECK(x && w && y, "null pointer");
    YDL_CHECK(aligned16(x) && aligned16(w) && aligned16(y), "16-byte alignment");
    const int npix = g->N * g->Ho * g->Wo;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == YDL_F32)
        gconv_launch<float, false>(x, g->ldx, w, y, g->ldy, stats_ws, round_up(g->Cout, 8), npix, g->Hi, g->Wi, g->k, g->Cin / groups,
                                   g->Cout / groups, groups, 0, st);
    else
        gconv_launch<bf16_t, false>(x, g->ldx, w, y, g->ldy, stats_ws, round_up(g->Cout, 8), npix, g->Hi, g->Wi, g->k, g->Cin / groups,
                                    g->Cout / groups, groups, 0, st);
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int ydl_gconv_dgrad(const ydl_conv_geom* g, int groups, int dtype, const void* dy, const void* wt, void* dx, int accumulate,
                               void* stream) {
    if (int e = gconv_check(g, groups, dtype)) return e;
    YDL_CHECK(dy && wt && dx, "null pointer");
    YDL_CHECK(aligned16(dy) && aligned16(wt) && aligned16(dx), "16-byte alignment");
    const int npix = g->N * g->Hi * g->Wi;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == YDL_F32)
        gconv_launch<float, true>(dy, g->ldy, wt, dx, g->ldx, nullptr, 0, npix, g->Hi, g->Wi, g->k, g->Cout / groups, g->Cin / groups,
                                  groups, accumulate != 0, st);
    else
        gconv_launch<bf16_t, true>(dy, g->ldy, wt, dx, g->ldx, nullptr, 0, npix, g->Hi, g->Wi, g->k, g->Cout / groups, g->Cin / groups,
                                   groups, accumulate != 0, st);
    YDL_LAUNCH_CHECK();
    return 0;
}

// launch shape of the weight gradient: a pure function of the geometry, so the result does not depend on the device
struct GwPlan { int nMc, nNc, steps, per, splits; long long total; };
static GwPlan gw_plan(const ydl_conv_geom* g, int groups) {
    GwPlan pl;
    const int Cig = g->Cin / groups, Cog = g->Cout / groups, kk = g->k * g->k;
    pl.nMc = (Cog + 63) / 64;
    pl.nNc = (Cig + 63) / 64;
    pl.steps = (int)cdiv64((int64_t)g->N * g->Ho * g->Wo, GW_PB);
    const int base = groups * kk * pl.nMc * pl.nNc;
    int want = 512 / base;
    want = want < 1 ? 1 : want > GW_MAX_SPLITS ? GW_MAX_SPLITS : want;
    if (want > pl.steps) want = pl.steps;
    pl.per = (pl.steps + want - 1) / want;
    pl.splits = (pl.steps + pl.per - 1) / pl.per;     // no split is empty
    pl.total = (long long)g->Cout * kk * Cig;
    return pl;
}
extern "C" int64_t ydl_gconv_wgrad_ws_bytes(const ydl_conv_geom* g, int groups, int dtype) {
    if (gconv_check(g, groups, dtype)) return 0;
    const GwPlan pl = gw_plan(g, groups);
    return (int64_t)pl.splits * pl.total * (int64_t)sizeof(float);
}
extern "C" int ydl_gconv_wgrad(const ydl_conv_geom* g, int groups, int dtype, const void* x, const void* dy, float* dw, float* ws,
                               void* stream) {
    if (int e = gconv_check(g, groups, dtype)) return e;
    YDL_CHECK(x && dy && dw && ws, "null pointer (ws: ydl_gconv_wgrad_ws_bytes)");
    YDL_CHECK(aligned16(x) && aligned16(dy), "16-byte alignment");
    const GwPlan pl = gw_plan(g, groups);
    const int npix = g->N * g->Ho * g->Wo, kk = g->k * g->k;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)pl.splits, (unsigned)(groups * kk * pl.nMc * pl.nNc));
    if (dtype == YDL_F32)
        gconv_wgrad_kernel<float><<<grid, 256, 0, st>>>((const float*)x, g->ldx, (const float*)dy, g->ldy, ws, npix, g->Hi, g->Wi, g->k,
                                                        g->Cin / groups, g->Cout / groups, pl.nMc, pl.nNc, pl.per, pl.steps, pl.total);
    else
        gconv_wgrad_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)x, g->ldx, (const bf16_t*)dy, g->ldy, ws, npix, g->Hi, g->Wi, g->k,
                                                         g->Cin / groups, g->Cout / groups, pl.nMc, pl.nNc, pl.per, pl.steps, pl.total);
    YDL_LAUNCH_CHECK();
    gconv_merge_kernel<<<(unsigned)((pl.total + 255) / 256), 256, 0, st>>>(ws, dw, pl.total, pl.splits);
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int ydl_gconv_weight_prep(int dtype, const float* master, void* w, void* wt, int Cout, int kk, int Cin, int groups, void* stream) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "bad dtype");
    YDL_CHECK(master && w && wt, "null pointer");
    YDL_CHECK(Cout > 0 && kk > 0 && Cin > 0 && groups >= 1 && Cin % groups == 0 && Cout % groups == 0, "bad sizes");
    const long long total = (long long)Cout * kk * (Cin / groups);
    hipStream_t st = (hipStream_t)stream;
    const unsigned nb = (unsigned)((total + 255) / 256);
    if (dtype == YDL_F32) gconv_prep_kernel<float><<<nb, 256, 0, st>>>(master, (float*)w, (float*)wt, total, kk, Cin / groups, Cout / groups);
    else gconv_prep_kernel<bf16_t><<<nb, 256, 0, st>>>(master, (bf16_t*)w, (bf16_t*)wt, total, kk, Cin / groups, Cout / groups);
    YDL_LAUNCH_CHECK();
    return 0;
}
