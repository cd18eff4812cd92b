// Cross convolution: a kernel of k taps along ONE image axis — nn.Conv2d(Cin, Cout, (1,k), (1,s), (0,k/2)) (YDL_AXIS_W) or
// nn.Conv2d(Cin, Cout, (k,1), (s,1), (k/2,0)) (YDL_AXIS_H), the two halves of models/common.py:147-158 CrossConv.  NHWC, f32 or
// bf16 storage, f32 accumulation, no atomics anywhere, groups = 1.
//
// Served set (ydl_xconv_supported): k odd in 3..9, s in {1, 2}, p = k/2, Cin and Cout multiples of 8 (a 16-byte piece of K never
// straddles a tap, a lane's four output channels are all inside or all outside the tensor), ldw = 0.
//
// Structure: the plain LDS-staged tile kernels of gconv.hip with another tap map.  A tap is a shift by one pixel (W) or by one image
// row (H) of the SAME sample; a shifted coordinate outside [0, L) contributes zero, so nothing wraps into the neighbouring row or
// sample.  K = k*C is walked in stages of 128 bytes per row.  The algorithm needs x from HBM once: the k shifted reads of one pixel
// come from neighbouring CTAs (W: the same or the next CTA, H: a CTA W pixels away) within microseconds of each other, so they are
// expected to be served by L2 (supposed from the work-item order; no cache counters were collected).
//   * forward / input gradient (xconv_kernel): a CTA owns 128 destination pixels x 16*NT channels; the weight tile is the MFMA A
//     operand and the pixel tile the B operand, so a lane holds four consecutive channels of one pixel.  The input gradient is the
//     same kernel on (dy, wt): destination coordinate i takes tap t from dy coordinate (i + p - t) / s where that quotient is exact
//     and inside the output (a gather; stride 2 leaves every other tap of a pixel zero).
//   * weight gradient (xconv_wgrad_kernel): a CTA owns (pixel split, group of <= 3 taps, <=64 x <=64 channel tile), transposes dy
//     once and the shifted x per tap in registers, writes them to LDS so that the pixel index is the MFMA K, and stores its partial
//     tiles; xconv_merge_kernel adds the splits in a fixed order.
#include "conv_common.h"

#define XC_PT 2                  // 16-pixel tiles per wave
#define XC_BM (64 * XC_PT)        // pixels per CTA = pixels per BatchNorm statistics row: a weight stage serves twice the pixels
#define XC_KB 128                // bytes of K per row and stage: two 64-byte MFMA chunks
#define XC_ROW (XC_KB + 16)      // LDS row stride: one 16-byte slot of padding spreads the rows over the banks
#define XW_KB 128                // weight gradient: bytes of pixels per LDS row and step (64 bf16 or 32 f32 pixels)
#define XW_ROW (XW_KB + 32)      // LDS row stride of 40 dwords: the 16-lane groups of a ds_read_b128 fragment read hit 16 distinct bank quads
#define XW_TG 3                  // taps per CTA: dy is staged once for all of them
#define XW_TILE_F (XW_TG * 4 * 1024)   // floats of one CTA's partial tiles in the workspace: XW_TG taps x 64 x 64
#define XW_MAX_SPLITS 512
#define XW_TARGET_CTAS 512       // two CTAs per CU; measured against 1024: the larger workspace costs more than the occupancy gains
#define XW_WS_BYTES (32ll << 20) // the splits' partial tiles stay within this, so the merge stays a small read

struct XcPix { int n, h, w, ok; };

// ------------------------------------------------------------------------------------------------------
// forward (DGRAD = false): dst[(n, a, b)][c] = sum_{t, cs} src[(n, a*s - p + t, b)][cs] * w[c][t][cs]          (a: the conv axis)
// input gradient (DGRAD = true): dst[(n, a, b)][c] = sum_{t, cs} src[(n, (a + p - t)/s, b)][cs] * wt[c][t][cs]  (exact quotients)
// (Hd, Wd): the destination image, (Hs, Ws): the source image; they differ along the axis only.
// ------------------------------------------------------------------------------------------------------
template <typename T, int NT, bool DGRAD>
__global__ __launch_bounds__(256) void xconv_kernel(const T* __restrict__ src, int lds_, const T* __restrict__ w, T* __restrict__ dst,
                                                    int ldd, float* __restrict__ part, int ldp, int npix, int Hd, int Wd, int Hs, int Ws,
                                                    int k, int s, int axis, int Cs, int Cd, int accumulate) {
    constexpr int ES = sizeof(T), BN = 16 * NT;
    static_assert(XC_PT == 2, "the statistics tail adds a lane's two pixels");
    __shared__ __attribute__((aligned(16))) unsigned char smem[(XC_BM + BN) * XC_ROW];
    unsigned char* Ps = smem;                         // [XC_BM pixels][XC_ROW]
    unsigned char* Wsm = smem + XC_BM * XC_ROW;       // [BN weight rows][XC_ROW]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int col0 = blockIdx.y * BN;                 // first destination channel of this CTA
    const int bx = xcd_remap(blockIdx.x, gridDim.x);  // pixel tile: neighbours in the image (the other taps' readers) share an XCD's L2
    const int K = k * Cs, p = k >> 1;
    const int Ls = axis ? Hs : Ws;
    const int nst = (K * ES + XC_KB - 1) / XC_KB;
    const int pc = tid & 7, r0 = tid >> 3;            // this thread stages piece pc of pixel rows r0 + 32 i and weight rows r0, r0 + 32

    XcPix px[XC_PT * 2];
#pragma unroll
    for (int i = 0; i < XC_PT * 2; ++i) {
        const long long q = (long long)bx * XC_BM + r0 + 32 * i;
        px[i].ok = q < npix;
        const long long qq = px[i].ok ? q : 0;
        px[i].w = (int)(qq % Wd);
        const long long t = qq / Wd;
        px[i].h = (int)(t % Hd);
        px[i].n = (int)(t / Hd);
    }

    uint4 rp[XC_PT * 2], rw[2];
    auto load = [&](int st) {
        const int kidx = (st * XC_KB + pc * 16) / ES;
        const bool valid = kidx < K;                  // the tail of the last stage is zero on both sides
        const int tap = valid ? kidx / Cs : 0;
        const int c = kidx - tap * Cs;
#pragma unroll
        for (int i = 0; i < XC_PT * 2; ++i) {
            const int a = axis ? px[i].h : px[i].w;
            int as;
            bool ok;
            if (DGRAD) {
                const int num = a + p - tap;
                ok = num >= 0 && (s == 1 || (num & 1) == 0);
                as = s == 2 ? num >> 1 : num;
                ok = ok && as < Ls;
            } else {
                as = a * s - p + tap;
                ok = (unsigned)as < (unsigned)Ls;
            }
            const int ih = axis ? as : px[i].h, iw = axis ? px[i].w : as;
            rp[i] = make_uint4(0u, 0u, 0u, 0u);
            if (valid && px[i].ok && ok) rp[i] = *(const uint4*)(src + ((size_t)((size_t)px[i].n * Hs + ih) * Ws + iw) * lds_ + c);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = r0 + 32 * i;
            rw[i] = make_uint4(0u, 0u, 0u, 0u);
            if (valid && row < BN && col0 + row < Cd) rw[i] = *(const uint4*)(w + (size_t)(col0 + row) * K + kidx);
        }
    };

    f32x4 acc[XC_PT][NT];
#pragma unroll
    for (int pt = 0; pt < XC_PT; ++pt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[pt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    load(0);
    for (int st = 0; st < nst; ++st) {
#pragma unroll
        for (int i = 0; i < XC_PT * 2; ++i) *(uint4*)(Ps + (r0 + 32 * i) * XC_ROW + pc * 16) = rp[i];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = r0 + 32 * i;
            if (row < BN) *(uint4*)(Wsm + row * XC_ROW + pc * 16) = rw[i];
        }
        __syncthreads();
        if (st + 1 < nst) load(st + 1);
#pragma unroll
        for (int kc = 0; kc < XC_KB / 64; ++kc) {
            if (st * XC_KB + kc * 64 < K * ES) {      // block-uniform: a 64-byte chunk wholly behind K is skipped
                uint4 b[XC_PT];
#pragma unroll
                for (int pt = 0; pt < XC_PT; ++pt) b[pt] = *(const uint4*)(Ps + ((wv * XC_PT + pt) * 16 + lr) * XC_ROW + kc * 64 + lq * 16);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const uint4 a = *(const uint4*)(Wsm + (nt * 16 + lr) * XC_ROW + kc * 64 + lq * 16);
#pragma unroll
                    for (int pt = 0; pt < XC_PT; ++pt) Mma<T>::run(a, b[pt], acc[pt][nt]);
                }
            }
        }
        __syncthreads();
    }

    // acc[pt][nt][r] = result of pixel ((wv*XC_PT + pt)*16 + lr), channel nt*16 + lq*4 + r of the CTA's columns
    // The statistics are taken of the values AS STORED, which go back into acc.
#pragma unroll
    for (int pt = 0; pt < XC_PT; ++pt) {
        const int pl = (wv * XC_PT + pt) * 16 + lr;
        const long long pix = (long long)bx * XC_BM + pl;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int cl = nt * 16 + lq * 4;
            float v[4] = {acc[pt][nt][0], acc[pt][nt][1], acc[pt][nt][2], acc[pt][nt][3]};
            if (pix < npix && col0 + cl < Cd) {       // Cd is a multiple of 8: the four channels are inside together
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
                    for (int e = 0; e < 4; ++e) v[e] = bf2f(f2bf(v[e]));   // the values as stored
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[pt][nt][e] = v[e];
        }
    }
    if (!part) return;
    // per channel (sum, M2 about the block mean) of the block's pixels, from the fragments: a lane adds its two pixels, the 16 lanes
    // of a row are reduced with shuffles (row_reduce), the four waves' partials are added in wave order — a fixed summation tree.
    // A pixel behind npix holds zeros: it adds nothing to the sum and is masked out of M2.
    constexpr int NV = 4 * NT;
    float* red = (float*)smem;                        // [4][BN] sums, [BN] totals, [4][BN] M2s (the staging tiles are dead)
    const int vi = lr & (NV - 1), cv = (vi >> 2) * 16 + lq * 4 + (vi & 3);   // the channel whose total row_reduce leaves in slot 0
    float sv[NV];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) sv[nt * 4 + e] = acc[0][nt][e] + acc[1][nt][e];
    row_reduce<NV>(sv, lr);
    if (lr < NV) red[wv * BN + cv] = sv[0];
    __syncthreads();
    if (tid < BN) red[4 * BN + tid] = ((red[tid] + red[BN + tid]) + red[2 * BN + tid]) + red[3 * BN + tid];
    __syncthreads();
    const long long left = (long long)npix - (long long)bx * XC_BM;
    const int cnt = left < XC_BM ? (int)left : XC_BM;
    const float inv = 1.f / (float)cnt;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const float4 tt = *(const float4*)(red + 4 * BN + nt * 16 + lq * 4);
        const float mu[4] = {tt.x * inv, tt.y * inv, tt.z * inv, tt.w * inv};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float q = 0.f;
#pragma unroll
            for (int pt = 0; pt < XC_PT; ++pt) {
                const float d = (wv * XC_PT + pt) * 16 + lr < cnt ? acc[pt][nt][e] - mu[e] : 0.f;
                q = fmaf(d, d, q);
            }
            sv[nt * 4 + e] = q;
        }
    }
    row_reduce<NV>(sv, lr);
    if (lr < NV) red[5 * BN + wv * BN + cv] = sv[0];
    __syncthreads();
    if (tid < BN && col0 + tid < Cd) {
        part[((size_t)bx * 2) * ldp + col0 + tid] = red[4 * BN + tid];
        part[((size_t)bx * 2 + 1) * ldp + col0 + tid] =
            ((red[5 * BN + tid] + red[6 * BN + tid]) + red[7 * BN + tid]) + red[8 * BN + tid];
    }
}

// ------------------------------------------------------------------------------------------------------
// weight gradient: ws[split][co][tap][ci] = sum over the split's output pixels (n, a, b) of dy[(n, a, b)][co] * x[(n, a*s - p + tap, b)][ci]
// A CTA owns (pixel split, group of <= XW_TG taps, <= 64 x <= 64 channel tile).  Per step of XW_KB bytes of pixels it stages dy^T ONCE
// and one x^T tile per tap of its group.  A staging task is V pixels x V channels (V = elements per 16 bytes): V 16-byte loads — the
// lanes of a wave run over the channel pieces of a pixel first, so a load instruction covers whole lines —, a V x V transpose in
// registers, V 16-byte LDS writes.  The next step's loads are issued before this step's MFMAs.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t xw_lo(uint32_t a, uint32_t b) { return (a & 0xffffu) | (b << 16); }
__device__ __forceinline__ uint32_t xw_hi(uint32_t a, uint32_t b) { return (a >> 16) | (b & 0xffff0000u); }

template <typename T>
__global__ __launch_bounds__(256) void xconv_wgrad_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ dy, int lddy,
                                                          float* __restrict__ ws, int npix, int Ho, int Wo, int Hi, int Wi, int k, int s,
                                                          int axis, int Cin, int Cout, int nMc, int nNc, int ntg, int per, int steps,
                                                          long long total) {
    constexpr int ES = sizeof(T), V = 16 / ES, PB = XW_KB / ES, NCH = 64 / V, TASKS = (PB / V) * NCH, NTK = (1 + XW_TG) * TASKS / 256;
    constexpr int TILE = 64 * XW_ROW;
    static_assert(TASKS % 64 == 0 && (1 + XW_TG) * TASKS % 256 == 0, "a wave's tasks belong to one tile");
    __shared__ __attribute__((aligned(16))) unsigned char smem[(1 + XW_TG) * TILE];   // dy^T, then x^T per tap: [64 channels][PB pixels]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int p = k >> 1;
    // linear work-item id in XCD-aware order: the CTAs of one pixel split (they read the same dy and x) share an XCD's L2
    const int base = ntg * nMc * nNc;
    const int L_ = xcd_remap(blockIdx.x, gridDim.x);
    const int split = L_ / base;
    int idx = L_ - split * base;
    const int nc = idx % nNc; idx /= nNc;
    const int mc = idx % nMc;
    const int tap0 = (idx / nMc) * XW_TG, ntap = min(XW_TG, k - tap0);
    const int mrows = min(64, Cout - mc * 64), nrows = min(64, Cin - nc * 64);
    const int co0 = mc * 64, ci0 = nc * 64;
    const int Li = axis ? Hi : Wi;
    const int s0 = split * per, s1 = min(steps, s0 + per);

    uint4 raw[NTK][V];
    auto load = [&](int step) {
#pragma unroll
        for (int i = 0; i < NTK; ++i) {
            const int j = tid + 256 * i, tile = j / TASKS, wi = j % TASKS, c = (wi % NCH) * V, pg = wi / NCH;   // tile: wave-uniform
            const unsigned q0 = (unsigned)step * PB + pg * V;        // < 2^31 + PB
            // The kernel is bound by the vector instructions of this staging, so the addresses are kept short: pixel indices are
            // 32-bit (the host checks the pixel counts), one 64-bit multiply-add per load.
            if (tile == 0) {
                const bool live = c < mrows;
                const T* b = dy + co0 + c;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    raw[i][e] = make_uint4(0u, 0u, 0u, 0u);
                    if (live && q0 + e < (unsigned)npix) raw[i][e] = *(const uint4*)(b + (size_t)(q0 + e) * (unsigned)lddy);
                }
            } else {
                const bool live = tile <= ntap && c < nrows;
                const int dt = tap0 + tile - 1 - p;
                const T* b = x + ci0 + c;
                int w = (int)(q0 % (unsigned)Wo);
                const unsigned t = q0 / (unsigned)Wo;
                int h = (int)(t % (unsigned)Ho), nh = (int)(t / (unsigned)Ho) * Hi;      // nh: first image row of the sample
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const int as = (axis ? h : w) * s + dt;
                    const int xp = (nh + (axis ? as : h)) * Wi + (axis ? w : as);       // read only where as is inside [0, Li)
                    raw[i][e] = make_uint4(0u, 0u, 0u, 0u);
                    if (live && q0 + e < (unsigned)npix && (unsigned)as < (unsigned)Li)
                        raw[i][e] = *(const uint4*)(b + (size_t)(unsigned)xp * (unsigned)ldx);
                    const bool cw = ++w == Wo;
                    w = cw ? 0 : w;
                    h += cw;
                    const bool ch = h == Ho;
                    h = ch ? 0 : h;
                    nh += ch ? Hi : 0;
                }
            }
        }
    };

    f32x4 acc[XW_TG][4];
#pragma unroll
    for (int t = 0; t < XW_TG; ++t)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[t][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (s0 < s1) load(s0);
    for (int step = s0; step < s1; ++step) {
        __syncthreads();                              // the previous step's fragments have been read
#pragma unroll
        for (int i = 0; i < NTK; ++i) {
            const int j = tid + 256 * i, tile = j / TASKS, wi = j % TASKS, c = (wi % NCH) * V, pg = wi / NCH;
            if (tile > ntap) continue;                // a tap tile this group does not have is never read
            unsigned char* d = smem + tile * TILE + c * XW_ROW + pg * 16;
            const uint32_t* r = (const uint32_t*)&raw[i][0];          // r[pixel * 4 + dword]
            if constexpr (ES == 2) {                  // dword jd of a pixel holds channels 2 jd, 2 jd + 1
#pragma unroll
                for (int jd = 0; jd < 4; ++jd) {
                    *(uint4*)(d + (2 * jd) * XW_ROW) = make_uint4(xw_lo(r[jd], r[4 + jd]), xw_lo(r[8 + jd], r[12 + jd]),
                                                                  xw_lo(r[16 + jd], r[20 + jd]), xw_lo(r[24 + jd], r[28 + jd]));
                    *(uint4*)(d + (2 * jd + 1) * XW_ROW) = make_uint4(xw_hi(r[jd], r[4 + jd]), xw_hi(r[8 + jd], r[12 + jd]),
                                                                      xw_hi(r[16 + jd], r[20 + jd]), xw_hi(r[24 + jd], r[28 + jd]));
                }
            } else {
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) *(uint4*)(d + cc * XW_ROW) = make_uint4(r[cc], r[4 + cc], r[8 + cc], r[12 + cc]);
            }
        }
        __syncthreads();
        if (step + 1 < s1) load(step + 1);
        // channel rows outside the tensor were staged as zeros, so the MFMAs of a full tap group run unconditionally (straight-line
        // code: the accumulators stay where they are); a group with fewer taps skips the tiles it never staged
        auto mma = [&](auto full) {
#pragma unroll
            for (int kc = 0; kc < XW_KB / 64; ++kc) {
                const uint4 a = *(const uint4*)(smem + (wv * 16 + lr) * XW_ROW + kc * 64 + lq * 16);
#pragma unroll
                for (int t = 0; t < XW_TG; ++t) {
                    if (decltype(full)::value || t < ntap) {
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt) {
                            const uint4 b = *(const uint4*)(smem + (1 + t) * TILE + (nt * 16 + lr) * XW_ROW + kc * 64 + lq * 16);
                            Mma<T>::run(a, b, acc[t][nt]);
                        }
                    }
                }
            }
        };
        if (ntap == XW_TG) mma(std::true_type{});
        else mma(std::false_type{});
    }
    // acc[t][nt][r]: output channel co0 + wv*16 + lq*4 + r, tap tap0 + t, input channel ci0 + nt*16 + lr.  The partial tiles go out in
    // fragment order, ws[split][tile][t][nt][wave][r][lane]: every store instruction writes whole lines; the merge maps them to dw
    // and leaves out what lies outside the tensor (the accumulators of a tap the group does not have hold zeros)
    float* out = ws + ((size_t)split * base + (L_ - split * base)) * XW_TILE_F + wv * 256 + lane;
#pragma unroll
    for (int t = 0; t < XW_TG; ++t)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(t * 4 + nt) * 1024 + r * 64] = acc[t][nt][r];
}

// dw[co][tap][ci] += the splits' partial tiles.  A CTA adds the splits of 32 elements of a tile: eight threads per element each add a
// contiguous eighth of the splits in split order (eight loads in flight at a time), and the eight partials are added in order — a
// fixed summation tree.
__global__ __launch_bounds__(256) void xconv_merge_kernel(const float* __restrict__ ws, float* __restrict__ dw, long long total, int splits,
                                                          int k, int Cin, int Cout, int nMc, int nNc) {
    __shared__ float red[8][32];
    const int e = threadIdx.x & 31, j = threadIdx.x >> 5;
    const long long i = (long long)blockIdx.x * 32 + e;              // < total = tiles * XW_TILE_F (a multiple of 32)
    const int tile = (int)(i / XW_TILE_F), rem = (int)(i % XW_TILE_F);
    const int ln = rem & 63, r = (rem >> 6) & 3, wv = (rem >> 8) & 3, nt = (rem >> 10) & 3, t = rem >> 12;
    const int nc = tile % nNc, mc = (tile / nNc) % nMc, tg = tile / (nNc * nMc);
    const int co = mc * 64 + wv * 16 + (ln >> 4) * 4 + r, ci = nc * 64 + nt * 16 + (ln & 15), tap = tg * XW_TG + t;
    const bool inside = co < Cout && ci < Cin && tap < k;
    const int q = (splits + 7) >> 3, a = min(splits, j * q), b = min(splits, a + q);
    float s = 0.f;
    if (inside) {
        const float* src = ws + i;
        int sp = a;
        for (; sp + 8 <= b; sp += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(sp + u) * total];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; sp < b; ++sp) s += src[(size_t)sp * total];
    }
    red[j][e] = s;
    __syncthreads();
    if (j == 0 && inside) {
        float sum = red[0][e];
#pragma unroll
        for (int u = 1; u < 8; ++u) sum += red[u][e];
        dw[((size_t)co * k + tap) * Cin + ci] += sum;
    }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
static int xconv_check(const ydl_conv_geom* g, int axis, int dtype) {
    YDL_CHECK(g != nullptr, "null geometry");
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "bad dtype");
    YDL_CHECK(axis == YDL_AXIS_W || axis == YDL_AXIS_H, "cross conv: axis must be YDL_AXIS_W or YDL_AXIS_H");
    YDL_CHECK(g->N > 0 && g->Hi > 0 && g->Wi > 0 && g->Cin > 0 && g->Cout > 0, "non-positive dims");
    YDL_CHECK(g->k >= 3 && g->k <= 9 && (g->k & 1) == 1, "cross conv: k must be odd, 3 <= k <= 9");
    YDL_CHECK(g->s == 1 || g->s == 2, "cross conv: s must be 1 or 2");
    YDL_CHECK(g->p == g->k / 2, "cross conv: p must be k/2");
    YDL_CHECK(g->Cin % 8 == 0 && g->Cout % 8 == 0, "cross conv: Cin and Cout must be multiples of 8");
    YDL_CHECK(g->ldw == 0, "cross conv: ldw must be 0 (dense weights)");
    const int Li = axis == YDL_AXIS_H ? g->Hi : g->Wi, Lo = (Li + 2 * g->p - g->k) / g->s + 1;
    YDL_CHECK(axis == YDL_AXIS_H ? (g->Ho == Lo && g->Wo == g->Wi) : (g->Wo == Lo && g->Ho == g->Hi),
              "cross conv: output size must be (L+2p-k)/s+1 along the axis and the input's extent along the other");
    const int es = esize(dtype);
    YDL_CHECK(g->ldx >= g->Cin && g->ldy >= g->Cout, "pixel stride smaller than channel count");
    YDL_CHECK((g->ldx * es) % 16 == 0 && (g->ldy * es) % 16 == 0, "pixel strides must be 16-byte multiples");
    YDL_CHECK((int64_t)g->N * g->Hi * g->Wi < (1ll << 31) && (int64_t)g->N * g->Ho * g->Wo < (1ll << 31), "too many pixels");
    return 0;
}
extern "C" int ydl_xconv_supported(const ydl_conv_geom* g, int axis, int dtype) { return xconv_check(g, axis, dtype) == 0 ? 1 : 0; }
extern "C" int ydl_xconv_fwd_block_m(const ydl_conv_geom* g, int axis, int dtype) { return xconv_check(g, axis, dtype) == 0 ? XC_BM : 0; }
extern "C" int64_t ydl_xconv_fwd_stats_ws_bytes(const ydl_conv_geom* g, int axis, int dtype) {
    if (xconv_check(g, axis, dtype)) return 0;
    const int64_t rows = cdiv64((int64_t)g->N * g->Ho * g->Wo, XC_BM);
    return (rows + rows / 64 + 2) * 2 * g->Cout * (int64_t)sizeof(float);      // + room for ydl_bn_finalize's level-1 rows
}

template <typename T, bool DGRAD>
static void xconv_launch(const void* src, int lds_, const void* w, void* dst, int ldd, float* part, int ldp, int npix, int Hd, int Wd,
                         int Hs, int Ws, int k, int s, int axis, int Cs, int Cd, int accumulate, hipStream_t st) {
    const int tiles = (Cd + 15) / 16;
    const int nt = tiles >= 3 ? 4 : tiles;            // 16, 32 or 64 channels per CTA
    dim3 grid((unsigned)((npix + XC_BM - 1) / XC_BM), (unsigned)((tiles + nt - 1) / nt));
#define XC_GO(NT_)                                                                                                                \
    xconv_kernel<T, NT_, DGRAD><<<grid, 256, 0, st>>>((const T*)src, lds_, (const T*)w, (T*)dst, ldd, part, ldp, npix, Hd, Wd, Hs, Ws, \
                                                     k, s, axis, Cs, Cd, accumulate)
    if (nt == 4) XC_GO(4);
    else if (nt == 2) XC_GO(2);
    else XC_GO(1);
#undef XC_GO
}

extern "C" int ydl_xconv_fwd(const ydl_conv_geom* g, int axis, int dtype, const void* x, const void* w, void* y, float* stats_ws,
                             void* stream) {
    if (int e = xconv_check(g, axis, dtype)) return e;
    YDL_CHECK(x && w && y, "null pointer");
    YDL_CHECK(aligned16(x) && aligned16(w) && aligned16(y), "16-byte alignment");
    const int npix = g->N * g->Ho * g->Wo;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == YDL_F32)
        xconv_launch<float, false>(x, g->ldx, w, y, g->ldy, stats_ws, g->Cout, npix, g->Ho, g->Wo, g->Hi, g->Wi, g->k, g->s, axis, g->Cin,
                                   g->Cout, 0, st);
    else
        xconv_launch<bf16_t, false>(x, g->ldx, w, y, g->ldy, stats_ws, g->Cout, npix, g->Ho, g->Wo, g->Hi, g->Wi, g->k, g->s, axis, g->Cin,
                                    g->Cout, 0, st);
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int ydl_xconv_dgrad(const ydl_conv_geom* g, int axis, int dtype, const void* dy, const void* wt, void* dx, int accumulate,
                               void* stream) {
    if (int e = xconv_check(g, axis, dtype)) return e;
    YDL_CHECK(dy && wt && dx, "null pointer");
    YDL_CHECK(aligned16(dy) && aligned16(wt) && aligned16(dx), "16-byte alignment");
    const int npix = g->N * g->Hi * g->Wi;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == YDL_F32)
        xconv_launch<float, true>(dy, g->ldy, wt, dx, g->ldx, nullptr, 0, npix, g->Hi, g->Wi, g->Ho, g->Wo, g->k, g->s, axis, g->Cout,
                                  g->Cin, accumulate != 0, st);
    else
        xconv_launch<bf16_t, true>(dy, g->ldy, wt, dx, g->ldx, nullptr, 0, npix, g->Hi, g->Wi, g->Ho, g->Wo, g->k, g->s, axis, g->Cout,
                                   g->Cin, accumulate != 0, st);
    YDL_LAUNCH_CHECK();
    return 0;
}

// launch shape of the weight gradient: a pure function of the geometry, so the result does not depend on the device
struct XwPlan { int nMc, nNc, ntg, steps, per, splits; long long total; };
static XwPlan xw_plan(const ydl_conv_geom* g, int dtype) {
    XwPlan pl;
    pl.nMc = (g->Cout + 63) / 64;
    pl.nNc = (g->Cin + 63) / 64;
    pl.ntg = (g->k + XW_TG - 1) / XW_TG;
    pl.steps = (int)cdiv64((int64_t)g->N * g->Ho * g->Wo, XW_KB / esize(dtype));
    const int base = pl.ntg * pl.nMc * pl.nNc;
    pl.total = (long long)base * XW_TILE_F;          // floats of one split in the workspace: whole tiles in fragment order
    long long want = XW_TARGET_CTAS / base;
    const long long fit = XW_WS_BYTES / (pl.total * (long long)sizeof(float));
    want = want > fit ? fit : want;
    want = want < 1 ? 1 : want > XW_MAX_SPLITS ? XW_MAX_SPLITS : want;
    if (want > pl.steps) want = pl.steps;
    pl.per = (int)((pl.steps + want - 1) / want);
    pl.splits = (pl.steps + pl.per - 1) / pl.per;     // no split is empty
    return pl;
}
extern "C" int64_t ydl_xconv_wgrad_ws_bytes(const ydl_conv_geom* g, int axis, int dtype) {
    if (xconv_check(g, axis, dtype)) return 0;
    const XwPlan pl = xw_plan(g, dtype);
    return (int64_t)pl.splits * pl.total * (int64_t)sizeof(float);
}
extern "C" int ydl_xconv_wgrad(const ydl_conv_geom* g, int axis, int dtype, const void* x, const void* dy, float* dw, float* ws,
                               void* stream) {
    if (int e = xconv_check(g, axis, dtype)) return e;
    YDL_CHECK(x && dy && dw && ws, "null pointer (ws: ydl_xconv_wgrad_ws_bytes)");
    YDL_CHECK(aligned16(x) && aligned16(dy), "16-byte alignment");
    const XwPlan pl = xw_plan(g, dtype);
    const int npix = g->N * g->Ho * g->Wo;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)(pl.splits * pl.ntg * pl.nMc * pl.nNc));
    if (dtype == YDL_F32)
        xconv_wgrad_kernel<float><<<grid, 256, 0, st>>>((const float*)x, g->ldx, (const float*)dy, g->ldy, ws, npix, g->Ho, g->Wo, g->Hi,
                                                        g->Wi, g->k, g->s, axis, g->Cin, g->Cout, pl.nMc, pl.nNc, pl.ntg, pl.per, pl.steps, pl.total);
    else
        xconv_wgrad_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)x, g->ldx, (const bf16_t*)dy, g->ldy, ws, npix, g->Ho, g->Wo, g->Hi,
                                                         g->Wi, g->k, g->s, axis, g->Cin, g->Cout, pl.nMc, pl.nNc, pl.ntg, pl.per,
                                                         pl.steps, pl.total);
    YDL_LAUNCH_CHECK();
    xconv_merge_kernel<<<(unsigned)(pl.total / 32), 256, 0, st>>>(ws, dw, pl.total, pl.splits, g->k, g->Cin, g->Cout, pl.nMc, pl.nNc);
    YDL_LAUNCH_CHECK();
    return 0;
}
