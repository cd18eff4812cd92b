// Local (windowed) self-attention of the stand-alone self-attention layers AttentionConv / AttentionStem (models/common.py:1509-1627),
// NHWC, for gfx950.  Q, K and the m value tensors V^0..V^{m-1} are bias-free 1x1 projections of x (the implicit-GEMM entry points);
// this file holds what is left: per sample n, channel c and pixel (h, w), independently, over the ks*ks taps t = i*ks + j reading
// position (h + i - p, w + j - p), p = ks/2 (K and V count as 0 outside the image; the tap stays in the softmax):
//     logit_t = Q[c] * (K_t[c] + r[c,t])            r[c,(i,j)] = rel_h[c][i] for c < C/2, rel_w[c - C/2][j] otherwise (or 0: no rel)
//     P       = softmax_t(logit)
//     out[c]  = sum_t P_t * U_t[c]                  U_t = sum_m E[m][t] * V^m_t   (E = 1 when no table is given)
// There is no sum over channels anywhere: an HBM/L2-bound stencil.  A work item is a pixel x 8 channels; a thread keeps its channel
// group and walks pixels with a grid stride, so the rel rows it needs stay in registers.
// Forward: one online-softmax sweep over the taps; also stores lse = max + log(sum) (f32) per (pixel, channel) so that the backward
// gets any P_t as exp(logit_t - lse) without a sweep of its own.
// Backward, gather form (no atomics): with dS_t = P_t * dout * (U_t - out)
//     la_bwd_q_kernel : per OUTPUT pixel: dQ = sum_t dS_t (K_t + r_t); partial sums of d rel (sum of dS*Q over pixels and the other
//                       window index) in registers and of dE[m][t] = sum P_t dout V^m_t in a thread-private LDS column; per-block
//                       partials go to the workspace and are merged in block order (bitwise reproducible)
//     la_bwd_kv_kernel: per INPUT position x: the ks*ks output pixels o = x - (i - p, j - p) whose window covers x give
//                       dK(x) = sum dS_t(o) Q(o) and dV^m(x) = sum E[m][t] P_t(o) dout(o); they need only Q, dout, out, lse of o
//                       and K, V of x itself.
// The AttentionStem mixing table E = softmax over m of (emb_mix @ emb_a)[m][i] + (emb_mix @ emb_b)[m][j] and its three parameter
// gradients are two single-block kernels at the end of the file.
#include "common.h"

#define LA_MAXBLK 1024          // per-block partial rows of the parameter gradients (grid.x cap of la_bwd_q_kernel)
#define LA_MAXM 8
#define LA_MAX_MT 196           // m * ks * ks: the dE columns of a 64-thread block stay under 64 KiB of LDS

struct LaArgs {
    const void *q, *k, *v, *o, *dout;
    void *out, *dq, *dk, *dv;
    float* lse;
    const float *rel_h, *rel_w, *emb;
    float* part;
    long long vstride, dvstride, eoff;
    int ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
    int N, H, W, C, m, acc, vec;
};

// 8 consecutive channels as floats; nv = how many of them exist (the rest read as 0 and are never stored).  vec: every row of
// every tensor of the call starts 16-byte aligned (wave-uniform), so a full group moves as 16-byte chunks.
template <typename T> __device__ __forceinline__ void ld8(const T* p, int nv, int vec, float* f) {
    if (vec && nv == 8) {
        if constexpr (ET<T>::V == 8) unpack16<T>(*(const uint4*)p, f);
        else { unpack16<T>(*(const uint4*)p, f); unpack16<T>(*(const uint4*)(p + 4), f + 4); }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = e < nv ? ET<T>::ld(p + e) : 0.f;
    }
}
template <typename T> __device__ __forceinline__ void st8(T* p, int nv, int vec, const float* f, int accumulate) {
    float o[8];
    if (accumulate) {
        float old[8];
        ld8<T>(p, nv, vec, old);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = f[e] + old[e];
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = f[e];
    }
    if (vec && nv == 8) {
        if constexpr (ET<T>::V == 8) *(uint4*)p = pack16<T>(o);
        else { *(uint4*)p = pack16<T>(o); *(uint4*)(p + 4) = pack16<T>(o + 4); }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (e < nv) ET<T>::st(p + e, o[e]);
    }
}

// thread -> (channel group, pixel lane): cpb channel groups and R = blockDim / cpb pixel lanes per block, grid.y over further groups
struct LaMap {
    int c0, nv, pl, R;
    bool live;
};
__device__ __forceinline__ LaMap la_map(int C) {
    const int BT = blockDim.x, cpp = (C + 7) / 8;
    const int cpb = cpp < BT ? cpp : BT;
    LaMap mp;
    mp.R = BT / cpb;
    const int cq = threadIdx.x % cpb, chunk = blockIdx.y * BT + cq;
    mp.pl = threadIdx.x / cpb;
    mp.live = mp.pl < mp.R && chunk < cpp;
    mp.c0 = chunk * 8;
    mp.nv = C - mp.c0 < 8 ? C - mp.c0 : 8;
    return mp;
}

// rel rows of the thread's 8 channels: rr[e][idx], idx = the window ROW for a channel of the first half, the COLUMN for the second
template <int KS> __device__ __forceinline__ void la_rel(const LaArgs& a, int c0, float (*rr)[KS], bool* ish) {
    const int half = a.C / 2;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = c0 + e;
        ish[e] = c < half;
#pragma unroll
        for (int i = 0; i < KS; ++i) rr[e][i] = 0.f;
        if (a.rel_h && c < a.C) {
            const float* rp = c < half ? a.rel_h + (size_t)c * KS : a.rel_w + (size_t)(c - half) * KS;
#pragma unroll
            for (int i = 0; i < KS; ++i) rr[e][i] = rp[i];
        }
    }
}

// K_t and U_t = sum_m E[m][t] V^m_t of the tap at (ih, iw) of image n (zeros outside the image)
template <typename T>
__device__ __forceinline__ void la_tap_kv(const LaArgs& a, int n, int ih, int iw, int t, int KK, int c0, int nv, float* kv, float* u) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { kv[e] = 0.f; u[e] = 0.f; }
    if ((unsigned)ih >= (unsigned)a.H || (unsigned)iw >= (unsigned)a.W) return;
    const size_t ip = ((size_t)n * a.H + ih) * a.W + iw;
    ld8<T>((const T*)a.k + ip * a.ldk + c0, nv, a.vec, kv);
    for (int mm = 0; mm < a.m; ++mm) {
        float vv[8];
        ld8<T>((const T*)a.v + mm * a.vstride + ip * a.ldv + c0, nv, a.vec, vv);
        const float em = a.emb ? a.emb[mm * KK + t] : 1.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) u[e] = fmaf(em, vv[e], u[e]);
    }
}

// ------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------
template <typename T, int KS>
__global__ __launch_bounds__(256) void la_fwd_kernel(const LaArgs a) {
    constexpr int KK = KS * KS, P = KS / 2;
    const LaMap mp = la_map(a.C);
    if (!mp.live) return;
    const int c0 = mp.c0, nv = mp.nv, Cp = (a.C + 7) / 8 * 8;
    float rr[8][KS];
    bool ish[8];
    la_rel<KS>(a, c0, rr, ish);
    const long long npix = (long long)a.N * a.H * a.W;
    for (long long pix = (long long)blockIdx.x * mp.R + mp.pl; pix < npix; pix += (long long)gridDim.x * mp.R) {
        const int w = (int)(pix % a.W);
        const long long t2 = pix / a.W;
        const int h = (int)(t2 % a.H), n = (int)(t2 / a.H);
        float q[8], mx[8], s[8], acc[8];
        ld8<T>((const T*)a.q + (size_t)pix * a.ldq + c0, nv, a.vec, q);
#pragma unroll
        for (int e = 0; e < 8; ++e) { mx[e] = -3.0e38f; s[e] = 0.f; acc[e] = 0.f; }
#pragma unroll
        for (int i = 0; i < KS; ++i) {
#pragma unroll
            for (int j = 0; j < KS; ++j) {
                float kv[8], u[8];
                la_tap_kv<T>(a, n, h + i - P, w + j - P, i * KS + j, KK, c0, nv, kv, u);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float r = ish[e] ? rr[e][i] : rr[e][j];
                    const float lg = q[e] * (kv[e] + r);
                    const float nm = fmaxf(mx[e], lg);
                    const float sc = __expf(mx[e] - nm), p = __expf(lg - nm);
                    s[e] = fmaf(s[e], sc, p);
                    acc[e] = fmaf(acc[e], sc, p * u[e]);
                    mx[e] = nm;
                }
            }
        }
        float o[8], l[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { o[e] = acc[e] / s[e]; l[e] = mx[e] + __logf(s[e]); }
        st8<T>((T*)a.out + (size_t)pix * a.ldo + c0, nv, a.vec, o, 0);
        if (a.lse) {
            float* lp = a.lse + (size_t)pix * Cp + c0;           // rows of Cp floats: all 8 lanes exist
            *(float4*)lp = make_float4(l[0], l[1], l[2], l[3]);
            *(float4*)(lp + 4) = make_float4(l[4], l[5], l[6], l[7]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// backward, output-pixel side: dQ and the per-block partials of d rel and dE
// ------------------------------------------------------------------------------------------------------
template <typename T, int KS>
__global__ __launch_bounds__(256) void la_bwd_q_kernel(const LaArgs a, int want_rel, int want_e) {
    constexpr int KK = KS * KS, P = KS / 2;
    extern __shared__ float ecol[];                  // [m*KK][blockDim]: column threadIdx.x belongs to this thread alone
    __shared__ float red[256 * 8];
    const int BT = blockDim.x;
    const LaMap mp = la_map(a.C);
    const int c0 = mp.c0, nv = mp.nv, Cp = (a.C + 7) / 8 * 8;
    const int MT = a.m * KK;
    if (want_e)
        for (int j = 0; j < MT; ++j) ecol[j * BT + threadIdx.x] = 0.f;
    float dr[8][KS];
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int i = 0; i < KS; ++i) dr[e][i] = 0.f;
    if (mp.live) {
        float rr[8][KS];
        bool ish[8];
        la_rel<KS>(a, c0, rr, ish);
        const long long npix = (long long)a.N * a.H * a.W;
        for (long long pix = (long long)blockIdx.x * mp.R + mp.pl; pix < npix; pix += (long long)gridDim.x * mp.R) {
            const int w = (int)(pix % a.W);
            const long long t2 = pix / a.W;
            const int h = (int)(t2 % a.H), n = (int)(t2 / a.H);
            float q[8], g[8], o[8], l[8], dq[8];
            ld8<T>((const T*)a.q + (size_t)pix * a.ldq + c0, nv, a.vec, q);
            ld8<T>((const T*)a.dout + (size_t)pix * a.lddo + c0, nv, a.vec, g);
            ld8<T>((const T*)a.o + (size_t)pix * a.ldo + c0, nv, a.vec, o);
            ld8<float>(a.lse + (size_t)pix * Cp + c0, 8, 1, l);
#pragma unroll
            for (int e = 0; e < 8; ++e) dq[e] = 0.f;
#pragma unroll
            for (int i = 0; i < KS; ++i) {
#pragma unroll
                for (int j = 0; j < KS; ++j) {
                    const int t = i * KS + j, ih = h + i - P, iw = w + j - P;
                    float kv[8], u[8], pg[8];
                    la_tap_kv<T>(a, n, ih, iw, t, KK, c0, nv, kv, u);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float kr = kv[e] + (ish[e] ? rr[e][i] : rr[e][j]);
                        pg[e] = __expf(q[e] * kr - l[e]) * g[e];
                        const float ds = pg[e] * (u[e] - o[e]);
                        dq[e] = fmaf(ds, kr, dq[e]);
                        const float dsq = ds * q[e];
                        if (ish[e]) dr[e][i] += dsq;
                        else dr[e][j] += dsq;
                    }
                    if (want_e && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W) {
                        const size_t ip = ((size_t)n * a.H + ih) * a.W + iw;
                        for (int mm = 0; mm < a.m; ++mm) {
                            float vv[8];
                            ld8<T>((const T*)a.v + mm * a.vstride + ip * a.ldv + c0, nv, a.vec, vv);
                            float sum = 0.f;
#pragma unroll
                            for (int e = 0; e < 8; ++e) sum = fmaf(pg[e], vv[e], sum);
                            ecol[(mm * KK + t) * BT + threadIdx.x] += sum;
                        }
                    }
                }
            }
            st8<T>((T*)a.dq + (size_t)pix * a.lddq + c0, nv, a.vec, dq, a.acc);
        }
    }
    if (want_rel) {
        // fold the R pixel lanes of every channel group, one window index at a time, in lane order
        const int cpp = (a.C + 7) / 8, cpb = cpp < BT ? cpp : BT;
#pragma unroll
        for (int i = 0; i < KS; ++i) {
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 8; ++e) red[threadIdx.x * 8 + e] = dr[e][i];
            __syncthreads();
            if ((int)threadIdx.x < cpb && mp.live) {             // pixel lane 0 of its channel group
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float sum = 0.f;
                    for (int lnp = 0; lnp < mp.R; ++lnp) sum += red[(lnp * cpb + threadIdx.x) * 8 + e];
                    if (e < nv) a.part[((size_t)blockIdx.x * a.C + c0 + e) * KS + i] = sum;
                }
            }
        }
    }
    if (want_e) {
        __syncthreads();
        float* pe = a.part + a.eoff + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * MT;
        for (int j = threadIdx.x; j < MT; j += BT) {
            float sum = 0.f;
            for (int lnp = 0; lnp < BT; ++lnp) sum += ecol[j * BT + ((lnp + j) & (BT - 1))];      // rotated start: no bank conflict
            pe[j] = sum;
        }
    }
}

// d rel_h / d rel_w += the block partials, in block order
__global__ __launch_bounds__(256) void la_rel_merge_kernel(const float* __restrict__ part, float* __restrict__ drel_h,
                                                           float* __restrict__ drel_w, int nblk, int C, int KS) {
    const int i = blockIdx.x * 256 + threadIdx.x, n = C * KS;
    if (i >= n) return;
    float s = 0.f;
    for (int b = 0; b < nblk; ++b) s += part[(size_t)b * n + i];
    const int c = i / KS, idx = i % KS, half = C / 2;
    if (c < half) drel_h[c * KS + idx] += s;
    else drel_w[(c - half) * KS + idx] += s;
}
// dE = the block partials, in block order
__global__ __launch_bounds__(256) void la_e_merge_kernel(const float* __restrict__ part, float* __restrict__ de, int nblk, int MT) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= MT) return;
    float s = 0.f;
    for (int b = 0; b < nblk; ++b) s += part[(size_t)b * MT + i];
    de[i] = s;
}

// ------------------------------------------------------------------------------------------------------
// backward, input-position side: dK and dV^m
// ------------------------------------------------------------------------------------------------------
template <typename T, int KS, int M>
__global__ __launch_bounds__(256) void la_bwd_kv_kernel(const LaArgs a) {
    constexpr int KK = KS * KS, P = KS / 2;
    const LaMap mp = la_map(a.C);
    if (!mp.live) return;
    const int c0 = mp.c0, nv = mp.nv, Cp = (a.C + 7) / 8 * 8;
    float rr[8][KS];
    bool ish[8];
    la_rel<KS>(a, c0, rr, ish);
    const long long npix = (long long)a.N * a.H * a.W;
    for (long long pix = (long long)blockIdx.x * mp.R + mp.pl; pix < npix; pix += (long long)gridDim.x * mp.R) {
        const int w = (int)(pix % a.W);
        const long long t2 = pix / a.W;
        const int h = (int)(t2 % a.H), n = (int)(t2 / a.H);
        float kx[8], vx[M][8], dk[8], dv[M][8];
        ld8<T>((const T*)a.k + (size_t)pix * a.ldk + c0, nv, a.vec, kx);
#pragma unroll
        for (int mm = 0; mm < M; ++mm) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { vx[mm][e] = 0.f; dv[mm][e] = 0.f; }
            if (mm < a.m) ld8<T>((const T*)a.v + mm * a.vstride + (size_t)pix * a.ldv + c0, nv, a.vec, vx[mm]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) dk[e] = 0.f;
#pragma unroll
        for (int i = 0; i < KS; ++i) {
#pragma unroll
            for (int j = 0; j < KS; ++j) {
                const int oh = h - i + P, ow = w - j + P;        // the output pixel that reads (h, w) as its tap (i, j)
                if ((unsigned)oh >= (unsigned)a.H || (unsigned)ow >= (unsigned)a.W) continue;
                const size_t op = ((size_t)n * a.H + oh) * a.W + ow;
                float q[8], g[8], o[8], l[8], em[M];
                ld8<T>((const T*)a.q + op * a.ldq + c0, nv, a.vec, q);
                ld8<T>((const T*)a.dout + op * a.lddo + c0, nv, a.vec, g);
                ld8<T>((const T*)a.o + op * a.ldo + c0, nv, a.vec, o);
                ld8<float>(a.lse + op * Cp + c0, 8, 1, l);
#pragma unroll
                for (int mm = 0; mm < M; ++mm) em[mm] = mm < a.m ? (a.emb ? a.emb[mm * KK + i * KS + j] : 1.f) : 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float kr = kx[e] + (ish[e] ? rr[e][i] : rr[e][j]);
                    const float pg = __expf(q[e] * kr - l[e]) * g[e];
                    float u = 0.f;
#pragma unroll
                    for (int mm = 0; mm < M; ++mm) {
                        u = fmaf(em[mm], vx[mm][e], u);
                        dv[mm][e] = fmaf(em[mm], pg, dv[mm][e]);
                    }
                    dk[e] = fmaf(pg * (u - o[e]), q[e], dk[e]);
                }
            }
        }
        st8<T>((T*)a.dk + (size_t)pix * a.lddk + c0, nv, a.vec, dk, a.acc);
#pragma unroll
        for (int mm = 0; mm < M; ++mm)
            if (mm < a.m) st8<T>((T*)a.dv + mm * a.dvstride + (size_t)pix * a.lddv + c0, nv, a.vec, dv[mm], a.acc);
    }
}

// ------------------------------------------------------------------------------------------------------
// host entry points
// ------------------------------------------------------------------------------------------------------
static int la_check(int dtype, const LaArgs& a, int ks) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "dtype must be YDL_F32 or YDL_BF16");
    YDL_CHECK(a.q && a.k && a.v, "q, k and v are required");
    YDL_CHECK(a.N > 0 && a.H > 0 && a.W > 0 && a.C > 0, "empty shape");
    YDL_CHECK(ks == 1 || ks == 3 || ks == 5 || ks == 7, "window size must be 1, 3, 5 or 7");
    YDL_CHECK(a.m >= 1 && a.m <= LA_MAXM && a.m * ks * ks <= LA_MAX_MT, "1 <= m <= 8 value tensors, m*ks*ks <= 196");
    YDL_CHECK(a.ldq >= a.C && a.ldk >= a.C && a.ldv >= a.C, "row strides smaller than the channel count");
    YDL_CHECK((a.rel_h == nullptr) == (a.rel_w == nullptr), "rel_h and rel_w come together");
    YDL_CHECK(!a.rel_h || a.C % 2 == 0, "the rel_h / rel_w split needs an even channel count");
    YDL_CHECK(a.emb || a.m == 1, "m > 1 value tensors need the mixing table");
    return 0;
}
static bool la_rows16(int dtype, const void* p, long long ld) {
    const int V = dtype == YDL_F32 ? 4 : 8;
    return !p || (aligned16(p) && ld % V == 0);
}
static dim3 la_grid(const LaArgs& a, int BT, int cap) {
    const int cpp = (a.C + 7) / 8, cpb = cpp < BT ? cpp : BT, R = BT / cpb;
    long long gx = ((long long)a.N * a.H * a.W + R - 1) / R;
    if (gx > cap) gx = cap;
    return dim3((unsigned)gx, (unsigned)((cpp + BT - 1) / BT));
}

#define LA_KS_SWITCH(ks, CALL) \
    do {                       \
        if (ks == 1) { CALL(1); } else if (ks == 3) { CALL(3); } else if (ks == 5) { CALL(5); } else { CALL(7); } \
    } while (0)

extern "C" int ydl_local_attn_fwd(int dtype, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int64_t v_stride,
                                  int m, const float* rel_h, const float* rel_w, const float* emb, void* out, int ldo, float* lse,
                                  int N, int H, int W, int C, int ks, void* stream) {
    LaArgs a = {};
    a.q = q; a.k = k; a.v = v; a.out = out; a.lse = lse; a.rel_h = rel_h; a.rel_w = rel_w; a.emb = emb;
    a.vstride = v_stride; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.N = N; a.H = H; a.W = W; a.C = C; a.m = m;
    if (int rc = la_check(dtype, a, ks)) return rc;
    YDL_CHECK(out && ldo >= C, "out is required, with a row stride of at least C");
    YDL_CHECK(!lse || aligned16(lse), "lse must be 16-byte aligned");
    a.vec = la_rows16(dtype, q, ldq) && la_rows16(dtype, k, ldk) && la_rows16(dtype, v, ldv) && la_rows16(dtype, v, v_stride) &&
            la_rows16(dtype, out, ldo);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid = la_grid(a, 256, 4096);
#define LA_FWD(KSV)                                                                        \
    if (dtype == YDL_F32) la_fwd_kernel<float, KSV><<<grid, 256, 0, st>>>(a);              \
    else la_fwd_kernel<bf16_t, KSV><<<grid, 256, 0, st>>>(a)
    LA_KS_SWITCH(ks, LA_FWD);
#undef LA_FWD
    YDL_LAUNCH_CHECK();
    return 0;
}

static int64_t la_rel_floats(int C, int ks) { return (int64_t)LA_MAXBLK * C * ks; }
extern "C" int64_t ydl_local_attn_bwd_ws_bytes(int C, int ks, int m) {
    if (C <= 0 || ks <= 0 || m <= 0) return 0;
    const int64_t gy = ((C + 7) / 8 + 63) / 64;              // grid.y at the smallest block the kernel is launched with
    return (la_rel_floats(C, ks) + (int64_t)LA_MAXBLK * gy * m * ks * ks) * (int64_t)sizeof(float);
}

extern "C" int ydl_local_attn_bwd(int dtype, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int64_t v_stride,
                                  int m, const float* rel_h, const float* rel_w, const float* emb, const void* out, int ldo,
                                  const float* lse, const void* dout, int lddo, void* dq, void* dk, void* dv, int ldd,
                                  int64_t dv_stride, int accumulate, float* drel_h, float* drel_w, float* demb, float* ws,
                                  int N, int H, int W, int C, int ks, void* stream) {
    LaArgs a = {};
    a.q = q; a.k = k; a.v = v; a.o = out; a.dout = dout; a.lse = (float*)lse; a.rel_h = rel_h; a.rel_w = rel_w; a.emb = emb;
    a.dq = dq; a.dk = dk; a.dv = dv; a.part = ws;
    a.vstride = v_stride; a.dvstride = dv_stride; a.eoff = la_rel_floats(C, ks);
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.lddo = lddo; a.lddq = ldd; a.lddk = ldd; a.lddv = ldd;
    a.N = N; a.H = H; a.W = W; a.C = C; a.m = m; a.acc = accumulate;
    if (int rc = la_check(dtype, a, ks)) return rc;
    YDL_CHECK(out && lse && dout && dq && dk && dv, "out, lse, dout, dq, dk and dv are required");
    YDL_CHECK(ldo >= C && lddo >= C && ldd >= C, "row strides smaller than the channel count");
    YDL_CHECK(aligned16(lse), "lse must be 16-byte aligned");
    YDL_CHECK((drel_h == nullptr) == (drel_w == nullptr) && (!drel_h || rel_h), "d rel_h and d rel_w come together, with rel given");
    YDL_CHECK(!demb || emb, "dE needs the mixing table");
    YDL_CHECK(!(drel_h || demb) || ws, "workspace of ydl_local_attn_bwd_ws_bytes() required for the parameter gradients");
    a.vec = la_rows16(dtype, q, ldq) && la_rows16(dtype, k, ldk) && la_rows16(dtype, v, ldv) && la_rows16(dtype, v, v_stride) &&
            la_rows16(dtype, out, ldo) && la_rows16(dtype, dout, lddo) && la_rows16(dtype, dq, ldd) && la_rows16(dtype, dk, ldd) &&
            la_rows16(dtype, dv, ldd) && la_rows16(dtype, dv, dv_stride);
    hipStream_t st = (hipStream_t)stream;
    const int want_rel = drel_h != nullptr, want_e = demb != nullptr;
    const int MT = m * ks * ks;
    // the dE columns take MT * block floats of LDS: the widest block that keeps them under 48 KiB
    const int BT = !want_e ? 256 : MT <= 48 ? 256 : MT <= 96 ? 128 : 64;
    const size_t lds = want_e ? (size_t)MT * BT * sizeof(float) : 0;
    const dim3 gq = la_grid(a, BT, LA_MAXBLK);
#define LA_BQ(KSV)                                                                                              \
    if (dtype == YDL_F32) la_bwd_q_kernel<float, KSV><<<gq, BT, lds, st>>>(a, want_rel, want_e);                \
    else la_bwd_q_kernel<bf16_t, KSV><<<gq, BT, lds, st>>>(a, want_rel, want_e)
    LA_KS_SWITCH(ks, LA_BQ);
#undef LA_BQ
    if (want_rel) la_rel_merge_kernel<<<(C * ks + 255) / 256, 256, 0, st>>>(ws, drel_h, drel_w, (int)gq.x, C, ks);
    if (want_e) la_e_merge_kernel<<<(MT + 255) / 256, 256, 0, st>>>(ws + a.eoff, demb, (int)(gq.x * gq.y), MT);
    const dim3 gkv = la_grid(a, 256, 4096);
#define LA_BKV(KSV)                                                                                             \
    if (dtype == YDL_F32) {                                                                                     \
        if (m == 1) la_bwd_kv_kernel<float, KSV, 1><<<gkv, 256, 0, st>>>(a);                                    \
        else if (m <= 4) la_bwd_kv_kernel<float, KSV, 4><<<gkv, 256, 0, st>>>(a);                               \
        else la_bwd_kv_kernel<float, KSV, 8><<<gkv, 256, 0, st>>>(a);                                           \
    } else {                                                                                                    \
        if (m == 1) la_bwd_kv_kernel<bf16_t, KSV, 1><<<gkv, 256, 0, st>>>(a);                                   \
        else if (m <= 4) la_bwd_kv_kernel<bf16_t, KSV, 4><<<gkv, 256, 0, st>>>(a);                              \
        else la_bwd_kv_kernel<bf16_t, KSV, 8><<<gkv, 256, 0, st>>>(a);                                          \
    }
    LA_KS_SWITCH(ks, LA_BKV);
#undef LA_BKV
    YDL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// AttentionStem mixing table (models/common.py:1600-1603): E[m][i*ks + j] = softmax over m of la[m][i] + lb[m][j],
// la = emb_mix @ emb_a, lb = emb_mix @ emb_b; emb_mix [m][Cg], emb_a / emb_b [Cg][ks].  One block each way.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stem_table_fwd_kernel(const float* __restrict__ mix, const float* __restrict__ ea,
                                                             const float* __restrict__ eb, float* __restrict__ E, int m, int Cg, int ks) {
    __shared__ float lab[2 * LA_MAXM * 7];           // la[m][ks] | lb[m][ks]
    const int mk = m * ks;
    for (int q = threadIdx.x; q < 2 * mk; q += blockDim.x) {
        const int which = q / mk, mm = (q % mk) / ks, i = q % ks;
        const float* tab = which ? eb : ea;
        float s = 0.f;
        for (int c = 0; c < Cg; ++c) s = fmaf(mix[mm * Cg + c], tab[c * ks + i], s);
        lab[q] = s;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < ks * ks; t += blockDim.x) {
        const int i = t / ks, j = t % ks;
        float mx = -3.0e38f;
        for (int mm = 0; mm < m; ++mm) mx = fmaxf(mx, lab[mm * ks + i] + lab[mk + mm * ks + j]);
        float s = 0.f;
        for (int mm = 0; mm < m; ++mm) s += expf(lab[mm * ks + i] + lab[mk + mm * ks + j] - mx);
        for (int mm = 0; mm < m; ++mm) E[mm * ks * ks + t] = expf(lab[mm * ks + i] + lab[mk + mm * ks + j] - mx) / s;
    }
}
__global__ __launch_bounds__(256) void stem_table_bwd_kernel(const float* __restrict__ mix, const float* __restrict__ ea,
                                                             const float* __restrict__ eb, const float* __restrict__ E,
                                                             const float* __restrict__ dE, float* __restrict__ dmix, float* __restrict__ dea,
                                                             float* __restrict__ deb, int m, int Cg, int ks) {
    __shared__ float dlg[LA_MAX_MT + 60];            // d logit [m][ks*ks]
    __shared__ float dlab[2 * LA_MAXM * 7];          // d la[m][ks] | d lb[m][ks]
    const int KK = ks * ks, mk = m * ks;
    for (int t = threadIdx.x; t < KK; t += blockDim.x) {
        float dot = 0.f;
        for (int mm = 0; mm < m; ++mm) dot = fmaf(E[mm * KK + t], dE[mm * KK + t], dot);
        for (int mm = 0; mm < m; ++mm) dlg[mm * KK + t] = E[mm * KK + t] * (dE[mm * KK + t] - dot);
    }
    __syncthreads();
    for (int q = threadIdx.x; q < 2 * mk; q += blockDim.x) {
        const int which = q / mk, mm = (q % mk) / ks, i = q % ks;
        float s = 0.f;
        for (int j = 0; j < ks; ++j) s += which ? dlg[mm * KK + j * ks + i] : dlg[mm * KK + i * ks + j];
        dlab[q] = s;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < m * Cg; q += blockDim.x) {
        const int mm = q / Cg, c = q % Cg;
        float s = 0.f;
        for (int i = 0; i < ks; ++i) s = fmaf(dlab[mm * ks + i], ea[c * ks + i], fmaf(dlab[mk + mm * ks + i], eb[c * ks + i], s));
        dmix[q] += s;
    }
    for (int q = threadIdx.x; q < Cg * ks; q += blockDim.x) {
        const int c = q / ks, i = q % ks;
        float sa = 0.f, sb = 0.f;
        for (int mm = 0; mm < m; ++mm) {
            sa = fmaf(mix[mm * Cg + c], dlab[mm * ks + i], sa);
            sb = fmaf(mix[mm * Cg + c], dlab[mk + mm * ks + i], sb);
        }
        dea[q] += sa;
        deb[q] += sb;
    }
}
static int stem_check(const void* a, const void* b, const void* c, const void* d, int m, int Cg, int ks) {
    YDL_CHECK(a && b && c && d, "null pointer");
    YDL_CHECK((ks == 1 || ks == 3 || ks == 5 || ks == 7) && m >= 1 && m <= LA_MAXM && m * ks * ks <= LA_MAX_MT && Cg > 0,
              "window size 1, 3, 5 or 7; 1 <= m <= 8; m*ks*ks <= 196");
    return 0;
}
extern "C" int ydl_attn_stem_table_fwd(const float* emb_mix, const float* emb_a, const float* emb_b, float* emb, int m, int Cg, int ks,
                                       void* stream) {
    if (int rc = stem_check(emb_mix, emb_a, emb_b, emb, m, Cg, ks)) return rc;
    stem_table_fwd_kernel<<<1, 256, 0, (hipStream_t)stream>>>(emb_mix, emb_a, emb_b, emb, m, Cg, ks);
    YDL_LAUNCH_CHECK();
    return 0;
}
extern "C" int ydl_attn_stem_table_bwd(const float* emb_mix, const float* emb_a, const float* emb_b, const float* emb, const float* demb,
                                       float* d_emb_mix, float* d_emb_a, float* d_emb_b, int m, int Cg, int ks, void* stream) {
    if (int rc = stem_check(emb_mix, emb_a, emb_b, emb, m, Cg, ks)) return rc;
    YDL_CHECK(demb && d_emb_mix && d_emb_a && d_emb_b, "null pointer");
    stem_table_bwd_kernel<<<1, 256, 0, (hipStream_t)stream>>>(emb_mix, emb_a, emb_b, emb, demb, d_emb_mix, d_emb_a, d_emb_b, m, Cg, ks);
    YDL_LAUNCH_CHECK();
    return 0;
}
