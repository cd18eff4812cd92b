// ConvNeXt block pieces on NHWC rows: LayerNorm over the channels of every pixel, bias + exact (erf) GELU, and the layer-scaled
// residual with per-sample keep factors (stochastic depth, "row" mode).  Streaming passes with 16-byte accesses and f32 arithmetic.
//
// LayerNorm gives every pixel one DPP row of 16 lanes: lane l of the row owns the chunks l, l + 16, ... of the pixel's channel row and
// keeps them in registers (K chunks per lane, K = ceil(C / V / 16), at most 64 floats), so the mean, the two-pass variance and the
// two sums of the backward are four v_add_f32_dpp each (quad_perm, row_half_mirror, row_mirror) and no LDS.  A wave handles four
// pixels, a CTA sixteen, for every served C.  GELU and the residual use the lane layout of bn.hip (common.h: Lay).
//
// No atomics.  Every per-channel sum goes through one partial row per CTA in the caller's workspace, with a fixed pixel -> CTA
// assignment, and cn_fold_kernel adds the rows in a fixed order in double: two runs give the same bits, and throughput and
// deterministic mode run the same launches.  Parameter gradients are ADDED into their destination.
#include "common.h"

#define CN_MAX_PARTIALS 1024
#define LN_MAX_C 1024

// part: [nblk][nrow][C] floats.  8 channels x 32 slices per CTA, rows summed in double in a fixed order, then dst[q][c] += total
// (a NULL dst[q] is skipped).
struct CnFoldDst { float* d[3]; };
__global__ __launch_bounds__(256) void cn_fold_kernel(const float* __restrict__ part, int nblk, int nrow, int C, CnFoldDst dst) {
    __shared__ double sh[3][32][9];
    const int cl = threadIdx.x & 7, sl = threadIdx.x >> 3;
    const int c = blockIdx.x * 8 + cl;           // C is a multiple of 8: always a live channel
    double a[3] = {0.0, 0.0, 0.0};
    for (int i = sl; i < nblk; i += 32) {
        const float* row = part + (size_t)i * nrow * C + c;
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (q < nrow) a[q] += (double)row[(size_t)q * C];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) sh[q][sl][cl] = a[q];
    __syncthreads();
    if (sl == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (q >= nrow || dst.d[q] == nullptr) continue;
            double t = 0.0;
            for (int i = 0; i < 32; ++i) t += sh[q][i][cl];
            dst.d[q][c] += (float)t;
        }
    }
}

static inline bool cn_rows_ok(int V, int C, int ld) { return ld >= C && ld % V == 0; }

// ------------------------------------------------------------------------------------------------------
// LayerNorm over C at every pixel
// ------------------------------------------------------------------------------------------------------
// sum over the 16 lanes of a DPP row, the same bits in every lane (each step adds a pair in either order)
__device__ __forceinline__ float row16_sum(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, false));      // quad_perm [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, false));      // quad_perm [2,3,0,1]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, false));     // row_half_mirror
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, false));     // row_mirror
    return v;
}

// u = x + pre_bias of chunk (p, c0), as floats.  The f32 parameter rows are read from the CTA's copy in LDS (ln_stage_rows), 16 bytes at
// a time: the optimizer keeps parameters back to back in one arena, so a row in global memory need not start on a 16-byte boundary, and
// element-wise loads of gamma, beta and pre_bias for every pixel cost more than the pixel's own row.
template <typename T>
__device__ __forceinline__ void ln_load_u(const T* __restrict__ x, long long off, const float* pb, int c0, float* u) {
    constexpr int V = ET<T>::V;
    unpack16<T>(*(const uint4*)(x + off), u);
    if (pb != nullptr) {
#pragma unroll
        for (int h = 0; h < V / 4; ++h) {
            const float4 b = *(const float4*)(pb + c0 + 4 * h);
            u[4 * h + 0] += b.x; u[4 * h + 1] += b.y; u[4 * h + 2] += b.z; u[4 * h + 3] += b.w;
        }
    }
}
template <int V>
__device__ __forceinline__ void ln_load_row(const float* p, int c0, float* f) {
#pragma unroll
    for (int h = 0; h < V / 4; ++h) {
        const float4 b = *(const float4*)(p + c0 + 4 * h);
        f[4 * h + 0] = b.x; f[4 * h + 1] = b.y; f[4 * h + 2] = b.z; f[4 * h + 3] = b.w;
    }
}
// the CTA's copy of up to three f32 parameter rows in LDS (row i at sp + i * LN_MAX_C; a NULL row is skipped)
__device__ __forceinline__ void ln_stage_rows(float* sp, const float* __restrict__ r0, const float* __restrict__ r1,
                                              const float* __restrict__ r2, int C) {
    for (int c = threadIdx.x; c < C; c += 256) {
        if (r0 != nullptr) sp[c] = r0[c];
        if (r1 != nullptr) sp[LN_MAX_C + c] = r1[c];
        if (r2 != nullptr) sp[2 * LN_MAX_C + c] = r2[c];
    }
    __syncthreads();
}

template <typename T, int K>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const T* __restrict__ x, int ldx, const float* pb,
                                                     const float* gamma, const float* beta, float eps,
                                                     T* __restrict__ y, int ldy, float* __restrict__ stats, long long npix, int C) {
    constexpr int V = ET<T>::V;
    const int l = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int cpp = C / V;
    const float fC = (float)C;
    __shared__ float sp[3 * LN_MAX_C];
    ln_stage_rows(sp, gamma, beta, pb, C);
    gamma = sp;
    beta = sp + LN_MAX_C;
    if (pb != nullptr) pb = sp + 2 * LN_MAX_C;
    for (long long base = (long long)blockIdx.x * 16; base < npix; base += (long long)gridDim.x * 16) {   // uniform per CTA
        const long long p = base + g;
        const bool live = p < npix;
        float u[K][V];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int j = k * 16 + l;
            if (live && j < cpp) {
                ln_load_u<T>(x, p * ldx + j * V, pb, j * V, u[k]);
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) u[k][e] = 0.f;
            }
#pragma unroll
            for (int e = 0; e < V; ++e) s += u[k][e];
        }
        const float mu = row16_sum(s) / fC;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (k * 16 + l < cpp) {
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    u[k][e] -= mu;
                    q += u[k][e] * u[k][e];
                }
            }
        }
        const float var = row16_sum(q) / fC;
        const float r = 1.f / sqrtf(var + eps);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int j = k * 16 + l;
            if (live && j < cpp) {
                float gm[V], bt[V];
                ln_load_row<V>(gamma, j * V, gm);
                ln_load_row<V>(beta, j * V, bt);
#pragma unroll
                for (int e = 0; e < V; ++e) u[k][e] = u[k][e] * r * gm[e] + bt[e];
                *(uint4*)(y + p * ldy + j * V) = pack16<T>(u[k]);
            }
        }
        if (stats != nullptr && live && l == 0) {
            stats[2 * p] = mu;
            stats[2 * p + 1] = r;
        }
    }
}

// One pass over x and dy.  part: this CTA's [3][C] row = (dgamma, dbeta, dpre_bias) over the pixels it walked.
template <typename T, int K>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const T* __restrict__ x, int ldx, const float* pb,
                                                     const float* gamma, const float* __restrict__ stats,
                                                     const T* __restrict__ dy, int lddy, T* __restrict__ dx, int lddx, int accumulate,
                                                     float* __restrict__ part, long long npix, int C) {
    constexpr int V = ET<T>::V;
    const int l = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int cpp = C / V;
    const float fC = (float)C;
    float ag[K][V], ab[K][V], ap[K][V];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int e = 0; e < V; ++e) { ag[k][e] = 0.f; ab[k][e] = 0.f; ap[k][e] = 0.f; }
    __shared__ float sp[2 * LN_MAX_C];
    ln_stage_rows(sp, gamma, pb, nullptr, C);
    gamma = sp;
    if (pb != nullptr) pb = sp + LN_MAX_C;
    for (long long base = (long long)blockIdx.x * 16; base < npix; base += (long long)gridDim.x * 16) {
        const long long p = base + g;
        const bool live = p < npix;
        const float mu = live ? stats[2 * p] : 0.f, r = live ? stats[2 * p + 1] : 0.f;
        float xh[K][V], gv[K][V];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int j = k * 16 + l;
            if (live && j < cpp) {
                float d[V], gm[V];
                ln_load_u<T>(x, p * ldx + j * V, pb, j * V, xh[k]);
                unpack16<T>(*(const uint4*)(dy + p * lddy + j * V), d);
                ln_load_row<V>(gamma, j * V, gm);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    xh[k][e] = (xh[k][e] - mu) * r;
                    gv[k][e] = d[e] * gm[e];
                    ag[k][e] += d[e] * xh[k][e];
                    ab[k][e] += d[e];
                    s1 += gv[k][e];
                    s2 += gv[k][e] * xh[k][e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) { xh[k][e] = 0.f; gv[k][e] = 0.f; }
            }
        }
        const float m1 = row16_sum(s1) / fC, m2 = row16_sum(s2) / fC;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int j = k * 16 + l;
            if (live && j < cpp) {
                float o[V];
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    o[e] = r * (gv[k][e] - m1 - xh[k][e] * m2);
                    ap[k][e] += o[e];
                }
                T* dst = dx + p * lddx + j * V;
                if (accumulate) {
                    float old[V];
                    unpack16<T>(*(const uint4*)dst, old);
#pragma unroll
                    for (int e = 0; e < V; ++e) o[e] += old[e];
                }
                *(uint4*)dst = pack16<T>(o);
            }
        }
    }
    // fold the CTA's sixteen pixel rows in row order, one (quantity, k) at a time
    __shared__ float red[256 * 8];
    float* row = part + (size_t)blockIdx.x * 3 * C;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float* src = q == 0 ? ag[k] : (q == 1 ? ab[k] : ap[k]);
#pragma unroll
            for (int e = 0; e < V; ++e) red[threadIdx.x * V + e] = src[e];
            __syncthreads();
            // one thread per (lane of the row, element): 16 V threads each add the sixteen rows' values in row order
            const int fl = threadIdx.x / V, fe = threadIdx.x % V;
            const int j = k * 16 + fl;
            if (fl < 16 && j < cpp) {
                float a = 0.f;
#pragma unroll
                for (int gg = 0; gg < 16; ++gg) a += red[(gg * 16 + fl) * V + fe];
                row[(size_t)q * C + j * V + fe] = a;
            }
            __syncthreads();
        }
    }
}

extern "C" int ydl_ln_supported(int C) { return C >= 8 && C <= LN_MAX_C && C % 8 == 0; }

static inline int ln_blocks(int64_t npix) {
    int64_t b = (npix + 15) / 16;
    return (int)(b > CN_MAX_PARTIALS ? CN_MAX_PARTIALS : b);
}
static inline int ln_k(int dtype, int C) { return (C / (dtype == YDL_F32 ? 4 : 8) + 15) / 16; }

#define YDL_LN_DISPATCH(T, need, GO)                                    \
    do {                                                                \
        if (need <= 1) GO(T, 1); else if (need <= 2) GO(T, 2);          \
        else if (need <= 3) GO(T, 3); else if (need <= 4) GO(T, 4);     \
        else if (need <= 6) GO(T, 6); else if (need <= 8) GO(T, 8);     \
        else if (need <= 12) GO(T, 12); else GO(T, 16);                 \
    } while (0)

// bf16: 8 elements per chunk, so at most 8 chunks per lane
#define YDL_LN_DISPATCH8(T, need, GO)                                   \
    do {                                                                \
        if (need <= 1) GO(T, 1); else if (need <= 2) GO(T, 2);          \
        else if (need <= 3) GO(T, 3); else if (need <= 4) GO(T, 4);     \
        else if (need <= 6) GO(T, 6); else GO(T, 8);                    \
    } while (0)

extern "C" int ydl_ln_fwd(int dtype, const void* x, int ldx, const float* pre_bias, const float* gamma, const float* beta, float eps,
                          void* y, int ldy, float* stats, int64_t npix, int C, void* stream) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "bad dtype");
    const int V = dtype == YDL_F32 ? 4 : 8;
    YDL_CHECK(x && y && gamma && beta, "null pointer");
    YDL_CHECK(ydl_ln_supported(C), "C must be a multiple of 8 in 8..1024");
    YDL_CHECK(npix > 0 && cn_rows_ok(V, C, ldx) && cn_rows_ok(V, C, ldy), "strides must be whole 16-byte chunks covering C");
    YDL_CHECK(aligned16(x) && aligned16(y), "16-byte alignment");
    YDL_CHECK(eps >= 0.f, "eps must not be negative");
    hipStream_t st = (hipStream_t)stream;
    const int grid = (int)((npix + 15) / 16 > 8192 ? 8192 : (npix + 15) / 16), need = ln_k(dtype, C);
#define YDL_LN_FWD(T, K) \
    ln_fwd_kernel<T, K><<<grid, 256, 0, st>>>((const T*)x, ldx, pre_bias, gamma, beta, eps, (T*)y, ldy, stats, (long long)npix, C)
    if (dtype == YDL_F32) YDL_LN_DISPATCH(float, need, YDL_LN_FWD);
    else YDL_LN_DISPATCH8(bf16_t, need, YDL_LN_FWD);
#undef YDL_LN_FWD
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t ydl_ln_bwd_ws_bytes(int64_t npix, int C) {
    if (npix <= 0 || !ydl_ln_supported(C)) return 0;
    return (int64_t)ln_blocks(npix) * 3 * C * (int64_t)sizeof(float);
}

extern "C" int ydl_ln_bwd(int dtype, const void* x, int ldx, const float* pre_bias, const float* gamma, const float* stats,
                          const void* dy, int lddy, void* dx, int lddx, int accumulate, float* dgamma, float* dbeta, float* dpre_bias,
                          float* ws, int64_t npix, int C, void* stream) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "bad dtype");
    const int V = dtype == YDL_F32 ? 4 : 8;
    YDL_CHECK(x && gamma && stats && dy && dx && dgamma && dbeta && ws, "null pointer");
    YDL_CHECK(ydl_ln_supported(C), "C must be a multiple of 8 in 8..1024");
    YDL_CHECK(npix > 0 && cn_rows_ok(V, C, ldx) && cn_rows_ok(V, C, lddy) && cn_rows_ok(V, C, lddx),
              "strides must be whole 16-byte chunks covering C");
    YDL_CHECK(aligned16(x) && aligned16(dy) && aligned16(dx), "16-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    const int grid = ln_blocks(npix), need = ln_k(dtype, C);
#define YDL_LN_BWD(T, K)                                                                                                            \
    ln_bwd_kernel<T, K><<<grid, 256, 0, st>>>((const T*)x, ldx, pre_bias, gamma, stats, (const T*)dy, lddy, (T*)dx, lddx, accumulate, \
                                              ws, (long long)npix, C)
    if (dtype == YDL_F32) YDL_LN_DISPATCH(float, need, YDL_LN_BWD);
    else YDL_LN_DISPATCH8(bf16_t, need, YDL_LN_BWD);
#undef YDL_LN_BWD
    CnFoldDst dst = {{dgamma, dbeta, dpre_bias}};
    cn_fold_kernel<<<C / 8, 256, 0, st>>>(ws, grid, 3, C, dst);
    YDL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// bias + exact GELU:  u = z + bias[c],  y = 0.5 * u * (1 + erf(u / sqrt 2));  dy/du = Phi(u) + u * phi(u)
// ------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void bias_gelu_fwd_kernel(const T* __restrict__ z, int ldz, const float* __restrict__ bias,
                                                            T* __restrict__ y, int ldy, long long npix, int C) {
    constexpr int V = ET<T>::V;
    const Lay L = make_lay<V>(C);
    if (!L.live) return;
    float b[V];
#pragma unroll
    for (int e = 0; e < V; ++e) b[e] = bias[L.c + e];
    const long long stride = (long long)gridDim.x * L.R;
    for (long long pix = (long long)blockIdx.x * L.R + L.pl; pix < npix; pix += stride) {
        float v[V];
        unpack16<T>(*(const uint4*)(z + pix * ldz + L.c), v);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float u = v[e] + b[e];
            v[e] = 0.5f * u * (1.f + erff(u * 0.70710678118654752f));
        }
        *(uint4*)(y + pix * ldy + L.c) = pack16<T>(v);
    }
}

// dz may be dy's own buffer: a thread reads its chunk of dy before it writes the same chunk of dz
template <typename T>
__global__ __launch_bounds__(256) void bias_gelu_bwd_kernel(const T* __restrict__ z, int ldz, const float* __restrict__ bias, const T* dy,
                                                            int lddy, T* dz, int lddz, float* __restrict__ part, long long npix, int C) {
    constexpr int V = ET<T>::V;
    const Lay L = make_lay<V>(C);
    float s[V];
#pragma unroll
    for (int e = 0; e < V; ++e) s[e] = 0.f;
    if (L.live) {
        float b[V];
#pragma unroll
        for (int e = 0; e < V; ++e) b[e] = bias[L.c + e];
        const long long stride = (long long)gridDim.x * L.R;
        for (long long pix = (long long)blockIdx.x * L.R + L.pl; pix < npix; pix += stride) {
            float v[V], d[V];
            unpack16<T>(*(const uint4*)(z + pix * ldz + L.c), v);
            unpack16<T>(*(const uint4*)(dy + pix * lddy + L.c), d);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float u = v[e] + b[e];
                const float cdf = 0.5f * (1.f + erff(u * 0.70710678118654752f));
                const float pdf = 0.3989422804014327f * expf(-0.5f * u * u);
                d[e] *= cdf + u * pdf;
                s[e] += d[e];
            }
            *(uint4*)(dz + pix * lddz + L.c) = pack16<T>(d);
        }
    }
    lay_partial_row<V>(L, s, part + (size_t)blockIdx.x * C, C);
}

extern "C" int ydl_bias_gelu_fwd(int dtype, const void* z, int ldz, const float* bias, void* y, int ldy, int64_t npix, int C,
                                 void* stream) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "bad dtype");
    const int V = dtype == YDL_F32 ? 4 : 8;
    YDL_CHECK(z && bias && y, "null pointer");
    YDL_CHECK(npix > 0 && C >= 8 && C % 8 == 0 && cn_rows_ok(V, C, ldz) && cn_rows_ok(V, C, ldy),
              "C must be a multiple of 8 and the strides whole 16-byte chunks covering it");
    YDL_CHECK(aligned16(z) && aligned16(y), "16-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    dim3 grid = lay_grid(npix, C, V, 256 * 8);
    if (dtype == YDL_F32) bias_gelu_fwd_kernel<float><<<grid, 256, 0, st>>>((const float*)z, ldz, bias, (float*)y, ldy, npix, C);
    else bias_gelu_fwd_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)z, ldz, bias, (bf16_t*)y, ldy, npix, C);
    YDL_LAUNCH_CHECK();
    return 0;
}

// the Lay kernels' partial rows: at most one CTA column per pixel, CN_MAX_PARTIALS at the most (an upper bound that needs no dtype)
static inline int64_t cn_lay_ws_bytes(int64_t npix, int C) {
    if (npix <= 0 || C < 8 || C % 8) return 0;
    return (npix > CN_MAX_PARTIALS ? CN_MAX_PARTIALS : npix) * C * (int64_t)sizeof(float);
}
extern "C" int64_t ydl_bias_gelu_bwd_ws_bytes(int64_t npix, int C) { return cn_lay_ws_bytes(npix, C); }

extern "C" int ydl_bias_gelu_bwd(int dtype, const void* z, int ldz, const float* bias, const void* dy, int lddy, void* dz, int lddz,
                                 float* dbias, float* ws, int64_t npix, int C, void* stream) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "bad dtype");
    const int V = dtype == YDL_F32 ? 4 : 8;
    YDL_CHECK(z && bias && dy && dz && dbias && ws, "null pointer");
    YDL_CHECK(npix > 0 && C >= 8 && C % 8 == 0 && cn_rows_ok(V, C, ldz) && cn_rows_ok(V, C, lddy) && cn_rows_ok(V, C, lddz),
              "C must be a multiple of 8 and the strides whole 16-byte chunks covering it");
    YDL_CHECK(aligned16(z) && aligned16(dy) && aligned16(dz), "16-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    dim3 grid = lay_grid(npix, C, V, CN_MAX_PARTIALS);
    if (dtype == YDL_F32)
        bias_gelu_bwd_kernel<float><<<grid, 256, 0, st>>>((const float*)z, ldz, bias, (const float*)dy, lddy, (float*)dz, lddz, ws, npix, C);
    else
        bias_gelu_bwd_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)z, ldz, bias, (const bf16_t*)dy, lddy, (bf16_t*)dz, lddz, ws, npix,
                                                           C);
    CnFoldDst dst = {{dbias, nullptr, nullptr}};
    cn_fold_kernel<<<C / 8, 256, 0, st>>>(ws, (int)grid.x, 1, C, dst);
    YDL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// layer-scaled residual:  out[n, p, c] = x + keep[n] * gamma[c] * y   (keep NULL: 1).  A sample whose keep factor is 0 copies x.
// ------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void scale_res_fwd_kernel(const T* __restrict__ y, int ldy, const float* __restrict__ gamma,
                                                            const float* __restrict__ keep, const T* __restrict__ x, int ldx,
                                                            T* __restrict__ out, int ldo, long long npix, long long hw, int C) {
    constexpr int V = ET<T>::V;
    const Lay L = make_lay<V>(C);
    if (!L.live) return;
    float gm[V];
#pragma unroll
    for (int e = 0; e < V; ++e) gm[e] = gamma[L.c + e];
    const long long stride = (long long)gridDim.x * L.R;
    for (long long pix = (long long)blockIdx.x * L.R + L.pl; pix < npix; pix += stride) {
        const float kf = keep != nullptr ? keep[pix / hw] : 1.f;
        uint4 xq = *(const uint4*)(x + pix * ldx + L.c);
        if (kf != 0.f) {
            float xv[V], yv[V];
            unpack16<T>(xq, xv);
            unpack16<T>(*(const uint4*)(y + pix * ldy + L.c), yv);
#pragma unroll
            for (int e = 0; e < V; ++e) xv[e] += (kf * gm[e]) * yv[e];
            xq = pack16<T>(xv);
        }
        *(uint4*)(out + pix * ldo + L.c) = xq;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void scale_res_bwd_kernel(const T* dout, int lddo, const T* __restrict__ y, int ldy,
                                                            const float* __restrict__ gamma, const float* __restrict__ keep, T* dy, int lddy,
                                                            T* dx, int lddx, int accumulate, float* __restrict__ part, long long npix,
                                                            long long hw, int C) {
    constexpr int V = ET<T>::V;
    const Lay L = make_lay<V>(C);
    float s[V];
#pragma unroll
    for (int e = 0; e < V; ++e) s[e] = 0.f;
    if (L.live) {
        float gm[V];
#pragma unroll
        for (int e = 0; e < V; ++e) gm[e] = gamma[L.c + e];
        const long long stride = (long long)gridDim.x * L.R;
        for (long long pix = (long long)blockIdx.x * L.R + L.pl; pix < npix; pix += stride) {
            const float kf = keep != nullptr ? keep[pix / hw] : 1.f;
            float d[V], yv[V], o[V];
            unpack16<T>(*(const uint4*)(dout + pix * lddo + L.c), d);
            unpack16<T>(*(const uint4*)(y + pix * ldy + L.c), yv);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                o[e] = (kf * gm[e]) * d[e];
                s[e] += kf * (d[e] * yv[e]);
            }
            if (dx != nullptr) {
                T* dst = dx + pix * lddx + L.c;
                if (accumulate) {
                    float old[V];
                    unpack16<T>(*(const uint4*)dst, old);
#pragma unroll
                    for (int e = 0; e < V; ++e) d[e] += old[e];
                }
                *(uint4*)dst = pack16<T>(d);
            }
            *(uint4*)(dy + pix * lddy + L.c) = pack16<T>(o);
        }
    }
    lay_partial_row<V>(L, s, part + (size_t)blockIdx.x * C, C);
}

extern "C" int ydl_scale_res_fwd(int dtype, const void* y, int ldy, const float* gamma, const float* keep, const void* x, int ldx,
                                 void* out, int ldo, int N, int64_t hw, int C, void* stream) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "bad dtype");
    const int V = dtype == YDL_F32 ? 4 : 8;
    YDL_CHECK(y && gamma && x && out, "null pointer");
    YDL_CHECK(N > 0 && hw > 0 && C >= 8 && C % 8 == 0 && cn_rows_ok(V, C, ldy) && cn_rows_ok(V, C, ldx) && cn_rows_ok(V, C, ldo),
              "C must be a multiple of 8 and the strides whole 16-byte chunks covering it");
    YDL_CHECK(aligned16(y) && aligned16(x) && aligned16(out), "16-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    const long long npix = (long long)N * hw;
    dim3 grid = lay_grid(npix, C, V, 256 * 8);
    if (dtype == YDL_F32)
        scale_res_fwd_kernel<float><<<grid, 256, 0, st>>>((const float*)y, ldy, gamma, keep, (const float*)x, ldx, (float*)out, ldo, npix,
                                                          (long long)hw, C);
    else
        scale_res_fwd_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)y, ldy, gamma, keep, (const bf16_t*)x, ldx, (bf16_t*)out, ldo,
                                                           npix, (long long)hw, C);
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t ydl_scale_res_bwd_ws_bytes(int N, int64_t hw, int C) {
    if (N <= 0 || hw <= 0) return 0;
    return cn_lay_ws_bytes((int64_t)N * hw, C);
}

extern "C" int ydl_scale_res_bwd(int dtype, const void* dout, int lddo, const void* y, int ldy, const float* gamma, const float* keep,
                                 void* dy, int lddy, void* dx, int lddx, int accumulate, float* dgamma, float* ws, int N, int64_t hw,
                                 int C, void* stream) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "bad dtype");
    const int V = dtype == YDL_F32 ? 4 : 8;
    YDL_CHECK(dout && y && gamma && dy && dgamma && ws, "null pointer");
    YDL_CHECK(N > 0 && hw > 0 && C >= 8 && C % 8 == 0 && cn_rows_ok(V, C, lddo) && cn_rows_ok(V, C, ldy) && cn_rows_ok(V, C, lddy),
              "C must be a multiple of 8 and the strides whole 16-byte chunks covering it");
    YDL_CHECK(dx == nullptr || (cn_rows_ok(V, C, lddx) && aligned16(dx)), "dx must be 16-byte aligned with a stride covering C");
    YDL_CHECK(aligned16(dout) && aligned16(y) && aligned16(dy), "16-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    const long long npix = (long long)N * hw;
    dim3 grid = lay_grid(npix, C, V, CN_MAX_PARTIALS);
    if (dtype == YDL_F32)
        scale_res_bwd_kernel<float><<<grid, 256, 0, st>>>((const float*)dout, lddo, (const float*)y, ldy, gamma, keep, (float*)dy, lddy,
                                                          (float*)dx, lddx, accumulate, ws, npix, (long long)hw, C);
    else
        scale_res_bwd_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)dout, lddo, (const bf16_t*)y, ldy, gamma, keep, (bf16_t*)dy, lddy,
                                                           (bf16_t*)dx, lddx, accumulate, ws, npix, (long long)hw, C);
    CnFoldDst dst = {{dgamma, nullptr, nullptr}};
    cn_fold_kernel<<<C / 8, 256, 0, st>>>(ws, (int)grid.x, 1, C, dst);
    YDL_LAUNCH_CHECK();
    return 0;
}
