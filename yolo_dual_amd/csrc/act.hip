// The learnable Conv activations that do not fit the BatchNorm apply kernels: AconC (utils/activations.py) and the max merge of
// FReLU.  Streaming passes over NHWC tensors with 16-byte accesses in the lane layout of bn.hip (common.h: Lay).  No float atomics:
// the per-channel sums of the AconC backward go through one partial row per CTA and a fixed-order fold, so the same launches serve
// throughput and deterministic mode and two runs give the same bits.
#include "common.h"

#define ACON_MAX_PARTIALS 1024

// ------------------------------------------------------------------------------------------------------
// AconC:  out = d * sigmoid(beta * d) + p2 * z,  d = (p1 - p2) * z,  per channel.
// beta is read at beta[sample * beta_stride + c]: beta_stride = 0 is AconC's one row for the whole batch, a per-sample row is what
// MetaAconC's generated beta needs.  p1 / p2 / beta rows hold C floats: channels [C, Cp) are computed with zeros.
// ------------------------------------------------------------------------------------------------------
template <typename T, bool PS>
__global__ __launch_bounds__(256) void acon_fwd_kernel(const T* __restrict__ z, int ldz, const float* __restrict__ p1,
                                                       const float* __restrict__ p2, const float* __restrict__ beta, long long bstride,
                                                       T* __restrict__ out, int ldo, long long npix, long long hw, int C, int Cp) {
    constexpr int V = ET<T>::V;
    const Lay L = make_lay<V>(Cp);
    if (!L.live) return;
    // the rows hold C floats: a clamped index keeps the loads unconditional (a predicated load per element compiled to a branch and
    // a wait each, 24 dependent round trips per thread), the select afterwards zeroes the channel tail
    float dp[V], q2[V], bt[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const int c = L.c + e, cc = c < C ? c : C - 1;
        const float a1 = p1[cc], a2 = p2[cc], b0 = PS ? 0.f : beta[cc];
        const bool ok = c < C;
        q2[e] = ok ? a2 : 0.f;
        dp[e] = ok ? a1 - a2 : 0.f;
        bt[e] = ok ? b0 : 0.f;
    }
    const long long stride = (long long)gridDim.x * L.R;
    for (long long pix = (long long)blockIdx.x * L.R + L.pl; pix < npix; pix += stride) {
        if (PS) {
            const float* br = beta + (pix / hw) * bstride;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int c = L.c + e;
                const float b0 = br[c < C ? c : C - 1];
                bt[e] = c < C ? b0 : 0.f;
            }
        }
        float v[V];
        unpack16<T>(*(const uint4*)(z + pix * ldz + L.c), v);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float d = dp[e] * v[e];
            v[e] = d * sigmoid_f(bt[e] * d) + q2[e] * v[e];
        }
        *(uint4*)(out + pix * ldo + L.c) = pack16<T>(v);
    }
}

extern "C" int ydl_acon_fwd(int dtype, const void* z, int ldz, const float* p1, const float* p2, const float* beta,
                            int64_t beta_stride, void* out, int ldo, int64_t npix, int64_t hw, int C, int Cp, void* stream) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "bad dtype");
    const int V = dtype == YDL_F32 ? 4 : 8;
    YDL_CHECK(z && out && p1 && p2 && beta, "null pointer");
    YDL_CHECK(npix > 0 && hw > 0 && npix % hw == 0 && beta_stride >= 0, "npix must be whole samples of hw pixels");
    YDL_CHECK(C > 0 && Cp >= C && Cp % V == 0 && ldz >= Cp && ldo >= Cp && ldz % V == 0 && ldo % V == 0,
              "Cp must be a chunk multiple covered by the strides");
    YDL_CHECK(aligned16(z) && aligned16(out), "16-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    dim3 grid = lay_grid(npix, Cp, V, 256 * 8);
#define YDL_ACON_FWD(T, PS) \
    acon_fwd_kernel<T, PS><<<grid, 256, 0, st>>>((const T*)z, ldz, p1, p2, beta, (long long)beta_stride, (T*)out, ldo, npix, hw, C, Cp)
    if (dtype == YDL_F32) {
        if (beta_stride) YDL_ACON_FWD(float, true);
        else YDL_ACON_FWD(float, false);
    } else {
        if (beta_stride) YDL_ACON_FWD(bf16_t, true);
        else YDL_ACON_FWD(bf16_t, false);
    }
    YDL_LAUNCH_CHECK();
    return 0;
}

// Backward, one pass over z and dout.  With s = sigmoid(beta * d) and g = d(d * s)/dd = s * (1 + beta * d * (1 - s)):
//   dz = dout * ((p1 - p2) * g + p2),  dp1 = sum dout * z * g,  dp2 = sum dout * z * (1 - g),  dbeta = sum dout * d^2 * s * (1 - s).
// blockIdx.z is a SEGMENT of seg_pix pixels that shares one beta row (the whole tensor for beta_stride = 0, one sample otherwise);
// CTA (x, z) writes partial row part[z * gridDim.x + x] = [3][Cp] with a fixed pixel -> CTA assignment.
template <typename T>
__global__ __launch_bounds__(256) void acon_bwd_kernel(const T* __restrict__ z, int ldz, const T* __restrict__ dout, int lddo,
                                                       const float* __restrict__ p1, const float* __restrict__ p2,
                                                       const float* __restrict__ beta, long long bstride, T* __restrict__ dz, int lddz,
                                                       int dz_acc, float* __restrict__ part, long long seg_pix, int C, int Cp) {
    constexpr int V = ET<T>::V;
    const Lay L = make_lay<V>(Cp);
    float s1[V], s2[V], s3[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { s1[e] = 0.f; s2[e] = 0.f; s3[e] = 0.f; }
    if (L.live) {
        const float* br = beta + (long long)blockIdx.z * bstride;
        float dp[V], q2[V], bt[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {          // clamped index, then select: see acon_fwd_kernel
            const int c = L.c + e, cc = c < C ? c : C - 1;
            const float a1 = p1[cc], a2 = p2[cc], b0 = br[cc];
            const bool ok = c < C;
            q2[e] = ok ? a2 : 0.f;
            dp[e] = ok ? a1 - a2 : 0.f;
            bt[e] = ok ? b0 : 0.f;
        }
        const long long base = (long long)blockIdx.z * seg_pix;
        const long long stride = (long long)gridDim.x * L.R;
        for (long long pl = (long long)blockIdx.x * L.R + L.pl; pl < seg_pix; pl += stride) {
            const long long pix = base + pl;
            float zv[V], dv[V], o[V];
            unpack16<T>(*(const uint4*)(z + pix * ldz + L.c), zv);
            unpack16<T>(*(const uint4*)(dout + pix * lddo + L.c), dv);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float d = dp[e] * zv[e];
                const float s = sigmoid_f(bt[e] * d);
                const float sm = s * (1.f - s);
                const float g = s + bt[e] * d * sm;
                const float dzv = dv[e] * zv[e];
                o[e] = dv[e] * (dp[e] * g + q2[e]);
                s1[e] += dzv * g;
                s2[e] += dzv * (1.f - g);
                s3[e] += dv[e] * d * d * sm;
            }
            T* dst = dz + pix * lddz + L.c;
            if (dz_acc) {
                float old[V];
                unpack16<T>(*(const uint4*)dst, old);
#pragma unroll
                for (int e = 0; e < V; ++e) o[e] += old[e];
            }
            *(uint4*)dst = pack16<T>(o);
        }
    }
    // fold the CTA's pixel lanes through LDS in lane order
    __shared__ float red[256 * 3 * 8];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        red[(threadIdx.x * 3 + 0) * V + e] = s1[e];
        red[(threadIdx.x * 3 + 1) * V + e] = s2[e];
        red[(threadIdx.x * 3 + 2) * V + e] = s3[e];
    }
    __syncthreads();
    if (threadIdx.x < L.cpb && L.live) {
        float* dst = part + ((size_t)blockIdx.z * gridDim.x + blockIdx.x) * 3 * Cp;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float a = 0.f, b = 0.f, c = 0.f;
            for (int l = 0; l < L.R; ++l) {
                const int tt = l * L.cpb + threadIdx.x;
                a += red[(tt * 3 + 0) * V + e];
                b += red[(tt * 3 + 1) * V + e];
                c += red[(tt * 3 + 2) * V + e];
            }
            dst[L.c + e] = a;
            dst[Cp + L.c + e] = b;
            dst[2 * Cp + L.c + e] = c;
        }
    }
}

// 8 channels x 32 slices per CTA, rows summed in double in a fixed order; dp1 / dp2 take the sum over all segments, dbeta one row per
// segment (row stride bstride).  accumulate != 0 adds to what the rows hold (the convention of the BatchNorm gradient rows).
__global__ __launch_bounds__(256) void acon_fold_kernel(const float* __restrict__ part, int nblk, int nseg, int Cp, int C, float* dp1,
                                                        float* dp2, float* dbeta, long long bstride, int accumulate) {
    __shared__ double sh[3][32][9];
    const int cl = threadIdx.x & 7, sl = threadIdx.x >> 3;
    const int c = blockIdx.x * 8 + cl;
    const int cc = c < Cp ? c : Cp - 1;
    double t1 = 0.0, t2 = 0.0;
    for (int seg = 0; seg < nseg; ++seg) {
        const float* rows = part + (size_t)seg * nblk * 3 * Cp;
        double a = 0.0, b = 0.0, d = 0.0;
        for (int i = sl; i < nblk; i += 32) {
            a += (double)rows[(size_t)i * 3 * Cp + cc];
            b += (double)rows[(size_t)i * 3 * Cp + Cp + cc];
            d += (double)rows[(size_t)i * 3 * Cp + 2 * Cp + cc];
        }
        sh[0][sl][cl] = a; sh[1][sl][cl] = b; sh[2][sl][cl] = d;
        __syncthreads();
        if (sl == 0 && c < C) {
            double ta = 0.0, tb = 0.0, td = 0.0;
            for (int i = 0; i < 32; ++i) { ta += sh[0][i][cl]; tb += sh[1][i][cl]; td += sh[2][i][cl]; }
            t1 += ta; t2 += tb;
            float* db = dbeta + (long long)seg * bstride + c;
            *db = (accumulate ? *db : 0.f) + (float)td;
        }
        __syncthreads();
    }
    if (sl == 0 && c < C) {
        dp1[c] = (accumulate ? dp1[c] : 0.f) + (float)t1;
        dp2[c] = (accumulate ? dp2[c] : 0.f) + (float)t2;
    }
}

static inline void acon_segments(int64_t npix, int64_t hw, int64_t beta_stride, int64_t& nseg, int64_t& seg_pix) {
    nseg = beta_stride ? npix / hw : 1;
    seg_pix = beta_stride ? hw : npix;
}

extern "C" int64_t ydl_acon_bwd_ws_bytes(int64_t npix, int64_t hw, int64_t beta_stride, int Cp) {
    if (npix <= 0 || hw <= 0 || Cp <= 0) return 0;
    int64_t nseg, seg_pix;
    acon_segments(npix, hw, beta_stride, nseg, seg_pix);
    return nseg * ACON_MAX_PARTIALS * 3 * (int64_t)Cp * (int64_t)sizeof(float);
}

extern "C" int ydl_acon_bwd(int dtype, const void* z, int ldz, const void* dout, int lddo, const float* p1, const float* p2,
                            const float* beta, int64_t beta_stride, void* dz, int lddz, int dz_accumulate, float* dp1, float* dp2,
                            float* dbeta, int accumulate_param_grads, float* ws, int64_t npix, int64_t hw, int C, int Cp, void* stream) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "bad dtype");
    const int V = dtype == YDL_F32 ? 4 : 8;
    YDL_CHECK(z && dout && dz && p1 && p2 && beta && dp1 && dp2 && dbeta && ws, "null pointer");
    YDL_CHECK(npix > 0 && hw > 0 && npix % hw == 0 && beta_stride >= 0, "npix must be whole samples of hw pixels");
    YDL_CHECK(C > 0 && Cp >= C && Cp % V == 0 && ldz >= Cp && lddo >= Cp && lddz >= Cp && ldz % V == 0 && lddo % V == 0 && lddz % V == 0,
              "Cp must be a chunk multiple covered by the strides");
    YDL_CHECK(aligned16(z) && aligned16(dout) && aligned16(dz), "16-byte alignment");
    int64_t nseg, seg_pix;
    acon_segments(npix, hw, beta_stride, nseg, seg_pix);
    YDL_CHECK(nseg <= 65535, "too many samples for one launch");
    hipStream_t st = (hipStream_t)stream;
    dim3 grid = lay_grid(seg_pix, Cp, V, ACON_MAX_PARTIALS);
    const int nblk = (int)grid.x;
    grid.z = (unsigned)nseg;
    if (dtype == YDL_F32)
        acon_bwd_kernel<float><<<grid, 256, 0, st>>>((const float*)z, ldz, (const float*)dout, lddo, p1, p2, beta, (long long)beta_stride,
                                                     (float*)dz, lddz, dz_accumulate, ws, seg_pix, C, Cp);
    else
        acon_bwd_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)z, ldz, (const bf16_t*)dout, lddo, p1, p2, beta,
                                                      (long long)beta_stride, (bf16_t*)dz, lddz, dz_accumulate, ws, seg_pix, C, Cp);
    acon_fold_kernel<<<(Cp + 7) / 8, 256, 0, st>>>(ws, nblk, (int)nseg, Cp, C, dp1, dp2, dbeta, (long long)beta_stride,
                                                   accumulate_param_grads);
    YDL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// FReLU's merge: out = max(a, b) element-wise.  Backward routes dout to the larger operand and gives HALF to each on a tie, torch's
// rule for torch.max(a, b).  da_acc / db_acc != 0 add to what the gradient holds, in f32 with one rounding.
// ------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void max2_fwd_kernel(const T* __restrict__ a, int lda, const T* __restrict__ b, int ldb,
                                                       T* __restrict__ out, int ldo, long long npix, int Cp) {
    constexpr int V = ET<T>::V;
    const Lay L = make_lay<V>(Cp);
    if (!L.live) return;
    const long long stride = (long long)gridDim.x * L.R;
    for (long long pix = (long long)blockIdx.x * L.R + L.pl; pix < npix; pix += stride) {
        float av[V], bv[V];
        unpack16<T>(*(const uint4*)(a + pix * lda + L.c), av);
        unpack16<T>(*(const uint4*)(b + pix * ldb + L.c), bv);
#pragma unroll
        for (int e = 0; e < V; ++e) av[e] = fmaxf(av[e], bv[e]);
        *(uint4*)(out + pix * ldo + L.c) = pack16<T>(av);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void max2_bwd_kernel(const T* __restrict__ a, int lda, const T* __restrict__ b, int ldb,
                                                       const T* __restrict__ dout, int lddo, T* __restrict__ da, int ldda, int da_acc,
                                                       T* __restrict__ db, int lddb, int db_acc, long long npix, int Cp) {
    constexpr int V = ET<T>::V;
    const Lay L = make_lay<V>(Cp);
    if (!L.live) return;
    const long long stride = (long long)gridDim.x * L.R;
    for (long long pix = (long long)blockIdx.x * L.R + L.pl; pix < npix; pix += stride) {
        float av[V], bv[V], dv[V], ga[V], gb[V];
        unpack16<T>(*(const uint4*)(a + pix * lda + L.c), av);
        unpack16<T>(*(const uint4*)(b + pix * ldb + L.c), bv);
        unpack16<T>(*(const uint4*)(dout + pix * lddo + L.c), dv);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float h = 0.5f * dv[e];
            ga[e] = av[e] > bv[e] ? dv[e] : (av[e] == bv[e] ? h : 0.f);
            gb[e] = bv[e] > av[e] ? dv[e] : (av[e] == bv[e] ? h : 0.f);
        }
        if (da != nullptr) {
            T* pa = da + pix * ldda + L.c;
            if (da_acc) {
                float old[V];
                unpack16<T>(*(const uint4*)pa, old);
#pragma unroll
                for (int e = 0; e < V; ++e) ga[e] += old[e];
            }
            *(uint4*)pa = pack16<T>(ga);
        }
        if (db != nullptr) {
            T* pb = db + pix * lddb + L.c;
            if (db_acc) {
                float old[V];
                unpack16<T>(*(const uint4*)pb, old);
#pragma unroll
                for (int e = 0; e < V; ++e) gb[e] += old[e];
            }
            *(uint4*)pb = pack16<T>(gb);
        }
    }
}

extern "C" int ydl_max2_fwd(int dtype, const void* a, int lda, const void* b, int ldb, void* out, int ldo, int64_t npix, int Cp,
                            void* stream) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "bad dtype");
    const int V = dtype == YDL_F32 ? 4 : 8;
    YDL_CHECK(a && b && out, "null pointer");
    YDL_CHECK(npix > 0 && Cp > 0 && Cp % V == 0 && lda >= Cp && ldb >= Cp && ldo >= Cp && lda % V == 0 && ldb % V == 0 && ldo % V == 0,
              "Cp must be a chunk multiple covered by the strides");
    YDL_CHECK(aligned16(a) && aligned16(b) && aligned16(out), "16-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    dim3 grid = lay_grid(npix, Cp, V, 256 * 8);
    if (dtype == YDL_F32)
        max2_fwd_kernel<float><<<grid, 256, 0, st>>>((const float*)a, lda, (const float*)b, ldb, (float*)out, ldo, npix, Cp);
    else
        max2_fwd_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)a, lda, (const bf16_t*)b, ldb, (bf16_t*)out, ldo, npix, Cp);
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int ydl_max2_bwd(int dtype, const void* a, int lda, const void* b, int ldb, const void* dout, int lddo, void* da, int ldda,
                            int da_accumulate, void* db, int lddb, int db_accumulate, int64_t npix, int Cp, void* stream) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "bad dtype");
    const int V = dtype == YDL_F32 ? 4 : 8;
    YDL_CHECK(a && b && dout && (da || db), "null pointer");
    YDL_CHECK(npix > 0 && Cp > 0 && Cp % V == 0 && lda >= Cp && ldb >= Cp && lddo >= Cp && lda % V == 0 && ldb % V == 0 && lddo % V == 0,
              "Cp must be a chunk multiple covered by the strides");
    YDL_CHECK(da == nullptr || (ldda >= Cp && ldda % V == 0 && aligned16(da)), "da must be 16-byte aligned with a stride covering Cp");
    YDL_CHECK(db == nullptr || (lddb >= Cp && lddb % V == 0 && aligned16(db)), "db must be 16-byte aligned with a stride covering Cp");
    YDL_CHECK(aligned16(a) && aligned16(b) && aligned16(dout), "16-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    dim3 grid = lay_grid(npix, Cp, V, 256 * 8);
    if (dtype == YDL_F32)
        max2_bwd_kernel<float><<<grid, 256, 0, st>>>((const float*)a, lda, (const float*)b, ldb, (const float*)dout, lddo, (float*)da, ldda,
                                                     da_accumulate, (float*)db, lddb, db_accumulate, npix, Cp);
    else
        max2_bwd_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)a, lda, (const bf16_t*)b, ldb, (const bf16_t*)dout, lddo, (bf16_t*)da,
                                                      ldda, da_accumulate, (bf16_t*)db, lddb, db_accumulate, npix, Cp);
    YDL_LAUNCH_CHECK();
    return 0;
}
