// Squeeze-and-excitation gate on NHWC rows (torchvision's SqueezeExcitation inside MobileNetV3's InvertedResidual and EfficientNet's
// MBConv):  p = mean_hw x,  h = W1 p + b1,  a = act(h),  z = W2 a + b2,  g = scale(z),  out = x * g[n, c].
//
//   se_pool_kernel     per-sample, per-channel sums over a slice of the pixels: grid (S slices, chunk blocks, N samples), the lane
//                      layout of bn.hip (common.h: Lay), one partial row [C] per CTA.  With a second tensor it sums the products:
//                      the gate gradient dgate = sum_hw dy * x goes through the same pass.
//   se_excite_fwd      one CTA per sample: folds the S partial rows in order, divides by HW, and runs the two tiny matrix-vector
//                      products out of LDS on the f32 masters as they stand (read by element: no alignment is asked of them).
//   se_excite_bwd      one CTA per sample for dz, dh and dpooled, then one element-wise launch that sums the four parameter
//                      gradients over the samples in order.
//   se_scale_bwd       dx (+)= dy * g[n, c] + dpooled[n, c] / HW, one pass, one rounding.
//
// f32 arithmetic, no atomics, fixed summation order everywhere: two runs give the same bits, and throughput and deterministic mode
// run the same launches.  The derivative of the gate is formed from the stored argument z (and that of the activation from h), never
// from a rounded gate.
#include "common.h"

#define SE_MAX_C 2048
#define SE_MAX_CS 512
#define SE_MAX_SPLITS 64
#define SE_SPLIT_PIX 64

extern "C" int ydl_se_supported(int C, int Cs) { return C >= 8 && C <= SE_MAX_C && C % 8 == 0 && Cs >= 1 && Cs <= SE_MAX_CS; }

// slices of the pixel range per sample: about SE_SPLIT_PIX pixels each, at most SE_MAX_SPLITS, and no more than 1024 / N
extern "C" int ydl_se_pool_splits(int N, int64_t HW) {
    if (N <= 0 || HW <= 0) return 0;
    int64_t s = cdiv64(HW, SE_SPLIT_PIX);
    int64_t cap = 1024 / N;
    if (cap < 1) cap = 1;
    if (cap > SE_MAX_SPLITS) cap = SE_MAX_SPLITS;
    return (int)(s < cap ? s : cap);
}
extern "C" int64_t ydl_se_pool_ws_bytes(int N, int64_t HW, int C) {
    if (N <= 0 || HW <= 0 || C < 8 || C % 8) return 0;
    return (int64_t)N * ydl_se_pool_splits(N, HW) * C * (int64_t)sizeof(float);
}

static inline bool se_rows_ok(int V, int C, int ld) { return ld >= C && ld % V == 0; }

// part[n][s][C] = sum over the pixels [s * Lp, min((s + 1) * Lp, HW)) of x (DOT: of x * y), sample n
template <typename T, bool DOT>
__global__ __launch_bounds__(256) void se_pool_kernel(const T* __restrict__ x, int ldx, const T* __restrict__ y, int ldy,
                                                      float* __restrict__ part, long long HW, long long Lp, int C) {
    constexpr int V = ET<T>::V;
    const Lay L = make_lay<V>(C);
    const int s = blockIdx.x, S = gridDim.x, n = blockIdx.z;
    float a[V];
#pragma unroll
    for (int e = 0; e < V; ++e) a[e] = 0.f;
    if (L.live) {
        const long long p0 = (long long)s * Lp;
        const long long p1 = p0 + Lp < HW ? p0 + Lp : HW;
        const T* xb = x + (size_t)n * HW * ldx + L.c;
        const T* yb = DOT ? y + (size_t)n * HW * ldy + L.c : nullptr;
        long long p = p0 + L.pl;
        for (; p + 3LL * L.R < p1; p += 4LL * L.R) {          // four loads in flight; added in pixel order
            uint4 q[4], r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                q[u] = *(const uint4*)(xb + (p + (long long)u * L.R) * ldx);
                if (DOT) r[u] = *(const uint4*)(yb + (p + (long long)u * L.R) * ldy);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float v[V], w[V];
                unpack16<T>(q[u], v);
                if (DOT) unpack16<T>(r[u], w);
#pragma unroll
                for (int e = 0; e < V; ++e) a[e] += DOT ? v[e] * w[e] : v[e];
            }
        }
        for (; p < p1; p += L.R) {
            float v[V], w[V];
            unpack16<T>(*(const uint4*)(xb + p * ldx), v);
            if (DOT) unpack16<T>(*(const uint4*)(yb + p * ldy), w);
#pragma unroll
            for (int e = 0; e < V; ++e) a[e] += DOT ? v[e] * w[e] : v[e];
        }
    }
    lay_partial_row<V>(L, a, part + ((size_t)n * S + s) * C, C);
}

extern "C" int ydl_se_pool_fwd(int dtype, const void* x, int ldx, const void* y, int ldy, float* ws, int N, int64_t HW, int C,
                               void* stream) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "bad dtype");
    const int V = dtype == YDL_F32 ? 4 : 8;
    YDL_CHECK(x && ws, "null pointer");
    YDL_CHECK(N > 0 && N <= 65535 && HW > 0 && C >= 8 && C <= SE_MAX_C && C % 8 == 0, "N in 1..65535, HW > 0, C a multiple of 8 in 8..2048");
    YDL_CHECK(se_rows_ok(V, C, ldx) && aligned16(x), "x must be 16-byte aligned with a stride of whole chunks covering C");
    YDL_CHECK(y == nullptr || (se_rows_ok(V, C, ldy) && aligned16(y)), "y must be 16-byte aligned with a stride of whole chunks covering C");
    const int S = ydl_se_pool_splits(N, HW);
    const long long Lp = cdiv64(HW, S);
    const int cpp = C / V;
    dim3 grid((unsigned)S, (unsigned)((cpp + 255) / 256), (unsigned)N);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == YDL_F32) {
        if (y) se_pool_kernel<float, true><<<grid, 256, 0, st>>>((const float*)x, ldx, (const float*)y, ldy, ws, HW, Lp, C);
        else se_pool_kernel<float, false><<<grid, 256, 0, st>>>((const float*)x, ldx, nullptr, 0, ws, HW, Lp, C);
    } else {
        if (y) se_pool_kernel<bf16_t, true><<<grid, 256, 0, st>>>((const bf16_t*)x, ldx, (const bf16_t*)y, ldy, ws, HW, Lp, C);
        else se_pool_kernel<bf16_t, false><<<grid, 256, 0, st>>>((const bf16_t*)x, ldx, nullptr, 0, ws, HW, Lp, C);
    }
    YDL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// the excitation: two matrix-vector products per sample
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float se_act(int act, float h) {
    if (act == YDL_ACT_RELU) return fmaxf(h, 0.f);
    return h / (1.f + expf(-h));                                       // YDL_ACT_SILU
}
__device__ __forceinline__ float se_act_grad(int act, float h) {
    if (act == YDL_ACT_RELU) return h > 0.f ? 1.f : 0.f;
    const float sg = 1.f / (1.f + expf(-h));
    return sg * (1.f + h * (1.f - sg));
}
__device__ __forceinline__ float se_gate(int kind, float z) {
    if (kind == YDL_SE_GATE_HSIGMOID) return fminf(fmaxf(z + 3.f, 0.f), 6.f) / 6.f;
    return 1.f / (1.f + expf(-z));
}
// sigmoid'(z) = e / (1 + e)^2 with e = exp(-|z|): no cancellation where the gate saturates.  Hardsigmoid: 1/6 inside (-3, 3), else 0.
__device__ __forceinline__ float se_gate_grad(int kind, float z) {
    if (kind == YDL_SE_GATE_HSIGMOID) return (z > -3.f && z < 3.f) ? (1.f / 6.f) : 0.f;
    const float e = expf(-fabsf(z));
    return e / ((1.f + e) * (1.f + e));
}

__global__ __launch_bounds__(256) void se_excite_fwd_kernel(const float* __restrict__ part, int S, float hw,
                                                            const float* __restrict__ w1, const float* __restrict__ b1,
                                                            const float* __restrict__ w2, const float* __restrict__ b2, int act, int kind,
                                                            float* __restrict__ pooled, float* __restrict__ h, float* __restrict__ z,
                                                            float* __restrict__ gate, int C, int Cs) {
    __shared__ float sp[SE_MAX_C];
    __shared__ float sa[SE_MAX_CS];
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = threadIdx.x; c < C; c += 256) {
        float t = 0.f;
        for (int s = 0; s < S; ++s) t += part[((size_t)n * S + s) * C + c];
        t /= hw;
        sp[c] = t;
        pooled[(size_t)n * C + c] = t;
    }
    __syncthreads();
    for (int j = wave; j < Cs; j += 4) {
        const float* row = w1 + (size_t)j * C;
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) acc += row[c] * sp[c];
        acc = wave_sum(acc);
        if (lane == 0) {
            const float hv = acc + b1[j];
            h[(size_t)n * Cs + j] = hv;
            sa[j] = se_act(act, hv);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        const float* row = w2 + (size_t)c * Cs;
        float acc = b2[c];
        for (int j = 0; j < Cs; ++j) acc += row[j] * sa[j];
        z[(size_t)n * C + c] = acc;
        gate[(size_t)n * C + c] = se_gate(kind, acc);
    }
}

static inline bool se_codes_ok(int act, int kind) {
    return (act == YDL_ACT_RELU || act == YDL_ACT_SILU) && (kind == YDL_SE_GATE_SIGMOID || kind == YDL_SE_GATE_HSIGMOID);
}

extern "C" int ydl_se_excite_fwd(const float* part, int S, const float* w1, const float* b1, const float* w2, const float* b2, int act,
                                 int gate_kind, float* pooled, float* h, float* z, float* gate, int N, int64_t HW, int C, int Cs,
                                 void* stream) {
    YDL_CHECK(part && w1 && b1 && w2 && b2 && pooled && h && z && gate, "null pointer");
    YDL_CHECK(ydl_se_supported(C, Cs), "C must be a multiple of 8 in 8..2048 and Cs in 1..512");
    YDL_CHECK(N > 0 && HW > 0 && HW < (1LL << 24) && S >= 1 && S <= SE_MAX_SPLITS, "N > 0, 0 < HW < 2^24, 1 <= S <= 64");
    YDL_CHECK(se_codes_ok(act, gate_kind), "act must be YDL_ACT_RELU or YDL_ACT_SILU, the gate YDL_SE_GATE_SIGMOID or _HSIGMOID");
    se_excite_fwd_kernel<<<N, 256, 0, (hipStream_t)stream>>>(part, S, (float)HW, w1, b1, w2, b2, act, gate_kind, pooled, h, z, gate, C, Cs);
    YDL_LAUNCH_CHECK();
    return 0;
}

// per sample: dz = dgate * scale'(z), dh = (W2^T dz) * act'(h), dpooled = W1^T dh; dz and dh are kept for the parameter sums
__global__ __launch_bounds__(256) void se_excite_bwd_kernel(const float* __restrict__ dgate, int S, const float* __restrict__ h,
                                                            const float* __restrict__ z, const float* __restrict__ w1,
                                                            const float* __restrict__ w2, int act, int kind, float* __restrict__ dpooled,
                                                            float* __restrict__ dz, float* __restrict__ dh, int C, int Cs) {
    __shared__ float sdz[SE_MAX_C];
    __shared__ float sdh[SE_MAX_CS];
    const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = threadIdx.x; c < C; c += 256) {
        float t = 0.f;
        for (int s = 0; s < S; ++s) t += dgate[((size_t)n * S + s) * C + c];
        t *= se_gate_grad(kind, z[(size_t)n * C + c]);
        sdz[c] = t;
        dz[(size_t)n * C + c] = t;
    }
    __syncthreads();
    for (int j = wave; j < Cs; j += 4) {
        float acc = 0.f;
        for (int c = lane; c < C; c += 64) acc += w2[(size_t)c * Cs + j] * sdz[c];
        acc = wave_sum(acc);
        if (lane == 0) {
            const float d = acc * se_act_grad(act, h[(size_t)n * Cs + j]);
            sdh[j] = d;
            dh[(size_t)n * Cs + j] = d;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float acc = 0.f;
        for (int j = 0; j < Cs; ++j) acc += w1[(size_t)j * C + c] * sdh[j];
        dpooled[(size_t)n * C + c] = acc;
    }
}

// dW1[j][c] += sum_n dh[n][j] p[n][c],  dW2[c][j] += sum_n dz[n][c] act(h[n][j]),  db1[j] += sum_n dh,  db2[c] += sum_n dz: one thread
// per element, the samples in order.  A NULL destination is skipped.
__global__ __launch_bounds__(256) void se_param_grad_kernel(const float* __restrict__ dz, const float* __restrict__ dh,
                                                            const float* __restrict__ pooled, const float* __restrict__ h, int act,
                                                            float* __restrict__ dw1, float* __restrict__ db1, float* __restrict__ dw2,
                                                            float* __restrict__ db2, int N, int C, int Cs) {
    const int nw = C * Cs, total = 2 * nw + Cs + C;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        float t = 0.f;
        if (i < nw) {
            if (dw1 == nullptr) continue;
            const int j = i / C, c = i - j * C;
            for (int n = 0; n < N; ++n) t += dh[(size_t)n * Cs + j] * pooled[(size_t)n * C + c];
            dw1[i] += t;
        } else if (i < 2 * nw) {
            if (dw2 == nullptr) continue;
            const int k = i - nw, c = k / Cs, j = k - c * Cs;
            for (int n = 0; n < N; ++n) t += dz[(size_t)n * C + c] * se_act(act, h[(size_t)n * Cs + j]);
            dw2[k] += t;
        } else if (i < 2 * nw + Cs) {
            if (db1 == nullptr) continue;
            const int j = i - 2 * nw;
            for (int n = 0; n < N; ++n) t += dh[(size_t)n * Cs + j];
            db1[j] += t;
        } else {
            if (db2 == nullptr) continue;
            const int c = i - 2 * nw - Cs;
            for (int n = 0; n < N; ++n) t += dz[(size_t)n * C + c];
            db2[c] += t;
        }
    }
}

extern "C" int64_t ydl_se_excite_bwd_ws_bytes(int N, int C, int Cs) {
    if (N <= 0 || !ydl_se_supported(C, Cs)) return 0;
    return (int64_t)N * (C + Cs) * (int64_t)sizeof(float);
}

extern "C" int ydl_se_excite_bwd(const float* dgate, int S, const float* pooled, const float* h, const float* z, const float* w1,
                                 const float* w2, int act, int gate_kind, float* dpooled, float* dw1, float* db1, float* dw2, float* db2,
                                 float* ws, int N, int C, int Cs, void* stream) {
    YDL_CHECK(dgate && pooled && h && z && w1 && w2 && dpooled && ws, "null pointer");
    YDL_CHECK(ydl_se_supported(C, Cs), "C must be a multiple of 8 in 8..2048 and Cs in 1..512");
    YDL_CHECK(N > 0 && S >= 1 && S <= SE_MAX_SPLITS, "N > 0, 1 <= S <= 64");
    YDL_CHECK(se_codes_ok(act, gate_kind), "act must be YDL_ACT_RELU or YDL_ACT_SILU, the gate YDL_SE_GATE_SIGMOID or _HSIGMOID");
    hipStream_t st = (hipStream_t)stream;
    float* dz = ws;
    float* dh = ws + (size_t)N * C;
    se_excite_bwd_kernel<<<N, 256, 0, st>>>(dgate, S, h, z, w1, w2, act, gate_kind, dpooled, dz, dh, C, Cs);
    if (dw1 || db1 || dw2 || db2) {
        const int total = 2 * C * Cs + Cs + C;
        se_param_grad_kernel<<<(total + 255) / 256, 256, 0, st>>>(dz, dh, pooled, h, act, dw1, db1, dw2, db2, N, C, Cs);
    }
    YDL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// dx (+)= dy * gate[n, c] + dpooled[n, c] / HW
// ------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void se_scale_bwd_kernel(const T* __restrict__ dy, int lddy, const float* __restrict__ gate,
                                                           const float* __restrict__ dpooled, T* dx, int lddx, int accumulate,
                                                           long long npix, long long hw, float hwf, int C) {
    constexpr int V = ET<T>::V;
    const Lay L = make_lay<V>(C);
    if (!L.live) return;
    // a CTA walks one contiguous run of pixels, so a lane changes sample (and reloads its gate and dpooled chunk) a few times at most
    const long long per = (npix + gridDim.x - 1) / gridDim.x;
    const long long run = (per + L.R - 1) / L.R * L.R;
    const long long first = (long long)blockIdx.x * run;
    const long long last = first + run < npix ? first + run : npix;
    long long ncur = -1;
    float g[V], dp[V];
    for (long long pix = first + L.pl; pix < last; pix += L.R) {
        const long long n = pix / hw;
        if (n != ncur) {
            ncur = n;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                g[e] = gate[(size_t)n * C + L.c + e];
                dp[e] = dpooled[(size_t)n * C + L.c + e] / hwf;
            }
        }
        float d[V];
        unpack16<T>(*(const uint4*)(dy + pix * lddy + L.c), d);
        T* dst = dx + pix * lddx + L.c;
        if (accumulate) {
            float old[V];
            unpack16<T>(*(const uint4*)dst, old);
#pragma unroll
            for (int e = 0; e < V; ++e) d[e] = (d[e] * g[e] + dp[e]) + old[e];
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) d[e] = d[e] * g[e] + dp[e];
        }
        *(uint4*)dst = pack16<T>(d);
    }
}

extern "C" int ydl_se_scale_bwd(int dtype, const void* dy, int lddy, const float* gate, const float* dpooled, void* dx, int lddx,
                                int accumulate, int N, int64_t HW, int C, void* stream) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "bad dtype");
    const int V = dtype == YDL_F32 ? 4 : 8;
    YDL_CHECK(dy && gate && dpooled && dx, "null pointer");
    YDL_CHECK(N > 0 && HW > 0 && HW < (1LL << 24) && C >= 8 && C <= SE_MAX_C && C % 8 == 0, "N > 0, 0 < HW < 2^24, C a multiple of 8 in 8..2048");
    YDL_CHECK(se_rows_ok(V, C, lddy) && se_rows_ok(V, C, lddx) && aligned16(dy) && aligned16(dx),
              "dy and dx must be 16-byte aligned with strides of whole chunks covering C");
    const long long npix = (long long)N * HW;
    dim3 grid = lay_grid(npix, C, V, 256 * 8);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == YDL_F32)
        se_scale_bwd_kernel<float><<<grid, 256, 0, st>>>((const float*)dy, lddy, gate, dpooled, (float*)dx, lddx, accumulate, npix,
                                                         (long long)HW, (float)HW, C);
    else
        se_scale_bwd_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)dy, lddy, gate, dpooled, (bf16_t*)dx, lddx, accumulate, npix,
                                                          (long long)HW, (float)HW, C);
    YDL_LAUNCH_CHECK();
    return 0;
}
