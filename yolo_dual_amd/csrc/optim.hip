// Weight re-layout (f32 KRSC master -> compute copies), wgrad un-padding, and the fused optimizer+EMA step over flat arenas
// (utils/torch_utils.py:318-346 smart_optimizer groups, :404-428 ModelEMA.update): SGD(nesterov), Adam, AdamW and RMSProp as four
// rules of one walk and one set of three kernels (host scalars, device hyper vector, run table).
#include "common.h"

// w[co][t][ci_p] = master[co][t][ci] (zero pad);  wt[ci][t][co_p] = master[co][t][ci]
template <typename T>
__global__ __launch_bounds__(256) void weight_prep_kernel(const float* __restrict__ master, T* __restrict__ w, T* __restrict__ wt,
                                                          int Cout, int kk, int Cin, int Cin_p, int Cout_p) {
    const long long n1 = (long long)Cout * kk * Cin_p;
    const long long n2 = (long long)Cin * kk * Cout_p;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n1 + n2; i += (long long)gridDim.x * blockDim.x) {
        if (i < n1) {
            if (w == nullptr) continue;
            int ci = (int)(i % Cin_p);
            long long r = i / Cin_p;           // co*kk + t
            float v = ci < Cin ? master[r * Cin + ci] : 0.f;
            ET<T>::st(w + i, v);
        } else {
            if (wt == nullptr) continue;
            long long j = i - n1;
            int co = (int)(j % Cout_p);
            long long r = j / Cout_p;          // ci*kk + t
            int t = (int)(r % kk);
            int ci = (int)(r / kk);
            float v = co < Cout ? master[((long long)co * kk + t) * Cin + ci] : 0.f;
            ET<T>::st(wt + j, v);
        }
    }
}

extern "C" int ydl_weight_prep(int dtype, const float* master, void* w, void* wt, int Cout, int kk, int Cin, void* stream) {
    YDL_CHECK(master && (w || wt) && Cout > 0 && kk > 0 && Cin > 0, "bad arguments");
    int Cin_p = round_up(Cin, 8), Cout_p = round_up(Cout, 8);
    long long total = (long long)Cout * kk * Cin_p + (long long)Cin * kk * Cout_p;
    int grid = (int)((total + 255) / 256);
    if (grid > 4096) grid = 4096;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == YDL_F32) weight_prep_kernel<float><<<grid, 256, 0, st>>>(master, (float*)w, (float*)wt, Cout, kk, Cin, Cin_p, Cout_p);
    else weight_prep_kernel<bf16_t><<<grid, 256, 0, st>>>(master, (bf16_t*)w, (bf16_t*)wt, Cout, kk, Cin, Cin_p, Cout_p);
    YDL_LAUNCH_CHECK();
    return 0;
}

// all layers of a model in ONE launch: blockIdx.y = layer, descriptors live in device memory
// desc[l] = {master*, w*, wt*, Cout, kk, Cin, 0, 0} as 8 x int64.
// Per tap the [Cout][Cin] matrix is walked in 32x32 tiles through LDS: the master rows are read coalesced once, `w` is
// written in the same order and `wt` transposed, both coalesced (the former element-wise version read the master with a
// k*k*Cin stride for `wt`: 549 MB fetched per step for 68 MB of weights in the PMC profile).
template <typename T>
__global__ __launch_bounds__(256) void weight_prep_batched_kernel(const long long* __restrict__ desc, int nlayers) {
    // tiles of ALL layers in one flat index space (one grid row per layer gave the 4.7 M-element layers 256 CTAs like the 8 K-element
    // ones: the launch took as long as its largest layer, 58 us for 68 MB in / 68 MB out).  Every CTA derives the per-layer tile
    // prefix itself: layer = thread, inclusive scan through LDS.
    __shared__ int s_end[256];
    __shared__ float tile[32][33];
    const int tid = threadIdx.x;
    {
        int nt = 0;
        if (tid < nlayers) {
            const long long* d = desc + (size_t)tid * 8;
            const int Cout = (int)d[3], kk = (int)d[4], Cin = (int)d[5];
            nt = ((Cout + 7) / 8 * 8 + 31) / 32 * (((Cin + 7) / 8 * 8 + 31) / 32) * kk;
        }
        s_end[tid] = nt;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int v = tid >= o ? s_end[tid - o] : 0;
            __syncthreads();
            s_end[tid] += v;
            __syncthreads();
        }
    }
    const int total = s_end[nlayers - 1];
    const int tx = tid & 31, ty = tid >> 5;
    int l = 0;
    for (int gt = blockIdx.x; gt < total; gt += gridDim.x) {
        while (gt >= s_end[l]) ++l;                       // gt only grows
        const long long* d = desc + (size_t)l * 8;
        const float* master = (const float*)d[0];
        T* w = (T*)d[1];
        T* wt = (T*)d[2];
        const int Cout = (int)d[3], kk = (int)d[4], Cin = (int)d[5];
        const int Cin_p = (Cin + 7) / 8 * 8, Cout_p = (Cout + 7) / 8 * 8;
        const int tci = (Cin_p + 31) / 32;
        const int tl = gt - (l ? s_end[l - 1] : 0);
        const int cit = tl % tci;
        const int r2 = tl / tci;
        const int t = r2 % kk;
        const int cot = r2 / kk;
        const int co0 = cot * 32, ci0 = cit * 32;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int co = co0 + ty + 8 * i, ci = ci0 + tx;
            float v = (co < Cout && ci < Cin) ? master[((size_t)co * kk + t) * Cin + ci] : 0.f;
            tile[ty + 8 * i][tx] = v;
            if (co < Cout && ci < Cin_p) ET<T>::st(w + ((size_t)co * kk + t) * Cin_p + ci, v);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ci = ci0 + ty + 8 * i, co = co0 + tx;
            if (ci < Cin && co < Cout_p) ET<T>::st(wt + ((size_t)ci * kk + t) * Cout_p + co, tile[tx][ty + 8 * i]);
        }
        __syncthreads();
    }
}

extern "C" int ydl_weight_prep_batched(int dtype, const int64_t* desc_dev, int nlayers, void* stream) {
    YDL_CHECK(desc_dev && nlayers > 0, "bad arguments");
    hipStream_t st = (hipStream_t)stream;
    for (int l0 = 0; l0 < nlayers; l0 += 256) {            // 256 layers per launch (one scan lane each)
        const int nl = nlayers - l0 < 256 ? nlayers - l0 : 256;
        const long long* d = (const long long*)desc_dev + (size_t)l0 * 8;
        if (dtype == YDL_F32) weight_prep_batched_kernel<float><<<2048, 256, 0, st>>>(d, nl);
        else weight_prep_batched_kernel<bf16_t><<<2048, 256, 0, st>>>(d, nl);
    }
    YDL_LAUNCH_CHECK();
    return 0;
}

__global__ void wgrad_unpad_kernel(const float* __restrict__ dw, float* __restrict__ grad, long long rows, int Cin, int Cin_p, int accumulate) {
    const long long total = rows * Cin;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        long long r = i / Cin;
        int c = (int)(i - r * Cin);
        float v = dw[r * Cin_p + c];
        grad[i] = accumulate ? grad[i] + v : v;
    }
}
extern "C" int ydl_wgrad_unpad(const float* dw, float* grad, int Cout, int kk, int Cin, int accumulate, void* stream) {
    YDL_CHECK(dw && grad, "null pointer");
    long long rows = (long long)Cout * kk;
    long long total = rows * Cin;
    int grid = (int)((total + 255) / 256);
    if (grid > 4096) grid = 4096;
    wgrad_unpad_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(dw, grad, rows, Cin, round_up(Cin, 8), accumulate);
    YDL_LAUNCH_CHECK();
    return 0;
}

// space-to-depth form of a stem weight (see ydl_nchw_to_s2d): master [Cout][k][k][C] (KRSC) ->
//   w2[co][(r2*k2 + c2)][(dy*s+dx)*C + c] = master[co][s*r2+dy][s*c2+dx][c],   k2 = k/s, row padded to Cs_p = round_up(s*s*C, 8)
template <typename T>
__global__ void weight_prep_s2d_kernel(const float* __restrict__ master, T* __restrict__ w2, int Cout, int k, int s, int C) {
    const int k2 = k / s, Cs = C * s * s, Cs_p = (Cs + 7) / 8 * 8;
    const long long total = (long long)Cout * k2 * k2 * Cs_p;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int ch = (int)(i % Cs_p);
        long long r = i / Cs_p;
        const int c2 = (int)(r % k2); r /= k2;
        const int r2 = (int)(r % k2);
        const int co = (int)(r / k2);
        float v = 0.f;
        if (ch < Cs) {
            const int c = ch % C, dd = ch / C, dx = dd % s, dy = dd / s;
            v = master[(((size_t)co * k + (s * r2 + dy)) * k + (s * c2 + dx)) * C + c];
        }
        ET<T>::st(w2 + i, v);
    }
}
extern "C" int ydl_weight_prep_s2d(int dtype, const float* master, void* w2, int Cout, int k, int s, int C, void* stream) {
    YDL_CHECK(master && w2 && Cout > 0 && C > 0 && s >= 1 && k % s == 0, "k must be a multiple of s");
    const int k2 = k / s;
    long long total = (long long)Cout * k2 * k2 * round_up(C * s * s, 8);
    int grid = (int)((total + 255) / 256);
    if (grid > 1024) grid = 1024;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == YDL_F32) weight_prep_s2d_kernel<float><<<grid, 256, 0, st>>>(master, (float*)w2, Cout, k, s, C);
    else weight_prep_s2d_kernel<bf16_t><<<grid, 256, 0, st>>>(master, (bf16_t*)w2, Cout, k, s, C);
    YDL_LAUNCH_CHECK();
    return 0;
}

// the inverse index map for the weight gradient: grad[co][s*r2+dy][s*c2+dx][c] (+)= dw2[co][r2*k2+c2][(dy*s+dx)*C + c]
__global__ void wgrad_unpack_s2d_kernel(const float* __restrict__ dw2, float* __restrict__ grad, int Cout, int k, int s, int C,
                                        int accumulate) {
    const int k2 = k / s, Cs = C * s * s, Cs_p = (Cs + 7) / 8 * 8;
    const long long total = (long long)Cout * k * k * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long long r = i / C;
        const int kw = (int)(r % k); r /= k;
        const int kh = (int)(r % k);
        const int co = (int)(r / k);
        const int r2 = kh / s, dy = kh % s, c2 = kw / s, dx = kw % s;
        const float v = dw2[(((size_t)co * k2 + r2) * k2 + c2) * Cs_p + (dy * s + dx) * C + c];
        grad[i] = accumulate ? grad[i] + v : v;
    }
}
extern "C" int ydl_wgrad_unpack_s2d(const float* dw2, float* grad, int Cout, int k, int s, int C, int accumulate, void* stream) {
    YDL_CHECK(dw2 && grad && Cout > 0 && C > 0 && s >= 1 && k % s == 0, "k must be a multiple of s");
    long long total = (long long)Cout * k * k * C;
    int grid = (int)((total + 255) / 256);
    if (grid > 1024) grid = 1024;
    wgrad_unpack_s2d_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(dw2, grad, Cout, k, s, C, accumulate);
    YDL_LAUNCH_CHECK();
    return 0;
}

// ---- SGD(nesterov) / Adam / AdamW / RMSProp + EMA over the flat arenas: one family, four rules ------------------------------------
// One streaming pass over [params | buffers]: the rule on the parameters (two lr / decay groups), the EMA on everything.  Seven
// words per parameter for SGD (p rw, g r, momentum rw, ema rw), nine for the others (state1 rw, state2 rw).  The three entry forms
// (host scalars, device hyper vector, run table) of every rule share ONE element function and ONE walk, so that they agree bit for
// bit.
//
// SGD, torch.optim.SGD(nesterov=True) (utils/torch_utils.py:318-346):
//   g = grad*grad_scale + wd*p ; buf = first ? g : mom*buf + g ; p -= lr*(g + mom*buf) ; ema = d*ema + (1-d)*p
// Its element function is compiled like the rest of the library, with -ffp-contract=on: the SOURCE expressions decide which
// products fuse (five fused multiply-adds and two multiplies per element), in every inlining context alike.
__device__ __forceinline__ void sgd_ema_elem(float& p, float g, float& b, float& e, bool is_param, bool dec, bool first, bool use_ema,
                                             float lr, float mom, float wd, float gscale, float d) {
    if (is_param) {
        g = g * gscale;
        if (dec && wd != 0.f) g = g + wd * p;
        b = first ? g : mom * b + g;
        const float upd = g + mom * b;
        p = p - lr * upd;
    }
    if (use_ema) {
        e = e * d;
        e = e + (1.f - d) * p;
    }
}

// Adam / AdamW / RMSProp, torch.optim.{Adam,AdamW,RMSprop}, single-tensor path: the element function keeps torch's operation order
// and is compiled WITHOUT FMA contraction (torch's CPU kernels do not contract either, and the trajectory tests measure against them).
constexpr int OPT_SGD = 0;     // internal: not a YDL_OPT_* value, ydl_optim_ema_step* refuse it; SGD enters through ydl_sgd_ema_step*
struct OptHyper {
    float step;        // Adam/AdamW: lr / (1 - beta1^t);  RMSProp, SGD: lr
    float bc2s;        // Adam/AdamW: sqrt(1 - beta2^t)
    float dmul;        // AdamW: 1 - lr*wd
    float wd;          // Adam/RMSProp/SGD: coupled decay
    float b1, b2, omb1, omb2, eps, gscale, d;      // b1: beta1 | momentum
    float step_nd;     // SGD: lr of the elements past n_decay (the host-scalar form takes two; otherwise == step)
};

template <int RULE>
__device__ __forceinline__ void optim_ema_elem(float& p, float g, float& s1, float& s2, float& e, bool is_param, bool dec, bool use_ema,
                                               const OptHyper& h) {
#pragma clang fp contract(off)
    if (is_param) {
        g = g * h.gscale;
        if (RULE == YDL_OPT_ADAMW) {
            if (dec) p = p * h.dmul;
        } else if (dec && h.wd != 0.f) {
            g = g + h.wd * p;
        }
        if (RULE != YDL_OPT_RMSPROP) {
            const float diff = g - s1;                                   // exp_avg.lerp_(grad, 1 - beta1)
            s1 = h.omb1 < 0.5f ? s1 + h.omb1 * diff : g - diff * (1.f - h.omb1);
            s2 = s2 * h.b2 + (h.omb2 * g) * g;                           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
            const float denom = sqrtf(s2) / h.bc2s + h.eps;
            p = p + (-h.step * s1) / denom;                              // param.addcdiv_(exp_avg, denom, value=-step_size)
        } else {
            s2 = s2 * h.b2 + (h.omb2 * g) * g;                           // square_avg.mul_(alpha).addcmul_(grad, grad, value=1 - alpha)
            const float avg = sqrtf(s2) + h.eps;
            if (h.b1 > 0.f) {
                s1 = s1 * h.b1 + g / avg;                                // buf.mul_(momentum).addcdiv_(grad, avg)
                p = p + (-h.step) * s1;                                  // param.add_(buf, alpha=-lr)
            } else {
                p = p + (-h.step * g) / avg;                             // param.addcdiv_(grad, avg, value=-lr)
            }
        }
    }
    if (use_ema) {
        e = e * h.d;
        e = e + (1.f - h.d) * p;
    }
}

// the element function of a rule (the contract(off) pragma above covers optim_ema_elem's own body only)
template <int RULE>
__device__ __forceinline__ void optim_ema_elem_of(float& p, float g, float& s1, float& s2, float& e, bool is_param, bool dec, bool first,
                                                  bool use_ema, const OptHyper& h) {
    if (RULE == OPT_SGD) sgd_ema_elem(p, g, s1, e, is_param, dec, first, use_ema, dec ? h.step : h.step_nd, h.b1, h.wd, h.gscale, h.d);
    else optim_ema_elem<RULE>(p, g, s1, s2, e, is_param, dec, use_ema, h);
}

// One run [off, off + n_total) of the arenas, walked in float4 groups aligned to the ARENA (16-byte accesses whatever the run's
// offset); the groups that straddle the run's ends, runs whose decay / parameter boundary is not the whole run, and arenas that are
// not co-aligned (`vec` false) take the element form.  Same arithmetic per element either way.  SGD has no second state array
// (`st2` is never touched) and does not read its momentum on the first step of a run (`first`; false for the other rules).
// The arrays do not alias; that is declared on the kernels' parameters and not repeated here: with __restrict__ on these
// parameters too the SLP vectorizer pairs SGD's arithmetic into v_pk_* instructions (34 VGPRs instead of 28, same results).
template <int RULE>
__device__ __forceinline__ void optim_ema_walk(float* params, const float* grads, float* st1, float* st2, float* ema, long long off,
                                               long long n_decay, long long n_params, long long n_total, const OptHyper& h, bool first,
                                               bool ue, bool vec) {
    constexpr bool us2 = RULE != OPT_SGD;
    const bool ws1 = RULE != YDL_OPT_RMSPROP || h.b1 > 0.f;              // RMSProp without momentum keeps no buffer
    const bool us1 = RULE == OPT_SGD ? !first : ws1;
    const long long a0 = off & ~3ll, end = off + n_total;
    const bool uniform = vec && (n_params == n_total || n_params == 0) && (n_decay == n_params || n_decay == 0);
    for (long long q = a0 + 4 * ((long long)blockIdx.x * blockDim.x + threadIdx.x); q < end; q += 4ll * gridDim.x * blockDim.x) {
        if (uniform && q >= off && q + 4 <= end) {
            const bool isp = n_params != 0, dec = n_decay != 0;
            float4 p4 = *(const float4*)(params + q), g4 = make_float4(0.f, 0.f, 0.f, 0.f), a4 = g4, b4 = g4, e4 = g4;
            if (isp) {
                g4 = *(const float4*)(grads + q);
                if (us1) a4 = *(const float4*)(st1 + q);
                if (us2) b4 = *(const float4*)(st2 + q);
            }
            if (ue) e4 = *(const float4*)(ema + q);
            optim_ema_elem_of<RULE>(p4.x, g4.x, a4.x, b4.x, e4.x, isp, dec, first, ue, h);
            optim_ema_elem_of<RULE>(p4.y, g4.y, a4.y, b4.y, e4.y, isp, dec, first, ue, h);
            optim_ema_elem_of<RULE>(p4.z, g4.z, a4.z, b4.z, e4.z, isp, dec, first, ue, h);
            optim_ema_elem_of<RULE>(p4.w, g4.w, a4.w, b4.w, e4.w, isp, dec, first, ue, h);
            if (isp) {
                *(float4*)(params + q) = p4;
                if (ws1) *(float4*)(st1 + q) = a4;
                if (us2) *(float4*)(st2 + q) = b4;
            }
            if (ue) *(float4*)(ema + q) = e4;
        } else {
            for (int k = 0; k < 4; ++k) {
                const long long i = q + k - off;
                if (i < 0 || i >= n_total) continue;
                const bool isp = i < n_params;
                float p = params[off + i], g = 0.f, a = 0.f, b = 0.f, e = 0.f;
                if (isp) {
                    g = grads[off + i];
                    if (us1) a = st1[off + i];
                    if (us2) b = st2[off + i];
                }
                if (ue) e = ema[off + i];
                optim_ema_elem_of<RULE>(p, g, a, b, e, isp, i < n_decay, first, ue, h);
                if (isp) {
                    params[off + i] = p;
                    if (ws1) st1[off + i] = a;
                    if (us2) st2[off + i] = b;
                }
                if (ue) ema[off + i] = e;
            }
        }
    }
}

__device__ __forceinline__ OptHyper optim_hyper_load(int rule, const float* __restrict__ hyper, int lr_idx, int cls, bool use_wd) {
    OptHyper h{};
    h.wd = use_wd ? hyper[4] : 0.f;
    h.b1 = hyper[3]; h.gscale = hyper[5]; h.d = hyper[6];
    if (rule == OPT_SGD) {                                                // its vector ends at [6]
        h.step = h.step_nd = hyper[lr_idx];
        return h;
    }
    const bool rms = rule == YDL_OPT_RMSPROP;
    h.step = rms ? hyper[lr_idx] : hyper[12 + 4 * cls + lr_idx];
    h.bc2s = rms ? 1.f : hyper[12 + 4 * cls + 3];
    h.dmul = hyper[11];
    h.b2 = hyper[7]; h.eps = hyper[8]; h.omb1 = hyper[9]; h.omb2 = hyper[10];
    return h;
}

template <int RULE>
__global__ __launch_bounds__(256) void optim_ema_kernel(float* __restrict__ params, const float* __restrict__ grads,
                                                        float* __restrict__ st1, float* __restrict__ st2, float* __restrict__ ema,
                                                        long long off, long long n_decay, long long n_params, long long n_total,
                                                        OptHyper h, int first, int vec) {
    optim_ema_walk<RULE>(params, grads, st1, st2, ema, off, n_decay, n_params, n_total, h, first != 0, h.d >= 0.f && ema != nullptr, vec != 0);
}

template <int RULE>
__global__ __launch_bounds__(256) void optim_ema_dev_kernel(float* __restrict__ params, const float* __restrict__ grads,
                                                            float* __restrict__ st1, float* __restrict__ st2, float* __restrict__ ema,
                                                            long long off, long long n_decay, long long n_params, long long n_total,
                                                            const float* __restrict__ hyper, int lr_idx, int cls, int use_wd, int first,
                                                            int use_ema, int vec) {
    const OptHyper h = optim_hyper_load(RULE, hyper, lr_idx, cls, use_wd != 0);
    optim_ema_walk<RULE>(params, grads, st1, st2, ema, off, n_decay, n_params, n_total, h, first != 0, use_ema && ema != nullptr, vec != 0);
}

// grid row y handles run y of the device table: {offset, n_decay, n_params, n_total, lr_index, flags (bit 0 weight decay, SGD: bit 1
// first step)} and, but for SGD whose rows end there, {bc_class, 0}
template <int RULE>
__global__ __launch_bounds__(256) void optim_ema_multi_kernel(float* __restrict__ params, const float* __restrict__ grads,
                                                              float* __restrict__ st1, float* __restrict__ st2, float* __restrict__ ema,
                                                              const long long* __restrict__ runs, const float* __restrict__ hyper,
                                                              int use_ema) {
    const long long* r = runs + (size_t)blockIdx.y * (RULE == OPT_SGD ? 6 : 8);
    const int flags = (int)r[5];
    const OptHyper h = optim_hyper_load(RULE, hyper, (int)r[4], RULE == OPT_SGD ? 0 : (int)r[6], (flags & 1) != 0);
    optim_ema_walk<RULE>(params, grads, st1, st2, ema, r[0], r[1], r[2], r[3], h, RULE == OPT_SGD && (flags & 2) != 0,
                         use_ema && ema != nullptr, true);
}

static inline unsigned optim_grid_x(long long n) {
    long long gx = (n + 4 + 1023) / 1024;                 // four elements per thread (+ the alignment slack of the first group)
    if (gx > 2048) gx = 2048;
    if (gx < 1) gx = 1;
    return (unsigned)gx;
}

// per-run forms: the pointers are arena + offset and need not be 16-byte aligned.  When every array the run touches sits at the
// same distance `lead` (0..3 elements) behind a 16-byte boundary, all are rebased onto that boundary and the run starts at `lead`
// (the vector walk); otherwise the element walk.  SGD has no `s2`.
static inline int optim_lead(const void* p) { return (int)((((uintptr_t)p) >> 2) & 3u); }
struct OptRebase { float *p, *s1, *s2, *e; const float* g; long long off; int vec; };
static OptRebase optim_rebase(float* params, const float* grads, float* s1, float* s2, float* ema, bool has_params, bool has_ema) {
    const int lead = optim_lead(params);
    bool co = (((uintptr_t)params) & 3u) == 0;
    if (has_params) co = co && optim_lead(grads) == lead && optim_lead(s1) == lead && (s2 == nullptr || optim_lead(s2) == lead);
    if (has_ema) co = co && optim_lead(ema) == lead;
    OptRebase r{params, s1, s2, ema, grads, 0, 0};
    if (co) {
        r.p = params - lead; r.g = grads - lead; r.s1 = s1 - lead; r.s2 = s2 ? s2 - lead : nullptr; r.e = ema ? ema - lead : nullptr;
        r.off = lead; r.vec = 1;
    }
    return r;
}

#define YDL_OPT_RULE_OK(rule) ((rule) == YDL_OPT_ADAM || (rule) == YDL_OPT_ADAMW || (rule) == YDL_OPT_RMSPROP)
#define YDL_OPT_DISPATCH(rule, KERNEL, grid, st, ...)                                              \
    do {                                                                                           \
        if ((rule) == OPT_SGD) KERNEL<OPT_SGD><<<grid, 256, 0, st>>>(__VA_ARGS__);                 \
        else if ((rule) == YDL_OPT_ADAM) KERNEL<YDL_OPT_ADAM><<<grid, 256, 0, st>>>(__VA_ARGS__);  \
        else if ((rule) == YDL_OPT_ADAMW) KERNEL<YDL_OPT_ADAMW><<<grid, 256, 0, st>>>(__VA_ARGS__); \
        else KERNEL<YDL_OPT_RMSPROP><<<grid, 256, 0, st>>>(__VA_ARGS__);                           \
    } while (0)

// The three entry forms of every rule: validation and launch.  The public entry points below add only what is theirs: the
// family's refuse a rule that is not a YDL_OPT_* value, SGD's pass OPT_SGD and no second state array.
static int optim_step(int rule, float* params, const float* grads, float* state1, float* state2, float* ema, int64_t n_decay,
                      int64_t n_params, int64_t n_total, const OptHyper& h, int first_step, void* stream) {
    YDL_CHECK(params && grads && state1 && (state2 || rule == OPT_SGD), "null pointer");
    YDL_CHECK(0 <= n_decay && n_decay <= n_params && n_params <= n_total, "bad arena partition");
    const OptRebase r = optim_rebase(params, grads, state1, state2, ema, n_params > 0, ema != nullptr && h.d >= 0.f);
    const dim3 grid(optim_grid_x(n_total));
    hipStream_t st = (hipStream_t)stream;
    YDL_OPT_DISPATCH(rule, optim_ema_kernel, grid, st, r.p, r.g, r.s1, r.s2, r.e, r.off, (long long)n_decay, (long long)n_params,
                     (long long)n_total, h, first_step, r.vec);
    YDL_LAUNCH_CHECK();
    return 0;
}

static int optim_step_dev(int rule, float* params, const float* grads, float* state1, float* state2, float* ema, int64_t n_decay,
                          int64_t n_params, int64_t n_total, const float* hyper_dev, int lr_index, int bc_class, int use_weight_decay,
                          int first_step, int use_ema, void* stream) {
    YDL_CHECK(params && grads && state1 && (state2 || rule == OPT_SGD) && hyper_dev, "null pointer");
    YDL_CHECK(0 <= n_decay && n_decay <= n_params && n_params <= n_total, "bad arena partition");
    YDL_CHECK(lr_index >= 0 && lr_index <= 2 && bc_class >= 0 && bc_class < YDL_OPT_MAX_CLASSES, "bad lr index or bias-correction class");
    const OptRebase r = optim_rebase(params, grads, state1, state2, ema, n_params > 0, ema != nullptr && use_ema);
    const dim3 grid(optim_grid_x(n_total));
    hipStream_t st = (hipStream_t)stream;
    YDL_OPT_DISPATCH(rule, optim_ema_dev_kernel, grid, st, r.p, r.g, r.s1, r.s2, r.e, r.off, (long long)n_decay, (long long)n_params,
                     (long long)n_total, hyper_dev, lr_index, bc_class, use_weight_decay, first_step, use_ema, r.vec);
    YDL_LAUNCH_CHECK();
    return 0;
}

static int optim_step_multi(int rule, float* params, const float* grads, float* state1, float* state2, float* ema,
                            const int64_t* runs_dev, int nruns, int64_t max_run, const float* hyper_dev, int use_ema, void* stream) {
    YDL_CHECK(params && grads && state1 && (state2 || rule == OPT_SGD) && runs_dev && hyper_dev, "null pointer");
    YDL_CHECK(nruns > 0 && nruns <= 65535 && max_run >= 0, "bad run count");
    YDL_CHECK(aligned16(params) && aligned16(grads) && aligned16(state1) && aligned16(state2) && (ema == nullptr || aligned16(ema)),
              "arenas must be 16-byte aligned");
    const dim3 grid(optim_grid_x(max_run), (unsigned)nruns);
    hipStream_t st = (hipStream_t)stream;
    YDL_OPT_DISPATCH(rule, optim_ema_multi_kernel, grid, st, params, grads, state1, state2, ema, (const long long*)runs_dev, hyper_dev,
                     use_ema);
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int ydl_sgd_ema_step(float* params, const float* grads, float* momentum, float* ema,
                                int64_t n_decay, int64_t n_params, int64_t n_total,
                                float lr_decay_group, float lr_nodecay_group, float mom, float weight_decay, float grad_scale,
                                int first_step, float ema_decay, void* stream) {
    OptHyper h{};
    h.step = lr_decay_group; h.step_nd = lr_nodecay_group; h.b1 = mom; h.wd = weight_decay; h.gscale = grad_scale; h.d = ema_decay;
    return optim_step(OPT_SGD, params, grads, momentum, nullptr, ema, n_decay, n_params, n_total, h, first_step, stream);
}

extern "C" int ydl_sgd_ema_step_dev(float* params, const float* grads, float* momentum, float* ema,
                                    int64_t n_decay, int64_t n_params, int64_t n_total, const float* hyper_dev,
                                    int lr_index, int use_weight_decay, int first_step, int use_ema, void* stream) {
    return optim_step_dev(OPT_SGD, params, grads, momentum, nullptr, ema, n_decay, n_params, n_total, hyper_dev, lr_index, 0,
                          use_weight_decay, first_step, use_ema, stream);
}

extern "C" int ydl_sgd_ema_step_multi(float* params, const float* grads, float* momentum, float* ema, const int64_t* runs_dev,
                                      int nruns, int64_t max_run, const float* hyper_dev, int use_ema, void* stream) {
    return optim_step_multi(OPT_SGD, params, grads, momentum, nullptr, ema, runs_dev, nruns, max_run, hyper_dev, use_ema, stream);
}

extern "C" int ydl_optim_ema_step(int rule, float* params, const float* grads, float* state1, float* state2, float* ema,
                                  int64_t n_decay, int64_t n_params, int64_t n_total,
                                  float step_size, float bc2_sqrt, float decay_mul, float weight_decay,
                                  float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps,
                                  float grad_scale, float ema_decay, void* stream) {
    YDL_CHECK(YDL_OPT_RULE_OK(rule), "unknown optimizer rule");
    const OptHyper h{step_size, bc2_sqrt, decay_mul, weight_decay, beta1, beta2, one_minus_beta1, one_minus_beta2, eps, grad_scale, ema_decay};
    return optim_step(rule, params, grads, state1, state2, ema, n_decay, n_params, n_total, h, 0, stream);
}

extern "C" int ydl_optim_ema_step_dev(int rule, float* params, const float* grads, float* state1, float* state2, float* ema,
                                      int64_t n_decay, int64_t n_params, int64_t n_total, const float* hyper_dev,
                                      int lr_index, int bc_class, int use_weight_decay, int use_ema, void* stream) {
    YDL_CHECK(YDL_OPT_RULE_OK(rule), "unknown optimizer rule");
    return optim_step_dev(rule, params, grads, state1, state2, ema, n_decay, n_params, n_total, hyper_dev, lr_index, bc_class,
                          use_weight_decay, 0, use_ema, stream);
}

extern "C" int ydl_optim_ema_step_multi(int rule, float* params, const float* grads, float* state1, float* state2, float* ema,
                                        const int64_t* runs_dev, int nruns, int64_t max_run, const float* hyper_dev, int use_ema,
                                        void* stream) {
    YDL_CHECK(YDL_OPT_RULE_OK(rule), "unknown optimizer rule");
    return optim_step_multi(rule, params, grads, state1, state2, ema, runs_dev, nruns, max_run, hyper_dev, use_ema, stream);
}
