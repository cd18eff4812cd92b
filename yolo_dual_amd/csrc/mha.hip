// Dense multi-head self-attention core of TransformerLayer (models/common.py:79-95: nn.MultiheadAttention without mask or dropout),
// NHWC, for gfx950, on MFMA.  The tokens of sample n are its S consecutive pixel rows; head h is the channel block [h*d, (h+1)*d) of a
// row.  Per (sample, head):   s_ij = scale * q_i . k_j,   P = softmax_j(s),   out_i = sum_j P_ij v_j,   lse_i = max_j s_ij + log sum_j.
//
// One byte geometry for both element types, as in igemm.hip: an MFMA step consumes 64 bytes of the summed dimension per operand row
// (v_mfma_f32_16x16x32_bf16 on 8 bf16 per lane, or four v_mfma_f32_16x16x4_f32 on the 4 floats of the same 16-byte read), every operand
// is a [row][summed dimension] image whose rows carry one 16-byte pad, and a streamed tile is TN = 128 / sizeof(T) rows (64 bf16, 32 f32)
// so that a row of P is 128 bytes in either type.  d is zero-padded in LDS / registers to DP in {32, 64, 128}.
//
// A workgroup is 4 waves and owns 64 rows ("own" rows: queries in the forward and the dQ kernel, keys in the dK/dV kernel); a wave owns
// 16 of them and keeps their operand fragments in registers for the whole sweep.  Every product puts the OWN row on the MFMA column
// (lane & 15) and the streamed row or the channel on the MFMA row, so that
//   * the score accumulators of a lane are 4 consecutive streamed rows of ONE own row: row maxima and sums are in-lane plus two
//     cross-lane steps, the running max / sum / lse / delta are per-lane scalars, and P goes to LDS as one 8- or 16-byte store;
//   * the output accumulators of a lane are 4 consecutive channels of one own row: 8- or 16-byte stores into NHWC rows.
//     mha_fwd_kernel   : S^T = K Q^T -> online softmax -> P (wave-private LDS, rounded to T) -> O^T += V^T P^T
//     mha_delta_kernel : delta_i = sum_c dout_ic out_ic
//     mha_bwd_q_kernel : per query tile, all keys:   P = exp(s - lse), dP^T = V dO^T, dS = P (dP - delta), dQ^T += K^T dS^T
//     mha_bwd_kv_kernel: per key tile, all queries:  the same P and dS with the key on the lane, dV^T += dO^T P, dK^T += Q^T dS
// The backward is in gather form: no atomics and no sums across workgroups, so two runs are bitwise equal.  It computes S and dP twice.
#include "common.h"

#define MHA_OWN 64            // own rows per workgroup (4 waves x 16)
#define MHA_TROW 144          // bytes per row of a [*][streamed row] image: 128 data + 16 pad

struct MhaArgs {
    const void *q, *k, *v, *o, *dout;
    void *out, *dq, *dk, *dv;
    float *lse, *delta;
    int ldq, ldk, ldv, ldo, lddo, ldd;
    int N, S, heads, d, acc, vec, tiles;
    float scale;
};

template <typename T> struct MhaMma;
template <> struct MhaMma<bf16_t> {
    __device__ static __forceinline__ void run(const uint4& a, const uint4& b, f32x4& acc) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    }
};
template <> struct MhaMma<float> {
    __device__ static __forceinline__ void run(const uint4& a, const uint4& b, f32x4& acc) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
    }
};

// 16 bytes of a row; vec: every row of every tensor of the call starts 16-byte aligned
template <typename T> __device__ __forceinline__ uint4 mha_ld16(const T* p, int vec) {
    if (vec) return *(const uint4*)p;
    uint4 u;
    if constexpr (sizeof(T) == 4) {
        u.x = __float_as_uint(p[0]); u.y = __float_as_uint(p[1]); u.z = __float_as_uint(p[2]); u.w = __float_as_uint(p[3]);
    } else {
        u.x = (uint32_t)p[0] | ((uint32_t)p[1] << 16); u.y = (uint32_t)p[2] | ((uint32_t)p[3] << 16);
        u.z = (uint32_t)p[4] | ((uint32_t)p[5] << 16); u.w = (uint32_t)p[6] | ((uint32_t)p[7] << 16);
    }
    return u;
}

// 4 consecutive floats of one row -> T, optionally added to what is there
template <typename T> __device__ __forceinline__ void mha_st4(T* p, const float* f, int vec, int accumulate) {
    float o[4] = {f[0], f[1], f[2], f[3]};
    if (accumulate) {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] += ET<T>::ld(p + e);
    }
    if (vec) {
        if constexpr (sizeof(T) == 4) *(float4*)p = make_float4(o[0], o[1], o[2], o[3]);
        else *(uint2*)p = make_uint2((uint32_t)f2bf(o[0]) | ((uint32_t)f2bf(o[1]) << 16), (uint32_t)f2bf(o[2]) | ((uint32_t)f2bf(o[3]) << 16));
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) ET<T>::st(p + e, o[e]);
    }
}
// the same into an LDS row (P and dS as MFMA operands: the one place they are rounded to T)
template <typename T> __device__ __forceinline__ void mha_lds4(char* p, const f32x4& f) {
    if constexpr (sizeof(T) == 4) *(float4*)p = make_float4(f[0], f[1], f[2], f[3]);
    else *(uint2*)p = make_uint2((uint32_t)f2bf(f[0]) | ((uint32_t)f2bf(f[1]) << 16), (uint32_t)f2bf(f[2]) | ((uint32_t)f2bf(f[3]) << 16));
}

template <typename T, int DP> struct MhaGeo {
    static constexpr int ES = (int)sizeof(T);
    static constexpr int EPC = 16 / ES;             // elements per 16-byte chunk
    static constexpr int TN = 128 / ES;             // streamed rows per tile
    static constexpr int NB = TN / 16;              // 16-row MFMA blocks of a streamed tile
    static constexpr int KS = DP * ES / 64;         // MFMA steps over the head dimension
    static constexpr int CB = DP / 16;              // 16-channel output blocks
    static constexpr int CPR = DP * ES / 16;        // chunks per natural row
    static constexpr int NROW = DP * ES + 16;       // bytes per natural row ([streamed row][channel])
    static constexpr int NAT = TN * NROW;           // bytes of a natural tile
    static constexpr int TRN = DP * MHA_TROW;       // bytes of a transposed tile ([channel][streamed row])
    static constexpr int PB = MHA_OWN * MHA_TROW;   // bytes of the P / dS image ([own row][streamed row])
};

// Rows [r0, r0 + TN) of one head of one sample -> LDS: `nat` as [row][channel] and / or `trn` as [channel][row]; rows >= S and channels
// >= d are zero.  src points at row 0 of the sample, at the head's first channel.
template <typename T, int DP>
__device__ __forceinline__ void mha_stage(char* nat, char* trn, const T* src, int ld, int r0, int S, int d, int vec) {
    using G = MhaGeo<T, DP>;
    for (int item = threadIdx.x; item < G::TN * G::CPR; item += blockDim.x) {
        const int row = item / G::CPR, ch = item % G::CPR;
        uint4 u = make_uint4(0, 0, 0, 0);
        if (r0 + row < S && ch * G::EPC < d) u = mha_ld16<T>(src + (size_t)(r0 + row) * ld + ch * G::EPC, vec);
        if (nat) *(uint4*)(nat + row * G::NROW + ch * 16) = u;
        if (trn) {
            const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int e = 0; e < G::EPC; ++e) {
                char* dst = trn + (ch * G::EPC + e) * MHA_TROW + row * G::ES;
                if constexpr (sizeof(T) == 4) *(uint32_t*)dst = w[e];
                else *(unsigned short*)dst = (unsigned short)(w[e >> 1] >> ((e & 1) * 16));
            }
        }
    }
}

// operand fragments of own row `row` (the MFMA column lane & 15): zero when the row or the channel chunk does not exist
template <typename T, int DP>
__device__ __forceinline__ void mha_frag(uint4* f, const T* src, int ld, int row, int S, int d, int vec) {
    using G = MhaGeo<T, DP>;
    const int g = threadIdx.x >> 4 & 3;
#pragma unroll
    for (int s = 0; s < G::KS; ++s) {
        const int c = (s * 4 + g) * G::EPC;
        f[s] = make_uint4(0, 0, 0, 0);
        if (row < S && c < d) f[s] = mha_ld16<T>(src + (size_t)row * ld + c, vec);
    }
}

// acc[nb] (+)= sum_c nat[nb*16 + m][c] * frag[own row][c] over the padded head dimension
template <typename T, int DP>
__device__ __forceinline__ void mha_scores(f32x4* acc, const char* nat, const uint4* frag) {
    using G = MhaGeo<T, DP>;
    const int lr = threadIdx.x & 15, g = threadIdx.x >> 4 & 3;
#pragma unroll
    for (int nb = 0; nb < G::NB; ++nb) {
        const char* a = nat + (nb * 16 + lr) * G::NROW + g * 16;
#pragma unroll
        for (int s = 0; s < G::KS; ++s) MhaMma<T>::run(*(const uint4*)(a + s * 64), frag[s], acc[nb]);
    }
}
// acc[cb] += sum_j trn[cb*16 + m][j] * pimg[own row][j] over the TN streamed rows of the tile
template <typename T, int DP>
__device__ __forceinline__ void mha_outer(f32x4* acc, const char* trn, const char* prow) {
    using G = MhaGeo<T, DP>;
    const int lr = threadIdx.x & 15, g = threadIdx.x >> 4 & 3;
    const uint4 b0 = *(const uint4*)(prow + g * 16), b1 = *(const uint4*)(prow + 64 + g * 16);
#pragma unroll
    for (int cb = 0; cb < G::CB; ++cb) {
        const char* a = trn + (cb * 16 + lr) * MHA_TROW + g * 16;
        MhaMma<T>::run(*(const uint4*)a, b0, acc[cb]);
        MhaMma<T>::run(*(const uint4*)(a + 64), b1, acc[cb]);
    }
}

__device__ __forceinline__ float mha_max4(float v) {       // over the 4 lanes that share lane & 15
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float mha_sum4(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// The P / dS images are wave-private: row wave*16 + lr is written by the four lanes of this wave that share lr and read back by this
// wave only.  LDS operations of one wave complete in issue order, so no workgroup barrier is needed between the write and the read:
// only the compiler has to keep them in order.
__device__ __forceinline__ void mha_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

extern __shared__ __attribute__((aligned(16))) char mha_smem[];

// ------------------------------------------------------------------------------------------------------
// forward: block = (sample, head, query tile)
// ------------------------------------------------------------------------------------------------------
template <typename T, int DP>
__global__ __launch_bounds__(256) void mha_fwd_kernel(const MhaArgs a) {
    using G = MhaGeo<T, DP>;
    const int tile = blockIdx.x % a.tiles, nh = blockIdx.x / a.tiles, h = nh % a.heads, n = nh / a.heads;
    const int wave = threadIdx.x >> 6, lr = threadIdx.x & 15, g = threadIdx.x >> 4 & 3;
    const int i = tile * MHA_OWN + wave * 16 + lr;                  // this lane's query row
    const size_t row0 = (size_t)n * a.S;
    const T* qp = (const T*)a.q + row0 * a.ldq + h * a.d;
    const T* kp = (const T*)a.k + row0 * a.ldk + h * a.d;
    const T* vp = (const T*)a.v + row0 * a.ldv + h * a.d;
    char* k_nat = mha_smem;
    char* v_trn = k_nat + G::NAT;
    char* p_img = v_trn + G::TRN;
    char* prow = p_img + (wave * 16 + lr) * MHA_TROW;

    uint4 qf[G::KS];
    mha_frag<T, DP>(qf, qp, a.ldq, i, a.S, a.d, a.vec);
    f32x4 o[G::CB];
#pragma unroll
    for (int cb = 0; cb < G::CB; ++cb) o[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    float mrun = -INFINITY, lrun = 0.f;

    for (int j0 = 0; j0 < a.S; j0 += G::TN) {
        __syncthreads();
        mha_stage<T, DP>(k_nat, nullptr, kp, a.ldk, j0, a.S, a.d, a.vec);
        mha_stage<T, DP>(nullptr, v_trn, vp, a.ldv, j0, a.S, a.d, a.vec);
        __syncthreads();
        f32x4 s[G::NB];
#pragma unroll
        for (int nb = 0; nb < G::NB; ++nb) s[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
        mha_scores<T, DP>(s, k_nat, qf);
        float mx = -INFINITY;
#pragma unroll
        for (int nb = 0; nb < G::NB; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + nb * 16 + g * 4 + r;
                s[nb][r] = j < a.S ? s[nb][r] * a.scale : -INFINITY;
                mx = fmaxf(mx, s[nb][r]);
            }
        mx = mha_max4(mx);                          // finite: every tile has at least one key
        const float mnew = fmaxf(mrun, mx);
        const float alpha = __expf(mrun - mnew);
        float sum = 0.f;
#pragma unroll
        for (int nb = 0; nb < G::NB; ++nb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[nb][r] = __expf(s[nb][r] - mnew);
                sum += s[nb][r];
            }
            mha_lds4<T>(prow + (nb * 16 + g * 4) * G::ES, s[nb]);
        }
        lrun = lrun * alpha + mha_sum4(sum);
        mrun = mnew;
#pragma unroll
        for (int cb = 0; cb < G::CB; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[cb][r] *= alpha;
        mha_wave_sync();
        mha_outer<T, DP>(o, v_trn, prow);
    }
    if (i >= a.S) return;
    const float inv = 1.f / lrun;
    T* op = (T*)a.out + (row0 + i) * a.ldo + h * a.d;
#pragma unroll
    for (int cb = 0; cb < G::CB; ++cb) {
        const int c = cb * 16 + g * 4;
        if (c < a.d) {
            const float f[4] = {o[cb][0] * inv, o[cb][1] * inv, o[cb][2] * inv, o[cb][3] * inv};
            mha_st4<T>(op + c, f, a.vec, 0);
        }
    }
    if (a.lse && g == 0) a.lse[((size_t)n * a.heads + h) * a.S + i] = mrun + logf(lrun);
}

// ------------------------------------------------------------------------------------------------------
// delta[n][h][i] = sum_c dout[i][h*d + c] * out[i][h*d + c]
// ------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void mha_delta_kernel(const MhaArgs a) {
    const long long total = (long long)a.N * a.heads * a.S;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int i = (int)(t % a.S);
    const long long nh = t / a.S;
    const int h = (int)(nh % a.heads), n = (int)(nh / a.heads);
    const size_t row = (size_t)n * a.S + i;
    const T* op = (const T*)a.o + row * a.ldo + h * a.d;
    const T* dp = (const T*)a.dout + row * a.lddo + h * a.d;
    float s = 0.f;
    for (int c = 0; c < a.d; ++c) s = fmaf(ET<T>::ld(dp + c), ET<T>::ld(op + c), s);
    a.delta[t] = s;
}

// ------------------------------------------------------------------------------------------------------
// dQ: block = (sample, head, query tile), sweeps the keys
// ------------------------------------------------------------------------------------------------------
template <typename T, int DP>
__global__ __launch_bounds__(256) void mha_bwd_q_kernel(const MhaArgs a) {
    using G = MhaGeo<T, DP>;
    const int tile = blockIdx.x % a.tiles, nh = blockIdx.x / a.tiles, h = nh % a.heads, n = nh / a.heads;
    const int wave = threadIdx.x >> 6, lr = threadIdx.x & 15, g = threadIdx.x >> 4 & 3;
    const int i = tile * MHA_OWN + wave * 16 + lr;
    const size_t row0 = (size_t)n * a.S;
    const T* qp = (const T*)a.q + row0 * a.ldq + h * a.d;
    const T* kp = (const T*)a.k + row0 * a.ldk + h * a.d;
    const T* vp = (const T*)a.v + row0 * a.ldv + h * a.d;
    const T* dop = (const T*)a.dout + row0 * a.lddo + h * a.d;
    char* k_nat = mha_smem;
    char* v_nat = k_nat + G::NAT;
    char* k_trn = v_nat + G::NAT;
    char* ds_img = k_trn + G::TRN;
    char* dsrow = ds_img + (wave * 16 + lr) * MHA_TROW;

    uint4 qf[G::KS], dof[G::KS];
    mha_frag<T, DP>(qf, qp, a.ldq, i, a.S, a.d, a.vec);
    mha_frag<T, DP>(dof, dop, a.lddo, i, a.S, a.d, a.vec);
    const size_t stat = ((size_t)n * a.heads + h) * a.S;
    const float lse = i < a.S ? a.lse[stat + i] : 0.f;
    const float delta = i < a.S ? a.delta[stat + i] : 0.f;
    f32x4 dq[G::CB];
#pragma unroll
    for (int cb = 0; cb < G::CB; ++cb) dq[cb] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int j0 = 0; j0 < a.S; j0 += G::TN) {
        __syncthreads();
        mha_stage<T, DP>(k_nat, k_trn, kp, a.ldk, j0, a.S, a.d, a.vec);
        mha_stage<T, DP>(v_nat, nullptr, vp, a.ldv, j0, a.S, a.d, a.vec);
        __syncthreads();
        f32x4 s[G::NB], dp[G::NB];
#pragma unroll
        for (int nb = 0; nb < G::NB; ++nb) { s[nb] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[nb] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        mha_scores<T, DP>(s, k_nat, qf);
        mha_scores<T, DP>(dp, v_nat, dof);
#pragma unroll
        for (int nb = 0; nb < G::NB; ++nb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + nb * 16 + g * 4 + r;
                const float p = j < a.S ? __expf(s[nb][r] * a.scale - lse) : 0.f;
                s[nb][r] = p * (dp[nb][r] - delta);
            }
            mha_lds4<T>(dsrow + (nb * 16 + g * 4) * G::ES, s[nb]);
        }
        mha_wave_sync();
        mha_outer<T, DP>(dq, k_trn, dsrow);
    }
    if (i >= a.S) return;
    T* dqp = (T*)a.dq + (row0 + i) * a.ldd + h * a.d;
#pragma unroll
    for (int cb = 0; cb < G::CB; ++cb) {
        const int c = cb * 16 + g * 4;
        if (c < a.d) {
            const float f[4] = {dq[cb][0] * a.scale, dq[cb][1] * a.scale, dq[cb][2] * a.scale, dq[cb][3] * a.scale};
            mha_st4<T>(dqp + c, f, a.vec, a.acc);
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// dK and dV: block = (sample, head, key tile), sweeps the queries
// ------------------------------------------------------------------------------------------------------
template <typename T, int DP>
__global__ __launch_bounds__(256) void mha_bwd_kv_kernel(const MhaArgs a) {
    using G = MhaGeo<T, DP>;
    const int tile = blockIdx.x % a.tiles, nh = blockIdx.x / a.tiles, h = nh % a.heads, n = nh / a.heads;
    const int wave = threadIdx.x >> 6, lr = threadIdx.x & 15, g = threadIdx.x >> 4 & 3;
    const int j = tile * MHA_OWN + wave * 16 + lr;                  // this lane's key row
    const size_t row0 = (size_t)n * a.S;
    const T* qp = (const T*)a.q + row0 * a.ldq + h * a.d;
    const T* kp = (const T*)a.k + row0 * a.ldk + h * a.d;
    const T* vp = (const T*)a.v + row0 * a.ldv + h * a.d;
    const T* dop = (const T*)a.dout + row0 * a.lddo + h * a.d;
    char* q_nat = mha_smem;
    char* do_nat = q_nat + G::NAT;
    char* q_trn = do_nat + G::NAT;
    char* do_trn = q_trn + G::TRN;
    char* p_img = do_trn + G::TRN;
    char* ds_img = p_img + G::PB;
    float* rowst = (float*)(ds_img + G::PB);                        // lse[TN] | delta[TN] of the streamed queries
    char* prow = p_img + (wave * 16 + lr) * MHA_TROW;
    char* dsrow = ds_img + (wave * 16 + lr) * MHA_TROW;

    uint4 kf[G::KS], vf[G::KS];
    mha_frag<T, DP>(kf, kp, a.ldk, j, a.S, a.d, a.vec);
    mha_frag<T, DP>(vf, vp, a.ldv, j, a.S, a.d, a.vec);
    const size_t stat = ((size_t)n * a.heads + h) * a.S;
    f32x4 dk[G::CB], dv[G::CB];
#pragma unroll
    for (int cb = 0; cb < G::CB; ++cb) { dk[cb] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[cb] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    for (int i0 = 0; i0 < a.S; i0 += G::TN) {
        __syncthreads();
        mha_stage<T, DP>(q_nat, q_trn, qp, a.ldq, i0, a.S, a.d, a.vec);
        mha_stage<T, DP>(do_nat, do_trn, dop, a.lddo, i0, a.S, a.d, a.vec);
        if (threadIdx.x < G::TN) {
            const int i = i0 + threadIdx.x;
            rowst[threadIdx.x] = i < a.S ? a.lse[stat + i] : 0.f;
            rowst[G::TN + threadIdx.x] = i < a.S ? a.delta[stat + i] : 0.f;
        }
        __syncthreads();
        f32x4 s[G::NB], dp[G::NB];
#pragma unroll
        for (int nb = 0; nb < G::NB; ++nb) { s[nb] = f32x4{0.f, 0.f, 0.f, 0.f}; dp[nb] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        mha_scores<T, DP>(s, q_nat, kf);
        mha_scores<T, DP>(dp, do_nat, vf);
#pragma unroll
        for (int nb = 0; nb < G::NB; ++nb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int il = nb * 16 + g * 4 + r;
                const float p = i0 + il < a.S ? __expf(s[nb][r] * a.scale - rowst[il]) : 0.f;
                s[nb][r] = p;
                dp[nb][r] = p * (dp[nb][r] - rowst[G::TN + il]);
            }
            mha_lds4<T>(prow + (nb * 16 + g * 4) * G::ES, s[nb]);
            mha_lds4<T>(dsrow + (nb * 16 + g * 4) * G::ES, dp[nb]);
        }
        mha_wave_sync();
        mha_outer<T, DP>(dv, do_trn, prow);
        mha_outer<T, DP>(dk, q_trn, dsrow);
    }
    if (j >= a.S) return;
    T* dkp = (T*)a.dk + (row0 + j) * a.ldd + h * a.d;
    T* dvp = (T*)a.dv + (row0 + j) * a.ldd + h * a.d;
#pragma unroll
    for (int cb = 0; cb < G::CB; ++cb) {
        const int c = cb * 16 + g * 4;
        if (c < a.d) {
            const float fk[4] = {dk[cb][0] * a.scale, dk[cb][1] * a.scale, dk[cb][2] * a.scale, dk[cb][3] * a.scale};
            const float fv[4] = {dv[cb][0], dv[cb][1], dv[cb][2], dv[cb][3]};
            mha_st4<T>(dkp + c, fk, a.vec, a.acc);
            mha_st4<T>(dvp + c, fv, a.vec, a.acc);
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------
static bool mha_rows16(int dtype, const void* p, int64_t ld) { return aligned16(p) && (ld * esize(dtype)) % 16 == 0; }

static int mha_check(int dtype, const MhaArgs& a) {
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "compute dtype must be f32 or bf16");
    YDL_CHECK(a.N > 0 && a.S > 0 && a.heads > 0, "empty problem");
    YDL_CHECK(a.d >= 8 && a.d <= 128 && a.d % 8 == 0, "head dimension must be a multiple of 8 between 8 and 128");
    YDL_CHECK(a.q && a.k && a.v, "q, k and v are required");
    const int C = a.heads * a.d;
    YDL_CHECK(a.ldq >= C && a.ldk >= C && a.ldv >= C, "row strides smaller than heads * d");
    YDL_CHECK((int64_t)a.N * a.heads * ((a.S + MHA_OWN - 1) / MHA_OWN) < (1ll << 31), "too many tiles for one launch");
    return 0;
}

template <typename T, int DP> static size_t mha_fwd_lds() { using G = MhaGeo<T, DP>; return G::NAT + G::TRN + G::PB; }
template <typename T, int DP> static size_t mha_bq_lds() { using G = MhaGeo<T, DP>; return 2 * G::NAT + G::TRN + G::PB; }
template <typename T, int DP> static size_t mha_bkv_lds() {
    using G = MhaGeo<T, DP>;
    return 2 * G::NAT + 2 * G::TRN + 2 * G::PB + 2 * G::TN * sizeof(float);
}

template <typename T, int DP> static int mha_launch_fwd(const MhaArgs& a, hipStream_t st) {
    const size_t lds = mha_fwd_lds<T, DP>();
    YDL_SET_MAX_LDS((mha_fwd_kernel<T, DP>), lds);
    mha_fwd_kernel<T, DP><<<a.N * a.heads * a.tiles, 256, lds, st>>>(a);
    return 0;
}
template <typename T, int DP> static int mha_launch_bwd(const MhaArgs& a, hipStream_t st) {
    const size_t lq = mha_bq_lds<T, DP>(), lkv = mha_bkv_lds<T, DP>();
    YDL_SET_MAX_LDS((mha_bwd_q_kernel<T, DP>), lq);
    YDL_SET_MAX_LDS((mha_bwd_kv_kernel<T, DP>), lkv);
    const long long rows = (long long)a.N * a.heads * a.S;
    mha_delta_kernel<T><<<(unsigned)((rows + 255) / 256), 256, 0, st>>>(a);
    mha_bwd_q_kernel<T, DP><<<a.N * a.heads * a.tiles, 256, lq, st>>>(a);
    mha_bwd_kv_kernel<T, DP><<<a.N * a.heads * a.tiles, 256, lkv, st>>>(a);
    return 0;
}
#define MHA_DISPATCH(FN, a, st)                                                                  \
    do {                                                                                         \
        int rc_;                                                                                 \
        if (dtype == YDL_F32) rc_ = a.d <= 32 ? FN<float, 32>(a, st) : a.d <= 64 ? FN<float, 64>(a, st) : FN<float, 128>(a, st);      \
        else rc_ = a.d <= 32 ? FN<bf16_t, 32>(a, st) : a.d <= 64 ? FN<bf16_t, 64>(a, st) : FN<bf16_t, 128>(a, st);                    \
        if (rc_) return rc_;                                                                     \
    } while (0)

extern "C" int ydl_mha_fwd(int dtype, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo,
                           float* lse, int N, int S, int heads, int d, float scale, void* stream) {
    MhaArgs a = {};
    a.q = q; a.k = k; a.v = v; a.out = out; a.lse = lse;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.N = N; a.S = S; a.heads = heads; a.d = d; a.scale = scale;
    if (int rc = mha_check(dtype, a)) return rc;
    YDL_CHECK(out && ldo >= heads * d, "out is required, with a row stride of at least heads * d");
    a.tiles = (S + MHA_OWN - 1) / MHA_OWN;
    a.vec = mha_rows16(dtype, q, ldq) && mha_rows16(dtype, k, ldk) && mha_rows16(dtype, v, ldv) && mha_rows16(dtype, out, ldo);
    MHA_DISPATCH(mha_launch_fwd, a, (hipStream_t)stream);
    YDL_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t ydl_mha_bwd_ws_bytes(int N, int S, int heads) {
    if (N <= 0 || S <= 0 || heads <= 0) return 0;
    return (int64_t)N * S * heads * (int64_t)sizeof(float);
}

extern "C" int ydl_mha_bwd(int dtype, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const void* out, int ldo,
                           const float* lse, const void* dout, int lddo, void* dq, void* dk, void* dv, int ldd, int accumulate,
                           float* ws, int N, int S, int heads, int d, float scale, void* stream) {
    MhaArgs a = {};
    a.q = q; a.k = k; a.v = v; a.o = out; a.dout = dout; a.lse = (float*)lse; a.delta = ws;
    a.dq = dq; a.dk = dk; a.dv = dv;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.lddo = lddo; a.ldd = ldd;
    a.N = N; a.S = S; a.heads = heads; a.d = d; a.scale = scale; a.acc = accumulate;
    if (int rc = mha_check(dtype, a)) return rc;
    YDL_CHECK(out && lse && dout && dq && dk && dv && ws, "out, lse, dout, dq, dk, dv and the workspace are required");
    YDL_CHECK(ldo >= heads * d && lddo >= heads * d && ldd >= heads * d, "row strides smaller than heads * d");
    a.tiles = (S + MHA_OWN - 1) / MHA_OWN;
    a.vec = mha_rows16(dtype, q, ldq) && mha_rows16(dtype, k, ldk) && mha_rows16(dtype, v, ldv) && mha_rows16(dtype, dout, lddo) &&
            mha_rows16(dtype, dq, ldd) && mha_rows16(dtype, dk, ldd) && mha_rows16(dtype, dv, ldd);
    MHA_DISPATCH(mha_launch_bwd, a, (hipStream_t)stream);
    YDL_LAUNCH_CHECK();
    return 0;
}
