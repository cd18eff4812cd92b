// Implicit-GEMM convolution on MFMA for gfx950: forward, dgrad (same kernel, different tap tables) and wgrad.
//
// Data layout: activations NHWC (pixel stride ld), weights KRSC [Cout][taps][Kc] (K contiguous).
// GEMM view (forward):  Y[cout][pixel] = sum_k W[cout][k] * X[k][pixel],  k = (tap, cin) flattened.
// The MFMA "A" operand is the weight tile (rows = cout) and the "B" operand the gathered activation tile
// (cols = pixels), so a lane's 4 accumulator registers are 4 consecutive output channels of ONE pixel:
// the epilogue stores 8 B (bf16) / 16 B (f32) per lane straight into NHWC rows.
//
// Both element types share one byte geometry: a K-step is 128 bytes per row (64 bf16 / 32 f32), moved as
// eight 16-byte chunks; an LDS row is 128+16 bytes (one access-width pad => conflict-free ds_read_b128).
// bf16: v_mfma_f32_16x16x32_bf16, lane reads 8 consecutive k.  f32: 4 x v_mfma_f32_16x16x4_f32 on the 4
// floats of the same 16-byte read (k permuted identically for both operands; exact f32 fmaf chains).
#include "common.h"
#include <type_traits>
#include <stdlib.h>

#define ROWB 144      // LDS row stride in bytes (128 data + 16 pad): wgrad tiles (transposed reads)
#define GROWB 128     // igemm tiles: unpadded rows, XOR-swizzled chunks
#define MAXTAPS 64

struct IgemmArgs {
    const void* A;    // gathered activations (x for fwd, dy for dgrad)
    const void* B;    // weights [rowsB][Ttot][Kc]
    void* C;          // output activations
    float* stats;     // optional BN partials [gridM][2][stats_ld]
    int N, Hi, Wi, lda;
    int Kc;           // K elements per tap (channel count of A padded to a chunk multiple)
    int Ho, Wo, ldc;  // output tensor
    int Cout;         // logical output channels (rows of B that exist)
    int Cst;          // channels stored (>= Cout, zero filled beyond Cout)
    int Hg, Wg;       // output grid points per image handled by this launch
    int in_mul, out_mul, out_h0, out_w0;
    int ntaps, Ttot;
    int accumulate;
    int M;            // N*Hg*Wg
    int stats_ld;
    int stats_atomic; // 0: stats = per-block partial rows [gridM][2][stats_ld] (sum, M2);  1: stats = [YDL_BN_REPLICAS][2][stats_ld]
                      //    running (sum, sum of squares), every block adds its share with f32 atomics (replica = block index & 7)
    unsigned bytesA, bytesB;   // buffer extents for the range-checked loads
    unsigned bytesC;           // extent of C (igemm2s_kernel's accumulate pre-pass reads it by LDS-DMA; 0 = not set)
    unsigned ldb_bytes;        // byte stride between weight rows (Ttot*Kc*ES when dense)
    // several output-parity classes in one launch (stride-s dgrad); ncls <= 1: the single-class fields above apply
    int ncls;
    int cls_tile0[5];          // first pixel tile of each class (prefix sums), [ncls] = total
    int cls_ntaps[4], cls_tap0[4], cls_Hg[4], cls_Wg[4], cls_M[4], cls_h0[4], cls_w0[4];
    int grid_n;                // number of output-channel tiles (the grid is 1-D: grid_m * grid_n)
    int grid_m;                // number of pixel tiles (all classes)
    int m_fastest;             // igemm2 tile order: 0 = channel tiles of one pixel tile are neighbours (activations shared in L2),
                               //                    1 = pixel tiles of one channel tile are neighbours (weight slab stays in L2)
    signed char dh[MAXTAPS], dw[MAXTAPS];
    unsigned char wt[MAXTAPS];
    ydl_bnred br;              // nseg > 0: the ring epilogue also runs the BatchNorm-backward reduce of the producers of C (dgrad only)
};

template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
    __device__ static __forceinline__ void run(const uint4& a, const uint4& b, f32x4& acc) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    __device__ static __forceinline__ void run(const uint4& a, const uint4& b, f32x4& acc) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
    }
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// XCD-aware work-item order (speed only, any placement is correct): the dispatcher deals consecutive workgroups
// round-robin over the 8 XCDs, each with a private L2.  Remapping linear id L -> (L % 8) * chunk + L / 8 hands every XCD
// a CONTIGUOUS range of logical tiles, so tiles that share operand panels (all N-tiles of one pixel tile, the halo
// neighbours of a 3x3 conv, all weight-gradient tiles of one pixel range) hit the same L2 at about the same time.
__device__ __forceinline__ int xcd_remap(int L, int total) {
    const int q = total >> 3, r = total & 7;
    const int xcd = L & 7, slot = L >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
}

// Sum NV per-lane values over the 16 lanes of a row (lanes 16g..16g+15).  Stages with more than one live value use
// the transposing butterfly: the lane whose bit s is 0 keeps the even-indexed values, its partner the odd ones, each
// adds the partner's copy => the live count halves and one shuffle serves two values.  Result: slot tt of lane r
// holds the total of value index (tt << 4 | r) when NV >= 16, or of (r & (NV-1)) in slot 0 otherwise.
template <int NV>
__device__ __forceinline__ void row_reduce(float (&v)[NV], int lrow) {
    int cnt = NV;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int mask = 1 << s;
        const bool hi = (lrow >> s) & 1;
        if (cnt > 1) {
#pragma unroll
            for (int i = 0; i < NV / 2; ++i)
                if (i < cnt / 2) {
                    float a = v[2 * i], b = v[2 * i + 1];
                    float keep = hi ? b : a, send = hi ? a : b;
                    v[i] = keep + __shfl_xor(send, mask, 64);
                }
            cnt >>= 1;
        } else {
            v[0] += __shfl_xor(v[0], mask, 64);
        }
    }
}

// Epilogue shared by the tiled kernels: optional accumulate, NHWC store (8 B bf16 / 16 B f32 per lane), and the block-local
// two-pass BN partial statistics.  ``smem`` is reused as scratch: every LDS read/DMA of the main loop must be complete and
// fenced by a barrier before the call.
template <typename T, int BM, int BN, int NW, int WP>
__device__ __forceinline__ void igemm_epilogue(const IgemmArgs& p, f32x4 (&acc)[(BN / (NW / WP)) / 16][BM / (16 * WP)],
                                               unsigned char* smem, int m0, int n0, int mtile, int c_M, int c_Wg, int c_Hg,
                                               int c_h0, int c_w0) {
    constexpr int WN = NW / WP;
    constexpr int BNW = BN / WN;
    constexpr int CT = BNW / 16;
    constexpr int PT = BM / (16 * WP);
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int wc = wave % WN, wp = wave / WN;
    const int lrow = lane & 15;
    // ---------------- epilogue: store ----------------
    T* Cg = (T*)p.C;
    const int cq = (lane >> 4) * 4;
    // accumulate: fold the previous contents of C into the accumulators first (whole-vector updates in a separate pass:
    // keeps the store loop and the statistics below free of per-element selects, which cost 100+ VGPRs when fused)
    if (p.accumulate) {
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            int m = m0 + wp * (BM / WP) + j * 16 + lrow;
            if (m < c_M) {
                int gw = m % c_Wg;
                int tmp = m / c_Wg;
                int gh = tmp % c_Hg;
                int n = tmp / c_Hg;
                size_t pix = ((size_t)(n * p.Ho + gh * p.out_mul + c_h0)) * p.Wo + (gw * p.out_mul + c_w0);
                const T* src = Cg + pix * p.ldc;
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    int co = n0 + wc * BNW + c * 16 + cq;
                    f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (co + 3 < p.Cst) {
                        if constexpr (sizeof(T) == 4) {
                            float4 q4 = *(const float4*)(src + co);
                            o = f32x4{q4.x, q4.y, q4.z, q4.w};
                        } else {
                            uint2 q2 = *(const uint2*)(src + co);
                            o = f32x4{__uint_as_float(q2.x << 16), __uint_as_float(q2.x & 0xffff0000u),
                                      __uint_as_float(q2.y << 16), __uint_as_float(q2.y & 0xffff0000u)};
                        }
                    } else {
                        float t0 = co < p.Cst ? ET<T>::ld(src + co) : 0.f;
                        float t1 = co + 1 < p.Cst ? ET<T>::ld(src + co + 1) : 0.f;
                        float t2 = co + 2 < p.Cst ? ET<T>::ld(src + co + 2) : 0.f;
                        o = f32x4{t0, t1, t2, 0.f};
                    }
                    acc[c][j] += o;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < PT; ++j) {
        int m = m0 + wp * (BM / WP) + j * 16 + lrow;
        if (m < c_M) {
            int gw = m % c_Wg;
            int tmp = m / c_Wg;
            int gh = tmp % c_Hg;
            int n = tmp / c_Hg;
            size_t pix = ((size_t)(n * p.Ho + gh * p.out_mul + c_h0)) * p.Wo + (gw * p.out_mul + c_w0);
            T* dst = Cg + pix * p.ldc;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                int co = n0 + wc * BNW + c * 16 + cq;
                if (co + 3 < p.Cst) {
                    if constexpr (sizeof(T) == 4) {
                        *(float4*)(dst + co) = make_float4(acc[c][j][0], acc[c][j][1], acc[c][j][2], acc[c][j][3]);
                    } else {
                        uint2 u;
                        u.x = (uint32_t)f2bf(acc[c][j][0]) | ((uint32_t)f2bf(acc[c][j][1]) << 16);
                        u.y = (uint32_t)f2bf(acc[c][j][2]) | ((uint32_t)f2bf(acc[c][j][3]) << 16);
                        *(uint2*)(dst + co) = u;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (co + e < p.Cst) ET<T>::st(dst + co + e, acc[c][j][e]);
                }
            }
        }
    }

    // ---------------- epilogue: BN partial statistics (block-local two-pass => Chan-mergeable) ----------
    // A lane holds NV = 4*CT channel values per pixel; the sum over the 16 pixel-lanes of a row is a transposing
    // butterfly (each stage halves the values a lane keeps): 30 shuffles for 32 values instead of 128.
    if (p.stats != nullptr) {
        constexpr int NV = 4 * CT;
        float* red = (float*)smem;             // [4][BN]; safe: all LDS reads finished at the last barrier
        float* smean = red + WP * BN;          // [BN]
        const int nvalid = min(BM, c_M - m0);
        const int lgrp = lane >> 4;
        float v[NV];
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float t2 = 0.f;
#pragma unroll
                for (int j = 0; j < PT; ++j) t2 += acc[c][j][e];   // rows beyond M are exact zeros
                v[c * 4 + e] = t2;
            }
        row_reduce<NV>(v, lrow);
        // after the reduce, slot tt of lane lrow holds value index (tt << 4 | lrow) (NV >= 16) or (lrow & (NV-1))
        auto chan_of = [&](int idx) { return wc * BNW + (idx >> 2) * 16 + lgrp * 4 + (idx & 3); };
        if (NV >= 16) {
#pragma unroll
            for (int tt = 0; tt < (NV >= 16 ? NV / 16 : 1); ++tt) red[wp * BN + chan_of((tt << 4) | lrow)] = v[tt];
        } else if (lrow < NV) {
            red[wp * BN + chan_of(lrow)] = v[0];
        }
        __syncthreads();
        float tot = 0.f;
        if (t < BN) {
            tot = 0.f;
#pragma unroll
            for (int g2 = 0; g2 < WP; ++g2) tot += red[g2 * BN + t];
            smean[t] = tot / (float)nvalid;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float mu = smean[wc * BNW + c * 16 + cq + e];
                float t2 = 0.f;
#pragma unroll
                for (int j = 0; j < PT; ++j) {
                    int m = m0 + wp * (BM / WP) + j * 16 + lrow;
                    float d = acc[c][j][e] - mu;
                    t2 += (m < c_M) ? d * d : 0.f;
                }
                v[c * 4 + e] = t2;
            }
        row_reduce<NV>(v, lrow);
        __syncthreads();   // everyone has read smean/red before red is overwritten
        if (NV >= 16) {
#pragma unroll
            for (int tt = 0; tt < (NV >= 16 ? NV / 16 : 1); ++tt) red[wp * BN + chan_of((tt << 4) | lrow)] = v[tt];
        } else if (lrow < NV) {
            red[wp * BN + chan_of(lrow)] = v[0];
        }
        __syncthreads();
        if (t < BN && n0 + t < p.Cout) {
            float m2 = 0.f;
#pragma unroll
            for (int g2 = 0; g2 < WP; ++g2) m2 += red[g2 * BN + t];
            if (p.stats_atomic) {
                float* dst = p.stats + (size_t)(mtile & (YDL_BN_REPLICAS - 1)) * 2 * p.stats_ld;
                atomicAdd(dst + n0 + t, tot);
                atomicAdd(dst + p.stats_ld + n0 + t, m2 + tot * tot / (float)nvalid);      // sum of squares of this block
            } else {
                float* dst = p.stats + (size_t)mtile * 2 * p.stats_ld;
                dst[n0 + t] = tot;
                dst[p.stats_ld + n0 + t] = m2;
            }
        }
    }
}

// BM = pixel tile (64 or 128), BN = output-channel tile (16, 64 or 128), NW = waves per CTA (4 or 8).
// Waves form a WP(=4, pixels) x WN(=NW/4, channels) grid: a wave owns BM/4 pixels x BN/WN channels.  The 8-wave
// form halves the accumulators and LDS fragment reads per wave and doubles the waves per SIMD at the same LDS
// footprint (more MFMA/VALU/LDS overlap between co-resident waves).
//
// Loader (the main loop is issue-bound on VALU if addresses are derived per K-step, so everything that does not
// depend on k is hoisted): per row a 32-bit byte offset of its (0,0) tap and a 64-bit tap-validity mask are computed
// once; a K-step adds one table entry (tap delta) and selects "offset or 0xFFFFFFFF" — the loads are raw buffer
// loads whose range check returns zeros for the padding taps and the tail rows, so there is no branch.
template <typename T, int BM, int BN, int NW, int WP = 4>
__global__ __launch_bounds__(NW * 64) void igemm_kernel(const IgemmArgs p) {
    constexpr int V = ET<T>::V;
    constexpr int ES = sizeof(T);
    constexpr int RPP = NW * 8;                 // tile rows covered by one loader pass (threads / 8 chunks)
    constexpr int AR = BM / RPP;                // A rows per thread
    constexpr int BR = (BN + RPP - 1) / RPP;    // B rows per thread
    constexpr int WN = NW / WP;                 // wave groups along output channels (WP groups along pixels)
    constexpr int BNW = BN / WN;                // channels per wave
    constexpr int CT = BNW / 16;                // cout tiles per wave
    constexpr int PT = BM / (16 * WP);          // pixel tiles per wave
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sA = smem;                           // [2][BM][GROWB]
    unsigned char* sB = smem + 2 * BM * GROWB;           // [2][BN][GROWB]
    int* sTapA = (int*)(smem + 2 * (BM + BN) * GROWB);   // [MAXTAPS] byte delta of the tap in A
    int* sTapB = sTapA + MAXTAPS;                        // [MAXTAPS] byte offset of the tap inside a weight row
    int* sTapD = sTapB + MAXTAPS;                        // [MAXTAPS] (dh & 0xffff) | (dw << 16)

    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int wc = wave % WN, wp = wave / WN;   // channel group / pixel group of this wave
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    int mtile = tile / p.grid_n;
    const int ntile = tile - mtile * p.grid_n;     // N-tiles of one pixel tile are neighbours
    // stride-s dgrad: one launch covers all s*s output-parity classes; a pixel tile belongs to ONE class, which selects
    // its slice of the tap table and its output sub-grid (all values wave-uniform: scalar loads)
    int c_ntaps = p.ntaps, c_tap0 = 0, c_Hg = p.Hg, c_Wg = p.Wg, c_M = p.M, c_h0 = p.out_h0, c_w0 = p.out_w0;
    if (p.ncls > 1) {
        int c = 0;
        while (c + 1 < p.ncls && mtile >= p.cls_tile0[c + 1]) ++c;
        mtile -= p.cls_tile0[c];
        c_ntaps = p.cls_ntaps[c]; c_tap0 = p.cls_tap0[c]; c_Hg = p.cls_Hg[c]; c_Wg = p.cls_Wg[c]; c_M = p.cls_M[c];
        c_h0 = p.cls_h0[c]; c_w0 = p.cls_w0[c];
    }
    const int m0 = mtile * BM;
    const int n0 = ntile * BN;

    if (t < MAXTAPS) {
        int da = 0, db = 0, dd = 0;
        if (t < c_ntaps) {
            da = ((int)p.dh[c_tap0 + t] * p.Wi + (int)p.dw[c_tap0 + t]) * p.lda * ES;
            db = (int)p.wt[c_tap0 + t] * p.Kc * ES;
            dd = ((int)p.dh[c_tap0 + t] & 0xffff) | ((int)p.dw[c_tap0 + t] << 16);
        }
        sTapA[t] = da;
        sTapB[t] = db;
        sTapD[t] = dd;
    }

    const int q = t & 7;        // chunk column
    const int r = t >> 3;       // row 0..RPP-1
    unsigned rowoff[AR];
    int ih0[AR], iw0[AR];
#pragma unroll
    for (int i = 0; i < AR; ++i) {
        int m = m0 + r + RPP * i;
        rowoff[i] = 0;
        ih0[i] = -100000;          // tail rows: every tap fails the range test => zeros
        iw0[i] = 0;
        if (m < c_M) {
            int gw = m % c_Wg;
            int tmp = m / c_Wg;
            int gh = tmp % c_Hg;
            int n = tmp / c_Hg;
            ih0[i] = gh * p.in_mul;
            iw0[i] = gw * p.in_mul;
            rowoff[i] = (unsigned)(((n * p.Hi + ih0[i]) * p.Wi + iw0[i]) * p.lda) * (unsigned)ES;
        }
    }
    unsigned browoff[BR];
    bool bvalid[BR];
#pragma unroll
    for (int i = 0; i < BR; ++i) {
        int row = r + RPP * i;
        int co = n0 + row;
        bvalid[i] = row < BN && co < p.Cout;
        browoff[i] = (unsigned)co * p.ldb_bytes;
    }
    const int cpt = p.Kc / V;                       // chunks per tap
    const int nchunks = c_ntaps * cpt;
    const int nk = (nchunks + 7) >> 3;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, p.bytesA, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)p.B, 0, p.bytesB, 0x00020000);

    constexpr int PF = 1;     // deeper register prefetch costs an occupancy step on the 128x128 tile (measured slower)
    uint4 ra[PF][AR], rb[PF][BR];
    __syncthreads();   // tap tables visible

    // K-steps are loaded strictly in order, so the (tap, chunk-in-tap) position of this thread's chunk is carried from
    // step to step: +8 chunks with at most one wrap when a tap has >= 8 chunks (the 32-bit division it replaces was a
    // dozen VALU instructions per K-step); layers with fewer chunks per tap (stem: 1) keep the division.
    int tap_s = q / cpt, cc_s = q - (q / cpt) * cpt, Q_s = q;
    auto gload = [&](int kk, uint4 (&xa)[AR], uint4 (&xb)[BR]) {
        (void)kk;
        const int Q = Q_s;
        const int tap = tap_s;
        const int cc = cc_s * (V * ES);               // byte offset inside the tap
        Q_s += 8;
        if (cpt >= 8) {
            cc_s += 8;
            if (cc_s >= cpt) { cc_s -= cpt; ++tap_s; }
        } else {
            tap_s = Q_s / cpt;
            cc_s = Q_s - tap_s * cpt;
        }
        const bool tv = Q < nchunks;
        const int tidx = tv ? tap : 0;
        const unsigned da = (unsigned)(sTapA[tidx] + cc);
        const unsigned db = (unsigned)(sTapB[tidx] + cc);
        const int dd = sTapD[tidx];
        const int dh = (int)(short)(dd & 0xffff), dw = dd >> 16;
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            bool ok = tv && (unsigned)(ih0[i] + dh) < (unsigned)p.Hi && (unsigned)(iw0[i] + dw) < (unsigned)p.Wi;
            unsigned off = ok ? rowoff[i] + da : 0xFFFFFFFFu;
            u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsA, off, 0, 0);
            xa[i] = make_uint4(v.x, v.y, v.z, v.w);
        }
#pragma unroll
        for (int i = 0; i < BR; ++i) {
            unsigned off = (tv && bvalid[i]) ? browoff[i] + db : 0xFFFFFFFFu;
            u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsB, off, 0, 0);
            xb[i] = make_uint4(v.x, v.y, v.z, v.w);
        }
    };
    // LDS image: unpadded 128-byte rows, 16-byte chunk q of row r stored at slot q ^ ((r >> 1) & 7).  With the
    // hardware's ds_read_b128 lane groups ({0-3,12-15,20-27}, ...) a fragment read (16 rows, two neighbouring chunk
    // columns) then touches 16 distinct 16-byte bank slots of the 256-byte bank row: conflict-free (the former
    // 144-byte padded rows collided 2-way: 35 % of the LDS cycles were conflict cycles in the PMC profile).
    const int sw_st = (r >> 1) & 7;
    unsigned char* const stA = sA + r * GROWB + ((q ^ sw_st) << 4);
    unsigned char* const stB = sB + r * GROWB + ((q ^ sw_st) << 4);
    auto sstore = [&](int buf, const uint4 (&xa)[AR], const uint4 (&xb)[BR]) {
#pragma unroll
        for (int i = 0; i < AR; ++i) *(uint4*)(stA + buf * (BM * GROWB) + i * RPP * GROWB) = xa[i];
#pragma unroll
        for (int i = 0; i < BR; ++i)
            if (r + RPP * i < BN) *(uint4*)(stB + buf * (BN * GROWB) + i * RPP * GROWB) = xb[i];
    };

    f32x4 acc[CT][PT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int j = 0; j < PT; ++j) acc[c][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int u = 0; u < PF; ++u)
        if (u < nk || u == 0) gload(u, ra[u], rb[u]);
    sstore(0, ra[0], rb[0]);
    __syncthreads();
    const int lrow = lane & 15;
    const int sw_rd = (lrow >> 1) & 7;
    const int lk0 = (((lane >> 4)) ^ sw_rd) << 4;            // k-step half 0: logical chunk (lane>>4)
    const int lk1 = (((lane >> 4) + 4) ^ sw_rd) << 4;        // k-step half 1: logical chunk 4 + (lane>>4)
    const unsigned char* const fa = sB + (wc * BNW + lrow) * GROWB;
    const unsigned char* const fb = sA + (wp * (BM / WP) + lrow) * GROWB;
    for (int kk0 = 0; kk0 < nk; kk0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int kk = kk0 + u;
            if (kk < nk) {
                const int cur = kk & 1;
                if (kk + PF < nk) gload(kk + PF, ra[u], rb[u]);      // set u was consumed by the previous sstore
                const unsigned char* a_base = fa + cur * (BN * GROWB);
                const unsigned char* b_base = fb + cur * (BM * GROWB);
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    uint4 af[CT], bfr[PT];
#pragma unroll
                    for (int c = 0; c < CT; ++c) af[c] = *(const uint4*)(a_base + c * 16 * GROWB + (s ? lk1 : lk0));
#pragma unroll
                    for (int j = 0; j < PT; ++j) bfr[j] = *(const uint4*)(b_base + j * 16 * GROWB + (s ? lk1 : lk0));
#pragma unroll
                    for (int c = 0; c < CT; ++c)
#pragma unroll
                        for (int j = 0; j < PT; ++j) Mma<T>::run(af[c], bfr[j], acc[c][j]);
                }
                if (kk + 1 < nk) sstore(cur ^ 1, ra[(u + 1) % PF], rb[(u + 1) % PF]);
                __syncthreads();
            }
        }
    }

    igemm_epilogue<T, BM, BN, NW, WP>(p, acc, smem, m0, n0, mtile, c_M, c_Wg, c_Hg, c_h0, c_w0);
}

// ------------------------------------------------------------------------------------------------------
// Epilogue of the bf16 ring kernel.
//  * stores: the accumulator layout gives a lane 4 consecutive channels of one pixel (8 bytes), so a direct store touches a
//    pixel row in 32-byte pieces from four different instructions.  Here the tile is transposed through the (now free) LDS
//    ring as bf16 [pixel][channel] with the 16-byte chunks XOR-swizzled by the row, then every lane stores 16 bytes and 8-16
//    neighbouring lanes cover a whole pixel row: full-line writes, 1/2 the store instructions.
//  * BN partials in ONE pass: per lane the exact (n, mean, M2) of its PT values, Chan-merged over the 16 pixel lanes with the
//    transposing butterfly (each stage halves the live values) and over the WP pixel waves through LDS — same [grid_m][2][C]
//    (sum, M2) contract as igemm_epilogue, one barrier instead of four.
// ------------------------------------------------------------------------------------------------------
// RED: the fused BatchNorm-backward reduce; scoef = LDS table [BN][4] (scale, shift, mean, invstd) of the tile's channels, zeros
// outside the segments (br_fill_coef)
template <int BN>
__device__ __forceinline__ void br_fill_coef(const IgemmArgs& p, float* scoef, int n0, int t) {
    if (t < BN) {
        const int c = n0 + t;
        const int sgm = (p.br.nseg > 1 && c >= p.br.c0[1]) ? 1 : 0;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c >= p.br.c0[sgm] && c < p.br.c1[sgm]) {
            const int cl = c - p.br.c0[sgm];
            v = make_float4(p.br.scale[sgm][cl], p.br.shift[sgm][cl], p.br.mean[sgm][cl], p.br.invstd[sgm][cl]);
        }
        *(float4*)(scoef + t * 4) = v;
    }
}
template <int BM, int BN, int NW, int WP, bool RED = false, bool STATS = true>
__device__ __forceinline__ void igemm2_epilogue(const IgemmArgs& p, f32x4 (&acc)[(BN / (NW / WP)) / 16][BM / (16 * WP)],
                                                unsigned char* smem, int m0, int n0, int mtile, int c_M, int c_Wg, int c_Hg,
                                                int c_h0, int c_w0, const float* scoef = nullptr, const bool acc_done = false) {
    using T = bf16_t;
    constexpr int WN = NW / WP;
    constexpr int BNW = BN / WN;
    constexpr int CT = BNW / 16;
    constexpr int PT = BM / (16 * WP);
    constexpr int NT = NW * 64;
    constexpr int CPR = BN / 8;                 // 16-byte chunks per tile row
    constexpr int ORB = BN * 2;                 // bytes per tile row
    constexpr int RPS = NT / CPR;               // rows per store pass
    static_assert(BM % RPS == 0, "store passes must tile the rows");
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int wc = wave % WN, wp = wave / WN;
    const int lrow = lane & 15, lgrp = lane >> 4;
    T* Cg = (T*)p.C;
    auto pixel_of = [&](int m) -> size_t {
        const int gw = m % c_Wg;
        const int tmp = m / c_Wg;
        const int gh = tmp % c_Hg;
        const int n = tmp / c_Hg;
        return ((size_t)(n * p.Ho + gh * p.out_mul + c_h0)) * p.Wo + (gw * p.out_mul + c_w0);
    };
    const bool dense = p.out_mul == 1 && c_h0 == 0 && c_w0 == 0 && c_Wg == p.Wo && c_Hg == p.Ho;
    if (p.accumulate && !acc_done) {          // fold the previous contents of C into the accumulators (register layout, 8-byte loads)
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const int m = m0 + wp * (BM / WP) + j * 16 + lrow;
            if (m < c_M) {
                const T* src = Cg + (dense ? (size_t)m : pixel_of(m)) * p.ldc;
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const int co = n0 + wc * BNW + c * 16 + lgrp * 4;
                    if (co < p.Cst) {          // Cst % 8 == 0: a 4-channel group is inside or outside
                        const uint2 q2 = *(const uint2*)(src + co);
                        acc[c][j] += f32x4{__uint_as_float(q2.x << 16), __uint_as_float(q2.x & 0xffff0000u),
                                           __uint_as_float(q2.y << 16), __uint_as_float(q2.y & 0xffff0000u)};
                    }
                }
            }
        }
    }
    // ---- BN partial statistics (before the transpose: the scratch is free, and the sums leave their registers at once).  Plain
    // per-channel (sum, sum of squares) of the tile in f32: per lane over its PT pixels, over the 16 pixel lanes of a row group by DPP
    // row rotations (one v_add_f32_dpp each, no LDS round trips), over the pixel waves through LDS.  Throughput mode adds them to the
    // replica rows with f32 atomics; the partial-row contract (deterministic mode) gets (sum, M2 = sum of squares - sum^2 / n) of the
    // block — over at most BM = 128 bf16-precision values the cancellation costs (1 + mean^2 / var) x 1e-7 relative, far below the
    // storage precision of this (bf16-only) kernel family.  The block-local (mean, M2) Chan merge this replaces (34 ds_bpermute round
    // trips and ~250 VALU instructions behind the main loop of every tile) cost 7..18 % of the forward time of the ring layers.
    if (STATS && p.stats != nullptr) {
        float* sred = (float*)smem;                    // [WP][BN][2]
        auto row_sum = [](float v) {
            v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false));     // row_ror:8
            v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xf, 0xf, false));     // row_ror:4
            v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122, 0xf, 0xf, false));     // row_ror:2
            v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xf, 0xf, false));     // row_ror:1
            return v;
        };
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            float a[4], b[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a[e] = 0.f; b[e] = 0.f;
#pragma unroll
                for (int j = 0; j < PT; ++j) { const float v = acc[c][j][e]; a[e] += v; b[e] += v * v; }    // rows beyond M are exact zeros
                a[e] = row_sum(a[e]);
                b[e] = row_sum(b[e]);
            }
            if (lrow == 0) {
                const int ch = wc * BNW + c * 16 + lgrp * 4;
                *(float4*)(sred + (wp * BN + ch) * 2) = make_float4(a[0], b[0], a[1], b[1]);
                *(float4*)(sred + (wp * BN + ch) * 2 + 4) = make_float4(a[2], b[2], a[3], b[3]);
            }
            __builtin_amdgcn_sched_barrier(0);         // one channel group at a time: eight reduction chains, not thirty-two
        }
        __syncthreads();
        if (t < BN && n0 + t < p.Cout) {
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int w = 0; w < WP; ++w) { const float2 v = *(const float2*)(sred + (w * BN + t) * 2); a += v.x; b += v.y; }
            if (p.stats_atomic) {
                float* dst = p.stats + (size_t)(mtile & (YDL_BN_REPLICAS - 1)) * 2 * p.stats_ld;
                atomicAdd(dst + n0 + t, a);
                atomicAdd(dst + p.stats_ld + n0 + t, b);
            } else {
                const float nvalid = (float)min(BM, c_M - m0);
                float* dst = p.stats + (size_t)mtile * 2 * p.stats_ld;
                dst[n0 + t] = a;
                dst[p.stats_ld + n0 + t] = fmaxf(b - a * a / nvalid, 0.f);
            }
        }
        __syncthreads();                               // the sums have been read: the transposed tile may overwrite them
    }
    // ---- transpose through LDS
#pragma unroll
    for (int j = 0; j < PT; ++j) {
        const int row = wp * (BM / WP) + j * 16 + lrow;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int ch = wc * BNW + c * 16 + lgrp * 4;          // first of 4 channels
            uint2 u;
            u.x = (uint32_t)f2bf(acc[c][j][0]) | ((uint32_t)f2bf(acc[c][j][1]) << 16);
            u.y = (uint32_t)f2bf(acc[c][j][2]) | ((uint32_t)f2bf(acc[c][j][3]) << 16);
            const int chunk = (ch >> 3) ^ (row & (CPR - 1) & 15);
            *(uint2*)(smem + row * ORB + (chunk << 4) + ((ch & 4) << 1)) = u;
        }
    }
    __syncthreads();
    {
        const int cq = t % CPR, r0 = t / CPR;
        const int co = n0 + cq * 8;
        // fused BatchNorm-backward reduce (ydl_conv_dgrad_bnred): this thread's 8 channels belong to one producer segment; the stored
        // (bf16-rounded) gradient is what the stand-alone reduce pass would read
        const bool br_on = RED && p.br.nseg > 0;       // RED instantiations only: the reduce costs registers the plain kernels must not pay
        if (!br_on) {
#pragma unroll
            for (int i = 0; i < BM / RPS; ++i) {
                const int row = r0 + i * RPS;
                const int m = m0 + row;
                if (m < c_M && co < p.Cst) {
                    const uint4 v = *(const uint4*)(smem + row * ORB + ((cq ^ (row & (CPR - 1) & 15)) << 4));
                    *(uint4*)(Cg + (dense ? (size_t)m : pixel_of(m)) * p.ldc + co) = v;
                }
            }
        }
        float sb[8], sg[8];
        if (br_on) {
            bool br_live = false;
            const T* by = nullptr;
            int bldy = 0;
            bool bsilu = false;
            {
                const int sgm = (p.br.nseg > 1 && co >= p.br.c0[1]) ? 1 : 0;
                br_live = co >= p.br.c0[sgm] && co < p.br.c1[sgm];
                if (br_live) {
                    by = (const T*)p.br.y[sgm] + (co - p.br.c0[sgm]);
                    bldy = p.br.ldy[sgm];
                    bsilu = p.br.act[sgm] == YDL_ACT_SILU;
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) { sb[e] = 0.f; sg[e] = 0.f; }
            // all of the thread's y rows are requested before the first is used (one memory round trip, not one per row)
            int pixs[BM / RPS];                            // (< 2^31 pixels: check_geom)
            uint4 yq[BM / RPS];
#pragma unroll
            for (int i = 0; i < BM / RPS; ++i) {
                const int m = m0 + r0 + i * RPS;
                const bool ok = m < c_M && co < p.Cst;
                pixs[i] = ok ? (dense ? m : (int)pixel_of(m)) : 0;
                yq[i] = (ok && br_live) ? *(const uint4*)(by + (size_t)pixs[i] * bldy) : make_uint4(0, 0, 0, 0);
            }
            const float* cfp = scoef + cq * 32;            // this thread's 8 channels x (scale, shift, mean, invstd)
#pragma unroll
            for (int i = 0; i < BM / RPS; ++i) {
                const int row = r0 + i * RPS;
                const int m = m0 + row;
                if (m < c_M && co < p.Cst) {
                    const uint4 v = *(const uint4*)(smem + row * ORB + ((cq ^ (row & (CPR - 1) & 15)) << 4));
                    *(uint4*)(Cg + (size_t)pixs[i] * p.ldc + co) = v;
                    if (br_live) {
                        float yv[8], dz[8];
                        unpack16<T>(yq[i], yv);
                        unpack16<T>(v, dz);
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const float4 c4 = *(const float4*)(cfp + e * 4);
                            if (bsilu) {
                                const float zz = yv[e] * c4.x + c4.y;
                                const float sgd = sigmoid_f(zz);
                                dz[e] *= sgd * (1.f + zz * (1.f - sgd));
                            }
                            sb[e] += dz[e];
                            sg[e] += dz[e] * ((yv[e] - c4.z) * c4.w);
                        }
                    }
                }
            }
        }
        if (br_on) {
            // lanes of a wave that share the channel chunk, then the NW waves through the (now free) scratch, then one add per channel
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int o = CPR; o < 64; o <<= 1) { sb[e] += __shfl_xor(sb[e], o, 64); sg[e] += __shfl_xor(sg[e], o, 64); }
            __syncthreads();                               // every thread has read its part of the transposed tile
            float* sred = (float*)smem;                    // [NW][BN][2]
            if (lane < CPR) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    sred[((wave * BN) + cq * 8 + e) * 2] = sb[e];
                    sred[((wave * BN) + cq * 8 + e) * 2 + 1] = sg[e];
                }
            }
            __syncthreads();
            if (t < BN) {
                const int c = n0 + t;
                const int sgm = (p.br.nseg > 1 && c >= p.br.c0[1]) ? 1 : 0;
                if (c >= p.br.c0[sgm] && c < p.br.c1[sgm]) {
                    float a = 0.f, b = 0.f;
#pragma unroll
                    for (int w = 0; w < NW; ++w) { a += sred[(w * BN + t) * 2]; b += sred[(w * BN + t) * 2 + 1]; }
                    float* dst = p.br.sums[sgm] + (size_t)(mtile & (YDL_BN_REPLICAS - 1)) * 2 * p.br.cp[sgm];
                    atomicAdd(dst + (c - p.br.c0[sgm]), a);
                    atomicAdd(dst + p.br.cp[sgm] + (c - p.br.c0[sgm]), b);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// igemm2: the same implicit GEMM with an ASYNCHRONOUS operand pipeline (bf16 throughput mode, Cin a multiple of 64).
// Both tiles go global -> LDS by LDS-DMA (`buffer_load_dwordx4 ... lds`: no staging VGPRs, no ds_write pass) into a ring
// of S stages; a K-step waits only for ITS stage with a counted `s_waitcnt vmcnt`, so S-2 younger K-steps stay in flight
// across the single `s_barrier` of the step.  One wave-instruction writes 1 KiB = 8 tile rows x 128 B at (wave-uniform
// M0 base) + lane*16, which is exactly the row-major image of igemm_kernel; the XOR swizzle of the 16-byte chunks moves
// to the per-lane SOURCE address (the lane at slot qs of row r fetches logical chunk qs ^ ((r>>1)&7)), the fragment reads
// are unchanged.  Padding taps, tail rows and the K-steps issued beyond the end are out-of-range buffer offsets, for which
// the DMA writes zeros (tools/lds_dma_probe.hip checks that on the hardware).
// With Cin % 64 == 0 every 64-deep K-step lies inside ONE tap, so the tap of a step is wave-uniform: per row the loader
// keeps a bit mask of its valid taps (computed once), a step costs one v_add3 + and/cmp/select per row.
// The DMAs are issued from inline asm: the compiler's own wait-count insertion treats an LDS-DMA as a pending LDS write
// and would drain vmcnt to 0 in front of every fragment read.  Per K-step and wave:
//     s_waitcnt vmcnt(L*(S-2))  own DMAs of step k have landed (S-2 younger steps stay in flight)
//     s_barrier                 everyone's have; every wave has finished reading step k-1
//     issue DMAs of step k+S-1  into the stage step k-1 occupied
//     fragment reads + MFMAs of step k
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void lds_dma16(const u32x4& rsrc, unsigned lds_addr, unsigned voff) {
    // M0 = LDS byte address of the wave's 1 KiB destination (wave-uniform); written in the statement that uses it
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lds_addr), "v"(voff), "s"(rsrc)
                 : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vm_barrier() {
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}

// STG (round 5): the eight waves of the CTA as two HALVES that run half a K-step apart.  Waves i and i + 4 share a SIMD; in the
// plain form both reach their fragment reads, their DMA issue and their MFMAs together, so the matrix pipe idles while both load and
// both queue for it afterwards.  Here waves 0-3 run   barrier_k | read(k) | issue | MFMA(k)          and waves 4-7 run
// barrier_k | MFMA(k-1) | issue | read(k)   — the younger half keeps a whole K-step of fragments in registers across the barrier and
// computes it while the older half loads: on every SIMD one wave is in its matrix segment while its partner is in its LDS / DMA
// segment.  Same barrier count, same DMA count per thread and step (the counted vmcnt is unchanged), results bit-identical.
template <int BM, int BN, int NW, int WP, int S, bool RED = false, int STG = 0>
__global__ __launch_bounds__(NW * 64, RED ? NW / 2 : 1) void igemm2_kernel(const IgemmArgs p) {
    using T = bf16_t;
    constexpr int ES = 2;
    constexpr int RPP = NW * 8;                 // tile rows covered by one DMA pass of the CTA (one wave = 8 rows)
    static_assert(BM % RPP == 0 && BN % RPP == 0, "tile rows must be a multiple of the rows one pass covers");
    constexpr int AR = BM / RPP, BR = BN / RPP;
    constexpr int L = AR + BR;                  // DMAs per thread per K-step
    constexpr int WN = NW / WP;
    constexpr int BNW = BN / WN;
    constexpr int CT = BNW / 16;
    constexpr int PT = BM / (16 * WP);
    constexpr int STAGE = (BM + BN) * GROWB;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int* sTapA = (int*)(smem + S * STAGE);
    int* sTapB = sTapA + MAXTAPS;
    int* sTapD = sTapB + MAXTAPS;

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wc = wave % WN, wp = wave / WN;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    int mtile, ntile;
    if (p.m_fastest) { ntile = tile / p.grid_m; mtile = tile - ntile * p.grid_m; }
    else { mtile = tile / p.grid_n; ntile = tile - mtile * p.grid_n; }
    int c_ntaps = p.ntaps, c_tap0 = 0, c_Hg = p.Hg, c_Wg = p.Wg, c_M = p.M, c_h0 = p.out_h0, c_w0 = p.out_w0;
    if (p.ncls > 1) {
        int c = 0;
        while (c + 1 < p.ncls && mtile >= p.cls_tile0[c + 1]) ++c;
        mtile -= p.cls_tile0[c];
        c_ntaps = p.cls_ntaps[c]; c_tap0 = p.cls_tap0[c]; c_Hg = p.cls_Hg[c]; c_Wg = p.cls_Wg[c]; c_M = p.cls_M[c];
        c_h0 = p.cls_h0[c]; c_w0 = p.cls_w0[c];
    }
    const int m0 = mtile * BM;
    const int n0 = ntile * BN;
    if (t < MAXTAPS) {
        int da = 0, db = 0, dd = 0;
        if (t < c_ntaps) {
            da = ((int)p.dh[c_tap0 + t] * p.Wi + (int)p.dw[c_tap0 + t]) * p.lda * ES;
            db = (int)p.wt[c_tap0 + t] * p.Kc * ES;
            dd = ((int)p.dh[c_tap0 + t] & 0xffff) | ((int)p.dw[c_tap0 + t] << 16);
        }
        sTapA[t] = da;
        sTapB[t] = db;
        sTapD[t] = dd;
    }
    float* const sCoef = (float*)(sTapD + MAXTAPS);      // RED: [BN][4] BatchNorm coefficients of this tile's channels
    if constexpr (RED) br_fill_coef<BN>(p, sCoef, n0, t);
    __syncthreads();   // tap tables visible (no DMA is in flight yet)

    // this thread's DMA slot: row r of each pass, 16-byte slot qs; it fetches the logical chunk q = qs ^ swizzle(r)
    const int r = t >> 3;
    const int qs = t & 7;
    const unsigned q16 = (unsigned)((qs ^ ((r >> 1) & 7)) << 4);
    unsigned rowoff[AR], vmask[AR];
    {
        int ih0[AR], iw0[AR];
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int m = m0 + r + RPP * i;
            rowoff[i] = 0;
            vmask[i] = 0;
            ih0[i] = -100000;          // tail rows: no tap is valid => zeros
            iw0[i] = 0;
            if (m < c_M) {
                const int gw = m % c_Wg;
                const int tmp = m / c_Wg;
                const int gh = tmp % c_Hg;
                const int n = tmp / c_Hg;
                ih0[i] = gh * p.in_mul;
                iw0[i] = gw * p.in_mul;
                rowoff[i] = (unsigned)(((n * p.Hi + ih0[i]) * p.Wi + iw0[i]) * p.lda) * (unsigned)ES + q16;
            }
        }
        for (int tp = 0; tp < c_ntaps; ++tp) {            // uniform loop, broadcast LDS reads
            const int dd = sTapD[tp];
            const int dh = (int)(short)(dd & 0xffff), dw = dd >> 16;
#pragma unroll
            for (int i = 0; i < AR; ++i) {
                const bool ok = (unsigned)(ih0[i] + dh) < (unsigned)p.Hi && (unsigned)(iw0[i] + dw) < (unsigned)p.Wi;
                vmask[i] |= ok ? (1u << tp) : 0u;
            }
        }
    }
    unsigned browoff[BR];
#pragma unroll
    for (int i = 0; i < BR; ++i) {
        const int co = n0 + r + RPP * i;
        // rows beyond Cout: a poisoned offset stays out of range whatever is added to it
        browoff[i] = co < p.Cout ? (unsigned)co * p.ldb_bytes + q16 : 0xF0000000u;
    }
    const int spt = p.Kc >> 6;                  // 64-channel blocks (Kc % 64 == 0)
    const int nk = c_ntaps * spt;
    u32x4 rsA, rsB;
    {
        const unsigned long long pa = (unsigned long long)p.A, pb = (unsigned long long)p.B;
        rsA = u32x4{(unsigned)pa, (unsigned)(pa >> 32) & 0xffffu, p.bytesA, 0x00020000u};
        rsB = u32x4{(unsigned)pb, (unsigned)(pb >> 32) & 0xffffu, p.bytesB, 0x00020000u};
    }
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned wave_lds = lds0 + (unsigned)wave * (8 * GROWB);

    // K order: 64-channel block outer, tap inner.  All taps of one channel block touch the same input lines (the tile's
    // halo), so they hit in L2 when they follow each other; tap-outer order re-fetched the whole input tile per tap from
    // beyond L2 (the reuse distance was the whole K loop) and left the kernel bound by the ~6 TB/s of L2-miss traffic.
    // Position of the NEXT step to issue (uniform); its table entries are prefetched one step ahead (off the issue path).
    int tap = 0, cb = 0;
    int nxtA = sTapA[0], nxtB = sTapB[0];
    auto issue = [&](int stg) {
        const int da = nxtA, db = nxtB;
        const bool live = cb < spt;                                // steps beyond the end: every lane out of range
        const unsigned kb = (unsigned)cb << 7;                      // byte offset of the channel block
        const unsigned tbit = live ? 1u << tap : 0u;
        const unsigned kbB = live ? kb : 0xF0000000u;
        if (++tap == c_ntaps) { tap = 0; ++cb; }
        nxtA = sTapA[tap];
        nxtB = sTapB[tap];
        const unsigned base = wave_lds + (unsigned)stg * STAGE;
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const unsigned off = (vmask[i] & tbit) ? rowoff[i] + (unsigned)da + kb : 0xFFFFFFFFu;
            lds_dma16(rsA, base + i * RPP * GROWB, off);
        }
#pragma unroll
        for (int i = 0; i < BR; ++i) lds_dma16(rsB, base + BM * GROWB + i * RPP * GROWB, browoff[i] + (unsigned)db + kbB);
    };

    f32x4 acc[CT][PT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int j = 0; j < PT; ++j) acc[c][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int u = 0; u < S - 1; ++u) issue(u);      // steps beyond nk are all-zero DMAs: the vmcnt arithmetic stays uniform

    const int lrow = lane & 15;
    const int sw_rd = (lrow >> 1) & 7;
    const int lk0 = (((lane >> 4)) ^ sw_rd) << 4;
    const int lk1 = (((lane >> 4) + 4) ^ sw_rd) << 4;
    const unsigned char* const fa = smem + BM * GROWB + (wc * BNW + lrow) * GROWB;     // weights  (MFMA A operand)
    const unsigned char* const fb = smem + (wp * (BM / WP) + lrow) * GROWB;             // pixels   (MFMA B operand)
    // Software-pipelined fragment reads: the fragments of half-step h+1 are in flight while the 16*... MFMAs of half-step h
    // issue (two register sets).  The wait + barrier that opens step k+1 sits between the two MFMA batches of step k:
    //   read F1 = frags(k, half 1) | MFMA(F0) | lgkmcnt(0), vmcnt, barrier | issue DMAs(k+S) | read F0 = frags(k+1, half 0) | MFMA(F1)
    // (by then every wave holds all of step k's fragments in registers, so the DMAs of step k+S may overwrite its stage)
    uint4 af0[CT], bf0[PT], af1[CT], bf1[PT];
    auto rdfrag = [&](int stg, int half, uint4 (&af)[CT], uint4 (&bfr)[PT]) {
        const unsigned char* a_base = fa + stg * STAGE + (half ? lk1 : lk0);
        const unsigned char* b_base = fb + stg * STAGE + (half ? lk1 : lk0);
#pragma unroll
        for (int c = 0; c < CT; ++c) af[c] = *(const uint4*)(a_base + c * 16 * GROWB);
#pragma unroll
        for (int j = 0; j < PT; ++j) bfr[j] = *(const uint4*)(b_base + j * 16 * GROWB);
    };
    auto mma = [&](const uint4 (&af)[CT], const uint4 (&bfr)[PT]) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int j = 0; j < PT; ++j) Mma<T>::run(af[c], bfr[j], acc[c][j]);
    };
    if constexpr (STG != 0) {
        static_assert(NW == 8, "the stagger splits the CTA into waves 0-3 and 4-7");
        auto rd_step = [&](int stg) { rdfrag(stg, 0, af0, bf0); rdfrag(stg, 1, af1, bf1); };
        auto mma_step = [&]() { mma(af0, bf0); mma(af1, bf1); };
        if (wave < NW / 2) {
            int stg = 0;
            for (int kk = 0; kk < nk; ++kk) {
                wait_vm_barrier<L * (S - 2)>();                // step kk landed everywhere; every wave holds step kk-1 in registers
                rd_step(stg);
                __builtin_amdgcn_sched_barrier(0);
                issue(stg == 0 ? S - 1 : stg - 1);             // step kk+S-1 -> the stage step kk-1 occupied
                __builtin_amdgcn_sched_barrier(0);
                mma_step();
                __builtin_amdgcn_sched_barrier(0);
                stg = stg + 1 == S ? 0 : stg + 1;
            }
        } else if (nk > 0) {
            wait_vm_barrier<L * (S - 2)>();
            issue(S - 1);
            rd_step(0);
            int stg = 1 % S;
            for (int kk = 1; kk < nk; ++kk) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // step kk-1 is in registers: its stage may be overwritten
                wait_vm_barrier<L * (S - 2)>();
                mma_step();                                             // step kk-1, while waves 0-3 read step kk
                __builtin_amdgcn_sched_barrier(0);
                issue(stg == 0 ? S - 1 : stg - 1);
                __builtin_amdgcn_sched_barrier(0);
                rd_step(stg);
                __builtin_amdgcn_sched_barrier(0);
                stg = stg + 1 == S ? 0 : stg + 1;
            }
            mma_step();
        }
    } else {
    if (nk > 0) {
        wait_vm_barrier<L * (S - 2)>();            // step 0 landed everywhere
        issue(S - 1);
        rdfrag(0, 0, af0, bf0);
    }
    for (int kk0 = 0; kk0 < nk; kk0 += S) {
#pragma unroll
        for (int u = 0; u < S; ++u) {
            const int kk = kk0 + u;
            if (kk < nk) {
                rdfrag(u, 1, af1, bf1);
                mma(af0, bf0);
                if (kk + 1 < nk) {
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave holds all of step kk in registers
                    wait_vm_barrier<L * (S - 2)>();                         // step kk+1 landed everywhere
                    issue(u);                                               // step kk+S -> the stage step kk occupied
                    rdfrag((u + 1) % S, 0, af0, bf0);
                }
                mma(af1, bf1);
            }
        }
    }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wait_vm_barrier<0>();              // the trailing all-zero DMAs must land before the epilogue reuses the LDS
    igemm2_epilogue<BM, BN, NW, WP, RED>(p, acc, smem, m0, n0, mtile, c_M, c_Wg, c_Hg, c_h0, c_w0, sCoef);
}

// ------------------------------------------------------------------------------------------------------
// igemm2l: the ring kernel with LOADER WAVES (round 5; the weight gradient's wgrad3s_kernel has the measurements that led here).
// In igemm2_kernel every wave issues its share of the step's DMAs and then multiplies; the no-DMA / no-MFMA ablations each remove
// 35-40 % of the time — the two phases ADD: a wave held at its LDS-DMA instructions by a full memory pipeline cannot issue MFMAs.
// Here NW multiplier waves (waves 0 .. NW-1: fragment reads + MFMAs, no vector-memory instruction in their loop, then the epilogue) and
// NL loader waves (waves NW ..: tap tables, row descriptors, every DMA of the ring, the counted waits) share ONE s_barrier per K-step:
//     loaders:      s_waitcnt vmcnt (step k landed) | s_barrier | issue step k+S-1 into the stage step k-1 occupied
//     multipliers:  ... MFMA(k-1, second half) | lgkmcnt(0) | s_barrier | read(k) | MFMA(k) ...     (software-pipelined as in igemm2)
// A DMA instruction writes 8 tile rows x 128 B; loader wave lw owns instruction slots j = lw, lw + NL, ... of the A rows and of the B
// rows, so a lane's rows are 8 j + (lane >> 3): with NL even the swizzle term ((row >> 1) & 7) is the same for all of a lane's slots.
// The loaders return before the epilogue (s_barrier counts the surviving waves only).
// ------------------------------------------------------------------------------------------------------
template <int BM, int BN, int NW, int WP, int S, int NL>
__global__ __launch_bounds__((NW + NL) * 64, S == 2 ? (NW + NL) / 2 : 1) void igemm2l_kernel(const IgemmArgs p) {      // (2nd argument: waves per SIMD — two CTAs per CU for the two-stage forms)
    using T = bf16_t;
    constexpr int ES = 2;
    constexpr int NAI = BM / 8, NBI = BN / 8;          // DMA instructions per K-step: activation rows, weight rows
    static_assert(NAI % NL == 0 && NBI % NL == 0 && NL % 2 == 0 && S >= 2, "every loader wave issues the same number of DMAs per step");
    constexpr int APL = NAI / NL, BPL = NBI / NL, LPL = APL + BPL;
    constexpr int WN = NW / WP;
    constexpr int BNW = BN / WN;
    constexpr int CT = BNW / 16;
    constexpr int PT = BM / (16 * WP);
    constexpr int STAGE = (BM + BN) * GROWB;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int* sTapA = (int*)(smem + S * STAGE);
    int* sTapB = sTapA + MAXTAPS;
    int* sTapD = sTapB + MAXTAPS;

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    int mtile, ntile;
    if (p.m_fastest) { ntile = tile / p.grid_m; mtile = tile - ntile * p.grid_m; }
    else { mtile = tile / p.grid_n; ntile = tile - mtile * p.grid_n; }
    int c_ntaps = p.ntaps, c_tap0 = 0, c_Hg = p.Hg, c_Wg = p.Wg, c_M = p.M, c_h0 = p.out_h0, c_w0 = p.out_w0;
    if (p.ncls > 1) {
        int c = 0;
        while (c + 1 < p.ncls && mtile >= p.cls_tile0[c + 1]) ++c;
        mtile -= p.cls_tile0[c];
        c_ntaps = p.cls_ntaps[c]; c_tap0 = p.cls_tap0[c]; c_Hg = p.cls_Hg[c]; c_Wg = p.cls_Wg[c]; c_M = p.cls_M[c];
        c_h0 = p.cls_h0[c]; c_w0 = p.cls_w0[c];
    }
    const int m0 = mtile * BM;
    const int n0 = ntile * BN;
    if (t < MAXTAPS) {
        int da = 0, db = 0, dd = 0;
        if (t < c_ntaps) {
            da = ((int)p.dh[c_tap0 + t] * p.Wi + (int)p.dw[c_tap0 + t]) * p.lda * ES;
            db = (int)p.wt[c_tap0 + t] * p.Kc * ES;
            dd = ((int)p.dh[c_tap0 + t] & 0xffff) | ((int)p.dw[c_tap0 + t] << 16);
        }
        sTapA[t] = da;
        sTapB[t] = db;
        sTapD[t] = dd;
    }
    __syncthreads();   // tap tables visible (no DMA is in flight yet)
    const int spt = p.Kc >> 6;
    const int nk = c_ntaps * spt;

    if (wave >= NW) {
        // ---------------- loader waves
        const int lw = wave - NW;
        const int r8 = lane >> 3, qs = lane & 7;
        const unsigned q16 = (unsigned)((qs ^ (((r8 >> 1) | ((lw & 1) << 2)) & 7)) << 4);      // (row >> 1) & 7 with row = 8 j + r8, j = lw (mod 2)
        unsigned rowoff[APL], vmask[APL];
        {
            int ih0[APL], iw0[APL];
#pragma unroll
            for (int i = 0; i < APL; ++i) {
                const int m = m0 + (lw + NL * i) * 8 + r8;
                rowoff[i] = 0;
                vmask[i] = 0;
                ih0[i] = -100000;          // tail rows: no tap is valid => zeros
                iw0[i] = 0;
                if (m < c_M) {
                    const int gw = m % c_Wg;
                    const int tmp = m / c_Wg;
                    const int gh = tmp % c_Hg;
                    const int n = tmp / c_Hg;
                    ih0[i] = gh * p.in_mul;
                    iw0[i] = gw * p.in_mul;
                    rowoff[i] = (unsigned)(((n * p.Hi + ih0[i]) * p.Wi + iw0[i]) * p.lda) * (unsigned)ES + q16;
                }
            }
            for (int tp = 0; tp < c_ntaps; ++tp) {            // uniform loop, broadcast LDS reads
                const int dd = sTapD[tp];
                const int dh = (int)(short)(dd & 0xffff), dw = dd >> 16;
#pragma unroll
                for (int i = 0; i < APL; ++i) {
                    const bool ok = (unsigned)(ih0[i] + dh) < (unsigned)p.Hi && (unsigned)(iw0[i] + dw) < (unsigned)p.Wi;
                    vmask[i] |= ok ? (1u << tp) : 0u;
                }
            }
        }
        unsigned browoff[BPL];
#pragma unroll
        for (int i = 0; i < BPL; ++i) {
            const int co = n0 + (lw + NL * i) * 8 + r8;
            browoff[i] = co < p.Cout ? (unsigned)co * p.ldb_bytes + q16 : 0xF0000000u;
        }
        u32x4 rsA, rsB;
        {
            const unsigned long long pa = (unsigned long long)p.A, pb = (unsigned long long)p.B;
            rsA = u32x4{(unsigned)pa, (unsigned)(pa >> 32) & 0xffffu, p.bytesA, 0x00020000u};
            rsB = u32x4{(unsigned)pb, (unsigned)(pb >> 32) & 0xffffu, p.bytesB, 0x00020000u};
        }
        const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
        const unsigned wave_lds = lds0 + (unsigned)lw * (8 * GROWB);
        int tap = 0, cb = 0;
        int nxtA = sTapA[0], nxtB = sTapB[0];
        auto issue = [&](int stg) {
            const int da = nxtA, db = nxtB;
            const bool live = cb < spt;                                // steps beyond the end: every lane out of range
            const unsigned kb = (unsigned)cb << 7;
            const unsigned tbit = live ? 1u << tap : 0u;
            const unsigned kbB = live ? kb : 0xF0000000u;
            if (++tap == c_ntaps) { tap = 0; ++cb; }
            nxtA = sTapA[tap];
            nxtB = sTapB[tap];
            const unsigned base = wave_lds + (unsigned)stg * STAGE;
#pragma unroll
            for (int i = 0; i < APL; ++i)
                lds_dma16(rsA, base + (unsigned)(NL * i) * (8 * GROWB), (vmask[i] & tbit) ? rowoff[i] + (unsigned)da + kb : 0xFFFFFFFFu);
#pragma unroll
            for (int i = 0; i < BPL; ++i)
                lds_dma16(rsB, base + BM * GROWB + (unsigned)(NL * i) * (8 * GROWB), browoff[i] + (unsigned)db + kbB);
        };
#pragma unroll
        for (int u = 0; u < S - 1; ++u) issue(u);
        int nxt = S - 1;
        for (int kk = 0; kk < nk; ++kk) {
            wait_vm_barrier<LPL * (S - 2)>();          // this wave's DMAs of step kk have landed; the multipliers hold step kk-1 in registers
            issue(nxt);                                // step kk+S-1 -> the stage step kk-1 occupied
            nxt = nxt + 1 == S ? 0 : nxt + 1;
        }
        wait_vm_barrier<0>();                          // the trailing all-zero DMAs have landed: the epilogue may reuse the LDS
        return;
    }

    // ---------------- multiplier waves
    const int wc = wave % WN, wp = wave / WN;
    f32x4 acc[CT][PT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int j = 0; j < PT; ++j) acc[c][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int lrow = lane & 15;
    const int sw_rd = (lrow >> 1) & 7;
    const int lk0 = (((lane >> 4)) ^ sw_rd) << 4;
    const int lk1 = (((lane >> 4) + 4) ^ sw_rd) << 4;
    const unsigned char* const fa = smem + BM * GROWB + (wc * BNW + lrow) * GROWB;     // weights  (MFMA A operand)
    const unsigned char* const fb = smem + (wp * (BM / WP) + lrow) * GROWB;             // pixels   (MFMA B operand)
    uint4 af0[CT], bf0[PT], af1[CT], bf1[PT];
    auto rdfrag = [&](int stg, int half, uint4 (&af)[CT], uint4 (&bfr)[PT]) {
        const unsigned char* a_base = fa + stg * STAGE + (half ? lk1 : lk0);
        const unsigned char* b_base = fb + stg * STAGE + (half ? lk1 : lk0);
#pragma unroll
        for (int c = 0; c < CT; ++c) af[c] = *(const uint4*)(a_base + c * 16 * GROWB);
#pragma unroll
        for (int j = 0; j < PT; ++j) bfr[j] = *(const uint4*)(b_base + j * 16 * GROWB);
    };
    auto mma = [&](const uint4 (&af)[CT], const uint4 (&bfr)[PT]) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int j = 0; j < PT; ++j) Mma<T>::run(af[c], bfr[j], acc[c][j]);
    };
    // barrier count: one per K-step (opening it) + the closing one — the same nk + 1 the loaders execute
    constexpr bool PIPE = NW >= 8;     // 64 x 64 wave tiles of a 4-wave CTA: ONE fragment set (the second costs 32 registers the two-CTA form lacks)
    if constexpr (PIPE) {
        if (nk > 0) {
            asm volatile("s_barrier" ::: "memory");            // step 0 landed everywhere
            rdfrag(0, 0, af0, bf0);
        }
        int stg = 0;
        for (int kk = 0; kk < nk; ++kk) {
            rdfrag(stg, 1, af1, bf1);
            mma(af0, bf0);
            stg = stg + 1 == S ? 0 : stg + 1;
            if (kk + 1 < nk) {
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // this wave holds all of step kk; step kk+1 landed everywhere
                rdfrag(stg, 0, af0, bf0);
            }
            mma(af1, bf1);
        }
    } else {
        int stg = 0;
        for (int kk = 0; kk < nk; ++kk) {
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");          // step kk landed everywhere; this wave is done reading step kk-1
            rdfrag(stg, 0, af0, bf0);
            mma(af0, bf0);
            rdfrag(stg, 1, af0, bf0);
            mma(af0, bf0);
            stg = stg + 1 == S ? 0 : stg + 1;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");              // (pairs with the loaders' closing barrier)
    igemm2_epilogue<BM, BN, NW, WP, false>(p, acc, smem, m0, n0, mtile, c_M, c_Wg, c_Hg, c_h0, c_w0, nullptr);
}

template <int BM, int BN, int NW, int WP, int S, int NL>
static int launch_igemm2l(IgemmArgs a, hipStream_t st, int fam) {
    a.grid_n = (a.Cst + BN - 1) / BN;
    int mtiles = (a.M + BM - 1) / BM;
    if (a.ncls > 1) {
        int acc = 0;
        for (int c = 0; c < a.ncls; ++c) { a.cls_tile0[c] = acc; acc += (a.cls_M[c] + BM - 1) / BM; }
        a.cls_tile0[a.ncls] = acc;
        mtiles = acc;
    }
    a.grid_m = mtiles;
    YDL_CHECK(a.bytesB < 0x08000000u, "ring kernel: weight matrix of 128 MiB or more is not supported");
    {
        const double wbytes = (double)a.Cout * a.Ttot * a.Kc * 2.0;
        const double abytes = (double)a.N * a.Hi * a.Wi * a.lda * 2.0;
        a.m_fastest = (wbytes > 2.0e6 && (double)mtiles * wbytes > (double)a.grid_n * abytes) ? 1 : 0;
    }
    const size_t smem = (size_t)S * (BM + BN) * GROWB + 3 * MAXTAPS * sizeof(int);
    static const std::string nm = std::string("igemm2l_kernel<") + std::to_string(BM) + "," + std::to_string(BN) + "," + std::to_string(NW) + "+" +
                                  std::to_string(NL) + "," + std::to_string(S) + ">";
    YDL_SET_MAX_LDS((igemm2l_kernel<BM, BN, NW, WP, S, NL>), smem);
    ydl_note_kernel(fam, nm.c_str());
    igemm2l_kernel<BM, BN, NW, WP, S, NL><<<dim3(mtiles * a.grid_n), (NW + NL) * 64, smem, st>>>(a);
    YDL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// igemm2p: the two-stage ring kernel as a PERSISTENT CTA that walks several output tiles, with the ring running across tile
// boundaries.  In igemm2_kernel a tile costs t0 + n_k t1 with t0 (tap tables, row decode, the first DMA round trip, the epilogue's
// LDS transpose, stores and statistics) as large as six K-steps; the step issued beyond a tile's last K-step was an all-zero dummy.
// Here that slot carries the NEXT tile's first K-step: it is in flight while the current tile's last MFMAs and its whole epilogue
// run, the epilogue uses the ring stage the last K-step just vacated as its scratch (a 128x128 bf16 tile is exactly one stage),
// and the next tile's row descriptors are computed at the start of the current tile, under its first DMA wait.
// Per K-step nothing changes: lgkmcnt(0), vmcnt(0) + s_barrier, issue the step after next, fragments, MFMAs (two stages:
// the counted wait is vmcnt(0) anyway, so the epilogue's stores and atomics need no counting).  The stage of a tile's step 0 is
// whatever parity the previous tile ended on (runtime parity, n_k may be odd).
// Tile order: linear index = blockIdx.x + j * gridDim.x, mapped through xcd_remap over ALL tiles: with a grid that is a multiple
// of 8 a CTA keeps drawing from its own XCD's contiguous tile range.
// ------------------------------------------------------------------------------------------------------
template <int BM, int BN, int NW, int WP, bool RED = false>
__global__ __launch_bounds__(NW * 64, NW / 2) void igemm2p_kernel(const IgemmArgs p) {
    using T = bf16_t;
    constexpr int ES = 2;
    constexpr int S = 2;
    constexpr int RPP = NW * 8;
    static_assert(BM % RPP == 0 && BN % RPP == 0, "tile rows must be a multiple of the rows one pass covers");
    constexpr int AR = BM / RPP, BR = BN / RPP;
    constexpr int WN = NW / WP;
    constexpr int BNW = BN / WN;
    constexpr int CT = BNW / 16;
    constexpr int PT = BM / (16 * WP);
    constexpr int STAGE = (BM + BN) * GROWB;
    static_assert(STAGE >= BM * BN * 2 && STAGE >= WP * BN * 8 + 64, "a stage must hold the epilogue's transposed tile and its statistics scratch");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int* sTapA = (int*)(smem + S * STAGE);
    int* sTapB = sTapA + MAXTAPS;
    int* sTapD = sTapB + MAXTAPS;

    float* const sCoef = (float*)(sTapD + MAXTAPS);      // RED: [BN][4] BatchNorm coefficients of the current tile's channels
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wc = wave % WN, wp = wave / WN;
    const int ntiles = p.grid_m * p.grid_n;
    // tap tables of every class (global tap index): written once
    if (t < MAXTAPS) {
        int total = p.ntaps;
        if (p.ncls > 1) { total = 0; for (int c = 0; c < p.ncls; ++c) total += p.cls_ntaps[c]; }
        int da = 0, db = 0, dd = 0;
        if (t < total) {
            da = ((int)p.dh[t] * p.Wi + (int)p.dw[t]) * p.lda * ES;
            db = (int)p.wt[t] * p.Kc * ES;
            dd = ((int)p.dh[t] & 0xffff) | ((int)p.dw[t] << 16);
        }
        sTapA[t] = da; sTapB[t] = db; sTapD[t] = dd;
    }
    __syncthreads();

    const int r = t >> 3;
    const int qs = t & 7;
    const unsigned q16 = (unsigned)((qs ^ ((r >> 1) & 7)) << 4);
    const int spt = p.Kc >> 6;
    u32x4 rsA, rsB;
    {
        const unsigned long long pa = (unsigned long long)p.A, pb = (unsigned long long)p.B;
        rsA = u32x4{(unsigned)pa, (unsigned)(pa >> 32) & 0xffffu, p.bytesA, 0x00020000u};
        rsB = u32x4{(unsigned)pb, (unsigned)(pb >> 32) & 0xffffu, p.bytesB, 0x00020000u};
    }
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned wave_lds = lds0 + (unsigned)wave * (8 * GROWB);

    struct TileInfo { int mtile, m0, n0, ntaps, tap0, Hg, Wg, M, h0, w0; };
    auto tile_info = [&](int lin) {
        TileInfo ti;
        const int tile = xcd_remap(lin, ntiles);
        int mtile, ntile;
        if (p.m_fastest) { ntile = tile / p.grid_m; mtile = tile - ntile * p.grid_m; }
        else { mtile = tile / p.grid_n; ntile = tile - mtile * p.grid_n; }
        ti.ntaps = p.ntaps; ti.tap0 = 0; ti.Hg = p.Hg; ti.Wg = p.Wg; ti.M = p.M; ti.h0 = p.out_h0; ti.w0 = p.out_w0;
        if (p.ncls > 1) {
            int c = 0;
            while (c + 1 < p.ncls && mtile >= p.cls_tile0[c + 1]) ++c;
            mtile -= p.cls_tile0[c];
            ti.ntaps = p.cls_ntaps[c]; ti.tap0 = p.cls_tap0[c]; ti.Hg = p.cls_Hg[c]; ti.Wg = p.cls_Wg[c]; ti.M = p.cls_M[c];
            ti.h0 = p.cls_h0[c]; ti.w0 = p.cls_w0[c];
        }
        // wave-uniform by construction; say so (the class tables are indexed dynamically, which lands them in VGPRs)
        mtile = __builtin_amdgcn_readfirstlane(mtile); ntile = __builtin_amdgcn_readfirstlane(ntile);
        ti.ntaps = __builtin_amdgcn_readfirstlane(ti.ntaps); ti.tap0 = __builtin_amdgcn_readfirstlane(ti.tap0);
        ti.Hg = __builtin_amdgcn_readfirstlane(ti.Hg); ti.Wg = __builtin_amdgcn_readfirstlane(ti.Wg);
        ti.M = __builtin_amdgcn_readfirstlane(ti.M); ti.h0 = __builtin_amdgcn_readfirstlane(ti.h0);
        ti.w0 = __builtin_amdgcn_readfirstlane(ti.w0);
        ti.mtile = mtile; ti.m0 = mtile * BM; ti.n0 = ntile * BN;
        return ti;
    };
    // per-thread DMA descriptors of a tile: byte offset of the (0,0) tap of each of its A rows + tap-validity bits, B row offsets
    auto describe = [&](const TileInfo& ti, unsigned (&rowoff)[AR], unsigned (&vmask)[AR], unsigned (&browoff)[BR]) {
        int ih0[AR], iw0[AR];
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const int m = ti.m0 + r + RPP * i;
            rowoff[i] = 0; vmask[i] = 0; ih0[i] = -100000; iw0[i] = 0;
            if (m < ti.M) {
                const int gw = m % ti.Wg;
                const int tmp = m / ti.Wg;
                const int gh = tmp % ti.Hg;
                const int n = tmp / ti.Hg;
                ih0[i] = gh * p.in_mul;
                iw0[i] = gw * p.in_mul;
                rowoff[i] = (unsigned)(((n * p.Hi + ih0[i]) * p.Wi + iw0[i]) * p.lda) * (unsigned)ES + q16;
            }
        }
        for (int tp = 0; tp < ti.ntaps; ++tp) {
            const int dd = sTapD[ti.tap0 + tp];
            const int dh = (int)(short)(dd & 0xffff), dw = dd >> 16;
#pragma unroll
            for (int i = 0; i < AR; ++i) {
                const bool ok = (unsigned)(ih0[i] + dh) < (unsigned)p.Hi && (unsigned)(iw0[i] + dw) < (unsigned)p.Wi;
                vmask[i] |= ok ? (1u << tp) : 0u;
            }
        }
#pragma unroll
        for (int i = 0; i < BR; ++i) {
            const int co = ti.n0 + r + RPP * i;
            browoff[i] = co < p.Cout ? (unsigned)co * p.ldb_bytes + q16 : 0xF0000000u;
        }
    };

    // ---- issue cursor: the K-step to DMA next; runs ahead of the MFMAs by one step and crosses into the next tile
    unsigned c_rowoff[AR], c_vmask[AR], c_browoff[BR];      // descriptors of the tile the cursor is in
    unsigned n_rowoff[AR], n_vmask[AR], n_browoff[BR];      // ... of the tile after it (prepared at the start of a tile)
    int ic_tap = 0, ic_cb = 0, ic_ntaps = 0, ic_tap0 = 0;
    int nx_ntaps = 0, nx_tap0 = 0;
    bool ic_valid = false, nx_valid = false;
    auto issue = [&](int stg) {
        const int da = sTapA[ic_tap0 + ic_tap], db = sTapB[ic_tap0 + ic_tap];
        const bool live = ic_valid;                               // beyond the CTA's last tile: every lane out of range (zeros)
        const unsigned kb = (unsigned)ic_cb << 7;
        const unsigned tbit = live ? 1u << ic_tap : 0u;
        const unsigned kbB = live ? kb : 0xF0000000u;
        const unsigned base = __builtin_amdgcn_readfirstlane(wave_lds + (unsigned)stg * STAGE);
#pragma unroll
        for (int i = 0; i < AR; ++i) {
            const unsigned off = (c_vmask[i] & tbit) ? (c_rowoff[i] + (unsigned)da + kb) : 0xFFFFFFFFu;
            lds_dma16(rsA, base + i * RPP * GROWB, off);
        }
#pragma unroll
        for (int i = 0; i < BR; ++i) lds_dma16(rsB, base + BM * GROWB + i * RPP * GROWB, c_browoff[i] + (unsigned)db + kbB);
        if (live && ++ic_tap == ic_ntaps) {
            ic_tap = 0;
            if (++ic_cb == spt) {                                 // the cursor leaves its tile
                ic_cb = 0;
                ic_valid = nx_valid;
                ic_ntaps = nx_ntaps; ic_tap0 = nx_tap0;
#pragma unroll
                for (int i = 0; i < AR; ++i) { c_rowoff[i] = n_rowoff[i]; c_vmask[i] = n_vmask[i]; }
#pragma unroll
                for (int i = 0; i < BR; ++i) c_browoff[i] = n_browoff[i];
                nx_valid = false;
            }
        }
    };

    const int lrow = lane & 15;
    const int sw_rd = (lrow >> 1) & 7;
    const int lk0 = (((lane >> 4)) ^ sw_rd) << 4;
    const int lk1 = (((lane >> 4) + 4) ^ sw_rd) << 4;
    const unsigned char* const fa = smem + BM * GROWB + (wc * BNW + lrow) * GROWB;
    const unsigned char* const fb = smem + (wp * (BM / WP) + lrow) * GROWB;
    uint4 af0[CT], bf0[PT], af1[CT], bf1[PT];
    auto rdfrag = [&](int stg, int half, uint4 (&af)[CT], uint4 (&bfr)[PT]) {
        const unsigned char* a_base = fa + stg * STAGE + (half ? lk1 : lk0);
        const unsigned char* b_base = fb + stg * STAGE + (half ? lk1 : lk0);
#pragma unroll
        for (int c = 0; c < CT; ++c) af[c] = *(const uint4*)(a_base + c * 16 * GROWB);
#pragma unroll
        for (int j = 0; j < PT; ++j) bfr[j] = *(const uint4*)(b_base + j * 16 * GROWB);
    };

    // (the launcher guarantees n_k >= 2 for every tile: the cursor then never runs further ahead than the tile whose descriptors
    //  were prepared at the start of the tile the MFMAs are in)
    int lin = blockIdx.x;
    if (lin >= ntiles) return;
    TileInfo cur = tile_info(lin);
    describe(cur, c_rowoff, c_vmask, c_browoff);
    ic_valid = true; ic_ntaps = cur.ntaps; ic_tap0 = cur.tap0;
    int par = 0;
    issue(par);                            // step 0 of the first tile
    for (; lin < ntiles; lin += gridDim.x) {
        const int nk = cur.ntaps * spt;
        // descriptors of the tile after this one, before the cursor can reach it (it is at step 1 of this tile now)
        const int lin_n = lin + gridDim.x;
        TileInfo nxt = cur;
        nx_valid = lin_n < ntiles;
        if (nx_valid) {
            nxt = tile_info(lin_n);
            describe(nxt, n_rowoff, n_vmask, n_browoff);
            nx_ntaps = nxt.ntaps; nx_tap0 = nxt.tap0;
        }
        f32x4 acc[CT][PT];
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int j = 0; j < PT; ++j) acc[c][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        auto mma = [&](const uint4 (&af)[CT], const uint4 (&bfr)[PT]) {
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int j = 0; j < PT; ++j) Mma<T>::run(af[c], bfr[j], acc[c][j]);
        };
        wait_vm_barrier<0>();              // step 0 landed everywhere; everyone is past the previous tile's epilogue
        if constexpr (RED) br_fill_coef<BN>(p, sCoef, cur.n0, t);      // read again only after the K loop's barriers
        issue(par ^ 1);                    // step 1
        rdfrag(par, 0, af0, bf0);
        for (int kk = 0; kk < nk; ++kk) {
            const int stg = (par + kk) & 1;
            rdfrag(stg, 1, af1, bf1);
            mma(af0, bf0);
            if (kk + 1 < nk) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave holds all of step kk in registers
                wait_vm_barrier<0>();                                   // step kk+1 landed everywhere
                issue(stg);                                             // step kk+2 (possibly the next tile's step 0) -> the stage step kk occupied
                rdfrag(stg ^ 1, 0, af0, bf0);
            }
            mma(af1, bf1);
        }
        const int sl = (par + nk - 1) & 1;     // the stage of the last K-step: free now, the epilogue's scratch
        par = sl ^ 1;                          // the next tile's step 0 is landing in the other one
        // every wave has its last fragments in registers before the scratch stage is overwritten (no vmcnt wait: the next tile's DMAs
        // stay in flight through the epilogue)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        igemm2_epilogue<BM, BN, NW, WP, RED>(p, acc, smem + sl * STAGE, cur.m0, cur.n0, cur.mtile, cur.M, cur.Wg, cur.Hg, cur.h0, cur.w0, sCoef);
        cur = nxt;
    }
    wait_vm_barrier<0>();              // trailing (all-zero) DMAs land before the CTA's LDS goes away
}

// ------------------------------------------------------------------------------------------------------
// igemm2h: the 3x3 / stride 1 / pad 1 convolution (forward, or the equally shaped dgrad) in PATCH form.  A CTA owns an 8 x 16 block
// of output pixels of one image; per 64-channel block it loads the (8+2) x (16+2) activation patch ONCE (LDS-DMA, rows swizzled by
// their patch row index) and serves all nine taps from it — the ring kernel fetches the 128 activation rows again for every tap
// (9x the L2 -> LDS activation traffic).  Weights still stream: one [BN][64] tile per (channel block, tap) through a two-stage ring,
// so the traffic of a 128 x 128 tile per channel block is 23 KB + 9 x 16 KB instead of 9 x 32 KB.
//   * patch rows: pixel (pr, pc) of the patch at LDS row pr * 18 + pc (184 rows allocated: 23 wave-instructions of 8 rows); pixels
//     outside the image are out-of-range DMA offsets (zeros = the padding); two patch buffers, the next channel block's patch is
//     requested at the first tap of the current one;
//   * a wave's 16-pixel MFMA row tile is one image row of the block, so its fragment rows for tap (dh, dw) are the 16 CONSECUTIVE
//     patch rows (tr + 1 + dh) * 18 + (1 + dw) + 0..15: the (row >> 1) & 7 chunk swizzle is conflict-free at any row offset;
//   * epilogue = igemm2_epilogue with the block described as a one-image "class" (Wg = 16, Hg = 8, origin = the block's corner).
// Requires Ho % 8 == 0 and Wo % 16 == 0 (every tile full: the BN-partial contract of 128-pixel blocks holds unchanged).
// ------------------------------------------------------------------------------------------------------
#define H_PW 18
#define H_PROWS 192      // 10 x 18 = 180 patch rows, rounded to whole DMA passes of the 8-wave CTA (3 x 64)
// outstanding DMAs (per thread) that may remain when step g's weights are needed: the S - 2 younger weight steps plus the patch
// passes issued by the S - 1 loop iterations before this one (one pass at each of the taps 0..2)
template <int S, int BR, int PP>
__host__ __device__ constexpr int halo_wait(int tap) {
    int n = (S - 2) * BR;
    for (int d = 1; d <= S - 1; ++d) n += ((tap - d + 9 * 8) % 9) < PP ? 1 : 0;
    return n;
}
template <int BN, int NW, int WP, int S>
__global__ __launch_bounds__(NW * 64) void igemm2h_kernel(const IgemmArgs p) {
    using T = bf16_t;
    constexpr int ES = 2;
    constexpr int BM = 128;
    constexpr int RPP = NW * 8;                              // LDS rows one DMA pass of the CTA covers
    constexpr int BR = BN / RPP;                             // weight DMAs per thread per step
    constexpr int PP = (H_PROWS + RPP - 1) / RPP;            // patch DMA passes per channel block, one per step at taps 0 .. PP-1
    constexpr int WN = NW / WP;
    constexpr int BNW = BN / WN;
    constexpr int CT = BNW / 16;
    constexpr int PT = BM / (16 * WP);
    constexpr int PBYTES = H_PROWS * GROWB;
    constexpr int RBYTES = BN * GROWB;
    static_assert(BN % RPP == 0 && PP <= 9 && S >= 2 && S <= 7 && PP + S <= 10, "stage geometry (the last patch pass must be older than the step that needs it)");
    static_assert(2 * PBYTES + S * RBYTES >= BM * BN * 2 + 8192, "epilogue scratch");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const ring = smem + 2 * PBYTES;

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wc = wave % WN, wp = wave / WN;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    int mtile, ntile;
    if (p.m_fastest) { ntile = tile / p.grid_m; mtile = tile - ntile * p.grid_m; }
    else { mtile = tile / p.grid_n; ntile = tile - mtile * p.grid_n; }
    const int tiles_w = p.Wo >> 4, tiles_hw = (p.Ho >> 3) * tiles_w;
    const int n = mtile / tiles_hw;
    const int rem = mtile - n * tiles_hw;
    const int h0 = (rem / tiles_w) << 3, w0 = (rem % tiles_w) << 4;
    const int n0 = ntile * BN;

    // this thread's DMA slots: row r of each pass, 16-byte slot qs; it fetches the logical chunk qs ^ swizzle(row in its buffer)
    const int r = t >> 3, qs = t & 7;
    unsigned poff[PP];
#pragma unroll
    for (int i = 0; i < PP; ++i) {
        const int rho = r + RPP * i;
        const int pr = rho / H_PW, pc = rho - pr * H_PW;
        const int h = h0 - 1 + pr, w = w0 - 1 + pc;
        const bool ok = rho < 10 * H_PW && (unsigned)h < (unsigned)p.Hi && (unsigned)w < (unsigned)p.Wi;
        poff[i] = ok ? (unsigned)(((n * p.Hi + h) * p.Wi + w) * p.lda) * (unsigned)ES + (unsigned)((qs ^ ((rho >> 1) & 7)) << 4) : 0xFFFFFFFFu;
    }
    unsigned browoff[BR];
#pragma unroll
    for (int i = 0; i < BR; ++i) {
        const int row = r + RPP * i;
        const int co = n0 + row;
        browoff[i] = co < p.Cout ? (unsigned)co * p.ldb_bytes + (unsigned)((qs ^ ((row >> 1) & 7)) << 4) : 0xF0000000u;
    }
    const int spt = p.Kc >> 6;
    const int nsteps = 9 * spt;
    u32x4 rsA, rsB;
    {
        const unsigned long long pa = (unsigned long long)p.A, pb = (unsigned long long)p.B;
        rsA = u32x4{(unsigned)pa, (unsigned)(pa >> 32) & 0xffffu, p.bytesA, 0x00020000u};
        rsB = u32x4{(unsigned)pb, (unsigned)(pb >> 32) & 0xffffu, p.bytesB, 0x00020000u};
    }
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned wave_lds = lds0 + (unsigned)wave * (8 * GROWB);
    // pass i of the patch of channel block cb -> patch buffer cb & 1.  EVERY thread issues exactly one DMA per call (the vmcnt
    // arithmetic is uniform); a block beyond the last sends out-of-range offsets into the buffer the last block does not use
    auto issue_patch = [&](int cb, int i) {
        const bool live = cb < spt && poff[i] != 0xFFFFFFFFu;
        const unsigned base = wave_lds + (unsigned)(cb & 1) * PBYTES + (unsigned)(i * RPP * GROWB);
        lds_dma16(rsA, base, live ? poff[i] + ((unsigned)cb << 7) : 0xFFFFFFFFu);
    };
    auto issue_w = [&](int g, int stg) {                     // weight tile of step g = (channel block g / 9, tap g % 9)
        const int cb = g / 9, tap = g - cb * 9;
        const bool live = g < nsteps;
        const unsigned add = live ? (unsigned)p.wt[tap] * (unsigned)p.Kc * ES + ((unsigned)cb << 7) : 0xF0000000u;
        const unsigned base = wave_lds + 2u * PBYTES + (unsigned)stg * RBYTES;
#pragma unroll
        for (int i = 0; i < BR; ++i) lds_dma16(rsB, base + i * RPP * GROWB, browoff[i] + add);
    };

    f32x4 acc[CT][PT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int j = 0; j < PT; ++j) acc[c][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int lrow = lane & 15, lgrp = lane >> 4;
    const int sw_w = (lrow >> 1) & 7;
    const unsigned char* const fa = ring + (wc * BNW + lrow) * GROWB;           // weights (MFMA A operand)
    // prologue: the first patch, then S - 1 weight steps
#pragma unroll
    for (int i = 0; i < PP; ++i) issue_patch(0, i);
#pragma unroll
    for (int u = 0; u < S - 1; ++u) issue_w(u, u);
    int stg = 0;
    // one step; the tap is a compile-time constant (the vmcnt immediate depends on it), FIRST = channel block 0
    auto step = [&](auto tapc, auto firstc, int cb) {
        constexpr int tap = decltype(tapc)::value;
        constexpr bool first = decltype(firstc)::value;
        const int g = cb * 9 + tap;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // outstanding DMAs younger than step g's weights: S - 2 weight steps + the patch passes of the iterations since its issue
        constexpr int npp = first ? (tap < S - 1 ? (tap < PP ? tap : PP) : halo_wait<S, BR, PP>(tap) - (S - 2) * BR)
                                  : halo_wait<S, BR, PP>(tap) - (S - 2) * BR;
        wait_vm_barrier<(S - 2) * BR + npp>();
        {
            int nst = stg + S - 1;
            if (nst >= S) nst -= S;
            issue_w(g + S - 1, nst);                         // into the stage step g - 1 occupied
        }
        if constexpr (tap < PP) issue_patch(cb + 1, tap);    // the next channel block's patch, one pass per step
        const int dh = (int)p.dh[tap], dw = (int)p.dw[tap];
        const unsigned char* const wst = fa + stg * RBYTES;
        const unsigned char* const pst = smem + (cb & 1) * PBYTES;
        int prow[PT];
#pragma unroll
        for (int j = 0; j < PT; ++j) prow[j] = (wp * PT + j + 1 + dh) * H_PW + (lrow + 1 + dw);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            uint4 af[CT], bfr[PT];
            const int kq = lgrp + 4 * half;
#pragma unroll
            for (int c = 0; c < CT; ++c) af[c] = *(const uint4*)(wst + c * 16 * GROWB + ((kq ^ sw_w) << 4));
#pragma unroll
            for (int j = 0; j < PT; ++j) bfr[j] = *(const uint4*)(pst + prow[j] * GROWB + ((kq ^ ((prow[j] >> 1) & 7)) << 4));
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int j = 0; j < PT; ++j) Mma<T>::run(af[c], bfr[j], acc[c][j]);
        }
        stg = stg + 1 == S ? 0 : stg + 1;
    };
#define H_STEPS(F, CB)                                                                                                          \
    step(std::integral_constant<int, 0>{}, F, CB); step(std::integral_constant<int, 1>{}, F, CB);                              \
    step(std::integral_constant<int, 2>{}, F, CB); step(std::integral_constant<int, 3>{}, F, CB);                              \
    step(std::integral_constant<int, 4>{}, F, CB); step(std::integral_constant<int, 5>{}, F, CB);                              \
    step(std::integral_constant<int, 6>{}, F, CB); step(std::integral_constant<int, 7>{}, F, CB);                              \
    step(std::integral_constant<int, 8>{}, F, CB)
    H_STEPS(std::true_type{}, 0);
    for (int cb = 1; cb < spt; ++cb) { H_STEPS(std::false_type{}, cb); }
#undef H_STEPS
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wait_vm_barrier<0>();                                    // the trailing all-zero DMAs have landed; the LDS is free
    igemm2_epilogue<BM, BN, NW, WP>(p, acc, smem, 0, n0, mtile, BM, 16, 8, n * p.Ho + h0, w0);
}

// The same kernel with a TWO-stage weight ring, 184-row patches and a rolled step loop: 79 VGPRs and 78 KB of LDS, so that two CTAs
// share a CU — for 128-wide tiles that matters more than ring depth (one CTA per CU with 3 / 4 / 6 weight stages in flight:
// 128->128 k3 @80^2 forward 62 / 61 / 66 us against 51 us here and 53 us for the ring kernel).
#define HS_PROWS 184
template <int BN, int NW, int WP, bool ONEP = false>      // ONEP: one channel block (Cin = 64) needs one patch buffer: 40 KB, four CTAs per CU
__global__ __launch_bounds__(NW * 64) void igemm2hs_kernel(const IgemmArgs p) {
    using T = bf16_t;
    constexpr int ES = 2;
    constexpr int BM = 128;
    constexpr int RPP = NW * 8;
    constexpr int BR = BN / RPP;
    constexpr int PP = (HS_PROWS + RPP - 1) / RPP;
    constexpr int WN = NW / WP;
    constexpr int BNW = BN / WN;
    constexpr int CT = BNW / 16;
    constexpr int PT = BM / (16 * WP);
    constexpr int PBYTES = HS_PROWS * GROWB;
    constexpr int RBYTES = BN * GROWB;
    static_assert(BN % RPP == 0 && (ONEP ? 1 : 2) * PBYTES + 2 * RBYTES >= BM * BN * 2 + 8192, "stage geometry");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NPB = ONEP ? 1 : 2;
    unsigned char* const ring = smem + NPB * PBYTES;
    // per-tap tables in LDS (patch-row delta of the tap, byte offset of its weight slice).  A run-time index into the byte arrays of
    // the kernel ARGUMENTS compiles to `global_load_sbyte` (there are no sub-dword scalar loads) and an `s_waitcnt vmcnt(0)` in front
    // of its first use — which drained the weight DMA issued just before it, in every step (tools/asm_loops.py flags such loads)
    int* const sTd = (int*)(ring + 2 * RBYTES);
    int* const sTw = sTd + 16;
    const int t = threadIdx.x;
    if (t < 9) {
        sTd[t] = (int)p.dh[t] * H_PW + (int)p.dw[t];
        sTw[t] = (int)p.wt[t] * p.Kc * ES;
    }
    __syncthreads();
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wc = wave % WN, wp = wave / WN;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    int mtile, ntile;
    if (p.m_fastest) { ntile = tile / p.grid_m; mtile = tile - ntile * p.grid_m; }
    else { mtile = tile / p.grid_n; ntile = tile - mtile * p.grid_n; }
    const int tiles_w = p.Wo >> 4, tiles_hw = (p.Ho >> 3) * tiles_w;
    const int n = mtile / tiles_hw;
    const int rem = mtile - n * tiles_hw;
    const int h0 = (rem / tiles_w) << 3, w0 = (rem % tiles_w) << 4;
    const int n0 = ntile * BN;
    const int r = t >> 3, qs = t & 7;
    unsigned poff[PP];
#pragma unroll
    for (int i = 0; i < PP; ++i) {
        const int rho = r + RPP * i;
        const int pr = rho / H_PW, pc = rho - pr * H_PW;
        const int h = h0 - 1 + pr, w = w0 - 1 + pc;
        const bool ok = rho < 10 * H_PW && (unsigned)h < (unsigned)p.Hi && (unsigned)w < (unsigned)p.Wi;
        poff[i] = ok ? (unsigned)(((n * p.Hi + h) * p.Wi + w) * p.lda) * (unsigned)ES + (unsigned)((qs ^ ((rho >> 1) & 7)) << 4) : 0xFFFFFFFFu;
    }
    unsigned browoff[BR];
#pragma unroll
    for (int i = 0; i < BR; ++i) {
        const int row = r + RPP * i;
        const int co = n0 + row;
        browoff[i] = co < p.Cout ? (unsigned)co * p.ldb_bytes + (unsigned)((qs ^ ((row >> 1) & 7)) << 4) : 0xF0000000u;
    }
    const int spt = p.Kc >> 6;
    const int nsteps = 9 * spt;
    u32x4 rsA, rsB;
    {
        const unsigned long long pa = (unsigned long long)p.A, pb = (unsigned long long)p.B;
        rsA = u32x4{(unsigned)pa, (unsigned)(pa >> 32) & 0xffffu, p.bytesA, 0x00020000u};
        rsB = u32x4{(unsigned)pb, (unsigned)(pb >> 32) & 0xffffu, p.bytesB, 0x00020000u};
    }
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned wave_lds = lds0 + (unsigned)wave * (8 * GROWB);
    auto issue_patch = [&](int cb) {
        const unsigned base = wave_lds + (unsigned)(ONEP ? 0 : (cb & 1)) * PBYTES;
        const unsigned kb = (unsigned)cb << 7;
#pragma unroll
        for (int i = 0; i < PP; ++i) {
            if (RPP * i + wave * 8 < HS_PROWS)               // (wave-uniform) rows beyond the allocation are not written
                lds_dma16(rsA, base + i * RPP * GROWB, poff[i] == 0xFFFFFFFFu ? 0xFFFFFFFFu : poff[i] + kb);
        }
    };
    auto issue_w = [&](int stg, int cbw, int woff) {          // weight tile of a step: channel block cbw, tap slice at byte offset woff
        const unsigned add = cbw < spt ? (unsigned)woff + ((unsigned)cbw << 7) : 0xF0000000u;
        const unsigned base = wave_lds + (unsigned)NPB * PBYTES + (unsigned)stg * RBYTES;
#pragma unroll
        for (int i = 0; i < BR; ++i) lds_dma16(rsB, base + i * RPP * GROWB, browoff[i] + add);
    };
    f32x4 acc[CT][PT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int j = 0; j < PT; ++j) acc[c][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int lrow = lane & 15, lgrp = lane >> 4;
    const int sw_w = (lrow >> 1) & 7;
    const unsigned char* const fa = ring + (wc * BNW + lrow) * GROWB;
    issue_patch(0);
    issue_w(0, 0, sTw[0]);
    // (cb, tap) of step g and the table entries it needs, read one step ahead: dcur = patch-row delta of step g, wnx = weight offset of
    // step g + 1
    int cb = 0, tap = 0;
    int dcur = sTd[0], wnx = sTw[1];
    for (int g = 0; g < nsteps; ++g) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        wait_vm_barrier<0>();                                // step g's weights (and its patch) landed; everyone is done with step g - 1
        const int t1 = tap == 8 ? 0 : tap + 1, c1 = tap == 8 ? cb + 1 : cb;      // step g + 1
        const int t2 = t1 == 8 ? 0 : t1 + 1;                                      // tap of step g + 2
        const int dnx = sTd[t1], wnn = sTw[t2];              // used by the next iteration
        issue_w((g + 1) & 1, c1, wnx);
        if constexpr (ONEP) {
            // one patch buffer: the next channel block's patch can only be requested once every wave has left the old one (the
            // barrier above), and is waited for at once — the other resident CTAs (four per CU at 40 KB) cover the round trip
            if (tap == 0 && cb > 0) {
                issue_patch(cb);
                wait_vm_barrier<0>();
            }
        } else {
            if (tap == 0 && cb + 1 < spt) issue_patch(cb + 1);
        }
        const unsigned char* const wst = fa + (g & 1) * RBYTES;
        const unsigned char* const pst = smem + (ONEP ? 0 : (cb & 1)) * PBYTES;
        int prow[PT];
#pragma unroll
        for (int j = 0; j < PT; ++j) prow[j] = (wp * PT + j + 1) * H_PW + (lrow + 1) + dcur;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            uint4 af[CT], bfr[PT];
            const int kq = lgrp + 4 * half;
#pragma unroll
            for (int c = 0; c < CT; ++c) af[c] = *(const uint4*)(wst + c * 16 * GROWB + ((kq ^ sw_w) << 4));
#pragma unroll
            for (int j = 0; j < PT; ++j) bfr[j] = *(const uint4*)(pst + prow[j] * GROWB + ((kq ^ ((prow[j] >> 1) & 7)) << 4));
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int j = 0; j < PT; ++j) Mma<T>::run(af[c], bfr[j], acc[c][j]);
        }
        dcur = dnx; wnx = wnn; tap = t1; cb = c1;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wait_vm_barrier<0>();
    igemm2_epilogue<BM, BN, NW, WP>(p, acc, smem, 0, n0, mtile, BM, 16, 8, n * p.Ho + h0, w0);
}

// ------------------------------------------------------------------------------------------------------
// igemm2w (round 5): 3x3 / stride 1 / pad 1 with ONE 64-channel block of K (Kc = 64: K = 576) and at most 128 output channels — the
// 64 -> 64 and 64 -> 128 layers at 160^2 of config 2, forward and the equally shaped data gradients — with the WEIGHTS IN REGISTERS.
// Every other MFMA kernel of this file stages both operands through the L2 -> LDS path, which delivers ~70 GB/s per CU: at 64 FLOP
// per staged byte (128 x 128 tiles) that is 55 % of the matrix peak before anything else, and these short-K layers sat at 0.24-0.34.
// Here the whole weight matrix of a CTA (CO x 576 bf16 = 72 / 144 KB) lives in the register file as MFMA A fragments — a wave holds
// 32 output channels x 576 = 36 fragments = 144 VGPRs, loaded once per persistent CTA — and the ONLY staged operand is the
// activation patch ((R + 2) x 34 pixels x 128 B per block of R x 32 output pixels, LDS-DMA, double-buffered): 260..460 FLOP per
// staged byte.  v_mfma_f32_32x32x16_bf16 (the 32-row A fragment is what makes 32 channels x 576 fit 144 registers; a 32-pixel B
// fragment is one image row of the block: 32 consecutive patch rows, conflict-free under the (row >> 1) & 7 chunk swizzle at any
// offset).  8 waves = CG channel groups x PG pixel groups, two image rows per wave; per block 72 MFMAs and 72 ds_read_b128 per
// wave (LDS at 50 % of its bandwidth), one DMA wait + two barriers.  Epilogue: bf16 through a swizzled LDS tile into whole pixel rows
// (asm stores, counted vmcnt); BatchNorm statistics (replica-sum mode only) are taken from the f32 ACCUMULATORS in the MFMA layout,
// before the rounding to bf16, like every other forward kernel of this file — a lane owns 16 channels for the whole kernel: (sum, sum
// of squares) in 32 registers, one cross-lane reduction and one atomic pass per CTA.  (They used to be taken from the bf16 tile:
// the sum of n rounded values is off by 1.7e-3 sqrt(sum of squares) rms, which the launch census saw at 5.07e-3 on one channel of
// ResNet50's 32 x 160 x 160 x 64 layer, above the 5e-3 every statistics launch is held to.)  The layers are then bound by HBM (64 -> 128: 157 MB) rather than by the staging path.
// ------------------------------------------------------------------------------------------------------
// A 16-byte store issued from inline asm: the hardware reads the four data registers over two cycles AFTER issue, and a vector
// instruction that rewrites one of them in the next cycle wins the race (the compiler's hazard recognizer pads a store it knows with
// a wait state; it cannot see into an asm statement).  Found as an LDS address in every third dword of dx: the `s_nop` is the fix.
__device__ __forceinline__ void buf_store16_asm(const u32x4& v, unsigned off, const u32x4& rsrc) {
    asm volatile("buffer_store_dwordx4 %0, %1, %2, 0 offen\n\ts_nop 1" ::"v"(v), "v"(off), "s"(rsrc) : "memory");
}
#define WR_PW 34
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
// NW = 8: one CTA per CU, its two waves per SIMD in lock-step; NW = 4: half the pixel rows per CTA, two CTAs per CU that drift apart
// (one's epilogue and DMA issue under the other's MFMAs — the pairing the 128 x 128 ring kernels rely on)
template <int CO, bool STATS, int NW>
__global__ __launch_bounds__(NW * 64, 2) void igemm2w_kernel(const IgemmArgs p, int nblocks) {
    using T = bf16_t;
    constexpr int CG = CO / 32, PG = NW / CG, RW = 2, R = PG * RW;      // channel groups, pixel groups, image rows per wave / per block
    constexpr int NT = NW * 64, PR = NW * 8;                              // threads; patch pixels per DMA pass
    constexpr int PROWS = (R + 2) * WR_PW;
    constexpr int PASSES = (PROWS + PR - 1) / PR;                         // DMA passes of the CTA
    constexpr int PBYTES = PASSES * PR * GROWB;
    constexpr int BPX = R * 32;                                           // output pixels per block
    constexpr int NCH = CO / 8;                                           // 16-byte chunks per output row
    constexpr int ORB = CO * 2;
    static_assert(BPX * NCH == 4 * NT && NT % NCH == 0, "four 16-byte store slots per thread, a fixed channel chunk per thread");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const stage = smem + 2 * PBYTES;                       // [BPX][ORB], chunk q of pixel x at slot q ^ (x & (NCH - 1))
    float* const sred = (float*)smem;                                     // (after the last block) [PG pixel groups][CO][2]
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int cg = wave % CG, pg = wave / CG;
    const int ln = lane & 31, lh = lane >> 5;
    const int blocks_w = p.Wo >> 5, blocks_img = (p.Ho / R) * blocks_w;
    u32x4 rsA, rsC;
    {
        const unsigned long long pa = (unsigned long long)p.A, pc = (unsigned long long)p.C;
        rsA = u32x4{(unsigned)pa, (unsigned)(pa >> 32) & 0xffffu, p.bytesA, 0x00020000u};
        rsC = u32x4{(unsigned)pc, (unsigned)(pc >> 32) & 0xffffu, p.bytesC, 0x00020000u};
    }
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned wave_lds = lds0 + (unsigned)wave * 1024u;
    // this thread's patch pixels: pass i -> pixel rho = PR i + t / 8 of the (R + 2) x 34 patch, 16-byte slot t & 7
    const int rq = t >> 3, qs = t & 7;
    int pprc[PASSES];                                                     // (patch row << 8 | patch column) of this thread's pixel of pass i
#pragma unroll
    for (int i = 0; i < PASSES; ++i) {
        const int rho = i * PR + rq;
        pprc[i] = rho < PROWS ? ((rho / WR_PW) << 8) | (rho - (rho / WR_PW) * WR_PW) : (4000000 << 8);  // (beyond the patch: a row outside any image)
    }
    auto block_origin = [&](int b, int& n, int& h0, int& w0) {
        n = b / blocks_img;
        const int rem = b - n * blocks_img;
        h0 = (rem / blocks_w) * R;
        w0 = (rem % blocks_w) << 5;
    };
    auto issue_patch = [&](int b, int buf) {
        int n, h0, w0;
        block_origin(b, n, h0, w0);
        const bool live = b < nblocks;
#pragma unroll
        for (int i = 0; i < PASSES; ++i) {
            const int rho = i * PR + rq;
            const int h = h0 - 1 + (pprc[i] >> 8), w = w0 - 1 + (pprc[i] & 255);
            const bool ok = live && (unsigned)h < (unsigned)p.Hi && (unsigned)w < (unsigned)p.Wi;
            const unsigned off = (unsigned)(((n * p.Hi + h) * p.Wi + w) * p.lda) * 2u + (unsigned)((qs ^ ((rho >> 1) & 7)) << 4);
            lds_dma16(rsA, wave_lds + (unsigned)buf * PBYTES + (unsigned)(i * PR * GROWB), ok ? off : 0xFFFFFFFFu);
        }
    };
    // persistent: a contiguous range of blocks per CTA
    const int per = (nblocks + (int)gridDim.x - 1) / (int)gridDim.x;
    const int b0 = blockIdx.x * per, b1 = min(nblocks, b0 + per);
    issue_patch(b0, 0);
    // ---- the weights: 36 A fragments (tap t, 16-channel step ks): row = output channel cg * 32 + ln, 8 channels ks * 16 + lh * 8 ..
    uint4 wreg[9][4];
    {
        const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)p.B, 0, p.bytesB, 0x00020000);
        const int co = cg * 32 + ln;
#pragma unroll
        for (int tp = 0; tp < 9; ++tp)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const unsigned off = co < p.Cout ? (unsigned)co * p.ldb_bytes + (unsigned)(((int)p.wt[tp] * p.Kc + ks * 16 + lh * 8) * 2) : 0xFFFFFFFFu;
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsB, off, 0, 0);
                wreg[tp][ks] = make_uint4(v.x, v.y, v.z, v.w);
            }
    }
    int tapd[9];
#pragma unroll
    for (int tp = 0; tp < 9; ++tp) tapd[tp] = (int)p.dh[tp] * WR_PW + (int)p.dw[tp];
    float s1[STATS ? 16 : 1], s2[STATS ? 16 : 1];                         // channel cg * 32 + 8 g + 4 lh + e at index 4 g + e
#pragma unroll
    for (int e = 0; e < (STATS ? 16 : 1); ++e) { s1[e] = 0.f; s2[e] = 0.f; }
    const bool want_stats = STATS && p.stats != nullptr;
    int ridx_base = (pg * RW + 1) * WR_PW + ln + 1;                       // patch pixel of (this wave's first row, column ln), tap (0, 0)
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");          // the first patch (and the weights) have landed
    int buf = 0;
    for (int b = b0; b < b1; ++b, buf ^= 1) {
        issue_patch(b + 1 < b1 ? b + 1 : nblocks, buf ^ 1);               // (beyond the range: all-zero DMAs, the count stays uniform)
        const unsigned char* const pst = smem + buf * PBYTES;
        f32x16_t acc[RW];
#pragma unroll
        for (int rb = 0; rb < RW; ++rb)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[rb][e] = 0.f;
        // (the fragment addresses are block-invariant: left visible, the compiler computes all 72 of them ahead of the block loop and
        //  spills the weights; behind the empty asm they are recomputed per tap — a handful of VALU per four MFMAs)
        asm volatile("" : "+v"(ridx_base));
        // 18 steps (tap, image row) of four fragment reads + four MFMAs (128 matrix cycles), software-pipelined one step deep: the reads
        // of step i + 1 are in flight under the MFMAs of step i (two fragment sets: the same 32 registers a whole tap's reads took)
        uint4 fq[2][4];
        auto rd = [&](int tp, int rb, uint4 (&f)[4]) {
            const int ridx = ridx_base + rb * WR_PW + tapd[tp];
            const unsigned char* const rowp = pst + ridx * GROWB;
            const int sw = (ridx >> 1) & 7;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) f[ks] = *(const uint4*)(rowp + (((2 * ks + lh) ^ sw) << 4));
        };
        rd(0, 0, fq[0]);
#pragma unroll
        for (int step = 0; step < 9 * RW; ++step) {
            const int tp = step / RW, rb = step % RW;
            if (step + 1 < 9 * RW) rd((step + 1) / RW, (step + 1) % RW, fq[(step + 1) & 1]);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
                acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wreg[tp][ks]),
                                                                  __builtin_bit_cast(bf16x8, fq[step & 1][ks]), acc[rb], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- epilogue: lane = pixel column ln of rows pg * RW + rb, channels cg * 32 + 8 g + 4 lh + e
        if constexpr (STATS) {
            if (want_stats) {
#pragma unroll
                for (int rb = 0; rb < RW; ++rb)
#pragma unroll
                    for (int e = 0; e < 16; ++e) { s1[e] += acc[rb][e]; s2[e] = fmaf(acc[rb][e], acc[rb][e], s2[e]); }
            }
        }
#pragma unroll
        for (int rb = 0; rb < RW; ++rb) {
            const int px = (pg * RW + rb) * 32 + ln;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                uint2 u;
                u.x = (uint32_t)f2bf(acc[rb][4 * g + 0]) | ((uint32_t)f2bf(acc[rb][4 * g + 1]) << 16);
                u.y = (uint32_t)f2bf(acc[rb][4 * g + 2]) | ((uint32_t)f2bf(acc[rb][4 * g + 3]) << 16);
                const int chq = cg * 4 + g;
                *(uint2*)(stage + px * ORB + ((chq ^ (px & (NCH - 1))) << 4) + (lh << 3)) = u;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        {
            int n, h0, w0;
            block_origin(b, n, h0, w0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int idx = t + NT * j;
                const int px = idx / NCH, ch = idx % NCH;                 // (ch = t % NCH for every j)
                const uint4 v = *(const uint4*)(stage + px * ORB + ((ch ^ (px & (NCH - 1))) << 4));
                const unsigned m = (unsigned)((n * p.Ho + h0 + (px >> 5)) * p.Wo + w0 + (px & 31));
                const unsigned off = ch * 8 < p.Cst ? (m * (unsigned)p.ldc + (unsigned)(ch * 8)) * 2u : 0xFFFFFFFFu;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                buf_store16_asm(u32x4{v.x, v.y, v.z, v.w}, off, rsC);
            }
        }
        // the next block's patch: younger than its DMAs are this block's four stores
        asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
    }
    if constexpr (!STATS) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // the trailing DMAs land before the LDS allocation goes away
        return;
    }
    if (want_stats) {
        // the 32 pixel columns of a half-wave hold the same 16 channels: sum over ln, then the CTA's pixel groups through LDS
#pragma unroll
        for (int e = 0; e < (STATS ? 16 : 1); ++e)
#pragma unroll
            for (int o = 1; o < 32; o <<= 1) { s1[e] += __shfl_xor(s1[e], o, 64); s2[e] += __shfl_xor(s2[e], o, 64); }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // trailing DMAs landed: the patch area is free
        if (ln == 0) {
#pragma unroll
            for (int e = 0; e < (STATS ? 16 : 1); ++e) {
                const int c = cg * 32 + (e >> 2) * 8 + lh * 4 + (e & 3);
                sred[(pg * CO + c) * 2] = s1[e];
                sred[(pg * CO + c) * 2 + 1] = s2[e];
            }
        }
        __syncthreads();
        if (t < CO && t < p.Cout) {
            float a = 0.f, b2 = 0.f;
#pragma unroll
            for (int w = 0; w < PG; ++w) { a += sred[(w * CO + t) * 2]; b2 += sred[(w * CO + t) * 2 + 1]; }
            float* dst = p.stats + (size_t)(blockIdx.x & (YDL_BN_REPLICAS - 1)) * 2 * p.stats_ld;
            atomicAdd(dst + t, a);
            atomicAdd(dst + p.stats_ld + t, b2);
        }
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // the trailing DMAs land before the LDS allocation goes away
    }
}

static int g_wreg = 1;          // ydl_debug_set key 17
static bool wreg_ok(const IgemmArgs& a) {
    if (!g_wreg || a.accumulate) return false;
    if (a.ncls > 1 || a.ntaps != 9 || a.Ttot != 9 || a.in_mul != 1 || a.out_mul != 1 || a.out_h0 != 0 || a.out_w0 != 0) return false;
    if (a.Hi != a.Ho || a.Wi != a.Wo || a.Hg != a.Ho || a.Wg != a.Wo || a.Kc != 64) return false;
    if (a.Cst != 64 && a.Cst != 128) return false;
    if ((a.Wo & 31) || a.Ho % (a.Cst == 128 ? 4 : 8)) return false;      // (blocks of 4 / 8 image rows x 32 columns; the 4-wave form: 2 / 4)
    if (a.stats != nullptr && !a.stats_atomic) return false;             // (replica-sum statistics only: no per-block partial rows)
    if ((long long)a.M < 4ll * 128 * ydl_device_cus()) return false;     // a few blocks per CTA, or the register load does not pay
    bool seen[9] = {false, false, false, false, false, false, false, false, false};
    for (int t = 0; t < 9; ++t) {
        const int dh = a.dh[t], dw = a.dw[t];
        if (dh < -1 || dh > 1 || dw < -1 || dw > 1 || seen[(dh + 1) * 3 + dw + 1]) return false;
        seen[(dh + 1) * 3 + dw + 1] = true;
    }
    return true;
}
// two 4-wave CTAs per CU.  Measured against one 8-wave CTA, same box: 64->64 @160^2 forward 50.0 -> 46.0 us, data gradient 45.3 -> 41.4 us,
// 64->128 data gradient 73..82 -> 71 us (patch kernels: 53.1 / 46.6 / 88..93 us); the step +0.9 %
template <int CO>
static int launch_igemm2w_cfg(IgemmArgs a, hipStream_t st, int fam) {
    constexpr int NW = 4, R = (NW / (CO / 32)) * 2, PR = NW * 8;
    const int nblocks = a.N * (a.Ho / R) * (a.Wo >> 5);
    constexpr int PASSES = ((R + 2) * WR_PW + PR - 1) / PR;
    const size_t smem = 2 * (size_t)PASSES * PR * GROWB + (size_t)R * 32 * CO * 2;
    YDL_SET_MAX_LDS((igemm2w_kernel<CO, true, NW>), smem);
    YDL_SET_MAX_LDS((igemm2w_kernel<CO, false, NW>), smem);
    const unsigned long long bc = ((unsigned long long)(a.N * a.Ho * a.Wo - 1) * a.ldc + a.Cst) * 2ull;
    YDL_CHECK(bc < 0xFFFFFFF0ull, "output larger than 4 GiB");
    a.bytesC = (unsigned)bc;
    ydl_note_kernel(fam, CO == 128 ? "igemm2w_kernel<128,nw4>" : "igemm2w_kernel<64,nw4>");
    const int ctas = std::min(ydl_device_cus() * 2, nblocks);
    if (a.stats != nullptr) igemm2w_kernel<CO, true, NW><<<ctas, NW * 64, smem, st>>>(a, nblocks);
    else igemm2w_kernel<CO, false, NW><<<ctas, NW * 64, smem, st>>>(a, nblocks);
    YDL_LAUNCH_CHECK();
    return 0;
}
static int launch_igemm2w(const IgemmArgs& a, hipStream_t st, int fam) {
    return a.Cst == 128 ? launch_igemm2w_cfg<128>(a, st, fam) : launch_igemm2w_cfg<64>(a, st, fam);
}

// ------------------------------------------------------------------------------------------------------
// igemm2s: the data gradient of a 3x3 / stride 2 / pad 1 convolution with all four output-parity classes FUSED in one CTA.
// The ring kernel runs such a dgrad as four dense sub-convolutions (1, 2, 2 and 4 taps): tiles with 2..8 K-steps whose fixed cost
// (descriptors, first DMA round trip, epilogue) is as large as their main loop, and every class fetches the same dy rows again.
// Here a CTA owns an 8 x 16 block of dy grid points (i, j) of one image and a 64-channel slice of dx, i.e. the 16 x 32 block of dx
// pixels (2i + ph, 2j + pw).  With p = 1:   dx[2i]   += dy[i] w[1]         dx[2i+1] += dy[i+1] w[0] + dy[i] w[2]   (same along w)
// so tap (kh, kw) reads dy at (i + [kh == 0], j + [kw == 0]) and feeds parity class (kh != 1, kw != 1): nine taps, one (8+1) x (16+1)
// dy patch per 64-channel block of dy (loaded once by LDS-DMA, out-of-image pixels are out-of-range offsets = zeros), four
// accumulator sets.  The taps are walked in groups that read the SAME dy pixels ((0,0): four taps, (0,1) and (1,0): two each,
// (1,1): one), so the pixel fragments are read from LDS once per group: 52 fragment reads per 72 MFMAs instead of 72.
// Weights stream as in igemm2hs_kernel: one [64 cin][64] tile per (channel block, tap) through a two-stage ring.
// Epilogue: igemm2_epilogue once per class (the block described as a one-image class with out_mul = 2 and the class's origin).
// Requires k = 3, s = 2, p = 1, Hdx = 2 Hdy, Wdx = 2 Wdy, Hdy % 8 == 0, Wdy % 16 == 0, Cout % 64 == 0 (the K dimension).
// ------------------------------------------------------------------------------------------------------
#define S2_PW 17
#define S2_PROWS 192      // 9 x 17 = 153 patch rows, rounded to whole DMA passes of the 8-wave CTA (3 x 64): every thread issues the same number of DMAs
__device__ constexpr int kS2Kh[9] = {1, 1, 2, 2, 1, 2, 0, 0, 0};       // tap order: groups (dh,dw) = (0,0) x4, (0,1) x2, (1,0) x2, (1,1)
__device__ constexpr int kS2Kw[9] = {1, 2, 1, 2, 0, 0, 1, 2, 0};
template <int NW, int WP, int S, bool ACC>      // ACC: dx += (its own instantiation: the pre-pass below costs the plain kernel registers it does not have)
__global__ __launch_bounds__(NW * 64, NW / 2) void igemm2s_kernel(const IgemmArgs p) {
    using T = bf16_t;
    constexpr int ES = 2;
    constexpr int BM = 128, BN = 64;
    constexpr int RPP = NW * 8;
    constexpr int BR = BN / RPP;
    constexpr int PP = (S2_PROWS + RPP - 1) / RPP;
    constexpr int WN = NW / WP;
    constexpr int BNW = BN / WN;
    constexpr int CT = BNW / 16;
    constexpr int PT = BM / (16 * WP);
    constexpr int PBYTES = S2_PROWS * GROWB;
    constexpr int RBYTES = BN * GROWB;
    static_assert(BN % RPP == 0 && BR == 1 && S2_PROWS % RPP == 0 && (S == 2 || S == 3), "one weight DMA per thread and step, whole patch passes");
    static_assert(2 * PBYTES + S * RBYTES >= BM * BN * 2, "epilogue scratch");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const ring = smem + 2 * PBYTES;
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wc = wave % WN, wp = wave / WN;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int mtile = tile / p.grid_n, ntile = tile - mtile * p.grid_n;
    const int tiles_w = p.Wi >> 4, tiles_hw = (p.Hi >> 3) * tiles_w;        // (Hi, Wi) = the dy grid
    const int n = mtile / tiles_hw;
    const int rem = mtile - n * tiles_hw;
    const int i0 = (rem / tiles_w) << 3, j0 = (rem % tiles_w) << 4;
    const int n0 = ntile * BN;
    const int r = t >> 3, qs = t & 7;
    const unsigned browoff = (n0 + r) < p.Cout ? (unsigned)(n0 + r) * p.ldb_bytes + (unsigned)((qs ^ ((r >> 1) & 7)) << 4) : 0xF0000000u;
    const int spt = p.Kc >> 6;
    u32x4 rsA, rsB;
    {
        const unsigned long long pa = (unsigned long long)p.A, pb = (unsigned long long)p.B;
        rsA = u32x4{(unsigned)pa, (unsigned)(pa >> 32) & 0xffffu, p.bytesA, 0x00020000u};
        rsB = u32x4{(unsigned)pb, (unsigned)(pb >> 32) & 0xffffu, p.bytesB, 0x00020000u};
    }
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned wave_lds = lds0 + (unsigned)wave * (8 * GROWB);
    // the patch of channel block cb -> buffer cb & 1; a block beyond the last sends out-of-range offsets (zeros) into the buffer the
    // last block does not use, so that every thread issues the same DMAs in every block (the counted waits below rely on it)
    auto issue_patch = [&](int cb) {
        const unsigned base = wave_lds + (unsigned)(cb & 1) * PBYTES;
        const unsigned kb = (unsigned)cb << 7;
        const bool live = cb < spt;
#pragma unroll
        for (int i = 0; i < PP; ++i) {
            // (the source offsets are recomputed per block rather than kept: three registers this kernel does not have)
            const int rho = r + RPP * i;
            const int pr = rho / S2_PW, pc = rho - pr * S2_PW;
            const int h = i0 + pr, w = j0 + pc;
            const bool ok = live && rho < 9 * S2_PW && h < p.Hi && w < p.Wi;
            const unsigned off = (unsigned)(((n * p.Hi + h) * p.Wi + w) * p.lda) * (unsigned)ES + (unsigned)((qs ^ ((rho >> 1) & 7)) << 4) + kb;
            lds_dma16(rsA, base + i * RPP * GROWB, ok ? off : 0xFFFFFFFFu);
        }
    };
    // weight tile of (channel block cb, tap slice kh*3+kw) -> ring stage stg; a block beyond the last sends out-of-range offsets (zeros)
    auto issue_w = [&](int stg, int cb, int slice) {
        const unsigned add = cb < spt ? (unsigned)slice * (unsigned)p.Kc * ES + ((unsigned)cb << 7) : 0xF0000000u;
        lds_dma16(rsB, wave_lds + 2u * PBYTES + (unsigned)stg * RBYTES, browoff + add);
    };
    f32x4 acc[4][CT][PT];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int j = 0; j < PT; ++j) acc[q][c][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int lrow = lane & 15, lgrp = lane >> 4;
    const int sw_w = (lrow >> 1) & 7;
    const unsigned char* const fa = ring + (wc * BNW + lrow) * GROWB;
    uint4 bq[2][PT];                                           // pixel fragments of the current tap group (both K halves)
    // one step: tap I of the walk (compile-time: its class selects the accumulator set), channel block cb
    auto step = [&](auto ic, int cb) {
        constexpr int I = decltype(ic)::value;
        constexpr int kh = kS2Kh[I], kw = kS2Kw[I];
        constexpr int dh = kh == 0 ? 1 : 0, dw = kw == 0 ? 1 : 0;
        constexpr int cls = (kh != 1 ? 2 : 0) + (kw != 1 ? 1 : 0);
        constexpr bool group_start = I == 0 || I == 4 || I == 6 || I == 8;
        // Issue order: step h issues W(h + S - 1) and then, at tap 0, the PP patch passes of the next block.  DMAs younger than step g's
        // weights when step g waits for them (S = 3): W(g + 1), plus the patch passes of steps g - 2 and g - 1 if those were tap 0
        constexpr int I1 = (I + 8) % 9, I2 = (I + 7) % 9;                      // taps of steps g - 1, g - 2
        constexpr int NY = S == 2 ? 0 : 1 + (I1 == 0 ? PP : 0) + (I2 == 0 ? PP : 0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        wait_vm_barrier<NY>();                                 // step g's weights (and patch) landed; everyone is done with step g - 1
        {
            constexpr int J = (I + S - 1) % 9;                 // step g + S - 1 = (block cbj, tap J) -> the stage step g - 1 occupied
            const int cbj = cb + (I + S - 1) / 9;
            issue_w(S == 3 ? J % 3 : (cbj + J) & 1, cbj, kS2Kh[J] * 3 + kS2Kw[J]);       // stage of a step: (9 cb + tap) % S
        }
        if constexpr (I == 0) issue_patch(cb + 1);
        const unsigned char* const wst = fa + (S == 3 ? I % 3 : (cb + I) & 1) * RBYTES;
        const unsigned char* const pst = smem + (cb & 1) * PBYTES;
        if constexpr (group_start) {
#pragma unroll
            for (int j = 0; j < PT; ++j) {
                const int prow = (wp * PT + j + dh) * S2_PW + (lrow + dw);
                const unsigned char* const rowp = pst + prow * GROWB;
                const int sw = (prow >> 1) & 7;
                bq[0][j] = *(const uint4*)(rowp + ((lgrp ^ sw) << 4));
                bq[1][j] = *(const uint4*)(rowp + (((lgrp + 4) ^ sw) << 4));
            }
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            uint4 aq[CT];
#pragma unroll
            for (int c = 0; c < CT; ++c) aq[c] = *(const uint4*)(wst + c * 16 * GROWB + (((lgrp + 4 * half) ^ sw_w) << 4));
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int j = 0; j < PT; ++j) Mma<T>::run(aq[c], bq[half][j], acc[cls][c][j]);
        }
    };
    issue_patch(0);
    issue_w(0, 0, kS2Kh[0] * 3 + kS2Kw[0]);
    if constexpr (S == 3) issue_w(1, 0, kS2Kh[1] * 3 + kS2Kw[1]);
    for (int cb = 0; cb < spt; ++cb) {
        step(std::integral_constant<int, 0>{}, cb); step(std::integral_constant<int, 1>{}, cb); step(std::integral_constant<int, 2>{}, cb);
        step(std::integral_constant<int, 3>{}, cb); step(std::integral_constant<int, 4>{}, cb); step(std::integral_constant<int, 5>{}, cb);
        step(std::integral_constant<int, 6>{}, cb); step(std::integral_constant<int, 7>{}, cb); step(std::integral_constant<int, 8>{}, cb);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wait_vm_barrier<0>();                                      // the trailing all-zero DMA has landed; the LDS is free
    if constexpr (ACC) {
        // dx += ...: the four class tiles of the previous dx come in by LDS-DMA as whole 128-byte rows (the register-layout pre-pass of
        // igemm2_epilogue reads 8 bytes per lane from 16 different rows per instruction — on the every-other-pixel rows of a parity
        // class that cost 60 us on the 64->128 layer), in the swizzled image the epilogue's transpose uses; then every lane adds
        // its 4-channel pieces (same arithmetic and rounding as the register pre-pass)
        constexpr int CPR = BN / 8, RPS = NW * 64 / CPR, ORB = BN * 2;
        static_assert(4 * BM * ORB <= 2 * PBYTES + S * RBYTES && CPR == 8, "the four previous tiles must fit the LDS");
        u32x4 rsC;
        {
            const unsigned long long pc = (unsigned long long)p.C;
            rsC = u32x4{(unsigned)pc, (unsigned)(pc >> 32) & 0xffffu, p.bytesC, 0x00020000u};
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int i = 0; i < BM / RPS; ++i) {
                const int row = r + i * RPS;                   // (r = t >> 3: the row of this thread's 16-byte slot, qs its slot)
                const int gh = row >> 4, gw = row & 15;
                const unsigned pix = (unsigned)((n * p.Ho + 2 * (i0 + gh) + (q >> 1)) * p.Wo + 2 * (j0 + gw) + (q & 1));
                const int co = n0 + ((qs ^ (row & 7)) << 3);
                lds_dma16(rsC, wave_lds + (unsigned)(q * BM * ORB + i * RPS * ORB), co < p.Cst ? (pix * (unsigned)p.ldc + (unsigned)co) * ES : 0xFFFFFFFFu);
                __builtin_amdgcn_sched_barrier(0);
            }
        wait_vm_barrier<0>();
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < PT; ++j) {
                const int row = wp * (BM / WP) + j * 16 + lrow;
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const int ch = wc * BNW + c * 16 + lgrp * 4;
                    const uint2 q2 = *(const uint2*)(smem + q * BM * ORB + row * ORB + ((((ch >> 3) ^ (row & 7))) << 4) + ((ch & 4) << 1));
                    acc[q][c][j] += f32x4{__uint_as_float(q2.x << 16), __uint_as_float(q2.x & 0xffff0000u),
                                          __uint_as_float(q2.y << 16), __uint_as_float(q2.y & 0xffff0000u)};
                }
                __builtin_amdgcn_sched_barrier(0);             // (all sixteen reads hoisted in front of the adds spill 50 registers)
            }
        __syncthreads();                                       // every lane has its pieces before the epilogues reuse the LDS
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q) __syncthreads();                                // the previous class's store pass has read the scratch
        igemm2_epilogue<BM, BN, NW, WP, false, false>(p, acc[q], smem, 0, n0, mtile, BM, 16, 8, n * p.Ho + 2 * i0 + (q >> 1), 2 * j0 + (q & 1), nullptr,
                                        true);                 // (ACC: the previous contents are in the accumulators already; otherwise the
                                                               //  launcher guarantees accumulate == 0: no register-layout pre-pass either way)
    }
}

// ------------------------------------------------------------------------------------------------------
// Point-wise (1x1, stride 1) convolutions with a short K (row = 128..512 bytes of K) on large pixel counts.
// These layers are HBM-bound (2 bytes in + 2 bytes out per MAC row) and the tiled kernel above runs them at ~45 % of
// the HBM rate: with 2..4 K-steps a CTA is three dependent memory round trips (load, load, store) and two CTAs per CU
// cannot cover them.  This kernel streams instead:
//   * weight-stationary: the whole [Cout][K] weight matrix is copied to LDS once per CTA (XOR-swizzled 16-byte chunks,
//     conflict-free ds_read_b128 fragments), CTAs are persistent over a CONTIGUOUS range of block_m pixels;
//   * activations never touch LDS: a lane loads its MFMA B-operand chunks (pixel = lane & 15, 16 bytes of K per lane
//     group) straight from global memory, NB pixel tiles in flight per wave => no barrier in the main loop;
//   * a wave owns 16 pixels x (CT*16) output channels per step: stores 8/16 B per lane into the NHWC rows;
//   * BN partials: per-lane (count, sum, sum of squares) over the wave's few tiles (n <= block_m/(16*WP): no
//     cancellation at that size), converted to (mean, M2) and Chan-merged over the 16 pixel lanes with the transposing
//     butterfly, then over the CTA's pixel waves through LDS => the same [grid_m][2][C] (sum, M2) contract.
// ------------------------------------------------------------------------------------------------------
struct PwArgs {
    const void* X; const void* W; void* Y; float* stats;
    int M, lda, ldc, Cout, WN, accumulate, block_m, stats_ld, stats_atomic;
    unsigned bytesX, ldw_bytes, bytesY;
    int tstore;          // 1: stores go through a per-wave LDS transpose (16 bytes per lane, whole pixel rows per instruction)
};

template <typename T, int RB, int CT, int NW, bool TS, bool ACC = false, bool STATS = true>
__global__ __launch_bounds__(NW * 64) void pw_kernel(const PwArgs p) {
    constexpr int ES = sizeof(T);
    constexpr int J = RB / 64;                  // fragment groups per K row (each = 4 lane-group chunks of 16 B)
    constexpr int CPR = RB / 16;                // chunks per row
    // pixel tiles in flight per wave (register budget; 512-byte rows x 128-channel waves with statistics AND transposed stores: one less)
    constexpr int NB = (J >= 8) ? ((CT == 8 && ((STATS && (TS || ACC)) || (TS && ACC))) ? 2 : 3) : 4;
    constexpr int NV = CT * 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sW = smem;                                      // [Cout][RB], chunk q of row r at slot q ^ sw(r)
    float* sred = (float*)(smem + (size_t)p.Cout * RB);            // [WP][Cout][2] (mean, M2) + [WP] counts
    unsigned char* const stage = smem + (size_t)p.Cout * RB;       // TS: per-wave transposed store tiles, the SAME bytes (dead after the
                                                                   // main loop; a barrier separates the two uses) — 256 x 256 weights
                                                                   // (128 KB) + 32 KB of tiles is exactly the CU's 160 KB
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int WN = p.WN, WP = NW / WN;
    const int wc = wave % WN, wp = wave / WN;
    const int lrow = lane & 15, lgrp = lane >> 4;
    const int m_begin = blockIdx.x * p.block_m;
    const int m_end = min(p.M, m_begin + p.block_m);
    const int ntiles = (m_end - m_begin + 15) >> 4;
    const int nsteps = (ntiles + WP - 1) / WP;
    const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc((void*)p.X, 0, p.bytesX, 0x00020000);
    const unsigned rowbytes = (unsigned)(p.lda * ES);

    uint4 bq[NB][J];
    auto load = [&](int i, uint4 (&b)[J]) {
        const int m = m_begin + ((i * WP + wp) << 4) + lrow;
        const bool ok = m < m_end;
        const unsigned base = (unsigned)m * rowbytes + (unsigned)(lgrp << 4);
#pragma unroll
        for (int j = 0; j < J; ++j) {
            u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsX, ok ? base + j * 64 : 0xFFFFFFFFu, 0, 0);      // (cache-policy bits 0; nt measured: see DESIGN.md)
            b[j] = make_uint4(v.x, v.y, v.z, v.w);
        }
    };
    // The weights go FIRST and by LDS-DMA (a wave instruction = 1 KiB of the image = 1024 / RB rows; the lane at slot s of row r
    // fetches the logical chunk s ^ sw(r): the swizzle moves to the source address), the first NB activation tiles behind them.
    // Memory operations return in order: issued the other way round (round 3) the weights queued behind NB x J x 1 KiB per wave
    // — 192 KB per CU, HALF of a 256 -> 256 @ 80^2 layer's input chip-wide — and the first MFMA waited for all of it: load,
    // multiply and store phases ran one after the other.
    {
        const unsigned long long pwg = (unsigned long long)p.W;
        const u32x4 rsW = u32x4{(unsigned)pwg, (unsigned)(pwg >> 32) & 0xffffu, (unsigned)p.Cout * p.ldw_bytes, 0x00020000u};
        const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
        const int uw = __builtin_amdgcn_readfirstlane(wave);
        constexpr int RPI = 1024 / RB;                        // rows per DMA instruction
        const int ninstr = (p.Cout * RB) >> 10;
        for (int k = uw; k < ninstr; k += NW) {
            const int r = k * RPI + lane / CPR, sl = lane & (CPR - 1);
            const int sw = CPR == 8 ? (r >> 1) & 7 : r & 15;
            lds_dma16(rsW, lds0 + (unsigned)k * 1024u, (unsigned)r * p.ldw_bytes + (unsigned)((sl ^ sw) << 4));
        }
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) load(u, bq[u]);                    // (tiles beyond the range are out-of-range offsets: zeros, no traffic)
    wait_vm_barrier<NB * J>();                                      // own DMAs landed (only the NB * J younger loads may be outstanding), then everyone's

    const int co0 = wc * CT * 16;
    const unsigned char* const wbase = sW + (co0 + lrow) * RB;
    const int swr = CPR == 8 ? (lrow >> 1) & 7 : lrow;
    T* const Yg = (T*)p.Y;
    // TS && ACC && STATS (round 5: the accumulating forward launch of the commuted Concat + 1x1 Conv, y += W a with statistics): the final
    // values exist in the ROW layout of the transposed store (a lane = 16 bytes = 8 channels of one pixel, always the same 8 channels),
    // so the statistics are per-lane (sum, sum of squares) of 8 channels there: 16 registers instead of 2 x CT x 4.
    constexpr bool ROWSTATS = TS && ACC && STATS && sizeof(T) == 2;
    float s1[ROWSTATS ? 8 : NV], s2[ROWSTATS ? 8 : NV];
#pragma unroll
    for (int v = 0; v < (ROWSTATS ? 8 : NV); ++v) { s1[v] = 0.f; s2[v] = 0.f; }
    float cnt = 0.f;
    const bool want_stats = STATS && p.stats != nullptr;      // (STATS = false: the input-gradient launches — 2 x CT x 4 registers less)

    // Steady loop of the non-accumulating launches: NO control flow and no exec-masked memory operation.  gfx950 counts loads and
    // stores in one in-order counter (vmcnt); behind a conditional prefetch (`if (i + NB < nsteps) load`) or an exec-masked store the
    // compiler no longer knows how many operations are outstanding, assumes the fewest and waits with vmcnt(7..0) for a tile's
    // loads — which also waits for every YOUNGER-but-one prefetch: the NB tiles "in flight" were one (tools/asm_loops.py; round 4).
    // Here every wave runs a multiple of NB steps, tiles beyond its range are out-of-range buffer offsets (loads return zeros,
    // stores are dropped, neither moves data), and the waits come out as vmcnt(NB * J + ...) as intended.
    {
        // (ACC: the previous contents of the output tile are FETCHED BEFORE the tile's MFMAs and the prefetch of tile i + NB — in the
        //  in-order memory counter they are older than the prefetch, so waiting for them leaves the NB x J younger loads in flight;
        //  fetched after the MFMAs, as the round-3 loop did, the wait drained the whole pipeline)
        const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc((void*)p.Y, 0, p.bytesY, 0x00020000);
        constexpr int NCH = CT * 16 * ES / 16;          // TS: 16-byte chunks per tile row
        constexpr int RPP = 64 / NCH;                   // TS: rows per store instruction
        auto step = [&](int i, uint4 (&b)[J], bool prefetch) {
            asm volatile("" ::: "memory");             // the weight fragments are re-read from LDS every step: without this fence the
                                                       // compiler hoists all J*CT loop-invariant ds_reads into registers (+128 VGPRs)
            const int tile_m = m_begin + ((i * WP + wp) << 4);
            u32x4 old_ts[TS ? 16 / RPP : 1];
            u32x4 old_d4[(!TS && sizeof(T) == 4) ? CT : 1];
            u32x2 old_d2[(!TS && sizeof(T) == 2) ? CT : 1];
            if constexpr (ACC) {
                if constexpr (TS) {
#pragma unroll
                    for (int ps = 0; ps < 16 / RPP; ++ps) {
                        const int row = ps * RPP + lane / NCH, ch = lane % NCH;
                        const unsigned off = ((unsigned)(tile_m + row) * (unsigned)p.ldc + (unsigned)co0) * ES + (unsigned)(ch << 4);
                        old_ts[ps] = __builtin_amdgcn_raw_buffer_load_b128(rsY, tile_m + row < m_end ? off : 0xFFFFFFFFu, 0, 0);
                    }
                } else {
                    const int m = tile_m + lrow;
                    const unsigned off = m < m_end ? ((unsigned)m * (unsigned)p.ldc + (unsigned)(co0 + lgrp * 4)) * ES : 0xFFFFFFFFu;
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        if constexpr (sizeof(T) == 4) old_d4[c] = __builtin_amdgcn_raw_buffer_load_b128(rsY, off, c * 16 * ES, 0);
                        else old_d2[c] = __builtin_amdgcn_raw_buffer_load_b64(rsY, off, c * 16 * ES, 0);
                    }
                }
            }
            f32x4 acc[CT];
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int koff = (((j << 2) | lgrp) ^ swr) << 4;
                uint4 af[CT];
#pragma unroll
                for (int c = 0; c < CT; ++c) af[c] = *(const uint4*)(wbase + c * 16 * RB + koff);
#pragma unroll
                for (int c = 0; c < CT; ++c) Mma<T>::run(af[c], b[j], acc[c]);
            }
            if (prefetch) load(i + NB, b);
            if constexpr (TS) {
                // The accumulator layout gives a lane 4 consecutive channels of one pixel: a direct store writes a pixel row
                // in 8-byte pieces from CT different instructions.  Transposed through a wave-private LDS tile (no barrier: one
                // wave's LDS operations complete in order) every lane stores 16 bytes and NCH neighbouring lanes one whole row.
                unsigned char* tb = stage + wave * (16 * NCH * 16);
                const int swm = (NCH - 1) & 15;
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    if constexpr (sizeof(T) == 4) {
                        const int ch = c * 4 + lgrp;
                        *(float4*)(tb + lrow * (NCH * 16) + ((ch ^ (lrow & swm)) << 4)) = make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
                    } else {
                        const int ch = c * 2 + (lgrp >> 1);
                        uint2 w2;
                        w2.x = (uint32_t)f2bf(acc[c][0]) | ((uint32_t)f2bf(acc[c][1]) << 16);
                        w2.y = (uint32_t)f2bf(acc[c][2]) | ((uint32_t)f2bf(acc[c][3]) << 16);
                        *(uint2*)(tb + lrow * (NCH * 16) + ((ch ^ (lrow & swm)) << 4) + ((lgrp & 1) << 3)) = w2;
                    }
                }
#pragma unroll
                for (int ps = 0; ps < 16 / RPP; ++ps) {
                    const int row = ps * RPP + lane / NCH, ch = lane % NCH;
                    uint4 v4 = *(const uint4*)(tb + row * (NCH * 16) + ((ch ^ (row & swm)) << 4));
                    if constexpr (ACC) {          // gradient fan-in: whole 16-byte read-modify-write rows (launcher: bf16, no statistics)
                        float a8[16 / ES], o8[16 / ES];
                        unpack16<T>(v4, a8);
                        unpack16<T>(make_uint4(old_ts[ps].x, old_ts[ps].y, old_ts[ps].z, old_ts[ps].w), o8);
#pragma unroll
                        for (int e = 0; e < 16 / ES; ++e) a8[e] += o8[e];
                        v4 = pack16<T>(a8);
                        if constexpr (ROWSTATS) {          // rows beyond the range: contribution and old value are both zeros
                            if (want_stats) {
#pragma unroll
                                for (int e = 0; e < 8; ++e) { s1[e] += a8[e]; s2[e] = fmaf(a8[e], a8[e], s2[e]); }
                            }
                        }
                    }
                    const unsigned off = ((unsigned)(tile_m + row) * (unsigned)p.ldc + (unsigned)co0) * ES + (unsigned)(ch << 4);
                    __builtin_amdgcn_raw_buffer_store_b128(u32x4{v4.x, v4.y, v4.z, v4.w}, rsY, tile_m + row < m_end ? off : 0xFFFFFFFFu, 0, 0);
                }
            } else {
                const int m = tile_m + lrow;
                const unsigned off = m < m_end ? ((unsigned)m * (unsigned)p.ldc + (unsigned)(co0 + lgrp * 4)) * ES : 0xFFFFFFFFu;
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    if constexpr (sizeof(T) == 4) {
                        if constexpr (ACC) {
                            acc[c][0] += __uint_as_float(old_d4[c].x); acc[c][1] += __uint_as_float(old_d4[c].y);
                            acc[c][2] += __uint_as_float(old_d4[c].z); acc[c][3] += __uint_as_float(old_d4[c].w);
                        }
                        __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(acc[c][0]), __float_as_uint(acc[c][1]), __float_as_uint(acc[c][2]),
                                                                     __float_as_uint(acc[c][3])}, rsY, off, c * 16 * ES, 0);
                    } else {
                        if constexpr (ACC) {
                            acc[c][0] += __uint_as_float(old_d2[c].x << 16); acc[c][1] += __uint_as_float(old_d2[c].x & 0xffff0000u);
                            acc[c][2] += __uint_as_float(old_d2[c].y << 16); acc[c][3] += __uint_as_float(old_d2[c].y & 0xffff0000u);
                        }
                        u32x2 w2;
                        w2.x = (uint32_t)f2bf(acc[c][0]) | ((uint32_t)f2bf(acc[c][1]) << 16);
                        w2.y = (uint32_t)f2bf(acc[c][2]) | ((uint32_t)f2bf(acc[c][3]) << 16);
                        __builtin_amdgcn_raw_buffer_store_b64(w2, rsY, off, c * 16 * ES, 0);
                    }
                }
            }
            if (!ROWSTATS && want_stats) {       // statistics of the stored f32 values (including an accumulated y); rows beyond the range are zeros
#pragma unroll
                for (int c = 0; c < CT; ++c)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        s1[c * 4 + e] += acc[c][e];
                        s2[c * 4 + e] = fmaf(acc[c][e], acc[c][e], s2[c * 4 + e]);
                    }
                cnt += (tile_m + lrow < m_end) ? 1.f : 0.f;
            }
        };
        const int nfull = nsteps / NB * NB;
        for (int i0 = 0; i0 < nfull; i0 += NB) {
#pragma unroll
            for (int u = 0; u < NB; ++u) step(i0 + u, bq[u], true);
        }
#pragma unroll
        for (int u = 0; u < NB - 1; ++u)                    // the last nsteps % NB tiles (their loads were issued above; nothing follows them)
            if (nfull + u < nsteps) step(nfull + u, bq[u], false);
    }

    if constexpr (ROWSTATS) {
        if (want_stats) {
            constexpr int NCH = CT * 16 * ES / 16;
            // lanes with equal (lane % NCH) hold the same 8 channels: butterfly over the others, then the pixel waves through LDS
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int o = NCH; o < 64; o <<= 1) { s1[e] += __shfl_xor(s1[e], o, 64); s2[e] += __shfl_xor(s2[e], o, 64); }
            __syncthreads();                                  // every wave is done with its store tiles: sred takes their place
            if (lane < NCH) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int ch = wc * CT * 16 + lane * 8 + e;
                    sred[((size_t)wp * p.Cout + ch) * 2] = s1[e];
                    sred[((size_t)wp * p.Cout + ch) * 2 + 1] = s2[e];
                }
            }
            __syncthreads();
            for (int ch = t; ch < p.Cout; ch += NW * 64) {
                float a = 0.f, b = 0.f;
                for (int w = 0; w < WP; ++w) { a += sred[((size_t)w * p.Cout + ch) * 2]; b += sred[((size_t)w * p.Cout + ch) * 2 + 1]; }
                if (p.stats_atomic) {
                    float* dst = p.stats + (size_t)(blockIdx.x & (YDL_BN_REPLICAS - 1)) * 2 * p.stats_ld;
                    atomicAdd(dst + ch, a);
                    atomicAdd(dst + p.stats_ld + ch, b);
                } else {                                      // partial-row contract: (sum, M2) of this block's m_end - m_begin values
                    const float n = (float)(m_end - m_begin);
                    float* dst = p.stats + (size_t)blockIdx.x * 2 * p.stats_ld;
                    dst[ch] = a;
                    dst[p.stats_ld + ch] = fmaxf(b - a * a / fmaxf(n, 1.f), 0.f);
                }
            }
        }
        return;
    }
    if (want_stats) {
        if constexpr (TS) __syncthreads();                   // every wave is done with its store tiles: sred takes their place
        // per-lane (count, mean, M2), then Chan-merge over the 16 pixel lanes: stage s pairs lanes that differ in bit s;
        // the lane whose bit is 0 keeps the even-indexed aggregates, its partner the odd ones (live values halve).
        float mean[NV], m2[NV];
        {
            const float rn = cnt > 0.f ? 1.f / cnt : 0.f;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                mean[v] = s1[v] * rn;
                m2[v] = fmaxf(s2[v] - s1[v] * mean[v], 0.f);
            }
        }
        int live = NV;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int mask = 1 << s;
            const bool hi = (lrow >> s) & 1;
            const float cnt_o = __shfl_xor(cnt, mask, 64);
            const float tot = cnt + cnt_o;
            const float rt = tot > 0.f ? 1.f / tot : 0.f;
            const float fo = cnt_o * rt, fx = cnt * cnt_o * rt;
            if (live > 1) {
#pragma unroll
                for (int k = 0; k < NV / 2; ++k)
                    if (k < live / 2) {
                        const float km = hi ? mean[2 * k + 1] : mean[2 * k], sm = hi ? mean[2 * k] : mean[2 * k + 1];
                        const float kq = hi ? m2[2 * k + 1] : m2[2 * k], sq = hi ? m2[2 * k] : m2[2 * k + 1];
                        const float om = __shfl_xor(sm, mask, 64), oq = __shfl_xor(sq, mask, 64);
                        const float d = om - km;
                        mean[k] = km + d * fo;
                        m2[k] = kq + oq + d * d * fx;
                    }
                live >>= 1;
            } else {
                const float om = __shfl_xor(mean[0], mask, 64), oq = __shfl_xor(m2[0], mask, 64);
                const float d = om - mean[0];
                mean[0] = mean[0] + d * fo;
                m2[0] = m2[0] + oq + d * d * fx;
            }
            cnt = tot;
        }
        // slot tt of lane lrow now holds value index (tt << 4 | lrow)  (NV >= 16), channel = co0 + (idx>>2)*16 + lgrp*4 + (idx&3)
        float* scnt = sred + (size_t)WP * p.Cout * 2;
#pragma unroll
        for (int tt = 0; tt < NV / 16; ++tt) {
            const int idx = (tt << 4) | lrow;
            const int ch = co0 + (idx >> 2) * 16 + lgrp * 4 + (idx & 3);
            sred[((size_t)wp * p.Cout + ch) * 2] = mean[tt];
            sred[((size_t)wp * p.Cout + ch) * 2 + 1] = m2[tt];
        }
        if (lane == 0 && wc == 0) scnt[wp] = cnt;
        __syncthreads();
        for (int ch = t; ch < p.Cout; ch += NW * 64) {
            float n = 0.f, mu = 0.f, q2 = 0.f;
            for (int w = 0; w < WP; ++w) {
                const float nb = scnt[w];
                const float mb = sred[((size_t)w * p.Cout + ch) * 2], qb = sred[((size_t)w * p.Cout + ch) * 2 + 1];
                const float tot = n + nb;
                const float rt = tot > 0.f ? 1.f / tot : 0.f;
                const float d = mb - mu;
                mu = mu + d * nb * rt;
                q2 = q2 + qb + d * d * n * nb * rt;
                n = tot;
            }
            if (p.stats_atomic) {
                float* dst = p.stats + (size_t)(blockIdx.x & (YDL_BN_REPLICAS - 1)) * 2 * p.stats_ld;
                atomicAdd(dst + ch, mu * n);
                atomicAdd(dst + p.stats_ld + ch, q2 + n * mu * mu);
            } else {
                float* dst = p.stats + (size_t)blockIdx.x * 2 * p.stats_ld;
                dst[ch] = mu * n;
                dst[p.stats_ld + ch] = q2;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// Thin-input 3x3 convolution: the stem after its space-to-depth rewrite (16 stored input channels -> 64 output channels,
// stride 1, pad 1; BASELINE config 2: 16 x 320 x 320 pixels).  K = 9 taps x 16 channels = 144: with 64-deep K-steps the tiled
// kernel spends its time on 16-byte-per-row gathers through LDS for 2.25 K-steps of work and runs at 1.9 TB/s of a layer whose
// bytes (52 MB in, 210 MB out) are all it costs.  Here, like the point-wise kernel:
//   * weight-stationary IN REGISTERS: a lane's MFMA A fragments of all 4 channel tiles x 5 K-slices (80 VGPRs) are loaded once;
//   * activations go global -> registers in the MFMA B layout: K-slice s = taps 2s and 2s+1, a lane (pixel = lane & 15,
//     k-group = lane >> 4) reads the 16-byte half (k-group & 1) of tap 2s + (k-group >> 1) at its pixel — 16 pixels x 32 bytes
//     contiguous per tap, range-checked buffer loads return zeros for the padding taps; the next tile's five loads are in
//     flight while the current tile's 20 MFMAs issue; no LDS, no barrier in the main loop;
//   * a wave owns 16 consecutive pixels of one image row per step (Wo % 16 == 0), output through a per-wave LDS transpose
//     into whole 128-byte NHWC rows, per-lane (sum, sum of squares) for the BN statistics, reduced once per CTA.
// ------------------------------------------------------------------------------------------------------
struct StemArgs {
    const bf16_t* X; const bf16_t* W; bf16_t* Y; float* stats;
    int H, Wd, ldc, M, block_m, stats_ld, stats_atomic;
    unsigned bytesX;
};
struct StemPlan { bool ok; int block_m, grid_m; };
static int g_stem_enabled = 1;
static StemPlan stem_plan(int M, int Wo) {
    StemPlan pl{};
    pl.ok = g_stem_enabled && Wo % 16 == 0 && M >= 4096;
    if (!pl.ok) return pl;
    const int slots = ydl_device_cus() * 3;
    pl.block_m = round_up((M + slots - 1) / slots, 64);
    pl.grid_m = (M + pl.block_m - 1) / pl.block_m;
    return pl;
}

#define STEM_ROWB 144       // LDS transpose rows: 128 data bytes + 16 (a wave's 8-byte writes of 16 rows spread over the banks)
__global__ __launch_bounds__(256, 2) void stem_kernel(const StemArgs p) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[4 * 16 * STEM_ROWB];
    __shared__ float red[4 * 64 * 2];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int lrow = lane & 15, lgrp = lane >> 4;
    const int chunk = lgrp & 1, tsel = lgrp >> 1;
    // weights: A fragment (ct, s) = w[ct*16 + lrow][tap 2s + tsel][chunk*8 .. +8]; tap 9 does not exist (zeros)
    uint4 af[4][5];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int sl = 0; sl < 5; ++sl) {
            const int tap = 2 * sl + tsel;
            af[ct][sl] = tap < 9 ? *(const uint4*)(p.W + ((size_t)(ct * 16 + lrow) * 9 + tap) * 16 + chunk * 8) : make_uint4(0, 0, 0, 0);
        }
    int dh[5], dw[5];
#pragma unroll
    for (int sl = 0; sl < 5; ++sl) {
        const int tap = 2 * sl + tsel;
        dh[sl] = tap < 9 ? tap / 3 - 1 : 100000;         // the missing tap is always out of range
        dw[sl] = tap < 9 ? tap % 3 - 1 : 0;
    }
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.X, 0, p.bytesX, 0x00020000);
    const int HW = p.H * p.Wd;
    const int m_begin = blockIdx.x * p.block_m;
    const int m_end = min(p.M, m_begin + p.block_m);
    float s1[16], s2[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { s1[i] = 0.f; s2[i] = 0.f; }

    auto load_tile = [&](int m0, uint4 (&b)[5]) {
        // m0: first pixel of a 16-pixel tile inside one image row (wave-uniform)
        const int n = m0 / HW;
        const int rem = m0 - n * HW;
        const int h = rem / p.Wd;
        const int w = rem - h * p.Wd + lrow;
#pragma unroll
        for (int sl = 0; sl < 5; ++sl) {
            const int ih = h + dh[sl], iw = w + dw[sl];
            const bool ok = m0 < m_end && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.Wd;
            const unsigned off = ok ? (unsigned)(((n * p.H + ih) * p.Wd + iw) * 32 + chunk * 16) : 0xFFFFFFFFu;
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
            b[sl] = make_uint4(v.x, v.y, v.z, v.w);
        }
    };
    unsigned char* my_stage = stage + wave * (16 * STEM_ROWB);
    uint4 bc[5], bn[5];
    int m0 = m_begin + wave * 16;
    load_tile(m0, bc);
    for (; m0 < m_end; m0 += 64) {
        load_tile(m0 + 64, bn);                      // (beyond m_end: every lane out of range)
        f32x4 acc[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sl = 0; sl < 5; ++sl)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) Mma<bf16_t>::run(af[ct][sl], bc[sl], acc[ct]);
        // lane: pixel m0 + lrow, channels ct*16 + lgrp*4 + e
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = acc[ct][e];
                s1[ct * 4 + e] += v;
                s2[ct * 4 + e] += v * v;
            }
            uint2 u;
            u.x = (uint32_t)f2bf(acc[ct][0]) | ((uint32_t)f2bf(acc[ct][1]) << 16);
            u.y = (uint32_t)f2bf(acc[ct][2]) | ((uint32_t)f2bf(acc[ct][3]) << 16);
            *(uint2*)(my_stage + lrow * STEM_ROWB + (ct * 16 + lgrp * 4) * 2) = u;
        }
        // (LDS instructions of one wave execute in order: the reads below see the writes above)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int slot = lane + 64 * i;
            const int row = slot >> 3, ch = slot & 7;
            const uint4 v = *(const uint4*)(my_stage + row * STEM_ROWB + ch * 16);
            *(uint4*)(p.Y + (size_t)(m0 + row) * p.ldc + ch * 8) = v;
        }
#pragma unroll
        for (int sl = 0; sl < 5; ++sl) bc[sl] = bn[sl];
    }
    // statistics: sum over the 16 pixel lanes (transposing butterfly), then over the CTA's 4 waves
    row_reduce<16>(s1, lrow);
    row_reduce<16>(s2, lrow);
    {
        const int ch = (lrow >> 2) * 16 + lgrp * 4 + (lrow & 3);     // value index lrow = ct*4 + e of this lane group
        red[(wave * 64 + ch) * 2] = s1[0];
        red[(wave * 64 + ch) * 2 + 1] = s2[0];
    }
    __syncthreads();
    if (p.stats != nullptr && t < 64) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) { a += red[(w * 64 + t) * 2]; b += red[(w * 64 + t) * 2 + 1]; }
        if (p.stats_atomic) {
            float* dst = p.stats + (size_t)(blockIdx.x & (YDL_BN_REPLICAS - 1)) * 2 * p.stats_ld;
            atomicAdd(dst + t, a);
            atomicAdd(dst + p.stats_ld + t, b);
        } else {
            const float n = (float)(m_end - m_begin);
            float* dst = p.stats + (size_t)blockIdx.x * 2 * p.stats_ld;
            dst[t] = a;
            dst[p.stats_ld + t] = fmaxf(b - a * a / n, 0.f);          // (sum, M2) of this block's pixels
        }
    }
}

static bool args_stem(const IgemmArgs& a) {
    if (!(a.ntaps == 9 && a.Ttot == 9 && a.Kc == 16 && a.lda == 16 && a.Cout == 64 && a.Cst == 64 && a.in_mul == 1 && a.out_mul == 1 &&
          a.ncls <= 1 && a.Hi == a.Ho && a.Wi == a.Wo && a.Hg == a.Ho && a.Wg == a.Wo && a.out_h0 == 0 && a.out_w0 == 0 &&
          a.accumulate == 0 && a.ldb_bytes == 9u * 16u * 2u))
        return false;
    for (int tp = 0; tp < 9; ++tp)
        if (a.dh[tp] != tp / 3 - 1 || a.dw[tp] != tp % 3 - 1 || a.wt[tp] != tp) return false;
    return true;
}

struct PwPlan { bool ok; int RB, CT, WN, NW, block_m, grid_m; size_t smem, tstage; };
static int g_pw_enabled = 1;
static int g_pw_acc_ts = -1;     // ydl_debug_set key 14: accumulating point-wise launches: 1 transposed stores (statistics in the row layout),
                                 // 2 transposed stores only without statistics, 0 direct stores; -1 = the default, 1
static int g_dgrad_merge = 1;
// eligibility + launch geometry; a pure function of its arguments (the stats-workspace queries call it too)
static PwPlan pw_plan(int M, int Kc, int Cout, int Cst, int es, bool pointwise) {
    PwPlan pl{};
    pl.ok = false;
    if (!g_pw_enabled || !pointwise || Cst != Cout || M < 65536) return pl;
    const int RB = Kc * es;
    if (RB != 128 && RB != 256 && RB != 512) return pl;
    if (Cout != 64 && Cout != 128 && Cout != 256) return pl;
    const long wbytes = (long)Cout * RB;
    if (wbytes > 128 * 1024) return pl;
    pl.RB = RB;
    // bf16: waves of 64 output channels instead of 128 wherever the weight matrix is at most 64 KB (tools/conv_bench.py: 128->128
    // @160^2 forward 59.4 -> 53.1 us, dgrad 53.1 -> 47.7; 128->256 @80^2 38.5 -> 27.6; 256->128 @80^2 29.6 -> 26.7; 64->128 @160^2
    // 40.3 -> 39.3) — but not 256->256 on 512-byte rows (42 -> 58 us: four waves would each fetch the whole activation tile).
    const bool split = es == 2 && (Cout == 128 || (Cout == 256 && RB <= 256));
    pl.CT = (Cout >= 128 && !split) ? 8 : 4;
    pl.WN = Cout / (pl.CT * 16);
    // 512-byte rows x 128+ channels need ~230 VGPRs: as 4-wave CTAs that is one wave per SIMD; one 8-wave CTA per CU
    // gives two
    pl.NW = (RB == 512 && pl.CT == 8) ? 8 : 4;
    const int slots = ydl_device_cus() * (pl.NW == 4 ? 2 : 1);      // CTAs per CU: the 4-wave forms are sized for two
    int bm = round_up((M + slots - 1) / slots, 16);
    pl.block_m = bm;
    pl.grid_m = (M + bm - 1) / bm;
    const int WP = pl.NW / pl.WN;
    pl.smem = (((size_t)wbytes + (size_t)WP * Cout * 2 * sizeof(float) + 64 + 15) & ~(size_t)15);      // direct stores: weights + reduction scratch
    pl.tstage = (size_t)pl.NW * 16 * (pl.CT * 16 * es);      // per-wave transposed store tiles (the reduction scratch aliases them)
    pl.ok = true;
    return pl;
}

template <typename T, int RB, int CT, int NW>
static int launch_pw_cfg(const PwArgs& a, const PwPlan& pl, hipStream_t st, int fam) {
    PwArgs a2 = a;
    // (bf16 only: the f32 instantiations lose an occupancy step or spill with the extra staging code; parity mode keeps direct stores)
    // (an accumulating launch takes the transposed path when it carries no statistics: the input-gradient fan-in.  Its own
    //  contribution is rounded to bf16 in the staging tile before the add — one rounding more than the direct path.)
    const int acc_ts = g_pw_acc_ts >= 0 ? g_pw_acc_ts : 1;       // ydl_debug_set key 14
    // measured per layer (tools/conv_bench.py dgrad --acc 1): faster everywhere (-8 ... -27 %) but on 256-byte K rows with 128-channel
    // wave tiles, where the direct read-modify-write wins (128->128 @160^2: 90 vs 111 us)
    // (round 5: with statistics too, bf16 — they are taken in the row layout of the transposed store, see ROWSTATS in the kernel;
    //  key 14 = 2 keeps the statistics launches on the direct path)
    const bool acc_ok = (a.stats == nullptr || (sizeof(T) == 2 && acc_ts == 1)) && acc_ts && !(RB == 256 && CT == 8);
    const size_t wbytes = (size_t)a.Cout * RB;
    const size_t ts_smem = wbytes + (pl.tstage > pl.smem - wbytes ? pl.tstage : pl.smem - wbytes);
    a2.tstore = (sizeof(T) == 2 && (!a.accumulate || acc_ok) && ts_smem <= 160 * 1024) ? 1 : 0;
    {
        // the store path is part of the recorded name: "ts" = per-wave LDS-transposed 16-byte stores, "direct" = register-layout stores
        static const std::string base = std::string("pw_kernel<") + (sizeof(T) == 4 ? "f32" : "bf16") + "," + std::to_string(RB) + "," +
                                        std::to_string(CT) + "," + std::to_string(NW);
        static const std::string nm_ts = base + ",ts>", nm_direct = base + ",direct>";
        ydl_note_kernel(fam, (a2.tstore ? nm_ts : nm_direct).c_str());
    }
    {
        const unsigned long long by = ((unsigned long long)(a.M - 1) * (unsigned long long)a.ldc + (unsigned long long)a.Cout) * sizeof(T);
        YDL_CHECK(by < 0xFFFFFFFFull, "point-wise output beyond the 4 GiB a buffer descriptor addresses");
        a2.bytesY = (unsigned)by;
    }
    const size_t sm = a2.tstore ? ts_smem : pl.smem;
#define PW_LAUNCH(TS_, ACC_, ST_)                                                     \
    do {                                                                              \
        YDL_SET_MAX_LDS((pw_kernel<T, RB, CT, NW, TS_, ACC_, ST_>), 160 * 1024);      \
        pw_kernel<T, RB, CT, NW, TS_, ACC_, ST_><<<pl.grid_m, NW * 64, sm, st>>>(a2); \
    } while (0)
    constexpr bool TS = sizeof(T) == 2;      // (the f32 kernels have no transposed-store form: tstore is 0 for them)
    if (a2.accumulate && a2.stats) {
        if (TS && a2.tstore) PW_LAUNCH(TS, true, true); else PW_LAUNCH(false, true, true);
    } else if (a2.accumulate) {
        if (TS && a2.tstore) PW_LAUNCH(TS, true, false); else PW_LAUNCH(false, true, false);
    } else if (a2.stats) {
        if (TS && a2.tstore) PW_LAUNCH(TS, false, true); else PW_LAUNCH(false, false, true);
    } else {
        if (TS && a2.tstore) PW_LAUNCH(TS, false, false); else PW_LAUNCH(false, false, false);
    }
#undef PW_LAUNCH
    YDL_LAUNCH_CHECK();
    return 0;
}

template <typename T>
static int launch_pw(const PwArgs& a, const PwPlan& pl, hipStream_t st, int fam) {
    if (pl.NW == 8) {
        YDL_CHECK(pl.RB == 512 && pl.CT == 8, "internal: unexpected point-wise plan");
        return launch_pw_cfg<T, 512, 8, 8>(a, pl, st, fam);
    }
    if constexpr (sizeof(T) == 4) {      // 128-channel waves on 128- and 256-byte rows: f32 only (pw_plan gives the bf16 layers 64-channel waves)
        if (pl.RB == 128 && pl.CT == 8) return launch_pw_cfg<T, 128, 8, 4>(a, pl, st, fam);
        if (pl.RB == 256 && pl.CT == 8) return launch_pw_cfg<T, 256, 8, 4>(a, pl, st, fam);
    }
    YDL_CHECK(pl.CT == 4, "internal: unexpected point-wise plan");
    if (pl.RB == 128) return launch_pw_cfg<T, 128, 4, 4>(a, pl, st, fam);
    if (pl.RB == 256) return launch_pw_cfg<T, 256, 4, 4>(a, pl, st, fam);
    return launch_pw_cfg<T, 512, 4, 4>(a, pl, st, fam);
}

static bool args_pointwise(const IgemmArgs& a) {
    return a.ntaps == 1 && a.Ttot == 1 && a.dh[0] == 0 && a.dw[0] == 0 && a.in_mul == 1 && a.out_mul == 1 && a.out_h0 == 0 &&
           a.out_w0 == 0 && a.Hg == a.Ho && a.Wg == a.Wo && a.Hi == a.Ho && a.Wi == a.Wo;
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
template <typename T, int BM, int BN, int NW = 4, int WP = 4>
static int launch_igemm(IgemmArgs a, hipStream_t st, int fam) {
    a.grid_n = (a.Cst + BN - 1) / BN;
    int mtiles = (a.M + BM - 1) / BM;
    if (a.ncls > 1) {
        int acc = 0;
        for (int c = 0; c < a.ncls; ++c) { a.cls_tile0[c] = acc; acc += (a.cls_M[c] + BM - 1) / BM; }
        a.cls_tile0[a.ncls] = acc;
        mtiles = acc;
    }
    dim3 grid(mtiles * a.grid_n);
    size_t smem = 2 * (BM + BN) * GROWB + 3 * MAXTAPS * sizeof(int);
    YDL_SET_MAX_LDS((igemm_kernel<T, BM, BN, NW, WP>), smem);
    {
        static const std::string nm = std::string("igemm_kernel<") + (sizeof(T) == 4 ? "f32" : "bf16") + "," + std::to_string(BM) + "," +
                                      std::to_string(BN) + "," + std::to_string(NW) + "," + std::to_string(WP) + ">";
        ydl_note_kernel(fam, nm.c_str());
    }
    igemm_kernel<T, BM, BN, NW, WP><<<grid, NW * 64, smem, st>>>(a);
    YDL_LAUNCH_CHECK();
    return 0;
}

// LDS-DMA ring instantiations (bf16): one row per instantiation pick_cfg can choose.  The plan, halo_ok, ring_has_bnred and the launchers
// all read this table.
enum RingId { RING_NONE, RING_128x128, RING_64x128, RING_128x64, RING_256x128_STG, RING_256x128_LOADERS, RING_128x128_LOADERS,
              RING_128x128_LOADERS_S2, RING_COUNT };
enum RingForm { FORM_RING, FORM_STAGGERED, FORM_LOADERS };      // igemm2_kernel, igemm2_kernel<..., STG>, igemm2l_kernel
struct RingCfg {
    int BM, BN;
    RingForm form;
    bool bnred;      // has an instantiation with the fused BatchNorm-backward reduce
    bool patch;      // a 3x3 / stride-1 layer that chose it may run on the patch-form kernels instead (halo_ok)
};
static const RingCfg kRing[RING_COUNT] = {
    {0, 0, FORM_RING, false, false},
    {128, 128, FORM_RING, true, true},           // 8 waves, 2 stages = 64 KB: two CTAs per CU
    {64, 128, FORM_RING, true, false},           // 4 waves of 32x64, 3 stages = 72 KB: two CTAs per CU (small M)
    {128, 64, FORM_RING, true, true},            // 8 waves of 32x32, 2 stages = 48 KB
    {256, 128, FORM_STAGGERED, false, true},     // 64x64 wave tiles, staggered halves, 3 stages = 144 KB: one CTA per CU
    {256, 128, FORM_LOADERS, false, true},       // 8 multipliers of 64x64 + 4 loaders, 3 stages = 144 KB
    {128, 128, FORM_LOADERS, false, false},      // 8 multipliers of 32x64 + 4 loaders, 3 stages = 96 KB
    {128, 128, FORM_LOADERS, false, true},       // 4 multipliers of 64x64 + 4 loaders, 2 stages: two CTAs (16 waves) per CU
};
// (measured and dropped — profiles/r5_ab_ring_loader_waves.log: 256 x 128 with two loaders 3..8 % behind four; 128 x 128 with two stages and two
//  CTAs per CU: four loaders = 24 waves = 80 registers, two loaders = 16 DMAs per loader and step — both 10..60 % slower.  256 x 256 tiles
//  spill 520..600 VGPRs.  DESIGN.md section 4 has the other forms that lost.)
static bool ring_has_bnred(int id) { return kRing[id].bnred; }

struct TileCfg { int BM, BN; int ring; };      // ring != RING_NONE: the kRing row (bf16 LDS-DMA ring), else the igemm_kernel tile
static int g_ring_loaders = -1;   // ydl_debug_set key 19: loader-wave ring kernel where it measured faster (-1: the default, on)
static int g_ring_enabled = 1;
static int g_ring_persist = 1;    // ydl_debug_set key 6

template <int BM, int BN, int NW, int WP, int S, bool RED = false, int STG = 0>
static int launch_igemm2(IgemmArgs a, hipStream_t st, int fam) {
    a.grid_n = (a.Cst + BN - 1) / BN;
    int mtiles = (a.M + BM - 1) / BM;
    if (a.ncls > 1) {
        int acc = 0;
        for (int c = 0; c < a.ncls; ++c) { a.cls_tile0[c] = acc; acc += (a.cls_M[c] + BM - 1) / BM; }
        a.cls_tile0[a.ncls] = acc;
        mtiles = acc;
    }
    dim3 grid(mtiles * a.grid_n);
    a.grid_m = mtiles;
    // the weight operand marks rows beyond Cout and K-steps beyond the end with a 0xF0000000 offset that must stay out of range
    // (>= bytesB) after the 32-bit additions of a row offset, a tap offset and a channel-block offset, each < bytesB
    YDL_CHECK(a.bytesB < 0x08000000u, "ring kernel: weight matrix of 128 MiB or more is not supported");
    {
        // tile order (speed only): which operand would be re-fetched from beyond L2?  channel-tile-fastest streams the whole
        // weight matrix once per pixel tile when it does not fit the XCD's L2; pixel-tile-fastest keeps one weight slab in
        // L2 and re-reads the activations once per channel tile
        const double wbytes = (double)a.Cout * a.Ttot * a.Kc * 2.0;
        const double abytes = (double)a.N * a.Hi * a.Wi * a.lda * 2.0;
        a.m_fastest = (wbytes > 2.0e6 && (double)mtiles * wbytes > (double)a.grid_n * abytes) ? 1 : 0;
    }
    const size_t smem = (size_t)S * (BM + BN) * GROWB + 3 * MAXTAPS * sizeof(int) + (RED ? BN * 16 : 0);
    static const std::string nm = std::string("igemm2_kernel<") + std::to_string(BM) + "," + std::to_string(BN) + "," +
                                  std::to_string(NW) + "," + std::to_string(WP) + "," + std::to_string(S) + (RED ? ",bnred>" : (STG ? ",stg>" : ">"));
    if constexpr (S == 2 && STG == 0 && BN == 128) {
        // persistent form (igemm2p_kernel): worth it when a CTA gets more than one tile; needs n_k >= 2 in every class
        const int spt = a.Kc >> 6;
        int min_taps = a.ntaps;
        if (a.ncls > 1) { min_taps = 1 << 30; for (int c = 0; c < a.ncls; ++c) min_taps = min(min_taps, a.cls_ntaps[c]); }
        static int per_cu = -1;                  // resident CTAs per CU of this instantiation (registers and LDS)
        YDL_SET_MAX_LDS((igemm2p_kernel<BM, BN, NW, WP, RED>), smem);
        if (per_cu < 0) {
            int nb = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, igemm2p_kernel<BM, BN, NW, WP, RED>, NW * 64, smem) != hipSuccess) nb = 0;
            per_cu = nb;
        }
        int G = ydl_device_cus() * per_cu;
        G -= G % 8;
        const int ntiles = mtiles * a.grid_n;
        // measured (tools/conv_bench.py --persist 0/1, config-2 layers): +5..10 % with 128-wide tiles once a CTA walks >= 2.5 tiles,
        // neutral to -12 % below that (a second resident CTA overlaps better than a short walk) and with 64-wide tiles
        // (not with the fused reduce: its epilogue on top of the walk's two descriptor sets spills 41 VGPRs)
        if (g_ring_persist && !RED && BN == 128 && min_taps * spt >= 2 && G >= 8 && 2 * ntiles >= 5 * G) {
            static const std::string nmp = nm + ":persistent";
            ydl_note_kernel(fam, nmp.c_str());
            igemm2p_kernel<BM, BN, NW, WP, RED><<<G, NW * 64, smem, st>>>(a);
            YDL_LAUNCH_CHECK();
            return 0;
        }
    }
    YDL_SET_MAX_LDS((igemm2_kernel<BM, BN, NW, WP, S, RED, STG>), smem);
    ydl_note_kernel(fam, nm.c_str());
    igemm2_kernel<BM, BN, NW, WP, S, RED, STG><<<grid, NW * 64, smem, st>>>(a);
    YDL_LAUNCH_CHECK();
    return 0;
}

// patch-form 3x3 / stride-1 kernels (igemm2h_kernel / igemm2hs_kernel): eligibility and launch.  (Not for a launch with the fused
// BatchNorm-backward reduce: conv_plan asks only without it.)
static int g_halo = 1;          // ydl_debug_set key 8
static bool halo_ok(const IgemmArgs& a, int id) {
    if (!g_halo || !kRing[id].patch) return false;
    if (a.ncls > 1 || a.ntaps != 9 || a.Ttot != 9 || a.in_mul != 1 || a.out_mul != 1 || a.out_h0 != 0 || a.out_w0 != 0) return false;
    if (a.Hi != a.Ho || a.Wi != a.Wo || a.Hg != a.Ho || a.Wg != a.Wo || (a.Ho & 7) || (a.Wo & 15) || (a.Kc & 63)) return false;
    bool seen[9] = {false, false, false, false, false, false, false, false, false};
    for (int t = 0; t < 9; ++t) {
        const int dh = a.dh[t], dw = a.dw[t];
        if (dh < -1 || dh > 1 || dw < -1 || dw > 1 || seen[(dh + 1) * 3 + dw + 1]) return false;
        seen[(dh + 1) * 3 + dw + 1] = true;
    }
    return true;
}
template <int BN, int S>
static int launch_igemm2h(IgemmArgs a, hipStream_t st, int fam) {
    constexpr int NW = 8, WP = 4;
    a.grid_n = (a.Cst + BN - 1) / BN;
    a.grid_m = a.M / 128;                                  // every tile is full (halo_ok)
    YDL_CHECK(a.bytesB < 0x08000000u, "ring kernel: weight matrix of 128 MiB or more is not supported");
    {
        const double wbytes = (double)a.Cout * a.Ttot * a.Kc * 2.0;
        const double abytes = (double)a.N * a.Hi * a.Wi * a.lda * 2.0;
        a.m_fastest = (wbytes > 2.0e6 && (double)a.grid_m * wbytes > (double)a.grid_n * abytes) ? 1 : 0;
    }
    static const std::string nm = std::string("igemm2h_kernel<128,") + std::to_string(BN) + "," + std::to_string(S) + ">";
    ydl_note_kernel(fam, nm.c_str());
    if constexpr (S == 2) {
        if (a.Kc == 64) {            // one channel block needs one patch buffer
            const size_t smem = (size_t)HS_PROWS * GROWB + 2 * (size_t)BN * GROWB + 128;
            YDL_SET_MAX_LDS((igemm2hs_kernel<BN, NW, WP, true>), smem);
            igemm2hs_kernel<BN, NW, WP, true><<<dim3(a.grid_m * a.grid_n), NW * 64, smem, st>>>(a);
        } else {
            const size_t smem = 2 * (size_t)HS_PROWS * GROWB + 2 * (size_t)BN * GROWB + 128;
            YDL_SET_MAX_LDS((igemm2hs_kernel<BN, NW, WP>), smem);
            igemm2hs_kernel<BN, NW, WP><<<dim3(a.grid_m * a.grid_n), NW * 64, smem, st>>>(a);
        }
    } else {
        const size_t smem = 2 * (size_t)H_PROWS * GROWB + (size_t)S * BN * GROWB;
        YDL_SET_MAX_LDS((igemm2h_kernel<BN, NW, WP, S>), smem);
        igemm2h_kernel<BN, NW, WP, S><<<dim3(a.grid_m * a.grid_n), NW * 64, smem, st>>>(a);
    }
    YDL_LAUNCH_CHECK();
    return 0;
}
// the patch form of a layer whose ring choice was ``id``
static int launch_patch(int id, const IgemmArgs& a, hipStream_t st, int fam) {
    if (kRing[id].BN == 128) return launch_igemm2h<128, 2>(a, st, fam);
    // 64-wide tiles, one channel block: the two-stage form with ONE patch buffer is 40 KB — four CTAs per CU (64->64 k3 @160^2: forward
    // 66.8 -> 58.5 us, dgrad 54.2 -> 51.2); more channel blocks: three weight stages of 8 KB, two patches = 72 KB, two CTAs per CU
    if (a.Kc == 64) return launch_igemm2h<64, 2>(a, st, fam);
    return launch_igemm2h<64, 3>(a, st, fam);
}

// fused-parity stride-2 dgrad (igemm2s_kernel): eligibility and launch.  ``a`` is the dgrad's base argument block (A = dy, C = dx).
static int g_s2fused = 1;       // ydl_debug_set key 9
static bool s2fused_ok(const ydl_conv_geom* g, int dtype) {
    if (!g_s2fused || !g_ring_enabled || dtype != YDL_BF16) return false;
    if (g->k != 3 || g->s != 2 || g->p != 1 || g->Hi != 2 * g->Ho || g->Wi != 2 * g->Wo) return false;
    if ((g->Ho & 7) || (g->Wo & 15) || (round_up(g->Cout, 8) & 63) || (g->Cin & 7) || g->Cin < 64) return false;
    return true;
}
template <bool ACC>
static int launch_igemm2s_cfg(const IgemmArgs& a, hipStream_t st, int fam) {
    // two weight stages (round 5): a three-stage form spilled 9 VGPRs at the 128-register budget of four waves per SIMD and measured
    // 2..5 % slower on both layers that run it (64->128 @160^2: 118.8 vs 112.8 us, 128->256 @80^2: 96.9 vs 94.9 us)
    constexpr int NW = 8, WP = 4, S = 2;
    const size_t smem = 2 * (size_t)S2_PROWS * GROWB + (size_t)S * 64 * GROWB;
    YDL_SET_MAX_LDS((igemm2s_kernel<NW, WP, S, ACC>), smem);
    ydl_note_kernel(fam, ACC ? "igemm2s_kernel<128,64,2,acc>" : "igemm2s_kernel<128,64,2>");
    igemm2s_kernel<NW, WP, S, ACC><<<dim3(a.grid_m * a.grid_n), NW * 64, smem, st>>>(a);
    YDL_LAUNCH_CHECK();
    return 0;
}
static int launch_igemm2s(IgemmArgs a, hipStream_t st, int fam) {
    a.grid_n = (a.Cst + 63) / 64;
    a.grid_m = a.N * (a.Hi >> 3) * (a.Wi >> 4);
    YDL_CHECK(a.bytesB < 0x08000000u, "ring kernel: weight matrix of 128 MiB or more is not supported");
    return a.accumulate ? launch_igemm2s_cfg<true>(a, st, fam) : launch_igemm2s_cfg<false>(a, st, fam);
}

static int launch_ring(int id, const IgemmArgs& a, hipStream_t st, int fam) {
    if (a.br.nseg > 0) {          // epilogue with the fused BatchNorm-backward reduce: the rows with kRing[id].bnred
        switch (id) {
            case RING_128x128: return launch_igemm2<128, 128, 8, 4, 2, true>(a, st, fam);
            case RING_64x128: return launch_igemm2<64, 128, 4, 2, 3, true>(a, st, fam);
            case RING_128x64: return launch_igemm2<128, 64, 8, 4, 2, true>(a, st, fam);
        }
        ydl_set_error("fused BatchNorm reduce: no instantiation for this ring configuration (query ydl_conv_dgrad_bnred_supported)");
        return 1;
    }
    switch (id) {
        case RING_128x128: return launch_igemm2<128, 128, 8, 4, 2>(a, st, fam);
        case RING_64x128: return launch_igemm2<64, 128, 4, 2, 3>(a, st, fam);
        case RING_128x64: return launch_igemm2<128, 64, 8, 4, 2>(a, st, fam);
        case RING_256x128_STG: return launch_igemm2<256, 128, 8, 4, 3, false, 1>(a, st, fam);
        case RING_256x128_LOADERS: return launch_igemm2l<256, 128, 8, 4, 3, 4>(a, st, fam);
        case RING_128x128_LOADERS: return launch_igemm2l<128, 128, 8, 4, 3, 4>(a, st, fam);
        case RING_128x128_LOADERS_S2: return launch_igemm2l<128, 128, 4, 2, 2, 4>(a, st, fam);
    }
    ydl_set_error("internal: unknown ring kernel id");
    return 1;
}

// Tile choice: a pure function of (M, Cst, K chunks, dtype) and the debug knobs.
static TileCfg pick_cfg(int M, int Cst, int nchunks, bool bf16, int Kc, int taps, bool one_class, bool loaders_ok) {
    TileCfg c;
    c.ring = RING_NONE;
    if (bf16 && g_ring_enabled && Cst >= 64 && Cst % 8 == 0 && nchunks >= 16 && Kc > 0 && Kc % 64 == 0 && taps <= 29) {
        // bf16 MFMA-bound layers (>= 2 K-steps of 64, >= 64 output channels): LDS-DMA ring kernel.  Measured on MI355X over the
        // 3x3 and wide 1x1 layers of BASELINE config 2 (tools/conv_bench.py, forward and dgrad): the 128x128 tile with a 2-stage
        // ring (64 KB of LDS, two CTAs per CU: one CTA's epilogue and load latency hide behind the other's MFMAs) beats the
        // deeper one-CTA-per-CU rings on every layer but the smallest grids, which prefer 64-pixel tiles (more CTAs).
        const long b128 = (long)((M + 127) / 128) * ((Cst + 127) / 128);
        int id = b128 < 256 ? RING_64x128 : RING_128x128;
        // Round 5: 256 x 128 tile, 64 x 64 wave tiles, three stages (144 KB: ONE CTA per CU) with the two wave halves staggered by half a
        // K-step (igemm2_kernel<..., STG>) — 25 % fewer staged bytes per MAC than 128 x 128.  Measured against the two plain tiles on
        // config 2 (tools/conv_bench.py): wins 3..8 % where one round of CTAs covers the layer and the K loop is long enough to
        // carry the un-overlapped prologue / epilogue (256->512 k3s2 @40^2 82 -> 79 us, 512->1024 k3s2 @20^2 73 -> 69, 256->256 k3
        // @40^2 42 -> 39, 2048->1024 @20^2 37 -> 34.5, 768->128 @80^2 54 -> 51); loses on the 9-step 160^2 layer (the persistent
        // 128 x 128 form keeps those), with 100 tiles (512->512 k3 @20^2: 59 vs 51 us) and on the multi-class strided dgrads.
        const long b256 = (long)((M + 255) / 256) * ((Cst + 127) / 128);
        if (one_class && Cst >= 128 && b256 >= 180 && b256 <= 512 && nchunks >= 96) id = RING_256x128_STG;
        // Round 5, loader waves (igemm2l_kernel: 8 multiplier + 4 loader waves, one CTA per CU, three stages): where the choice was a
        // one-CTA-per-CU tile anyway it wins 3..12 % over the staggered 256 x 128 (256->512 k3s2 @40^2 85.7 -> 75.1 us, 256->256 k3 @40^2
        // 41.0 -> 38.5, 2048->1024 @20^2 35.1 -> 32.4, 512->1024 k3s2 @20^2 65.4 -> 62.0), and as 128 x 128 it replaces the 64 x 128 tile of
        // the small grids (512->512 k3 @20^2 forward 44.9 -> 37.8 us, dgrad 42.4 -> 35.6; 1024->512 @20^2 15.8 -> 14.1).  The two-CTA
        // 128 x 128 ring keeps everything else: with 24 waves per CU the split form has 80 registers and loses 10-40 %.
        // (ydl_debug_set key 19 = 0: off)
        if (g_ring_loaders && loaders_ok) {     // (not for a launch with the fused BatchNorm-backward reduce, nor for its support query)
            if (id == RING_256x128_STG && nchunks >= 128) id = RING_256x128_LOADERS;      // (12 K-steps, 768 -> 128 @80^2: 42.8 against 41.2 us — the staggered form keeps it)
            if (id == RING_64x128 && b128 >= 64) id = RING_128x128_LOADERS;
            // the two-CTA 128 x 128 ring where it is NOT walked persistently (fewer than 2.5 tiles per resident CTA): 4 multiplier waves of
            // 64 x 64 + 4 loader waves, two stages, two CTAs per CU (128 registers) — 3..8 % faster than the 8-wave form (512->512 @40^2
            // forward 31.4 -> 29.6 us, dgrad 28.6 -> 26.2; 768->128 @80^2 42.3 -> 40.2); the persistent walk keeps the many-tile layers
            // (64->128 k3s2 @160^2: 112 against 123 us)
            if (id == RING_128x128 && b128 < 1280) id = RING_128x128_LOADERS_S2;
        }
        // 64..127 stored output channels: 128x64 tile, 8 waves, 2 stages = 48 KB (three CTAs per CU).  Measured against the register-staged
        // kernel: 64->128 k3s2 dgrad @320^2 231 -> 199 us, 64->64 k3 @160^2 78/72 -> 77/60 us, 128->64 k3 @160^2 fwd 120 -> 106 us
        if (Cst < 128) id = RING_128x64;
        c.ring = id; c.BM = kRing[id].BM; c.BN = kRing[id].BN;
        return c;
    }
    c.BN = Cst <= 16 ? 16 : (Cst <= 64 ? 64 : 128);
    c.BM = 128;
    // small-M layers: shrink the pixel tile so that the grid still covers the 256 CUs a few times
    long blocks = (long)((M + 127) / 128) * ((Cst + c.BN - 1) / c.BN);
    if (blocks < 512 && c.BN == 128) {
        // halve the channel tile first (measured 6-11 % faster than halving the pixel tile on the 20x20 layers, equal
        // elsewhere), then the pixel tile
        long b1 = (long)((M + 127) / 128) * ((Cst + 63) / 64);
        if (b1 >= 512) { c.BN = 64; return c; }
    }
    if (blocks < 512 && c.BN != 16) c.BM = 64;
    if (c.BM == 64 && c.BN == 128) {
        long b2 = (long)((M + 63) / 64) * ((Cst + 127) / 128);
        if (b2 < 512) c.BN = 64;
    }
    return c;
}

// The launch plan of one forward / dgrad argument block: which kernel runs it and the statistics partial rows it writes.  A pure host
// function: the ydl_conv_fwd_* queries, the accumulate check of conv_fwd_impl, ydl_conv_dgrad_bnred_supported and dispatch_igemm all
// read this one result, so a query cannot describe another kernel than the launch runs.
//   es: element size; fam: 0 forward, 1 dgrad; with_reduce: the launch carries the fused BatchNorm-backward reduce (a.br of a launch,
//   or the question ydl_conv_dgrad_bnred_supported asks)
// Order of refusals: the weights-in-registers kernel refuses partial rows BEFORE its device-dependent conditions (wreg_ok), so the
// forward queries, which always describe a launch with partial rows, need no device.
enum ConvFamily { CONV_STEM, CONV_PW, CONV_WREG, CONV_PATCH, CONV_RING, CONV_TILE };
struct ConvPlan {
    ConvFamily family;      // stem_kernel, pw_kernel, igemm2w_kernel, igemm2h / igemm2hs_kernel, igemm2 / igemm2p / igemm2l_kernel, igemm_kernel
    TileCfg tile;           // the instantiation: CONV_PATCH / CONV_RING tile.ring = the kRing row, CONV_TILE the (BM, BN) of igemm_kernel
    PwPlan pw;              //                    CONV_PW (pw_plan)
    int grid_m, block_m;    // grid_m partial rows of block_m pixels, the last one may be shorter (CONV_WREG writes none: 0, 0)
    bool has_bnred;         // that instantiation has a form with the fused reduce
};
static ConvPlan conv_plan(const IgemmArgs& a, int es, int fam, bool with_reduce) {
    ConvPlan pl{};
    if (es == 2 && fam == 0 && args_stem(a)) {
        const StemPlan sp = stem_plan(a.M, a.Wo);
        if (sp.ok) { pl.family = CONV_STEM; pl.grid_m = sp.grid_m; pl.block_m = sp.block_m; return pl; }
    }
    pl.pw = pw_plan(a.M, a.Kc, a.Cout, a.Cst, es, args_pointwise(a));
    if (pl.pw.ok) { pl.family = CONV_PW; pl.grid_m = pl.pw.grid_m; pl.block_m = pl.pw.block_m; return pl; }
    // weights-in-registers kernel: 3x3 / s1 over one 64-channel block (a launch WITH the fused reduce runs on the ring instead)
    if (es == 2 && !with_reduce && wreg_ok(a)) { pl.family = CONV_WREG; return pl; }
    // K chunks of the shortest class (multi-class dgrad): the ring kernel wants >= 2 K-steps everywhere
    int nch = a.ntaps * (a.Kc / (16 / es));
    if (a.ncls > 1) {
        nch = 1 << 30;
        for (int i = 0; i < a.ncls; ++i) nch = min(nch, a.cls_ntaps[i] * (a.Kc / (16 / es)));
    }
    pl.tile = pick_cfg(a.M, a.Cst, nch, es == 2, a.Kc, a.Ttot, a.ncls <= 1, !with_reduce);
    pl.block_m = pl.tile.BM;
    pl.family = CONV_TILE;
    if (pl.tile.ring) {
        const bool patch = !with_reduce && halo_ok(a, pl.tile.ring);
        pl.family = patch ? CONV_PATCH : CONV_RING;
        if (patch) pl.block_m = 128;                     // (igemm2h / igemm2hs: one 8 x 16 patch per tile)
        pl.has_bnred = !patch && ring_has_bnred(pl.tile.ring);
    }
    pl.grid_m = (a.M + pl.block_m - 1) / pl.block_m;
    return pl;
}

template <typename T>
static int dispatch_igemm(const IgemmArgs& a, hipStream_t st, int fam) {
    const ConvPlan pl = conv_plan(a, (int)sizeof(T), fam, a.br.nseg > 0);
    switch (pl.family) {
        case CONV_STEM: {
            StemArgs q{};
            q.X = (const bf16_t*)a.A; q.W = (const bf16_t*)a.B; q.Y = (bf16_t*)a.C; q.stats = a.stats;
            q.H = a.Hi; q.Wd = a.Wi; q.ldc = a.ldc; q.M = a.M; q.block_m = pl.block_m; q.stats_ld = a.stats_ld;
            q.stats_atomic = a.stats_atomic; q.bytesX = a.bytesA;
            ydl_note_kernel(fam, "stem_kernel<bf16,16,64>");
            stem_kernel<<<pl.grid_m, 256, 0, st>>>(q);
            YDL_LAUNCH_CHECK();
            return 0;
        }
        case CONV_PW: {
            YDL_CHECK(a.br.nseg == 0, "fused BatchNorm reduce: this geometry runs on the point-wise kernel (query ydl_conv_dgrad_bnred_supported)");
            PwArgs q{};
            q.X = a.A; q.W = a.B; q.Y = a.C; q.stats = a.stats;
            q.M = a.M; q.lda = a.lda; q.ldc = a.ldc; q.Cout = a.Cout; q.WN = pl.pw.WN; q.accumulate = a.accumulate;
            q.block_m = pl.pw.block_m; q.stats_ld = a.stats_ld; q.stats_atomic = a.stats_atomic; q.bytesX = a.bytesA; q.ldw_bytes = a.ldb_bytes;
            return launch_pw<T>(q, pl.pw, st, fam);
        }
        case CONV_WREG: return launch_igemm2w(a, st, fam);
        case CONV_PATCH: return launch_patch(pl.tile.ring, a, st, fam);
        case CONV_RING: return launch_ring(pl.tile.ring, a, st, fam);
        case CONV_TILE: break;
    }
    YDL_CHECK(a.br.nseg == 0, "fused BatchNorm reduce: this geometry runs on the register-staged kernel (query ydl_conv_dgrad_bnred_supported)");
    const TileCfg& c = pl.tile;
    if (c.BM == 128 && c.BN == 128) return launch_igemm<T, 128, 128, 8>(a, st, fam);
    if (c.BM == 128 && c.BN == 64) return launch_igemm<T, 128, 64>(a, st, fam);
    if (c.BM == 128 && c.BN == 16) return launch_igemm<T, 128, 16>(a, st, fam);
    if (c.BM == 64 && c.BN == 128) return launch_igemm<T, 64, 128, 8>(a, st, fam);
    if (c.BM == 64 && c.BN == 64) return launch_igemm<T, 64, 64>(a, st, fam);
    return launch_igemm<T, 64, 16>(a, st, fam);
}

// byte extents of the gathered tensor and of the weight matrix (raw-buffer range checks: must stay below 4 GiB)
static int set_extents(IgemmArgs& a, int dtype) {
    const unsigned long long es = (unsigned long long)esize(dtype);
    unsigned long long ba = (unsigned long long)a.N * a.Hi * a.Wi * a.lda * es;
    if (a.ldb_bytes == 0) a.ldb_bytes = (unsigned)((unsigned long long)a.Ttot * a.Kc * es);
    unsigned long long bb = (unsigned long long)(a.Cout - 1) * a.ldb_bytes + (unsigned long long)a.Ttot * a.Kc * es;
    YDL_CHECK(ba < 0xFFFFFFF0ull && bb < 0xFFFFFFF0ull, "tensor larger than 4 GiB: not addressable by the 32-bit buffer loads");
    a.bytesA = (unsigned)ba;
    a.bytesB = (unsigned)bb;
    return 0;
}

static int check_geom(const ydl_conv_geom* g, int dtype) {
    YDL_CHECK(g != nullptr, "null geometry");
    YDL_CHECK(dtype == YDL_F32 || dtype == YDL_BF16, "bad dtype");
    YDL_CHECK(g->N > 0 && g->Hi > 0 && g->Wi > 0 && g->Cin > 0 && g->Cout > 0, "non-positive dims");
    YDL_CHECK(g->k >= 1 && g->k * g->k <= MAXTAPS && g->s >= 1 && g->p >= 0, "unsupported kernel/stride/pad");
    YDL_CHECK(g->Ho == (g->Hi + 2 * g->p - g->k) / g->s + 1 && g->Wo == (g->Wi + 2 * g->p - g->k) / g->s + 1,
              "output size does not match (H+2p-k)/s+1");
    int es = esize(dtype);
    YDL_CHECK(g->ldx >= round_up(g->Cin, 8) && g->ldy >= g->Cout, "pixel stride smaller than channel count");
    YDL_CHECK((g->ldx * es) % 16 == 0 && (g->ldy * es) % 16 == 0, "pixel strides must be 16-byte multiples");
    YDL_CHECK((int64_t)g->N * g->Hi * g->Wi < (1ll << 31) && (int64_t)g->N * g->Ho * g->Wo < (1ll << 31), "too many pixels");
    YDL_CHECK(g->ldw == 0 || (g->ldw >= g->k * g->k * round_up(g->Cin, 8) && (g->ldw * es) % 16 == 0),
              "ldw must be 0 (dense) or a 16-byte-multiple row stride >= k*k*round_up(Cin, 8)");
    return 0;
}

// argument block of a forward launch (ydl_conv_fwd / _sums and the statistics queries build it the same way)
static int fwd_args(const ydl_conv_geom* g, int dtype, const void* x, const void* w, void* y, float* stats_ws, int stats_atomic,
                    int accumulate, IgemmArgs& a) {
    if (int e = check_geom(g, dtype)) return e;
    a = IgemmArgs{};
    a.A = x; a.B = w; a.C = y; a.stats = stats_ws;
    a.N = g->N; a.Hi = g->Hi; a.Wi = g->Wi; a.lda = g->ldx;
    a.Kc = round_up(g->Cin, 8);
    a.Ho = g->Ho; a.Wo = g->Wo; a.ldc = g->ldy; a.Cout = g->Cout;
    a.Cst = round_up(g->Cout, 8) <= g->ldy ? round_up(g->Cout, 8) : g->Cout;
    a.Hg = g->Ho; a.Wg = g->Wo; a.in_mul = g->s; a.out_mul = 1; a.out_h0 = 0; a.out_w0 = 0;
    a.ntaps = g->k * g->k; a.Ttot = a.ntaps; a.accumulate = accumulate ? 1 : 0;
    a.M = g->N * g->Ho * g->Wo;
    a.stats_ld = round_up(g->Cout, 8);
    a.stats_atomic = stats_atomic;
    a.ldb_bytes = (unsigned)(g->ldw * esize(dtype));
    for (int r = 0; r < g->k; ++r)
        for (int s = 0; s < g->k; ++s) {
            int tpi = r * g->k + s;
            a.dh[tpi] = (signed char)(r - g->p); a.dw[tpi] = (signed char)(s - g->p); a.wt[tpi] = (unsigned char)tpi;
        }
    return set_extents(a, dtype);
}

// (grid_m, block_m) of ydl_conv_fwd with partial rows: the rows a launch with accumulate = 0 writes (a launch that accumulates checks
// that it writes the same ones).  (0, 0) on a bad geometry.
static ConvPlan fwd_blocks(const ydl_conv_geom* g, int dtype) {
    static float stats_tag;                // any non-null pointer: the queries describe a launch WITH partial rows
    IgemmArgs a;
    if (fwd_args(g, dtype, nullptr, nullptr, nullptr, &stats_tag, 0, 0, a)) return ConvPlan{};
    return conv_plan(a, esize(dtype), 0, false);
}

extern "C" int64_t ydl_conv_fwd_stats_ws_bytes(const ydl_conv_geom* g, int dtype) {
    // [gridM][2][round_up(Cout,8)] floats + room for ydl_bn_finalize's level-1 chunk partials (gridM/64 + 1 rows)
    const ConvPlan r = fwd_blocks(g, dtype);
    if (r.grid_m <= 0) return 0;
    return ((int64_t)r.grid_m + r.grid_m / 64 + 2) * 2 * round_up(g->Cout, 8) * (int64_t)sizeof(float);
}
extern "C" int ydl_conv_fwd_grid_m(const ydl_conv_geom* g, int dtype) { return fwd_blocks(g, dtype).grid_m; }
extern "C" int ydl_conv_fwd_block_m(const ydl_conv_geom* g, int dtype) { return fwd_blocks(g, dtype).block_m; }

static int conv_fwd_impl(const ydl_conv_geom* g, int dtype, const void* x, const void* w, void* y,
                         float* stats_ws, int stats_atomic, int accumulate, void* stream) {
    IgemmArgs a;
    if (int e = fwd_args(g, dtype, x, w, y, stats_ws, stats_atomic, accumulate, a)) return e;
    YDL_CHECK(aligned16(x) && aligned16(w) && aligned16(y), "pointers must be 16-byte aligned");
    if (stats_ws != nullptr && !stats_atomic && accumulate) {
        // the queries describe the launch without accumulation: this one must write the same rows (the thin-input stem kernel,
        // for one, runs only without it)
        IgemmArgs a0 = a;
        a0.accumulate = 0;
        const ConvPlan r0 = conv_plan(a0, esize(dtype), 0, false), r1 = conv_plan(a, esize(dtype), 0, false);
        YDL_CHECK(r0.grid_m == r1.grid_m && r0.block_m == r1.block_m,
                  "partial-row statistics with accumulate != 0: this geometry runs on another kernel than ydl_conv_fwd_grid_m / _block_m describe");
    }
    hipStream_t st = (hipStream_t)stream;
    return dtype == YDL_F32 ? dispatch_igemm<float>(a, st, 0) : dispatch_igemm<bf16_t>(a, st, 0);
}

extern "C" int ydl_conv_fwd(const ydl_conv_geom* g, int dtype, const void* x, const void* w, void* y,
                            float* stats_ws, int accumulate, void* stream) {
    return conv_fwd_impl(g, dtype, x, w, y, stats_ws, 0, accumulate, stream);
}
extern "C" int ydl_conv_fwd_sums(const ydl_conv_geom* g, int dtype, const void* x, const void* w, void* y,
                                 float* sums, int accumulate, void* stream) {
    YDL_CHECK(sums != nullptr, "null sums");
    return conv_fwd_impl(g, dtype, x, w, y, sums, 1, accumulate, stream);
}

static int conv_dgrad_impl(const ydl_conv_geom* g, int dtype, const void* dy, const void* wt, void* dx,
                           int accumulate, const ydl_bnred* red, ConvPlan* plan_out, void* stream) {
    if (int e = check_geom(g, dtype)) return e;
    YDL_CHECK(plan_out || (aligned16(dy) && aligned16(wt) && aligned16(dx)), "pointers must be 16-byte aligned");
    YDL_CHECK(g->ldy >= round_up(g->Cout, 8), "dy pixel stride must cover Cout rounded up to 8");
    hipStream_t st = (hipStream_t)stream;
    const int s = g->s, k = g->k, pd = g->p;
    // dx[h] gets dy[(h + p - r)/s] * w[r] for taps r with (h + p - r) % s == 0: per output-parity class (ph, pw) a dense
    // convolution over its own tap subset (no zero MACs).  All classes run in ONE launch (a pixel tile belongs to one
    // class; heavier classes first): four separate launches each paid their own tail and launch gap.
    struct Cls { int ph, pw, nt, Hg, Wg; signed char dh[MAXTAPS], dw[MAXTAPS]; unsigned char wt[MAXTAPS]; };
    static thread_local Cls cls[16];
    int ncls = 0, total_taps = 0;
    YDL_CHECK(s * s <= 16, "stride too large for the dgrad class table");
    for (int ph = 0; ph < s; ++ph)
        for (int pw = 0; pw < s; ++pw) {
            Cls& c = cls[ncls];
            c.ph = ph; c.pw = pw;
            c.Hg = (g->Hi - ph + s - 1) / s; c.Wg = (g->Wi - pw + s - 1) / s;
            if (c.Hg <= 0 || c.Wg <= 0) continue;
            int nt = 0;
            for (int r = 0; r < k; ++r) {
                int nh = ph + pd - r;
                if (((nh % s) + s) % s != 0) continue;
                for (int cc = 0; cc < k; ++cc) {
                    int nw = pw + pd - cc;
                    if (((nw % s) + s) % s != 0) continue;
                    int dh = nh >= 0 ? nh / s : -((-nh) / s), dw = nw >= 0 ? nw / s : -((-nw) / s);
                    c.dh[nt] = (signed char)dh; c.dw[nt] = (signed char)dw; c.wt[nt] = (unsigned char)(r * k + cc);
                    ++nt;
                }
            }
            c.nt = nt;                       // nt == 0 (k < s): the gradient of this class is zero, the kernel stores zeros
            total_taps += nt;
            ++ncls;
        }
    auto base_args = [&]() {
        IgemmArgs a{};
        a.A = dy; a.B = wt; a.C = dx; a.stats = nullptr;
        a.N = g->N; a.Hi = g->Ho; a.Wi = g->Wo; a.lda = g->ldy;
        a.Kc = round_up(g->Cout, 8);
        a.Ho = g->Hi; a.Wo = g->Wi; a.ldc = g->ldx; a.Cout = g->Cin;
        a.Cst = g->Cin;
        a.in_mul = 1; a.out_mul = s;
        a.Ttot = k * k; a.accumulate = accumulate;
        if (red) a.br = *red;
        return a;
    };
    // plan_out != nullptr (ydl_conv_dgrad_bnred_supported): no launch, *plan_out = the plan of this gradient as ONE launch WITH the fused reduce
    auto run = [&](const IgemmArgs& a) -> int {
        if (plan_out) { *plan_out = conv_plan(a, esize(dtype), 1, true); return 0; }
        return dtype == YDL_F32 ? dispatch_igemm<float>(a, st, 1) : dispatch_igemm<bf16_t>(a, st, 1);
    };
    if (red == nullptr && plan_out == nullptr && ncls == 4 && s2fused_ok(g, dtype)) {
        // k3 s2 p1: all four parity classes in one CTA (igemm2s_kernel)
        IgemmArgs a = base_args();
        a.M = g->N * g->Ho * g->Wo; a.Hg = g->Ho; a.Wg = g->Wo; a.ntaps = 9;
        if (int e2 = set_extents(a, dtype)) return e2;
        const unsigned long long bc = (unsigned long long)g->N * g->Hi * g->Wi * g->ldx * 2ull;
        if (bc < 0xFFFFFFF0ull) {                            // (a larger dx is not addressable by the accumulate pre-pass: ring kernel)
            a.bytesC = (unsigned)bc;
            return launch_igemm2s(a, st, 1);
        }
    }
    if (g_dgrad_merge && ncls > 1 && ncls <= 4 && total_taps <= MAXTAPS) {
        // heavier classes first (their CTAs run longest)
        int order[4] = {0, 1, 2, 3};
        for (int i = 0; i < ncls; ++i)
            for (int j = i + 1; j < ncls; ++j)
                if (cls[order[j]].nt > cls[order[i]].nt) { int t = order[i]; order[i] = order[j]; order[j] = t; }
        IgemmArgs a = base_args();
        a.ncls = ncls;
        int tp = 0;
        for (int i = 0; i < ncls; ++i) {
            const Cls& c = cls[order[i]];
            a.cls_ntaps[i] = c.nt; a.cls_tap0[i] = tp; a.cls_Hg[i] = c.Hg; a.cls_Wg[i] = c.Wg;
            a.cls_M[i] = g->N * c.Hg * c.Wg; a.cls_h0[i] = c.ph; a.cls_w0[i] = c.pw;
            for (int t = 0; t < c.nt; ++t) { a.dh[tp + t] = c.dh[t]; a.dw[tp + t] = c.dw[t]; a.wt[tp + t] = c.wt[t]; }
            tp += c.nt;
        }
        // single-class fields: defaults
        a.Hg = a.cls_Hg[0]; a.Wg = a.cls_Wg[0]; a.out_h0 = a.cls_h0[0]; a.out_w0 = a.cls_w0[0];
        a.ntaps = a.cls_ntaps[0];
        a.M = 0;
        for (int i = 0; i < ncls; ++i) a.M += a.cls_M[i];       // tile choice sees the whole launch
        if (int e2 = set_extents(a, dtype)) return e2;
        return run(a);
    }
    if (plan_out && ncls > 1) { *plan_out = ConvPlan{}; plan_out->family = CONV_TILE; return 0; }       // one launch per class (debug knob): no fused form
    YDL_CHECK(red == nullptr || ncls == 1, "fused BatchNorm reduce needs the single-launch dgrad");
    for (int ci = 0; ci < ncls; ++ci) {
        const Cls& c = cls[ci];
        IgemmArgs a = base_args();
        a.Hg = c.Hg; a.Wg = c.Wg; a.out_h0 = c.ph; a.out_w0 = c.pw;
        a.M = g->N * a.Hg * a.Wg;
        a.ntaps = c.nt;
        for (int t = 0; t < c.nt; ++t) { a.dh[t] = c.dh[t]; a.dw[t] = c.dw[t]; a.wt[t] = c.wt[t]; }
        if (int e2 = set_extents(a, dtype)) return e2;
        if (int e = run(a)) return e;
    }
    return 0;
}

extern "C" int ydl_conv_dgrad(const ydl_conv_geom* g, int dtype, const void* dy, const void* wt, void* dx,
                              int accumulate, void* stream) {
    return conv_dgrad_impl(g, dtype, dy, wt, dx, accumulate, nullptr, nullptr, stream);
}

extern "C" int ydl_conv_dgrad_bnred_supported(const ydl_conv_geom* g, int dtype) {
    if (g == nullptr || dtype != YDL_BF16) return 0;
    ConvPlan pl{};
    if (conv_dgrad_impl(g, dtype, nullptr, nullptr, nullptr, 0, nullptr, &pl, nullptr) != 0) return 0;
    return pl.family == CONV_RING && pl.has_bnred ? 1 : 0;
}

extern "C" int ydl_conv_dgrad_bnred(const ydl_conv_geom* g, int dtype, const void* dy, const void* wt, void* dx,
                                    int accumulate, const ydl_bnred* red, void* stream) {
    YDL_CHECK(red != nullptr && (red->nseg == 1 || red->nseg == 2), "one or two channel segments");
    YDL_CHECK(dtype == YDL_BF16, "the fused reduce exists for bf16 only");
    for (int i = 0; i < red->nseg; ++i) {
        YDL_CHECK(red->c0[i] >= 0 && red->c0[i] < red->c1[i] && red->c0[i] % 8 == 0 && red->c1[i] % 8 == 0 && red->c1[i] <= round_up(g->Cin, 8),
                  "segment channel range must be 8-aligned inside the gradient's channels");
        YDL_CHECK(red->cp[i] >= red->c1[i] - red->c0[i] && red->ldy[i] >= red->c1[i] - red->c0[i], "segment strides too small");
        YDL_CHECK(red->y[i] && red->scale[i] && red->shift[i] && red->mean[i] && red->invstd[i] && red->sums[i], "null segment pointer");
        YDL_CHECK(aligned16(red->y[i]) && (red->ldy[i] * 2) % 16 == 0, "segment y must be 16-byte aligned");
        YDL_CHECK(red->act[i] == YDL_ACT_NONE || red->act[i] == YDL_ACT_SILU, "segment activation: none or SiLU");
    }
    YDL_CHECK(red->nseg == 1 || red->c1[0] <= red->c0[1], "segments must be ordered and disjoint");
    return conv_dgrad_impl(g, dtype, dy, wt, dx, accumulate, red, nullptr, stream);
}

// ======================================================================================================
// wgrad: dW[cout][j] += sum_pixels dY[pixel][cout] * Xcol[pixel][j],   j = (tap, cin) flattened
// Tiles: 128 bytes of cout x 128 bytes of j (64x64 bf16 / 32x32 f32), 64 pixels per stage, split-K over
// pixels (gridDim.z), f32 atomics into dW.  bf16 operands are transposed on the LDS read path by
// ds_read_b64_tr_b16 (the contraction index = pixel is the row index of both NHWC tiles).
// ======================================================================================================
struct WgradArgs {
    const void* X; const void* dY; float* dW;
    int N, Hi, Wi, ldx, Kc;       // Kc = padded Cin
    int Ho, Wo, ldy, Cout;
    int k, s, p;
    int M;                        // N*Ho*Wo
    int chunk;                    // pixels per split (multiple of 64)
    int ntaps;
    unsigned long long magicW, magicHW;   // ceil(2^40 / Wo), ceil(2^40 / (Ho*Wo)): division-free pixel decode
    unsigned bytesX, bytesY;
    int njt, nct;                 // tile counts (1-D grid = njt * nct * splits)
    int ldw;                      // dW row stride (floats)
    float* slab;                  // deterministic mode: [splits][Cout][ntaps*Kc] partial sums (plain stores), else NULL
};

__device__ __forceinline__ unsigned fastdiv40(unsigned n, unsigned long long magic) {
    return (unsigned)(((unsigned long long)n * magic) >> 40);
}

#define WG_BKP 64

// TR = true: bf16 fragments via ds_read_b64_tr_b16; false: eight scalar LDS reads per fragment (debug/reference)
template <typename T, bool TR>
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradArgs p) {
    constexpr int V = ET<T>::V;
    constexpr int TE = 128 / sizeof(T);        // elements per 128-byte tile row: 64 bf16 / 32 f32
    // bf16: unpadded 128-byte rows with the 32-byte blocks XOR-swizzled by f(row) = bit1(row) | bit3(row) << 1, which makes
    // every 32-lane half of a ds_read_b64_tr_b16 (rows {0-3, 8-11} x one block) hit 8 distinct 32-byte bank segments
    // (the 144-byte padded rows were 2-way conflicting: 1/3 of the LDS cycles).  f32 keeps the padded layout.
    constexpr int WROW = (sizeof(T) == 2) ? 128 : ROWB;
    __shared__ __attribute__((aligned(16))) unsigned char sY[WG_BKP * WROW];
    __shared__ __attribute__((aligned(16))) unsigned char sX[WG_BKP * WROW];
    auto wsw = [](int row, int colbyte) {          // byte offset of (row, colbyte) in a tile
        if constexpr (sizeof(T) == 2) {
            const int f = ((row >> 1) & 1) | (((row >> 3) & 1) << 1);
            return row * 128 + ((((colbyte >> 5) ^ f) << 5) | (colbyte & 31));
        } else {
            return row * ROWB + colbyte;
        }
    };
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wi = wave >> 1, wj = wave & 1;   // wave grid over (cout, j)
    const int tile = xcd_remap(blockIdx.x, gridDim.x);      // all tiles of one pixel range share an XCD's L2
    const int jt = tile % p.njt, ct = (tile / p.njt) % p.nct, zt = tile / (p.njt * p.nct);
    const int q = t & 7, r = t >> 3;
    const int cpt = p.Kc / V;
    const int nchunks = p.ntaps * cpt;
    // this thread's X chunk is fixed for the whole kernel
    const int Q = jt * 8 + q;
    const bool qv = Q < nchunks;
    const int tap = qv ? Q / cpt : 0;
    const int cc = (Q - tap * cpt) * V;
    const int dh = tap / p.k - p.p, dw = tap % p.k - p.p;
    const int co_chunk = ct * TE + q * V;          // first cout of this thread's dY chunk
    const bool yv = co_chunk < p.Cout;             // Cout % V may be != 0: tail handled by ldy padding zeros
    const T* Xg = (const T*)p.X;
    const T* Yg = (const T*)p.dY;
    const int pbeg = zt * p.chunk;
    const int pend = min(p.M, pbeg + p.chunk);

    constexpr int NT = (sizeof(T) == 2) ? 2 : 1;   // 16x16 tiles per wave per dim
    f32x4 acc[NT][NT];
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int HoWo = p.Ho * p.Wo;
    const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc((void*)p.X, 0, p.bytesX, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc((void*)p.dY, 0, p.bytesY, 0x00020000);
    uint4 vy[2], vx[2];
    // range-checked buffer loads (zeros for padding taps / tail rows).  The (image, row, column) of this thread's two pixels are
    // decoded once by multiply-shift and then carried from stage to stage (stages are loaded in order, WG_BKP pixels apart): the two
    // divisions per load were a third of this kernel's VALU instructions (10 per MFMA, round-4 SQ counters)
    // ... and so are the two BYTE OFFSETS (round 5): both are linear in (image, row, column), so a stage step is one add plus a
    // correction at each wrap instead of six 32-bit multiply-adds per pixel (measured neutral: this kernel is not VALU-bound)
    int xho[2], xwo[2];
    unsigned xoff[2], yoff[2];
    auto x_offset = [&](int n, int ho, int wo) {
        return (unsigned)(((n * p.Hi + ho * p.s + dh) * p.Wi + wo * p.s + dw) * p.ldx + cc) * (unsigned)sizeof(T);
    };
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const unsigned m = (unsigned)(pbeg + r + 32 * i);
        const unsigned n = fastdiv40(m, p.magicHW);
        const unsigned rem = m - n * (unsigned)HoWo;
        const unsigned ho = fastdiv40(rem, p.magicW);
        xho[i] = (int)ho; xwo[i] = (int)(rem - ho * (unsigned)p.Wo);
        xoff[i] = x_offset((int)n, xho[i], xwo[i]);
        yoff[i] = (unsigned)((int)m * p.ldy + co_chunk) * (unsigned)sizeof(T);
    }
    const int adv_h = WG_BKP / p.Wo, adv_w = WG_BKP - adv_h * p.Wo;
    const bool slow_decode = adv_h + 1 > p.Ho;           // maps narrower than a stage is long: decode by division every time
    const unsigned adv_step = (unsigned)(((adv_h * p.s) * p.Wi + adv_w * p.s) * p.ldx) * (unsigned)sizeof(T);     // WG_BKP pixels on
    const unsigned adv_wrap_w = (unsigned)((p.s * p.Wi - p.Wo * p.s) * p.ldx) * (unsigned)sizeof(T);               // one row down, Wo columns back
    const unsigned adv_wrap_h = (unsigned)(((p.Hi - p.Ho * p.s) * p.Wi) * p.ldx) * (unsigned)sizeof(T);            // into the next image
    const unsigned adv_y = (unsigned)(WG_BKP * p.ldy) * (unsigned)sizeof(T);
    auto gload = [&](int p0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int m = p0 + r + 32 * i;
            bool in = m < pend;
            u32x4 a = __builtin_amdgcn_raw_buffer_load_b128(rsY, (in && yv) ? yoff[i] : 0xFFFFFFFFu, 0, 0);
            vy[i] = make_uint4(a.x, a.y, a.z, a.w);
            yoff[i] += adv_y;
            if (slow_decode) {
                const unsigned n = fastdiv40((unsigned)m, p.magicHW);
                const unsigned rem = (unsigned)m - n * (unsigned)HoWo;
                const unsigned ho = fastdiv40(rem, p.magicW);
                xho[i] = (int)ho; xwo[i] = (int)(rem - ho * (unsigned)p.Wo);
                xoff[i] = x_offset((int)n, xho[i], xwo[i]);
            }
            int ih = __mul24(xho[i], p.s) + dh, iw = __mul24(xwo[i], p.s) + dw;       // (full-rate 24-bit multiplies: map sides < 2^21, conv_wgrad_impl)
            bool ok = in && qv && (unsigned)ih < (unsigned)p.Hi && (unsigned)iw < (unsigned)p.Wi;
            u32x4 b = __builtin_amdgcn_raw_buffer_load_b128(rsX, ok ? xoff[i] : 0xFFFFFFFFu, 0, 0);
            vx[i] = make_uint4(b.x, b.y, b.z, b.w);
            xwo[i] += adv_w; xho[i] += adv_h; xoff[i] += adv_step;
            if (xwo[i] >= p.Wo) { xwo[i] -= p.Wo; xho[i] += 1; xoff[i] += adv_wrap_w; }
            if (xho[i] >= p.Ho) { xho[i] -= p.Ho; xoff[i] += adv_wrap_h; }
        }
    };
    gload(pbeg);
    for (int p0 = pbeg; p0 < pend; p0 += WG_BKP) {
        __syncthreads();   // previous stage's LDS reads done
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            *(uint4*)(sY + wsw(r + 32 * i, q * 16)) = vy[i];
            *(uint4*)(sX + wsw(r + 32 * i, q * 16)) = vx[i];
        }
        __syncthreads();
        if (p0 + WG_BKP < pend) gload(p0 + WG_BKP);      // next stage in flight while this one is multiplied
        if constexpr (sizeof(T) == 2 && !TR) {
            const int g = lane >> 4, li = lane & 15;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                uint4 af[NT], bfv[NT];
#pragma unroll
                for (int a = 0; a < NT; ++a) {
                    unsigned short e[8];
#pragma unroll
                    for (int x = 0; x < 8; ++x)
                        e[x] = *(const unsigned short*)(sY + wsw(ks * 32 + g * 8 + x, (wi * 32 + a * 16 + li) * 2));
                    af[a] = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
                }
#pragma unroll
                for (int b = 0; b < NT; ++b) {
                    unsigned short e[8];
#pragma unroll
                    for (int x = 0; x < 8; ++x)
                        e[x] = *(const unsigned short*)(sX + wsw(ks * 32 + g * 8 + x, (wj * 32 + b * 16 + li) * 2));
                    bfv[b] = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
                }
#pragma unroll
                for (int a = 0; a < NT; ++a)
#pragma unroll
                    for (int b = 0; b < NT; ++b) Mma<bf16_t>::run(af[a], bfv[b], acc[a][b]);
            }
        } else if constexpr (sizeof(T) == 2) {
            // group g = lane>>4 covers pixels 8g..8g+7 of a 32-pixel k-step; lane 4q'+p' of the group addresses
            // row q' (pixel), columns 4p'..4p'+3 (channels); result element e = pixel row e, channel = lane&15.
            const int g = lane >> 4, lq = (lane & 15) >> 2, lp = lane & 3;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                uint4 af[NT], bfv[NT];
#pragma unroll
                for (int a = 0; a < NT; ++a) {
                    const unsigned char* base = sY + wsw(ks * 32 + g * 8 + lq, (wi * 32 + a * 16 + lp * 4) * 2);
                    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base));
                    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + 4 * WROW));
                    uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
                    af[a] = make_uint4(l2.x, l2.y, h2.x, h2.y);
                }
#pragma unroll
                for (int b = 0; b < NT; ++b) {
                    const unsigned char* base = sX + wsw(ks * 32 + g * 8 + lq, (wj * 32 + b * 16 + lp * 4) * 2);
                    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base));
                    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + 4 * WROW));
                    uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
                    bfv[b] = make_uint4(l2.x, l2.y, h2.x, h2.y);
                }
#pragma unroll
                for (int a = 0; a < NT; ++a)
#pragma unroll
                    for (int b = 0; b < NT; ++b) Mma<bf16_t>::run(af[a], bfv[b], acc[a][b]);
            }
        } else {
            // f32: A[i = lane&15][k = lane>>4] = dY[pixel k][cout i]; one float per lane per MFMA (k = 4 pixels)
            const int li = lane & 15, lk = lane >> 4;
#pragma unroll 4
            for (int ks = 0; ks < WG_BKP / 4; ++ks) {
                float a = *(const float*)(sY + (ks * 4 + lk) * ROWB + (wi * 16 + li) * 4);
                float b = *(const float*)(sX + (ks * 4 + lk) * ROWB + (wj * 16 + li) * 4);
                acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[0][0], 0, 0, 0);
            }
        }
    }
    // epilogue: D[row = cout][col = j]; lane holds col = lane&15, rows (lane>>4)*4 + e
    constexpr int SUB = (sizeof(T) == 2) ? 32 : 16;
    const size_t wrow = (size_t)p.ntaps * p.Kc;
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) {
            int j = jt * TE + wj * SUB + b * 16 + (lane & 15);
            if (j < (int)wrow) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int co = ct * TE + wi * SUB + a * 16 + (lane >> 4) * 4 + e;
                    if (co < p.Cout) {
                        if (p.slab) p.slab[((size_t)zt * p.Cout + co) * wrow + j] = acc[a][b][e];
                        else atomicAdd(p.dW + (size_t)co * p.ldw + j, acc[a][b][e]);
                    }
                }
            }
        }
}

// ======================================================================================================
// wgrad, bf16 fast path: 128-byte... no: 256-byte rows.  CTA tile = TCO output channels x 128 flattened-K columns,
// 64 pixels per stage, register-prefetched (the next stage's global loads are in flight while the MFMAs of the
// current one run), pixel decode by multiply-shift (no integer division in the loop).
//   TCO = 128: waves 2 (cout) x 2 (j), each 64 x 64 = 4 x 4 MFMA tiles;  TCO = 64: waves 1 x 4, each 64 x 32.
// ======================================================================================================
#define W2_ROWB 256      // unpadded; 32-byte blocks XOR-swizzled by f(row) = (row & 3) | bit3(row) << 2  (conflict-free tr reads)
__device__ __forceinline__ int w2sw(int row, int colbyte) {
    const int f = (row & 3) | (((row >> 3) & 1) << 2);
    return row * W2_ROWB + ((((colbyte >> 5) ^ f) << 5) | (colbyte & 31));
}

struct Wgrad2Args {
    const bf16_t* X; const bf16_t* dY; float* dW;
    int N, Hi, Wi, ldx, Kc;
    int Ho, Wo, ldy, Cout;
    int k, s, p;
    int M, chunk, ntaps;
    unsigned long long magicW, magicHW;   // ceil(2^40 / Wo), ceil(2^40 / (Ho*Wo))
    unsigned bytesX, bytesY;
    int njt, nct;
    int ldw;                              // dW row stride (floats)
    float* slab;                          // deterministic mode: [splits][Cout][ntaps*Kc] partial sums, else NULL
};

template <int TCO>
__global__ __launch_bounds__(256, 2) void wgrad2_kernel(const Wgrad2Args p) {
    constexpr int WCO = TCO / 64;              // waves along cout
    constexpr int WJ = 4 / WCO;                // waves along j
    constexpr int JW = 128 / WJ;               // j columns per wave
    constexpr int NA = 4;                      // cout tiles per wave (64 / 16)
    constexpr int NB = JW / 16;                // j tiles per wave
    constexpr int YCH = TCO / 8;               // 16-byte chunks per dY tile row
    constexpr int YR = (64 * YCH) / 256;       // dY rows per thread
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* sY = smem;                              // [2][64][W2_ROWB]
    unsigned char* sX = smem + 2 * 64 * W2_ROWB;           // [2][64][W2_ROWB]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wi = wave / WJ, wj = wave % WJ;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int jt = tile % p.njt, ct = (tile / p.njt) % p.nct, zt = tile / (p.njt * p.nct);
    const int cpt = p.Kc / 8;
    const int nchunks = p.ntaps * cpt;
    // X tile: 16 chunks per row, 16 rows per pass, 4 passes;  this thread's chunk (=> tap, channel) is fixed
    const int xq = t & 15, xr = t >> 4;
    const int Q = jt * 16 + xq;
    const bool qv = Q < nchunks;
    const int tap = qv ? Q / cpt : 0;
    const int cc = (Q - tap * cpt) * 8;
    const int dh = tap / p.k - p.p, dw = tap % p.k - p.p;
    // dY tile: YCH chunks per row
    const int yq = t % YCH, yr = t / YCH;
    const int co_chunk = ct * TCO + yq * 8;
    const bool yv = co_chunk < p.Cout;
    const int pbeg = zt * p.chunk;
    const int pend = min(p.M, pbeg + p.chunk);
    const int HoWo = p.Ho * p.Wo;
    const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc((void*)p.X, 0, p.bytesX, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc((void*)p.dY, 0, p.bytesY, 0x00020000);

    f32x4 acc[NA][NB];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    // two register sets: the loads of stage s+2 are issued while stage s is multiplied and stage s+1 (already in
    // registers) is written to the other LDS buffer => every global load has two full stages to land
    uint4 vy[2][YR], vx[2][4];
    auto gload = [&](int p0, uint4 (&ry)[YR], uint4 (&rx)[4]) {
#pragma unroll
        for (int i = 0; i < YR; ++i) {
            int m = p0 + yr + (256 / YCH) * i;
            unsigned off = (yv && m < pend) ? (unsigned)(m * p.ldy + co_chunk) * 2u : 0xFFFFFFFFu;
            u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsY, off, 0, 0);
            ry[i] = make_uint4(v.x, v.y, v.z, v.w);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int m = p0 + xr + 16 * i;
            unsigned n = fastdiv40((unsigned)m, p.magicHW);
            unsigned rem = (unsigned)m - n * (unsigned)HoWo;
            unsigned ho = fastdiv40(rem, p.magicW);
            unsigned wo = rem - ho * (unsigned)p.Wo;
            int ih = (int)ho * p.s + dh, iw = (int)wo * p.s + dw;
            bool ok = qv && m < pend && (unsigned)ih < (unsigned)p.Hi && (unsigned)iw < (unsigned)p.Wi;
            unsigned off = ok ? (unsigned)(((int)(n * p.Hi + ih) * p.Wi + iw) * p.ldx + cc) * 2u : 0xFFFFFFFFu;
            u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsX, off, 0, 0);
            rx[i] = make_uint4(v.x, v.y, v.z, v.w);
        }
    };
    auto sstore = [&](int buf, const uint4 (&ry)[YR], const uint4 (&rx)[4]) {
#pragma unroll
        for (int i = 0; i < YR; ++i)
            *(uint4*)(sY + buf * (64 * W2_ROWB) + w2sw(yr + (256 / YCH) * i, yq * 16)) = ry[i];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *(uint4*)(sX + buf * (64 * W2_ROWB) + w2sw(xr + 16 * i, xq * 16)) = rx[i];
    };
    const int g = lane >> 4, lq = (lane & 15) >> 2, lp = lane & 3;
    auto compute = [&](int cur) {
        const unsigned char* by = sY + cur * (64 * W2_ROWB);
        const unsigned char* bx = sX + cur * (64 * W2_ROWB);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            uint4 af[NA], bfv[NB];
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                const unsigned char* base = by + w2sw(ks * 32 + g * 8 + lq, (wi * 64 + a * 16 + lp * 4) * 2);
                s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base));
                s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + 4 * W2_ROWB));
                uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
                af[a] = make_uint4(l2.x, l2.y, h2.x, h2.y);
            }
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const unsigned char* base = bx + w2sw(ks * 32 + g * 8 + lq, (wj * JW + b * 16 + lp * 4) * 2);
                s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base));
                s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + 4 * W2_ROWB));
                uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
                bfv[b] = make_uint4(l2.x, l2.y, h2.x, h2.y);
            }
#pragma unroll
            for (int a = 0; a < NA; ++a)
#pragma unroll
                for (int b = 0; b < NB; ++b) Mma<bf16_t>::run(af[a], bfv[b], acc[a][b]);
        }
    };

    gload(pbeg, vy[0], vx[0]);
    gload(pbeg + 64, vy[1], vx[1]);            // rows beyond pend load zeros: an odd stage count just multiplies zeros
    sstore(0, vy[0], vx[0]);
    __syncthreads();
    // stage s is multiplied from LDS buffer (s & 1); at an even stage register set 1 holds stage s+1 and set 0 is free.
    // Straight-line pairs (no early exit): the accumulators stay in one register set.
    for (int p0 = pbeg; p0 < pend; p0 += 128) {
        gload(p0 + 128, vy[0], vx[0]);
        compute(0);
        sstore(1, vy[1], vx[1]);
        __syncthreads();
        gload(p0 + 192, vy[1], vx[1]);
        compute(1);
        sstore(0, vy[0], vx[0]);
        __syncthreads();
    }
    const size_t wrow = (size_t)p.ntaps * p.Kc;
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            int j = jt * 128 + wj * JW + b * 16 + (lane & 15);
            if (j < (int)wrow) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int co = ct * TCO + wi * 64 + a * 16 + (lane >> 4) * 4 + e;
                    if (co < p.Cout) {
                        if (p.slab) p.slab[((size_t)zt * p.Cout + co) * wrow + j] = acc[a][b][e];
                        else atomicAdd(p.dW + (size_t)co * p.ldw + j, acc[a][b][e]);
                    }
                }
            }
        }
}

// ======================================================================================================
// wgrad3: the same tile (TCO output channels x 128 flattened-K columns, 64 pixels per stage, transposed LDS reads) fed by
// LDS-DMA like igemm2 — `buffer_load_dwordx4 ... lds` straight into the LDS image, no staging registers and no ds_write pass.
// Why: the register-staged kernel above is bound by its LDS WRITES (ds_write_b128 moves address + data VGPRs at ~79 B/clk/CU,
// 335 LDS cycles against 128 MFMA cycles per stage in the 64x64-tile kernel, profiles/r2_pmc_wgrad_*.txt), not by MFMA issue.
// A wave-instruction writes 1 KiB = (wave-uniform M0 base) + lane*16: exactly the row-major images the register kernel
// builds (X: 4 rows x 256 B per instruction; dY: 4 rows x 256 B for TCO = 128, 8 rows x 128 B for TCO = 64), so the thread ->
// (row, 16-byte slot) map is unchanged and the XOR swizzle of the 32-byte blocks moves to the per-lane SOURCE address: the
// lane at slot qs of row r fetches the logical chunk (((qs >> 1) ^ f(r)) << 1) | (qs & 1).  f depends on row bits that the
// per-pass row stride (16 / 32 rows) leaves alone, so a thread's (tap, channel) stays fixed for the whole kernel.
// Pipeline: two LDS stages; per stage  s_waitcnt vmcnt(0) + s_barrier (stage s landed everywhere, everyone is done with the
// buffer stage s+1 goes to) -> issue the DMAs of stage s+1 -> MFMAs of stage s.  Rows beyond the pixel range and padding taps
// are out-of-range buffer offsets: the DMA writes zeros.  64 KB (TCO 128) / 48 KB (TCO 64) of LDS: two / three CTAs per CU.
// ======================================================================================================
template <int ROWB_>
__device__ __forceinline__ int w3f(int row) {
    // XOR applied to the 32-byte block index of a row: 256-byte rows (8 blocks) use (row & 3) | bit3 << 2 as wgrad2 does;
    // 128-byte rows (4 blocks, two rows per 256-byte bank line) use bit1 | bit3 << 1 — rows {0,2,8,10} / {1,3,9,11} of a
    // transposed read's half-wave then cover the 64 banks exactly once
    return ROWB_ == 256 ? ((row & 3) | (((row >> 3) & 1) << 2)) : (((row >> 1) & 1) | (((row >> 3) & 1) << 1));
}
template <int ROWB_>
__device__ __forceinline__ int w3sw(int row, int colbyte) {
    return row * ROWB_ + ((((colbyte >> 5) ^ w3f<ROWB_>(row)) << 5) | (colbyte & 31));
}

template <int TCO, int SP, int S>
__global__ __launch_bounds__(256, 2) void wgrad3_kernel(const Wgrad2Args p) {
    // SP = pixels per stage (32 or 64), S = stages of the LDS ring: S-1 stages are in flight while one is multiplied.  The loads are
    // latency-bound (timing experiment without MFMAs: 90 % of the kernel's time, 10 TB/s of L2->LDS traffic at ~64 KB in flight per
    // CU), so the ring is cut into more, smaller stages rather than made bigger.
    constexpr int WCO = TCO / 64;              // waves along cout
    constexpr int WJ = 4 / WCO;                // waves along j
    constexpr int JW = 128 / WJ;               // j columns per wave
    constexpr int NA = 4;                      // cout tiles per wave (64 / 16)
    constexpr int NB = JW / 16;                // j tiles per wave
    constexpr int YCH = TCO / 8;               // 16-byte chunks per dY tile row
    constexpr int YROWB = TCO * 2;             // dY tile row bytes (128 or 256): the DMA image has no gaps
    constexpr int YRP = 256 / YCH;             // dY rows per pass of the CTA
    constexpr int YR = SP / YRP;               // dY DMAs per thread per stage
    constexpr int XR = SP / 16;                // X DMAs per thread per stage
    constexpr int L = YR + XR;
    constexpr int YBYTES = SP * YROWB, XBYTES = SP * 256, STAGE = YBYTES + XBYTES;
    static_assert(YR >= 1 && SP % 32 == 0 && S >= 2, "stage geometry");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wi = wave / WJ, wj = wave % WJ;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int jt = tile % p.njt, ct = (tile / p.njt) % p.nct, zt = tile / (p.njt * p.nct);
    const int cpt = p.Kc / 8;
    const int nchunks = p.ntaps * cpt;
    // X image: 16 slots per row, 16 rows per pass; this thread's slot xq of rows xr + 16 i holds logical chunk xlog
    const int xq = t & 15, xr = t >> 4;
    const int xlog = (((xq >> 1) ^ w3f<256>(xr)) << 1) | (xq & 1);
    const int Q = jt * 16 + xlog;
    const bool qv = Q < nchunks;
    const int tap = qv ? Q / cpt : 0;
    const int cc = (Q - tap * cpt) * 8;
    const int dh = tap / p.k - p.p, dw = tap % p.k - p.p;
    // dY image: YCH slots per row, YRP rows per pass
    const int yq = t % YCH, yr = t / YCH;
    const int ylog = (((yq >> 1) ^ w3f<YROWB>(yr)) << 1) | (yq & 1);
    const int co_chunk = ct * TCO + ylog * 8;
    const bool yv = co_chunk < p.Cout;
    const int pbeg = zt * p.chunk;
    const int pend = min(p.M, pbeg + p.chunk);
    const int HoWo = p.Ho * p.Wo;
    u32x4 rsX, rsY;
    {
        const unsigned long long px = (unsigned long long)p.X, py = (unsigned long long)p.dY;
        rsX = u32x4{(unsigned)px, (unsigned)(px >> 32) & 0xffffu, p.bytesX, 0x00020000u};
        rsY = u32x4{(unsigned)py, (unsigned)(py >> 32) & 0xffffu, p.bytesY, 0x00020000u};
    }
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned wave_y = lds0 + (unsigned)wave * 1024u;                     // a wave's 1 KiB of each dY pass
    const unsigned wave_x = lds0 + (unsigned)YBYTES + (unsigned)wave * 1024u;  // ... and of each X pass

    f32x4 acc[NA][NB];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Output row / column of this thread's XR pixels of the NEXT stage to issue, and the BYTE OFFSET of the tap-shifted input pixel they
    // read, carried from stage to stage by additions only (stages are issued in order, SP pixels apart).  The offset is linear in
    // (image, row, column), so a step of SP pixels is one add plus a correction at each wrap; rows / columns outside the image keep a
    // meaningless offset that the bounds test below never lets through.  (Round 5: replaces four v_mad_u64_u32 and a v_mul_lo_u32 per
    // DMA.  Measured neutral, +-1 % on every layer: the loop is not bound by the vector ALU either — see wgrad3s_kernel for what it IS
    // bound by.)
    int xho[XR], xwo[XR];
    unsigned xoff[XR];
    auto x_offset = [&](int n, int ho, int wo) {
        return (unsigned)(((n * p.Hi + ho * p.s + dh) * p.Wi + wo * p.s + dw) * p.ldx + cc) * 2u;
    };
#pragma unroll
    for (int i = 0; i < XR; ++i) {
        const unsigned m = (unsigned)(pbeg + xr + 16 * i);
        const unsigned n = fastdiv40(m, p.magicHW);
        const unsigned rem = m - n * (unsigned)HoWo;
        const unsigned ho = fastdiv40(rem, p.magicW);
        xho[i] = (int)ho; xwo[i] = (int)(rem - ho * (unsigned)p.Wo);
        xoff[i] = x_offset((int)n, xho[i], xwo[i]);
    }
    const int adv_h = SP / p.Wo, adv_w = SP - adv_h * p.Wo;      // (wave-uniform; one conditional wrap each: adv_w < Wo, adv_h + 1 <= Ho)
    const bool slow_decode = adv_h + 1 > p.Ho;
    const unsigned adv_step = (unsigned)(((adv_h * p.s) * p.Wi + adv_w * p.s) * p.ldx) * 2u;      // SP pixels on
    const unsigned adv_wrap_w = (unsigned)((p.s * p.Wi - p.Wo * p.s) * p.ldx) * 2u;                // one row down, Wo columns back
    const unsigned adv_wrap_h = (unsigned)(((p.Hi - p.Ho * p.s) * p.Wi) * p.ldx) * 2u;             // into the next image
    auto issue = [&](int p0, int buf) {
        const unsigned base = (unsigned)buf * (unsigned)STAGE;
#pragma unroll
        for (int i = 0; i < YR; ++i) {
            const int m = p0 + yr + YRP * i;
            const unsigned off = (yv && m < pend) ? (unsigned)(m * p.ldy + co_chunk) * 2u : 0xFFFFFFFFu;
            lds_dma16(rsY, wave_y + base + (unsigned)i * 4096u, off);
        }
#pragma unroll
        for (int i = 0; i < XR; ++i) {
            const int m = p0 + xr + 16 * i;
            // (n*Ho + ho, wo) of pixel m are carried from stage to stage (stages are issued in order, SP pixels apart): the two
            // multiply-shift divisions per DMA made the loop VALU-bound (81 VALU instructions per 16 MFMAs; timing experiment with
            // a shift/mask decode: 64 -> 128 k3s2 @160^2 118 -> 86 us, 64 -> 64 k3 @160^2 102 -> 66 us)
            if (slow_decode) {                           // maps narrower than a stage is long (SP / Wo + 1 > Ho): decode by division
                const unsigned n = fastdiv40((unsigned)m, p.magicHW);
                const unsigned rem = (unsigned)m - n * (unsigned)HoWo;
                const unsigned ho = fastdiv40(rem, p.magicW);
                xho[i] = (int)ho; xwo[i] = (int)(rem - ho * (unsigned)p.Wo);
                xoff[i] = x_offset((int)n, xho[i], xwo[i]);
            }
            const int ih = __mul24(xho[i], p.s) + dh, iw = __mul24(xwo[i], p.s) + dw;      // (full-rate 24-bit multiplies: map sides < 2^21, conv_wgrad_impl)
            const bool ok = qv && m < pend && (unsigned)ih < (unsigned)p.Hi && (unsigned)iw < (unsigned)p.Wi;
            lds_dma16(rsX, wave_x + base + (unsigned)i * 4096u, ok ? xoff[i] : 0xFFFFFFFFu);
            xwo[i] += adv_w; xho[i] += adv_h; xoff[i] += adv_step;
            if (xwo[i] >= p.Wo) { xwo[i] -= p.Wo; xho[i] += 1; xoff[i] += adv_wrap_w; }
            if (xho[i] >= p.Ho) { xho[i] -= p.Ho; xoff[i] += adv_wrap_h; }
        }
    };
    const int g = lane >> 4, lq = (lane & 15) >> 2, lp = lane & 3;
    auto compute = [&](int cur) {
        const unsigned char* by = smem + cur * STAGE;
        const unsigned char* bx = by + YBYTES;
#pragma unroll
        for (int ks = 0; ks < SP / 32; ++ks) {
            uint4 af[NA], bfv[NB];
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                const int row = ks * 32 + g * 8 + lq;
                const unsigned char* lo_p = by + w3sw<YROWB>(row, (wi * 64 + a * 16 + lp * 4) * 2);
                const unsigned char* hi_p = by + w3sw<YROWB>(row + 4, (wi * 64 + a * 16 + lp * 4) * 2);
                s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lo_p));
                s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(hi_p));
                uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
                af[a] = make_uint4(l2.x, l2.y, h2.x, h2.y);
            }
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int row = ks * 32 + g * 8 + lq;
                const unsigned char* lo_p = bx + w3sw<256>(row, (wj * JW + b * 16 + lp * 4) * 2);
                const unsigned char* hi_p = bx + w3sw<256>(row + 4, (wj * JW + b * 16 + lp * 4) * 2);
                s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lo_p));
                s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(hi_p));
                uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
                bfv[b] = make_uint4(l2.x, l2.y, h2.x, h2.y);
            }
#pragma unroll
            for (int a = 0; a < NA; ++a)
#pragma unroll
                for (int b = 0; b < NB; ++b) Mma<bf16_t>::run(af[a], bfv[b], acc[a][b]);
        }
    };

    // ring: stage k of this CTA lives in buffer k % S.  Per stage: wait until only the S-2 youngest stages' DMAs are outstanding
    // (stage k has landed), barrier (everyone's have; every wave is done with stage k-1), issue stage k+S-1 into the buffer stage
    // k-1 occupied, multiply stage k.  Stages beyond pend are all-out-of-range DMAs (zeros nobody multiplies): the vmcnt
    // arithmetic stays uniform.
#pragma unroll
    for (int u = 0; u < S - 1; ++u) issue(pbeg + u * SP, u);
    int buf = 0, nxt = S - 1;
    for (int p0 = pbeg; p0 < pend; p0 += SP) {
        wait_vm_barrier<L * (S - 2)>();
        issue(p0 + (S - 1) * SP, nxt);
        compute(buf);
        buf = buf + 1 == S ? 0 : buf + 1;
        nxt = nxt + 1 == S ? 0 : nxt + 1;
    }
    wait_vm_barrier<0>();                          // the trailing DMAs land before the CTA (and its LDS allocation) goes away
    const size_t wrow = (size_t)p.ntaps * p.Kc;
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            int j = jt * 128 + wj * JW + b * 16 + (lane & 15);
            if (j < (int)wrow) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int co = ct * TCO + wi * 64 + a * 16 + (lane >> 4) * 4 + e;
                    if (co < p.Cout) {
                        if (p.slab) p.slab[((size_t)zt * p.Cout + co) * wrow + j] = acc[a][b][e];
                        else atomicAdd(p.dW + (size_t)co * p.ldw + j, acc[a][b][e]);
                    }
                }
            }
        }
}

// ------------------------------------------------------------------------------------------------------
// wgrad3s: wgrad3 with the two jobs of a wave SPLIT over different waves (round 5).  Measured on wgrad3 (no-DMA / no-MFMA ablations): the DMA + barrier
// loop alone takes 45-65 % of the kernel, the MFMA + fragment-read loop alone 40-55 %, and the whole is their SUM — a wave that is
// held at its LDS-DMA instructions by a full memory pipeline cannot issue its MFMAs, and with one or two waves per SIMD nobody else can.
// Here waves 0-3 only multiply (fragment reads + MFMAs, no vector-memory instruction in their loop) and NL extra LOADER waves only
// issue the DMAs of the ring and wait for them: a stalled loader costs no matrix issue slot.  Same LDS images, same ring, same single
// barrier per stage (every wave takes part):
//     loaders:    s_waitcnt vmcnt (stage k landed) | s_barrier | issue stage k+S-1          multipliers:   s_barrier | stage k
// A loader instruction still writes 1 KiB = 4 rows x 256 B (8 x 128 B for the 64-channel dY image) at (wave-uniform M0) + lane * 16; a
// loader wave owns instruction slots j = lw, lw + NL, ... of each image, so its lanes' rows are j * rows_per_instruction + lane / slots
// and the row-dependent swizzle makes the lane's logical chunk (=> tap, channel) a function of j: kept per slot.
// ------------------------------------------------------------------------------------------------------
template <int TCO, int SP, int S, int NL>
__global__ __launch_bounds__(256 + 64 * NL, 2) void wgrad3s_kernel(const Wgrad2Args p) {
    constexpr int WCO = TCO / 64;
    constexpr int WJ = 4 / WCO;
    constexpr int JW = 128 / WJ;
    constexpr int NA = 4;
    constexpr int NB = JW / 16;
    constexpr int YCH = TCO / 8;
    constexpr int YROWB = TCO * 2;
    constexpr int YBYTES = SP * YROWB, XBYTES = SP * 256, STAGE = YBYTES + XBYTES;
    constexpr int NYI = YBYTES / 1024, NXI = XBYTES / 1024;        // DMA instructions per stage and image
    constexpr int RPI_Y = 64 / YCH;                                 // rows one dY instruction covers (4 or 8); an X instruction covers 4
    static_assert(NYI % NL == 0 && NXI % NL == 0 && S >= 2, "every loader wave issues the same number of DMAs per stage");
    constexpr int YPL = NYI / NL, XPL = NXI / NL, LPL = YPL + XPL;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int jt = tile % p.njt, ct = (tile / p.njt) % p.nct, zt = tile / (p.njt * p.nct);
    const int pbeg = zt * p.chunk;
    const int pend = min(p.M, pbeg + p.chunk);
    if (wave >= 4) {
        // ---------------- loader waves
        const int lw = wave - 4;
        const int cpt = p.Kc / 8;
        const int nchunks = p.ntaps * cpt;
        const int HoWo = p.Ho * p.Wo;
        u32x4 rsX, rsY;
        {
            const unsigned long long px = (unsigned long long)p.X, py = (unsigned long long)p.dY;
            rsX = u32x4{(unsigned)px, (unsigned)(px >> 32) & 0xffffu, p.bytesX, 0x00020000u};
            rsY = u32x4{(unsigned)py, (unsigned)(py >> 32) & 0xffffu, p.bytesY, 0x00020000u};
        }
        const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
        // dY slots of this lane
        const int yq = lane % YCH, yrl = lane / YCH;
        unsigned yoff[YPL];
        int yrow[YPL];
        unsigned yvmask = 0;
#pragma unroll
        for (int i = 0; i < YPL; ++i) {
            const int row = (lw + NL * i) * RPI_Y + yrl;
            const int ylog = (((yq >> 1) ^ w3f<YROWB>(row)) << 1) | (yq & 1);
            const int co_chunk = ct * TCO + ylog * 8;
            yrow[i] = row;
            if (co_chunk < p.Cout) yvmask |= 1u << i;
            yoff[i] = (unsigned)((pbeg + row) * p.ldy + co_chunk) * 2u;
        }
        const unsigned adv_y = (unsigned)(SP * p.ldy) * 2u;
        // X slots of this lane: (tap, channel chunk) and the running (row, column, byte offset) of its pixel
        const int xq = lane & 15, xrl = lane >> 4;
        int xrow[XPL], xdhw[XPL], xho[XPL], xwo[XPL];
        unsigned xoff[XPL];
        unsigned xvmask = 0;
#pragma unroll
        for (int i = 0; i < XPL; ++i) {
            const int row = (lw + NL * i) * 4 + xrl;
            const int xlog = (((xq >> 1) ^ w3f<256>(row)) << 1) | (xq & 1);
            const int Q = jt * 16 + xlog;
            const bool qv = Q < nchunks;
            const int tap = qv ? Q / cpt : 0;
            const int cc = (Q - tap * cpt) * 8;
            const int dh = tap / p.k - p.p, dw = tap % p.k - p.p;
            xrow[i] = row;
            xdhw[i] = (dh & 0xffff) | (dw << 16);
            if (qv) xvmask |= 1u << i;
            const unsigned m = (unsigned)(pbeg + row);
            const unsigned n = fastdiv40(m, p.magicHW);
            const unsigned rem = m - n * (unsigned)HoWo;
            const unsigned ho = fastdiv40(rem, p.magicW);
            xho[i] = (int)ho; xwo[i] = (int)(rem - ho * (unsigned)p.Wo);
            xoff[i] = (unsigned)((((int)n * p.Hi + xho[i] * p.s + dh) * p.Wi + xwo[i] * p.s + dw) * p.ldx + cc) * 2u;
        }
        const int adv_h = SP / p.Wo, adv_w = SP - adv_h * p.Wo;
        const bool slow_decode = adv_h + 1 > p.Ho;
        const unsigned adv_step = (unsigned)(((adv_h * p.s) * p.Wi + adv_w * p.s) * p.ldx) * 2u;
        const unsigned adv_wrap_w = (unsigned)((p.s * p.Wi - p.Wo * p.s) * p.ldx) * 2u;
        const unsigned adv_wrap_h = (unsigned)(((p.Hi - p.Ho * p.s) * p.Wi) * p.ldx) * 2u;
        auto issue = [&](int p0, int buf) {
            const unsigned base = lds0 + (unsigned)buf * (unsigned)STAGE + (unsigned)lw * 1024u;
#pragma unroll
            for (int i = 0; i < YPL; ++i) {
                const int m = p0 + yrow[i];
                lds_dma16(rsY, base + (unsigned)(NL * i) * 1024u, (((yvmask >> i) & 1u) && m < pend) ? yoff[i] : 0xFFFFFFFFu);
                yoff[i] += adv_y;
            }
#pragma unroll
            for (int i = 0; i < XPL; ++i) {
                const int m = p0 + xrow[i];
                const int dh = (int)(short)(xdhw[i] & 0xffff), dw = xdhw[i] >> 16;
                if (slow_decode) {                       // maps narrower than a stage is long: decode by division
                    const unsigned n = fastdiv40((unsigned)m, p.magicHW);
                    const unsigned rem = (unsigned)m - n * (unsigned)HoWo;
                    const unsigned ho = fastdiv40(rem, p.magicW);
                    xho[i] = (int)ho; xwo[i] = (int)(rem - ho * (unsigned)p.Wo);
                    // (channel chunk of the slot: recovered from the carried offset's low part is not possible here: recompute)
                    const int xlog = (((xq >> 1) ^ w3f<256>(xrow[i])) << 1) | (xq & 1);
                    const int Q = jt * 16 + xlog;
                    const int tap = ((xvmask >> i) & 1u) ? Q / cpt : 0;
                    const int cc = (Q - tap * cpt) * 8;
                    xoff[i] = (unsigned)((((int)n * p.Hi + xho[i] * p.s + dh) * p.Wi + xwo[i] * p.s + dw) * p.ldx + cc) * 2u;
                }
                const int ih = __mul24(xho[i], p.s) + dh, iw = __mul24(xwo[i], p.s) + dw;
                const bool ok = ((xvmask >> i) & 1u) && m < pend && (unsigned)ih < (unsigned)p.Hi && (unsigned)iw < (unsigned)p.Wi;
                lds_dma16(rsX, base + (unsigned)YBYTES + (unsigned)(NL * i) * 1024u, ok ? xoff[i] : 0xFFFFFFFFu);
                xwo[i] += adv_w; xho[i] += adv_h; xoff[i] += adv_step;
                if (xwo[i] >= p.Wo) { xwo[i] -= p.Wo; xho[i] += 1; xoff[i] += adv_wrap_w; }
                if (xho[i] >= p.Ho) { xho[i] -= p.Ho; xoff[i] += adv_wrap_h; }
            }
        };
#pragma unroll
        for (int u = 0; u < S - 1; ++u) issue(pbeg + u * SP, u);
        int nxt = S - 1;
        for (int p0 = pbeg; p0 < pend; p0 += SP) {
            wait_vm_barrier<LPL * (S - 2)>();          // this wave's DMAs of stage k have landed; the multipliers are done with stage k-1
            issue(p0 + (S - 1) * SP, nxt);
            nxt = nxt + 1 == S ? 0 : nxt + 1;
        }
        wait_vm_barrier<0>();                          // the trailing DMAs land before the CTA's LDS goes away
        return;
    }
    // ---------------- multiplier waves
    const int wi = wave / WJ, wj = wave % WJ;
    f32x4 acc[NA][NB];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int g = lane >> 4, lq = (lane & 15) >> 2, lp = lane & 3;
    auto compute = [&](int cur) {
        const unsigned char* by = smem + cur * STAGE;
        const unsigned char* bx = by + YBYTES;
#pragma unroll
        for (int ks = 0; ks < SP / 32; ++ks) {
            uint4 af[NA], bfv[NB];
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                const int row = ks * 32 + g * 8 + lq;
                const unsigned char* lo_p = by + w3sw<YROWB>(row, (wi * 64 + a * 16 + lp * 4) * 2);
                const unsigned char* hi_p = by + w3sw<YROWB>(row + 4, (wi * 64 + a * 16 + lp * 4) * 2);
                s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lo_p));
                s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(hi_p));
                uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
                af[a] = make_uint4(l2.x, l2.y, h2.x, h2.y);
            }
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int row = ks * 32 + g * 8 + lq;
                const unsigned char* lo_p = bx + w3sw<256>(row, (wj * JW + b * 16 + lp * 4) * 2);
                const unsigned char* hi_p = bx + w3sw<256>(row + 4, (wj * JW + b * 16 + lp * 4) * 2);
                s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lo_p));
                s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(hi_p));
                uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
                bfv[b] = make_uint4(l2.x, l2.y, h2.x, h2.y);
            }
#pragma unroll
            for (int a = 0; a < NA; ++a)
#pragma unroll
                for (int b = 0; b < NB; ++b) Mma<bf16_t>::run(af[a], bfv[b], acc[a][b]);
        }
    };
    int buf = 0;
    for (int p0 = pbeg; p0 < pend; p0 += SP) {
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // this wave holds stage k-1 in registers; stage k is in LDS
        compute(buf);
        buf = buf + 1 == S ? 0 : buf + 1;
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");          // (pairs with the loaders' last barrier)
    const size_t wrow = (size_t)p.ntaps * p.Kc;
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            int j = jt * 128 + wj * JW + b * 16 + (lane & 15);
            if (j < (int)wrow) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    int co = ct * TCO + wi * 64 + a * 16 + (lane >> 4) * 4 + e;
                    if (co < p.Cout) {
                        if (p.slab) p.slab[((size_t)zt * p.Cout + co) * wrow + j] = acc[a][b][e];
                        else atomicAdd(p.dW + (size_t)co * p.ldw + j, acc[a][b][e]);
                    }
                }
            }
        }
}

template <int TCO, int SP, int S, int NL>
static int launch_wgrad3s(const Wgrad2Args& a, dim3 grid, hipStream_t st) {
    const size_t smem = (size_t)S * (SP * (TCO * 2) + SP * 256);
    YDL_SET_MAX_LDS((wgrad3s_kernel<TCO, SP, S, NL>), smem);
    wgrad3s_kernel<TCO, SP, S, NL><<<grid, 256 + 64 * NL, smem, st>>>(a);
    YDL_LAUNCH_CHECK();
    return 0;
}

template <int TCO, int SP, int S>
static int launch_wgrad3(const Wgrad2Args& a, dim3 grid, hipStream_t st) {
    const size_t smem = (size_t)S * (SP * (TCO * 2) + SP * 256);
    YDL_SET_MAX_LDS((wgrad3_kernel<TCO, SP, S>), smem);
    wgrad3_kernel<TCO, SP, S><<<grid, 256, smem, st>>>(a);
    YDL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// pwbw: input gradient AND weight gradient of a 1x1 / stride-1 convolution with 128 input and 128 output channels in ONE pass over dy
// (round 5, VERDICT r4 item 3 ii).  Both are HBM-bound on the 160^2 maps of config 2 (the five 128 -> 128 layers: dgrad 47 us for
// dy + dx, wgrad 58 us for x + dy, 210 MB each): run separately dy is fetched twice.  Here a persistent CTA (512 threads, one per CU)
// walks a contiguous pixel range in 32-pixel stages; a stage's dy and x rows arrive by LDS-DMA in wgrad3's swizzled 256-byte-row
// image (S stages, counted vmcnt), and feed
//   * the weight gradient  dW[co][ci] += sum_p dy[p][co] x[p][ci]   — wgrad3's transposed fragment reads, waves 2 (co) x 4 (ci),
//     accumulators live for the whole range, one f32 atomic pass at the end;
//   * the input gradient   dx[p][ci]  = sum_co dy[p][co] wt[ci][co] — wt (32 KB) stationary in LDS, dy fragments read again from the
//     SAME image with ds_read_b128 (conflict-free under its 32-byte-block XOR: the 16 lanes of a read group see all 8 values of
//     f(row) in both 16-byte halves), wave w owns input channels 16 w .. 16 w + 15; results go through a double-buffered staging
//     tile and leave as whole 256-byte pixel rows ONE STAGE LATER (after the ring's barrier — no barrier of their own), optionally
//     added to the previous contents of dx (gradient fan-in).
// HBM bytes: x + dy + dx once (315 MB instead of 420 MB).  Every thread issues the same memory operations per stage — two DMAs, [the
// old dx row chunk,] one store; rows outside the range are out-of-range buffer offsets — so the in-order vmcnt arithmetic is uniform.
// ------------------------------------------------------------------------------------------------------
struct PwbwArgs {
    const bf16_t* X; const bf16_t* dY; const bf16_t* Wt; bf16_t* dX; float* dW;
    int M, ldx, ldy, lddx, ldw, chunk;
    unsigned bytesX, bytesY, bytesDX, bytesWt;
};
#define PWBW_SP 32
struct PwbwBnArgs {
    PwbwArgs c;                     // c.dY is y, c.ldy its pixel stride
    const bf16_t* dO; bf16_t* dYo;  // dout resource base (the lower segment pointer), optional dy_out
    const float *mean, *invstd, *scale, *shift, *sums0, *sums1;
    float *dgamma, *dbeta;
    unsigned segoff[2], bytesDO, bytesDYo;
    int lddo[2], lddyo, nseg, acc_param;
    float invM;
};
__device__ __forceinline__ const PwbwArgs& pwbw_core(const PwbwArgs& a) { return a; }
__device__ __forceinline__ const PwbwArgs& pwbw_core(const PwbwBnArgs& a) { return a.c; }
// BN = 0: dy comes from memory (ydl_conv_bwd_pw, A = PwbwArgs).  BN = 1 + activation (YDL_ACT_NONE / YDL_ACT_SILU): dy is formed from y
// and dout in the kernel (ydl_conv_bwd_pw_bn, A = PwbwBnArgs; see the comment in front of that entry point)
template <int S, bool ACC, int BN = 0, typename A = PwbwArgs>
__global__ __launch_bounds__(512, BN ? 1 : 2) void pwbw_kernel(const A pa) {
    const PwbwArgs& p = pwbw_core(pa);
    constexpr int ACT = BN - 1;
    constexpr int SP = PWBW_SP;
    constexpr int YB = SP * 256;
    constexpr int OD = BN ? 3 : 2;                        // tiles per stage: dy (BN: y, which becomes dy), x, [BN: dout,] [ACC: old dx]
    constexpr int NT = OD + (ACC ? 1 : 0);
    constexpr int STAGE = NT * YB;
    constexpr int LOPS = NT + (BN ? 2 : 1);               // vector-memory operations per thread and stage: NT DMAs + the dx store [+ the dy_out store]
    // younger than a stage's DMAs when its turn comes.  BN = 0: its own store + S - 2 stages.  BN: the stage is needed one iteration
    // earlier, for the transform (derivation in front of ydl_conv_bwd_pw_bn)
    constexpr int NWAIT0 = (S - 2) * LOPS + 1;
    constexpr int NWAIT = BN ? (S - 3) * LOPS + 2 : (S - 2) * LOPS + 1;
    static_assert(S >= 3, "the transform runs one stage ahead of compute()");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const sWt = smem + S * STAGE;          // [128 ci][256 B of co], chunk q of row r at slot q ^ (r & 15)
    unsigned char* const sSt = sWt + 128 * 256;           // [2][32 px][256 B of ci], chunk q of row r at slot q ^ (r & 15)
    [[maybe_unused]] float* const sK = (float*)(sSt + 2 * SP * 256);       // BN: [6][128] scale, shift, mean, invstd, kb, kg
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int pbeg = blockIdx.x * p.chunk;
    const int pend = min(p.M, pbeg + p.chunk);
    const int r = t >> 4, q = t & 15;
    const unsigned qlog = (unsigned)((((q >> 1) ^ w3f<256>(r)) << 1) | (q & 1)) << 4;
    // ---- BN: per-channel constants of this thread's eight channels, BEFORE the first DMA (the compiler's waits for these loads then
    // drain nothing)
    [[maybe_unused]] float sc[8], sf[8], mu[8], is[8], kb[8], kg[8];
    if constexpr (BN != 0) {
    const int ch0 = (int)(qlog >> 4) * 8;
    if (t < 128) {
        const int seg = pa.nseg == 2 ? t >> 6 : 0, cs = pa.nseg == 2 ? 64 : 128, c = t - seg * 64;
        const float* sums = seg ? pa.sums1 : pa.sums0;
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int rr = 0; rr < YDL_BN_REPLICAS; ++rr) {
            s1 += (double)sums[(size_t)(2 * rr) * cs + c];
            s2 += (double)sums[(size_t)(2 * rr + 1) * cs + c];
        }
        const float db = (float)s1, dg = (float)s2;
        if (blockIdx.x == 0) {
            if (pa.dbeta) pa.dbeta[t] = (pa.acc_param ? pa.dbeta[t] : 0.f) + db;
            if (pa.dgamma) pa.dgamma[t] = (pa.acc_param ? pa.dgamma[t] : 0.f) + dg;
        }
        sK[t] = pa.scale[t]; sK[128 + t] = pa.shift[t]; sK[256 + t] = pa.mean[t]; sK[384 + t] = pa.invstd[t];
        sK[512 + t] = db * pa.invM; sK[640 + t] = dg * pa.invM;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        sc[e] = sK[ch0 + e]; sf[e] = sK[128 + ch0 + e]; mu[e] = sK[256 + ch0 + e]; is[e] = sK[384 + ch0 + e];
        kb[e] = sK[512 + ch0 + e]; kg[e] = sK[640 + ch0 + e];
    }
    }
    u32x4 rsX, rsY, rsD, rsW;
    [[maybe_unused]] u32x4 rsO, rsYo;
    {
        const unsigned long long px = (unsigned long long)p.X, py = (unsigned long long)p.dY, pd = (unsigned long long)p.dX,
                                 pw = (unsigned long long)p.Wt;
        rsX = u32x4{(unsigned)px, (unsigned)(px >> 32) & 0xffffu, p.bytesX, 0x00020000u};
        rsY = u32x4{(unsigned)py, (unsigned)(py >> 32) & 0xffffu, p.bytesY, 0x00020000u};
        rsD = u32x4{(unsigned)pd, (unsigned)(pd >> 32) & 0xffffu, p.bytesDX, 0x00020000u};
        rsW = u32x4{(unsigned)pw, (unsigned)(pw >> 32) & 0xffffu, p.bytesWt, 0x00020000u};
        if constexpr (BN != 0) {
            const unsigned long long po = (unsigned long long)pa.dO, pyo = (unsigned long long)pa.dYo;
            rsO = u32x4{(unsigned)po, (unsigned)(po >> 32) & 0xffffu, pa.bytesDO, 0x00020000u};
            rsYo = u32x4{(unsigned)pyo, (unsigned)(pyo >> 32) & 0xffffu, pa.bytesDYo, 0x00020000u};      // (no dy_out: zero bytes, every store dropped)
        }
    }
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned wave_lds = lds0 + (unsigned)wave * 1024u;
    // BN, dout: the thread's chunk lies in segment (chunk >> 3) when there are two
    [[maybe_unused]] unsigned dstride = 0, dcol = 0;
    if constexpr (BN != 0) {
        const int dseg = pa.nseg == 2 ? (int)(qlog >> 7) : 0;
        dstride = (unsigned)((dseg ? pa.lddo[1] : pa.lddo[0]) * 2);
        dcol = (dseg ? pa.segoff[1] : pa.segoff[0]) + (pa.nseg == 2 ? (qlog & 127u) : qlog);
    }
    auto dx_off = [&](int p0) -> unsigned {
        const int m = p0 + r;
        return (m >= pbeg && m < pend) ? (unsigned)m * (unsigned)(p.lddx * 2) + (unsigned)(q << 4) : 0xFFFFFFFFu;
    };
    auto issue = [&](int p0, int buf) {
        const int m = p0 + r;
        const bool ok = m < pend;
        lds_dma16(rsY, wave_lds + (unsigned)buf * STAGE, ok ? (unsigned)m * (unsigned)(p.ldy * 2) + qlog : 0xFFFFFFFFu);
        lds_dma16(rsX, wave_lds + (unsigned)buf * STAGE + YB, ok ? (unsigned)m * (unsigned)(p.ldx * 2) + qlog : 0xFFFFFFFFu);
        if constexpr (BN != 0) lds_dma16(rsO, wave_lds + (unsigned)buf * STAGE + 2 * YB, ok ? (unsigned)m * dstride + dcol : 0xFFFFFFFFu);
        if constexpr (ACC) lds_dma16(rsD, wave_lds + (unsigned)buf * STAGE + OD * YB, dx_off(p0));
    };
    // BN: y and dout of this thread's slot -> dy, over the y slot (rows past the range: zeros, as the DMA of a dy tile leaves them)
    [[maybe_unused]] auto fetch_ydo = [&](int buf, uint4& yq, uint4& dq) {
        yq = *(const uint4*)(smem + buf * STAGE + t * 16);
        dq = *(const uint4*)(smem + buf * STAGE + 2 * YB + t * 16);
    };
    [[maybe_unused]] auto transform = [&](int p0, int buf, const uint4& yq, const uint4& dq) {
        if constexpr (BN != 0) {
            const int m = p0 + r;
            uint4 v = bn_bwd_dy_bf16x8<ACT>(yq, dq, sc, sf, mu, is, kb, kg);
            if (m >= pend) v = make_uint4(0u, 0u, 0u, 0u);
            *(uint4*)(smem + buf * STAGE + t * 16) = v;
            buf_store16_asm(u32x4{v.x, v.y, v.z, v.w}, (m < pend && pa.dYo) ? (unsigned)m * (unsigned)(pa.lddyo * 2) + qlog : 0xFFFFFFFFu, rsYo);
        }
    };
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = r + 32 * i;
        lds_dma16(rsW, lds0 + (unsigned)(S * STAGE) + (unsigned)i * 8192u + (unsigned)wave * 1024u,
                  (unsigned)row * 256u + (unsigned)((q ^ (row & 15)) << 4));
    }
    // prologue: S - 1 stages, each followed by the (dropped) store(s) a loop iteration issues behind its DMAs: the count stays uniform
    // (BN: the last stage's second store is transform(0)'s)
#pragma unroll
    for (int u = 0; u < S - 1; ++u) {
        issue(pbeg + u * SP, u);
        buf_store16_asm(u32x4{0u, 0u, 0u, 0u}, 0xFFFFFFFFu, rsD);
        if (BN != 0 && u < S - 2) buf_store16_asm(u32x4{0u, 0u, 0u, 0u}, 0xFFFFFFFFu, rsD);
    }
    if constexpr (BN != 0) {
        wait_vm_barrier<NWAIT0>();
        uint4 yq, dq;
        fetch_ydo(0, yq, dq);
        transform(pbeg, 0, yq, dq);
    }

    const int lrow = lane & 15, lgrp = lane >> 4;
    const int wi = wave >> 2, wj = wave & 3;
    const int g4 = lane >> 4, lq = (lane & 15) >> 2, lp = lane & 3;
    f32x4 accw[4][2];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) accw[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto trfrag = [&](const unsigned char* tile, int col) -> uint4 {
        const int row = g4 * 8 + lq;
        const unsigned char* lo_p = tile + w3sw<256>(row, col * 2);
        const unsigned char* hi_p = tile + w3sw<256>(row + 4, col * 2);
        s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lo_p));
        s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(hi_p));
        uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
        return make_uint4(l2.x, l2.y, h2.x, h2.y);
    };
    const unsigned char* const wrow = sWt + (wave * 16 + lrow) * 256;
    // weight-gradient fragments (wgrad3's map): waves 2 (co) x 4 (ci), 64 x 32 per wave; input gradient: wave w owns ci 16 w .. 16 w + 15
    // (MFMA A rows), all 32 pixels (two B tiles)
    auto compute = [&](int buf, int sbuf) {
        const unsigned char* by = smem + buf * STAGE;
        const unsigned char* bx = by + YB;
        {
            uint4 af[4], bfv[2];
#pragma unroll
            for (int a = 0; a < 4; ++a) af[a] = trfrag(by, wi * 64 + a * 16 + lp * 4);
#pragma unroll
            for (int b = 0; b < 2; ++b) bfv[b] = trfrag(bx, wj * 32 + b * 16 + lp * 4);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) Mma<bf16_t>::run(af[a], bfv[b], accw[a][b]);
        }
        f32x4 accd[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int ch = ks * 4 + lgrp;
            const uint4 a = *(const uint4*)(wrow + ((ch ^ lrow) << 4));
#pragma unroll
            for (int pt = 0; pt < 2; ++pt) {
                const uint4 b = *(const uint4*)(by + w3sw<256>(pt * 16 + lrow, ch * 16));
                Mma<bf16_t>::run(a, b, accd[pt]);
            }
        }
        unsigned char* const st = sSt + sbuf * (SP * 256);
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
            const int px = pt * 16 + lrow;
            const int chq = wave * 2 + (lgrp >> 1);
            uint2 u;
            u.x = (uint32_t)f2bf(accd[pt][0]) | ((uint32_t)f2bf(accd[pt][1]) << 16);
            u.y = (uint32_t)f2bf(accd[pt][2]) | ((uint32_t)f2bf(accd[pt][3]) << 16);
            *(uint2*)(st + px * 256 + ((chq ^ (px & 15)) << 4) + ((lgrp & 1) << 3)) = u;
        }
    };
    auto fetch_rows = [&](int sbuf, int obuf, uint4& v, uint4& o) {
        v = *(const uint4*)(sSt + sbuf * (SP * 256) + r * 256 + ((q ^ (r & 15)) << 4));
        if constexpr (ACC) o = *(const uint4*)(smem + obuf * STAGE + OD * YB + t * 16);
    };
    auto store_rows = [&](int p0, uint4 v, const uint4& o) {
        if constexpr (ACC) {
            float a8[8], o8[8];
            unpack16<bf16_t>(v, a8);
            unpack16<bf16_t>(o, o8);
#pragma unroll
            for (int e = 0; e < 8; ++e) a8[e] += o8[e];
            v = pack16<bf16_t>(a8);
        }
        buf_store16_asm(u32x4{v.x, v.y, v.z, v.w}, dx_off(p0), rsD);
    };

    int buf = 0, buf1 = 1, nxt = S - 1, k = 0;
    for (int p0 = pbeg; p0 < pend; p0 += SP, ++k) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // own staging / dy-tile writes and fragment reads of the previous stage are done
        wait_vm_barrier<NWAIT>();
        // out of LDS BEFORE the DMAs below overwrite the buffer (nxt) the previous stage's old-dx tile sits in
        uint4 v, o = make_uint4(0u, 0u, 0u, 0u);
        [[maybe_unused]] uint4 yq, dq;
        fetch_rows((k + 1) & 1, nxt, v, o);
        if constexpr (BN != 0) fetch_ydo(buf1, yq, dq);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w), "+v"(o.x), "+v"(o.y), "+v"(o.z), "+v"(o.w)::"memory");
        issue(p0 + (S - 1) * SP, nxt);
        store_rows(p0 - SP, v, o);                               // (stage -1: out-of-range offset, dropped)
        if constexpr (BN != 0) transform(p0 + SP, buf1, yq, dq);
        compute(buf, k & 1);
        buf = buf1;
        buf1 = buf1 + 1 == S ? 0 : buf1 + 1;
        nxt = nxt + 1 == S ? 0 : nxt + 1;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wait_vm_barrier<0>();
    if (k > 0) {
        uint4 v, o = make_uint4(0u, 0u, 0u, 0u);
        fetch_rows((k - 1) & 1, nxt, v, o);                      // (nxt == the last stage's buffer: (k - 1) % S)
        store_rows(pbeg + (k - 1) * SP, v, o);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int j = wj * 32 + b * 16 + (lane & 15);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int co = wi * 64 + a * 16 + (lane >> 4) * 4 + e;
                atomicAdd(p.dW + (size_t)co * p.ldw + j, accw[a][b][e]);
            }
        }
}

static int g_pwbw = 1;          // ydl_debug_set key 15
static bool pwbw_ok(const ydl_conv_geom* g, int dtype) {
    static const int env = getenv("YDL_PWBW") ? atoi(getenv("YDL_PWBW")) : 1;
    if (!env || !g_pwbw || g == nullptr || dtype != YDL_BF16) return false;
    if (g->k != 1 || g->s != 1 || g->p != 0 || g->Cin != 128 || g->Cout != 128) return false;
    if (g->Hi != g->Ho || g->Wi != g->Wo) return false;
    const long long M = (long long)g->N * g->Ho * g->Wo;
    if (M < 131072 || M >= (1ll << 30)) return false;                  // HBM-bound sizes only: the deep layers keep their MFMA kernels
    if (g->ldx < 128 || g->ldy < 128 || (g->ldx & 7) || (g->ldy & 7)) return false;
    if ((unsigned long long)M * (unsigned long long)max(g->ldx, g->ldy) * 2ull >= 0xFFFFFFF0ull) return false;
    return true;
}
extern "C" int ydl_conv_bwd_pw_supported(const ydl_conv_geom* g, int dtype) { return pwbw_ok(g, dtype) ? 1 : 0; }

extern "C" int ydl_conv_bwd_pw(const ydl_conv_geom* g, int dtype, const void* x, const void* dy, const void* wt, void* dx, int lddx,
                               int accumulate, float* dw, void* stream) {
    YDL_CHECK(pwbw_ok(g, dtype), "ydl_conv_bwd_pw: geometry not supported (query ydl_conv_bwd_pw_supported)");
    YDL_CHECK(x && dy && wt && dx && dw, "null pointer");
    YDL_CHECK(aligned16(x) && aligned16(dy) && aligned16(wt) && aligned16(dx), "pointers must be 16-byte aligned");
    YDL_CHECK(lddx >= 128 && (lddx & 7) == 0, "dx pixel stride");
    const int M = g->N * g->Ho * g->Wo;
    YDL_CHECK((unsigned long long)M * (unsigned long long)lddx * 2ull < 0xFFFFFFF0ull, "dx larger than 4 GiB");
    PwbwArgs a{};
    a.X = (const bf16_t*)x; a.dY = (const bf16_t*)dy; a.Wt = (const bf16_t*)wt; a.dX = (bf16_t*)dx; a.dW = dw;
    a.M = M; a.ldx = g->ldx; a.ldy = g->ldy; a.lddx = lddx; a.ldw = g->ldw ? g->ldw : 128;
    int ctas = ydl_device_cus();
    int chunk = (M + ctas - 1) / ctas;
    chunk = (chunk + PWBW_SP - 1) / PWBW_SP * PWBW_SP;
    ctas = (M + chunk - 1) / chunk;
    a.chunk = chunk;
    a.bytesX = (unsigned)((unsigned long long)(M - 1) * g->ldx * 2ull + 256ull);
    a.bytesY = (unsigned)((unsigned long long)(M - 1) * g->ldy * 2ull + 256ull);
    a.bytesDX = (unsigned)((unsigned long long)(M - 1) * lddx * 2ull + 256ull);
    a.bytesWt = 128u * 256u;
    hipStream_t st = (hipStream_t)stream;
    ydl_note_kernel(1, accumulate ? "pwbw_kernel<128,128,acc>" : "pwbw_kernel<128,128>");
    ydl_note_kernel(2, "pwbw_kernel<128,128>");
    if (accumulate) {          // three tiles per stage (the old dx rows travel with the stage): four stages = 96 KB of ring
        constexpr int S = 4;
        const size_t smem = (size_t)S * 3 * PWBW_SP * 256 + 128 * 256 + 2 * PWBW_SP * 256;
        YDL_SET_MAX_LDS((pwbw_kernel<S, true>), smem);
        pwbw_kernel<S, true><<<ctas, 512, smem, st>>>(a);
    } else {
        constexpr int S = 5;
        const size_t smem = (size_t)S * 2 * PWBW_SP * 256 + 128 * 256 + 2 * PWBW_SP * 256;
        YDL_SET_MAX_LDS((pwbw_kernel<S, false>), smem);
        pwbw_kernel<S, false><<<ctas, 512, smem, st>>>(a);
    }
    YDL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// pwbw_kernel<S, ACC, BN != 0>: pwbw for a layer whose dy is the output of a BatchNorm backward that nobody else reads.  The apply launch
// (bn_bwd_apply_sums_kernel: y and dout in, dy out) disappears: a stage brings the 32 rows of y and of dout instead of dy, and the
// thread that issued a 16-byte slot of the y tile (one pixel, the eight channels of logical chunk qlog >> 4 — fixed for the whole
// kernel) reads back its own y and dout slots, forms the eight dy values with the apply kernel's own arithmetic (common.h:
// bn_bwd_dy_bf16x8) and writes them OVER its y slot: the y tile becomes the swizzled dy tile compute() expects, with no change to the
// fragment reads.  HBM: y + dout + x + dx [+ old dx] instead of (y + dout + dy) + (dy + x + dx [+ old dx]).
//   * The transform of stage k + 1 runs in iteration k, behind the ring's barrier and in front of compute(k): the barrier of iteration
//     k + 1 publishes it, there is no second barrier per stage.  A thread reads only what its own DMA lanes wrote, after its own
//     counted vmcnt (and the barrier that follows it).
//   * Per-channel constants (scale, shift, mean, invstd, kb = sum dz / M, kg = sum dz xhat / M) are formed once per CTA — the replica
//     rows summed in double as the apply kernel does — pass through LDS and stay in 48 registers; block 0 writes dgamma / dbeta.
//   * dout comes as one 128-channel segment or as two 64-channel segments with strides of their own (a fused sibling pair activates
//     its halves into two places): ONE buffer resource based at the lower pointer, the segment's distance in the per-thread offset.
//   * dy_out (optional): the thread also stores its 16 bytes, for a second reader of dy.
// Stage = y | x | dout [| old dx] tiles, three (S = 4) or four (S = 3) of 8 KB: 96 KB of ring + 48 KB weights and staging + 3 KB.
// Vector-memory operations per thread and stage, always all of them (out-of-range offsets where there is nothing to do):
//   group j = [ NT DMAs of stage j | dx store of some earlier stage | dy_out store of some earlier stage ],  LOPS = NT + 2.
// The prologue issues groups 0 .. S-2 (dummy stores; the last group's dy_out store is the one of transform(0)); iteration k
// completes group k + S - 1.  Waits (operations younger than the DMAs that must have landed):
//   * before transform(0), the DMAs of group 0: its own two stores, S - 3 whole groups, and group S - 2 without its last store:
//     2 + (S - 3) LOPS + (LOPS - 1) = (S - 2) LOPS + 1;
//   * top of iteration k, the DMAs of group k + 1 (transformed in this iteration; group k's are older): groups up to k + S - 2 are
//     complete, so its own two stores and S - 3 whole groups:  NWAIT = (S - 3) LOPS + 2.
// ------------------------------------------------------------------------------------------------------
extern "C" int ydl_conv_bwd_pw_bn_supported(const ydl_conv_geom* g, int dtype) { return pwbw_ok(g, dtype) ? 1 : 0; }

extern "C" int ydl_conv_bwd_pw_bn(const ydl_conv_geom* g, int dtype, const void* x, const void* y, int ldy, const void* dout0, int lddo0,
                                  const void* dout1, int lddo1, const float* mean, const float* invstd, const float* scale,
                                  const float* shift, const float* sums0, const float* sums1, int64_t npix, int act, float* dgamma,
                                  float* dbeta, int accumulate_param_grads, void* dy_out, int lddy, const void* wt, void* dx, int lddx,
                                  int accumulate, float* dw, void* stream) {
    YDL_CHECK(pwbw_ok(g, dtype), "ydl_conv_bwd_pw_bn: geometry not supported (query ydl_conv_bwd_pw_bn_supported)");
    YDL_CHECK(x && y && dout0 && wt && dx && dw && mean && invstd && scale && shift && sums0, "null pointer");
    YDL_CHECK((dout1 == nullptr) == (sums1 == nullptr), "the second dout segment and its sums come together");
    YDL_CHECK(act == YDL_ACT_NONE || act == YDL_ACT_SILU, "activation must be NONE or SILU");
    YDL_CHECK(aligned16(x) && aligned16(y) && aligned16(dout0) && aligned16(dout1) && aligned16(wt) && aligned16(dx) && aligned16(dy_out),
              "pointers must be 16-byte aligned");
    const int nseg = dout1 ? 2 : 1, segw = dout1 ? 64 : 128;
    YDL_CHECK(lddx >= 128 && (lddx & 7) == 0 && ldy >= 128 && (ldy & 7) == 0, "dx / y pixel stride");
    YDL_CHECK(lddo0 >= segw && (lddo0 & 7) == 0 && (dout1 == nullptr || (lddo1 >= 64 && (lddo1 & 7) == 0)), "dout pixel stride");
    YDL_CHECK(dy_out == nullptr || (lddy >= 128 && (lddy & 7) == 0), "dy_out pixel stride");
    const int M = g->N * g->Ho * g->Wo;
    YDL_CHECK(npix == (int64_t)M, "npix must be the layer's pixel count");
    const unsigned long long rows = (unsigned long long)(M - 1);
    YDL_CHECK((unsigned long long)M * (unsigned long long)lddx * 2ull < 0xFFFFFFF0ull, "dx larger than 4 GiB");
    YDL_CHECK((unsigned long long)M * (unsigned long long)ldy * 2ull < 0xFFFFFFF0ull, "y larger than 4 GiB");
    YDL_CHECK(dy_out == nullptr || (unsigned long long)M * (unsigned long long)lddy * 2ull < 0xFFFFFFF0ull, "dy_out larger than 4 GiB");
    PwbwBnArgs b{};
    PwbwArgs& a = b.c;
    a.X = (const bf16_t*)x; a.dY = (const bf16_t*)y; a.Wt = (const bf16_t*)wt; a.dX = (bf16_t*)dx; a.dW = dw;
    a.M = M; a.ldx = g->ldx; a.ldy = ldy; a.lddx = lddx; a.ldw = g->ldw ? g->ldw : 128;
    int ctas = ydl_device_cus();
    int chunk = (M + ctas - 1) / ctas;
    chunk = (chunk + PWBW_SP - 1) / PWBW_SP * PWBW_SP;
    ctas = (M + chunk - 1) / chunk;
    a.chunk = chunk;
    a.bytesX = (unsigned)(rows * g->ldx * 2ull + 256ull);
    a.bytesY = (unsigned)(rows * ldy * 2ull + 256ull);
    a.bytesDX = (unsigned)(rows * lddx * 2ull + 256ull);
    a.bytesWt = 128u * 256u;
    // dout: one resource from the lower segment pointer; both segments must end within 4 GiB of it
    const uintptr_t d0 = (uintptr_t)dout0, d1 = dout1 ? (uintptr_t)dout1 : d0, dlo = d0 < d1 ? d0 : d1;
    const unsigned long long end0 = (unsigned long long)(d0 - dlo) + rows * lddo0 * 2ull + (unsigned long long)segw * 2ull;
    const unsigned long long end1 = dout1 ? (unsigned long long)(d1 - dlo) + rows * lddo1 * 2ull + 128ull : 0ull;
    YDL_CHECK(end0 < 0xFFFFFFF0ull && end1 < 0xFFFFFFF0ull, "dout segments must lie within 4 GiB of each other");
    b.dO = (const bf16_t*)dlo; b.dYo = (bf16_t*)dy_out;
    b.segoff[0] = (unsigned)(d0 - dlo); b.segoff[1] = (unsigned)(d1 - dlo);
    b.lddo[0] = lddo0; b.lddo[1] = dout1 ? lddo1 : lddo0;
    b.bytesDO = (unsigned)(end0 > end1 ? end0 : end1);
    b.bytesDYo = dy_out ? (unsigned)(rows * lddy * 2ull + 256ull) : 0u;
    b.lddyo = dy_out ? lddy : 0; b.nseg = nseg; b.acc_param = accumulate_param_grads;
    b.mean = mean; b.invstd = invstd; b.scale = scale; b.shift = shift; b.sums0 = sums0; b.sums1 = sums1;
    b.dgamma = dgamma; b.dbeta = dbeta;
    b.invM = 1.0f / (float)npix;
    hipStream_t st = (hipStream_t)stream;
    const bool silu = act == YDL_ACT_SILU;
    // the kernel is pwbw_kernel, as for ydl_conv_bwd_pw (families 1 and 2); family 6 tells how this instantiation gets its dy
    ydl_note_kernel(1, accumulate ? "pwbw_kernel<128,128,acc>" : "pwbw_kernel<128,128>");
    ydl_note_kernel(2, "pwbw_kernel<128,128>");
    ydl_note_kernel(6, accumulate ? (silu ? "pwbw_kernel<128,128,bn-silu,acc>" : "pwbw_kernel<128,128,bn-none,acc>")
                                  : (silu ? "pwbw_kernel<128,128,bn-silu>" : "pwbw_kernel<128,128,bn-none>"));
#define YDL_PWBWBN_LAUNCH(S_, ACC_, ACT_)                                                                       \
    do {                                                                                                        \
        const size_t smem = (size_t)(S_) * ((ACC_) ? 4 : 3) * PWBW_SP * 256 + 128 * 256 + 2 * PWBW_SP * 256 + 6 * 128 * 4; \
        YDL_SET_MAX_LDS((pwbw_kernel<S_, ACC_, 1 + (ACT_), PwbwBnArgs>), smem);                                 \
        pwbw_kernel<S_, ACC_, 1 + (ACT_), PwbwBnArgs><<<ctas, 512, smem, st>>>(b);                              \
    } while (0)
    if (accumulate) {          // four tiles per stage: three stages
        if (silu) YDL_PWBWBN_LAUNCH(3, true, YDL_ACT_SILU);
        else YDL_PWBWBN_LAUNCH(3, true, YDL_ACT_NONE);
    } else {
        if (silu) YDL_PWBWBN_LAUNCH(4, false, YDL_ACT_SILU);
        else YDL_PWBWBN_LAUNCH(4, false, YDL_ACT_NONE);
    }
#undef YDL_PWBWBN_LAUNCH
    YDL_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------------
// Weight gradient of the space-to-depth stem (3x3, stride 1, pad 1, 16 stored input channels -> 64 output channels; BASELINE
// config 2: 16 x 320 x 320 pixels).  K = 9 taps x 16 channels = 144 columns: the tiled kernel above needs TWO 128-column tiles
// (the second one 16 columns wide: every dY byte is fetched twice, half of the MFMAs multiply zeros) and gathers the nine taps of
// every pixel separately — 156 us for 262 MB (1.7 TB/s), the last kernel of the backward pass with nothing to overlap.
// Patch form, like the 3x3 forward kernels: a stage is 64 pixels of ONE output row — dY rows by LDS-DMA in wgrad3's swizzled
// 128-byte-row image, and the 3 x 66 pixel input patch (32 bytes per pixel, 128 bytes of padding behind every 8 pixels so that
// the transposed reads of two 8-pixel groups fall into different bank halves) — all nine taps read the same patch at shifted
// addresses.  Waves: 2 pixel halves (one 32-pixel MFMA K-slice each) x 2 halves of the output channels; a wave owns
// 32 channels x 9 taps x 16 columns = 18 accumulator tiles.  CTAs are persistent over contiguous stage ranges; at the end the
// two pixel halves are added through LDS and the CTA adds its 64 x 144 block to dW with atomics (grid x 36 KB).
// ------------------------------------------------------------------------------------------------------
#define SW_PROW 3456                    // patch row: 9 groups x (8 pixels x 32 B + 128 B padding)
#define SW_YBYTES 8192                  // 64 pixels x 128 B
#define SW_XBYTES 11264                 // 3 patch rows (10368 B) rounded up to whole 1 KiB DMA instructions (11)
#define SW_STAGE (SW_YBYTES + SW_XBYTES)
struct StemwArgs {
    const bf16_t* X; const bf16_t* dY; float* dW;
    int H, W, segs, ldy, ldw, nstages, chunk;
    unsigned bytesX, bytesY;
};
template <int S>
__global__ __launch_bounds__(256, 2) void stemw_kernel(const StemwArgs p) {
    constexpr int L = 5;                        // DMA instructions per wave and stage: 8 (dY) + 11 (patch) + 1 dummy = 20 = 4 x 5
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int h = wave & 1, c = wave >> 1;
    u32x4 rsX, rsY;
    {
        const unsigned long long px = (unsigned long long)p.X, py = (unsigned long long)p.dY;
        rsX = u32x4{(unsigned)px, (unsigned)(px >> 32) & 0xffffu, p.bytesX, 0x00020000u};
        rsY = u32x4{(unsigned)py, (unsigned)(py >> 32) & 0xffffu, p.bytesY, 0x00020000u};
    }
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned dump = lds0 + (unsigned)(S * SW_STAGE);             // 1 KiB nobody reads: destination of the dummy instruction
    // this lane's part of the wave's five instructions i = wave + 4 k: what it fetches is fixed, only the stage origin moves
    int ykind[L];          // 0 = dY, 1 = patch, 2 = dummy
    unsigned dst[L];       // LDS offset inside the stage
    int a0[L], a1[L], a2[L];   // dY: (row, channel offset, -) / patch: (patch row, patch pixel, 16-byte half)
#pragma unroll
    for (int k = 0; k < L; ++k) {
        const int i = wave + 4 * k;
        if (i < 8) {
            const int row = 8 * i + (lane >> 3), qs = lane & 7;
            const int logical = (((qs >> 1) ^ w3f<128>(row)) << 1) | (qs & 1);
            ykind[k] = 0; dst[k] = (unsigned)i * 1024u; a0[k] = row; a1[k] = logical * 8; a2[k] = 0;
        } else if (i < 19) {
            const int o = (i - 8) * 1024 + lane * 16;
            const int pr = o / SW_PROW, rem = o - pr * SW_PROW;
            const int grp = rem / 384, b = rem - grp * 384;
            const int px = grp * 8 + (b >> 5);
            const bool ok = pr < 3 && b < 256 && px < 66;
            ykind[k] = 1; dst[k] = (unsigned)SW_YBYTES + (unsigned)(i - 8) * 1024u;
            a0[k] = ok ? pr : -100000; a1[k] = px; a2[k] = (b >> 4) & 1;
        } else {
            ykind[k] = 2; dst[k] = 0; a0[k] = a1[k] = a2[k] = 0;
        }
    }
    const int pbeg = blockIdx.x * p.chunk;
    const int pend = min(p.nstages, pbeg + p.chunk);
    // (n * H + r, seg) of the next stage to issue
    int inr = pbeg / p.segs, iseg = pbeg - inr * p.segs, isidx = pbeg;
    auto issue = [&](int buf) {
        const unsigned base = lds0 + (unsigned)buf * (unsigned)SW_STAGE;
        const bool live = isidx < pend;
        const int r = inr % p.H;
        const int c0 = iseg * 64;
#pragma unroll
        for (int k = 0; k < L; ++k) {
            if (ykind[k] == 0) {
                const unsigned m = (unsigned)(inr * p.W + c0 + a0[k]);
                lds_dma16(rsY, base + dst[k], live ? (m * (unsigned)p.ldy + (unsigned)a1[k]) * 2u : 0xFFFFFFFFu);
            } else if (ykind[k] == 1) {
                const int row = r - 1 + a0[k], col = c0 - 1 + a1[k];
                const bool ok = live && (unsigned)row < (unsigned)p.H && (unsigned)col < (unsigned)p.W;
                const unsigned pix = (unsigned)((inr - r + row) * p.W + col);
                lds_dma16(rsX, base + dst[k], ok ? (pix * 16u + (unsigned)a2[k] * 8u) * 2u : 0xFFFFFFFFu);
            } else {
                lds_dma16(rsX, dump, 0xFFFFFFFFu);
            }
        }
        ++isidx;
        if (++iseg == p.segs) { iseg = 0; ++inr; }
    };

    f32x4 acc[2][9];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int tp = 0; tp < 9; ++tp) acc[a][tp] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int g = lane >> 4, lq = (lane & 15) >> 2, lp = lane & 3;
    const int krow = h * 32 + g * 8 + lq;                       // this lane's pixel of the stage (low read; the high read is + 4)
    auto compute = [&](int cur) {
        const unsigned char* by = smem + cur * SW_STAGE;
        const unsigned char* bx = by + SW_YBYTES;
        uint4 af[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int colb = (c * 32 + a * 16 + lp * 4) * 2;
            s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(by + w3sw<128>(krow, colb)));
            s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(by + w3sw<128>(krow + 4, colb)));
            uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
            af[a] = make_uint4(l2.x, l2.y, h2.x, h2.y);
        }
#pragma unroll
        for (int ti = 0; ti < 3; ++ti)
#pragma unroll
            for (int tj = 0; tj < 3; ++tj) {
                const int pl = krow + tj, ph = pl + 4;
                const unsigned char* lo_p = bx + ti * SW_PROW + (pl >> 3) * 384 + (pl & 7) * 32 + lp * 8;
                const unsigned char* hi_p = bx + ti * SW_PROW + (ph >> 3) * 384 + (ph & 7) * 32 + lp * 8;
                s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lo_p));
                s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(hi_p));
                uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
                const uint4 bf = make_uint4(l2.x, l2.y, h2.x, h2.y);
#pragma unroll
                for (int a = 0; a < 2; ++a) Mma<bf16_t>::run(af[a], bf, acc[a][ti * 3 + tj]);
            }
    };
#pragma unroll
    for (int u = 0; u < S - 1; ++u) issue(u);
    int buf = 0, nxt = S - 1;
    for (int s0 = pbeg; s0 < pend; ++s0) {
        wait_vm_barrier<L * (S - 2)>();
        issue(nxt);
        compute(buf);
        buf = buf + 1 == S ? 0 : buf + 1;
        nxt = nxt + 1 == S ? 0 : nxt + 1;
    }
    wait_vm_barrier<0>();
    // pixel halves: h = 1 parks its tiles in LDS (the ring is dead), h = 0 adds them and owns the atomics
    f32x4* park = (f32x4*)smem + (size_t)c * 18 * 64;
    if (h == 1) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int tp = 0; tp < 9; ++tp) park[(a * 9 + tp) * 64 + lane] = acc[a][tp];
    }
    __syncthreads();
    if (h == 0) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int tp = 0; tp < 9; ++tp) {
                const f32x4 o = park[(a * 9 + tp) * 64 + lane];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int co = c * 32 + a * 16 + (lane >> 4) * 4 + e;
                    atomicAdd(p.dW + (size_t)co * p.ldw + tp * 16 + (lane & 15), acc[a][tp][e] + o[e]);
                }
            }
    }
}
static int g_stemw = 1;
static bool stemw_ok(const ydl_conv_geom* g, int dtype) {
    return g_stemw && dtype == YDL_BF16 && g->k == 3 && g->s == 1 && g->p == 1 && g->Cin <= 16 && g->Cin > 8 && g->ldx == 16 &&
           g->Cout == 64 && g->Hi == g->Ho && g->Wi == g->Wo && g->Wo % 64 == 0 && (long)g->N * g->Ho * g->Wo >= 65536;
}
static int launch_stemw(const ydl_conv_geom* g, const void* x, const void* dy, float* dw, int ldw, unsigned bx, unsigned by, hipStream_t st) {
    constexpr int S = 4;
    StemwArgs a{};
    a.X = (const bf16_t*)x; a.dY = (const bf16_t*)dy; a.dW = dw;
    a.H = g->Ho; a.W = g->Wo; a.segs = g->Wo / 64; a.ldy = g->ldy; a.ldw = ldw;
    a.nstages = g->N * g->Ho * a.segs;
    constexpr int ctas = 512;
    a.chunk = (a.nstages + ctas - 1) / ctas;
    const int grid = (a.nstages + a.chunk - 1) / a.chunk;
    a.bytesX = bx; a.bytesY = by;
    const size_t smem = (size_t)S * SW_STAGE + 1024;
    static_assert((size_t)S * SW_STAGE >= 2 * 18 * 64 * 16, "the parked accumulators reuse the ring");
    YDL_SET_MAX_LDS((stemw_kernel<S>), smem);
    ydl_note_kernel(2, "stemw_kernel");
    stemw_kernel<S><<<grid, 256, smem, st>>>(a);
    YDL_LAUNCH_CHECK();
    return 0;
}

// ---- wgrad launch plan: a pure function of (geometry, dtype, debug knobs); the workspace query and the launch share it
struct WgradPlan { int kind;     // 0: wgrad_kernel<float>, 1: wgrad_kernel<bf16,tr>, 2: wgrad_kernel<bf16,scalar>, 3: wgrad2<64>, 4: wgrad2<128>
                   int jtiles, ctiles, splits, chunk; };

static int g_wgrad_tr = 1;
static int g_wg3_loaders = -1;   // ydl_debug_set key 18: loader waves of the LDS-DMA weight-gradient kernel (-1: the default, 4; 0 off)
static int wg3_loaders() {
    const int v = g_wg3_loaders >= 0 ? g_wg3_loaders : 4;
    return (v == 1 || v == 2 || v == 4) ? v : 0;
}
static int g_wgrad_dma = 1;      // 128-wide weight-gradient kernel: 1 = LDS-DMA feed (wgrad3_kernel), 0 = register-staged (wgrad2_kernel)

static WgradPlan wgrad_plan(const ydl_conv_geom* g, int dtype) {
    WgradPlan pl{};
    const int Kc = round_up(g->Cin, 8), ntaps = g->k * g->k;
    const int M = g->N * g->Ho * g->Wo;
    // measured on MI355X: the 128-wide pipelined kernel wins on the large-M layers (>= 160x160 at bs 16), the small
    // 64x64-tile kernel (8 CTAs/CU) wins where M is small and the grid of big tiles would be latency-bound
    constexpr int wg2_min_m = 200000;
    // mid-size layers (M below the threshold): the 128-wide kernel sized to exactly ONE wave of CTAs (2 per CU x 256 CUs): its
    // time is very sensitive to the CTA count (atomic volume grows with it, and a second partial wave costs a full tile time) —
    // 128->256 k3s2 @80^2: 270 CTAs 154 us, 396 CTAs 117 us, 522 CTAs 154 us; the 64x64-tile kernel 148 us
    // (3x3 layers only: 256->512 k3s2 @40^2 124 -> 93 us, 256->256 k3 @40^2 67 -> 63 us; the 1x1 layers lose 5-18 us with it)
    constexpr long mid_slots = 512, mid_minfill = 410;
    bool mid = false;
    if (dtype == YDL_BF16 && g_wgrad_tr == 1 && M < wg2_min_m && Kc % 8 == 0) {
        const int TCO = g->Cout > 64 ? 128 : 64;
        const long tiles = (long)((ntaps * Kc + 127) / 128) * ((g->Cout + TCO - 1) / TCO);
        const long sp = mid_slots / tiles;
        mid = sp >= 1 && tiles * sp >= mid_minfill && (M + 63) / 64 >= 4 * sp && ntaps > 1;
    }
    // Round 5: with loader waves the 128-wide kernel also wins on the small-map layers that carry enough work (measured against the
    // 64 x 64-tile kernel, same box: 512->1024 k3s2 @20^2 134 -> 108 us, 2048->1024 @20^2 71 -> 52, 768->128 @80^2 59 -> 53, 512->512 @40^2
    // 35.1 -> 33.5, 1024->1024 @20^2 34.2 -> 32.6; loses below ~13 GFLOP: 128->256 @80^2 25 -> 36, 256->128 @80^2 25.5 -> 28)
    const bool heavy = !mid && wg3_loaders() == 4 && g_wgrad_dma && Kc % 8 == 0 && 2.0 * M * (double)g->Cout * ntaps * Kc >= 12.0e9;
    if (dtype == YDL_BF16 && g_wgrad_tr == 1 && (M >= wg2_min_m || mid || heavy)) {
        const int TCO = g->Cout > 64 ? 128 : 64;
        pl.kind = TCO == 128 ? 4 : 3;
        pl.jtiles = (ntaps * Kc + 127) / 128;
        pl.ctiles = (g->Cout + TCO - 1) / TCO;
        const long tiles = (long)pl.jtiles * pl.ctiles;
        const int stages = (M + 63) / 64;
        if (mid) {
            int splits = (int)(mid_slots / tiles);
            const int per = (stages + splits - 1) / splits;
            pl.chunk = per * 64;
            pl.splits = (M + pl.chunk - 1) / pl.chunk;
            return pl;
        }
        // Split-K CTA count.  Every CTA ends with one atomic pass over its 128 x TCO f32 tile, and device-scope f32 atomics
        // sustain only ~1.3 TB/s chip-wide (measured), so the atomic volume T * tile_bytes is budgeted at ~20-30 % of the
        // layer's streaming/MFMA time: short 1x1 layers get 256 CTAs, long 3x3 layers up to 2048 (measured optimum per layer
        // on MI355X: 128->128 k1 @160: 256 CTAs 55 us vs 1024 CTAs 92 us; 128->64 k3 @160: 1024-1536 CTAs).
        long target2;
        {
            const double bytes_in = ((double)g->N * g->Hi * g->Wi * g->Cin + (double)M * g->Cout) * 2.0;
            const double flops = 2.0 * M * g->Cout * ntaps * Kc;
            const double d0 = bytes_in / 4.5e12 > flops / 450e12 ? bytes_in / 4.5e12 : flops / 450e12;
            const double share = Kc <= 16 ? 0.3 : 0.2;      // measured: the 3-channel stem prefers more, shorter CTAs
            const double t = share * d0 * 1.3e12 / (128.0 * TCO * 4.0);
            target2 = (long)(t / 256.0 + 0.5) * 256;
            if (target2 < 256) target2 = 256;
            if (target2 > 2048) target2 = 2048;
        }
        int splits = (int)((target2 + tiles - 1) / tiles);
        if (splits > stages / 4) splits = stages / 4;
        if (splits < 1) splits = 1;
        if (splits > 1024) splits = 1024;
        const int per = (stages + splits - 1) / splits;
        pl.chunk = per * 64;
        pl.splits = (M + pl.chunk - 1) / pl.chunk;
        return pl;
    }
    pl.kind = dtype == YDL_F32 ? 0 : (g_wgrad_tr ? 1 : 2);
    const int TE = dtype == YDL_F32 ? 32 : 64;
    pl.jtiles = (ntaps * Kc + TE - 1) / TE;
    pl.ctiles = (g->Cout + TE - 1) / TE;
    // split-K over pixels.  Every split adds one f32 atomic pass over the dW tile (chip-wide atomic rate ~1.3 TB/s),
    // so splits are bounded by the CTA target
    const long tiles = (long)pl.jtiles * pl.ctiles;
    const int stages = (M + WG_BKP - 1) / WG_BKP;
    // (measured: the short 1x1 layers are atomic-bound earlier: 1024 CTAs beat 2048 there, 3x3 layers are flat 2048-4096)
    const long target_ctas = ntaps == 1 ? 1024 : 2048;
    int splits = (int)((target_ctas + tiles - 1) / tiles);
    if (splits > stages / 4) splits = stages / 4;
    if (splits < 1) splits = 1;
    if (splits > 1024) splits = 1024;
    const int per = (stages + splits - 1) / splits;
    pl.chunk = per * WG_BKP;
    pl.splits = (M + pl.chunk - 1) / pl.chunk;
    return pl;
}

// deterministic split-K: dW[co][j] += slab[0][co][j] + slab[1][co][j] + ... in that fixed order (one thread per element)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slab, float* __restrict__ dW, int splits,
                                                           int Cout, int wrow, int ldw) {
    const size_t n = (size_t)Cout * wrow;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float s = 0.f;
        for (int z = 0; z < splits; ++z) s += slab[(size_t)z * n + i];
        const size_t co = i / wrow, j = i - co * wrow;
        dW[co * ldw + j] += s;
    }
}

// debug knobs: key 0 = bf16 wgrad path: 1 (default) 128-wide tr-read kernel, 2 64x64 tr-read kernel, 0 64x64 scalar-LDS-read kernel
//              key 2 = strided dgrad: 1 (default) all output-parity classes in one launch, 0 one launch per class
//              key 1 = streaming point-wise kernel for short-K 1x1 convolutions: 1 (default) on, 0 off (tiled kernel everywhere)
//              key 3 = bf16 LDS-DMA ring kernel (igemm2) for the MFMA-bound layers: 1 (default) on, 0 off (igemm_kernel everywhere)
//              key 8 = patch-form kernel for the 3x3 / stride-1 layers (igemm2h_kernel): 1 (default) on, 0 ring kernel
//              key 9 = fused-parity kernel for the k3 s2 p1 data gradients (igemm2s_kernel): 1 (default) on, 0 ring kernel
//              key 10 = integer-factor bilinear resize backward (resize_bwd_int_kernel): 1 (default) on, 0 generic gather
//              key 11 = row-walking resize forward: 1 (default) on, 0 element-indexed kernel
//              key 12 = patch-form weight gradient of the space-to-depth stem (stemw_kernel): 1 (default) on, 0 tiled kernel
//              key 20 = deformable-convolution backward with the LDS window (deform_bwd_window_kernel): 1 (default) on, 0 per-corner atomics
//              key 19 = loader-wave ring kernel (igemm2l_kernel) where pick_cfg prefers it: 1 (default) on, 0 off
//              key 18 = loader waves of the LDS-DMA weight-gradient kernel (wgrad3s_kernel): 4 (default) / 2 / 1 loader waves per CTA, 0 = wgrad3_kernel
//              key 17 = weights-in-registers kernel for 3x3 / s1 over one 64-channel block (igemm2w_kernel): 1 (default) on, 0 off
//              key 16 = DCNv3 tile backward (grad_input scatter as S x grad_output on the MFMA): 1 (default) on, 0 off
//              key 15 = one-pass input + weight gradient of the 128 -> 128 1x1 layers (pwbw_kernel): 1 (default) on, 0 two launches
//              key 14 = accumulating point-wise launches: 1 (default) per-wave transposed stores also with statistics, 2 only without, 0 never
//              key 13 = DCNv3 backward with the register window (dcnv3_bwd_win_kernel): 1 (default) on, 0 plain per-corner atomics
//              key 6 = persistent form of the two-stage ring kernel (igemm2p_kernel): 1 (default) on, 0 off
//              key 5 = thin-input 3x3 kernel for the space-to-depth stem: 1 (default) on, 0 off (tiled kernel)
//              key 4 = 128-wide bf16 weight-gradient kernel: 1 (default) LDS-DMA feed (wgrad3_kernel), 0 register-staged (wgrad2_kernel)
// Process-wide and test-only: they change launch geometry, so callers that cache ydl_conv_fwd_grid_m/... must drop the cache
// after a change (yolo_dual_amd._lib.debug_set does).
extern int g_resize_int, g_resize_rows;       // spatial.hip
void ydl_dcn_debug_set(int key, int val);     // dcnv3.hip
void ydl_deform_debug_set(int key, int val);  // deform.hip
extern "C" void ydl_debug_set(int key, int val) {
    ydl_dcn_debug_set(key, val);
    ydl_deform_debug_set(key, val);
    if (key == 0) g_wgrad_tr = val;
    if (key == 1) g_pw_enabled = val;
    if (key == 2) g_dgrad_merge = val;
    if (key == 3) g_ring_enabled = val;
    if (key == 4) g_wgrad_dma = val;
    if (key == 5) g_stem_enabled = val;
    if (key == 6) g_ring_persist = val;
    if (key == 8) g_halo = val;
    if (key == 9) g_s2fused = val;
    if (key == 10) g_resize_int = val;
    if (key == 11) g_resize_rows = val;
    if (key == 12) g_stemw = val;
    if (key == 14) g_pw_acc_ts = val;
    if (key == 15) g_pwbw = val;
    if (key == 17) g_wreg = val;
    if (key == 18) g_wg3_loaders = val;
    if (key == 19) g_ring_loaders = val;
}

extern "C" int64_t ydl_conv_wgrad_ws_bytes(const ydl_conv_geom* g, int dtype) {
    if (g == nullptr || g->Cin <= 0 || g->Cout <= 0 || g->k < 1) return 0;
    const WgradPlan pl = wgrad_plan(g, dtype);
    return (int64_t)pl.splits * g->Cout * (int64_t)(g->k * g->k * round_up(g->Cin, 8)) * (int64_t)sizeof(float);
}

static int conv_wgrad_impl(const ydl_conv_geom* g, int dtype, const void* x, const void* dy, float* dw, float* slab, void* stream) {
    if (int e = check_geom(g, dtype)) return e;
    YDL_CHECK(aligned16(x) && aligned16(dy) && aligned16(dw), "pointers must be 16-byte aligned");
    const int V = dtype == YDL_F32 ? 4 : 8;
    YDL_CHECK(g->ldy >= round_up(g->Cout, V), "dy pixel stride must cover Cout rounded up to a 16-byte chunk");
    const WgradPlan pl = wgrad_plan(g, dtype);
    const int Kc = round_up(g->Cin, 8), ntaps = g->k * g->k;
    const int M = g->N * g->Ho * g->Wo;
    const unsigned long long es = (unsigned long long)esize(dtype);
    const unsigned long long bx = (unsigned long long)g->N * g->Hi * g->Wi * g->ldx * es, by = (unsigned long long)M * g->ldy * es;
    // pixel decode by multiply-shift with magic = ceil(2^40 / d), d <= Ho*Wo: exact for every n <= M while M * d < 2^40
    YDL_CHECK(bx < 0xFFFFFFF0ull && by < 0xFFFFFFF0ull && (unsigned long long)M * ((unsigned long long)g->Ho * g->Wo) < (1ull << 40),
              "tensor too large for the 32-bit wgrad addressing");
    YDL_CHECK(g->Ho < (1 << 21) && g->Wo < (1 << 21), "map side of 2^21 or more: not supported by the weight-gradient kernels (24-bit row / column arithmetic)");
    const unsigned long long magicW = ((1ull << 40) + g->Wo - 1) / g->Wo;
    const unsigned long long magicHW = ((1ull << 40) + (unsigned long long)g->Ho * g->Wo - 1) / ((unsigned long long)g->Ho * g->Wo);
    const int ldw = g->ldw ? g->ldw : ntaps * Kc;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(pl.jtiles * pl.ctiles * pl.splits);
    if (slab == nullptr && stemw_ok(g, dtype)) return launch_stemw(g, x, dy, dw, ldw, (unsigned)bx, (unsigned)by, st);
    if (pl.kind >= 3) {
        Wgrad2Args a{};
        a.X = (const bf16_t*)x; a.dY = (const bf16_t*)dy; a.dW = dw;
        a.N = g->N; a.Hi = g->Hi; a.Wi = g->Wi; a.ldx = g->ldx; a.Kc = Kc;
        a.Ho = g->Ho; a.Wo = g->Wo; a.ldy = g->ldy; a.Cout = g->Cout;
        a.k = g->k; a.s = g->s; a.p = g->p; a.ntaps = ntaps;
        a.ldw = ldw; a.M = M; a.chunk = pl.chunk;
        a.bytesX = (unsigned)bx; a.bytesY = (unsigned)by; a.magicW = magicW; a.magicHW = magicHW;
        a.njt = pl.jtiles; a.nct = pl.ctiles; a.slab = slab;
        if (g_wgrad_dma) {
            // loader-wave form (wgrad3s_kernel): four loader waves per CTA by default (ydl_debug_set key 18 = 0: every wave loads and
            // multiplies, wgrad3_kernel; 1, 2: fewer loader waves — measured slower than no split, 4: -12..-20 % on every layer)
            // (ring shape, measured with four loaders: 32-pixel stages x 4; 64 x 2 is equal within 3 % either way, 64 x 3 — one CTA per
            //  CU — loses 10-20 % on the 3x3 layers)
            const int loaders = wg3_loaders();
            int e = 0;
            if (loaders) {
                ydl_note_kernel(2, pl.kind == 4 ? "wgrad3s_kernel<128>" : "wgrad3s_kernel<64>");
                if (pl.kind == 4) e = loaders == 1 ? launch_wgrad3s<128, 32, 4, 1>(a, grid, st) : (loaders == 2 ? launch_wgrad3s<128, 32, 4, 2>(a, grid, st) : launch_wgrad3s<128, 32, 4, 4>(a, grid, st));
                else e = loaders == 1 ? launch_wgrad3s<64, 32, 4, 1>(a, grid, st) : (loaders == 2 ? launch_wgrad3s<64, 32, 4, 2>(a, grid, st) : launch_wgrad3s<64, 32, 4, 4>(a, grid, st));
            } else {
                ydl_note_kernel(2, pl.kind == 4 ? "wgrad3_kernel<128>" : "wgrad3_kernel<64>");
                e = pl.kind == 4 ? launch_wgrad3<128, 32, 4>(a, grid, st) : launch_wgrad3<64, 32, 4>(a, grid, st);
            }
            if (e) return e;
        } else {
            const size_t smem = 4 * 64 * W2_ROWB;
            YDL_SET_MAX_LDS((wgrad2_kernel<128>), smem);
            YDL_SET_MAX_LDS((wgrad2_kernel<64>), smem);
            ydl_note_kernel(2, pl.kind == 4 ? "wgrad2_kernel<128>" : "wgrad2_kernel<64>");
            if (pl.kind == 4) wgrad2_kernel<128><<<grid, 256, smem, st>>>(a);
            else wgrad2_kernel<64><<<grid, 256, smem, st>>>(a);
            YDL_LAUNCH_CHECK();
        }
    } else {
        WgradArgs a{};
        a.X = x; a.dY = dy; a.dW = dw;
        a.N = g->N; a.Hi = g->Hi; a.Wi = g->Wi; a.ldx = g->ldx; a.Kc = Kc;
        a.Ho = g->Ho; a.Wo = g->Wo; a.ldy = g->ldy; a.Cout = g->Cout;
        a.k = g->k; a.s = g->s; a.p = g->p; a.ntaps = ntaps;
        a.ldw = ldw; a.M = M; a.chunk = pl.chunk;
        a.bytesX = (unsigned)bx; a.bytesY = (unsigned)by; a.magicW = magicW; a.magicHW = magicHW;
        a.njt = pl.jtiles; a.nct = pl.ctiles; a.slab = slab;
        if (pl.kind == 0) { ydl_note_kernel(2, "wgrad_kernel<f32>"); wgrad_kernel<float, false><<<grid, 256, 0, st>>>(a); }
        else if (pl.kind == 1) { ydl_note_kernel(2, "wgrad_kernel<bf16,tr>"); wgrad_kernel<bf16_t, true><<<grid, 256, 0, st>>>(a); }
        else { ydl_note_kernel(2, "wgrad_kernel<bf16,scalar>"); wgrad_kernel<bf16_t, false><<<grid, 256, 0, st>>>(a); }
        YDL_LAUNCH_CHECK();
    }
    if (slab) {
        const int wrow = ntaps * Kc;
        const size_t n = (size_t)g->Cout * wrow;
        int blocks = (int)((n + 255) / 256);
        if (blocks > 2048) blocks = 2048;
        wgrad_reduce_kernel<<<blocks, 256, 0, st>>>(slab, dw, pl.splits, g->Cout, wrow, ldw);
        YDL_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int ydl_conv_wgrad(const ydl_conv_geom* g, int dtype, const void* x, const void* dy, float* dw, void* stream) {
    return conv_wgrad_impl(g, dtype, x, dy, dw, nullptr, stream);
}

extern "C" int ydl_conv_wgrad_det(const ydl_conv_geom* g, int dtype, const void* x, const void* dy, float* dw, float* ws,
                                  void* stream) {
    YDL_CHECK(ws != nullptr && aligned16(ws), "deterministic wgrad needs a 16-byte aligned workspace of ydl_conv_wgrad_ws_bytes()");
    return conv_wgrad_impl(g, dtype, x, dy, dw, ws, stream);
}
