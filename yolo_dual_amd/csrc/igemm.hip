// Implicit-GEMM convolution on MFMA for gfx950: forward and dgrad (same kernel, different tap tables); wgrad.hip has the weight gradients.
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
#include "conv_common.h"

#define GROWB 128     // igemm tiles: unpadded rows, XOR-swizzled chunks


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

// ---- set-up shared by the tiled kernels: everything a CTA derives from its tile before the K loop ----------------------------------
// The tile a CTA works on.  A pixel tile belongs to ONE output-parity class (stride-s dgrad: one launch covers all s*s classes), which
// selects its slice of the tap table and its output sub-grid; ncls <= 1: the single-class fields of the arguments.  All values are
// wave-uniform (scalar loads).  ``tile`` is the linear tile index after xcd_remap.
struct ConvTile { int mtile, ntile, ntaps, tap0, Hg, Wg, M, h0, w0; };
__device__ __forceinline__ ConvTile tile_of(const IgemmArgs& p, int tile) {
    ConvTile ti;
    if (p.m_fastest) { ti.ntile = tile / p.grid_m; ti.mtile = tile - ti.ntile * p.grid_m; }
    else { ti.mtile = tile / p.grid_n; ti.ntile = tile - ti.mtile * p.grid_n; }
    ti.ntaps = p.ntaps; ti.tap0 = 0; ti.Hg = p.Hg; ti.Wg = p.Wg; ti.M = p.M; ti.h0 = p.out_h0; ti.w0 = p.out_w0;
    if (p.ncls > 1) {
        int c = 0;
        while (c + 1 < p.ncls && ti.mtile >= p.cls_tile0[c + 1]) ++c;
        ti.mtile -= p.cls_tile0[c];
        ti.ntaps = p.cls_ntaps[c]; ti.tap0 = p.cls_tap0[c]; ti.Hg = p.cls_Hg[c]; ti.Wg = p.cls_Wg[c]; ti.M = p.cls_M[c];
        ti.h0 = p.cls_h0[c]; ti.w0 = p.cls_w0[c];
    }
    return ti;
}

// The three tap tables [MAXTAPS] of taps tap0 .. tap0 + ntaps - 1 (zeros beyond): sTapA = byte delta of the tap in A, sTapB = byte offset
// of the tap inside a weight row, sTapD = (dh & 0xffff) | (dw << 16).  The caller's barrier makes them visible.
__device__ __forceinline__ void fill_tap_tables(const IgemmArgs& p, int t, int ntaps, int tap0, int es, int* sTapA, int* sTapB, int* sTapD) {
    if (t < MAXTAPS) {
        int da = 0, db = 0, dd = 0;
        if (t < ntaps) {
            da = ((int)p.dh[tap0 + t] * p.Wi + (int)p.dw[tap0 + t]) * p.lda * es;
            db = (int)p.wt[tap0 + t] * p.Kc * es;
            dd = ((int)p.dh[tap0 + t] & 0xffff) | ((int)p.dw[tap0 + t] << 16);
        }
        sTapA[t] = da;
        sTapB[t] = db;
        sTapD[t] = dd;
    }
}

// Per-thread LDS-DMA row descriptors of a tile (igemm2_kernel, igemm2p_kernel; igemm2l_kernel's loader waves keep their own copy, see
// there).  The thread owns tile rows row0 + stride * i of both operands and
// fetches the logical 16-byte chunk at byte q16 of a K-step.  rowoff = byte offset of the row's (0,0) tap in A, vmask = bit tp set when
// tap tp of the tile (sTapD[tp]) lies inside the image (tail rows: no tap is valid => zeros), browoff = byte offset of the weight row;
// rows beyond Cout get a poisoned offset that stays out of range whatever is added to it.
template <int NA, int NB>
__device__ __forceinline__ void row_descriptors(const IgemmArgs& p, const ConvTile& ti, int m0, int n0, int row0, int stride, unsigned q16,
                                                const int* sTapD, unsigned (&rowoff)[NA], unsigned (&vmask)[NA], unsigned (&browoff)[NB]) {
    int ih0[NA], iw0[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int m = m0 + row0 + stride * i;
        rowoff[i] = 0;
        vmask[i] = 0;
        ih0[i] = -100000;
        iw0[i] = 0;
        if (m < ti.M) {
            const int gw = m % ti.Wg;
            const int tmp = m / ti.Wg;
            const int gh = tmp % ti.Hg;
            const int n = tmp / ti.Hg;
            ih0[i] = gh * p.in_mul;
            iw0[i] = gw * p.in_mul;
            rowoff[i] = (unsigned)(((n * p.Hi + ih0[i]) * p.Wi + iw0[i]) * p.lda) * 2u + q16;
        }
    }
    for (int tp = 0; tp < ti.ntaps; ++tp) {            // uniform loop, broadcast LDS reads
        const int dd = sTapD[tp];
        const int dh = (int)(short)(dd & 0xffff), dw = dd >> 16;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const bool ok = (unsigned)(ih0[i] + dh) < (unsigned)p.Hi && (unsigned)(iw0[i] + dw) < (unsigned)p.Wi;
            vmask[i] |= ok ? (1u << tp) : 0u;
        }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int co = n0 + row0 + stride * i;
        browoff[i] = co < p.Cout ? (unsigned)co * p.ldb_bytes + q16 : 0xF0000000u;
    }
}

// Raw buffer descriptors of the two operands (out-of-range offsets read zeros: padding taps, tail rows, K-steps beyond the end)
__device__ __forceinline__ void ring_rsrc(const IgemmArgs& p, u32x4& rsA, u32x4& rsB) {
    rsA = buf_rsrc(p.A, p.bytesA);
    rsB = buf_rsrc(p.B, p.bytesB);
}

// Fragment reads and MFMAs of one wave of a ring stage [BM activation rows][BN weight rows] x GROWB: wave (wc, wp) of the WN x WP grid
// multiplies BN / WN channels (MFMA A operand) by BM / WP pixels (B operand); a K-step is two halves of four 16-byte chunks.
template <int BM, int BN, int NW, int WP>
struct RingFrag {
    static constexpr int BNW = BN / (NW / WP), CT = BNW / 16, PT = BM / (16 * WP), STAGE = (BM + BN) * GROWB;
    const unsigned char *fa, *fb;
    int lk0, lk1;
    __device__ __forceinline__ RingFrag(const unsigned char* smem, int lane, int wc, int wp) {
        const int lrow = lane & 15;
        const int sw_rd = (lrow >> 1) & 7;
        lk0 = (((lane >> 4)) ^ sw_rd) << 4;
        lk1 = (((lane >> 4) + 4) ^ sw_rd) << 4;
        fa = smem + BM * GROWB + (wc * BNW + lrow) * GROWB;
        fb = smem + (wp * (BM / WP) + lrow) * GROWB;
    }
    __device__ __forceinline__ void read(int stg, int half, uint4 (&af)[CT], uint4 (&bfr)[PT]) const {
        const unsigned char* a_base = fa + stg * STAGE + (half ? lk1 : lk0);
        const unsigned char* b_base = fb + stg * STAGE + (half ? lk1 : lk0);
#pragma unroll
        for (int c = 0; c < CT; ++c) af[c] = *(const uint4*)(a_base + c * 16 * GROWB);
#pragma unroll
        for (int j = 0; j < PT; ++j) bfr[j] = *(const uint4*)(b_base + j * 16 * GROWB);
    }
    static __device__ __forceinline__ void mma(const uint4 (&af)[CT], const uint4 (&bfr)[PT], f32x4 (&acc)[CT][PT]) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int j = 0; j < PT; ++j) Mma<bf16_t>::run(af[c], bfr[j], acc[c][j]);
    }
};

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
    const ConvTile ti = tile_of(p, xcd_remap(blockIdx.x, gridDim.x));      // (m_fastest = 0: N-tiles of one pixel tile are neighbours)
    const int m0 = ti.mtile * BM, n0 = ti.ntile * BN;
    fill_tap_tables(p, t, ti.ntaps, ti.tap0, ES, sTapA, sTapB, sTapD);

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
        if (m < ti.M) {
            int gw = m % ti.Wg;
            int tmp = m / ti.Wg;
            int gh = tmp % ti.Hg;
            int n = tmp / ti.Hg;
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
    const int nchunks = ti.ntaps * cpt;
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

    igemm_epilogue<T, BM, BN, NW, WP>(p, acc, smem, m0, n0, ti.mtile, ti.M, ti.Wg, ti.Hg, ti.h0, ti.w0);
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

// STG (round 5): the eight waves of the CTA as two HALVES that run half a K-step apart.  Waves i and i + 4 share a SIMD; in the
// plain form both reach their fragment reads, their DMA issue and their MFMAs together, so the matrix pipe idles while both load and
// both queue for it afterwards.  Here waves 0-3 run   barrier_k | read(k) | issue | MFMA(k)          and waves 4-7 run
// barrier_k | MFMA(k-1) | issue | read(k)   — the younger half keeps a whole K-step of fragments in registers across the barrier and
// computes it while the older half loads: on every SIMD one wave is in its matrix segment while its partner is in its LDS / DMA
// segment.  Same barrier count, same DMA count per thread and step (the counted vmcnt is unchanged), results bit-identical.
template <int BM, int BN, int NW, int WP, int S, bool RED = false, int STG = 0>
__global__ __launch_bounds__(NW * 64, RED ? NW / 2 : 1) void igemm2_kernel(const IgemmArgs p) {
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
    const ConvTile ti = tile_of(p, xcd_remap(blockIdx.x, gridDim.x));
    const int m0 = ti.mtile * BM, n0 = ti.ntile * BN;
    fill_tap_tables(p, t, ti.ntaps, ti.tap0, ES, sTapA, sTapB, sTapD);
    float* const sCoef = (float*)(sTapD + MAXTAPS);      // RED: [BN][4] BatchNorm coefficients of this tile's channels
    if constexpr (RED) br_fill_coef<BN>(p, sCoef, n0, t);
    __syncthreads();   // tap tables visible (no DMA is in flight yet)

    // this thread's DMA slot: row r of each pass, 16-byte slot qs; it fetches the logical chunk q = qs ^ swizzle(r)
    const int r = t >> 3;
    const int qs = t & 7;
    const unsigned q16 = (unsigned)((qs ^ ((r >> 1) & 7)) << 4);
    unsigned rowoff[AR], vmask[AR], browoff[BR];
    row_descriptors(p, ti, m0, n0, r, RPP, q16, sTapD, rowoff, vmask, browoff);
    const int spt = p.Kc >> 6;                  // 64-channel blocks (Kc % 64 == 0)
    const int nk = ti.ntaps * spt;
    u32x4 rsA, rsB;
    ring_rsrc(p, rsA, rsB);
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
        if (++tap == ti.ntaps) { tap = 0; ++cb; }
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

    const RingFrag<BM, BN, NW, WP> fr(smem, lane, wc, wp);
    // Software-pipelined fragment reads: the fragments of half-step h+1 are in flight while the 16*... MFMAs of half-step h
    // issue (two register sets).  The wait + barrier that opens step k+1 sits between the two MFMA batches of step k:
    //   read F1 = frags(k, half 1) | MFMA(F0) | lgkmcnt(0), vmcnt, barrier | issue DMAs(k+S) | read F0 = frags(k+1, half 0) | MFMA(F1)
    // (by then every wave holds all of step k's fragments in registers, so the DMAs of step k+S may overwrite its stage)
    uint4 af0[CT], bf0[PT], af1[CT], bf1[PT];
    if constexpr (STG != 0) {
        static_assert(NW == 8, "the stagger splits the CTA into waves 0-3 and 4-7");
        auto rd_step = [&](int stg) { fr.read(stg, 0, af0, bf0); fr.read(stg, 1, af1, bf1); };
        auto mma_step = [&]() { fr.mma(af0, bf0, acc); fr.mma(af1, bf1, acc); };
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
        fr.read(0, 0, af0, bf0);
    }
    for (int kk0 = 0; kk0 < nk; kk0 += S) {
#pragma unroll
        for (int u = 0; u < S; ++u) {
            const int kk = kk0 + u;
            if (kk < nk) {
                fr.read(u, 1, af1, bf1);
                fr.mma(af0, bf0, acc);
                if (kk + 1 < nk) {
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave holds all of step kk in registers
                    wait_vm_barrier<L * (S - 2)>();                         // step kk+1 landed everywhere
                    issue(u);                                               // step kk+S -> the stage step kk occupied
                    fr.read((u + 1) % S, 0, af0, bf0);
                }
                fr.mma(af1, bf1, acc);
            }
        }
    }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wait_vm_barrier<0>();              // the trailing all-zero DMAs must land before the epilogue reuses the LDS
    igemm2_epilogue<BM, BN, NW, WP, RED>(p, acc, smem, m0, n0, ti.mtile, ti.M, ti.Wg, ti.Hg, ti.h0, ti.w0, sCoef);
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
    const ConvTile ti = tile_of(p, xcd_remap(blockIdx.x, gridDim.x));
    const int m0 = ti.mtile * BM, n0 = ti.ntile * BN;
    fill_tap_tables(p, t, ti.ntaps, ti.tap0, ES, sTapA, sTapB, sTapD);
    __syncthreads();   // tap tables visible (no DMA is in flight yet)
    const int spt = p.Kc >> 6;
    const int nk = ti.ntaps * spt;

    if (wave >= NW) {
        // ---------------- loader waves
        const int lw = wave - NW;
        const int r8 = lane >> 3, qs = lane & 7;
        const unsigned q16 = (unsigned)((qs ^ (((r8 >> 1) | ((lw & 1) << 2)) & 7)) << 4);      // (row >> 1) & 7 with row = 8 j + r8, j = lw (mod 2)
        // (the same descriptors as row_descriptors, written out: through the helper the loader waves, whose set-up is on the path to the
        //  first DMA, came out with 25 more scalar loads and 12 more waits, and 3..8 % slower on the short-K layers)
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
            for (int tp = 0; tp < ti.ntaps; ++tp) {            // uniform loop, broadcast LDS reads
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
        ring_rsrc(p, rsA, rsB);
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
            if (++tap == ti.ntaps) { tap = 0; ++cb; }
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
    const RingFrag<BM, BN, NW, WP> fr(smem, lane, wc, wp);
    uint4 af0[CT], bf0[PT], af1[CT], bf1[PT];
    // barrier count: one per K-step (opening it) + the closing one — the same nk + 1 the loaders execute
    constexpr bool PIPE = NW >= 8;     // 64 x 64 wave tiles of a 4-wave CTA: ONE fragment set (the second costs 32 registers the two-CTA form lacks)
    if constexpr (PIPE) {
        if (nk > 0) {
            asm volatile("s_barrier" ::: "memory");            // step 0 landed everywhere
            fr.read(0, 0, af0, bf0);
        }
        int stg = 0;
        for (int kk = 0; kk < nk; ++kk) {
            fr.read(stg, 1, af1, bf1);
            fr.mma(af0, bf0, acc);
            stg = stg + 1 == S ? 0 : stg + 1;
            if (kk + 1 < nk) {
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // this wave holds all of step kk; step kk+1 landed everywhere
                fr.read(stg, 0, af0, bf0);
            }
            fr.mma(af1, bf1, acc);
        }
    } else {
        int stg = 0;
        for (int kk = 0; kk < nk; ++kk) {
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");          // step kk landed everywhere; this wave is done reading step kk-1
            fr.read(stg, 0, af0, bf0);
            fr.mma(af0, bf0, acc);
            fr.read(stg, 1, af0, bf0);
            fr.mma(af0, bf0, acc);
            stg = stg + 1 == S ? 0 : stg + 1;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");              // (pairs with the loaders' closing barrier)
    igemm2_epilogue<BM, BN, NW, WP, false>(p, acc, smem, m0, n0, ti.mtile, ti.M, ti.Wg, ti.Hg, ti.h0, ti.w0, nullptr);
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
template <int BM, int BN, int NW, int WP>
__global__ __launch_bounds__(NW * 64, NW / 2) void igemm2p_kernel(const IgemmArgs p) {
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

    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wc = wave % WN, wp = wave / WN;
    const int ntiles = p.grid_m * p.grid_n;
    // tap tables of every class (global tap index): written once
    {
        int total = p.ntaps;
        if (p.ncls > 1) { total = 0; for (int c = 0; c < p.ncls; ++c) total += p.cls_ntaps[c]; }
        fill_tap_tables(p, t, total, 0, ES, sTapA, sTapB, sTapD);
    }
    __syncthreads();

    const int r = t >> 3;
    const int qs = t & 7;
    const unsigned q16 = (unsigned)((qs ^ ((r >> 1) & 7)) << 4);
    const int spt = p.Kc >> 6;
    u32x4 rsA, rsB;
    ring_rsrc(p, rsA, rsB);
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const unsigned wave_lds = lds0 + (unsigned)wave * (8 * GROWB);

    // the tile of a linear index; wave-uniform by construction: say so (the class tables are indexed dynamically, which lands them in VGPRs)
    auto tile_info = [&](int lin) {
        ConvTile ti = tile_of(p, xcd_remap(lin, ntiles));
        ti.mtile = __builtin_amdgcn_readfirstlane(ti.mtile); ti.ntile = __builtin_amdgcn_readfirstlane(ti.ntile);
        ti.ntaps = __builtin_amdgcn_readfirstlane(ti.ntaps); ti.tap0 = __builtin_amdgcn_readfirstlane(ti.tap0);
        ti.Hg = __builtin_amdgcn_readfirstlane(ti.Hg); ti.Wg = __builtin_amdgcn_readfirstlane(ti.Wg);
        ti.M = __builtin_amdgcn_readfirstlane(ti.M); ti.h0 = __builtin_amdgcn_readfirstlane(ti.h0);
        ti.w0 = __builtin_amdgcn_readfirstlane(ti.w0);
        return ti;
    };
    // per-thread DMA descriptors of a tile (the tap tables hold every class: the tile's slice starts at tap0)
    auto describe = [&](const ConvTile& ti, unsigned (&rowoff)[AR], unsigned (&vmask)[AR], unsigned (&browoff)[BR]) {
        row_descriptors(p, ti, ti.mtile * BM, ti.ntile * BN, r, RPP, q16, sTapD + ti.tap0, rowoff, vmask, browoff);
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

    const RingFrag<BM, BN, NW, WP> fr(smem, lane, wc, wp);
    uint4 af0[CT], bf0[PT], af1[CT], bf1[PT];

    // (the launcher guarantees n_k >= 2 for every tile: the cursor then never runs further ahead than the tile whose descriptors
    //  were prepared at the start of the tile the MFMAs are in)
    int lin = blockIdx.x;
    if (lin >= ntiles) return;
    ConvTile cur = tile_info(lin);
    describe(cur, c_rowoff, c_vmask, c_browoff);
    ic_valid = true; ic_ntaps = cur.ntaps; ic_tap0 = cur.tap0;
    int par = 0;
    issue(par);                            // step 0 of the first tile
    for (; lin < ntiles; lin += gridDim.x) {
        const int nk = cur.ntaps * spt;
        // descriptors of the tile after this one, before the cursor can reach it (it is at step 1 of this tile now)
        const int lin_n = lin + gridDim.x;
        ConvTile nxt = cur;
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
        wait_vm_barrier<0>();              // step 0 landed everywhere; everyone is past the previous tile's epilogue
        issue(par ^ 1);                    // step 1
        fr.read(par, 0, af0, bf0);
        for (int kk = 0; kk < nk; ++kk) {
            const int stg = (par + kk) & 1;
            fr.read(stg, 1, af1, bf1);
            fr.mma(af0, bf0, acc);
            if (kk + 1 < nk) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave holds all of step kk in registers
                wait_vm_barrier<0>();                                   // step kk+1 landed everywhere
                issue(stg);                                             // step kk+2 (possibly the next tile's step 0) -> the stage step kk occupied
                fr.read(stg ^ 1, 0, af0, bf0);
            }
            fr.mma(af1, bf1, acc);
        }
        const int sl = (par + nk - 1) & 1;     // the stage of the last K-step: free now, the epilogue's scratch
        par = sl ^ 1;                          // the next tile's step 0 is landing in the other one
        // every wave has its last fragments in registers before the scratch stage is overwritten (no vmcnt wait: the next tile's DMAs
        // stay in flight through the epilogue)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        igemm2_epilogue<BM, BN, NW, WP>(p, acc, smem + sl * STAGE, cur.mtile * BM, cur.ntile * BN, cur.mtile, cur.M, cur.Wg, cur.Hg, cur.h0, cur.w0);
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
    ring_rsrc(p, rsA, rsB);
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
    ring_rsrc(p, rsA, rsB);
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
    const u32x4 rsA = buf_rsrc(p.A, p.bytesA), rsC = buf_rsrc(p.C, p.bytesC);
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
    ring_rsrc(p, rsA, rsB);
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
        const u32x4 rsC = buf_rsrc(p.C, p.bytesC);
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
// ---- launch geometry shared by the tiled kernels
// Tile counts of a launch with BM x BN tiles: grid_n, grid_m and, with several output-parity classes, the first pixel tile of each class
static void tile_grid(IgemmArgs& a, int BM, int BN) {
    a.grid_n = (a.Cst + BN - 1) / BN;
    a.grid_m = (a.M + BM - 1) / BM;
    if (a.ncls > 1) {
        int acc = 0;
        for (int c = 0; c < a.ncls; ++c) { a.cls_tile0[c] = acc; acc += (a.cls_M[c] + BM - 1) / BM; }
        a.cls_tile0[a.ncls] = acc;
        a.grid_m = acc;
    }
}
// The LDS-DMA kernels mark weight rows beyond Cout and K-steps beyond the end with a 0xF0000000 offset that must stay out of range
// (>= bytesB) after the 32-bit additions of a row offset, a tap offset and a channel-block offset, each < bytesB
static int check_ring_weights(const IgemmArgs& a) {
    YDL_CHECK(a.bytesB < 0x08000000u, "ring kernel: weight matrix of 128 MiB or more is not supported");
    return 0;
}
// Launch geometry of an LDS-DMA ring or patch kernel: tile counts, the weight-extent check and the tile order.
static int ring_grid(IgemmArgs& a, int BM, int BN) {
    tile_grid(a, BM, BN);
    if (int e = check_ring_weights(a)) return e;
    // tile order (speed only): which operand would be re-fetched from beyond L2?  channel-tile-fastest streams the whole
    // weight matrix once per pixel tile when it does not fit the XCD's L2; pixel-tile-fastest keeps one weight slab in
    // L2 and re-reads the activations once per channel tile
    const double wbytes = (double)a.Cout * a.Ttot * a.Kc * 2.0;
    const double abytes = (double)a.N * a.Hi * a.Wi * a.lda * 2.0;
    a.m_fastest = (wbytes > 2.0e6 && (double)a.grid_m * wbytes > (double)a.grid_n * abytes) ? 1 : 0;
    return 0;
}

template <typename T, int BM, int BN, int NW = 4, int WP = 4>
static int launch_igemm(IgemmArgs a, hipStream_t st, int fam) {
    tile_grid(a, BM, BN);
    dim3 grid(a.grid_m * a.grid_n);
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
    if (int e = ring_grid(a, BM, BN)) return e;
    dim3 grid(a.grid_m * a.grid_n);
    const size_t smem = (size_t)S * (BM + BN) * GROWB + 3 * MAXTAPS * sizeof(int) + (RED ? BN * 16 : 0);
    static const std::string nm = std::string("igemm2_kernel<") + std::to_string(BM) + "," + std::to_string(BN) + "," +
                                  std::to_string(NW) + "," + std::to_string(WP) + "," + std::to_string(S) + (RED ? ",bnred>" : (STG ? ",stg>" : ">"));
    if constexpr (S == 2 && STG == 0 && BN == 128 && !RED) {
        // persistent form (igemm2p_kernel): worth it when a CTA gets more than one tile; needs n_k >= 2 in every class
        const int spt = a.Kc >> 6;
        int min_taps = a.ntaps;
        if (a.ncls > 1) { min_taps = 1 << 30; for (int c = 0; c < a.ncls; ++c) min_taps = min(min_taps, a.cls_ntaps[c]); }
        static int per_cu = -1;                  // resident CTAs per CU of this instantiation (registers and LDS)
        YDL_SET_MAX_LDS((igemm2p_kernel<BM, BN, NW, WP>), smem);
        if (per_cu < 0) {
            int nb = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, igemm2p_kernel<BM, BN, NW, WP>, NW * 64, smem) != hipSuccess) nb = 0;
            per_cu = nb;
        }
        int G = ydl_device_cus() * per_cu;
        G -= G % 8;
        const int ntiles = a.grid_m * a.grid_n;
        // measured (tools/conv_bench.py --persist 0/1, config-2 layers): +5..10 % with 128-wide tiles once a CTA walks >= 2.5 tiles,
        // neutral to -12 % below that (a second resident CTA overlaps better than a short walk) and with 64-wide tiles
        // (not with the fused reduce: its epilogue on top of the walk's two descriptor sets spills 41 VGPRs)
        if (g_ring_persist && min_taps * spt >= 2 && G >= 8 && 2 * ntiles >= 5 * G) {
            static const std::string nmp = nm + ":persistent";
            ydl_note_kernel(fam, nmp.c_str());
            igemm2p_kernel<BM, BN, NW, WP><<<G, NW * 64, smem, st>>>(a);
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

template <int BM, int BN, int NW, int WP, int S, int NL>
static int launch_igemm2l(IgemmArgs a, hipStream_t st, int fam) {
    if (int e = ring_grid(a, BM, BN)) return e;
    const size_t smem = (size_t)S * (BM + BN) * GROWB + 3 * MAXTAPS * sizeof(int);
    static const std::string nm = std::string("igemm2l_kernel<") + std::to_string(BM) + "," + std::to_string(BN) + "," + std::to_string(NW) + "+" +
                                  std::to_string(NL) + "," + std::to_string(S) + ">";
    YDL_SET_MAX_LDS((igemm2l_kernel<BM, BN, NW, WP, S, NL>), smem);
    ydl_note_kernel(fam, nm.c_str());
    igemm2l_kernel<BM, BN, NW, WP, S, NL><<<dim3(a.grid_m * a.grid_n), (NW + NL) * 64, smem, st>>>(a);
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
    if (int e = ring_grid(a, 128, BN)) return e;              // one class, every tile full (halo_ok): grid_m = M / 128
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
    if (int e = check_ring_weights(a)) return e;
    a.grid_n = (a.Cst + 63) / 64;
    a.grid_m = a.N * (a.Hi >> 3) * (a.Wi >> 4);      // 8 x 16 blocks of the dy grid
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
void ydl_wgrad_debug_set(int key, int val);   // wgrad.hip
extern "C" void ydl_debug_set(int key, int val) {
    ydl_dcn_debug_set(key, val);
    ydl_deform_debug_set(key, val);
    ydl_wgrad_debug_set(key, val);
    if (key == 1) g_pw_enabled = val;
    if (key == 2) g_dgrad_merge = val;
    if (key == 3) g_ring_enabled = val;
    if (key == 5) g_stem_enabled = val;
    if (key == 6) g_ring_persist = val;
    if (key == 8) g_halo = val;
    if (key == 9) g_s2fused = val;
    if (key == 10) g_resize_int = val;
    if (key == 11) g_resize_rows = val;
    if (key == 14) g_pw_acc_ts = val;
    if (key == 17) g_wreg = val;
    if (key == 19) g_ring_loaders = val;
}
