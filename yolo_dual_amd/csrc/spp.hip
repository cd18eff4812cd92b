// The PARALLEL pooling pyramid of SPP / C3SPP / SPPCSPC (models/common.py:1282-1286, :1439-1446): y_i = max-pool(x; k_i, stride 1,
// pad k_i / 2, -inf padding) for three window sizes, all three of the SAME x, in ONE launch per direction.  The forward values equal
// SPPF's chain (ydl_sppf_pool_fwd), the gradients do not wherever values tie: ATen routes a window's gradient to the first maximum
// in scan order of that k x k window of x, the chain routes it through two intermediate arg-max planes, and in bf16 storage ties are
// the normal case.  So this is a kernel pair of its own with the contract ydl_sppf_pool_* has for the chain: values, arg-max codes
// (window offset ky * k + kx of the first maximum in scan order, update rule `v > best || isnan(v)`) and the backward's summation
// order and per-stage rounding are those of three ydl_maxpool_fwd / ydl_maxpool_bwd calls (spatial.hip), bit for bit.
//
// A CTA owns the H x W plane of one image for one 16-byte channel chunk and keeps it in LDS; lanes walk consecutive pixels, so every
// LDS access is a run of consecutive 16-byte words (ds_read_b128 / ds_write_b128 without bank conflicts) next to a run of consecutive
// code words.  Both directions use HW * (32 + V) bytes (V = elements per chunk): 40 KB for a 32 x 32 bf16 plane.
#include "common.h"

namespace {
// V arg-max codes (one byte each) of an item as one LDS word / double word
template <int V> struct PyrCodes;
template <> struct PyrCodes<8> {
    typedef uint2 W;
    __device__ static __forceinline__ W pack(const int* c) {
        return make_uint2((unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16) | ((unsigned)c[3] << 24),
                          (unsigned)c[4] | ((unsigned)c[5] << 8) | ((unsigned)c[6] << 16) | ((unsigned)c[7] << 24));
    }
    __device__ static __forceinline__ int get(const W& w, int e) { return (int)(((e < 4 ? w.x : w.y) >> ((e & 3) * 8)) & 0xffu); }
};
template <> struct PyrCodes<4> {
    typedef unsigned W;
    __device__ static __forceinline__ W pack(const int* c) {
        return (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16) | ((unsigned)c[3] << 24);
    }
    __device__ static __forceinline__ int get(const W& w, int e) { return (int)((w >> (e * 8)) & 0xffu); }
};
}  // namespace

// Forward: each pool is SEPARABLE, as sppf_pool_fwd_kernel argues — a row pass keeps (row maximum, kx of its first occurrence), a
// column pass takes the first row whose maximum beats the running one.  With ATen's update rule applied along both passes the result
// is still the first maximum in (ky, kx) scan order (a NaN wins and the last one stays, in either formulation; the first in-range
// tap initialises): 2 * (k1 + k2 + k3) window taps per element instead of k1^2 + k2^2 + k3^2.
template <typename T>
__global__ __launch_bounds__(256) void spp_pool_fwd_kernel(const T* __restrict__ x, int ldx, T* __restrict__ y1, T* __restrict__ y2,
                                                           T* __restrict__ y3, int ldy, uint8_t* __restrict__ i1, uint8_t* __restrict__ i2,
                                                           uint8_t* __restrict__ i3, int H, int W, int Cp, int k1, int k2, int k3) {
    constexpr int V = ET<T>::V;
    typedef PyrCodes<V> CW;
    extern __shared__ __attribute__((aligned(16))) unsigned char spp_lds[];
    const int HW = H * W;
    uint4* cur = (uint4*)spp_lds;                                  // [HW] the plane of x
    uint4* rmax = cur + HW;                                         // [HW] row maxima of the current pool
    typename CW::W* rkx = (typename CW::W*)(rmax + HW);             // [HW] kx of the row maxima, one byte per channel
    const int n = blockIdx.y;
    const int c0 = blockIdx.x * V;                                  // (grid.x = Cp / V: every chunk is a real one)
    const size_t img = (size_t)n * HW;
    for (int pix = threadIdx.x; pix < HW; pix += 256) cur[pix] = *(const uint4*)(x + (img + pix) * ldx + c0);
    __syncthreads();
    T* const ys[3] = {y1, y2, y3};
    uint8_t* const is[3] = {i1, i2, i3};
    const int ks[3] = {k1, k2, k3};
#pragma unroll
    for (int st = 0; st < 3; ++st) {
        const int k = ks[st], p = k / 2;
        for (int pix = threadIdx.x; pix < HW; pix += 256) {             // row pass
            const int wo = pix % W, row = pix - wo;
            const int lo = wo - p < 0 ? 0 : wo - p, hi = wo + p > W - 1 ? W - 1 : wo + p;
            float best[V];
            int bk[V];
            unpack16<T>(cur[row + lo], best);                           // the first in-range tap initialises
#pragma unroll
            for (int e = 0; e < V; ++e) bk[e] = lo - (wo - p);
            for (int iw = lo + 1; iw <= hi; ++iw) {
                float v[V];
                unpack16<T>(cur[row + iw], v);
                const int kx = iw - (wo - p);
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (v[e] > best[e] || v[e] != v[e]) { best[e] = v[e]; bk[e] = kx; }
            }
            rmax[pix] = pack16<T>(best);
            rkx[pix] = CW::pack(bk);
        }
        __syncthreads();
        for (int pix = threadIdx.x; pix < HW; pix += 256) {             // column pass
            const int wo = pix % W, ho = pix / W;
            const int lo = ho - p < 0 ? 0 : ho - p, hi = ho + p > H - 1 ? H - 1 : ho + p;
            float best[V];
            int bi[V];
            unpack16<T>(rmax[lo * W + wo], best);
            {
                const typename CW::W rk = rkx[lo * W + wo];
                const int ky = lo - (ho - p);
#pragma unroll
                for (int e = 0; e < V; ++e) bi[e] = ky * k + CW::get(rk, e);
            }
            for (int ih = lo + 1; ih <= hi; ++ih) {
                float v[V];
                unpack16<T>(rmax[ih * W + wo], v);
                const typename CW::W rk = rkx[ih * W + wo];
                const int ky = ih - (ho - p);
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (v[e] > best[e] || v[e] != v[e]) { best[e] = v[e]; bi[e] = ky * k + CW::get(rk, e); }
            }
            *(uint4*)(ys[st] + (img + pix) * ldy + c0) = pack16<T>(best);
            if (is[st]) *(typename CW::W*)(is[st] + (img + pix) * Cp + c0) = CW::pack(bi);
        }
        if (st < 2) __syncthreads();                                    // the next row pass overwrites rmax / rkx
    }
}

// Backward: dx = [dx +] mp1'(dy1), then += mp2'(dy2), then += mp3'(dy3), every stage the gather of maxpool_bwd_kernel: an input
// element visits, ky then kx ascending, the output positions whose window holds it and adds dy where the code names it; the running
// value is rounded to the storage type after each stage, as three launches that accumulate into dx would leave it.  A stage's dy
// and code planes are read from LDS; the running value of an element stays with the thread that owns it.  No atomics, no workspace.
template <typename T>
__global__ __launch_bounds__(256) void spp_pool_bwd_kernel(const T* __restrict__ dy1, const T* __restrict__ dy2, const T* __restrict__ dy3,
                                                           int lddy, const uint8_t* __restrict__ i1, const uint8_t* __restrict__ i2,
                                                           const uint8_t* __restrict__ i3, T* __restrict__ dx, int lddx, int accumulate,
                                                           int H, int W, int Cp, int k1, int k2, int k3) {
    constexpr int V = ET<T>::V;
    typedef PyrCodes<V> CW;
    extern __shared__ __attribute__((aligned(16))) unsigned char spp_lds[];
    const int HW = H * W;
    uint4* dyp = (uint4*)spp_lds;                                  // [HW] the stage's output gradient
    uint4* acc = dyp + HW;                                          // [HW] running dx, touched by the owning thread only
    typename CW::W* icode = (typename CW::W*)(acc + HW);            // [HW] the stage's arg-max codes
    const int n = blockIdx.y;
    const int c0 = blockIdx.x * V;
    const size_t img = (size_t)n * HW;
    const T* const dys[3] = {dy1, dy2, dy3};
    const uint8_t* const is[3] = {i1, i2, i3};
    const int ks[3] = {k1, k2, k3};
#pragma unroll
    for (int st = 0; st < 3; ++st) {
        const int k = ks[st], p = k / 2;
        for (int pix = threadIdx.x; pix < HW; pix += 256) {
            dyp[pix] = *(const uint4*)(dys[st] + (img + pix) * lddy + c0);
            icode[pix] = *(const typename CW::W*)(is[st] + (img + pix) * Cp + c0);
        }
        __syncthreads();
        for (int pix = threadIdx.x; pix < HW; pix += 256) {
            const int iw = pix % W, ih = pix / W;
            float g[V];
#pragma unroll
            for (int e = 0; e < V; ++e) g[e] = 0.f;
            if (st > 0) unpack16<T>(acc[pix], g);
            else if (accumulate) unpack16<T>(*(const uint4*)(dx + (img + pix) * lddx + c0), g);
            // ho = ih + p - ky in [0, H): ky from max(0, ih + p - H + 1) to min(k - 1, ih + p); likewise kx
            const int ky0 = ih + p - H + 1 > 0 ? ih + p - H + 1 : 0, ky1 = ih + p < k - 1 ? ih + p : k - 1;
            const int kx0 = iw + p - W + 1 > 0 ? iw + p - W + 1 : 0, kx1 = iw + p < k - 1 ? iw + p : k - 1;
            for (int ky = ky0; ky <= ky1; ++ky) {
                const int orow = (ih + p - ky) * W + iw + p;
                for (int kx = kx0; kx <= kx1; ++kx) {
                    float d[V];
                    unpack16<T>(dyp[orow - kx], d);
                    const typename CW::W cw = icode[orow - kx];
                    const int code = ky * k + kx;
#pragma unroll
                    for (int e = 0; e < V; ++e) g[e] += (CW::get(cw, e) == code) ? d[e] : 0.f;
                }
            }
            const uint4 o = pack16<T>(g);
            if (st < 2) acc[pix] = o;
            else *(uint4*)(dx + (img + pix) * lddx + c0) = o;
        }
        if (st < 2) __syncthreads();                                    // the next stage overwrites dyp / icode
    }
}

static inline size_t spp_smem(int dtype, int H, int W) {
    const int V = dtype == YDL_F32 ? 4 : 8;
    return (size_t)H * (size_t)W * (2 * 16 + V);       // forward: x, row maxima, their kx; backward: dy, running dx, codes
}
static inline bool spp_k_ok(int k) { return k >= 3 && k <= 15 && k % 2 == 1; }      // k * k <= 255: the code range of a byte
extern "C" int ydl_spp_pool_supported(int dtype, int H, int W, int C, int k1, int k2, int k3) {
    if (dtype != YDL_F32 && dtype != YDL_BF16) return 0;
    if (!spp_k_ok(k1) || !spp_k_ok(k2) || !spp_k_ok(k3) || H < 1 || W < 1 || C < 1) return 0;
    return spp_smem(dtype, H, W) <= 64 * 1024 ? 1 : 0;
}
extern "C" int ydl_spp_pool_fwd(int dtype, const void* x, int ldx, void* y1, void* y2, void* y3, int ldy,
                                uint8_t* idx1, uint8_t* idx2, uint8_t* idx3, int N, int H, int W, int C, int k1, int k2, int k3, void* stream) {
    const int V = dtype == YDL_F32 ? 4 : 8;
    const int Cp = round_up(C, V);
    YDL_CHECK(ydl_spp_pool_supported(dtype, H, W, C, k1, k2, k3), "window sizes must be odd, 3..15, and the plane must fit the LDS-resident form (query ydl_spp_pool_supported)");
    YDL_CHECK(x && y1 && y2 && y3 && ldx >= Cp && ldy >= Cp && N >= 1 && N <= 65535, "bad arguments");
    YDL_CHECK((idx1 == nullptr) == (idx2 == nullptr) && (idx2 == nullptr) == (idx3 == nullptr), "the three index planes come together");
    YDL_CHECK(aligned16(x) && aligned16(y1) && aligned16(y2) && aligned16(y3) && ldx % V == 0 && ldy % V == 0, "16-byte alignment");
    YDL_CHECK(((uintptr_t)idx1 | (uintptr_t)idx2 | (uintptr_t)idx3) % 8 == 0, "index planes must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(Cp / V, N);
    const size_t smem = spp_smem(dtype, H, W);
    if (dtype == YDL_F32) spp_pool_fwd_kernel<float><<<grid, 256, smem, st>>>((const float*)x, ldx, (float*)y1, (float*)y2, (float*)y3, ldy, idx1, idx2, idx3, H, W, Cp, k1, k2, k3);
    else spp_pool_fwd_kernel<bf16_t><<<grid, 256, smem, st>>>((const bf16_t*)x, ldx, (bf16_t*)y1, (bf16_t*)y2, (bf16_t*)y3, ldy, idx1, idx2, idx3, H, W, Cp, k1, k2, k3);
    YDL_LAUNCH_CHECK();
    return 0;
}
extern "C" int ydl_spp_pool_bwd(int dtype, const void* dy1, const void* dy2, const void* dy3, int lddy, const uint8_t* idx1,
                                const uint8_t* idx2, const uint8_t* idx3, void* dx, int lddx, int accumulate,
                                int N, int H, int W, int C, int k1, int k2, int k3, void* stream) {
    const int V = dtype == YDL_F32 ? 4 : 8;
    const int Cp = round_up(C, V);
    YDL_CHECK(ydl_spp_pool_supported(dtype, H, W, C, k1, k2, k3), "window sizes must be odd, 3..15, and the plane must fit the LDS-resident form (query ydl_spp_pool_supported)");
    YDL_CHECK(dy1 && dy2 && dy3 && idx1 && idx2 && idx3 && dx && lddy >= Cp && lddx >= Cp && N >= 1 && N <= 65535, "bad arguments");
    YDL_CHECK(aligned16(dy1) && aligned16(dy2) && aligned16(dy3) && aligned16(dx) && lddy % V == 0 && lddx % V == 0, "16-byte alignment");
    YDL_CHECK(((uintptr_t)idx1 | (uintptr_t)idx2 | (uintptr_t)idx3) % 8 == 0, "index planes must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(Cp / V, N);
    const size_t smem = spp_smem(dtype, H, W);
    if (dtype == YDL_F32) spp_pool_bwd_kernel<float><<<grid, 256, smem, st>>>((const float*)dy1, (const float*)dy2, (const float*)dy3, lddy, idx1, idx2, idx3, (float*)dx, lddx, accumulate, H, W, Cp, k1, k2, k3);
    else spp_pool_bwd_kernel<bf16_t><<<grid, 256, smem, st>>>((const bf16_t*)dy1, (const bf16_t*)dy2, (const bf16_t*)dy3, lddy, idx1, idx2, idx3, (bf16_t*)dx, lddx, accumulate, H, W, Cp, k1, k2, k3);
    YDL_LAUNCH_CHECK();
    return 0;
}
