// Weight gradients of the implicit-GEMM convolution on MFMA for gfx950, and the one-pass kernels that read (x, dy) together:
// wgrad_kernel, wgrad2 / wgrad3 / wgrad3s, pwbw_kernel (1x1 input + weight gradient), stemw_kernel.  Layout and number formats as in igemm.hip.
#include "conv_common.h"

#define ROWB 144      // LDS row stride in bytes (128 data + 16 pad): wgrad tiles (transposed reads)

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
    const u32x4 rsX = buf_rsrc(p.X, p.bytesX), rsY = buf_rsrc(p.dY, p.bytesY);
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
        const u32x4 rsX = buf_rsrc(p.X, p.bytesX), rsY = buf_rsrc(p.dY, p.bytesY);
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
    const u32x4 rsX = buf_rsrc(p.X, p.bytesX), rsY = buf_rsrc(p.dY, p.bytesY), rsD = buf_rsrc(p.dX, p.bytesDX), rsW = buf_rsrc(p.Wt, p.bytesWt);
    [[maybe_unused]] u32x4 rsO, rsYo;
    if constexpr (BN != 0) {
        rsO = buf_rsrc(pa.dO, pa.bytesDO);
        rsYo = buf_rsrc(pa.dYo, pa.bytesDYo);      // (no dy_out: zero bytes, every store dropped)
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
    const u32x4 rsX = buf_rsrc(p.X, p.bytesX), rsY = buf_rsrc(p.dY, p.bytesY);
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

// debug knobs of this file (ydl_debug_set of igemm.hip forwards every key; its comment lists them all)
void ydl_wgrad_debug_set(int key, int val) {
    if (key == 0) g_wgrad_tr = val;
    if (key == 4) g_wgrad_dma = val;
    if (key == 12) g_stemw = val;
    if (key == 15) g_pwbw = val;
    if (key == 18) g_wg3_loaders = val;
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
