// Shared by the convolution translation units: igemm.hip (forward and data gradient) and wgrad.hip (everything that reads (x, dy)).
#pragma once
#include "common.h"
#include <type_traits>
#include <stdlib.h>

#define MAXTAPS 64

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

// LDS-DMA (`buffer_load_dwordx4 ... lds`): one wave-instruction writes 1 KiB at (wave-uniform M0 base) + lane*16.  The kernels that
// use it count their own waits (wait_vm_barrier); the comment above igemm2_kernel in igemm.hip has the reason.
// Raw buffer descriptor of [ptr, ptr + bytes): loads beyond the extent return zeros, stores beyond it are dropped.
__device__ __forceinline__ u32x4 buf_rsrc(const void* ptr, unsigned bytes) {
    const unsigned long long a = (unsigned long long)ptr;
    return u32x4{(unsigned)a, (unsigned)(a >> 32) & 0xffffu, bytes, 0x00020000u};
}
__device__ __forceinline__ void lds_dma16(const u32x4& rsrc, unsigned lds_addr, unsigned voff) {
    // M0 = LDS byte address of the wave's 1 KiB destination (wave-uniform); written in the statement that uses it
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(lds_addr), "v"(voff), "s"(rsrc)
                 : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vm_barrier() {
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}

// A 16-byte store issued from inline asm: the hardware reads the four data registers over two cycles AFTER issue, and a vector
// instruction that rewrites one of them in the next cycle wins the race (the compiler's hazard recognizer pads a store it knows with
// a wait state; it cannot see into an asm statement).  Found as an LDS address in every third dword of dx: the `s_nop` is the fix.
__device__ __forceinline__ void buf_store16_asm(const u32x4& v, unsigned off, const u32x4& rsrc) {
    asm volatile("buffer_store_dwordx4 %0, %1, %2, 0 offen\n\ts_nop 1" ::"v"(v), "v"(off), "s"(rsrc) : "memory");
}

inline int check_geom(const ydl_conv_geom* g, int dtype) {
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
