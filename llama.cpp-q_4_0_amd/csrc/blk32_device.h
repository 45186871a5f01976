// blk32_device.h — device helpers shared by the kernels of the 32-weight block types (blk32_w.hip: Q8_0, Q4_1, Q5_0,
// Q5_1 and the k_gemm8 image writer, q4_0 included; q5x_gemm.hip: Q4_1 / Q5_1): the block geometry, the 4-byte aligned
// load of a block pair and its decode into two blocks of eight dwords; the layouts and the alignment rule they serve
// are stated at the top of blk32_w.hip.
#pragma once
#include "q4_0_device.h"

namespace ghip {

template <bool QH, bool MIN>
struct Q5x {
    static constexpr int BLK = 18 + 2 * MIN + 4 * QH;     // 20 / 22 / 24
    static constexpr int PAIR = 2 * BLK;                  // 40 / 44 / 48
    static constexpr int DW = PAIR / 4;
    static constexpr int OFF_QH = 2 + 2 * MIN, OFF_QS = OFF_QH + 4 * QH;
};

// the four bits b of a nibble -> bit 4 of byte k for bit k (b * 0x204081 puts bit k at 8 k among others: the
// sixteen partial positions are distinct, so nothing carries)
__device__ __forceinline__ uint32_t q5x_spread4(uint32_t qh, int shift) {
    return ((((qh >> shift) & 0xFu) * 0x00204081u) & 0x01010101u) << 4;
}

// four bytes at a 2-byte aligned address from the aligned dwords that hold them (one dword when p is aligned)
__device__ __forceinline__ uint32_t blk32_ld32(const uint8_t *p) {
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3);
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p - mis);   // (pointer arithmetic: stays a global address)
    return __builtin_amdgcn_alignbyte(q[mis >> 1], q[0], mis);
}

typedef u32x4 g5x_u32x4_a4 __attribute__((aligned(4)));
typedef uint32_t g5x_u32x2_t __attribute__((ext_vector_type(2)));
typedef g5x_u32x2_t g5x_u32x2_a4 __attribute__((aligned(4)));
typedef __attribute__((address_space(1))) const g5x_u32x4_a4 g5x_gx4;
typedef __attribute__((address_space(1))) const g5x_u32x2_a4 g5x_gx2;
typedef __attribute__((address_space(1))) const uint32_t g5x_gx1;

// a pair of 9 (q4_0), 10 (Q4_1), 11 (Q5_0) or 12 (Q5_1) dwords
template <int DW>
struct PairX {
    uint32_t w[DW];
};

template <int DW>
__device__ __forceinline__ PairX<DW> load_pairx(const uint8_t *p) {
    PairX<DW> v;
    const u32x4 a = *(g5x_gx4 *)(p), b = *(g5x_gx4 *)(p + 16);
    v.w[0] = a.x; v.w[1] = a.y; v.w[2] = a.z; v.w[3] = a.w;
    v.w[4] = b.x; v.w[5] = b.y; v.w[6] = b.z; v.w[7] = b.w;
    if constexpr (DW == 12) {
        const u32x4 c = *(g5x_gx4 *)(p + 32);
        v.w[8] = c.x; v.w[9] = c.y; v.w[10] = c.z; v.w[11] = c.w;
    } else if constexpr (DW == 9) {
        v.w[8] = *(g5x_gx1 *)(p + 32);
    } else {
        const g5x_u32x2_t c = *(g5x_gx2 *)(p + 32);
        v.w[8] = c.x; v.w[9] = c.y;
        if constexpr (DW == 11) v.w[10] = *(g5x_gx1 *)(p + 40);
    }
    return v;
}

// a Q8_0 pair: 17 dwords, kept as the vectors they are loaded as
struct Pair8 {
    u32x4 a, b, c, d;
    uint32_t e;
};

// The vector loads are written from the top of the pair down: the compiler issues them in that order in the GEMV
// (48, 32, 16, 0), which lets the first wait of an item cover the loads after it.  Written bottom up they come out as
// 16, 0, 64, 32, 48 and every instantiation takes one or two more s_waitcnt (profiles/blk32_isa.json is the check).
__device__ __forceinline__ Pair8 load_pair8(const uint8_t *p68) {
    Pair8 v;
    v.d = *(g5x_gx4 *)(p68 + 48);
    v.c = *(g5x_gx4 *)(p68 + 32);
    v.b = *(g5x_gx4 *)(p68 + 16);
    v.a = *(g5x_gx4 *)(p68);
    v.e = *(g5x_gx1 *)(p68 + 64);
    return v;
}

// one block: its 32 values as eight dwords in element order (Q4_1 / Q5_0 / Q5_1: the unsigned 0..15 / 0..31; Q8_0:
// the int8 weights), fp16 d and m as f32
struct BlockX {
    uint32_t q[8];
    float d, m;
};

template <bool QH>
__device__ __forceinline__ void q5x_expand(BlockX &o, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t qh) {
    const uint32_t s[4] = {s0, s1, s2, s3};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        o.q[i] = s[i] & 0x0F0F0F0Fu;
        o.q[4 + i] = (s[i] >> 4) & 0x0F0F0F0Fu;
        if (QH) {
            o.q[i] |= q5x_spread4(qh, 4 * i);
            o.q[4 + i] |= q5x_spread4(qh, 16 + 4 * i);
        }
    }
}

template <bool QH, bool MIN>
__device__ __forceinline__ void q5x_decode_pair(const PairX<Q5x<QH, MIN>::DW> &v, BlockX &A, BlockX &B) {
    const uint32_t *w = v.w;
    if constexpr (!MIN) {                                   // Q5_0: 22-byte blocks
        A.d = h2f(w[0] & 0xFFFFu);
        B.d = h2f(w[5] >> 16);
        A.m = B.m = 0.0f;
        q5x_expand<true>(A, __builtin_amdgcn_alignbyte(w[2], w[1], 2), __builtin_amdgcn_alignbyte(w[3], w[2], 2),
                         __builtin_amdgcn_alignbyte(w[4], w[3], 2), __builtin_amdgcn_alignbyte(w[5], w[4], 2),
                         __builtin_amdgcn_alignbyte(w[1], w[0], 2));
        q5x_expand<true>(B, w[7], w[8], w[9], w[10], w[6]);
    } else if constexpr (QH) {                              // Q5_1: 24-byte blocks
        A.d = h2f(w[0] & 0xFFFFu);
        A.m = h2f(w[0] >> 16);
        B.d = h2f(w[6] & 0xFFFFu);
        B.m = h2f(w[6] >> 16);
        q5x_expand<true>(A, w[2], w[3], w[4], w[5], w[1]);
        q5x_expand<true>(B, w[8], w[9], w[10], w[11], w[7]);
    } else {                                                // Q4_1: 20-byte blocks
        A.d = h2f(w[0] & 0xFFFFu);
        A.m = h2f(w[0] >> 16);
        B.d = h2f(w[5] & 0xFFFFu);
        B.m = h2f(w[5] >> 16);
        q5x_expand<false>(A, w[1], w[2], w[3], w[4], 0u);
        q5x_expand<false>(B, w[6], w[7], w[8], w[9], 0u);
    }
}

// Q8_0: even block d = a.x[15:0], qs = bytes 2..33 (re-aligned); odd block d = c.x[31:16], qs = c.y .. e
__device__ __forceinline__ void q8_0_decode_pair(const Pair8 &v, BlockX &A, BlockX &B) {
    A.d = h2f(v.a.x & 0xFFFFu);
    B.d = h2f(v.c.x >> 16);
    A.m = B.m = 0.0f;
    A.q[0] = __builtin_amdgcn_alignbyte(v.a.y, v.a.x, 2); A.q[1] = __builtin_amdgcn_alignbyte(v.a.z, v.a.y, 2);
    A.q[2] = __builtin_amdgcn_alignbyte(v.a.w, v.a.z, 2); A.q[3] = __builtin_amdgcn_alignbyte(v.b.x, v.a.w, 2);
    A.q[4] = __builtin_amdgcn_alignbyte(v.b.y, v.b.x, 2); A.q[5] = __builtin_amdgcn_alignbyte(v.b.z, v.b.y, 2);
    A.q[6] = __builtin_amdgcn_alignbyte(v.b.w, v.b.z, 2); A.q[7] = __builtin_amdgcn_alignbyte(v.c.x, v.b.w, 2);
    B.q[0] = v.c.y; B.q[1] = v.c.z; B.q[2] = v.c.w; B.q[3] = v.d.x;
    B.q[4] = v.d.y; B.q[5] = v.d.z; B.q[6] = v.d.w; B.q[7] = v.e;
}

}  // namespace ghip
