// q5x_device.h — device helpers shared by the Q4_1 / Q5_0 / Q5_1 kernels (q5x_w.hip, q5x_gemm.hip): the block
// geometry, the 4-byte aligned load of a block pair and its decode into the unsigned values; the layouts and the
// alignment rule they serve are stated at the top of q5x_w.hip.
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

typedef u32x4 g5x_u32x4_a4 __attribute__((aligned(4)));
typedef uint32_t g5x_u32x2_t __attribute__((ext_vector_type(2)));
typedef g5x_u32x2_t g5x_u32x2_a4 __attribute__((aligned(4)));
typedef __attribute__((address_space(1))) const g5x_u32x4_a4 g5x_gx4;
typedef __attribute__((address_space(1))) const g5x_u32x2_a4 g5x_gx2;
typedef __attribute__((address_space(1))) const uint32_t g5x_gx1;

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
    } else {
        const g5x_u32x2_t c = *(g5x_gx2 *)(p + 32);
        v.w[8] = c.x; v.w[9] = c.y;
        if constexpr (DW == 11) v.w[10] = *(g5x_gx1 *)(p + 40);
    }
    return v;
}

// one block: the 32 values 0..15 / 0..31 as eight dwords in element order, fp16 d and m as f32
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

}  // namespace ghip
