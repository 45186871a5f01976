// q23_k_device.h — device helpers of the Q3_K / Q2_K kernels (q23_k.hip); the block layouts and the alignment rule
// they serve are stated at the top of q23_k.hip.
#pragma once
#include "q6_k_device.h"

namespace ghip {

template <bool Q3>
struct Q23 {
    static constexpr int BYTES = Q3 ? Q3KB : Q2KB;
    static constexpr int QS = Q3 ? 32 : 16;                // byte offset of qs[64]
    static constexpr int SC = Q3 ? 96 : 0;                 // byte offset of scales[12] / scales[16]
    static constexpr int D = Q3 ? 108 : 80;                // byte offset of fp16 d (Q2_K: dmin behind it)
};

// A block's dword j (bytes 4j .. 4j + 3 of the block) where the block sits at mis = 0 or 2 bytes behind the aligned
// address q: from the aligned dwords q[j] and q[j + mis / 2] (the same dword twice for an aligned block, so nothing
// behind the block's last dword is touched) and one v_alignbyte_b32.
__device__ __forceinline__ uint32_t blk_dword(uint32_t lo, uint32_t hi, uint32_t mis) {
    return __builtin_amdgcn_alignbyte(hi, lo, mis);
}
__device__ __forceinline__ uint32_t ld_blk_dword(const uint32_t *q, uint32_t mis, int j) {
    return blk_dword(q[j], q[j + (int)(mis >> 1)], mis);
}

// The four groups of four values that lane (n, i) of a superblock owns, one per k = 0..3: elements 128n + 32k + 4i ..
// + 3, as signed bytes.  qsd = qs dword 8n + i; Q3_K: hm = hmask dword i, whose bits 4n + k are the groups' high
// bits; a clear high bit means q - 4, which is low2 | 0xFC as a signed byte (no subtraction, no borrow).
template <bool Q3>
__device__ __forceinline__ void q23_values(uint32_t qsd, uint32_t hm, int n, uint32_t v[4]) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t q = (qsd >> (2 * k)) & 0x03030303u;
        if (Q3) q |= ((~hm >> (4 * n + k)) & 0x01010101u) * 0xFCu;
        v[k] = q;
    }
}

// The scales of those four groups, s_k = 8n + 2k + h (h = i >= 4).
// Q3_K: from the three scale dwords a0 a1 a2 (k_quants.c:1854-1860): the low four bits of scale s are nibble s / 8
// of byte s % 8 of (a0, a1), the high two are bits 2 (s / 4) of byte s % 4 of a2; minus 32.
__device__ __forceinline__ void q3_scales(uint32_t a0, uint32_t a1, uint32_t a2, int n, int h, int sc[4]) {
    const int sh = 8 * h + 4 * n;
    const uint32_t w0 = a0 >> sh, w1 = a1 >> sh, x = a2 >> sh;
    sc[0] = (int)((w0 & 0xFu) | ((x & 3u) << 4)) - 32;
    sc[1] = (int)(((w0 >> 16) & 0xFu) | (((x >> 16) & 3u) << 4)) - 32;
    sc[2] = (int)((w1 & 0xFu) | (((x >> 2) & 3u) << 4)) - 32;
    sc[3] = (int)(((w1 >> 16) & 0xFu) | (((x >> 18) & 3u) << 4)) - 32;
}
// Q2_K: s0, s1 = the dwords 2n and 2n + 1 of scales[16]; the scale is the low nibble of byte s_k
__device__ __forceinline__ void q2_scales(uint32_t s0, uint32_t s1, int h, int sc[4]) {
    const uint32_t w0 = s0 >> (8 * h), w1 = s1 >> (8 * h);
    sc[0] = (int)(w0 & 0xFu);
    sc[1] = (int)((w0 >> 16) & 0xFu);
    sc[2] = (int)(w1 & 0xFu);
    sc[3] = (int)((w1 >> 16) & 0xFu);
}

// sum over each row of 16 consecutive lanes (every lane of the row gets the result; int32, exact)
__device__ __forceinline__ int row16_sum(int v) {
    v += dpp_i<DPP_QUAD_XOR1>(v);
    v += dpp_i<DPP_QUAD_XOR2>(v);
    v += dpp_i<DPP_ROW_HALF_MIRROR>(v);
    return v + dpp_i<DPP_ROW_MIRROR>(v);
}

}  // namespace ghip
