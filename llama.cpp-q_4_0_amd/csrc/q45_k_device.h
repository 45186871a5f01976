// q45_k_device.h — device helpers shared by the Q5_K / Q4_K kernels (q45_k.hip, q45_k_gemm.hip); the block layout
// and the alignment rule they serve are stated at the top of q45_k.hip.
#pragma once
#include "q6_k_device.h"

namespace ghip {

template <bool QH>
struct Q45 {
    static constexpr int BYTES = QH ? Q5KB : Q4KB;
    static constexpr int QS = QH ? 48 : 16;                // byte offset of qs[128]
};

// the 6-bit scales and mins of one superblock from its three scale dwords (k_quants.c:2462-2467): bytes of
// sc_lo | sc_hi are sc[0..3] | sc[4..7], bytes of m_lo | m_hi are m[0..3] | m[4..7]
struct ScaleMin {
    uint32_t sc_lo, sc_hi, m_lo, m_hi;
};
__device__ __forceinline__ ScaleMin unpack_scales_k4(uint32_t s0, uint32_t s1, uint32_t s2) {
    ScaleMin r;
    r.m_hi = ((s2 >> 4) & 0x0F0F0F0Fu) | (((s1 >> 6) & 0x03030303u) << 4);
    r.m_lo = s1 & 0x3F3F3F3Fu;
    r.sc_hi = (s2 & 0x0F0F0F0Fu) | (((s0 >> 6) & 0x03030303u) << 4);
    r.sc_lo = s0 & 0x3F3F3F3Fu;
    return r;
}

}  // namespace ghip
