// q6_k_device.h — device helpers shared by the Q6_K kernels (q6_k.hip, q6_k_gemm.hip); the alignment rule
// they serve is stated at the top of q6_k.hip.
#pragma once
#include "q4_0_device.h"

namespace ghip {

__device__ __forceinline__ uint32_t ld_u32_a2(const uint8_t *p) {
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3);
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p - mis);   // (pointer arithmetic: stays a global address)
    const uint32_t lo = q[0], hi = q[1];
    return __builtin_amdgcn_alignbyte(hi, lo, mis);
}

// four 6-bit values (one per byte, 0..63) -> q - 32 as int8 (the set top bit keeps the bytes from borrowing)
__device__ __forceinline__ uint32_t q6_recentre(uint32_t q) { return ((q | 0x80808080u) - 0x20202020u) ^ 0x80808080u; }

// One q8_K block over the 64 lanes of a wave, lane l holding elements 4l .. 4l + 3: returns the lane's four
// int8 (packed) and the block's d in every lane.  max is the FIRST element of largest |x| (strict >, in element
// order), and its sign is iscale's: the 64-bit key |x| bits : 255 - index : sign bit orders exactly that way
// under an unsigned max.  nearest_int is the reference's 12582912.f add (round half to even); the element of
// equal magnitude and opposite sign gives +128, clamped to 127.  amax == 0: d = 0, qs = 0.
__device__ __forceinline__ uint32_t q8k_block_lane(float4 v, int lane, float &d) {
    const float xs[4] = {v.x, v.y, v.z, v.w};
    unsigned long long key = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t bits = __float_as_uint(xs[k]);
        const unsigned long long kk = ((unsigned long long)(bits & 0x7FFFFFFFu) << 32) |
                                      ((unsigned long long)(255 - (4 * lane + k)) << 1) | (bits >> 31);
        key = kk > key ? kk : key;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off, 64);
        key = o > key ? o : key;
    }
    const uint32_t abits = (uint32_t)(key >> 32);
    if (abits == 0) {
        d = 0.0f;
        return 0;
    }
    const float mx = __uint_as_float(abits | ((uint32_t)(key & 1) << 31));
    const float iscale = __fdiv_rn(-128.f, mx);
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const float val = __fadd_rn(__fmul_rn(iscale, xs[k]), 12582912.f);
        int q = (int)(__float_as_uint(val) & 0x007FFFFFu) - 0x00400000;
        q = q > 127 ? 127 : q;
        packed |= (uint32_t)(q & 0xFF) << (8 * k);
    }
    d = __fdiv_rn(1.0f, iscale);
    return packed;
}


}  // namespace ghip
