// The f16 hi / lo split under every "f16x3" kernel (kernel_mfma3.h, kernel_mfma3w.h, kernel_tenc.h):
//     x = hi + lo,  hi = f16(x),  lo = f16(x - hi)         (x - hi is exact in fp32)
// carries 22 significant bits of x, and a product of two split operands is three
// v_mfma_f32_16x16x32_f16 with fp32 accumulation (lo.hi + hi.lo + hi.hi; the dropped lo.lo term is
// ~2^-22 relative).  Two forms of the same arithmetic: one value with plain casts, and a pair with
// packed converts.  Both give the same bits; a call site keeps the form it was tuned with.
#pragma once
#include <cstdint>

namespace b2h {

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <typename V> // f16x4 or f16x8: x -> element j of hi and of lo
__device__ __forceinline__ void split1(float x, V& hi, V& lo, int j) {
    const _Float16 a = (_Float16)x;
    hi[j] = a;
    lo[j] = (_Float16)(x - (float)a);
}

// hi = f16(x) packed two per instruction (v_cvt_pk_f16_f32), residual x - hi as ONE mixed-precision
// FMA per value (v_fma_mix_f32 reads the f16 half straight out of the packed register; written as
// asm because hipcc otherwise converts hi back with v_cvt_f32_f16 and subtracts), lo = f16(residual)
// packed: 4 VALU per pair, half of what two split1 cost.
__device__ __forceinline__ void split2(float x0, float x1, f16x2& hi, f16x2& lo) {
    hi = f16x2{(_Float16)x0, (_Float16)x1};
    const uint32_t hb = __builtin_bit_cast(uint32_t, hi);
    float r0, r1;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(hb), "v"(x0));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(hb), "v"(x1));
    lo = f16x2{(_Float16)r0, (_Float16)r1};
}

__device__ __forceinline__ void split8(const float (&v)[8], f16x8& hi, f16x8& lo) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f16x2 h, l;
        split2(v[2 * i], v[2 * i + 1], h, l);
        hi[2 * i] = h[0]; hi[2 * i + 1] = h[1];
        lo[2 * i] = l[0]; lo[2 * i + 1] = l[1];
    }
}

} // namespace b2h
