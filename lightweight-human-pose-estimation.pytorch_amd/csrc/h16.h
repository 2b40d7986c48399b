// The two 16-bit storage types of the conv stack (LWP_BF16, LWP_F16) as seen by the kernels: one set of kernel templates is
// instantiated for each.  Both are 16-bit MFMA operands with f32 accumulation at the same rate (v_mfma_f32_16x16x32_{bf16,f16},
// v_mfma_f32_32x32x16_{bf16,f16}); they differ only in the split of the 16 bits (bf16 8-bit significand / 8-bit exponent,
// fp16 11 / 5).  The f32 -> 16-bit pack and the 16-bit -> f32 unpack are the C++ conversions `(T)x` / `(float)x`: round to
// nearest even in both directions that round (never the truncating v_cvt_pkrtz), fp16 subnormals kept (no flush).
#pragma once
#include <hip/hip_runtime.h>

namespace lwp {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <typename T> struct H16;

template <> struct H16<__bf16> {
    typedef __bf16 x8 __attribute__((ext_vector_type(8)));
    typedef __bf16 x4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ f32x4 mfma16(const x8& a, const x8& b, const f32x4& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x16 mfma32(const x8& a, const x8& b, const f32x16& c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
};

template <> struct H16<_Float16> {
    typedef _Float16 x8 __attribute__((ext_vector_type(8)));
    typedef _Float16 x4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ f32x4 mfma16(const x8& a, const x8& b, const f32x4& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x16 mfma32(const x8& a, const x8& b, const f32x16& c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
};

}  // namespace lwp
