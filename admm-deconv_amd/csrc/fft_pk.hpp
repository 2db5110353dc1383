// fft_pk.hpp -- packed-FP32 forms of the register butterflies (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32: both
// components of a complex value in one VALU instruction), for the translation units built with ADMM_PK_F32 (the
// fused 256x256 kernels).  Included by fft_reg.hpp; every other translation unit keeps the scalar forms.
//
// Every result is bitwise the scalar form's: the same operations with the same roundings per component.  Signs go
// into constants -- x * -c == -(x * c), fma(a, 1, b) == a + b and fma(a, -1, b) == b - a exactly -- because the
// compiler folds a whole-vector negation and any swizzle into the instruction's modifiers, but not the negation of
// one component (that costs a v_xor and a v_mov).  Values are native 2-vectors end to end, so that they live in
// aligned register pairs; the float2 forms in fft_reg.hpp / line_pair.hpp convert at their boundaries only.
#pragma once
#include <hip/hip_runtime.h>

namespace admm {

typedef float f2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float2 pk(f2v v) { return make_float2(v.x, v.y); }
__device__ __forceinline__ f2v vec(float2 a) { return f2v{a.x, a.y}; }
__device__ __forceinline__ f2v pk_fma(f2v a, f2v b, f2v c) { return __builtin_elementwise_fma(a, b, c); }

// a + (b.y, -b.x) (S = false) or a + (-b.y, b.x) (S = true): a -+ i b
template <bool S>
__device__ __forceinline__ f2v vadd_rot(f2v a, f2v b) {
    return pk_fma(b.yx, S ? f2v{-1.0f, 1.0f} : f2v{1.0f, -1.0f}, a);
}
// a + conj(b) (S = false) or a - conj(b) (S = true)
template <bool S>
__device__ __forceinline__ f2v vadd_conj(f2v a, f2v b) {
    return pk_fma(b, S ? f2v{-1.0f, 1.0f} : f2v{1.0f, -1.0f}, a);
}
// multiply by -i (forward) or +i (inverse), as a value (one multiply; in the butterflies it is vadd_rot's operand)
template <bool INV>
__device__ __forceinline__ f2v vrot(f2v a) {
    return a.yx * (INV ? f2v{-1.0f, 1.0f} : f2v{1.0f, -1.0f});
}

// v * (c + i s) = (fma(v.x, c, -v.y * s), fma(v.x, s, v.y * c)), two ways:
// vmulc_reg: packed, the constants as 2-vectors that the compiler keeps in scalar register pairs (VOP3P takes no
// literal on gfx950).  For the three W16 constants only: given all ~110 W256 twiddles of a line transform the
// compiler hoists them out of the iteration loop and spills the scalar registers into VGPR lanes (a v_readlane per
// use), and moved into scalar registers at each use they cost four s_mov for the two VALU instructions saved --
// with two waves per SIMD a wave's SALU instructions take issue slots like its VALU ones (measured: the line
// round trips 1.00 -> 0.95 ms with 32 % fewer VALU instructions but as many instructions as before).
__device__ __forceinline__ f2v vmulc_reg(f2v v, float c, float s) {
    return pk_fma(v.xx, f2v{c, s}, v.yy * f2v{-s, c});
}
// vmulc_lit: the scalar instructions, whose constants are literals of the instruction (the W256 twiddles)
__device__ __forceinline__ f2v vmulc_lit(f2v v, float c, float s) {
    return f2v{fmaf(v.x, c, -v.y * s), fmaf(v.x, s, v.y * c)};
}

template <bool INV>
__device__ __forceinline__ void vdft4(f2v& v0, f2v& v1, f2v& v2, f2v& v3) {
    const f2v s02 = v0 + v2, d02 = v0 - v2;
    const f2v s13 = v1 + v3, d13 = v1 - v3;
    v0 = s02 + s13;
    v2 = s02 - s13;
    v1 = vadd_rot<INV>(d02, d13);
    v3 = vadd_rot<!INV>(d02, d13);
}

}  // namespace admm
