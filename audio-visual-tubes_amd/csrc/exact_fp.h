// Separately rounded arithmetic for kernels whose results a numpy restatement must reproduce bit for bit.
//
// hipcc compiles device code with -ffp-contract=fast-honor-pragmas: a product feeding a sum becomes one FMA, across
// statements and through __fmul_rn / __fadd_rn / __dmul_rn / __dadd_rn too (plain operators in hipcc's headers,
// compiled under that default).  The operators below are compiled with contraction off, so what they return is
// rounded once each and never fused with a neighbour.  The divide is IEEE correctly rounded (no fast-math here).
#pragma once

namespace avt {

template <typename T>
__device__ __forceinline__ T mul_rn(T a, T b) {
#pragma clang fp contract(off)
  return a * b;
}
template <typename T>
__device__ __forceinline__ T add_rn(T a, T b) {
#pragma clang fp contract(off)
  return a + b;
}
template <typename T>
__device__ __forceinline__ T sub_rn(T a, T b) {
#pragma clang fp contract(off)
  return a - b;
}
template <typename T>
__device__ __forceinline__ T div_rn(T a, T b) {
#pragma clang fp contract(off)
  return a / b;
}

}  // namespace avt
