// What the row kernels of elementwise.hip and the network-end kernels of net_end.hip share: the 16-byte item, the rule for when it applies,
// the grid of a grid-stride loop and the dtype dispatch of a launcher.
#pragma once
#include <initializer_list>
#include <type_traits>
#include "common.h"

namespace miseg {

// workgroups of a grid-stride loop over `total` items, 256 lanes each
static constexpr int EW_GRID_CAP = 8192;
static inline int ew_grid(int64_t total, int cap = EW_GRID_CAP) {
  int64_t b = (total + 255) / 256;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// VEC consecutive elements of T as floats: one 16-byte access when VEC == Vec16<T>::N, one element when VEC == 1
template <class T, int VEC> struct V {
  float v[VEC];
  __device__ __forceinline__ void load(const T* p) {
    if constexpr (VEC == 1) v[0] = to_f32(p[0]);
    else {
      typename Vec16<T>::type t = *reinterpret_cast<const typename Vec16<T>::type*>(p);
#pragma unroll
      for (int i = 0; i < VEC; ++i) v[i] = to_f32(t[i]);
    }
  }
  __device__ __forceinline__ void store(T* p) const {
    if constexpr (VEC == 1) p[0] = from_f32<T>(v[0]);
    else {
      typename Vec16<T>::type t;
#pragma unroll
      for (int i = 0; i < VEC; ++i) t[i] = from_f32<T>(v[i]);
      *reinterpret_cast<typename Vec16<T>::type*>(p) = t;
    }
  }
};

static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Whether rows may be walked in 16-byte items of n = Vec16<T>::N elements: every count a row address is built from (channel counts, leading
// dimensions) is a multiple of n and every operand starts on a 16-byte boundary.  An operand left out is one the kernel reads by element.
static inline bool vec16_ok(int n, std::initializer_list<int64_t> counts, std::initializer_list<const void*> ptrs) {
  bool ok = true;
  for (int64_t c : counts) ok = ok && c % n == 0;
  for (const void* p : ptrs) ok = ok && al16(p);
  return ok;
}

// The one choice between a kernel's <T, Vec16<T>::N> and <T, 1> forms: calls launch(std::integral_constant<int, VEC>, cv) with cv = C / VEC,
// the items of one row.
template <class T, class L> static inline void vec_pick(bool vec, int C, L&& launch) {
  constexpr int N = Vec16<T>::N;
  if (vec) launch(std::integral_constant<int, N>{}, C / N);
  else launch(std::integral_constant<int, 1>{}, C);
}

}  // namespace miseg

// body of an extern "C" launcher with a `dtype` field: runs the statements with T = float or bf16 and returns MISEG_OK
#define DT(p, ...)                                                          \
  return miseg::dispatch_dtype((p)->dtype, [&](auto* tag) -> int {          \
    typedef typename std::remove_pointer<decltype(tag)>::type T;            \
    __VA_ARGS__;                                                            \
    return MISEG_OK;                                                        \
  })
