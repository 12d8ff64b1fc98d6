// Launch shape of the per-sample map kernels (pointwise.hip, vmf.hip): one thread per
// element, 256-thread blocks, a grid capped at 65,536 blocks with a grid-stride loop beyond.
#pragma once
#include "lv_common.h"

namespace lv {

constexpr int kBlock = 256;

inline dim3 grid_for(int64_t n) {
  int64_t b = (n + kBlock - 1) / kBlock;
  if (b > 65536) b = 65536;  // grid-stride beyond
  return dim3((unsigned)b);
}

#define LV_FOR_EACH(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

template <typename T, int K>
__device__ __forceinline__ void ld(const T* p, T (&x)[K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) x[i] = p[i];
}
template <typename T, int K>
__device__ __forceinline__ void st(T* p, const T (&x)[K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) p[i] = x[i];
}

}  // namespace lv
