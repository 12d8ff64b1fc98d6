// Projection onto SO(3) and the rotation moment (extension: the SVD mean head, the chordal
// mean and the Procrustes steps of pose alignment; so3_device.h so3_project).
//   lv_so3_project_fwd / _bwd   one thread per matrix, like the other per-sample maps
//   lv_so3_moment               S[s] = sum_i w_i op(X_i) C_s op(Y_i), its projection: two
//                               launches, fixed summation order, no atomics
#include "lv_common.h"
#include "pointwise_launch.h"
#include "so3_device.h"

namespace lv {

template <typename T>
__global__ void __launch_bounds__(kBlock) so3_project_fwd_k(const T* M, T* R, int64_t n) {
  LV_FOR_EACH(i, n) {
    T m[9], r[9];
    ld(M + i * 9, m);
    ProjectEig<T> pe;
    so3_project(m, r, pe);
    st(R + i * 9, r);
  }
}
template <typename T>
__global__ void __launch_bounds__(kBlock) so3_project_bwd_k(const T* M, const T* gR, T* gM, int64_t n) {
  LV_FOR_EACH(i, n) {
    T m[9], g[9], o[9];
    ld(M + i * 9, m);
    ld(gR + i * 9, g);
    so3_project_vjp(m, g, o);
    st(gM + i * 9, o);
  }
}

// ---------------------------------------------------------------- moment
// Stage 1: the grid is a function of n alone (never of the device), each thread adds its
// samples in ascending order in fp64, the block combines its 256 threads in a fixed order
// (xor butterflies inside a wave, then the four waves in order) and writes one partial of
// NS * 9 + 1 doubles to the workspace.  Stage 2: one block sums the partials in ascending
// order, projects in fp64 and writes S, wsum and R.  The same n gives the same bits.
constexpr int kMomentMaxBlocks = 128;
constexpr int kMomentMaxNs = 8;

inline int moment_blocks(int64_t n) {
  const int64_t b = (n + kBlock - 1) / kBlock;
  return (int)(b > kMomentMaxBlocks ? kMomentMaxBlocks : b);
}

__device__ __forceinline__ double wave_sum_f64(double x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

template <typename T, int NS>
__global__ void __launch_bounds__(kBlock) so3_moment_partial_k(const T* X, const T* Y, const T* w, const T* C,
                                                               int flags, double* part, int64_t n) {
  constexpr int W = NS * 9 + 1;
  __shared__ double cs[NS * 9];
  __shared__ double red[kBlock / 64][W];
  if (threadIdx.x < NS * 9) {
    const int s = threadIdx.x / 9, k = threadIdx.x % 9;
    const int kt = (flags & LV_MOMENT_CT) ? (k % 3) * 3 + k / 3 : k;
    cs[threadIdx.x] = C ? (double)C[s * 9 + kt] : ((k == 0 || k == 4 || k == 8) ? 1.0 : 0.0);
  }
  __syncthreads();
  double acc[NS][9], wacc = 0.0;
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[s][k] = 0.0;
  const bool xt = flags & LV_MOMENT_XT, yt = flags & LV_MOMENT_YT;
  LV_FOR_EACH(i, n) {
    // transposes by selects between compile-time indices: no run-time index into x or y
    double x[9], y[9];
    T raw[9];
    ld(X + i * 9, raw);
#pragma unroll
    for (int k = 0; k < 9; ++k) x[k] = (double)(xt ? raw[(k % 3) * 3 + k / 3] : raw[k]);
    if (Y) {
      ld(Y + i * 9, raw);
#pragma unroll
      for (int k = 0; k < 9; ++k) y[k] = (double)(yt ? raw[(k % 3) * 3 + k / 3] : raw[k]);
    }
    const double wi = w ? (double)w[i] : 1.0;
    wacc += wi;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      double c[9], t[9], u[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) c[k] = cs[s * 9 + k];
      if (C) {
        matmul3(x, c, t);
      } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) t[k] = x[k];
      }
      if (Y) {
        matmul3(t, y, u);
      } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) u[k] = t[k];
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) acc[s][k] += wi * u[k];
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const double r = wave_sum_f64(acc[s][k]);
      if (lane == 0) red[wave][s * 9 + k] = r;
    }
  {
    const double r = wave_sum_f64(wacc);
    if (lane == 0) red[wave][W - 1] = r;
  }
  __syncthreads();
  if (threadIdx.x < W) {
    double r = red[0][threadIdx.x];
#pragma unroll
    for (int v = 1; v < kBlock / 64; ++v) r += red[v][threadIdx.x];
    part[(int64_t)blockIdx.x * W + threadIdx.x] = r;
  }
}

template <typename T>
__global__ void __launch_bounds__(kBlock) so3_moment_final_k(const double* part, int blocks, int ns, double* S,
                                                             double* wsum, T* R) {
  __shared__ double tot[kMomentMaxNs * 9 + 1];
  const int W = ns * 9 + 1;
  if ((int)threadIdx.x < W) {
    double r = 0.0;
    for (int b = 0; b < blocks; ++b) r += part[(int64_t)b * W + threadIdx.x];
    tot[threadIdx.x] = r;
    if ((int)threadIdx.x < W - 1) S[threadIdx.x] = r;
    else if (wsum) *wsum = r;
  }
  __syncthreads();
  if (R && (int)threadIdx.x < ns) {
    double m[9], r[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = tot[threadIdx.x * 9 + k];
    ProjectEig<double> pe;
    so3_project(m, r, pe);
#pragma unroll
    for (int k = 0; k < 9; ++k) R[threadIdx.x * 9 + k] = (T)r[k];
  }
}

template <typename T>
int moment_launch(const T* X, const T* Y, const T* w, const T* C, int ns, int flags, double* S,
                  double* wsum, T* R, int64_t n, void* ws, size_t ws_bytes, void* stream) {
  clear_error();
  LV_CHECK_ARG(n >= 0, "n must be >= 0");
  LV_CHECK_ARG(ns >= 1 && ns <= kMomentMaxNs, "ns must be in [1, %d]", kMomentMaxNs);
  LV_CHECK_ARG(C || ns == 1, "ns must be 1 without C (the identity)");
  LV_CHECK_ARG((flags & ~(LV_MOMENT_XT | LV_MOMENT_YT | LV_MOMENT_CT)) == 0, "unknown flags");
  LV_CHECK_ARG(S, "null pointer argument (S)");
  LV_CHECK_ARG(n == 0 || X, "null pointer argument (X)");
  const size_t need = lv_so3_moment_workspace(n, ns);
  LV_CHECK_ARG(need == 0 || (ws && ws_bytes >= need), "workspace too small: %zu < %zu bytes",
               ws ? ws_bytes : (size_t)0, need);
  const int blocks = n > 0 ? moment_blocks(n) : 0;
  double* part = (double*)ws;
  if (blocks > 0) {
#define LV_MOMENT_CASE(NS)                                                                       \
  case NS:                                                                                       \
    hipLaunchKernelGGL((so3_moment_partial_k<T, NS>), dim3(blocks), dim3(kBlock), 0,             \
                       (hipStream_t)stream, X, Y, w, C, flags, part, n);                         \
    break;
    switch (ns) {
      LV_MOMENT_CASE(1)
      LV_MOMENT_CASE(2)
      LV_MOMENT_CASE(3)
      LV_MOMENT_CASE(4)
      LV_MOMENT_CASE(5)
      LV_MOMENT_CASE(6)
      LV_MOMENT_CASE(7)
      LV_MOMENT_CASE(8)
    }
#undef LV_MOMENT_CASE
    LV_CHECK_LAUNCH("so3_moment_partial_k");
  }
  hipLaunchKernelGGL(so3_moment_final_k<T>, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, part,
                     blocks, ns, S, wsum, R);
  LV_RETURN_LAUNCH("so3_moment_final_k");
}

}  // namespace lv

using namespace lv;

#define LV_PROJECT_LAUNCH(kern, n, ...)                                                      \
  do {                                                                                       \
    clear_error();                                                                           \
    if ((n) == 0) return LV_OK;                                                              \
    hipLaunchKernelGGL(kern, grid_for(n), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); \
    LV_RETURN_LAUNCH(#kern);                                                                 \
  } while (0)

extern "C" {

size_t lv_so3_moment_workspace(int64_t n, int ns) {
  if (n <= 0 || ns < 1 || ns > kMomentMaxNs) return 0;
  return sizeof(double) * (size_t)moment_blocks(n) * (size_t)(ns * 9 + 1);
}

#define LV_SO3_PROJECT_ENTRIES(T, SUF)                                                          \
  int lv_so3_project_fwd##SUF(const T* M, T* R, int64_t n, void* stream) {                      \
    LV_CHECK_ARG(n >= 0, "n must be >= 0");                                                     \
    LV_CHECK_ARG(n == 0 || (M && R), "null pointer argument");                                  \
    LV_PROJECT_LAUNCH(so3_project_fwd_k<T>, n, M, R, n);                                        \
  }                                                                                             \
  int lv_so3_project_bwd##SUF(const T* M, const T* gR, T* gM, int64_t n, void* stream) {        \
    LV_CHECK_ARG(n >= 0, "n must be >= 0");                                                     \
    LV_CHECK_ARG(n == 0 || (M && gR && gM), "null pointer argument");                           \
    LV_PROJECT_LAUNCH(so3_project_bwd_k<T>, n, M, gR, gM, n);                                   \
  }                                                                                             \
  int lv_so3_moment##SUF(const T* X, const T* Y, const T* w, const T* C, int ns, int flags,     \
                         double* S, double* wsum, T* R, int64_t n, void* workspace,             \
                         size_t workspace_bytes, void* stream) {                                \
    return moment_launch<T>(X, Y, w, C, ns, flags, S, wsum, R, n, workspace, workspace_bytes,   \
                            stream);                                                            \
  }
LV_SO3_PROJECT_ENTRIES(float, )
LV_SO3_PROJECT_ENTRIES(double, _f64)
#undef LV_SO3_PROJECT_ENTRIES

}  // extern "C"
