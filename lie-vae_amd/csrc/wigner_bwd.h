#pragma once
// VJP of the Wigner-D blocks (lv_wigner_d_block_bwd, lv_wigner_d_bwd): gD -> gang.  The
// reference gets it from autograd through lie_tools.py:211-223.  Instantiated once per
// degree in action_bwd_inst.hip (-DLV_INST_L=k), like the forward's wigner_d_kernel.
#include "action_bwd.h"

namespace lv {

// <g, dX_l(θ)/dθ · x> on one slot's multiples (xrot_dot_deriv's arithmetic in
// action_chain.h, operation for operation).
template <int l>
__device__ __forceinline__ float xm_dot_deriv(const Mult<l>& m, const float (&g)[2 * l + 1],
                                              const float (&x)[2 * l + 1]) {
  float acc = 0.f;
  sfor<2 * l + 1>([&](auto I) {
    constexpr int i = LV_CV(I);
    constexpr int f = l - i;
    if constexpr (f > 0) {
      const float d = fmaf(-m.s[f], x[i], m.c[f] * x[2 * l - i]);
      acc = fmaf(g[i], (float)f * d, acc);
    } else if constexpr (f < 0) {
      const float d = fmaf(m.s[-f], x[i], m.c[-f] * x[2 * l - i]);
      acc = fmaf(g[i], (float)f * d, acc);
    }
  });
  return acc;
}

// <G, dX_l(θ)/dθ · x> and y = X_l(θ)^T G in one pass over the row pairs (i, 2l-i), with G
// read through ld(row) right where the pair needs it, so that no (2l+1)-register copy of G
// stays live (xm_dot_deriv's and xm_t's terms; the sum runs pair by pair).
template <int l, class Ld>
__device__ __forceinline__ float xm_t_dot_deriv_ld(const Mult<l>& m, Ld&& ld, const float (&x)[2 * l + 1],
                                                   float (&y)[2 * l + 1]) {
  float acc = 0.f;
  sfor<l>([&](auto I) {
    constexpr int i = LV_CV(I);
    constexpr int f = l - i;
    const float a = ld(i), b = ld(2 * l - i);
    const float da = fmaf(-m.s[f], x[i], m.c[f] * x[2 * l - i]);
    const float db = fmaf(m.s[f], x[2 * l - i], m.c[f] * x[i]);
    acc = fmaf(a, (float)f * da, acc);
    acc = fmaf(b, (float)(-f) * db, acc);
    y[i] = fmaf(m.c[f], a, -(m.s[f] * b));
    y[2 * l - i] = fmaf(m.c[f], b, m.s[f] * a);
  });
  y[l] = ld(l);
  return acc;
}

// Samples per block of the backward: whole samples only, so that a sample's 2l+1 column
// partials meet in one block's LDS (at most 64: the multiples take 3 threads per sample).
template <int l>
constexpr int wig_bwd_samples() {
  return kWigThreads / (2 * l + 1) < 64 ? kWigThreads / (2 * l + 1) : 64;
}
constexpr int wig_bwd_samples_rt(int l) { return kWigThreads / (2 * l + 1) < 64 ? kWigThreads / (2 * l + 1) : 64; }

// One lane per (sample, column q) of D_l.  With G = gD[s, :, q] and e_q the unit vector:
//   P1 = Xc e_q, P2 = J P1, P3 = Xb P2, P4 = J P3            (forward recompute)
//   ga_q = <G, Xa' P4>;  Q4 = Xa^T G, Q3 = J Q4         (one pass over G's row pairs)
//   gb_q = <Q3, Xb' P2>; Q2 = Xb^T Q3, Q1 = J Q2
//   gc_q = <Q1, Xc' e_q>
// and gang[s] = sum_q (ga_q, gb_q, gc_q), added in ascending q by one thread per (sample,
// angle) from the block's LDS: no atomics, no workspace, and a sample's result depends on
// nothing but its own angles and gD (bitwise the same alone, anywhere in a batch, in any
// grid).  The multiples live in an LDS row per sample (the register table is 6(l+1) VGPRs;
// beside P2, P4 and G it does not fit at l = 20), one Euler slot's in registers at a time.
// Lanes past the block's last sample mirror it (defined values, nothing written).
// accumulate: gang += instead of gang = (the packed VJP's degrees 1..L; every element has
// one owning thread per launch and the launches are ordered by the stream).
template <int l>
__global__ __launch_bounds__(kWigThreads)
void wigner_d_bwd_kernel(const float* ang, const float* gD, float* gang, int64_t n, int64_t pitch, int off,
                         int accumulate) {
  constexpr int nn = 2 * l + 1;
  constexpr int S = wig_bwd_samples<l>();
  constexpr int kRow = TrigLds<l>::kRow;
  static_assert(3 * S <= kWigThreads && S * nn <= kWigThreads, "wigner backward block layout");
  __shared__ __attribute__((aligned(16))) float trig[S * kRow];
  __shared__ float part[3][S * nn];
  const int tid = (int)threadIdx.x;
  const int64_t s0 = (int64_t)blockIdx.x * S;
  const int Sv = (int)min((int64_t)S, n - s0);  // >= 1: blockIdx.x < ceil(n / S)
  // multiples: thread 3 j + slot fills sample j's row for that Euler slot
  const int jt = tid / 3, slot = tid - 3 * jt;
  if (jt < S) {
    float sq, cq;
    sincosf(ang[(s0 + min(jt, Sv - 1)) * 3 + slot], &sq, &cq);
    trig_row_fill1<l>(trig + jt * kRow, cq, sq, slot, l);
  }
  __syncthreads();
  const int jr = tid / nn;
  const int q = tid - jr * nn;
  const bool lane_on = jr < S;
  const int j = min(jr, S - 1);
  const float* tj = trig + j * kRow;

  float x[nn], y[nn], p2[nn], p4[nn];
  sfor<nn>([&](auto K) { x[LV_CV(K)] = (LV_CV(K) == q) ? 1.f : 0.f; });
  {
    const Mult<l> mc = mult_lds<l, 2, l>(tj);
    xm<l>(mc, x, y);
  }
  jmul<l>(y, p2);
  {
    const Mult<l> mb = mult_lds<l, 1, l>(tj);
    xm<l>(mb, p2, y);
  }
  jmul<l>(y, p4);
  float ga, gb, gc;
  {
    // G by buffer loads based at the block's first sample: the lane's 32-bit byte offset in
    // a VGPR and the row's in the scalar offset, so the 2l+1 loads need no address registers
    // of their own (rows past a 12-bit immediate would take a 64-bit address each)
    const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(gD) + s0 * pitch + off, 0, (int)(((Sv - 1) * pitch + nn * nn) * 4), kRawBufferFlags);
    const int voff = (int)((min(j, Sv - 1) * pitch + q) * 4);
    auto ldg = [&](int row) {
      return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(grs, voff, row * nn * 4, 0));
    };
    const Mult<l> ma = mult_lds<l, 0, l>(tj);
    ga = xm_t_dot_deriv_ld<l>(ma, ldg, p4, y);  // and Q4
  }
  jmul<l>(y, x);  // Q3
  {
    const Mult<l> mb = mult_lds<l, 1, l>(tj);
    gb = xm_dot_deriv<l>(mb, x, p2);
    xm_t<l>(mb, x, y);  // Q2
  }
  jmul<l>(y, x);  // Q1
  {
    sfor<nn>([&](auto K) { y[LV_CV(K)] = (LV_CV(K) == q) ? 1.f : 0.f; });
    const Mult<l> mc = mult_lds<l, 2, l>(tj);
    gc = xm_dot_deriv<l>(mc, x, y);
  }
  if (lane_on) {
    part[0][tid] = ga;
    part[1][tid] = gb;
    part[2][tid] = gc;
  }
  __syncthreads();
  if (jt < Sv) {
    const float* pj = part[slot] + jt * nn;
    float acc = pj[0];
#pragma unroll
    for (int k = 1; k < nn; ++k) acc += pj[k];
    float* dst = gang + (s0 + jt) * 3 + slot;
    *dst = accumulate ? *dst + acc : acc;
  }
}

struct WigBwdLaunch {
  const float* ang;
  const float* gD;
  float* gang;
  int64_t n;
  int64_t pitch;   // floats per sample of gD
  bool packed;     // block l at wigner_block_off(l) of the row, else at 0
  bool accumulate;
  hipStream_t stream;
};

template <int l>
struct WigBwdLauncher {
  static int run(WigBwdLaunch& p);  // out of class: see FwdLauncher
};
template <int l>
int WigBwdLauncher<l>::run(WigBwdLaunch& p) {
  hipLaunchKernelGGL((wigner_d_bwd_kernel<l>), dim3(ceil_div(p.n, wig_bwd_samples<l>())), dim3(kWigThreads), 0,
                     p.stream, p.ang, p.gD, p.gang, p.n, p.pitch, p.packed ? wigner_block_off(l) : 0,
                     p.accumulate ? 1 : 0);
  LV_RETURN_LAUNCH("wigner_d_bwd_kernel");
}

#define LV_EXTERN_WIG_BWD(L) extern template struct WigBwdLauncher<L>;

}  // namespace lv
