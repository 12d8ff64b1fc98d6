// Real spherical harmonics on S^2 (extension: the signal f(x) = sum_k F_k Y_k(x) behind the
// action decoder's ((L+1)^2, C) spectrum).
//   lv_s2_harmonics_fwd   Y (P, M), one point per lane
//   lv_s2_synthesis_fwd   values[b,p,c] = sum_k Y_k(x_p) F[b,k,c]; Y lives in registers, the
//                         coefficient tile of one (batch, channel tile) is staged once per
//                         block in LDS and read back as same-address (broadcast) reads
//   lv_s2_analysis_fwd    F[b,k,c] = sum_p w_p Y_k(x_p) values[b,p,c], the adjoint: one wave per
//                         partial, a fixed-order butterfly over the 64 lanes, partial sums in a
//                         caller workspace, then a second launch that adds them in order
// Basis: orthonormal, real, no Condon-Shortley phase, k = l^2 + l + m, m < 0 sine-type:
//   Y_l^{+-m}(x) = sqrt2 q_l^m(z) {Re, Im}(x + iy)^m,   Y_l^0 = q_l^0(z),
//   q_m^m = sqrt((1/4pi) prod_{k<=m} (2k+1)/(2k)),  q_l^m = A_lm (z q_{l-1}^m - B_lm q_{l-2}^m),
//   A = sqrt((4l^2-1)/(l^2-m^2)),  B = sqrt(((l-1)^2-m^2)/(4(l-1)^2-1)).
// No trigonometric call and no division by sin(theta): the poles are ordinary points.  For
// |z| > 1/2 the product z q is formed from 1 - |z| (s2_for_each), which keeps the colatitude's
// precision near the poles.
#include <climits>

#include "lv_common.h"

namespace lv {

constexpr int kS2MaxL = LV_MAX_DEGREE;
constexpr int kS2Tab = (kS2MaxL + 1) * (kS2MaxL + 2) / 2;  // (l, m <= l) pairs
constexpr int kS2Wave = 64;
constexpr int kS2Block = 256;
constexpr int kS2MaxTile = 16;          // channels a lane accumulates
constexpr int64_t kS2SmallGrid = 512;   // below this many 256-thread blocks: 64-thread blocks
constexpr int64_t kS2TargetWaves = 2048;  // analysis: partials per (batch, tile) are cut to this
constexpr int kS2ReduceBlock = 256;

// The recurrence's constants, computed by each block in fp64 and rounded once: ab[l(l+1)/2+m]
// = (A_lm, B_lm) for l > m, start[m] = q_m^m (times sqrt2 for m > 0, the recurrence is linear).
struct S2Tables {
  float2 ab[kS2Tab];
  float start[kS2MaxL + 1];
};

__device__ __forceinline__ void s2_fill_tables(S2Tables& t, int L) {
  for (int i = threadIdx.x; i < kS2Tab; i += blockDim.x) {
    int l = 0;
    while ((l + 1) * (l + 2) / 2 <= i) ++l;
    const int m = i - l * (l + 1) / 2;
    float2 v = make_float2(0.f, 0.f);
    if (l > m && l <= L) {
      const double l2 = (double)l * l, m2 = (double)m * m, p2 = (double)(l - 1) * (l - 1);
      v.x = (float)sqrt((4.0 * l2 - 1.0) / (l2 - m2));
      v.y = (float)sqrt((p2 - m2) / (4.0 * p2 - 1.0));
    }
    t.ab[i] = v;
  }
  for (int m = threadIdx.x; m <= kS2MaxL; m += blockDim.x) {
    double s = 0.25 / 3.14159265358979323846;
    for (int k = 1; k <= m; ++k) s *= (2.0 * k + 1.0) / (2.0 * k);
    t.start[m] = (float)sqrt(m > 0 ? 2.0 * s : s);
  }
}

// The point's direction.  A point with a non-finite component, or the zero vector, has no
// direction: its three components become NaN and so does every harmonic of it (Y_0 too).
__device__ __forceinline__ bool s2_direction(const float* x, float& ux, float& uy, float& uz) {
  const float a = x[0], b = x[1], c = x[2];
  const float s = fmaxf(fmaxf(fabsf(a), fabsf(b)), fabsf(c));
  const bool ok = isfinite(a) && isfinite(b) && isfinite(c) && s > 0.f;
  if (!ok) {
    ux = uy = uz = __builtin_nanf("");
    return false;
  }
  const float sa = a / s, sb = b / s, sc = c / s;  // first by the largest: no overflow in r
  const float r = sqrtf(sa * sa + sb * sb + sc * sc);
  ux = sa / r;
  uy = sb / r;
  uz = sc / r;
  return true;
}

// f(k, Y_k) for every k < (L+1)^2 in one fixed order: m ascending, then l ascending, the
// cosine-type row before the sine-type one.  At +-z, ux = uy = 0 exactly and every m != 0
// harmonic is q * 0 = 0 exactly.
template <class Fn>
__device__ __forceinline__ void s2_for_each(const S2Tables& tab, int L, bool ok, float ux, float uy,
                                            float uz, Fn&& f) {
  const float nan = __builtin_nanf("");
  // Near a pole a rounded z no longer resolves the colatitude (d theta = dz / sin theta), but
  // 1 - |z| = (x^2 + y^2) / (1 + |z|) does, to its own relative precision: there z q is taken
  // as +-(q - t q) with one rounding.  This holds the fp32 error at 1.5e-6 of the row's norm
  // where the plain product loses 1.2e-5 within 0.3 rad of a pole.
  const float t = (ux * ux + uy * uy) / (1.f + fabsf(uz));
  const bool polar = fabsf(uz) > 0.5f;
  float re = 1.f, im = 0.f;
  for (int m = 0; m <= L; ++m) {
    if (m > 0) {  // (x + iy)^m
      const float nr = re * ux - im * uy, ni = re * uy + im * ux;
      re = nr;
      im = ni;
    }
    float q1 = ok ? tab.start[m] : nan, q2 = 0.f;  // q_l^m, q_{l-1}^m
    for (int l = m; l <= L; ++l) {
      if (l > m) {
        const float2 ab = tab.ab[l * (l + 1) / 2 + m];
        const float v = fmaf(-t, q1, q1);
        const float zq = polar ? (uz < 0.f ? -v : v) : uz * q1;
        const float q = ab.x * (zq - ab.y * q2);
        q2 = q1;
        q1 = q;
      }
      const int k0 = l * l + l;
      if (m == 0) {
        f(k0, q1);
      } else {
        f(k0 + m, q1 * re);
        f(k0 - m, q1 * im);
      }
    }
  }
}

// ---------------------------------------------------------------- basis
__global__ void __launch_bounds__(kS2Block) s2_harmonics_k(const float* __restrict__ x,
                                                           float* __restrict__ Y, int64_t P, int L) {
  __shared__ S2Tables tab;
  s2_fill_tables(tab, L);
  __syncthreads();
  const int64_t p = (int64_t)blockIdx.x * kS2Block + threadIdx.x;
  if (p >= P) return;
  float ux, uy, uz;
  const bool ok = s2_direction(x + p * 3, ux, uy, uz);
  float* row = Y + p * (int64_t)((L + 1) * (L + 1));
  s2_for_each(tab, L, ok, ux, uy, uz, [&](int k, float y) { row[k] = y; });
}

// ---------------------------------------------------------------- synthesis
// Block (batch b, channel tile ct, point block pb), flattened into blockIdx.x.  The tile
// F[b, :, ct*CT .. ct*CT+CT) (channels past C read as 0) sits in LDS as (M, CT); every lane
// reads the same row, so a read is one broadcast and never a bank conflict.
template <int CT>
__global__ void __launch_bounds__(kS2Block) s2_synthesis_k(const float* __restrict__ F,
                                                           int64_t f_stride,
                                                           const float* __restrict__ x,
                                                           float* __restrict__ out, int64_t P, int L,
                                                           int C, int ctiles, int64_t pblocks) {
  __shared__ S2Tables tab;
  extern __shared__ __attribute__((aligned(16))) float fs[];
  const int M = (L + 1) * (L + 1);
  const int64_t pb = blockIdx.x % pblocks;
  const int64_t bc = blockIdx.x / pblocks;
  const int ct = (int)(bc % ctiles);
  const int64_t b = bc / ctiles;
  s2_fill_tables(tab, L);
  const float* Fb = F + b * f_stride;
  for (int i = threadIdx.x; i < M * CT; i += blockDim.x) {
    const int k = i / CT, c = ct * CT + i % CT;
    fs[i] = c < C ? Fb[(int64_t)k * C + c] : 0.f;
  }
  __syncthreads();
  const int64_t p = pb * blockDim.x + threadIdx.x;
  if (p >= P) return;
  float ux, uy, uz;
  const bool ok = s2_direction(x + p * 3, ux, uy, uz);
  float acc[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) acc[c] = 0.f;
  s2_for_each(tab, L, ok, ux, uy, uz, [&](int k, float y) {
    const float* f = fs + k * CT;
    if constexpr (CT % 4 == 0) {
#pragma unroll
      for (int c = 0; c < CT; c += 4) {
        const float4 v = *reinterpret_cast<const float4*>(f + c);
        acc[c] = fmaf(y, v.x, acc[c]);
        acc[c + 1] = fmaf(y, v.y, acc[c + 1]);
        acc[c + 2] = fmaf(y, v.z, acc[c + 2]);
        acc[c + 3] = fmaf(y, v.w, acc[c + 3]);
      }
    } else {
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c] = fmaf(y, f[c], acc[c]);
    }
  });
  float* o = out + (b * P + p) * (int64_t)C + ct * CT;
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (ct * CT + c < C) o[c] = acc[c];
}

// ---------------------------------------------------------------- analysis
// One wave per (batch b, channel tile ct, partial `part`), flattened into blockIdx.x.  The wave
// walks its chunks of 64 points (part, part + nparts, ...) in ascending order, one point per
// lane; a lane past P carries zeros.  For each row k the CT products of a lane are summed over
// the wave by a butterfly that halves the array at masks 1, 2, ... CT/2 and then folds the one
// remaining value at masks CT ... 32: lane j ends with channel j % CT.  The order is fixed, so
// the same inputs give the same bits.  The wave owns its slab of the workspace: the first
// chunk writes it, later chunks add to it (plain loads and stores by the one owning lane).
template <int CT>
__device__ __forceinline__ float s2_wave_reduce(float (&t)[CT], int lane) {
#pragma unroll
  for (int s = 1, n = CT; n > 1; s <<= 1, n >>= 1) {
    const bool hi = lane & s;
#pragma unroll
    for (int j = 0; j < n / 2; ++j) {
      const float keep = hi ? t[2 * j + 1] : t[2 * j];
      const float send = hi ? t[2 * j] : t[2 * j + 1];
      t[j] = keep + __shfl_xor(send, s);
    }
  }
  float r = t[0];
#pragma unroll
  for (int s = CT; s < kS2Wave; s <<= 1) r += __shfl_xor(r, s);
  return r;
}

template <int CT>
__global__ void __launch_bounds__(kS2Wave) s2_analysis_partial_k(const float* __restrict__ values,
                                                                 const float* __restrict__ x,
                                                                 const float* __restrict__ w,
                                                                 float* part_out, int64_t B,
                                                                 int64_t P, int L, int C,
                                                                 int ctiles, int64_t nparts) {
  __shared__ S2Tables tab;
  const int M = (L + 1) * (L + 1);
  const int64_t part = blockIdx.x % nparts;
  const int64_t bc = blockIdx.x / nparts;
  const int ct = (int)(bc % ctiles);
  const int64_t b = bc / ctiles;
  s2_fill_tables(tab, L);
  __syncthreads();
  const int lane = threadIdx.x;
  const int my_c = ct * CT + lane % CT;
  float* slab = part_out + ((part * B + b) * M) * (int64_t)C;
  const int64_t chunks = (P + kS2Wave - 1) / kS2Wave;
  for (int64_t chunk = part; chunk < chunks; chunk += nparts) {
    const int64_t p = chunk * kS2Wave + lane;
    float ux = 0.f, uy = 0.f, uz = 1.f, v[CT];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < CT; ++c) v[c] = 0.f;
    if (p < P) {
      ok = s2_direction(x + p * 3, ux, uy, uz);
      const float wp = w ? w[p] : 1.f;
      const float* src = values + (b * P + p) * (int64_t)C + ct * CT;
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (ct * CT + c < C) v[c] = wp * src[c];
    }
    const bool first = chunk == part;
    s2_for_each(tab, L, ok, ux, uy, uz, [&](int k, float y) {
      float t[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c) t[c] = y * v[c];
      const float r = s2_wave_reduce<CT>(t, lane);
      if (lane < CT && my_c < C) {
        float* dst = slab + (int64_t)k * C + my_c;
        *dst = first ? r : *dst + r;
      }
    });
  }
}

// F[i] = sum over the partials in ascending order, i over B * M * C.
__global__ void __launch_bounds__(kS2ReduceBlock) s2_analysis_reduce_k(const float* __restrict__ part,
                                                                       float* __restrict__ F,
                                                                       int64_t n, int64_t nparts) {
  for (int64_t i = (int64_t)blockIdx.x * kS2ReduceBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kS2ReduceBlock) {
    float r = part[i];
    for (int64_t q = 1; q < nparts; ++q) r += part[q * n + i];
    F[i] = r;
  }
}

// ---------------------------------------------------------------- plans
struct S2Plan {
  int tile;         // channels per lane (0: the basis)
  int ctiles;
  int threads;
  int64_t pblocks;  // point blocks (basis, synthesis)
  int64_t grid;
  int64_t lds;      // static + dynamic bytes per block
  int64_t nparts;   // analysis: partial sums per (batch, k, c)
  int64_t grid2;    // analysis: blocks of the second launch
  size_t ws_bytes;  // analysis
};

inline int s2_tile(int C) { return C <= 1 ? 1 : C <= 2 ? 2 : C <= 4 ? 4 : C <= 8 ? 8 : kS2MaxTile; }

// Shape checks and dispatch shared by the launches, lv_s2_plan and lv_s2_analysis_workspace.
int s2_plan(int op, int64_t B, int64_t P, int L, int C, S2Plan* pl) {
  LV_CHECK_ARG(op >= LV_S2_OP_HARMONICS && op <= LV_S2_OP_ANALYSIS, "s2: unknown op %d", op);
  LV_CHECK_ARG(L >= 0 && L <= kS2MaxL, "s2: L must be in 0..%d (got %d)", kS2MaxL, L);
  LV_CHECK_ARG(P >= 0, "s2: P must be >= 0 (got %lld)", (long long)P);
  const int64_t M = (int64_t)(L + 1) * (L + 1);
  *pl = S2Plan{};
  pl->threads = kS2Block;
  pl->lds = (int64_t)sizeof(S2Tables);
  const int64_t lim = INT64_MAX / 4;  // byte offsets stay inside int64
  if (op == LV_S2_OP_HARMONICS) {
    LV_CHECK_ARG(P <= lim / M, "s2: P * (L+1)^2 exceeds the index range (P = %lld)", (long long)P);
    pl->pblocks = (P + kS2Block - 1) / kS2Block;
    LV_CHECK_ARG(pl->pblocks <= INT_MAX, "s2: P = %lld needs more than 2^31-1 blocks", (long long)P);
    pl->grid = pl->pblocks;
    return LV_OK;
  }
  LV_CHECK_ARG(C >= 1 && C <= LV_MAX_CHANNELS, "s2: C must be in 1..%d (got %d)", LV_MAX_CHANNELS, C);
  LV_CHECK_ARG(B >= 0, "s2: B must be >= 0 (got %lld)", (long long)B);
  LV_CHECK_ARG(B == 0 || (B <= lim / (M * C) && (P == 0 || B <= lim / C / P)),
               "s2: B * P * C or B * (L+1)^2 * C exceeds the index range (B = %lld, P = %lld)",
               (long long)B, (long long)P);
  pl->tile = s2_tile(C);
  pl->ctiles = (C + pl->tile - 1) / pl->tile;
  const int64_t per_point_block = B * pl->ctiles;
  if (op == LV_S2_OP_SYNTHESIS) {
    pl->pblocks = (P + kS2Block - 1) / kS2Block;
    if (pl->pblocks > 0 && per_point_block <= kS2SmallGrid / pl->pblocks) {
      // a small problem: more, smaller blocks (each output is one lane's sum, so the block
      // size never changes a bit)
      pl->threads = kS2Wave;
      pl->pblocks = (P + kS2Wave - 1) / kS2Wave;
    }
    LV_CHECK_ARG(pl->pblocks == 0 || per_point_block <= INT_MAX / pl->pblocks,
                 "s2: the problem needs more than 2^31-1 blocks (B = %lld, P = %lld)", (long long)B,
                 (long long)P);
    pl->grid = per_point_block * pl->pblocks;
    pl->lds += M * pl->tile * (int64_t)sizeof(float);
    return LV_OK;
  }
  pl->threads = kS2Wave;
  const int64_t chunks = (P + kS2Wave - 1) / kS2Wave;
  int64_t want = per_point_block > 0 ? (kS2TargetWaves + per_point_block - 1) / per_point_block : 1;
  if (want < 1) want = 1;
  pl->nparts = chunks < want ? chunks : want;
  if (B == 0) pl->nparts = 0;
  LV_CHECK_ARG(pl->nparts == 0 || per_point_block <= INT_MAX / pl->nparts,
               "s2: the problem needs more than 2^31-1 blocks (B = %lld, P = %lld)", (long long)B,
               (long long)P);
  pl->grid = per_point_block * pl->nparts;
  const int64_t n = B * M * C;
  LV_CHECK_ARG(pl->nparts == 0 || n <= lim / pl->nparts,
               "s2: the analysis workspace exceeds the index range (B = %lld, P = %lld)",
               (long long)B, (long long)P);
  pl->ws_bytes = (size_t)(pl->nparts * n) * sizeof(float);
  const int64_t g2 = (n + kS2ReduceBlock - 1) / kS2ReduceBlock;
  pl->grid2 = pl->nparts == 0 ? 0 : (g2 > 65536 ? 65536 : g2);
  return LV_OK;
}

}  // namespace lv

using namespace lv;

extern "C" {

int lv_s2_plan(int op, int64_t B, int64_t P, int L, int C, int64_t* plan) {
  clear_error();
  LV_CHECK_ARG(plan, "null pointer argument");
  S2Plan pl;
  if (int rc = s2_plan(op, B, P, L, C, &pl)) return rc;
  plan[0] = pl.tile;
  plan[1] = pl.grid;
  plan[2] = pl.threads;
  plan[3] = pl.lds;
  plan[4] = pl.nparts;
  plan[5] = pl.grid2;
  return LV_OK;
}

size_t lv_s2_analysis_workspace(int64_t B, int64_t P, int L, int C) {
  S2Plan pl;
  if (s2_plan(LV_S2_OP_ANALYSIS, B, P, L, C, &pl) != LV_OK) return 0;
  return pl.ws_bytes;
}

int lv_s2_harmonics_fwd(const float* x, float* Y, int64_t P, int L, void* stream) {
  clear_error();
  S2Plan pl;
  if (int rc = s2_plan(LV_S2_OP_HARMONICS, 1, P, L, 1, &pl)) return rc;
  if (P == 0) return LV_OK;
  LV_CHECK_ARG(x && Y, "null pointer argument");
  hipLaunchKernelGGL(s2_harmonics_k, dim3((unsigned)pl.grid), dim3(kS2Block), 0,
                     (hipStream_t)stream, x, Y, P, L);
  LV_RETURN_LAUNCH("s2_harmonics_k");
}

int lv_s2_synthesis_fwd(const float* F, int64_t F_batch_stride, const float* x, float* values,
                        int64_t B, int64_t P, int L, int C, void* stream) {
  clear_error();
  S2Plan pl;
  if (int rc = s2_plan(LV_S2_OP_SYNTHESIS, B, P, L, C, &pl)) return rc;
  const int64_t M = (int64_t)(L + 1) * (L + 1);
  LV_CHECK_ARG(F_batch_stride == 0 || F_batch_stride == M * C,
               "s2_synthesis: F_batch_stride must be 0 (shared) or (L+1)^2 * C = %lld (got %lld)",
               (long long)(M * C), (long long)F_batch_stride);
  if (B == 0 || P == 0) return LV_OK;
  LV_CHECK_ARG(F && x && values, "null pointer argument");
  const size_t dyn = (size_t)(M * pl.tile) * sizeof(float);
#define LV_S2_SYNTH_CASE(CT)                                                                   \
  case CT:                                                                                     \
    hipLaunchKernelGGL(s2_synthesis_k<CT>, dim3((unsigned)pl.grid), dim3(pl.threads), dyn,     \
                       (hipStream_t)stream, F, F_batch_stride, x, values, P, L, C, pl.ctiles,  \
                       pl.pblocks);                                                            \
    break;
  switch (pl.tile) {
    LV_S2_SYNTH_CASE(1)
    LV_S2_SYNTH_CASE(2)
    LV_S2_SYNTH_CASE(4)
    LV_S2_SYNTH_CASE(8)
    LV_S2_SYNTH_CASE(16)
  }
#undef LV_S2_SYNTH_CASE
  LV_RETURN_LAUNCH("s2_synthesis_k");
}

int lv_s2_analysis_fwd(const float* values, const float* x, const float* w, float* F, int64_t B,
                       int64_t P, int L, int C, void* workspace, size_t workspace_bytes,
                       void* stream) {
  clear_error();
  S2Plan pl;
  if (int rc = s2_plan(LV_S2_OP_ANALYSIS, B, P, L, C, &pl)) return rc;
  if (B == 0 || P == 0) return LV_OK;
  LV_CHECK_ARG(values && x && F, "null pointer argument");
  LV_CHECK_ARG(workspace && workspace_bytes >= pl.ws_bytes, "workspace too small: %zu < %zu bytes",
               workspace ? workspace_bytes : (size_t)0, pl.ws_bytes);
  float* part = (float*)workspace;
#define LV_S2_ANA_CASE(CT)                                                                     \
  case CT:                                                                                     \
    hipLaunchKernelGGL(s2_analysis_partial_k<CT>, dim3((unsigned)pl.grid), dim3(kS2Wave), 0,   \
                       (hipStream_t)stream, values, x, w, part, B, P, L, C, pl.ctiles,         \
                       pl.nparts);                                                             \
    break;
  switch (pl.tile) {
    LV_S2_ANA_CASE(1)
    LV_S2_ANA_CASE(2)
    LV_S2_ANA_CASE(4)
    LV_S2_ANA_CASE(8)
    LV_S2_ANA_CASE(16)
  }
#undef LV_S2_ANA_CASE
  LV_CHECK_LAUNCH("s2_analysis_partial_k");
  const int64_t n = B * (int64_t)(L + 1) * (L + 1) * C;
  hipLaunchKernelGGL(s2_analysis_reduce_k, dim3((unsigned)pl.grid2), dim3(kS2ReduceBlock), 0,
                     (hipStream_t)stream, part, F, n, pl.nparts);
  LV_RETURN_LAUNCH("s2_analysis_reduce_k");
}

}  // extern "C"
