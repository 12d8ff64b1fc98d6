// Image-space and encoding-space kernels of the encoder regularisers
// (reference lie_vae/losses/equivariance_loss.py, encoder_continuity_loss.py):
//   rotate_k          per-image planar rotation with bilinear taps (EquivarianceLoss.rotate:
//                     affine_grid + grid_sample in one pass, no (N, H, W, 2) grid in memory);
//   equiv_diff_*_k    diffs[n] = sum (g_n enc_n - enc_rot_n)^2, g = s2s1rodrigues(e_x, cs);
//   pair_sqdist_*_k   diffs[n] = sum (enc[2n] - enc[2n+1])^2 over D columns.
// Built with -ffp-contract=off like the conversion kernels; the rotation asks for its two
// FMAs explicitly (fmaf).
#include <climits>

#include "lv_common.h"
#include "so3_device.h"

namespace lv {

constexpr int kImgBlock = 256;
constexpr int64_t kStagedMaxBytes = 65536;  // one source plane in LDS
constexpr int64_t kMaxGrid = 65536;         // grid-stride beyond (direct path, loss kernels)

// Pixel-space form of affine_grid + grid_sample's coordinate maps.  With dx = j - (W-1)/2,
// dy = i - (H-1)/2 (exact in fp32: half-integers) the source position of output pixel
// (i, j) under theta = [[c, -s, 0], [s, c, 0]] is
//   ix = (W-1)/2 + c dx - s ax dy,   iy = (H-1)/2 + s ay dx + c dy,
// ax = W/H, ay = H/W (align_corners = 0) or (W-1)/(H-1), (H-1)/(W-1) (align_corners = 1; 0
// where the denominator is 0: that axis has one pixel, so its offset is 0).  Two roundings
// per coordinate, and (c, s) = (1, 0), (-1, 0) and, for H = W, (0, +-1) give integer
// positions exactly, so those rotations copy pixels bit for bit.
struct RotGeom {
  int H, W;
  float cx, cy, ax, ay;
};

// One output pixel from four taps of the source plane `src` (LDS or global memory; both
// paths call this, so they agree bitwise).  Taps outside the plane read as zero
// (grid_sample padding_mode='zeros'); weights and summation order as torch's
// grid_sampler_2d (nw, ne, sw, se).
template <typename P>
__device__ __forceinline__ float rotate_tap(P src, const RotGeom& g, float c, float sx, float sy,
                                            int i, int j) {
  const float dx = (float)j - g.cx;
  const float dy = (float)i - g.cy;
  const float ix = fmaf(c, dx, fmaf(-sx, dy, g.cx));
  const float iy = fmaf(c, dy, fmaf(sy, dx, g.cy));
  const float fx = floorf(ix), fy = floorf(iy);
  // positions outside (-1, W) x (-1, H) have no tap inside the plane (and would overflow
  // the int casts for non-finite cs)
  if (!(fx >= -1.f && fx <= (float)(g.W - 1) && fy >= -1.f && fy <= (float)(g.H - 1))) return 0.f;
  const int x0 = (int)fx, y0 = (int)fy;
  const int x1 = x0 + 1, y1 = y0 + 1;
  const float wx1 = ix - fx, wy1 = iy - fy;
  const float wx0 = (fx + 1.f) - ix, wy0 = (fy + 1.f) - iy;
  const bool xin0 = x0 >= 0, xin1 = x1 < g.W, yin0 = y0 >= 0, yin1 = y1 < g.H;
  const float nw = (xin0 && yin0) ? src[y0 * g.W + x0] : 0.f;
  const float ne = (xin1 && yin0) ? src[y0 * g.W + x1] : 0.f;
  const float sw = (xin0 && yin1) ? src[y1 * g.W + x0] : 0.f;
  const float se = (xin1 && yin1) ? src[y1 * g.W + x1] : 0.f;
  return ((nw * (wx0 * wy0) + ne * (wx1 * wy0)) + sw * (wx0 * wy1)) + se * (wx1 * wy1);
}

// RUN consecutive output pixels of one plane, starting at flat index q (rows may wrap).
template <int RUN, typename P>
__device__ __forceinline__ void rotate_run(P src, const RotGeom& g, float c, float sx, float sy,
                                           int q, float* dst) {
  int i = q / g.W, j = q - i * g.W;
  float o[RUN];
#pragma unroll
  for (int k = 0; k < RUN; ++k) {
    o[k] = rotate_tap(src, g, c, sx, sy, i, j);
    if (++j == g.W) { j = 0; ++i; }
  }
  if constexpr (RUN == 4) {
    *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int k = 0; k < RUN; ++k) dst[k] = o[k];
  }
}

// Staged path: block = one (sample, channel) plane, copied to LDS, then gathered from there.
// RUN = 4: H·W % 4 == 0 and 16-byte aligned tensors (16-byte loads and stores); RUN = 1 else.
template <int RUN>
__global__ __launch_bounds__(kImgBlock) void rotate_staged_k(const float* __restrict__ img,
                                                             const float* __restrict__ cs,
                                                             float* __restrict__ out, int C,
                                                             RotGeom g) {
  extern __shared__ float plane[];
  const int64_t p = blockIdx.x;
  const int HW = g.H * g.W;
  const float* src = img + p * HW;
  float* dst = out + p * HW;
  if constexpr (RUN == 4) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* p4 = reinterpret_cast<float4*>(plane);
    for (int t = threadIdx.x; t < HW / 4; t += kImgBlock) p4[t] = s4[t];
  } else {
    for (int t = threadIdx.x; t < HW; t += kImgBlock) plane[t] = src[t];
  }
  const int64_t n = p / C;
  const float c = cs[n * 2], s = cs[n * 2 + 1];
  const float sx = s * g.ax, sy = s * g.ay;
  __syncthreads();
  for (int q = threadIdx.x * RUN; q < HW; q += kImgBlock * RUN)
    rotate_run<RUN>((const float*)plane, g, c, sx, sy, q, dst + q);
}

// Direct path: grid-stride over runs of output pixels, taps from global memory.
template <int RUN>
__global__ __launch_bounds__(kImgBlock) void rotate_direct_k(const float* __restrict__ img,
                                                             const float* __restrict__ cs,
                                                             float* __restrict__ out, int64_t NC,
                                                             int C, RotGeom g) {
  const int HW = g.H * g.W;
  const int runs = HW / RUN;  // per plane
  const int64_t total = NC * runs;
  for (int64_t r = (int64_t)blockIdx.x * kImgBlock + threadIdx.x; r < total;
       r += (int64_t)gridDim.x * kImgBlock) {
    const int64_t p = r / runs;
    const int q = (int)(r - p * runs) * RUN;
    const int64_t n = p / C;
    const float c = cs[n * 2], s = cs[n * 2 + 1];
    rotate_run<RUN>(img + p * HW, g, c, s * g.ax, s * g.ay, q, out + p * HW + q);
  }
}

// ---------------------------------------------------------------- loss kernels
#define LV_IMG_FOR_EACH(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// g = s2s1rodrigues((1, 0, 0), cs): equivariance_loss.py:28-30.
__device__ __forceinline__ void equiv_g(const float* cs, int64_t i, float g[9]) {
  const float ex[3] = {1.f, 0.f, 0.f};
  const float c[2] = {cs[i * 2], cs[i * 2 + 1]};
  s2s1_fwd(ex, c, g);
}

// equivariance_loss.py:32,36: enc_rot = g.bmm(enc); diffs = (enc_rot - e2).pow(2).sum().
__global__ void equiv_diff_fwd_k(const float* cs, const float* enc, const float* enc_rot,
                                 float* diffs, int64_t n) {
  LV_IMG_FOR_EACH(i, n) {
    float g[9], e[9], r[9], ge[9];
    equiv_g(cs, i, g);
#pragma unroll
    for (int k = 0; k < 9; ++k) { e[k] = enc[i * 9 + k]; r[k] = enc_rot[i * 9 + k]; }
    matmul3(g, e, ge);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float d = ge[k] - r[k];
      acc += d * d;
    }
    diffs[i] = acc;
  }
}

// d = g enc - enc_rot;  g_enc_rot = -2 gdiffs d;  g_enc = g^T (2 gdiffs d).
__global__ void equiv_diff_bwd_k(const float* cs, const float* enc, const float* enc_rot,
                                 const float* gdiffs, float* g_enc, float* g_enc_rot, int64_t n) {
  LV_IMG_FOR_EACH(i, n) {
    float g[9], e[9], ge[9], gd[9], o[9];
    equiv_g(cs, i, g);
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = enc[i * 9 + k];
    matmul3(g, e, ge);
    const float w = gdiffs[i];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      gd[k] = (2.f * (ge[k] - enc_rot[i * 9 + k])) * w;
      g_enc_rot[i * 9 + k] = -gd[k];
    }
    matmul3_tn(g, gd, o);
#pragma unroll
    for (int k = 0; k < 9; ++k) g_enc[i * 9 + k] = o[k];
  }
}

// encoder_continuity_loss.py:18-20: rows 2i and 2i+1 are a pair.
__global__ void pair_sqdist_fwd_k(const float* enc, float* diffs, int64_t n, int D) {
  LV_IMG_FOR_EACH(i, n) {
    const float* a = enc + i * 2 * D;
    float acc = 0.f;
    for (int k = 0; k < D; ++k) {
      const float d = a[k] - a[D + k];
      acc += d * d;
    }
    diffs[i] = acc;
  }
}
// one thread per element of g_enc (2n, D)
__global__ void pair_sqdist_bwd_k(const float* enc, const float* gdiffs, float* g_enc,
                                  int64_t n, int D) {
  LV_IMG_FOR_EACH(t, n * 2 * D) {
    const int64_t i = t / (2 * D);
    const int k = (int)(t - i * 2 * D);
    const float* a = enc + i * 2 * D;
    const int col = k < D ? k : k - D;
    const float gd = (2.f * (a[col] - a[D + col])) * gdiffs[i];
    g_enc[t] = k < D ? gd : -gd;
  }
}

inline dim3 img_grid(int64_t n) {
  int64_t b = (n + kImgBlock - 1) / kImgBlock;
  return dim3((unsigned)(b > kMaxGrid ? kMaxGrid : b));
}

struct RotPlan {
  int staged;
  int64_t grid;
  int lds;
};

// Shape checks and the dispatch shared by lv_rotate_bilinear_fwd and lv_rotate_plan.
int rotate_plan(int64_t N, int C, int H, int W, int flags, RotPlan* pl) {
  LV_CHECK_ARG(N >= 0, "rotate: N must be >= 0 (got %lld)", (long long)N);
  LV_CHECK_ARG(C >= 1, "rotate: C must be >= 1 (got %d)", C);
  LV_CHECK_ARG(H >= 1 && W >= 1, "rotate: H and W must be >= 1 (got %d x %d)", H, W);
  LV_CHECK_ARG((flags & ~LV_ROTATE_DIRECT) == 0, "rotate: unknown flags 0x%x", flags);
  LV_CHECK_ARG((int64_t)H * W <= INT_MAX / 2, "rotate: plane %d x %d too large", H, W);
  LV_CHECK_ARG(N <= INT_MAX / C, "rotate: N*C planes exceed %d (N = %lld, C = %d)", INT_MAX,
               (long long)N, C);
  const int64_t bytes = (int64_t)H * W * 4;
  pl->staged = bytes <= kStagedMaxBytes && !(flags & LV_ROTATE_DIRECT);
  if (pl->staged) {
    pl->grid = N * C;
    pl->lds = (int)bytes;
  } else {
    // sized for four-pixel runs; grid-stride covers the rest (and the one-pixel variant)
    const int64_t runs = N * C * (((int64_t)H * W + 3) / 4);
    pl->grid = img_grid(runs).x;
    pl->lds = 0;
  }
  return LV_OK;
}

}  // namespace lv

using namespace lv;

extern "C" {

int lv_rotate_plan(int64_t N, int C, int H, int W, int flags, int64_t* plan) {
  clear_error();
  LV_CHECK_ARG(plan, "null pointer argument");
  RotPlan pl;
  if (int rc = rotate_plan(N, C, H, W, flags, &pl)) return rc;
  plan[0] = pl.staged;
  plan[1] = N == 0 ? 0 : pl.grid;
  plan[2] = kImgBlock;
  plan[3] = pl.lds;
  return LV_OK;
}

int lv_rotate_bilinear_fwd(const float* img, const float* cs, float* out, int64_t N, int C, int H,
                           int W, int align_corners, int flags, void* stream) {
  clear_error();
  RotPlan pl;
  if (int rc = rotate_plan(N, C, H, W, flags, &pl)) return rc;
  LV_CHECK_ARG(align_corners == 0 || align_corners == 1,
               "rotate: align_corners must be 0 or 1 (got %d)", align_corners);
  if (N == 0) return LV_OK;
  LV_CHECK_ARG(img && cs && out, "null pointer argument");
  RotGeom g;
  g.H = H;
  g.W = W;
  g.cx = (float)(W - 1) * 0.5f;
  g.cy = (float)(H - 1) * 0.5f;
  if (align_corners) {
    g.ax = H > 1 ? (float)(W - 1) / (float)(H - 1) : 0.f;
    g.ay = W > 1 ? (float)(H - 1) / (float)(W - 1) : 0.f;
  } else {
    g.ax = (float)W / (float)H;
    g.ay = (float)H / (float)W;
  }
  const int64_t HW = (int64_t)H * W;
  const bool vec = HW % 4 == 0 && ((uintptr_t)img | (uintptr_t)out) % 16 == 0;
  hipStream_t st = (hipStream_t)stream;
  if (pl.staged) {
    if (vec)
      hipLaunchKernelGGL(rotate_staged_k<4>, dim3((unsigned)pl.grid), dim3(kImgBlock), pl.lds, st,
                         img, cs, out, C, g);
    else
      hipLaunchKernelGGL(rotate_staged_k<1>, dim3((unsigned)pl.grid), dim3(kImgBlock), pl.lds, st,
                         img, cs, out, C, g);
    LV_RETURN_LAUNCH("rotate_staged_k");
  }
  if (vec)
    hipLaunchKernelGGL(rotate_direct_k<4>, dim3((unsigned)pl.grid), dim3(kImgBlock), 0, st, img,
                       cs, out, N * C, C, g);
  else
    hipLaunchKernelGGL(rotate_direct_k<1>, dim3((unsigned)pl.grid), dim3(kImgBlock), 0, st, img,
                       cs, out, N * C, C, g);
  LV_RETURN_LAUNCH("rotate_direct_k");
}

int lv_equivariance_diff_fwd(const float* cs, const float* enc, const float* enc_rot, float* diffs,
                             int64_t n, void* stream) {
  clear_error();
  LV_CHECK_ARG(n >= 0, "n must be >= 0");
  if (n == 0) return LV_OK;
  LV_CHECK_ARG(cs && enc && enc_rot && diffs, "null pointer argument");
  hipLaunchKernelGGL(equiv_diff_fwd_k, img_grid(n), dim3(kImgBlock), 0, (hipStream_t)stream, cs,
                     enc, enc_rot, diffs, n);
  LV_RETURN_LAUNCH("equiv_diff_fwd_k");
}

int lv_equivariance_diff_bwd(const float* cs, const float* enc, const float* enc_rot,
                             const float* gdiffs, float* g_enc, float* g_enc_rot, int64_t n,
                             void* stream) {
  clear_error();
  LV_CHECK_ARG(n >= 0, "n must be >= 0");
  if (n == 0) return LV_OK;
  LV_CHECK_ARG(cs && enc && enc_rot && gdiffs && g_enc && g_enc_rot, "null pointer argument");
  hipLaunchKernelGGL(equiv_diff_bwd_k, img_grid(n), dim3(kImgBlock), 0, (hipStream_t)stream, cs,
                     enc, enc_rot, gdiffs, g_enc, g_enc_rot, n);
  LV_RETURN_LAUNCH("equiv_diff_bwd_k");
}

static int pair_check(int64_t rows, int D) {
  LV_CHECK_ARG(rows >= 0, "pair_sqdist: rows must be >= 0 (got %lld)", (long long)rows);
  LV_CHECK_ARG(rows % 2 == 0, "pair_sqdist: rows must be even, adjacent rows pair (got %lld)",
               (long long)rows);
  LV_CHECK_ARG(D >= 1, "pair_sqdist: D must be >= 1 (got %d)", D);
  return LV_OK;
}

int lv_pair_sqdist_fwd(const float* enc, float* diffs, int64_t rows, int D, void* stream) {
  clear_error();
  if (int rc = pair_check(rows, D)) return rc;
  if (rows == 0) return LV_OK;
  LV_CHECK_ARG(enc && diffs, "null pointer argument");
  hipLaunchKernelGGL(pair_sqdist_fwd_k, img_grid(rows / 2), dim3(kImgBlock), 0,
                     (hipStream_t)stream, enc, diffs, rows / 2, D);
  LV_RETURN_LAUNCH("pair_sqdist_fwd_k");
}

int lv_pair_sqdist_bwd(const float* enc, const float* gdiffs, float* g_enc, int64_t rows, int D,
                       void* stream) {
  clear_error();
  if (int rc = pair_check(rows, D)) return rc;
  if (rows == 0) return LV_OK;
  LV_CHECK_ARG(enc && gdiffs && g_enc, "null pointer argument");
  hipLaunchKernelGGL(pair_sqdist_bwd_k, img_grid(rows * D), dim3(kImgBlock), 0,
                     (hipStream_t)stream, enc, gdiffs, g_enc, rows / 2, D);
  LV_RETURN_LAUNCH("pair_sqdist_bwd_k");
}

}  // extern "C"
