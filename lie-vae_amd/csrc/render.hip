// Sphere-cube renderer: poses in, images out (the data the reference renders with Blender
// from cube.blend; here the scene is our own).
//   render_k<RUN>   one thread traces the S x S rays of each of RUN consecutive pixels of one
//                   image once and writes every channel plane from that trace.
// Scene (object frame fixed, the pose R is the camera frame):
//   camera     o = 5 R[:,2], looking along its own -z with +y up; pinhole of half-width 0.4 at
//              unit distance; sub-sample (a, b) of pixel (i, j): kx = j + (b + .5)/S,
//              ky = i + (a + .5)/S, u = (kx/size - .5) .8, v = (.5 - ky/size) .8,
//              d = R (u, v, -1), unnormalised;
//   cube       [-1,1]^3 by slabs, one albedo per face; sphere: centre (0,0,1), radius 0.6,
//              discriminant as r^2 - |oc - (oc.d/d.d) d|^2, near root only;
//   shading    albedo (0.3 + 0.7 max(0, n.l)), l = (1,2,3)/sqrt(14); nearest hit wins,
//              background 0; a pixel is the mean of its sub-samples added row by row.
// Forward only (the image is piecewise constant in the pose at edges).  No memory is indexed
// by a computed value, so no R -- finite or not -- can make the kernel read or write out of
// bounds; every output is finite (n.l is clamped to [0, 1], a hit test that sees a NaN fails).
// Built with -ffp-contract=off: the one-pixel and four-pixel variants run the same
// arithmetic and agree bit for bit.
#include <climits>
#include <cmath>

#include "lv_common.h"

namespace lv {

constexpr int kRenderBlock = 256;
constexpr int64_t kRenderMaxGrid = 65536;  // grid-stride over tiles beyond
constexpr int kRenderMaxSize = 1024;

struct Rgb {
  float r, g, b;
};

// Face f = 2 axis + (0: +, 1: -): albedo times the face's constant shade
// 0.3 + 0.7 max(0, +-l_axis), l = (1, 2, 3) / sqrt(14).
constexpr double kInvSqrt14 = 0.2672612419124244;
constexpr double face_shade(int f) {
  const double nl = ((f & 1) ? -1.0 : 1.0) * (double)(f / 2 + 1) * kInvSqrt14;
  return 0.3 + 0.7 * (nl > 0.0 ? nl : 0.0);
}
constexpr double kFaceAlbedo[6][3] = {{.9, .1, .1}, {.1, .8, .8}, {.1, .8, .1},
                                      {.8, .1, .8}, {.1, .1, .9}, {.9, .9, .1}};
#define LV_FACE_RGB(f)                                                              \
  Rgb {                                                                             \
    (float)(kFaceAlbedo[f][0] * face_shade(f)), (float)(kFaceAlbedo[f][1] * face_shade(f)), \
        (float)(kFaceAlbedo[f][2] * face_shade(f))                                  \
  }

// One slab of the cube along an axis: the ray's parameter interval inside |x| <= 1.  A
// component that is zero (or so small that its reciprocal overflows) never meets 0 * inf:
// the ray is parallel to the slab and is inside it for all t or for none.
__device__ __forceinline__ void slab(float o, float d, float& tn, float& tf) {
  const float inv = 1.f / d;
  if (d == 0.f || isinf(inv)) {
    const bool inside = fabsf(o) <= 1.f;
    tn = inside ? -INFINITY : INFINITY;
    tf = inside ? INFINITY : -INFINITY;
  } else {
    const float t1 = (-1.f - o) * inv, t2 = (1.f - o) * inv;
    tn = fminf(t1, t2);
    tf = fmaxf(t1, t2);
  }
}

// Colour seen along the ray o + t d, d = u X + v Y - Z (X, Y, Z the columns of R).
__device__ __forceinline__ Rgb trace(const float R[9], const float o[3], float u, float v) {
  float d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = (u * R[3 * k] + v * R[3 * k + 1]) - R[3 * k + 2];

  // ---- cube
  float tn[3], tf[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) slab(o[k], d[k], tn[k], tf[k]);
  float t_in = tn[0], d_ax = d[0];
  int axis = 0;
  if (tn[1] > t_in) { t_in = tn[1]; d_ax = d[1]; axis = 1; }
  if (tn[2] > t_in) { t_in = tn[2]; d_ax = d[2]; axis = 2; }
  const float t_out = fminf(fminf(tf[0], tf[1]), tf[2]);
  const bool cube = t_in <= t_out && t_out > 0.f;
  const int face = 2 * axis + (d_ax < 0.f ? 0 : 1);

  // ---- sphere, centre (0, 0, 1), radius 0.6
  const float oc[3] = {o[0], o[1], o[2] - 1.f};
  const float dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  const float od = (oc[0] * d[0] + oc[1] * d[1]) + oc[2] * d[2];
  const float s = od / dd;
  float p[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = oc[k] - s * d[k];
  const float disc = (float)(0.6 * 0.6) - ((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
  const float t_s = -s - sqrtf(disc / dd);
  const bool sphere = disc >= 0.f && t_s > 0.f;

  Rgb c = {0.f, 0.f, 0.f};
  if (sphere && (!cube || t_s < t_in)) {
    float nrm[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) nrm[k] = (oc[k] + t_s * d[k]) / 0.6f;
    const float l0 = (float)kInvSqrt14, l1 = (float)(2.0 * kInvSqrt14), l2 = (float)(3.0 * kInvSqrt14);
    float nl = (nrm[0] * l0 + nrm[1] * l1) + nrm[2] * l2;
    nl = fminf(fmaxf(nl, 0.f), 1.f);  // <= 1 up to rounding; keeps an overflowed R finite
    const float shade = 0.3f + 0.7f * nl;
    c.r = c.g = c.b = 0.95f * shade;
  } else if (cube) {
    // selects, not a table in memory: nothing is indexed by a computed value
    c = LV_FACE_RGB(0);
    if (face == 1) c = LV_FACE_RGB(1);
    if (face == 2) c = LV_FACE_RGB(2);
    if (face == 3) c = LV_FACE_RGB(3);
    if (face == 4) c = LV_FACE_RGB(4);
    if (face == 5) c = LV_FACE_RGB(5);
  }
  return c;
}

// Mean colour of pixel (i, j) over its S x S sub-samples, rows of sub-samples first.
__device__ __forceinline__ Rgb pixel(const float R[9], const float o[3], int i, int j, int size,
                                     int S) {
  const float fsize = (float)size, fS = (float)S;
  Rgb acc = {0.f, 0.f, 0.f};
  for (int a = 0; a < S; ++a) {
    const float ky = (float)i + ((float)a + 0.5f) / fS;
    const float v = (0.5f - ky / fsize) * 0.8f;
    for (int b = 0; b < S; ++b) {
      const float kx = (float)j + ((float)b + 0.5f) / fS;
      const float u = (kx / fsize - 0.5f) * 0.8f;
      const Rgb c = trace(R, o, u, v);
      acc.r += c.r;
      acc.g += c.g;
      acc.b += c.b;
    }
  }
  const float cnt = (float)(S * S);
  return Rgb{acc.r / cnt, acc.g / cnt, acc.b / cnt};
}

// A tile is kRenderBlock runs of RUN pixels of ONE image (tiles_per_image tiles cover an
// image; the last may be partly empty), so the tile's R is addressed by block-uniform values
// alone and is read once per tile into uniform registers, never per ray.  Blocks stride over
// the tiles.  RUN = 4 needs size % 4 == 0 (a run stays inside one row, and with a 16-byte
// aligned `out` every run is 16-byte aligned) and stores float4; RUN = 1 has no condition.
template <int RUN>
__global__ __launch_bounds__(kRenderBlock) void render_k(const float* __restrict__ Rs,
                                                         float* __restrict__ out, int64_t tiles,
                                                         int tiles_per_image, int size,
                                                         int channels, int S) {
  const int plane = size * size;  // <= 2^20
  const int runs = plane / RUN;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t n = t / tiles_per_image;
    const int part = (int)(t - n * tiles_per_image);
    float R[9], o[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rs[n * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = 5.f * R[3 * k + 2];
    const int run = part * kRenderBlock + (int)threadIdx.x;
    if (run >= runs) continue;
    const int q = run * RUN;
    const int i = q / size, j = q - i * size;
    Rgb c[RUN];
#pragma unroll
    for (int k = 0; k < RUN; ++k) c[k] = pixel(R, o, i, j + k, size, S);
    float* dst = out + n * channels * plane + q;
    if (channels == 1) {
      float g[RUN];
#pragma unroll
      for (int k = 0; k < RUN; ++k) g[k] = ((c[k].r + c[k].g) + c[k].b) / 3.f;
      if constexpr (RUN == 4) {
        *reinterpret_cast<float4*>(dst) = make_float4(g[0], g[1], g[2], g[3]);
      } else {
        dst[0] = g[0];
      }
    } else {
      if constexpr (RUN == 4) {
        *reinterpret_cast<float4*>(dst) = make_float4(c[0].r, c[1].r, c[2].r, c[3].r);
        *reinterpret_cast<float4*>(dst + plane) = make_float4(c[0].g, c[1].g, c[2].g, c[3].g);
        *reinterpret_cast<float4*>(dst + 2 * plane) = make_float4(c[0].b, c[1].b, c[2].b, c[3].b);
      } else {
        dst[0] = c[0].r;
        dst[plane] = c[0].g;
        dst[2 * plane] = c[0].b;
      }
    }
  }
}

struct RenderPlan {
  int wide;
  int64_t tiles, grid;
  int tiles_per_image;
};

// Shape checks and the dispatch shared by lv_render_spherecube_fwd and lv_render_plan.  The
// wide path is planned from the shape alone; the launch falls back to one-pixel runs when
// `out` is not 16-byte aligned (then the grid is the scalar plan's).
int render_plan(int64_t n, int size, int channels, int samples, int flags, RenderPlan* pl) {
  LV_CHECK_ARG(n >= 0, "render: n must be >= 0 (got %lld)", (long long)n);
  LV_CHECK_ARG(size >= 1 && size <= kRenderMaxSize, "render: size must be in 1..%d (got %d)",
               kRenderMaxSize, size);
  LV_CHECK_ARG(channels == 1 || channels == 3, "render: channels must be 1 or 3 (got %d)",
               channels);
  LV_CHECK_ARG(samples >= 1 && samples <= 4, "render: samples must be in 1..4 (got %d)", samples);
  LV_CHECK_ARG((flags & ~LV_RENDER_SCALAR) == 0, "render: unknown flags 0x%x", flags);
  // the kernel's indices (elements of out, tiles) are int64 and at most n * channels * size^2
  const int64_t per_image = (int64_t)channels * size * size;
  LV_CHECK_ARG(n <= INT64_MAX / 4 / per_image,
               "render: n * channels * size^2 exceeds the index range (n = %lld, %d x %d x %d)",
               (long long)n, channels, size, size);
  pl->wide = size % 4 == 0 && !(flags & LV_RENDER_SCALAR);
  const int runs = size * size / (pl->wide ? 4 : 1);
  pl->tiles_per_image = (runs + kRenderBlock - 1) / kRenderBlock;
  pl->tiles = n * pl->tiles_per_image;
  pl->grid = pl->tiles > kRenderMaxGrid ? kRenderMaxGrid : pl->tiles;
  return LV_OK;
}

}  // namespace lv

using namespace lv;

extern "C" {

int lv_render_plan(int64_t n, int size, int channels, int samples, int flags, int64_t* plan) {
  clear_error();
  LV_CHECK_ARG(plan, "null pointer argument");
  RenderPlan pl;
  if (int rc = render_plan(n, size, channels, samples, flags, &pl)) return rc;
  plan[0] = pl.wide;
  plan[1] = pl.grid;
  plan[2] = kRenderBlock;
  plan[3] = 0;  // R travels in uniform registers
  return LV_OK;
}

int lv_render_spherecube_fwd(const float* R, float* out, int64_t n, int size, int channels,
                             int samples, int flags, void* stream) {
  clear_error();
  RenderPlan pl;
  if (int rc = render_plan(n, size, channels, samples, flags, &pl)) return rc;
  if (n == 0) return LV_OK;
  LV_CHECK_ARG(R && out, "null pointer argument");
  if (pl.wide && (uintptr_t)out % 16 != 0)
    if (int rc = render_plan(n, size, channels, samples, flags | LV_RENDER_SCALAR, &pl)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (pl.wide)
    hipLaunchKernelGGL(render_k<4>, dim3((unsigned)pl.grid), dim3(kRenderBlock), 0, st, R, out,
                       pl.tiles, pl.tiles_per_image, size, channels, samples);
  else
    hipLaunchKernelGGL(render_k<1>, dim3((unsigned)pl.grid), dim3(kRenderBlock), 0, st, R, out,
                       pl.tiles, pl.tiles_per_image, size, channels, samples);
  LV_RETURN_LAUNCH("render_k");
}

}  // extern "C"
