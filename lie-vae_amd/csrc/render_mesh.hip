// Triangle-mesh renderer: poses and a packed set of meshes in, images out.
//   mesh_pack_k        one thread turns one indexed triangle into a 16-float record
//                      (v0, e1, e2, lit front colour, lit back colour, 0).
//   render_mesh_k<RUN> one thread traces the S x S rays of each of RUN consecutive pixels of
//                      one image, one ray at a time, each ray over all triangles of the image's
//                      mesh in index order, and writes every channel plane from that trace.
// The scene conventions are render.hip's, so the two renderers are interchangeable: the pose R
// is the camera frame, o = 5 R[:,2], d = (u X + v Y) - Z with the same sub-sample positions,
// light l = (1,2,3)/sqrt(14) in the object frame, ambient 0.3 + Lambert 0.7, flat shading,
// background 0, a pixel the mean of its sub-samples added row by row.  Meshes are two-sided:
// nothing is culled by winding, a triangle seen from behind shows its back colour.
// Intersection (Moeller-Trumbore, every dot product as (a0 b0 + a1 b1) + a2 b2):
//   p = d x e2, det = p.e1, inv = 1/det, s = o - v0, u = (s.p) inv, q = s x e1,
//   v = (d.q) inv, t = (q.e2) inv; hit: det != 0, u >= 0, v >= 0, u + v <= 1, t > 0, t < best.
// A comparison that sees a NaN fails and the colours of a record are in [0, 1] by
// construction, so every R and every vertex, finite or not, gives a finite image in [0, 1].
// Only two loads are addressed by a loaded value: ranges[mesh_id] (the id is checked against
// [0, K) first) and the records of that range (the range is checked against the record count
// in the kernel, with block-uniform integer compares).  Forward only, no atomics in the
// renderer, no barrier.  Built with -ffp-contract=off: tests/mesh_ref.py follows the arithmetic
// operation for operation, and the one-pixel and four-pixel variants agree bit for bit.
#include <climits>
#include <cmath>

#include "lv_common.h"

namespace lv {

constexpr int kMeshBlock = 256;
constexpr int64_t kMeshMaxGrid = 65536;  // grid-stride over tiles beyond
constexpr int kMeshMaxSize = 1024;
constexpr int kRecFloats = 16;
constexpr double kMeshInvSqrt14 = 0.2672612419124244;

struct Col {
  float r, g, b;
};

__device__ __forceinline__ float dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
  return (a0 * b0 + a1 * b1) + a2 * b2;
}

// ------------------------------------------------------------------ packing
// faces are checked before they address anything: a triangle with an index outside [0, V)
// becomes an all-zero record (det == 0 for every ray: never hit) and is counted in *bad.
__global__ __launch_bounds__(kMeshBlock) void mesh_pack_k(const float* __restrict__ verts, int V,
                                                          const int* __restrict__ faces,
                                                          const float* __restrict__ albedo, int T,
                                                          float* __restrict__ rec,
                                                          int* __restrict__ bad) {
  const int t = blockIdx.x * kMeshBlock + (int)threadIdx.x;
  if (t >= T) return;
  float4* dst = reinterpret_cast<float4*>(rec + (int64_t)t * kRecFloats);
  const int i0 = faces[3 * (int64_t)t], i1 = faces[3 * (int64_t)t + 1], i2 = faces[3 * (int64_t)t + 2];
  if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    dst[0] = z;
    dst[1] = z;
    dst[2] = z;
    dst[3] = z;
    atomicAdd(bad, 1);
    return;
  }
  float v0[3], e1[3], e2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    v0[k] = verts[3 * (int64_t)i0 + k];
    e1[k] = verts[3 * (int64_t)i1 + k] - v0[k];
    e2[k] = verts[3 * (int64_t)i2 + k] - v0[k];
  }
  const float c0 = e1[1] * e2[2] - e1[2] * e2[1];
  const float c1 = e1[2] * e2[0] - e1[0] * e2[2];
  const float c2 = e1[0] * e2[1] - e1[1] * e2[0];
  const float len = sqrtf(dot3(c0, c1, c2, c0, c1, c2));
  const float l0 = (float)kMeshInvSqrt14, l1 = (float)(2.0 * kMeshInvSqrt14),
              l2 = (float)(3.0 * kMeshInvSqrt14);
  const float nl = dot3(c0 / len, c1 / len, c2 / len, l0, l1, l2);
  // fmaxf / fminf drop a NaN: n.l in [0, 1] whatever the vertices hold
  const float nf = fminf(fmaxf(nl, 0.f), 1.f), nb = fminf(fmaxf(-nl, 0.f), 1.f);
  const bool solid = len > 0.f && len < INFINITY;  // false without area, for a NaN, on overflow
  float f[3], b[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float a = fminf(fmaxf(albedo[3 * (int64_t)t + k], 0.f), 1.f);
    f[k] = solid ? a * (0.3f + 0.7f * nf) : 0.f;
    b[k] = solid ? a * (0.3f + 0.7f * nb) : 0.f;
  }
  // a triangle that is not solid gets zero edges too: det == 0 exactly, never hit
  dst[0] = make_float4(v0[0], v0[1], v0[2], solid ? e1[0] : 0.f);
  dst[1] = make_float4(solid ? e1[1] : 0.f, solid ? e1[2] : 0.f, solid ? e2[0] : 0.f,
                       solid ? e2[1] : 0.f);
  dst[2] = make_float4(solid ? e2[2] : 0.f, f[0], f[1], f[2]);
  dst[3] = make_float4(b[0], b[1], b[2], 0.f);
}

// ------------------------------------------------------------------ tracing
// Colour seen along o + t d over the records [start, start + count).  The record address is
// block-uniform (start, count and k are), so the 16 floats arrive by scalar loads and stay in
// scalar registers; the lanes differ only in d.
__device__ __forceinline__ Col trace_mesh(const float R[9], const float o[3], float u, float v,
                                          const float4* __restrict__ rec, int start, int count) {
  float d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = (u * R[3 * k] + v * R[3 * k + 1]) - R[3 * k + 2];
  float best = INFINITY;
  Col c = {0.f, 0.f, 0.f};
  for (int k = 0; k < count; ++k) {
    const float4* r = rec + (int64_t)(start + k) * 4;
    const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    const float v0[3] = {r0.x, r0.y, r0.z}, e1[3] = {r0.w, r1.x, r1.y}, e2[3] = {r1.z, r1.w, r2.x};
    const float p0 = d[1] * e2[2] - d[2] * e2[1];
    const float p1 = d[2] * e2[0] - d[0] * e2[2];
    const float p2 = d[0] * e2[1] - d[1] * e2[0];
    const float det = dot3(p0, p1, p2, e1[0], e1[1], e1[2]);
    const float inv = 1.f / det;
    const float s0 = o[0] - v0[0], s1 = o[1] - v0[1], s2 = o[2] - v0[2];
    const float uu = dot3(s0, s1, s2, p0, p1, p2) * inv;
    const float q0 = s1 * e1[2] - s2 * e1[1];
    const float q1 = s2 * e1[0] - s0 * e1[2];
    const float q2 = s0 * e1[1] - s1 * e1[0];
    const float vv = dot3(d[0], d[1], d[2], q0, q1, q2) * inv;
    const float t = dot3(q0, q1, q2, e2[0], e2[1], e2[2]) * inv;
    const bool hit = det != 0.f && uu >= 0.f && vv >= 0.f && uu + vv <= 1.f && t > 0.f && t < best;
    const bool front = det > 0.f;
    best = hit ? t : best;
    c.r = hit ? (front ? r2.y : r3.x) : c.r;
    c.g = hit ? (front ? r2.z : r3.y) : c.g;
    c.b = hit ? (front ? r2.w : r3.z) : c.b;
  }
  return c;
}

// Mean colour of pixel (i, j) over its S x S sub-samples, rows of sub-samples first
// (render.hip's positions and order).
__device__ __forceinline__ Col pixel_mesh(const float R[9], const float o[3], int i, int j,
                                          int size, int S, const float4* __restrict__ rec,
                                          int start, int count) {
  const float fsize = (float)size, fS = (float)S;
  Col acc = {0.f, 0.f, 0.f};
  for (int a = 0; a < S; ++a) {
    const float ky = (float)i + ((float)a + 0.5f) / fS;
    const float v = (0.5f - ky / fsize) * 0.8f;
    for (int b = 0; b < S; ++b) {
      const float kx = (float)j + ((float)b + 0.5f) / fS;
      const float u = (kx / fsize - 0.5f) * 0.8f;
      const Col c = trace_mesh(R, o, u, v, rec, start, count);
      acc.r += c.r;
      acc.g += c.g;
      acc.b += c.b;
    }
  }
  const float cnt = (float)(S * S);
  return Col{acc.r / cnt, acc.g / cnt, acc.b / cnt};
}

// The tiling is render_k's: a tile is kMeshBlock runs of RUN pixels of ONE image, so R, the
// mesh id and the record range are addressed by block-uniform values alone and are read once
// per tile; blocks stride over the tiles.  RUN = 4 needs size % 4 == 0 and a 16-byte aligned
// `out` (float4 stores); RUN = 1 has no condition.
template <int RUN>
__global__ __launch_bounds__(kMeshBlock) void render_mesh_k(
    const float* __restrict__ Rs, const int64_t* __restrict__ mesh_id,
    const float4* __restrict__ rec, const int* __restrict__ ranges, int K, int total,
    float* __restrict__ out, int64_t tiles, int tiles_per_image, int size, int channels, int S) {
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
    // an id outside [0, K) addresses nothing and renders the background; so does a range that
    // leaves [0, total)
    const int64_t id = mesh_id ? mesh_id[n] : 0;
    int start = 0, count = 0;
    if (id >= 0 && id < K) {
      start = ranges[2 * id];
      count = ranges[2 * id + 1];
      if (start < 0 || count < 0 || start > total - count) count = 0;
    }
    const int run = part * kMeshBlock + (int)threadIdx.x;
    if (run >= runs) continue;
    const int q = run * RUN;
    const int i = q / size, j = q - i * size;
    Col c[RUN];
#pragma unroll
    for (int k = 0; k < RUN; ++k) c[k] = pixel_mesh(R, o, i, j + k, size, S, rec, start, count);
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

struct MeshPlan {
  int wide;
  int64_t tiles, grid;
  int tiles_per_image;
};

// Shape checks and the dispatch shared by lv_render_mesh_fwd and lv_render_mesh_plan.  The
// wide path is planned from the shape alone; the launch falls back to one-pixel runs when
// `out` is not 16-byte aligned.
int mesh_plan(int K, int64_t total, int64_t n, int size, int channels, int samples, int flags,
              int64_t max_blocks, MeshPlan* pl) {
  LV_CHECK_ARG(n >= 0, "render_mesh: n must be >= 0 (got %lld)", (long long)n);
  LV_CHECK_ARG(size >= 1 && size <= kMeshMaxSize, "render_mesh: size must be in 1..%d (got %d)",
               kMeshMaxSize, size);
  LV_CHECK_ARG(channels == 1 || channels == 3, "render_mesh: channels must be 1 or 3 (got %d)",
               channels);
  LV_CHECK_ARG(samples >= 1 && samples <= 4, "render_mesh: samples must be in 1..4 (got %d)",
               samples);
  LV_CHECK_ARG(K >= 1, "render_mesh: K must be >= 1 (got %d)", K);
  LV_CHECK_ARG(total >= 0 && total <= INT_MAX,
               "render_mesh: total_records must be in 0..2^31-1 (got %lld)", (long long)total);
  LV_CHECK_ARG((flags & ~LV_MESH_SCALAR) == 0, "render_mesh: unknown flags 0x%x", flags);
  LV_CHECK_ARG(max_blocks >= 0, "render_mesh: max_blocks must be >= 0 (got %lld)",
               (long long)max_blocks);
  const int64_t per_image = (int64_t)channels * size * size;
  LV_CHECK_ARG(n <= INT64_MAX / 4 / per_image,
               "render_mesh: n * channels * size^2 exceeds the index range (n = %lld, %d x %d x %d)",
               (long long)n, channels, size, size);
  pl->wide = size % 4 == 0 && !(flags & LV_MESH_SCALAR);
  const int runs = size * size / (pl->wide ? 4 : 1);
  pl->tiles_per_image = (runs + kMeshBlock - 1) / kMeshBlock;
  pl->tiles = n * pl->tiles_per_image;
  const int64_t cap = max_blocks > 0 && max_blocks < kMeshMaxGrid ? max_blocks : kMeshMaxGrid;
  pl->grid = pl->tiles > cap ? cap : pl->tiles;
  return LV_OK;
}

}  // namespace lv

using namespace lv;

extern "C" {

int lv_mesh_pack(const float* verts, int64_t V, const int32_t* faces, const float* albedo,
                 int64_t T, float* records, int32_t* bad_counter, void* stream) {
  clear_error();
  LV_CHECK_ARG(V >= 0 && V <= INT_MAX / 3, "mesh_pack: V must be in 0..%d (got %lld)", INT_MAX / 3,
               (long long)V);
  LV_CHECK_ARG(T >= 0 && T <= INT_MAX / kRecFloats, "mesh_pack: T must be in 0..%d (got %lld)",
               INT_MAX / kRecFloats, (long long)T);
  if (T == 0) return LV_OK;
  LV_CHECK_ARG(faces && albedo && records && bad_counter && (verts || V == 0),
               "null pointer argument");
  LV_CHECK_ARG((uintptr_t)records % 16 == 0, "mesh_pack: records must be 16-byte aligned");
  const int blocks = (int)((T + kMeshBlock - 1) / kMeshBlock);
  hipLaunchKernelGGL(mesh_pack_k, dim3((unsigned)blocks), dim3(kMeshBlock), 0, (hipStream_t)stream,
                     verts, (int)V, faces, albedo, (int)T, records, bad_counter);
  LV_RETURN_LAUNCH("mesh_pack_k");
}

int lv_render_mesh_plan(const int32_t* host_ranges, int K, int64_t total_records, int64_t n,
                        int size, int channels, int samples, int flags, int64_t max_blocks,
                        int64_t* plan) {
  clear_error();
  LV_CHECK_ARG(plan, "null pointer argument");
  MeshPlan pl;
  if (int rc = mesh_plan(K, total_records, n, size, channels, samples, flags, max_blocks, &pl))
    return rc;
  if (host_ranges)
    for (int k = 0; k < K; ++k) {
      const int64_t start = host_ranges[2 * k], count = host_ranges[2 * k + 1];
      LV_CHECK_ARG(start >= 0 && count >= 0 && start + count <= total_records,
                   "render_mesh: range %d = [%lld, %lld + %lld) leaves the %lld records", k,
                   (long long)start, (long long)start, (long long)count, (long long)total_records);
    }
  plan[0] = pl.wide;
  plan[1] = pl.grid;
  plan[2] = kMeshBlock;
  plan[3] = 0;  // R and the records travel in uniform registers
  return LV_OK;
}

int lv_render_mesh_fwd(const float* R, const int64_t* mesh_id, const float* records,
                       const int32_t* ranges, int K, int64_t total_records, float* out, int64_t n,
                       int size, int channels, int samples, int flags, int64_t max_blocks,
                       void* stream) {
  clear_error();
  MeshPlan pl;
  if (int rc = mesh_plan(K, total_records, n, size, channels, samples, flags, max_blocks, &pl))
    return rc;
  if (n == 0) return LV_OK;
  LV_CHECK_ARG(R && out && ranges && (records || total_records == 0), "null pointer argument");
  LV_CHECK_ARG((uintptr_t)records % 16 == 0, "render_mesh: records must be 16-byte aligned");
  if (pl.wide && (uintptr_t)out % 16 != 0)
    if (int rc = mesh_plan(K, total_records, n, size, channels, samples, flags | LV_MESH_SCALAR,
                           max_blocks, &pl))
      return rc;
  hipStream_t st = (hipStream_t)stream;
  const float4* rec = reinterpret_cast<const float4*>(records);
  if (pl.wide)
    hipLaunchKernelGGL(render_mesh_k<4>, dim3((unsigned)pl.grid), dim3(kMeshBlock), 0, st, R,
                       mesh_id, rec, ranges, K, (int)total_records, out, pl.tiles,
                       pl.tiles_per_image, size, channels, samples);
  else
    hipLaunchKernelGGL(render_mesh_k<1>, dim3((unsigned)pl.grid), dim3(kMeshBlock), 0, st, R,
                       mesh_id, rec, ranges, K, (int)total_records, out, pl.tiles,
                       pl.tiles_per_image, size, channels, samples);
  LV_RETURN_LAUNCH("render_mesh_k");
}

}  // extern "C"
