// von Mises-Fisher latent on S^3 (reparameterize.py:58-97, latent modes vmf / vmfq): the
// rejection sampler with its pathwise backward, KL(vMF || uniform) and the log-density.
// Written from the published definitions (Davidson et al. 2018; Ulrich 1984 / Wood 1994 for
// the sampler), m = 4 only.  One thread per sample, or per datum where a sum over the samples
// of a datum is formed (ascending s, no atomics).  DESIGN.md §4.6 has the forms.
#include <cmath>

#include "lv_common.h"
#include "pointwise_launch.h"

namespace lv {

constexpr int kVmfMaxTrials = 64;
constexpr float kThreeLog3 = 3.295836866004329f;       // 3 ln 3
constexpr double kLogAreaS3 = 2.9826069522587457;     // ln(2 pi^2)
constexpr double kTwoLogTwoPi = 3.6757541328186907;    // 2 ln(2 pi)
constexpr double kBesselCrossover = 20.0;
constexpr int kSeriesTerms = 64;  // ascending series below the crossover: term 64 < 1e-60 of the sum
constexpr int kHankelTerms = 24;  // asymptotic series above it: term 24 < 1e-14 at kappa = 20

// Wood's constants for m - 1 = 3.  b in the form that does not cancel at large kappa.
__device__ __forceinline__ void vmf_constants(float k, float& a, float& b, float& c, float& d) {
  c = sqrtf(4.f * k * k + 9.f);
  b = 3.f / (2.f * k + c);
  a = (3.f + 2.f * k + c) / 4.f;
  d = 4.f * a * b / (1.f + b) - kThreeLog3;
}

// eps = (1 + x) / 2 ~ Beta(3/2, 3/2) and 1 - eps, x = g0 / |g|, neither by subtraction.
__device__ __forceinline__ void vmf_proposal(const float g[4], float& e, float& eb) {
  const float s = g[1] * g[1] + g[2] * g[2] + g[3] * g[3];
  const float n = sqrtf(s + g[0] * g[0]);
  const float ag = fabsf(g[0]);
  const float small = s / (n * (n + ag));  // 1 - |x|
  const float big = 1.f + ag / n;          // 1 + |x|
  const bool pos = g[0] > 0.f;
  e = 0.5f * (pos ? big : small);
  eb = 0.5f * (pos ? small : big);
}

// x' = (w, sqrt(1 - w^2) v), v the normalised tangent normals.
__device__ __forceinline__ void vmf_point(float b, float e, float eb, const float tn[3], float& w,
                                          float& r, float v[3]) {
  const float D = eb + b * e;
  w = (eb - b * e) / D;
  r = 2.f * sqrtf(b * e * eb) / D;
  const float nn = sqrtf(tn[0] * tn[0] + tn[1] * tn[1] + tn[2] * tn[2]);
#pragma unroll
  for (int j = 0; j < 3; ++j) v[j] = tn[j] / nn;
}

// The reflection that takes e1 to sgn * mu: u = e1 - sgn * mu with sgn = +1 for mu[0] <= 0 and
// -1 otherwise, so u.u >= 2 on unit mu; the map is z = sgn * (x - 2 u (u.x) / (u.u)).
__device__ __forceinline__ float vmf_axis(const float mu[4], float u[4]) {
  const float sgn = mu[0] <= 0.f ? 1.f : -1.f;
  u[0] = 1.f - sgn * mu[0];
#pragma unroll
  for (int j = 1; j < 4; ++j) u[j] = -sgn * mu[j];
  return sgn;
}
__device__ __forceinline__ float dot4(const float a[4], const float b[4]) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
}

__global__ void vmf_sample_fwd_k(const float* mu, const float* kappa, const float* noise, float* z,
                                 int32_t* accepted, int64_t ns, int64_t B, int trials) {
  const int64_t W = 6 * (int64_t)trials + 3;
  LV_FOR_EACH(i, ns * B) {
    const int64_t bi = i % B;
    const float* row = noise + i * W;
    float a, b, c, d;
    vmf_constants(kappa[bi], a, b, c, d);
    float e = 0.f, eb = 0.f;
    int acc = trials;  // none accepted: the last proposal stands
    for (int t = 0; t < trials; ++t) {
      float g[4];
      ld(row + 6 * t, g);
      const float h0 = row[6 * t + 4], h1 = row[6 * t + 5];
      vmf_proposal(g, e, eb);
      const float tt = 2.f * a * b / (eb + b * e);
      const float lhs = 3.f * logf(tt) - tt + d;
      const float rhs = -0.5f * (h0 * h0 + h1 * h1);  // ln U as minus an Exp(1) draw
      if (lhs >= rhs) {
        acc = t;
        break;
      }
    }
    float tn[3], v[3], w, r, m[4], u[4];
    ld(row + 6 * trials, tn);
    vmf_point(b, e, eb, tn, w, r, v);
    const float x[4] = {w, r * v[0], r * v[1], r * v[2]};
    ld(mu + bi * 4, m);
    const float sgn = vmf_axis(m, u);
    const float f = 2.f * dot4(u, x) / dot4(u, u);
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = sgn * (x[j] - f * u[j]);
    st(z + i * 4, o);
    accepted[i] = acc;
  }
}

// Pathwise gradient with the accepted proposal held fixed: through b(kappa) into (w, r) and
// through u into the reflection.  With G the gradient at x', the kappa term of a sample is
// -(r / c) (-r G0 + w G.v): dw/db = -r^2 / (2b), dr/db = r w / (2b), db/dkappa = -2b / c.
__global__ void vmf_sample_bwd_k(const float* mu, const float* kappa, const float* noise,
                                 const int32_t* accepted, const float* gz, float* gmu,
                                 float* gkappa, int64_t ns, int64_t B, int trials) {
  const int64_t W = 6 * (int64_t)trials + 3;
  LV_FOR_EACH(bi, B) {
    float a, b, c, d, m[4], u[4];
    vmf_constants(kappa[bi], a, b, c, d);
    ld(mu + bi * 4, m);
    const float sgn = vmf_axis(m, u);
    const float q = dot4(u, u);
    float gm[4] = {0.f, 0.f, 0.f, 0.f}, gk = 0.f;
    for (int64_t s = 0; s < ns; ++s) {
      const int64_t i = s * B + bi;
      const float* row = noise + i * W;
      int t = accepted[i];
      t = t < 0 ? 0 : (t >= trials ? trials - 1 : t);  // the fallback used the last proposal
      float g4[4], tn[3], v[3], e, eb, w, r, g[4];
      ld(row + 6 * t, g4);
      ld(row + 6 * trials, tn);
      vmf_proposal(g4, e, eb);
      vmf_point(b, e, eb, tn, w, r, v);
      const float x[4] = {w, r * v[0], r * v[1], r * v[2]};
      ld(gz + i * 4, g);
#pragma unroll
      for (int j = 0; j < 4; ++j) g[j] *= sgn;  // gradient at y = x - 2 u (u.x) / (u.u)
      const float p = dot4(u, x), ug = dot4(u, g);
      // G = g - 2 u (u.g) / q
      const float fg = 2.f * ug / q;
      const float G0 = g[0] - fg * u[0];
      const float Gv = (g[1] - fg * u[1]) * v[0] + (g[2] - fg * u[2]) * v[1] + (g[3] - fg * u[3]) * v[2];
      gk += -(r / c) * (w * Gv - r * G0);
      // dL/du = -2 (g p / q + x (u.g) / q - 2 u p (u.g) / q^2); u = e1 - sgn mu
      const float pq = p / q, uq = ug / q, cu = 2.f * pq * uq;
#pragma unroll
      for (int j = 0; j < 4; ++j) gm[j] += sgn * 2.f * (g[j] * pq + x[j] * uq - cu * u[j]);
    }
    st(gmu + bi * 4, gm);
    gkappa[bi] = gk;
  }
}

// ln(I_1(k) e^{-k}) and A = I_2(k) / I_1(k) in fp64: the ascending series (all terms positive)
// below the crossover, Hankel's asymptotic series above it, fixed term counts.
__device__ __forceinline__ void vmf_bessel(double k, double& ln_i1s, double& A) {
  if (k < kBesselCrossover) {
    const double q = 0.25 * k * k;
    double t1 = 1.0, s1 = 1.0, t2 = 0.5, s2 = 0.5;  // 1 / (0! 1!), 1 / (0! 2!)
    for (int j = 1; j < kSeriesTerms; ++j) {
      t1 *= q / ((double)j * (j + 1));
      t2 *= q / ((double)j * (j + 2));
      s1 += t1;
      s2 += t2;
    }
    ln_i1s = log(0.5 * k * s1) - k;
    A = 0.5 * k * s2 / s1;
  } else {
    const double r8 = 1.0 / (8.0 * k);
    double t1 = 1.0, s1 = 1.0, t2 = 1.0, s2 = 1.0;
    for (int j = 1; j < kHankelTerms; ++j) {
      const double o = (2.0 * j - 1.0) * (2.0 * j - 1.0);
      t1 *= -(4.0 - o) * r8 / j;
      t2 *= -(16.0 - o) * r8 / j;
      s1 += t1;
      s2 += t2;
    }
    ln_i1s = log(s1) - 0.5 * log(6.283185307179586 * k);
    A = s2 / s1;
  }
}
// ln C + kappa, C = kappa / ((2 pi)^2 I_1(kappa))
__device__ __forceinline__ double vmf_log_norm_shifted(double k, double ln_i1s) {
  return log(k) - kTwoLogTwoPi - ln_i1s;
}

// KL(vMF(mu, kappa) || U(S^3)) = kappa A + ln C + ln(2 pi^2), as -kappa (1 - A) + (ln C + kappa).
__global__ void vmf_kl_fwd_k(const float* kappa, float* kl, int64_t B) {
  LV_FOR_EACH(i, B) {
    const double k = (double)kappa[i];
    double l, A;
    vmf_bessel(k, l, A);
    kl[i] = (float)(-k * (1.0 - A) + vmf_log_norm_shifted(k, l) + kLogAreaS3);
  }
}
// dKL/dkappa = kappa A', A' = 1 - A^2 - 3 A / kappa
__global__ void vmf_kl_bwd_k(const float* kappa, const float* gkl, float* gkappa, int64_t B) {
  LV_FOR_EACH(i, B) {
    const double k = (double)kappa[i];
    double l, A;
    vmf_bessel(k, l, A);
    gkappa[i] = (float)((double)gkl[i] * k * (1.0 - A * A - 3.0 * A / k));
  }
}

__device__ __forceinline__ double vmf_sqdist(const float z[4], const float m[4]) {
  double d2 = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double t = (double)z[j] - (double)m[j];
    d2 += t * t;
  }
  return d2;
}

// log q(z) = ln C + kappa mu.z = (ln C + kappa) - kappa |z - mu|^2 / 2
__global__ void vmf_log_prob_fwd_k(const float* mu, const float* kappa, const float* z, float* out,
                                   int64_t ns, int64_t B) {
  LV_FOR_EACH(i, ns * B) {
    const int64_t bi = i % B;
    const double k = (double)kappa[bi];
    double l, A;
    vmf_bessel(k, l, A);
    float zz[4], m[4];
    ld(z + i * 4, zz);
    ld(mu + bi * 4, m);
    out[i] = (float)(vmf_log_norm_shifted(k, l) - 0.5 * k * vmf_sqdist(zz, m));
  }
}
// gz = -g kappa (z - mu); gmu = sum_s g kappa (z - mu); gkappa = sum_s g ((1 - A) - |z - mu|^2 / 2)
__global__ void vmf_log_prob_bwd_k(const float* mu, const float* kappa, const float* z,
                                   const float* gout, float* gmu, float* gkappa, float* gz,
                                   int64_t ns, int64_t B) {
  LV_FOR_EACH(bi, B) {
    const float kf = kappa[bi];
    double l, A;
    vmf_bessel((double)kf, l, A);
    float m[4], gm[4] = {0.f, 0.f, 0.f, 0.f};
    ld(mu + bi * 4, m);
    double gk = 0.0;
    for (int64_t s = 0; s < ns; ++s) {
      const int64_t i = s * B + bi;
      float zz[4], o[4];
      ld(z + i * 4, zz);
      const float g = gout[i];
      gk += (double)g * ((1.0 - A) - 0.5 * vmf_sqdist(zz, m));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float t = g * kf * (zz[j] - m[j]);
        gm[j] += t;
        o[j] = -t;
      }
      st(gz + i * 4, o);
    }
    st(gmu + bi * 4, gm);
    gkappa[bi] = (float)gk;
  }
}

}  // namespace lv

using namespace lv;

#define LV_VMF_SIZES() LV_CHECK_ARG(ns >= 0 && B >= 0, "ns and B must be >= 0 (got %lld, %lld)", \
                                    (long long)ns, (long long)B)
#define LV_VMF_TRIALS()                                                                     \
  LV_CHECK_ARG(trials >= 1 && trials <= kVmfMaxTrials, "trials must be in [1, %d] (got %d)", \
               kVmfMaxTrials, trials)
#define LV_VMF_LAUNCH(kern, n, ...)                                                           \
  do {                                                                                        \
    hipLaunchKernelGGL(kern, grid_for(n), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); \
    LV_RETURN_LAUNCH(#kern);                                                                  \
  } while (0)

extern "C" {

int lv_vmf_sample_fwd(const float* mu, const float* kappa, const float* noise, float* z,
                      int32_t* accepted, int64_t ns, int64_t B, int trials, void* stream) {
  clear_error();
  LV_VMF_SIZES();
  LV_VMF_TRIALS();
  if (ns == 0 || B == 0) return LV_OK;
  LV_CHECK_ARG(mu && kappa && noise && z && accepted, "null pointer argument");
  LV_VMF_LAUNCH(vmf_sample_fwd_k, ns * B, mu, kappa, noise, z, accepted, ns, B, trials);
}

int lv_vmf_sample_bwd(const float* mu, const float* kappa, const float* noise,
                      const int32_t* accepted, const float* gz, float* gmu, float* gkappa,
                      int64_t ns, int64_t B, int trials, void* stream) {
  clear_error();
  LV_VMF_SIZES();
  LV_VMF_TRIALS();
  if (ns == 0 || B == 0) return LV_OK;
  LV_CHECK_ARG(mu && kappa && noise && accepted && gz && gmu && gkappa, "null pointer argument");
  LV_VMF_LAUNCH(vmf_sample_bwd_k, B, mu, kappa, noise, accepted, gz, gmu, gkappa, ns, B, trials);
}

int lv_vmf_kl_fwd(const float* kappa, float* kl, int64_t B, void* stream) {
  clear_error();
  LV_CHECK_ARG(B >= 0, "B must be >= 0 (got %lld)", (long long)B);
  if (B == 0) return LV_OK;
  LV_CHECK_ARG(kappa && kl, "null pointer argument");
  LV_VMF_LAUNCH(vmf_kl_fwd_k, B, kappa, kl, B);
}

int lv_vmf_kl_bwd(const float* kappa, const float* gkl, float* gkappa, int64_t B, void* stream) {
  clear_error();
  LV_CHECK_ARG(B >= 0, "B must be >= 0 (got %lld)", (long long)B);
  if (B == 0) return LV_OK;
  LV_CHECK_ARG(kappa && gkl && gkappa, "null pointer argument");
  LV_VMF_LAUNCH(vmf_kl_bwd_k, B, kappa, gkl, gkappa, B);
}

int lv_vmf_log_prob_fwd(const float* mu, const float* kappa, const float* z, float* out,
                        int64_t ns, int64_t B, void* stream) {
  clear_error();
  LV_VMF_SIZES();
  if (ns == 0 || B == 0) return LV_OK;
  LV_CHECK_ARG(mu && kappa && z && out, "null pointer argument");
  LV_VMF_LAUNCH(vmf_log_prob_fwd_k, ns * B, mu, kappa, z, out, ns, B);
}

int lv_vmf_log_prob_bwd(const float* mu, const float* kappa, const float* z, const float* gout,
                        float* gmu, float* gkappa, float* gz, int64_t ns, int64_t B, void* stream) {
  clear_error();
  LV_VMF_SIZES();
  if (ns == 0 || B == 0) return LV_OK;
  LV_CHECK_ARG(mu && kappa && z && gout && gmu && gkappa && gz, "null pointer argument");
  LV_VMF_LAUNCH(vmf_log_prob_bwd_k, B, mu, kappa, z, gout, gmu, gkappa, gz, ns, B);
}

}  // extern "C"
