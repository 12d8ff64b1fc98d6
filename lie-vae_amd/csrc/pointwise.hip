// Per-sample SO(3) conversions and reparameterisation kernels (forward + backward).
// One thread per sample; all state in registers (so3_device.h).  These are
// latency-trivial, byte-bound maps; they exist so the whole latent path runs on the
// GPU through the C ABI rather than as chains of tiny torch ops.
#include <cmath>
#include <cstdarg>
#include <cstring>

#include "lv_common.h"
#include "pointwise_launch.h"
#include "so3_device.h"

namespace lv {

namespace {
thread_local char g_err[512] = {0};
}

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
void clear_error() { g_err[0] = 0; }

// kBlock, grid_for, LV_FOR_EACH, ld / st: pointwise_launch.h (shared with vmf.hip)

template <typename T>
__global__ void so3_exp_fwd_k(const T* v, T* R, int64_t n) {
  LV_FOR_EACH(i, n) {
    T a[3], r[9];
    ld(v + i * 3, a);
    rodrigues_fwd(a, r);
    st(R + i * 9, r);
  }
}
template <typename T>
__global__ void so3_exp_bwd_k(const T* v, const T* gR, T* gv, int64_t n) {
  LV_FOR_EACH(i, n) {
    T a[3], g[9], o[3];
    ld(v + i * 3, a);
    ld(gR + i * 9, g);
    rodrigues_bwd(a, g, o);
    st(gv + i * 3, o);
  }
}

// z[s,b] = mu[b] @ exp(v[s,b])
template <typename T>
__global__ void so3_sample_fwd_k(const T* mu, const T* v, T* z, int64_t ns, int64_t B) {
  LV_FOR_EACH(i, ns * B) {
    const int64_t b = i % B;
    T a[3], r[9], m[9], o[9];
    ld(v + i * 3, a);
    ld(mu + b * 9, m);
    rodrigues_fwd(a, r);
    matmul3(m, r, o);
    st(z + i * 9, o);
  }
}
// gv[s,b] via exp backward of mu^T gz; gmu[b] = sum_s gz R^T (fixed order)
template <typename T>
__global__ void so3_sample_bwd_k(const T* mu, const T* v, const T* gz, T* gmu,
                                 T* gv, int64_t ns, int64_t B) {
  LV_FOR_EACH(b, B) {
    T m[9], acc[9];
    ld(mu + b * 9, m);
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = T(0);
    for (int64_t s = 0; s < ns; ++s) {
      const int64_t i = s * B + b;
      T a[3], r[9], g[9], gr[9], t[9], o[3];
      ld(v + i * 3, a);
      ld(gz + i * 9, g);
      rodrigues_fwd(a, r);
      matmul3_nt(g, r, t);
#pragma unroll
      for (int k = 0; k < 9; ++k) acc[k] += t[k];
      matmul3_tn(m, g, gr);
      rodrigues_bwd(a, gr, o);
      st(gv + i * 3, o);
    }
    st(gmu + b * 9, acc);
  }
}

// Backward of the fused path's prologue, z = mu @ exp(v) (mu optional) -> ZYZ angles, in
// one pass per sample: the composition of so3_sample_fwd/so3_exp_fwd, mat_to_eazyz_bwd
// and so3_sample_bwd/so3_exp_bwd above (same device functions, same operation order)
// without the three launches and the (n,3,3) round trips through memory.  The fp64 entry
// gives bitwise the gradients of the fp64 modular kernels; the fp32 entry runs the same
// fp64 chain on its inputs cast up and rounds once (so3_device.h
// exp_eazyz_vjp_sample_wide: the fp32 chain loses up to ~1e-3 of a sample's gradient near
// beta = 0 / pi), i.e. the fp64 modular kernels' gradients rounded to fp32.
// reparameterize.py:269-273 + vae.py:182 (autograd in the reference).
template <typename T>
__global__ void exp_eazyz_vjp_k(const T* mu, const T* v, const T* ga, T* gmu,
                                T* gv, int64_t n) {
  LV_FOR_EACH(i, n) {
    T a[3], g[3], m[9], gm[9], o[3];
    ld(v + i * 3, a);
    ld(ga + i * 3, g);
    if (mu) ld(mu + i * 9, m);
    // fp32: the chain in fp64, rounded once (exp_eazyz_vjp_sample_wide)
    if constexpr (std::is_same_v<T, float>) exp_eazyz_vjp_sample_wide(a, mu != nullptr, m, g, gm, o);
    else exp_eazyz_vjp_sample(a, mu != nullptr, m, g, gm, o);
    if (mu) st(gmu + i * 9, gm);
    st(gv + i * 3, o);
  }
}

template <typename T>
__global__ void quat_to_mat_fwd_k(const T* q, T* R, int64_t n) {
  LV_FOR_EACH(i, n) {
    T a[4], r[9];
    ld(q + i * 4, a);
    quat_to_mat_fwd(a, r);
    st(R + i * 9, r);
  }
}
template <typename T>
__global__ void quat_to_mat_bwd_k(const T* q, const T* gR, T* gq, int64_t n) {
  LV_FOR_EACH(i, n) {
    T a[4], g[9], o[4];
    ld(q + i * 4, a);
    ld(gR + i * 9, g);
    quat_to_mat_bwd(a, g, o);
    st(gq + i * 4, o);
  }
}

template <typename T>
__global__ void mat_to_quat_fwd_k(const T* R, T* q, int64_t n) {
  LV_FOR_EACH(i, n) {
    T r[9], o[4];
    ld(R + i * 9, r);
    mat_to_quat_fwd(r, o, nullptr);
    st(q + i * 4, o);
  }
}
template <typename T>
__global__ void mat_to_quat_bwd_k(const T* R, const T* gq, T* gR, int64_t n) {
  LV_FOR_EACH(i, n) {
    T r[9], g[4], o[9];
    ld(R + i * 9, r);
    ld(gq + i * 4, g);
    mat_to_quat_bwd(r, g, o);
    st(gR + i * 9, o);
  }
}

template <typename T>
__global__ void quat_to_eazyz_fwd_k(const T* q, T* ang, int64_t n) {
  LV_FOR_EACH(i, n) {
    T a[4], o[3];
    ld(q + i * 4, a);
    quat_to_eazyz_fwd(a, o);
    st(ang + i * 3, o);
  }
}
template <typename T>
__global__ void quat_to_eazyz_bwd_k(const T* q, const T* ga, T* gq, int64_t n) {
  LV_FOR_EACH(i, n) {
    T a[4], g[3], o[4];
    ld(q + i * 4, a);
    ld(ga + i * 3, g);
    quat_to_eazyz_bwd(a, g, o);
    st(gq + i * 4, o);
  }
}

template <typename T>
__global__ void mat_to_eazyz_fwd_k(const T* R, T* ang, int64_t n) {
  LV_FOR_EACH(i, n) {
    T r[9], q[4], o[3];
    ld(R + i * 9, r);
    mat_to_quat_fwd(r, q, nullptr);
    quat_to_eazyz_fwd(q, o);
    st(ang + i * 3, o);
  }
}
template <typename T>
__global__ void mat_to_eazyz_bwd_k(const T* R, const T* ga, T* gR, int64_t n) {
  LV_FOR_EACH(i, n) {
    T r[9], q[4], g[3], gq[4], o[9];
    ld(R + i * 9, r);
    ld(ga + i * 3, g);
    mat_to_quat_fwd(r, q, nullptr);
    quat_to_eazyz_bwd(q, g, gq);
    mat_to_quat_bwd(r, gq, o);
    st(gR + i * 9, o);
  }
}

template <typename T>
__global__ void s2s1_fwd_k(const T* ax, const T* cs, T* R, int64_t n) {
  LV_FOR_EACH(i, n) {
    T a[3], c[2], r[9];
    ld(ax + i * 3, a);
    ld(cs + i * 2, c);
    s2s1_fwd(a, c, r);
    st(R + i * 9, r);
  }
}
template <typename T>
__global__ void s2s1_bwd_k(const T* ax, const T* cs, const T* gR, T* gax,
                           T* gcs, int64_t n) {
  LV_FOR_EACH(i, n) {
    T a[3], c[2], g[9], oa[3], oc[2];
    ld(ax + i * 3, a);
    ld(cs + i * 2, c);
    ld(gR + i * 9, g);
    s2s1_bwd(a, c, g, oa, oc);
    st(gax + i * 3, oa);
    st(gcs + i * 2, oc);
  }
}

__global__ void s2s2_fwd_k(const double* v1, const double* v2, double* R, int64_t n) {
  LV_FOR_EACH(i, n) {
    double a[3], b[3];
    for (int k = 0; k < 3; ++k) { a[k] = v1[i * 3 + k]; b[k] = v2[i * 3 + k]; }
    S2S2State s;
    s2s2_fwd(a, b, s);
    for (int k = 0; k < 3; ++k) {
      R[i * 9 + k] = s.e1[k];
      R[i * 9 + 3 + k] = s.e2[k];
      R[i * 9 + 6 + k] = s.e3[k];
    }
  }
}
__global__ void s2s2_bwd_k(const double* v1, const double* v2, const double* gR, double* g1,
                           double* g2, int64_t n) {
  LV_FOR_EACH(i, n) {
    double a[3], b[3], g[9], o1[3], o2[3];
    for (int k = 0; k < 3; ++k) { a[k] = v1[i * 3 + k]; b[k] = v2[i * 3 + k]; }
    for (int k = 0; k < 9; ++k) g[k] = gR[i * 9 + k];
    s2s2_bwd(a, b, g, o1, o2);
    for (int k = 0; k < 3; ++k) { g1[i * 3 + k] = o1[k]; g2[i * 3 + k] = o2[k]; }
  }
}

// ---------------------------------------------------------------- so(3) log family
// v = log R (so3_device.h so3_log_polar); backward on the tangent space, gR = R hat(u).
template <typename T>
__global__ void so3_log_fwd_k(const T* R, T* v, int64_t n) {
  LV_FOR_EACH(i, n) {
    T r[9];
    ld(R + i * 9, r);
    LogPolar<T> p;
    so3_log_polar(r, p);
    st(v + i * 3, p.v);
  }
}
template <typename T>
__global__ void so3_log_bwd_k(const T* R, const T* gv, T* gR, int64_t n) {
  LV_FOR_EACH(i, n) {
    T r[9], g[3], u[3], o[9];
    ld(R + i * 9, r);
    ld(gv + i * 3, g);
    LogPolar<T> p;
    so3_log_polar(r, p);
    so3_log_tangent(p, g, u);
    mul_hat(r, u, o);
    st(gR + i * 9, o);
  }
}

// v[s,b] = log(mu[b]^T z[s,b]): the inverse of so3_sample_fwd_k
template <typename T>
__global__ void so3_rel_log_fwd_k(const T* mu, const T* z, T* v, int64_t ns, int64_t B) {
  LV_FOR_EACH(i, ns * B) {
    const int64_t b = i % B;
    T m[9], zz[9], q[9];
    ld(mu + b * 9, m);
    ld(z + i * 9, zz);
    matmul3_tn(m, zz, q);
    LogPolar<T> p;
    so3_log_polar(q, p);
    st(v + i * 3, p.v);
  }
}
// gz[s,b] = z hat(u); gmu[b] = sum_s mu hat(-Q u), Q = mu^T z (fixed order, one thread per b)
// (launch bounds: every launch here uses kBlock threads; without them the fp64 twin is held to
// the 128 registers of a 1,024-thread block and spills)
template <typename T>
__global__ void __launch_bounds__(kBlock) so3_rel_log_bwd_k(const T* mu, const T* z, const T* gv, T* gmu, T* gz,
                                  int64_t ns, int64_t B) {
  LV_FOR_EACH(b, B) {
    T m[9], acc[3];
    ld(mu + b * 9, m);
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] = T(0);
    for (int64_t s = 0; s < ns; ++s) {
      const int64_t i = s * B + b;
      T zz[9], q[9], g[3], u[3], o[9];
      ld(z + i * 9, zz);
      ld(gv + i * 3, g);
      matmul3_tn(m, zz, q);
      LogPolar<T> p;
      so3_log_polar(q, p);
      so3_log_tangent(p, g, u);
      mul_hat(zz, u, o);
      st(gz + i * 9, o);
      // mu hat(.) is linear: sum the vectors -Q u, one product with mu at the end
#pragma unroll
      for (int k = 0; k < 3; ++k)
        acc[k] -= (q[k * 3 + 0] * u[0] + q[k * 3 + 1] * u[1]) + q[k * 3 + 2] * u[2];
    }
    T om[9];
    mul_hat(m, acc, om);
    st(gmu + b * 9, om);
  }
}

// theta[i] = rotation angle of A[i]^T B[i]; gB = B hat(gtheta a / 2), gA = -A hat(gtheta a / 2)
template <typename T>
__global__ void so3_angle_fwd_k(const T* A, const T* Bm, T* theta, int64_t n) {
  LV_FOR_EACH(i, n) {
    T a[9], b[9], q[9];
    ld(A + i * 9, a);
    ld(Bm + i * 9, b);
    matmul3_tn(a, b, q);
    LogPolar<T> p;
    so3_log_polar(q, p);
    theta[i] = p.th;
  }
}
template <typename T>
__global__ void so3_angle_bwd_k(const T* A, const T* Bm, const T* gtheta, T* gA, T* gB, int64_t n) {
  LV_FOR_EACH(i, n) {
    T a[9], b[9], q[9], u[3], oa[9], ob[9];
    ld(A + i * 9, a);
    ld(Bm + i * 9, b);
    matmul3_tn(a, b, q);
    LogPolar<T> p;
    so3_log_polar(q, p);
    const T h = T(0.5) * gtheta[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) u[k] = h * p.a[k];
    mul_hat(b, u, ob);
#pragma unroll
    for (int k = 0; k < 3; ++k) u[k] = -u[k];
    mul_hat(a, u, oa);
    st(gA + i * 9, oa);
    st(gB + i * 9, ob);
  }
}

// ---------------------------------------------------------------- N0 + SO(3) density
// softplus(x) = log1p(exp(x)), identity above threshold 20 (torch defaults).
__global__ void softplus_fwd_k(const float* h, float* s, int64_t n) {
  LV_FOR_EACH(i, n) {
    const float x = h[i];
    s[i] = x > 20.f ? x : log1pf(expf(x));
  }
}
__global__ void softplus_bwd_k(const float* h, const float* gs, float* gh, int64_t n) {
  LV_FOR_EACH(i, n) {
    const float x = h[i];
    const float z = expf(x);
    gh[i] = x > 20.f ? gs[i] : gs[i] * z / (z + 1.f);
  }
}
__global__ void n0_sample_fwd_k(const float* sigma, const float* eps, float* v, int64_t ns, int64_t B) {
  LV_FOR_EACH(i, ns * B * 3) {
    const int64_t bj = i % (B * 3);
    v[i] = eps[i] * sigma[bj];
  }
}
__global__ void n0_sample_bwd_k(const float* eps, const float* gv, float* gs, int64_t ns, int64_t B) {
  LV_FOR_EACH(bj, B * 3) {
    float acc = 0.f;
    for (int64_t s = 0; s < ns; ++s) acc += gv[s * B * 3 + bj] * eps[s * B * 3 + bj];
    gs[bj] = acc;
  }
}

// log q(z|x) for z = exp(v): reparameterize.py:233-263 with torch.distributions.Normal
// log_prob (loc 0) and the max-shifted logsumexp of lie_vae/utils.py:4-26.
constexpr float kTwoPi = 6.283185307179586f;
constexpr float kHalfLog2Pi = 0.9189385332046727f;  // log(sqrt(2 pi))

constexpr int kMaxWrap = 64;

// Volume term of wrapped angle thk (reparameterize.py:255-259), both clamps.
__device__ __forceinline__ float logpost_vol(float thk) {
  const float th2 = fmaxf(thk * thk, 1e-3f);
  const float den = fmaxf(2.f - 2.f * cosf(thk), 1e-3f);
  return logf(th2 / den);
}

// One wrapped term l_t of the density (reparameterize.py:240-260), logs of sigma hoisted.
__device__ __forceinline__ float logpost_term(int t, float th, const float u[3],
                                              const float var[3], const float logsig[3]) {
  const float thk = th + (float)t * kTwoPi;
  float lp = 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float x = u[j] * thk;
    const float term = (-(x * x) / (2.f * var[j]) - logsig[j]) - kHalfLog2Pi;
    lp = (j == 0) ? term : lp + term;
  }
  return lp + logpost_vol(thk);
}

// max-shifted logsumexp over t = -k..k (lie_vae/utils.py:4-26), two passes: the largest
// term m and sum_t exp(l_t - m); the value is m + log(sum).
__device__ __forceinline__ void logpost_max_sum(float th, const float u[3], const float var[3],
                                                const float logsig[3], int k, float& m,
                                                float& sum) {
  m = -INFINITY;
  for (int t = -k; t <= k; ++t) m = fmaxf(m, logpost_term(t, th, u, var, logsig));
  sum = 0.f;
  for (int t = -k; t <= k; ++t) sum += expf(logpost_term(t, th, u, var, logsig) - m);
}

// The backward's weight of term t is softmax_t = exp(l_t - m) / sum, as autograd forms it for
// the reference's logsumexp: never exp(l_t - lse).  lse = m + log(sum) is rounded to fp32, so at
// a narrow sigma (|lse| ~ 1e4, half an ulp 5e-4) every weight of the sample, and with it gv
// and gsigma, would be off by up to 5e-4 relative.
//
// The weights see only differences of terms, and the Gaussian part of a term, -q thk^2 / 2 with
// q = sum_j (u_j / sigma_j)^2, reaches 1e3..1e4 at a narrow sigma: its fp32 roundings (and that
// of theta = |v| itself) move a difference by ~1e-4.  Where two terms carry weight with
// opposite slopes (theta near pi: t = 0 and t = -1 at +-pi, slopes -+theta q) that is 1e-4 of
// the whole gradient.  So the backward takes the Gaussian part in fp64 from the fp32 inputs:
// three divisions and a square root per sample, one multiply-add per term, no fp64
// transcendental; -log sigma_j and the constant are common to all t and drop out.  The volume
// part, of order 1, stays fp32.
struct LogpostWide {
  double th, q;  // |v|; sum_j (v_j / sigma_j)^2 / |v|^2
};
__device__ __forceinline__ LogpostWide logpost_wide(const float a[3], const float sg[3]) {
  LogpostWide p;
  const double a0 = a[0], a1 = a[1], a2 = a[2];
  const double r0 = a0 / (double)sg[0], r1 = a1 / (double)sg[1], r2 = a2 / (double)sg[2];
  const double n2 = a0 * a0 + a1 * a1 + a2 * a2;
  p.th = sqrt(n2);
  p.q = (r0 * r0 + r1 * r1 + r2 * r2) / n2;
  return p;
}
// l_t up to the terms common to all t; th is the fp32 angle the volume term is taken at.
__device__ __forceinline__ double logpost_term_wide(int t, const LogpostWide& p, float th) {
  const double thk = p.th + (double)t * 6.283185307179586;
  return -0.5 * p.q * thk * thk + (double)logpost_vol(th + (float)t * kTwoPi);
}

__global__ void so3_logpost_fwd_k(const float* v, const float* sigma, float* out, int64_t ns,
                                  int64_t B, int k) {
  LV_FOR_EACH(i, ns * B) {
    const int64_t b = i % B;
    float a[3], sg[3], var[3], ls[3];
    ld(v + i * 3, a);
    ld(sigma + b * 3, sg);
    for (int j = 0; j < 3; ++j) { var[j] = sg[j] * sg[j]; ls[j] = logf(sg[j]); }
    const float th = norm3(a);
    const float u[3] = {a[0] / th, a[1] / th, a[2] / th};
    float m, sum;
    logpost_max_sum(th, u, var, ls, k, m, sum);
    out[i] = m + logf(sum);
  }
}

__global__ void so3_logpost_bwd_k(const float* v, const float* sigma, const float* gout, float* gv,
                                  float* gsig, int64_t ns, int64_t B, int k) {
  LV_FOR_EACH(b, B) {
    float sg[3], var[3], ls[3];
    ld(sigma + b * 3, sg);
    for (int j = 0; j < 3; ++j) { var[j] = sg[j] * sg[j]; ls[j] = logf(sg[j]); }
    float gsacc[3] = {0.f, 0.f, 0.f};
    for (int64_t s = 0; s < ns; ++s) {
      const int64_t i = s * B + b;
      float a[3];
      ld(v + i * 3, a);
      const float th = norm3(a);
      const float u[3] = {a[0] / th, a[1] / th, a[2] / th};
      const LogpostWide wd = logpost_wide(a, sg);
      double m = -INFINITY;
      for (int t = -k; t <= k; ++t) m = fmax(m, logpost_term_wide(t, wd, th));
      float sum = 0.f;
      for (int t = -k; t <= k; ++t) sum += expf((float)(logpost_term_wide(t, wd, th) - m));
      const float g = gout[i] / sum;
      float gth = 0.f, gu[3] = {0.f, 0.f, 0.f};
      for (int t = -k; t <= k; ++t) {
        const float w = g * expf((float)(logpost_term_wide(t, wd, th) - m));
        const float thk = th + (float)t * kTwoPi;
        float dth = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const float x = u[j] * thk;
          dth -= x * u[j] / var[j];
          gu[j] -= w * x * thk / var[j];
          gsacc[j] += w * ((x * x) / (var[j] * sg[j]) - 1.f / sg[j]);
        }
        if (thk * thk >= 1e-3f) dth += 2.f * thk / (thk * thk);
        const float den = 2.f - 2.f * cosf(thk);
        if (den >= 1e-3f) dth -= 2.f * sinf(thk) / den;
        gth += w * dth;
      }
      float o[3];
      polar_vjp(a, th, gu, gth, o);
      st(gv + i * 3, o);
    }
    st(gsig + b * 3, gsacc);
  }
}

// Wave-per-element variants: lane t holds wrapped term t - k (2k+1 <= 64), max and sum
// over the terms by cross-lane reductions.  The thread-per-element kernels above run the
// 2k+1 terms (x2 passes, x3 in backward) serially per thread: at training sizes
// (ns * B = 512) that is a latency chain of ~60 transcendental terms on a few waves.
// Same per-term arithmetic; only the order of the exp-sum (and gradient sums) differs.
constexpr int kWaveMaxK = 31;
constexpr int64_t kWaveMaxElems = 1 << 16;  // beyond: enough elements to fill the chip per thread

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x = fmax(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

#define LV_FOR_EACH_WAVE(i, n)                                                          \
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < (n);        \
       i += ((int64_t)gridDim.x * blockDim.x) >> 6)

__global__ void so3_logpost_fwd_wave_k(const float* v, const float* sigma, float* out, int64_t ns,
                                       int64_t B, int k) {
  const int lane = threadIdx.x & 63;
  const bool on = lane < 2 * k + 1;
  LV_FOR_EACH_WAVE(i, ns * B) {
    const int64_t b = i % B;
    float a[3], sg[3], var[3], ls[3];
    ld(v + i * 3, a);
    ld(sigma + b * 3, sg);
    for (int j = 0; j < 3; ++j) { var[j] = sg[j] * sg[j]; ls[j] = logf(sg[j]); }
    const float th = norm3(a);
    const float u[3] = {a[0] / th, a[1] / th, a[2] / th};
    const float term = on ? logpost_term(lane - k, th, u, var, ls) : -INFINITY;
    const float m = wave_max(term);
    const float sum = wave_sum(on ? expf(term - m) : 0.f);
    if (lane == 0) out[i] = m + logf(sum);
  }
}

__global__ void so3_logpost_bwd_wave_k(const float* v, const float* sigma, const float* gout,
                                       float* gv, float* gsig, int64_t ns, int64_t B, int k) {
  const int lane = threadIdx.x & 63;
  const bool on = lane < 2 * k + 1;
  const int t = lane - k;
  LV_FOR_EACH_WAVE(b, B) {
    float sg[3], var[3], ls[3];
    ld(sigma + b * 3, sg);
    for (int j = 0; j < 3; ++j) { var[j] = sg[j] * sg[j]; ls[j] = logf(sg[j]); }
    float gsacc[3] = {0.f, 0.f, 0.f};
    for (int64_t s = 0; s < ns; ++s) {
      const int64_t i = s * B + b;
      float a[3];
      ld(v + i * 3, a);
      const float th = norm3(a);
      const float u[3] = {a[0] / th, a[1] / th, a[2] / th};
      const LogpostWide wd = logpost_wide(a, sg);
      const double term = on ? logpost_term_wide(t, wd, th) : (double)-INFINITY;
      const double m = wave_max(term);
      const float e = on ? expf((float)(term - m)) : 0.f;
      const float sum = wave_sum(e);
      float gth = 0.f, gu[3] = {0.f, 0.f, 0.f};
      if (on) {
        const float w = gout[i] * (e / sum);
        const float thk = th + (float)t * kTwoPi;
        float dth = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const float x = u[j] * thk;
          dth -= x * u[j] / var[j];
          gu[j] = -(w * x * thk / var[j]);
          gsacc[j] += w * ((x * x) / (var[j] * sg[j]) - 1.f / sg[j]);
        }
        if (thk * thk >= 1e-3f) dth += 2.f * thk / (thk * thk);
        const float den = 2.f - 2.f * cosf(thk);
        if (den >= 1e-3f) dth -= 2.f * sinf(thk) / den;
        gth = w * dth;
      }
      gth = wave_sum(gth);
#pragma unroll
      for (int j = 0; j < 3; ++j) gu[j] = wave_sum(gu[j]);
      if (lane == 0) {
        float o[3];
        polar_vjp(a, th, gu, gth, o);
        st(gv + i * 3, o);
      }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) gsacc[j] = wave_sum(gsacc[j]);
    if (lane == 0) st(gsig + b * 3, gsacc);
  }
}

inline dim3 grid_for_waves(int64_t nwaves) {
  int64_t b = (nwaves * 64 + kBlock - 1) / kBlock;
  if (b > 65536) b = 65536;
  return dim3((unsigned)b);
}

// Sizes and k shared by lv_so3_log_posterior_fwd / _bwd / _plan.
int logpost_check(int64_t ns, int64_t B, int k) {
  LV_CHECK_ARG(ns >= 0 && B >= 0, "bad sizes");
  LV_CHECK_ARG(k >= 0 && k <= kMaxWrap, "k must be in [0, %d]", kMaxWrap);
  return LV_OK;
}
// The dispatch of the density, one rule per direction (the entry points and the plan call
// these): the forward has ns * B elements, the backward one element per b (it sums over s).
inline bool logpost_fwd_wave(int64_t ns, int64_t B, int k) {
  const int64_t n = ns * B;
  return n > 0 && k <= kWaveMaxK && n <= kWaveMaxElems;
}
inline bool logpost_bwd_wave(int64_t ns, int64_t B, int k) {
  return ns > 0 && B > 0 && k <= kWaveMaxK && B <= kWaveMaxElems;
}

}  // namespace lv

using namespace lv;

#define LV_PTRS(...) LV_CHECK_ARG(n == 0 || (__VA_ARGS__), "null pointer argument")
#define LV_LAUNCH1(kern, n, ...)                                                     \
  do {                                                                               \
    clear_error();                                                                   \
    LV_CHECK_ARG((n) >= 0, "n must be >= 0");                                        \
    if ((n) == 0) return LV_OK;                                                      \
    hipLaunchKernelGGL(kern, grid_for(n), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); \
    LV_RETURN_LAUNCH(#kern);                                                         \
  } while (0)

extern "C" {

int lv_abi_version(void) { return 1; }
const char* lv_last_error(void) { return g_err; }
int lv_max_degree(void) { return LV_MAX_DEGREE; }

int lv_so3_exp_fwd(const float* v, float* R, int64_t n, void* stream) {
  LV_PTRS(v && R);
  LV_LAUNCH1(so3_exp_fwd_k<float>, n, v, R, n);
}
int lv_so3_exp_bwd(const float* v, const float* gR, float* gv, int64_t n, void* stream) {
  LV_PTRS(v && gR && gv);
  LV_LAUNCH1(so3_exp_bwd_k<float>, n, v, gR, gv, n);
}
int lv_so3_sample_fwd(const float* mu, const float* v, float* z, int64_t ns, int64_t B, void* stream) {
  const int64_t n = ns * B;
  LV_CHECK_ARG(ns >= 0 && B >= 0, "bad sizes");
  LV_PTRS(mu && v && z);
  LV_LAUNCH1(so3_sample_fwd_k<float>, n, mu, v, z, ns, B);
}
int lv_so3_sample_bwd(const float* mu, const float* v, const float* gz, float* gmu, float* gv,
                      int64_t ns, int64_t B, void* stream) {
  const int64_t n = B;
  LV_CHECK_ARG(ns >= 0 && B >= 0, "bad sizes");
  LV_PTRS(mu && v && gz && gmu && gv);
  if (ns == 0) {
    (void)hipMemsetAsync(gmu, 0, sizeof(float) * 9 * B, (hipStream_t)stream);
    return LV_OK;
  }
  LV_LAUNCH1(so3_sample_bwd_k<float>, n, mu, v, gz, gmu, gv, ns, B);
}
int lv_exp_eazyz_vjp(const float* mu, const float* v, const float* gang, float* gmu, float* gv,
                     int64_t n, void* stream) {
  LV_PTRS(v && gang && gv && (!mu || gmu));
  LV_LAUNCH1(exp_eazyz_vjp_k<float>, n, mu, v, gang, gmu, gv, n);
}
int lv_quat_to_mat_fwd(const float* q, float* R, int64_t n, void* stream) {
  LV_PTRS(q && R);
  LV_LAUNCH1(quat_to_mat_fwd_k<float>, n, q, R, n);
}
int lv_quat_to_mat_bwd(const float* q, const float* gR, float* gq, int64_t n, void* stream) {
  LV_PTRS(q && gR && gq);
  LV_LAUNCH1(quat_to_mat_bwd_k<float>, n, q, gR, gq, n);
}
int lv_mat_to_quat_fwd(const float* R, float* q, int64_t n, void* stream) {
  LV_PTRS(R && q);
  LV_LAUNCH1(mat_to_quat_fwd_k<float>, n, R, q, n);
}
int lv_mat_to_quat_bwd(const float* R, const float* gq, float* gR, int64_t n, void* stream) {
  LV_PTRS(R && gq && gR);
  LV_LAUNCH1(mat_to_quat_bwd_k<float>, n, R, gq, gR, n);
}
int lv_quat_to_eazyz_fwd(const float* q, float* ang, int64_t n, void* stream) {
  LV_PTRS(q && ang);
  LV_LAUNCH1(quat_to_eazyz_fwd_k<float>, n, q, ang, n);
}
int lv_quat_to_eazyz_bwd(const float* q, const float* gang, float* gq, int64_t n, void* stream) {
  LV_PTRS(q && gang && gq);
  LV_LAUNCH1(quat_to_eazyz_bwd_k<float>, n, q, gang, gq, n);
}
int lv_mat_to_eazyz_fwd(const float* R, float* ang, int64_t n, void* stream) {
  LV_PTRS(R && ang);
  LV_LAUNCH1(mat_to_eazyz_fwd_k<float>, n, R, ang, n);
}
int lv_mat_to_eazyz_bwd(const float* R, const float* gang, float* gR, int64_t n, void* stream) {
  LV_PTRS(R && gang && gR);
  LV_LAUNCH1(mat_to_eazyz_bwd_k<float>, n, R, gang, gR, n);
}
int lv_s2s1_fwd(const float* axis, const float* cs, float* R, int64_t n, void* stream) {
  LV_PTRS(axis && cs && R);
  LV_LAUNCH1(s2s1_fwd_k<float>, n, axis, cs, R, n);
}
int lv_s2s1_bwd(const float* axis, const float* cs, const float* gR, float* gaxis, float* gcs,
                int64_t n, void* stream) {
  LV_PTRS(axis && cs && gR && gaxis && gcs);
  LV_LAUNCH1(s2s1_bwd_k<float>, n, axis, cs, gR, gaxis, gcs, n);
}
// fp64 twins of the per-sample maps above: the reference's maps follow the input dtype
// (lie_tools.py:28-38,61 -- new_tensor / eye(dtype=v.dtype)), and its own self-tests run
// them in fp64 (lie_tools.py:271-291).  Same templates, T = double.
int lv_so3_exp_fwd_f64(const double* v, double* R, int64_t n, void* stream) {
  LV_PTRS(v && R);
  LV_LAUNCH1(so3_exp_fwd_k<double>, n, v, R, n);
}
int lv_so3_exp_bwd_f64(const double* v, const double* gR, double* gv, int64_t n, void* stream) {
  LV_PTRS(v && gR && gv);
  LV_LAUNCH1(so3_exp_bwd_k<double>, n, v, gR, gv, n);
}
int lv_so3_sample_fwd_f64(const double* mu, const double* v, double* z, int64_t ns, int64_t B, void* stream) {
  const int64_t n = ns * B;
  LV_CHECK_ARG(ns >= 0 && B >= 0, "bad sizes");
  LV_PTRS(mu && v && z);
  LV_LAUNCH1(so3_sample_fwd_k<double>, n, mu, v, z, ns, B);
}
int lv_so3_sample_bwd_f64(const double* mu, const double* v, const double* gz, double* gmu, double* gv,
                      int64_t ns, int64_t B, void* stream) {
  const int64_t n = B;
  LV_CHECK_ARG(ns >= 0 && B >= 0, "bad sizes");
  LV_PTRS(mu && v && gz && gmu && gv);
  if (ns == 0) {
    (void)hipMemsetAsync(gmu, 0, sizeof(double) * 9 * B, (hipStream_t)stream);
    return LV_OK;
  }
  LV_LAUNCH1(so3_sample_bwd_k<double>, n, mu, v, gz, gmu, gv, ns, B);
}
int lv_exp_eazyz_vjp_f64(const double* mu, const double* v, const double* gang, double* gmu, double* gv,
                     int64_t n, void* stream) {
  LV_PTRS(v && gang && gv && (!mu || gmu));
  LV_LAUNCH1(exp_eazyz_vjp_k<double>, n, mu, v, gang, gmu, gv, n);
}
int lv_quat_to_mat_fwd_f64(const double* q, double* R, int64_t n, void* stream) {
  LV_PTRS(q && R);
  LV_LAUNCH1(quat_to_mat_fwd_k<double>, n, q, R, n);
}
int lv_quat_to_mat_bwd_f64(const double* q, const double* gR, double* gq, int64_t n, void* stream) {
  LV_PTRS(q && gR && gq);
  LV_LAUNCH1(quat_to_mat_bwd_k<double>, n, q, gR, gq, n);
}
int lv_mat_to_quat_fwd_f64(const double* R, double* q, int64_t n, void* stream) {
  LV_PTRS(R && q);
  LV_LAUNCH1(mat_to_quat_fwd_k<double>, n, R, q, n);
}
int lv_mat_to_quat_bwd_f64(const double* R, const double* gq, double* gR, int64_t n, void* stream) {
  LV_PTRS(R && gq && gR);
  LV_LAUNCH1(mat_to_quat_bwd_k<double>, n, R, gq, gR, n);
}
int lv_quat_to_eazyz_fwd_f64(const double* q, double* ang, int64_t n, void* stream) {
  LV_PTRS(q && ang);
  LV_LAUNCH1(quat_to_eazyz_fwd_k<double>, n, q, ang, n);
}
int lv_quat_to_eazyz_bwd_f64(const double* q, const double* gang, double* gq, int64_t n, void* stream) {
  LV_PTRS(q && gang && gq);
  LV_LAUNCH1(quat_to_eazyz_bwd_k<double>, n, q, gang, gq, n);
}
int lv_mat_to_eazyz_fwd_f64(const double* R, double* ang, int64_t n, void* stream) {
  LV_PTRS(R && ang);
  LV_LAUNCH1(mat_to_eazyz_fwd_k<double>, n, R, ang, n);
}
int lv_mat_to_eazyz_bwd_f64(const double* R, const double* gang, double* gR, int64_t n, void* stream) {
  LV_PTRS(R && gang && gR);
  LV_LAUNCH1(mat_to_eazyz_bwd_k<double>, n, R, gang, gR, n);
}
int lv_s2s1_fwd_f64(const double* axis, const double* cs, double* R, int64_t n, void* stream) {
  LV_PTRS(axis && cs && R);
  LV_LAUNCH1(s2s1_fwd_k<double>, n, axis, cs, R, n);
}
int lv_s2s1_bwd_f64(const double* axis, const double* cs, const double* gR, double* gaxis, double* gcs,
                int64_t n, void* stream) {
  LV_PTRS(axis && cs && gR && gaxis && gcs);
  LV_LAUNCH1(s2s1_bwd_k<double>, n, axis, cs, gR, gaxis, gcs, n);
}
int lv_s2s2_fwd_f64(const double* v1, const double* v2, double* R, int64_t n, void* stream) {
  LV_PTRS(v1 && v2 && R);
  LV_LAUNCH1(s2s2_fwd_k, n, v1, v2, R, n);
}
int lv_s2s2_bwd_f64(const double* v1, const double* v2, const double* gR, double* gv1,
                    double* gv2, int64_t n, void* stream) {
  LV_PTRS(v1 && v2 && gR && gv1 && gv2);
  LV_LAUNCH1(s2s2_bwd_k, n, v1, v2, gR, gv1, gv2, n);
}
// so(3) log family, fp32 and the fp64 twins (the maps follow their input dtype): one body.
#define LV_SO3_LOG_ENTRIES(T, SUF)                                                              \
  int lv_so3_log_fwd##SUF(const T* R, T* v, int64_t n, void* stream) {                          \
    LV_CHECK_ARG(n >= 0, "n must be >= 0");                                                     \
    LV_PTRS(R && v);                                                                            \
    LV_LAUNCH1(so3_log_fwd_k<T>, n, R, v, n);                                                   \
  }                                                                                             \
  int lv_so3_log_bwd##SUF(const T* R, const T* gv, T* gR, int64_t n, void* stream) {            \
    LV_CHECK_ARG(n >= 0, "n must be >= 0");                                                     \
    LV_PTRS(R && gv && gR);                                                                     \
    LV_LAUNCH1(so3_log_bwd_k<T>, n, R, gv, gR, n);                                              \
  }                                                                                             \
  int lv_so3_rel_log_fwd##SUF(const T* mu, const T* z, T* v, int64_t ns, int64_t B,             \
                              void* stream) {                                                   \
    LV_CHECK_ARG(ns >= 0 && B >= 0, "ns and B must be >= 0");                                   \
    const int64_t n = ns * B;                                                                   \
    LV_PTRS(mu && z && v);                                                                      \
    LV_LAUNCH1(so3_rel_log_fwd_k<T>, n, mu, z, v, ns, B);                                       \
  }                                                                                             \
  int lv_so3_rel_log_bwd##SUF(const T* mu, const T* z, const T* gv, T* gmu, T* gz, int64_t ns,  \
                              int64_t B, void* stream) {                                        \
    LV_CHECK_ARG(ns >= 0 && B >= 0, "ns and B must be >= 0");                                   \
    const int64_t n = B;                                                                        \
    LV_CHECK_ARG(n == 0 || (mu && gmu && (ns == 0 || (z && gv && gz))), "null pointer argument"); \
    if (ns == 0 && B > 0) {                                                                     \
      clear_error();                                                                            \
      (void)hipMemsetAsync(gmu, 0, sizeof(T) * 9 * B, (hipStream_t)stream);                     \
      return LV_OK;                                                                             \
    }                                                                                           \
    LV_LAUNCH1(so3_rel_log_bwd_k<T>, n, mu, z, gv, gmu, gz, ns, B);                             \
  }                                                                                             \
  int lv_so3_angle_fwd##SUF(const T* A, const T* B, T* theta, int64_t n, void* stream) {        \
    LV_CHECK_ARG(n >= 0, "n must be >= 0");                                                     \
    LV_PTRS(A && B && theta);                                                                   \
    LV_LAUNCH1(so3_angle_fwd_k<T>, n, A, B, theta, n);                                          \
  }                                                                                             \
  int lv_so3_angle_bwd##SUF(const T* A, const T* B, const T* gtheta, T* gA, T* gB, int64_t n,   \
                            void* stream) {                                                     \
    LV_CHECK_ARG(n >= 0, "n must be >= 0");                                                     \
    LV_PTRS(A && B && gtheta && gA && gB);                                                      \
    LV_LAUNCH1(so3_angle_bwd_k<T>, n, A, B, gtheta, gA, gB, n);                                 \
  }
LV_SO3_LOG_ENTRIES(float, )
LV_SO3_LOG_ENTRIES(double, _f64)
#undef LV_SO3_LOG_ENTRIES

int lv_softplus_fwd(const float* h, float* sigma, int64_t n, void* stream) {
  LV_PTRS(h && sigma);
  LV_LAUNCH1(softplus_fwd_k, n, h, sigma, n);
}
int lv_softplus_bwd(const float* h, const float* gsigma, float* gh, int64_t n, void* stream) {
  LV_PTRS(h && gsigma && gh);
  LV_LAUNCH1(softplus_bwd_k, n, h, gsigma, gh, n);
}
int lv_n0_sample_fwd(const float* sigma, const float* eps, float* v, int64_t ns, int64_t B,
                     void* stream) {
  const int64_t n = ns * B * 3;
  LV_CHECK_ARG(ns >= 0 && B >= 0, "bad sizes");
  LV_PTRS(sigma && eps && v);
  LV_LAUNCH1(n0_sample_fwd_k, n, sigma, eps, v, ns, B);
}
int lv_n0_sample_bwd(const float* eps, const float* gv, float* gsigma, int64_t ns, int64_t B,
                     void* stream) {
  const int64_t n = B * 3;
  LV_CHECK_ARG(ns >= 0 && B >= 0, "bad sizes");
  LV_PTRS(eps && gv && gsigma);
  LV_LAUNCH1(n0_sample_bwd_k, n, eps, gv, gsigma, ns, B);
}
int lv_so3_log_posterior_fwd(const float* v, const float* sigma, float* out, int64_t ns,
                             int64_t B, int k, void* stream) {
  const int64_t n = ns * B;
  if (int rc = logpost_check(ns, B, k)) return rc;
  LV_PTRS(v && sigma && out);
  if (logpost_fwd_wave(ns, B, k)) {
    clear_error();
    hipLaunchKernelGGL(so3_logpost_fwd_wave_k, grid_for_waves(n), dim3(kBlock), 0,
                       (hipStream_t)stream, v, sigma, out, ns, B, k);
    LV_RETURN_LAUNCH("so3_logpost_fwd_wave_k");
  }
  LV_LAUNCH1(so3_logpost_fwd_k, n, v, sigma, out, ns, B, k);
}
int lv_so3_log_posterior_bwd(const float* v, const float* sigma, const float* gout, float* gv,
                             float* gsigma, int64_t ns, int64_t B, int k, void* stream) {
  const int64_t n = B;
  if (int rc = logpost_check(ns, B, k)) return rc;
  // ns == 0: v, gout and gv are empty (null from an empty tensor); gsigma is a sum of nothing
  LV_CHECK_ARG(n == 0 || (sigma && gsigma && (ns == 0 || (v && gout && gv))),
               "null pointer argument");
  if (ns == 0) {
    clear_error();
    if (B > 0) (void)hipMemsetAsync(gsigma, 0, sizeof(float) * 3 * B, (hipStream_t)stream);
    return LV_OK;
  }
  if (logpost_bwd_wave(ns, B, k)) {
    clear_error();
    hipLaunchKernelGGL(so3_logpost_bwd_wave_k, grid_for_waves(n), dim3(kBlock), 0,
                       (hipStream_t)stream, v, sigma, gout, gv, gsigma, ns, B, k);
    LV_RETURN_LAUNCH("so3_logpost_bwd_wave_k");
  }
  LV_LAUNCH1(so3_logpost_bwd_k, n, v, sigma, gout, gv, gsigma, ns, B, k);
}
int lv_so3_log_posterior_plan(int64_t ns, int64_t B, int k, int64_t* plan) {
  clear_error();
  LV_CHECK_ARG(plan, "null pointer argument");
  if (int rc = logpost_check(ns, B, k)) return rc;
  const bool fw = logpost_fwd_wave(ns, B, k), bw = logpost_bwd_wave(ns, B, k);
  const int64_t nf = ns * B, nb = ns > 0 ? B : 0;  // ns == 0: the backward is a memset
  plan[0] = fw;
  plan[1] = bw;
  plan[2] = nf == 0 ? 0 : (fw ? grid_for_waves(nf) : grid_for(nf)).x;
  plan[3] = nb == 0 ? 0 : (bw ? grid_for_waves(nb) : grid_for(nb)).x;
  plan[4] = kBlock;
  return LV_OK;
}

}  // extern "C"
