// Per-sample SO(3) math, forward and hand-derived backward, in registers.
//
// Every function restates one reference op (file:line under the reference root) and
// keeps its evaluation order (the library is built with -ffp-contract=off, so nothing
// here is silently fused into an FMA).  Backward functions return the gradient autograd
// would produce for the same composition of torch ops.  The maps are templates on the
// scalar type T: the reference's maps follow their input dtype (v.new_tensor,
// eye(dtype=v.dtype), lie_tools.py:28-38,61), so fp64 inputs get fp64 kernels; T = T
// is the hot path and compiles to exactly the former fp32 code.
#pragma once
#include <hip/hip_runtime.h>

namespace lv {

// Scalar-type helpers: overloads so that one template body gives the fp32 code
// (sincosf) for float and the fp64 code (sincos) for double.
template <typename T>
struct lv_nondeduced { using type = T; };
__device__ __forceinline__ void lv_sincos(float x, float* s, float* c) { sincosf(x, s, c); }
__device__ __forceinline__ void lv_sincos(double x, double* s, double* c) { sincos(x, s, c); }

// ---------------------------------------------------------------- rodrigues
// lie_tools.py:17-43 (hat) and :56-64 (rodrigues).  K = hat(u), K2 = K@K.
template <typename T>
__device__ __forceinline__ void hat_sq(const T u[3], T K[9], T K2[9]) {
  K[0] = T(0.);   K[1] = -u[2]; K[2] = u[1];
  K[3] = u[2];  K[4] = T(0.);   K[5] = -u[0];
  K[6] = -u[1]; K[7] = u[0];  K[8] = T(0.);
  // (K@K)_ij summed k = 0..2 exactly as the matmul does (zero products drop out).
  K2[0] = -u[2] * u[2] - u[1] * u[1];
  K2[1] = u[1] * u[0];
  K2[2] = u[2] * u[0];
  K2[3] = u[0] * u[1];
  K2[4] = -u[2] * u[2] - u[0] * u[0];
  K2[5] = u[2] * u[1];
  K2[6] = u[0] * u[2];
  K2[7] = u[1] * u[2];
  K2[8] = -u[1] * u[1] - u[0] * u[0];
}

template <typename T>
__device__ __forceinline__ T norm3(const T v[3]) {
  return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
}

// The angle-dependent pieces rodrigues_fwd and rodrigues_bwd both start from, computed
// once when a caller needs both (exp_eazyz_vjp_sample): the same operations, so the same
// bits as computing them twice.
template <typename T>
struct RodPrep {
  T th, u[3], K[9], K2[9], s, c;
};
template <typename T>
__device__ __forceinline__ void rodrigues_prep(const T v[3], RodPrep<T>& p) {
  p.th = norm3(v);
  p.u[0] = v[0] / p.th;  // NaN at th == 0, like the reference
  p.u[1] = v[1] / p.th;
  p.u[2] = v[2] / p.th;
  hat_sq(p.u, p.K, p.K2);
  lv_sincos(p.th, &p.s, &p.c);
}
template <typename T>
__device__ __forceinline__ void rodrigues_fwd_p(const RodPrep<T>& p, T R[9]) {
  const T omc = T(1.) - p.c;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const T eye = (i == 0 || i == 4 || i == 8) ? T(1.) : T(0.);
    R[i] = (eye + p.s * p.K[i]) + omc * p.K2[i];
  }
}
template <typename T>
__device__ __forceinline__ void rodrigues_fwd(const T v[3], T R[9]) {
  RodPrep<T> p;
  rodrigues_prep(v, p);
  rodrigues_fwd_p(p, R);
}

// d/du of <g, s K(u) + w (u u^T - |u|^2 I)>
template <typename T>
__device__ __forceinline__ void hat_sq_vjp(const T u[3], const T g[9], T s, T w,
                                           T gu[3]) {
  const T tr = g[0] + g[4] + g[8];
  T gsym_u[3];
#pragma unroll
  for (int m = 0; m < 3; ++m)
    gsym_u[m] = (g[m * 3 + 0] + g[0 * 3 + m]) * u[0] + (g[m * 3 + 1] + g[1 * 3 + m]) * u[1] +
                (g[m * 3 + 2] + g[2 * 3 + m]) * u[2];
  gu[0] = s * (g[7] - g[5]) + w * (gsym_u[0] - T(2.) * tr * u[0]);
  gu[1] = s * (g[2] - g[6]) + w * (gsym_u[1] - T(2.) * tr * u[1]);
  gu[2] = s * (g[3] - g[1]) + w * (gsym_u[2] - T(2.) * tr * u[2]);
}

// (theta, u = v/theta) -> v chain rule.
template <typename T>
__device__ __forceinline__ void polar_vjp(const T v[3], T th, const T gu[3], T gth,
                                          T gv[3]) {
  const T dot = gu[0] * v[0] + gu[1] * v[1] + gu[2] * v[2];
  const T inv = T(1.) / th;
  const T inv3 = inv * inv * inv;
#pragma unroll
  for (int i = 0; i < 3; ++i) gv[i] = gu[i] * inv - dot * v[i] * inv3 + gth * v[i] * inv;
}

template <typename T>
__device__ __forceinline__ void rodrigues_bwd_p(const T v[3], const RodPrep<T>& p, const T gR[9], T gv[3]) {
  T gth = T(0.);
#pragma unroll
  for (int i = 0; i < 9; ++i) gth += gR[i] * (p.c * p.K[i] + p.s * p.K2[i]);
  T gu[3];
  hat_sq_vjp(p.u, gR, p.s, T(1.) - p.c, gu);
  polar_vjp(v, p.th, gu, gth, gv);
}
template <typename T>
__device__ __forceinline__ void rodrigues_bwd(const T v[3], const T gR[9], T gv[3]) {
  RodPrep<T> p;
  rodrigues_prep(v, p);
  rodrigues_bwd_p(v, p, gR, gv);
}

// ------------------------------------------------------------------ 3x3 ops
template <typename T>
__device__ __forceinline__ void matmul3(const T A[9], const T B[9], T C[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      C[i * 3 + j] = (A[i * 3 + 0] * B[0 * 3 + j] + A[i * 3 + 1] * B[1 * 3 + j]) +
                     A[i * 3 + 2] * B[2 * 3 + j];
}
// C = A^T B
template <typename T>
__device__ __forceinline__ void matmul3_tn(const T A[9], const T B[9], T C[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      C[i * 3 + j] = A[0 * 3 + i] * B[0 * 3 + j] + A[1 * 3 + i] * B[1 * 3 + j] +
                     A[2 * 3 + i] * B[2 * 3 + j];
}
// C = A B^T
template <typename T>
__device__ __forceinline__ void matmul3_nt(const T A[9], const T B[9], T C[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      C[i * 3 + j] = A[i * 3 + 0] * B[j * 3 + 0] + A[i * 3 + 1] * B[j * 3 + 1] +
                     A[i * 3 + 2] * B[j * 3 + 2];
}

// ------------------------------------------------------------------ so(3) log
// lie_tools.py:100-109 (log_map) gives theta / sin(theta) * (R - R^T)/2 with theta = acos of
// the trace: NaN at the identity, and no digits left near theta = pi, where R - R^T vanishes
// and acos of an fp32 cosine is useless (as for beta above).  Here, per sample:
//   w = vee(R - R^T)/2, s = |w| = sin(theta), c = (tr R - 1)/2, theta = atan2(s, c) in [0, pi].
//   c >= 0: v = (theta/s) w; below s = kLogSeriesS, theta/s = asin(s)/s by its series, so R = I
//           gives v = 0 exactly.
//   c <  0: the axis from the symmetric part S = (R + R^T)/2 = c I + (1 - c) a a^T: the largest
//           a_i^2 = (S_ii - c)/(1 - c) (>= 1/3, so the root and the division are well
//           conditioned), the other two components from row i of S, renormalised, the sign such
//           that a.w >= 0; v = theta a.  At theta = pi exactly (w = 0) both signs are logs of R:
//           a_i > 0 is kept, i.e. the component of largest magnitude is positive.
// LogPolar also carries the unit axis (0 where s == 0 on the c >= 0 side: the identity).
constexpr double kLogSeriesS = 0.03;
constexpr double kKappaSeriesTh = 0.25;

template <typename T>
struct LogPolar {
  T th, v[3], a[3];
};

template <typename T>
__device__ __forceinline__ void so3_log_polar(const T r[9], LogPolar<T>& p) {
  // scalars and selects throughout: no small array is indexed or passed by address, so
  // nothing lands in scratch memory
  const T w0 = T(0.5) * (r[7] - r[5]), w1 = T(0.5) * (r[2] - r[6]), w2 = T(0.5) * (r[3] - r[1]);
  const T s = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
  const T c = T(0.5) * (((r[0] + r[4]) + r[8]) - T(1.));
  const T th = atan2(s, c);
  T a0, a1, a2, v0, v1, v2;
  if (c >= T(0.)) {
    const T s2 = s * s;
    const T k = s < T(kLogSeriesS)
                    ? T(1.) + s2 * (T(1. / 6.) + s2 * (T(3. / 40.) + s2 * T(15. / 336.)))
                    : th / s;
    const T inv = s > T(0.) ? T(1.) / s : T(0.);
    v0 = k * w0; v1 = k * w1; v2 = k * w2;
    a0 = w0 * inv; a1 = w1 * inv; a2 = w2 * inv;
  } else {
    const T omc = T(1.) - c;
    const T d0 = (r[0] - c) / omc, d1 = (r[4] - c) / omc, d2 = (r[8] - c) / omc;
    const int i = (d0 >= d1 && d0 >= d2) ? 0 : (d1 >= d2 ? 1 : 2);
    const T ai = sqrt(i == 0 ? d0 : (i == 1 ? d1 : d2));
    const T den = omc * ai;
    const T s01 = T(0.5) * (r[1] + r[3]), s02 = T(0.5) * (r[2] + r[6]), s12 = T(0.5) * (r[5] + r[7]);
    // row i of S over (1 - c) a_i, a_i itself on the diagonal
    const T b0 = i == 0 ? ai : (i == 1 ? s01 : s02) / den;
    const T b1 = i == 1 ? ai : (i == 0 ? s01 : s12) / den;
    const T b2 = i == 2 ? ai : (i == 0 ? s02 : s12) / den;
    const T nrm = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
    const T sgn = (b0 * w0 + b1 * w1) + b2 * w2 < T(0.) ? -T(1.) : T(1.);
    a0 = sgn * (b0 / nrm); a1 = sgn * (b1 / nrm); a2 = sgn * (b2 / nrm);
    v0 = th * a0; v1 = th * a1; v2 = th * a2;
  }
  p.th = th;
  p.v[0] = v0; p.v[1] = v1; p.v[2] = v2;
  p.a[0] = a0; p.a[1] = a1; p.a[2] = a2;
}

// kappa(theta) = 1/theta^2 - cot(theta/2) / (2 theta): 1/12 at 0 (series below
// kKappaSeriesTh, where the two terms cancel), 1/pi^2 at pi.
template <typename T>
__device__ __forceinline__ T so3_kappa(T th) {
  if (th < T(kKappaSeriesTh)) {
    const T t2 = th * th;
    return T(1. / 12.) +
           t2 * (T(1. / 720.) + t2 * (T(1. / 30240.) + t2 * (T(1. / 1209600.) + t2 * T(1. / 47900160.))));
  }
  T sh, ch;
  lv_sincos(T(0.5) * th, &sh, &ch);
  return T(1.) / (th * th) - ch / ((T(2.) * th) * sh);
}

// Backward of the log.  The input is a rotation, so the gradient is defined on the tangent
// space of SO(3) at R: with log(R exp(xi)) = v + J_r^-1(v) xi + O(xi^2) and
// J_r^-1(v) = I + hat(v)/2 + kappa(|v|) hat(v)^2, the gradient is gR = R hat(u),
// u = J_r^-T(v) gv / 2 = (gv - v x gv / 2 + kappa v x (v x gv)) / 2, finite up to theta = pi.
// Its component normal to SO(3) is zero by definition; composed with any parametrisation that
// stays in SO(3) it gives the parameter gradients autograd finds through any other formula.
template <typename T>
__device__ __forceinline__ void cross3(const T a[3], const T b[3], T c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
template <typename T>
__device__ __forceinline__ void so3_log_tangent(const LogPolar<T>& p, const T gv[3], T u[3]) {
  T x1[3], x2[3];
  cross3(p.v, gv, x1);
  cross3(p.v, x1, x2);
  const T kap = so3_kappa(p.th);
#pragma unroll
  for (int j = 0; j < 3; ++j) u[j] = T(0.5) * ((gv[j] - T(0.5) * x1[j]) + kap * x2[j]);
}
// G = R hat(u)
template <typename T>
__device__ __forceinline__ void mul_hat(const T r[9], const T u[3], T g[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    g[i * 3 + 0] = r[i * 3 + 1] * u[2] - r[i * 3 + 2] * u[1];
    g[i * 3 + 1] = r[i * 3 + 2] * u[0] - r[i * 3 + 0] * u[2];
    g[i * 3 + 2] = r[i * 3 + 0] * u[1] - r[i * 3 + 1] * u[0];
  }
}

// ----------------------------------------------- group_matrix_to_quaternions
// lie_tools.py:112-157: 4-case trace method, eps 1e-6, case = first argmax.
template <typename T>
struct QuatCase {
  T pre[4];
  T den[4];
  int k;
};

template <typename T>
__device__ __forceinline__ void mat_to_quat_fwd(const T r[9], T q[4],
                                                typename lv_nondeduced<QuatCase<T>>::type* qc) {
  const T a = r[0], b = r[4], c = r[8];
  T pre[4] = {((T(1.) + a) - b) - c, ((T(1.) - a) + b) - c, ((T(1.) - a) - b) + c,
                  ((T(1.) + a) + b) + c};
  T den[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) den[i] = T(0.5) * sqrt(T(1e-6) + fabs(pre[i]));
  int k = 0;
  T best = den[0];
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (den[i] > best) { best = den[i]; k = i; }
  const T s01 = r[1] + r[3], s02 = r[2] + r[6], s12 = r[5] + r[7];
  const T d12 = r[5] - r[7], d20 = r[6] - r[2], d01 = r[1] - r[3];
  const T d4 = T(4.) * best;
  switch (k) {
    case 0: q[0] = best;      q[1] = s01 / d4;  q[2] = s02 / d4;  q[3] = d12 / d4; break;
    case 1: q[0] = s01 / d4;  q[1] = best;      q[2] = s12 / d4;  q[3] = d20 / d4; break;
    case 2: q[0] = s02 / d4;  q[1] = s12 / d4;  q[2] = best;      q[3] = d01 / d4; break;
    default: q[0] = d12 / d4; q[1] = d20 / d4;  q[2] = d01 / d4;  q[3] = best; break;
  }
  if (qc) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { qc->pre[i] = pre[i]; qc->den[i] = den[i]; }
    qc->k = k;
  }
}

// The backward from the forward's own q and case (mat_to_quat_fwd(r, q, &qc) already run).
// Written without run-time indexing of small arrays (case tables, q[k], den[k]): those put
// the arrays in scratch memory, a dependent global round trip on the VJP's serial chain.
// Every gr entry receives exactly one term, 0 + g or 0 - g, so the selects below give the
// same bits as the per-case accumulation.
template <typename T>
__device__ __forceinline__ T sel4(int k, T a0, T a1, T a2, T a3) {
  return k == 0 ? a0 : (k == 1 ? a1 : (k == 2 ? a2 : a3));
}
template <typename T>
__device__ __forceinline__ void mat_to_quat_bwd_qc(const T q[4], const QuatCase<T>& qc, const T gq[4], T gr[9]) {
  const int k = qc.k;
  const T d = sel4(k, qc.den[0], qc.den[1], qc.den[2], qc.den[3]);
  const T inv4d = T(1.) / (T(4.) * d);
  // gradient into the denominator: q_k = d, q_j = N_j / (4 d)
  T gd = sel4(k, gq[0], gq[1], gq[2], gq[3]);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j != k) gd -= gq[j] * q[j] / d;
  // N_j partials.  Numerators per case: case0 (s01, s02, d12) at q1..q3; case1 (s01, s12,
  // d20) at q0, q2, q3; case2 (s02, s12, d01) at q0, q1, q3; case3 (d12, d20, d01) at q0..q2;
  // s01 = r01 + r10, s02 = r02 + r20, s12 = r12 + r21, d12 = r12 - r21, d20 = r20 - r02,
  // d01 = r01 - r10.
  T g[4];
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) g[jj] = gq[jj] * inv4d;
  const T z = T(0.);
  gr[1] = z + sel4(k, g[1], g[0], g[3], g[2]);                      // s01 | d01
  gr[3] = k < 2 ? z + sel4(k, g[1], g[0], g[0], g[0]) : z - sel4(k, g[0], g[0], g[3], g[2]);
  gr[2] = (k == 0 || k == 2) ? z + sel4(k, g[2], g[2], g[0], g[0]) : z - sel4(k, g[3], g[3], g[3], g[1]);
  gr[6] = z + sel4(k, g[2], g[3], g[0], g[1]);                      // s02 | d20
  gr[5] = z + sel4(k, g[3], g[2], g[1], g[0]);                      // d12 | s12
  gr[7] = (k == 1 || k == 2) ? z + sel4(k, g[2], g[2], g[1], g[2]) : z - sel4(k, g[3], g[3], g[3], g[0]);
  // d = 0.5 sqrt(1e-6 + |pre_k|)
  const T p = sel4(k, qc.pre[0], qc.pre[1], qc.pre[2], qc.pre[3]);
  const T t = sqrt(T(1e-6) + fabs(p));
  const T sg = (p > T(0.)) ? T(1.) : ((p < T(0.)) ? -T(1.) : T(0.));
  const T gpre = gd * T(0.25) / t * sg;
  // coef[k][i] = +1 if k == 3 or k == i, else -1
  gr[0] = z + ((k == 3 || k == 0) ? gpre : -gpre);
  gr[4] = z + ((k == 3 || k == 1) ? gpre : -gpre);
  gr[8] = z + ((k == 3 || k == 2) ? gpre : -gpre);
}
template <typename T>
__device__ __forceinline__ void mat_to_quat_bwd(const T r[9], const T gq[4], T gr[9]) {
  T q[4];
  QuatCase<T> qc;
  mat_to_quat_fwd(r, q, &qc);
  mat_to_quat_bwd_qc(q, qc, gq, gr);
}

// ----------------------------------------------------- quaternions_to_eazyz
// lie_tools.py:160-175 (q scalar-last; beta clamped to [-1+1e-6, 1-1e-6]).
constexpr float kEazyzLo = (float)(-1.0 + 1e-6);
constexpr float kEazyzHi = (float)(1.0 - 1e-6);
template <typename T>
__device__ __forceinline__ T eazyz_lo() { return (T)(-1.0 + 1e-6); }
template <typename T>
__device__ __forceinline__ T eazyz_hi() { return (T)(1.0 - 1e-6); }

template <typename T>
__device__ __forceinline__ void quat_to_eazyz_fwd(const T q[4], T ang[3]) {
  const T a1 = q[1] * q[2] - q[0] * q[3];
  const T b1 = q[0] * q[2] + q[1] * q[3];
  const T cb = ((q[3] * q[3] - q[0] * q[0]) - q[1] * q[1]) + q[2] * q[2];
  const T a3 = q[0] * q[3] + q[1] * q[2];
  const T b3 = q[1] * q[3] - q[0] * q[2];
  ang[0] = atan2(a1, b1);
  ang[1] = acos(fmin(fmax(cb, eazyz_lo<T>()), eazyz_hi<T>()));
  ang[2] = atan2(a3, b3);
}

template <typename T>
__device__ __forceinline__ void quat_to_eazyz_bwd(const T q[4], const T ga[3], T gq[4]) {
  const T a1 = q[1] * q[2] - q[0] * q[3];
  const T b1 = q[0] * q[2] + q[1] * q[3];
  const T cb = ((q[3] * q[3] - q[0] * q[0]) - q[1] * q[1]) + q[2] * q[2];
  const T a3 = q[0] * q[3] + q[1] * q[2];
  const T b3 = q[1] * q[3] - q[0] * q[2];
  const T r1 = a1 * a1 + b1 * b1, r3 = a3 * a3 + b3 * b3;
  const T ga1 = ga[0] * b1 / r1, gb1 = ga[0] * -a1 / r1;
  const T ga3 = ga[2] * b3 / r3, gb3 = ga[2] * -a3 / r3;
  const T x = fmin(fmax(cb, eazyz_lo<T>()), eazyz_hi<T>());
  const bool pass = (cb >= eazyz_lo<T>()) && (cb <= eazyz_hi<T>());
  const T gcb = pass ? (-ga[1] / sqrt(T(1.) - x * x)) : T(0.);
  gq[0] = -q[3] * ga1 + q[2] * gb1 + q[3] * ga3 - q[2] * gb3 - T(2.) * q[0] * gcb;
  gq[1] = q[2] * ga1 + q[3] * gb1 + q[2] * ga3 + q[3] * gb3 - T(2.) * q[1] * gcb;
  gq[2] = q[1] * ga1 + q[0] * gb1 + q[1] * ga3 - q[0] * gb3 + T(2.) * q[2] * gcb;
  gq[3] = -q[0] * ga1 + q[1] * gb1 + q[0] * ga3 + q[1] * gb3 + T(2.) * q[3] * gcb;
}

// ------------------------------------------------ quaternions_to_group_matrix
// lie_tools.py:183-192: normalise, then the reference's (transposed-active) matrix.
template <typename T>
__device__ __forceinline__ void quat_to_mat_fwd(const T q0[4], T R[9]) {
  const T nrm = sqrt(q0[0] * q0[0] + q0[1] * q0[1] + q0[2] * q0[2] + q0[3] * q0[3]);
  const T x = q0[0] / nrm, y = q0[1] / nrm, z = q0[2] / nrm, w = q0[3] / nrm;
  R[0] = ((x * x - y * y) - z * z) + w * w;
  R[1] = T(2.) * (x * y + z * w);
  R[2] = T(2.) * (x * z - y * w);
  R[3] = T(2.) * (x * y - z * w);
  R[4] = ((-x * x + y * y) - z * z) + w * w;
  R[5] = T(2.) * (y * z + x * w);
  R[6] = T(2.) * (x * z + y * w);
  R[7] = T(2.) * (y * z - x * w);
  R[8] = ((-x * x - y * y) + z * z) + w * w;
}

template <typename T>
__device__ __forceinline__ void quat_to_mat_bwd(const T q0[4], const T g[9], T gq[4]) {
  const T nrm = sqrt(q0[0] * q0[0] + q0[1] * q0[1] + q0[2] * q0[2] + q0[3] * q0[3]);
  const T x = q0[0] / nrm, y = q0[1] / nrm, z = q0[2] / nrm, w = q0[3] / nrm;
  T gn[4];
  gn[0] = T(2.) * (x * (g[0] - g[4] - g[8]) + y * (g[1] + g[3]) + z * (g[2] + g[6]) + w * (g[5] - g[7]));
  gn[1] = T(2.) * (-y * (g[0] - g[4] + g[8]) + x * (g[1] + g[3]) - w * (g[2] - g[6]) + z * (g[5] + g[7]));
  gn[2] = T(2.) * (-z * (g[0] + g[4] - g[8]) + w * (g[1] - g[3]) + x * (g[2] + g[6]) + y * (g[5] + g[7]));
  gn[3] = T(2.) * (w * (g[0] + g[4] + g[8]) + z * (g[1] - g[3]) - y * (g[2] - g[6]) + x * (g[5] - g[7]));
  const T dot = gn[0] * x + gn[1] * y + gn[2] * z + gn[3] * w;
  gq[0] = (gn[0] - dot * x) / nrm;
  gq[1] = (gn[1] - dot * y) / nrm;
  gq[2] = (gn[2] - dot * z) / nrm;
  gq[3] = (gn[3] - dot * w) / nrm;
}

// ------------------------------------------------- exp -> ZYZ vector-Jacobian product
// The autograd backward of z = mu @ rodrigues(v) (or z = rodrigues(v)) followed by
// group_matrix_to_eazyz (reparameterize.py:269-273, lie_tools.py:56-64,112-180): g = dL/d
// angles -> gm = dL/dmu (when m != nullptr), gv = dL/dv, in the same operation order as
// the modular kernels lv_so3_exp_fwd + lv_mat_to_eazyz_bwd + lv_so3_exp_bwd (or the
// so3_sample pair), hence bitwise equal to them.  Shared by lv_exp_eazyz_vjp and the
// fused backward tile kernel's tail.
// has_m selects the mu path (a flag, not a nullable pointer: selecting between a local
// array's address and nullptr forces the array into scratch memory).
template <typename T>
__device__ __forceinline__ void exp_eazyz_vjp_sample(const T a[3], bool has_m, const T m[9], const T g[3],
                                                     T gm[9], T gv[3]) {
  // the Rodrigues and quaternion intermediates are computed once and shared by the forward
  // and backward steps (the same operations the modular kernels repeat: same bits)
  T r[9], z[9], q[4], gq[4], gz[9];
  RodPrep<T> rp;
  rodrigues_prep(a, rp);
  rodrigues_fwd_p(rp, r);
  if (has_m) {
    matmul3(m, r, z);
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) z[k] = r[k];
  }
  QuatCase<T> qc;
  mat_to_quat_fwd(z, q, &qc);
  quat_to_eazyz_bwd(q, g, gq);
  mat_to_quat_bwd_qc(q, qc, gq, gz);
  if (has_m) {
    T t[9], gr[9];
    matmul3_nt(gz, r, t);
#pragma unroll
    for (int k = 0; k < 9; ++k) gm[k] = T(0) + t[k];
    matmul3_tn(m, gz, gr);
    rodrigues_bwd_p(a, rp, gr, gv);
  } else {
    rodrigues_bwd_p(a, rp, gz, gv);
  }
}

// The fp32 entry points' VJP: fp32 in and out, the chain itself in fp64, rounded once.  Near
// beta = 0 / pi the chain is ill-conditioned in fp32 -- r1 = a1^2 + b1^2 -> 0 in
// quat_to_eazyz_bwd, and the angle gradients g[0], g[2] cancel to O(beta) -- so its own
// rounding costs up to ~1e-3 of a sample's gradient at beta ~ 1e-2 (as the reference's fp32
// autograd does there); in fp64 every sample stays within ~3e-5 of the fp64 autograd, what
// remains being the fp32 rounding of g.  One dependent chain per sample either way.
__device__ __forceinline__ void exp_eazyz_vjp_sample_wide(const float a[3], bool has_m, const float m[9],
                                                          const float g[3], float gm[9], float gv[3]) {
  double ad[3], gd[3], md[9], gmd[9], gvd[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { ad[k] = a[k]; gd[k] = g[k]; }
  if (has_m) {
#pragma unroll
    for (int k = 0; k < 9; ++k) md[k] = m[k];
  }
  exp_eazyz_vjp_sample<double>(ad, has_m, md, gd, gmd, gvd);
  if (has_m) {
#pragma unroll
    for (int k = 0; k < 9; ++k) gm[k] = (float)gmd[k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) gv[k] = (float)gvd[k];
}

// ------------------------------------------------------------- s2s1rodrigues
// lie_tools.py:67-78: R = I + sin K + (1 - cos) K@K, K = hat(axis), (cos, sin) given.
template <typename T>
__device__ __forceinline__ void s2s1_fwd(const T a[3], const T cs[2], T R[9]) {
  T K[9], K2[9];
  hat_sq(a, K, K2);
  const T omc = T(1.) - cs[0];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const T eye = (i == 0 || i == 4 || i == 8) ? T(1.) : T(0.);
    R[i] = (eye + cs[1] * K[i]) + omc * K2[i];
  }
}

template <typename T>
__device__ __forceinline__ void s2s1_bwd(const T a[3], const T cs[2], const T g[9],
                                         T ga[3], T gcs[2]) {
  T K[9], K2[9];
  hat_sq(a, K, K2);
  T gs = T(0.), gc = T(0.);
#pragma unroll
  for (int i = 0; i < 9; ++i) { gs += g[i] * K[i]; gc -= g[i] * K2[i]; }
  hat_sq_vjp(a, g, cs[1], T(1.) - cs[0], ga);
  gcs[0] = gc;
  gcs[1] = gs;
}

// ------------------------------------------------- s2s2_gram_schmidt (fp64)
// lie_tools.py:81-89 (cross product along the last axis).
__device__ __forceinline__ void cross3d(const double a[3], const double b[3], double c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

struct S2S2State {
  double n1, n1c, e1[3], dot, u2[3], n2, n2c, e2[3], e3[3];
};

__device__ __forceinline__ void s2s2_fwd(const double v1[3], const double v2[3], S2S2State& st) {
  st.n1 = sqrt(v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2]);
  st.n1c = fmax(st.n1, 1e-5);
  for (int i = 0; i < 3; ++i) st.e1[i] = v1[i] / st.n1c;
  st.dot = (st.e1[0] * v2[0] + st.e1[1] * v2[1]) + st.e1[2] * v2[2];
  for (int i = 0; i < 3; ++i) st.u2[i] = v2[i] - st.dot * st.e1[i];
  st.n2 = sqrt(st.u2[0] * st.u2[0] + st.u2[1] * st.u2[1] + st.u2[2] * st.u2[2]);
  st.n2c = fmax(st.n2, 1e-5);
  for (int i = 0; i < 3; ++i) st.e2[i] = st.u2[i] / st.n2c;
  cross3d(st.e1, st.e2, st.e3);
}

__device__ __forceinline__ void s2s2_bwd(const double v1[3], const double v2[3], const double g[9],
                                         double gv1[3], double gv2[3]) {
  S2S2State st;
  s2s2_fwd(v1, v2, st);
  double ge1[3] = {g[0], g[1], g[2]}, ge2[3] = {g[3], g[4], g[5]};
  const double ge3[3] = {g[6], g[7], g[8]};
  double t[3];
  cross3d(st.e2, ge3, t);  // d(e1 x e2)/de1 . g = e2 x g
  for (int i = 0; i < 3; ++i) ge1[i] += t[i];
  cross3d(ge3, st.e1, t);  // d/de2 = g x e1
  for (int i = 0; i < 3; ++i) ge2[i] += t[i];
  // e2 = u2 / clamp(|u2|, 1e-5)
  double gu2[3];
  const double de2 = ge2[0] * st.e2[0] + ge2[1] * st.e2[1] + ge2[2] * st.e2[2];
  const bool pass2 = st.n2 >= 1e-5;
  for (int i = 0; i < 3; ++i) gu2[i] = (ge2[i] - (pass2 ? de2 * st.e2[i] : 0.0)) / st.n2c;
  // u2 = v2 - dot e1 ; dot = <e1, v2>
  double gdot = 0.0;
  for (int i = 0; i < 3; ++i) {
    gv2[i] = gu2[i];
    gdot -= gu2[i] * st.e1[i];
    ge1[i] -= st.dot * gu2[i];
  }
  for (int i = 0; i < 3; ++i) {
    ge1[i] += gdot * v2[i];
    gv2[i] += gdot * st.e1[i];
  }
  // e1 = v1 / clamp(|v1|, 1e-5)
  const double de1 = ge1[0] * st.e1[0] + ge1[1] * st.e1[1] + ge1[2] * st.e1[2];
  const bool pass1 = st.n1 >= 1e-5;
  for (int i = 0; i < 3; ++i) gv1[i] = (ge1[i] - (pass1 ? de1 * st.e1[i] : 0.0)) / st.n1c;
}

// ------------------------------------------------- projection onto SO(3) (extension)
// R = argmin over rotations of |R - M|_F = U diag(1, 1, det UV^T) V^T, by Davenport's
// q-method: tr(R(q)^T M) = q^T K q with the symmetric traceless
//   K = [ M + M^T - tr(M) I   z ;  z^T   tr(M) ],  z = vee(M - M^T),  q = (x, y, z, w),
// whose eigenvalues are {s1+s2+s3', s1-s2-s3', -s1+s2-s3', -s1-s2+s3'} (s3' = s3 det UV^T):
// the top eigenvector is the quaternion of R, lam1 + lam2 = 2 s1 and lam1 - lam2 =
// 2 (s2 + s3'), the gap that conditions the map.  K is diagonalised by a fixed number of
// cyclic Jacobi sweeps, the six (p, q) pairs unrolled so that every entry of K and of the
// eigenvector matrix has a compile-time index and lives in a register; the top column is
// picked by selects.  M is first scaled by the power of two that brings its largest entry
// into [1/2, 1) (exact), so every finite M is handled; ties of the largest eigenvalue go
// to the scalar part first, so M = 0 gives the identity.
template <typename T>
__device__ __forceinline__ constexpr int project_sweeps() { return sizeof(T) == 8 ? 8 : 6; }
// gamma = (s2 + s3')/s1 <= sqrt(eps): the forward has lost half its digits, the backward is masked
template <typename T>
__device__ __forceinline__ constexpr T project_mask() {
  return sizeof(T) == 8 ? T(1.4901161193847656e-08) : T(2.44140625e-04);  // 2^-26, 2^-12
}

template <int P, int Q, typename T>
__device__ __forceinline__ void jacobi_rotate(T (&a)[4][4], T (&v)[4][4]) {
  // t = tan of the rotation angle, the smaller root of t^2 + 2 tau t - 1 = 0 with
  // tau = d / b, written without forming tau: |b| / (|d| + sqrt(d^2 + b^2)), signed as d b.
  // The denominator is >= |b|; holding it there keeps t finite where d = 0 and b^2 underflows
  // (the last sweeps on a matrix with repeated eigenvalues, e.g. K of an exact rotation).
  const T apq = a[P][Q];
  const bool nz = apq != T(0.);
  const T d = a[Q][Q] - a[P][P], b = T(2.) * apq;
  T t = fabs(b) / fmax(fabs(d) + sqrt(d * d + b * b), fabs(b));
  t = ((d >= T(0.)) == (b >= T(0.))) ? t : -t;
  t = nz ? t : T(0.);
  const T c = T(1.) / sqrt(T(1.) + t * t);
  const T s = t * c;
  const T h = t * apq;
  a[P][P] = a[P][P] - h;
  a[Q][Q] = a[Q][Q] + h;
  a[P][Q] = a[Q][P] = T(0.);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r != P && r != Q) {
      const T arp = a[r][P], arq = a[r][Q];
      a[r][P] = a[P][r] = c * arp - s * arq;
      a[r][Q] = a[Q][r] = s * arp + c * arq;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const T vrp = v[r][P], vrq = v[r][Q];
    v[r][P] = c * vrp - s * vrq;
    v[r][Q] = s * vrp + c * vrq;
  }
}

__device__ __forceinline__ float lv_ldexp(float x, int e) { return ldexpf(x, e); }
__device__ __forceinline__ double lv_ldexp(double x, int e) { return ldexp(x, e); }
__device__ __forceinline__ float lv_frexp(float x, int* e) { return frexpf(x, e); }
__device__ __forceinline__ double lv_frexp(double x, int* e) { return frexp(x, e); }

template <typename T>
struct ProjectEig {
  T lam1, lam2;  // the two largest eigenvalues of K (of the scaled M)
};

template <typename T>
__device__ __forceinline__ void so3_project(const T M[9], T R[9], ProjectEig<T>& pe) {
  T mx = fabs(M[0]);
#pragma unroll
  for (int k = 1; k < 9; ++k) mx = fmax(mx, fabs(M[k]));
  int e;
  (void)lv_frexp(mx, &e);
  T m[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = lv_ldexp(M[k], -e);
  const T tr = (m[0] + m[4]) + m[8];
  T a[4][4], v[4][4];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      a[i][j] = i == j ? (m[i * 3 + j] + m[j * 3 + i]) - tr : m[i * 3 + j] + m[j * 3 + i];
  a[0][3] = a[3][0] = m[7] - m[5];
  a[1][3] = a[3][1] = m[2] - m[6];
  a[2][3] = a[3][2] = m[3] - m[1];
  a[3][3] = tr;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) v[r][k] = r == k ? T(1.) : T(0.);
#pragma unroll 1
  for (int sweep = 0; sweep < project_sweeps<T>(); ++sweep) {
    // round-robin order: the two rotations of a line touch disjoint rows and columns, so
    // the second one's angle does not wait for the first (two chains in flight per thread)
    jacobi_rotate<0, 1>(a, v);
    jacobi_rotate<2, 3>(a, v);
    jacobi_rotate<0, 2>(a, v);
    jacobi_rotate<1, 3>(a, v);
    jacobi_rotate<0, 3>(a, v);
    jacobi_rotate<1, 2>(a, v);
  }
  const T d0 = a[0][0], d1 = a[1][1], d2 = a[2][2], d3 = a[3][3];
  int k = 3;
  T best = d3;
  if (d0 > best) { best = d0; k = 0; }
  if (d1 > best) { best = d1; k = 1; }
  if (d2 > best) { best = d2; k = 2; }
  const T q0 = sel4(k, v[0][0], v[0][1], v[0][2], v[0][3]);
  const T q1 = sel4(k, v[1][0], v[1][1], v[1][2], v[1][3]);
  const T q2 = sel4(k, v[2][0], v[2][1], v[2][2], v[2][3]);
  const T q3 = sel4(k, v[3][0], v[3][1], v[3][2], v[3][3]);
  pe.lam1 = best;
  pe.lam2 = fmax(fmax(fmin(d0, d1), fmin(d2, d3)), fmin(fmax(d0, d1), fmax(d2, d3)));
  const T nrm = sqrt((q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3));
  const T x = q0 / nrm, y = q1 / nrm, z = q2 / nrm, w = q3 / nrm;
  R[0] = ((w * w + x * x) - y * y) - z * z;
  R[1] = T(2.) * (x * y - w * z);
  R[2] = T(2.) * (x * z + w * y);
  R[3] = T(2.) * (x * y + w * z);
  R[4] = ((w * w - x * x) + y * y) - z * z;
  R[5] = T(2.) * (y * z - w * x);
  R[6] = T(2.) * (x * z - w * y);
  R[7] = T(2.) * (y * z + w * x);
  R[8] = ((w * w - x * x) - y * y) + z * z;
}

// Backward of the projection: the output is a rotation, so the gradient is the tangent-space
// gradient gM = R hat(u) with (tr(P) I - P) u = vee(R^T gR - gR^T R), P = sym(R^T M), the
// symmetric factor of the polar decomposition (eigenvalues of the system: s_i + s_j with s3'
// signed; neither U nor V is needed).  Solved by cofactors.  Where gamma <= sqrt(eps) the
// sample's gradient is exactly 0.
template <typename T>
__device__ __forceinline__ void so3_project_vjp(const T M[9], const T gR[9], T gM[9]) {
  T R[9], Q[9], G[9];
  ProjectEig<T> pe;
  so3_project(M, R, pe);
  const bool keep = (pe.lam1 - pe.lam2) > project_mask<T>() * (pe.lam1 + pe.lam2);
  matmul3_tn(R, M, Q);
  const T p00 = T(0.5) * (Q[0] + Q[0]), p11 = T(0.5) * (Q[4] + Q[4]), p22 = T(0.5) * (Q[8] + Q[8]);
  const T p01 = T(0.5) * (Q[1] + Q[3]), p02 = T(0.5) * (Q[2] + Q[6]), p12 = T(0.5) * (Q[5] + Q[7]);
  const T tr = (p00 + p11) + p22;
  const T a = tr - p00, b = -p01, c = -p02, d = tr - p11, e = -p12, f = tr - p22;
  const T c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
  const T c11 = a * f - c * c, c12 = b * c - a * e, c22 = a * d - b * b;
  T det = (a * c00 + b * c01) + c * c02;
  det = keep ? det : T(1.);
  matmul3_tn(R, gR, G);
  const T r0 = G[7] - G[5], r1 = G[2] - G[6], r2 = G[3] - G[1];
  T u[3];
  u[0] = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
  u[1] = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
  u[2] = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
  mul_hat(R, u, gM);
#pragma unroll
  for (int k = 0; k < 9; ++k) gM[k] = keep ? gM[k] : T(0.);
}

}  // namespace lv
