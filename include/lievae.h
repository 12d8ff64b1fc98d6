/*
 * lievae.h — C ABI of liblievae_hip.so, the MI355X (gfx950) kernels behind the
 * drop-in `lie_vae` Python API (SO(3) latent hot path of pimdh/lie-vae).
 *
 * The reference has no FFI: its "operator API" is the Python functions of
 * lie_vae/lie_tools.py, the modules of lie_vae/reparameterize.py and
 * lie_vae/decoders.py.  Each entry point below names the reference symbol
 * (file:line under the reference root) it replaces.  The ctypes binding that
 * calls them is lie-vae_amd/lie_vae/_lib.py.
 *
 * Conventions
 *  - All tensor arguments are device pointers to contiguous row-major arrays,
 *    allocated and owned by the caller.  The library never allocates device
 *    memory; backward passes that need scratch take a caller workspace sized
 *    by the matching *_workspace() query.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls
 *    are asynchronous on that stream and never synchronise the host, so they
 *    are safe to capture in a hipGraph.
 *  - Return 0 (LV_OK) or a negative LV_ERR_* code; lv_last_error() returns a
 *    thread-local message for the last failing call on this thread.
 *  - n == 0 is a valid no-op.
 *  - Rotation matrices are (n,3,3); quaternions are scalar-LAST (x,y,z,w) as in
 *    the reference; Euler angles are ZYZ (alpha, beta, gamma).
 */
#ifndef LIEVAE_H_
#define LIEVAE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LV_OK 0
#define LV_ERR_ARG (-1)         /* bad shape / pointer / unsupported size */
#define LV_ERR_HIP (-2)         /* HIP runtime error (launch failure)      */
#define LV_ERR_WORKSPACE (-3)   /* workspace too small                    */

#define LV_DTYPE_F32 0
#define LV_DTYPE_BF16 1

#define LV_MAX_DEGREE 20        /* largest l_max compiled in              */
#define LV_MAX_CHANNELS 64      /* largest rep_copies C per call          */

int lv_abi_version(void);
const char* lv_last_error(void);
int lv_max_degree(void);

/* ---- so(3) exponential: lie_tools.py:56-64 `rodrigues` (a1+a2) --------------
 * v (n,3) -> R (n,3,3).  No small-angle branch: |v| == 0 gives NaN like the
 * reference. */
int lv_so3_exp_fwd(const float* v, float* R, int64_t n, void* stream);
int lv_so3_exp_bwd(const float* v, const float* gR, float* gv, int64_t n, void* stream);

/* ---- SO3reparameterize.nsample: reparameterize.py:269-273 --------------------
 * z[s,b] = mu[b] @ rodrigues(v[s,b]);  v (ns,B,3), mu (B,3,3), z (ns,B,3,3).
 * Backward sums gmu over the ns samples in a fixed order (deterministic). */
int lv_so3_sample_fwd(const float* mu, const float* v, float* z, int64_t ns, int64_t B,
                      void* stream);
int lv_so3_sample_bwd(const float* mu, const float* v, const float* gz, float* gmu, float* gv,
                      int64_t ns, int64_t B, void* stream);

/* ---- backward of z = mu @ exp(v) -> group_matrix_to_eazyz(z) in one pass ----
 * reparameterize.py:269-273 -> vae.py:182 (the fused path's prologue).  mu may be NULL
 * (z = exp(v)); then gmu is not written.  gang (n,3) -> gv (n,3), gmu (n,3,3).
 * The chain runs in fp64 on the fp32 inputs and is rounded once (in fp32 it loses up to
 * ~1e-3 of a sample's gradient near beta = 0 / pi): bitwise lv_so3_exp_fwd_f64 /
 * lv_mat_to_eazyz_bwd_f64 / lv_so3_exp_bwd_f64 in turn on the inputs cast up, rounded to
 * fp32. */
int lv_exp_eazyz_vjp(const float* mu, const float* v, const float* gang, float* gmu, float* gv,
                     int64_t n, void* stream);

/* ---- quaternions_to_group_matrix: lie_tools.py:183-192 (a3) ---------------- */
int lv_quat_to_mat_fwd(const float* q, float* R, int64_t n, void* stream);
int lv_quat_to_mat_bwd(const float* q, const float* gR, float* gq, int64_t n, void* stream);

/* ---- group_matrix_to_quaternions: lie_tools.py:112-157 (a4) -----------------
 * Mirrors the 1e-6 epsilon and the argmax case choice (gradient flows through
 * the chosen case only). */
int lv_mat_to_quat_fwd(const float* R, float* q, int64_t n, void* stream);
int lv_mat_to_quat_bwd(const float* R, const float* gq, float* gR, int64_t n, void* stream);

/* ---- quaternions_to_eazyz: lie_tools.py:160-175 (a5) ----------------------- */
int lv_quat_to_eazyz_fwd(const float* q, float* ang, int64_t n, void* stream);
int lv_quat_to_eazyz_bwd(const float* q, const float* gang, float* gq, int64_t n, void* stream);

/* ---- group_matrix_to_eazyz: lie_tools.py:178-180 (a6 = a4 then a5) --------- */
int lv_mat_to_eazyz_fwd(const float* R, float* ang, int64_t n, void* stream);
int lv_mat_to_eazyz_bwd(const float* R, const float* gang, float* gR, int64_t n, void* stream);

/* ---- s2s1rodrigues: lie_tools.py:67-78 (S2S1Mean, reparameterize.py:167-181) */
int lv_s2s1_fwd(const float* axis, const float* cs, float* R, int64_t n, void* stream);
int lv_s2s1_bwd(const float* axis, const float* cs, const float* gR, float* gaxis, float* gcs,
                int64_t n, void* stream);

/* ---- fp64 twins of the per-sample maps ---------------------------------------
 * The reference's maps follow their input dtype (lie_tools.py:28-38,61: v.new_tensor,
 * eye(dtype=v.dtype)) and its self-tests run them in fp64 (lie_tools.py:271-291).
 * Same contracts as the fp32 entry points above, double pointers. */
int lv_so3_exp_fwd_f64(const double* v, double* R, int64_t n, void* stream);
int lv_so3_exp_bwd_f64(const double* v, const double* gR, double* gv, int64_t n, void* stream);
int lv_so3_sample_fwd_f64(const double* mu, const double* v, double* z, int64_t ns, int64_t B,
                          void* stream);
int lv_so3_sample_bwd_f64(const double* mu, const double* v, const double* gz, double* gmu,
                          double* gv, int64_t ns, int64_t B, void* stream);
int lv_exp_eazyz_vjp_f64(const double* mu, const double* v, const double* gang, double* gmu,
                         double* gv, int64_t n, void* stream);
int lv_quat_to_mat_fwd_f64(const double* q, double* R, int64_t n, void* stream);
int lv_quat_to_mat_bwd_f64(const double* q, const double* gR, double* gq, int64_t n, void* stream);
int lv_mat_to_quat_fwd_f64(const double* R, double* q, int64_t n, void* stream);
int lv_mat_to_quat_bwd_f64(const double* R, const double* gq, double* gR, int64_t n, void* stream);
int lv_quat_to_eazyz_fwd_f64(const double* q, double* ang, int64_t n, void* stream);
int lv_quat_to_eazyz_bwd_f64(const double* q, const double* gang, double* gq, int64_t n,
                             void* stream);
int lv_mat_to_eazyz_fwd_f64(const double* R, double* ang, int64_t n, void* stream);
int lv_mat_to_eazyz_bwd_f64(const double* R, const double* gang, double* gR, int64_t n,
                            void* stream);
int lv_s2s1_fwd_f64(const double* axis, const double* cs, double* R, int64_t n, void* stream);
int lv_s2s1_bwd_f64(const double* axis, const double* cs, const double* gR, double* gaxis,
                    double* gcs, int64_t n, void* stream);

/* ---- so(3) log map: lie_tools.py:100-109 `log_map`, batched and stable -------
 * v = log(R): R (n,3,3) -> v (n,3), |v| in [0, pi].  The reference's expression
 * theta / sin(theta) * (R - R^T)/2 with theta = acos((tr R - 1)/2) is NaN at the identity
 * and has no digits near pi; here theta = atan2(|w|, c) with w = vee(R - R^T)/2 and
 * c = (tr R - 1)/2, v = (theta/|w|) w for c >= 0 (a series near 0: the identity gives exactly
 * 0), and for c < 0 the axis comes from the symmetric part (R + R^T)/2 = c I + (1 - c) a a^T,
 * signed so that a.w >= 0.  At theta = pi exactly (w = 0) both signs are logs of R: the
 * component of largest magnitude is made positive.
 * Backward: the input is a rotation, so the gradient is the tangent-space gradient at R,
 * gR = R hat(u), u = J_r^-T(v) gv / 2, J_r^-1(v) = I + hat(v)/2 + kappa hat(v)^2,
 * kappa = 1/theta^2 - cot(theta/2)/(2 theta); finite up to pi.  Its component normal to SO(3)
 * is zero by definition: composed with a parametrisation that stays in SO(3) it gives the
 * parameter gradients autograd would find through any other formula of the log.
 * Negative sizes, or a null pointer with work to do, return LV_ERR_ARG before any launch;
 * empty sizes return LV_OK with nothing launched. */
int lv_so3_log_fwd(const float* R, float* v, int64_t n, void* stream);
int lv_so3_log_bwd(const float* R, const float* gv, float* gR, int64_t n, void* stream);
/* inverse of lv_so3_sample_fwd: v[s,b] = log(mu[b]^T z[s,b]); mu (B,3,3), z (ns,B,3,3),
 * v (ns,B,3).  Backward: gz = z hat(u), gmu[b] = sum_s mu hat(-Q u) with Q = mu^T z, summed
 * over s in ascending order by one thread per b (bitwise reproducible); ns == 0 zero-fills
 * gmu. */
int lv_so3_rel_log_fwd(const float* mu, const float* z, float* v, int64_t ns, int64_t B,
                       void* stream);
int lv_so3_rel_log_bwd(const float* mu, const float* z, const float* gv, float* gmu, float* gz,
                       int64_t ns, int64_t B, void* stream);
/* rotation angle of A^T B (the geodesic distance): (n,3,3),(n,3,3) -> (n), in [0, pi].
 * Backward: gB = B hat(gtheta a / 2), gA = -A hat(gtheta a / 2), a the unit axis of
 * log(A^T B); exactly 0 where theta = 0 (the kink of a norm). */
int lv_so3_angle_fwd(const float* A, const float* B, float* theta, int64_t n, void* stream);
int lv_so3_angle_bwd(const float* A, const float* B, const float* gtheta, float* gA, float* gB,
                     int64_t n, void* stream);
/* fp64 twins (the per-sample maps follow their input dtype) */
int lv_so3_log_fwd_f64(const double* R, double* v, int64_t n, void* stream);
int lv_so3_log_bwd_f64(const double* R, const double* gv, double* gR, int64_t n, void* stream);
int lv_so3_rel_log_fwd_f64(const double* mu, const double* z, double* v, int64_t ns, int64_t B,
                           void* stream);
int lv_so3_rel_log_bwd_f64(const double* mu, const double* z, const double* gv, double* gmu,
                           double* gz, int64_t ns, int64_t B, void* stream);
int lv_so3_angle_fwd_f64(const double* A, const double* B, double* theta, int64_t n,
                         void* stream);
int lv_so3_angle_bwd_f64(const double* A, const double* B, const double* gtheta, double* gA,
                         double* gB, int64_t n, void* stream);

/* ---- projection onto SO(3) (extension; not in the reference) -- csrc/so3_stats.hip -------
 * R = argmin over rotations of |R - M|_F = U diag(1, 1, det UV^T) V^T for M = U diag(s) V^T:
 * M (n,3,3) -> R (n,3,3).  With s3' = s3 det(UV^T) the map is well defined where
 * s2 + s3' > 0; gamma = (s2 + s3')/s1 is the inverse of its condition number.  Computed by
 * Davenport's q-method (the top eigenvector of a symmetric 4x4 by cyclic Jacobi sweeps), one
 * thread per matrix.  For every finite M the output is a rotation (orthonormal to a few ulp,
 * det > 0, no NaN); where the minimiser is not unique (gamma = 0: M = 0, rank 1, a
 * reflection) the choice is deterministic, and M = 0 gives the identity.
 * Backward: the output is a rotation, so the gradient is the tangent-space gradient
 * gM = R hat(u) with (tr(P) I - P) u = vee(R^T gR - gR^T R), P = sym(R^T M).  Where
 * gamma <= sqrt(eps) of the compute type (2^-12 in fp32, 2^-26 in fp64) the forward itself
 * has lost half its digits: there the sample's gradient is exactly 0 (masked).
 * Negative n, or a null pointer with work to do, return LV_ERR_ARG before any launch. */
int lv_so3_project_fwd(const float* M, float* R, int64_t n, void* stream);
int lv_so3_project_bwd(const float* M, const float* gR, float* gM, int64_t n, void* stream);
int lv_so3_project_fwd_f64(const double* M, double* R, int64_t n, void* stream);
int lv_so3_project_bwd_f64(const double* M, const double* gR, double* gM, int64_t n,
                           void* stream);

/* ---- rotation moment: the reduction behind the chordal mean and both Procrustes steps of
 * pose alignment (extension) ----------------------------------------------------------------
 *   S[s] = sum_i w_i op(X_i) C_s op(Y_i),  s < ns <= 8      S (ns,3,3) double
 *   wsum = sum_i w_i                                          double (may be NULL)
 *   R[s] = project(S[s]), projected in fp64                   (ns,3,3) of the input type (may
 *                                                             be NULL)
 * X, Y (n,3,3); Y NULL = identity; w (n) or NULL = ones; C (ns,3,3) in device memory or NULL =
 * identity with ns = 1; flags: LV_MOMENT_XT / _YT / _CT transpose X_i / Y_i / C_s.  One pass
 * reads X and Y once for all ns constants.  Two launches: partial sums whose grid depends on
 * n alone (each thread adds its samples in ascending order in fp64, each block combines in a
 * fixed order) into the caller's workspace of lv_so3_moment_workspace(n, ns) bytes, then one
 * block that adds the partials in order.  No atomics: the same inputs give the same bits on
 * every run and every device.  n = 0 writes S = 0, wsum = 0 and R = I.
 * n < 0, ns outside [1, 8] (or ns > 1 without C), unknown flags, a null S, a null X with
 * n > 0 or a short workspace return LV_ERR_ARG before any launch. */
#define LV_MOMENT_XT 1
#define LV_MOMENT_YT 2
#define LV_MOMENT_CT 4
size_t lv_so3_moment_workspace(int64_t n, int ns);
int lv_so3_moment(const float* X, const float* Y, const float* w, const float* C, int ns,
                  int flags, double* S, double* wsum, float* R, int64_t n, void* workspace,
                  size_t workspace_bytes, void* stream);
int lv_so3_moment_f64(const double* X, const double* Y, const double* w, const double* C, int ns,
                      int flags, double* S, double* wsum, double* R, int64_t n, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- s2s2_gram_schmidt, fp64: lie_tools.py:81-89 (S2S2Mean, reparameterize.py:184-197)
 * Crosses along the last axis (the reference's torch.cross without dim is
 * wrong at batch 3; documented deviation). */
int lv_s2s2_fwd_f64(const double* v1, const double* v2, double* R, int64_t n, void* stream);
int lv_s2s2_bwd_f64(const double* v1, const double* v2, const double* gR, double* gv1,
                    double* gv2, int64_t n, void* stream);

/* ---- wigner_d_matrix for l = 0..L, packed: lie_tools.py:211-223 (a9) -------
 * ang (n,3) -> D (n, sum_l (2l+1)^2), block l row-major at offset
 * sum_{k<l}(2k+1)^2.  One launch per degree.  The decoder's hot path never materialises
 * D (it applies the factors to the spectrum, a10 below); these entry points serve code
 * written against D itself, and are differentiable in the angles like the reference's
 * tensor expression.  l or L outside 0..LV_MAX_DEGREE, n < 0, an n whose grid would not
 * fit one launch, or (with n > 0) a null pointer return LV_ERR_ARG before anything runs. */
int lv_wigner_d_fwd(const float* ang, float* D, int64_t n, int L, void* stream);
/* VJP of the above: gD (n, sum_l (2l+1)^2) -> gang (n,3).  The per-degree kernels of
 * lv_wigner_d_block_bwd run for l = 0..L in ascending order on the stream; degree 0 writes
 * gang and each later degree adds to it in place (one owning thread per element): a fixed
 * summation order, no atomics, no workspace. */
int lv_wigner_d_bwd(const float* ang, const float* gD, float* gang, int64_t n, int L, void* stream);
/* D_l only: ang (n,3) -> D (n, 2l+1, 2l+1) row-major, one launch; bit for bit block l of
 * lv_wigner_d_fwd. */
int lv_wigner_d_block_fwd(const float* ang, float* D, int64_t n, int l, void* stream);
/* VJP of lv_wigner_d_block_fwd: gD (n, 2l+1, 2l+1) -> gang (n,3).  One lane per (sample,
 * column q) recomputes the chain on e_q and contracts it with gD[s, :, q]; the 2l+1 column
 * partials of a sample are added in ascending q inside the kernel.  A sample's gradient
 * depends only on its own angles and gD -- not on n, its position in the batch or the grid --
 * so it is bitwise reproducible and bitwise equal to the same sample run alone.  Exactly
 * zero at l = 0. */
int lv_wigner_d_block_bwd(const float* ang, const float* gD, float* gang, int64_t n, int l,
                          void* stream);

/* ---- block_wigner_matrix_multiply: lie_tools.py:226-253 (a10) --------------
 * out[s, l^2 + i, c] = sum_j D_l(ang[s])[i,j] (or D^T if transpose) F[s, l^2 + j, c]
 * F is (M, C) shared when F_batch_stride == 0 (ActionNet's expand, decoders.py:53)
 * or (n, M, C) with F_batch_stride == M*C.  M = (L+1)^2, 1 <= C <= 64.
 * out (n, M, C) in out_dtype (LV_DTYPE_F32 | LV_DTYPE_BF16); arithmetic is fp32. */
int lv_group_action_fwd(const float* ang, const float* F, int64_t F_batch_stride, void* out,
                        int out_dtype, int64_t n, int L, int C, int transpose, void* stream);

/* Backward of lv_group_action_fwd (fp32 gout).  gang (n,3).  gF is (M,C) summed
 * over the batch (deterministic two-stage reduction through the workspace) when
 * F_batch_stride == 0, else (n,M,C).  Workspace bytes from the query below.
 * ABI note (version 2 of the workspace contract, round 5): with a shared spectrum the
 * workspace holds the dF slabs AND a 12-byte-per-sample angle-gradient region that only
 * lv_fused_exp_action_bwd writes; both entry points take the same query, so a caller that
 * cached an older (slabs-only) size gets LV_ERR_WORKSPACE -- re-query per (n, L, C).
 * The slab count follows the device's CU count (lv_compute_units), so query on the device
 * the call runs on. */
size_t lv_group_action_bwd_workspace(int64_t n, int L, int C, int shared_F);

/* Compute units of the current HIP device (hipDeviceAttributeMultiprocessorCount, cached
 * per device; 256, the MI355X count, when no device is visible): the persistent
 * backward's grid is 3 blocks per CU, so its plan, workspace and dF summation order
 * follow the part (a CPX partition has fewer CUs). */
int lv_compute_units(void);

/* Launch plans (host only, no kernel launch; for tests and capacity planning; both read the
 * device's CU count as lv_compute_units does: the forward's waves per block and the
 * backward's persistent grid follow it).  plan[] gets
 * LV_PLAN_LEN values: [0] forward: tile kernel (1) or grid-stride kernel (0); backward:
 * spectrum mode (0 per-sample, 1 shared in LDS, 2 shared from global memory with the dF
 * slab in the workspace -- the large-tile fallback, 3 the persistent kernel: C = 10,
 * 3 <= l <= 10, shared spectrum, from CUs + 1 six-sample groups (257 on MI355X), a grid
 * of min(groups, 3 * CUs) blocks, one dF slab per block), [1] grid blocks,
 * [2] degree segments, [3] threads per block, [4] dynamic LDS bytes per block,
 * [5] samples per block group, [6] forward: write-through stores / backward: workspace
 * bytes, [7..23] segment boundaries seg_lo[0..segments] (then -1), [24..39] the degree
 * set of wave k (bit l = degree l; 0 past the last wave): the kernels run these sets --
 * contiguous ranges seg_lo where a kernel stages per-wave spectrum rows, cost-balanced
 * sets otherwise.  n > 0. */
#define LV_PLAN_LEN 40
int lv_action_fwd_plan(int fused, int64_t F_batch_stride, int out_dtype, int64_t n, int L, int C,
                       int64_t* plan);
int lv_group_action_bwd_plan(int64_t n, int L, int C, int shared_F, int64_t* plan);
int lv_group_action_bwd(const float* ang, const float* F, int64_t F_batch_stride,
                        const float* gout, float* gang, float* gF, int64_t n, int L, int C,
                        int transpose, void* workspace, size_t ws_bytes, void* stream);

/* ---- fused metric kernel: z = mu @ rodrigues(v) -> ZYZ -> block D(z)·F ------
 * reparameterize.py:269-273 + vae.py:182 + decoders.py:47-56 in one pass.
 * mu (n,3,3) or NULL (identity); v (n,3); optional ang_out (n,3) receives the
 * Euler angles (for the backward; beta = atan2(sin, cos) of the pair D is evaluated with,
 * accurate near 0 / pi where acos of an fp32 cosine is not).  Other arguments as
 * lv_group_action_fwd. */
int lv_fused_exp_action_fwd(const float* mu, const float* v, const float* F,
                            int64_t F_batch_stride, void* out, int out_dtype, float* ang_out,
                            int64_t n, int L, int C, int transpose, void* stream);
/* Its backward in two launches (shared spectrum): the group-action backward writes the
 * angle gradient to the workspace, and the exp -> ZYZ VJP runs per sample in the dF
 * reduce's launch, beside the reduce;
 * gmu (n,3,3, when mu is given), gv (n,3), gF (M,C).  Bitwise equal to
 * lv_group_action_bwd + lv_exp_eazyz_vjp.  ang = the forward's ang_out; workspace as
 * lv_group_action_bwd_workspace(n, L, C, 1). */
int lv_fused_exp_action_bwd(const float* mu, const float* v, const float* ang, const float* F,
                            const float* gout, float* gmu, float* gv, float* gF, int64_t n, int L,
                            int C, int transpose, void* workspace, size_t ws_bytes, void* stream);

/* ---- N0reparameterize: reparameterize.py:100-145 (a12) ---------------------
 * sigma = softplus(h) (beta 1, threshold 20), h/sigma (B,3). */
int lv_softplus_fwd(const float* h, float* sigma, int64_t n, void* stream);
int lv_softplus_bwd(const float* h, const float* gsigma, float* gh, int64_t n, void* stream);
/* v[s,b,:] = eps[s,b,:] * sigma[b,:]; backward sums gsigma over s (deterministic). */
int lv_n0_sample_fwd(const float* sigma, const float* eps, float* v, int64_t ns, int64_t B,
                     void* stream);
int lv_n0_sample_bwd(const float* eps, const float* gv, float* gsigma, int64_t ns, int64_t B,
                     void* stream);

/* ---- SO3reparameterize.log_posterior: reparameterize.py:233-263 (a13+a15) ---
 * v (ns,B,3), sigma (B,3) -> out (ns,B): logsumexp over the 2k+1 wrapped terms. */
int lv_so3_log_posterior_fwd(const float* v, const float* sigma, float* out, int64_t ns,
                             int64_t B, int k, void* stream);
int lv_so3_log_posterior_bwd(const float* v, const float* sigma, const float* gout, float* gv,
                             float* gsigma, int64_t ns, int64_t B, int k, void* stream);
/* Host-only dispatch of the two entries above (no GPU call; refuses the same sizes and k).
 * k must lie in [0, 64].  Two kernels per direction: a wave per element (lane t holds wrapped
 * term t - k) and a thread per element (the 2k+1 terms in a loop).  The forward takes the
 * wave kernel when k <= 31 and 0 < ns*B <= 65536; the backward works per b (it sums gsigma
 * over s) and takes the wave kernel when k <= 31 and 0 < B <= 65536, ns > 0; otherwise the
 * thread kernel.  ns == 0: the backward only zeroes gsigma (v, gout, gv may be null).
 * plan[0] fwd_wave, [1] bwd_wave, [2] fwd_blocks, [3] bwd_blocks (0: nothing launched),
 * [4] threads per block. */
#define LV_SO3_LOG_POSTERIOR_PLAN_LEN 5
int lv_so3_log_posterior_plan(int64_t ns, int64_t B, int k, int64_t* plan);

/* ---- Sreparameterize, the vMF latent on S^3: reparameterize.py:58-97 (csrc/vmf.hip) -----
 * Latent modes vmf / vmfq.  m = 4 only.  mu (B,4) unit vectors, kappa (B) > 0 (the module
 * gives softplus + 1 >= 1; 4 kappa^2 must stay finite in fp32).  All entry points:
 * ns == 0 or B == 0 is LV_OK with nothing launched; negative sizes, trials outside 1..64 or a
 * null pointer with work to do return LV_ERR_ARG before any launch.
 *
 * Sampler (Ulrich 1984 / Wood 1994, rejection from standard normals alone): noise
 * (ns, B, 6 trials + 3); trial t owns g[0..3] = noise[6t .. 6t+3] and h[0..1] =
 * noise[6t+4 .. 6t+5], the last three values are the tangent direction.  eps = (1 + g0/|g|)/2
 * ~ Beta(3/2, 3/2); the trial is accepted iff 3 ln t - t + d >= -(h0^2 + h1^2)/2 with Wood's
 * a, b, d and t = 2ab / (1 - (1 - b) eps).  The first accepted trial wins: accepted (ns, B)
 * gets its index, or the value `trials` when none was accepted and the last proposal was
 * used (probability <= 0.3125^trials).  One launch, a loop bounded by `trials`, no host sync.
 * z (ns, B, 4) = the reflection taking e1 to mu applied to (w, sqrt(1 - w^2) v). */
int lv_vmf_sample_fwd(const float* mu, const float* kappa, const float* noise, float* z,
                      int32_t* accepted, int64_t ns, int64_t B, int trials, void* stream);
/* Pathwise gradient (the accepted proposal held fixed; the acceptance-correction term of the
 * rejection-reparameterisation estimator is left out): gz (ns, B, 4) -> gmu (B, 4), gkappa
 * (B), each summed over the ns samples of a datum in ascending s by one thread (no atomics,
 * bitwise reproducible).  Re-reads the accepted trial's six normals from noise. */
int lv_vmf_sample_bwd(const float* mu, const float* kappa, const float* noise,
                      const int32_t* accepted, const float* gz, float* gmu, float* gkappa,
                      int64_t ns, int64_t B, int trials, void* stream);
/* KL(vMF(mu, kappa) || U(S^3)) = kappa A + ln C + ln(2 pi^2), A = I_2 / I_1, ln C = ln kappa
 * - 2 ln 2pi - ln I_1(kappa); kl (B).  Evaluated per datum in fp64 from exponentially scaled
 * Bessel values (ascending series below kappa = 20, Hankel's asymptotic series above) and
 * rounded once.  Backward: gkappa = gkl kappa A', A' = 1 - A^2 - 3A / kappa. */
int lv_vmf_kl_fwd(const float* kappa, float* kl, int64_t B, void* stream);
int lv_vmf_kl_bwd(const float* kappa, const float* gkl, float* gkappa, int64_t B, void* stream);
/* log q(z) = ln C + kappa mu.z, evaluated as (ln C + kappa) - kappa |z - mu|^2 / 2 (no lost
 * digits near the mode at large kappa; equal for unit mu and z); z (ns, B, 4), out (ns, B).
 * Backward: gout (ns, B) -> gmu (B, 4), gkappa (B) (summed over s in ascending order), gz
 * (ns, B, 4), mu and z treated as free 4-vectors. */
int lv_vmf_log_prob_fwd(const float* mu, const float* kappa, const float* z, float* out,
                        int64_t ns, int64_t B, void* stream);
int lv_vmf_log_prob_bwd(const float* mu, const float* kappa, const float* z, const float* gout,
                        float* gmu, float* gkappa, float* gz, int64_t ns, int64_t B, void* stream);

/* ---- timing helper for bench.py: K back-to-back launches of the fused kernel
 * from C, so the host-side launch cost is not Python's.  Same arguments as
 * lv_fused_exp_action_fwd plus the repeat count. */
int lv_fused_exp_action_fwd_repeat(const float* mu, const float* v, const float* F,
                                   int64_t F_batch_stride, void* out, int out_dtype,
                                   float* ang_out, int64_t n, int L, int C, int transpose,
                                   int repeats, void* stream);

/* ---- decoder ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1) on MFMA (§8 f1) -----
 * Replaces the MIOpen transposed convolution behind nn.ConvTranspose2d.forward for the
 * DeconvNet upsampling layers (reference experiments/nets.py:60-75), bf16 NHWC in/out,
 * fp32 accumulate.  Cin % 8 == 0, Cout % 4 == 0, Cout <= 208.  The weight (Cin, Cout, 4, 4)
 * bf16 is first repacked into lv_deconv4s2_packed_weight_elems(Cin) bf16 elements (four
 * output phases x 208 channels x 4*Cin taps, + 64 zero bytes); bias (Cout) fp32 or NULL.
 * The same call computes the input gradient of Conv2d(Cout, Cin, 4, 2, 1) (the encoder's
 * strided convolutions, nets.py:33-57): gx = conv_transpose2d(gy, W) with the Conv2d
 * weight W (Cin_conv_out, Cout_conv_in, 4, 4) read as this layer's (Cin, Cout, 4, 4). */
size_t lv_deconv4s2_packed_weight_elems(int Cin);
int lv_deconv4s2_pack_weight_bf16(const void* w, void* wt, int Cin, int Cout, void* stream);
int lv_deconv4s2_fwd_bf16(const void* x, const void* wt, const float* bias, void* y, int64_t N,
                          int H, int W, int Cin, int Cout, void* stream);
/* The same layer with Cout <= 4 (the decoder's RGB output layer, nets.py:74): one GEMM row
 * per output quad over the 3x3 input neighbourhood, all four phases x Cout in one 16-wide
 * MFMA tile.  Weight repacked into lv_deconv4s2_small_packed_weight_elems(Cin) bf16. */
size_t lv_deconv4s2_small_packed_weight_elems(int Cin);
int lv_deconv4s2_small_pack_weight_bf16(const void* w, void* wq, int Cin, int Cout, void* stream);
int lv_deconv4s2_small_fwd_bf16(const void* x, const void* wq, const float* bias, void* y,
                                int64_t N, int H, int W, int Cin, int Cout, void* stream);
/* Backward of the small-Cout layer: gx (dgrad; needs the weight repacked by
 * lv_deconv4s2_small_pack_dgrad_weight_bf16 into lv_deconv4s2_small_dgrad_weight_elems(Cin)
 * bf16), gw (bf16, the weight's (Cin, Cout, 4, 4) layout) and gb (fp32, optional, only with
 * gw) from x and gy (bf16 channels-last).  gx or gw may be null to skip that product; gw
 * needs ws of lv_deconv4s2_small_bwd_workspace_elems(...) floats.  Cin + 1 <= 256. */
size_t lv_deconv4s2_small_dgrad_weight_elems(int Cin);
int lv_deconv4s2_small_pack_dgrad_weight_bf16(const void* w, void* wd, int Cin, int Cout, void* stream);
size_t lv_deconv4s2_small_bwd_workspace_elems(int64_t N, int H, int W, int Cin, int Cout);
int lv_deconv4s2_small_bwd_bf16(const void* x, const void* gy, const void* wd, void* gx, void* gw, float* gb,
                                float* ws, int64_t N, int H, int W, int Cin, int Cout, void* stream);
/* out[c] = sum_p g[p, c] for a channels-last (P, C) bf16 tensor (the bias gradient of a
 * convolution), C % 8 == 0; fixed-order (deterministic) two-pass sum, ws of
 * lv_channel_sum_workspace_elems(P, C) floats. */
size_t lv_channel_sum_workspace_elems(int64_t P, int C);
int lv_channel_sum_bf16(const void* g, float* out, float* ws, int64_t P, int C, void* stream);
/* ---- encoder BatchNorm2d + LeakyReLU (csrc/bn.hip; reference nets.py:33-57) ------------
 * x: channels-last (P, C) bf16, P = N·H·W.  Supported when lv_bn_supported(P, C): C >= 8,
 * C / gcd(C, 8) <= 256 and P a multiple of 8 / gcd(C, 8).  training = 1: batch statistics
 * (biased variance), save_mean / save_invstd written, running stats (may be null) updated
 * with `momentum` (unbiased variance), as torch.nn.BatchNorm2d; training = 0: the running
 * statistics normalise.  y = z > 0 ? z : slope·z, z = gamma·(x - mean)·invstd + beta
 * (gamma / beta null = 1 / 0).  ws: lv_bn_workspace_elems(P, C) floats.  Deterministic. */
int lv_bn_supported(int64_t P, int C);
size_t lv_bn_workspace_elems(int64_t P, int C);
int lv_bn_lrelu_fwd_bf16(const void* x, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, int training, float momentum, float eps, float slope, void* y,
                         float* save_mean, float* save_invstd, float* ws, int64_t P, int C, void* stream);
/* Backward of the training-mode forward: gx (bf16), ggamma / gbeta (fp32, may be null). */
int lv_bn_lrelu_bwd_bf16(const void* g, const void* x, const float* gamma, const float* beta,
                         const float* save_mean, const float* save_invstd, float slope, void* gx,
                         float* ggamma, float* gbeta, float* ws, int64_t P, int C, void* stream);
/* acc[i] += (float)g[i], i < n: a bf16 parameter gradient (the autocast copy's) added in
 * place into its fp32 master gradient, one pass (replaces the cast + AccumulateGrad add pair
 * of torch.autocast's weight casts in the bf16 training step; deterministic). */
int lv_accumulate_bf16_f32(const void* g, float* acc, int64_t n, void* stream);
/* Fused ReLU around the decoder layers (DeconvNet's nn.ReLU, nets.py:62-72), flags:
 *   LV_DECONV_RELU_OUT  y = max(conv_transpose(x) + b, 0) (the ReLU after the layer);
 *   LV_DECONV_MASK_GX   (backward, small-Cout layer) gx masked by x > 0 only: x is already a
 *                       ReLU output (e.g. written with LV_DECONV_RELU_OUT), so forward and
 *                       wgrad need no max and gx is the gradient w.r.t. the ReLU's input. */
#define LV_DECONV_RELU_OUT 1
#define LV_DECONV_MASK_GX 4
int lv_deconv4s2_fwd_bf16_ex(const void* x, const void* wt, const float* bias, void* y, int64_t N,
                             int H, int W, int Cin, int Cout, int flags, void* stream);
int lv_deconv4s2_small_bwd_bf16_ex(const void* x, const void* gy, const void* wd, void* gx, void* gw,
                                   float* gb, float* ws, int64_t N, int H, int W, int Cin, int Cout,
                                   int flags, void* stream);
/* The same layer in fp32 (the reference trains in fp32: unsupervised.py:108-117), on fp32
 * MFMA (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulate).  x channels-last
 * (N, H, W, Cin) fp32, y NCHW (N, Cout, 2H, 2W) fp32; Cin % 4 == 0, 1 <= Cout <= 208.  The
 * weight (Cin, Cout, 4, 4) fp32 repacked into lv_deconv4s2_packed_weight_elems_f32(Cin)
 * floats; bias (Cout) or NULL; flags 0 or LV_DECONV_RELU_OUT.  y_cl (or NULL, Cout % 4 == 0):
 * the same output also channels-last (N, 2H, 2W, Cout), e.g. the next such layer's x. */
size_t lv_deconv4s2_packed_weight_elems_f32(int Cin);
int lv_deconv4s2_pack_weight_f32(const float* w, float* wt, int Cin, int Cout, void* stream);
int lv_deconv4s2_fwd_f32(const float* x, const float* wt, const float* bias, float* y, float* y_cl,
                         int64_t N, int H, int W, int Cin, int Cout, int flags, void* stream);

/* ---- encoder regularisers (csrc/image.hip) ---------------------------------------------
 * EquivarianceLoss.rotate: losses/equivariance_loss.py:50-57 (affine_grid + grid_sample in
 * one pass).  img, out (N, C, H, W) fp32; cs (N, 2) = (cos, sin) of each image's angle, the
 * convention of the s2s1 map above.  out[n, c] = img[n, c] sampled bilinearly, zeros outside,
 * at the positions the affine matrix [[c, -s, 0], [s, c, 0]] gives in normalised
 * coordinates, under either align_corners convention (0: torch's present default, what the
 * reference runs with today; 1: the default when it was written; equal to rounding for
 * H == W).  Positions are evaluated in pixel space about the image centre, so (c, s) =
 * (1, 0) copies the input bit for bit, (-1, 0) is the exact half turn, and (0, +-1) are the
 * exact quarter turns when H == W.  A plane of at most 64 KB is staged in LDS by one block
 * per (n, c); larger planes, or flags & LV_ROTATE_DIRECT, read their taps from global
 * memory.  Both paths give the same bits.  No backward: the reference never differentiates
 * the image, and the angles carry no gradient.  N * C <= INT_MAX. */
#define LV_ROTATE_DIRECT 1
int lv_rotate_bilinear_fwd(const float* img, const float* cs, float* out, int64_t N, int C, int H,
                           int W, int align_corners, int flags, void* stream);
/* Host-only dispatch of the call above: plan[0] staged path (1) or direct (0), [1] grid
 * blocks, [2] threads per block, [3] dynamic LDS bytes per block. */
#define LV_ROTATE_PLAN_LEN 4
int lv_rotate_plan(int64_t N, int C, int H, int W, int flags, int64_t* plan);
/* EquivarianceLoss.forward: losses/equivariance_loss.py:28-36 with lie_tools.py:67-78.
 * diffs[n] = sum_ij (g_n enc_n - enc_rot_n)_ij^2, g_n the rotation about the x axis by the
 * angle of cs[n] = (cos, sin); cs (n, 2), enc and enc_rot (n, 3, 3), diffs (n).  The backward
 * takes gdiffs (n) and writes g_enc and g_enc_rot (n, 3, 3). */
int lv_equivariance_diff_fwd(const float* cs, const float* enc, const float* enc_rot, float* diffs,
                             int64_t n, void* stream);
int lv_equivariance_diff_bwd(const float* cs, const float* enc, const float* enc_rot,
                             const float* gdiffs, float* g_enc, float* g_enc_rot, int64_t n,
                             void* stream);
/* EncoderContinuityLoss.forward: losses/encoder_continuity_loss.py:18-20.  enc (rows, D),
 * rows even; rows 2i and 2i+1 are a pair: diffs[i] = sum_k (enc[2i, k] - enc[2i+1, k])^2,
 * diffs (rows / 2).  The backward takes gdiffs (rows / 2) and writes g_enc (rows, D). */
int lv_pair_sqdist_fwd(const float* enc, float* diffs, int64_t rows, int D, void* stream);
int lv_pair_sqdist_bwd(const float* enc, const float* gdiffs, float* g_enc, int64_t rows, int D,
                       void* stream);

/* ---- sphere-cube renderer (csrc/render.hip) ----------------------------------------------
 * The images the reference's SphereCubeDataset / ScPairsDataset read from disk
 * (experiments/datasets.py:87-127, rendered there by Blender from cube.blend), rendered on the
 * device from the poses instead.  The scene is this project's own: the
 * cube [-1,1]^3 with one albedo per face and a sphere of radius 0.6 at (0,0,1) in a fixed
 * object frame, Lambert + ambient light from (1,2,3)/sqrt(14); the pose is the CAMERA frame
 * (position 5 R[:,2], looking along -z of R, +y of R up, half-width 0.4 at unit distance).
 * R (n,3,3) -> out (n, channels, size, size) fp32 in [0, 1], channels 3 (RGB) or 1 (the mean
 * of the three); a pixel is the mean of samples x samples regular sub-samples.  One launch:
 * a thread traces a run of 4 consecutive pixels (size % 4 == 0 and a 16-byte aligned out;
 * float4 stores) or 1 pixel (otherwise, or with LV_RENDER_SCALAR) once and writes every
 * channel from that trace; both give the same bits.  Forward only.  Every R, finite or not,
 * gives a finite image and no fault: no address depends on a computed value.
 * n < 0, size outside 1..1024, channels not 1 or 3, samples outside 1..4, unknown flags, a
 * null pointer with n > 0, or n * channels * size^2 * 4 beyond INT64_MAX return LV_ERR_ARG
 * before any launch. */
#define LV_RENDER_SCALAR 1
int lv_render_spherecube_fwd(const float* R, float* out, int64_t n, int size, int channels,
                             int samples, int flags, void* stream);
/* Host-only dispatch of the call above (for an aligned out): plan[0] four-pixel path (1) or
 * one-pixel (0), [1] grid blocks = min(65536, n * ceil(runs / 256)) with runs = size^2 / 4 or
 * size^2 per image (blocks stride over the rest), [2] threads per block, [3] dynamic LDS bytes
 * per block. */
#define LV_RENDER_PLAN_LEN 4
int lv_render_plan(int64_t n, int size, int channels, int samples, int flags, int64_t* plan);

/* ---- triangle-mesh renderer (csrc/render_mesh.hip) --------------------------------------
 * The images the reference's ShapeDataset reads from directories of rendered ShapeNet objects
 * (experiments/datasets.py:18-85), rendered on the device from triangle meshes and poses
 * instead.  Camera, sub-samples, light and shading are those of the
 * sphere-cube renderer above, so the two are interchangeable; shading is flat with one albedo
 * per triangle, and meshes are two-sided (a triangle seen from behind is lit on that side;
 * nothing is culled by winding).
 *
 * Packing: verts (V,3) fp32, faces (T,3) int32, albedo (T,3) fp32 (clamped to [0, 1]) ->
 * records (T,16) fp32, 16-byte aligned: v0, e1 = v1 - v0, e2 = v2 - v0, front rgb, back rgb,
 * 0, with n = (e1 x e2)/|e1 x e2|, front = albedo (0.3 + 0.7 max(0, n.l)),
 * back = albedo (0.3 + 0.7 max(0, -n.l)), l = (1,2,3)/sqrt(14).  A face index outside [0, V)
 * is never used as an address: that triangle's record is all zeros (never hit) and
 * *bad_counter (int32, device, zeroed by the caller) is incremented.  A triangle whose
 * |e1 x e2| is zero, infinite or NaN gets zero edges and zero colours and is never hit.  T == 0 is a no-op.  V outside 0..(2^31-1)/3 or T
 * outside 0..(2^31-1)/16 return LV_ERR_ARG. */
int lv_mesh_pack(const float* verts, int64_t V, const int32_t* faces, const float* albedo,
                 int64_t T, float* records, int32_t* bad_counter, void* stream);
/* Rendering: R (n,3,3), mesh_id (n) int64 or NULL (every image shows mesh 0), records
 * (total_records,16) holding K meshes back to back, ranges (K,2) int32 = (first record, count)
 * per mesh, all on the device -> out (n, channels, size, size) fp32 in [0, 1].  A ray walks
 * its mesh's triangles in index order (Moeller-Trumbore; the nearest hit wins, the lower index
 * among equal distances; background 0).  An image whose id is outside [0, K), or whose range
 * leaves [0, total_records), renders the background: no input can make the kernel read or
 * write out of bounds, and every R and vertex, finite or not, gives a finite image.  One
 * launch: runs of 4 pixels with float4 stores (size % 4 == 0 and a 16-byte aligned out) or of
 * 1 pixel (otherwise, or with LV_MESH_SCALAR), the same bits.  max_blocks caps the grid below
 * the default 65536 (0 = default); blocks stride over the remaining tiles.  Forward only.
 * n < 0, size outside 1..1024, channels not 1 or 3, samples outside 1..4, K < 1,
 * total_records outside 0..2^31-1, unknown flags, max_blocks < 0, a null or misaligned pointer
 * with n > 0, or n * channels * size^2 * 4 beyond INT64_MAX return LV_ERR_ARG before any
 * launch. */
#define LV_MESH_SCALAR 1
int lv_render_mesh_fwd(const float* R, const int64_t* mesh_id, const float* records,
                       const int32_t* ranges, int K, int64_t total_records, float* out, int64_t n,
                       int size, int channels, int samples, int flags, int64_t max_blocks,
                       void* stream);
/* Host-only: the checks and dispatch of the call above (for an aligned out), and, when
 * host_ranges (K,2) is not NULL, a check of every range against total_records (a packer calls
 * this before it accepts its ranges; LV_ERR_ARG names the first range that leaves the
 * records).  plan[0] four-pixel path (1) or one-pixel (0), [1] grid blocks =
 * min(cap, n * ceil(runs / 256)), cap = max_blocks if 0 < max_blocks < 65536 else 65536,
 * [2] threads per block, [3] dynamic LDS bytes per block. */
#define LV_RENDER_MESH_PLAN_LEN 4
int lv_render_mesh_plan(const int32_t* host_ranges, int K, int64_t total_records, int64_t n,
                        int size, int channels, int samples, int flags, int64_t max_blocks,
                        int64_t* plan);

/* ---- spherical harmonics on S^2 (csrc/s2.hip) --------------------------------------------
 * The signal behind the action decoder's spectrum (experiments/main.py:169, "the virtual
 * signal on the Sphere"): f(x) = sum_k F_k Y_k(x), and the way back.  The reference
 * has neither; the basis is the one its J tables belong to.  All fp32, L in 0..LV_MAX_DEGREE,
 * M = (L+1)^2, C in 1..LV_MAX_CHANNELS.
 *
 * Basis: orthonormal real harmonics without the Condon-Shortley phase, flat index
 * k = l^2 + l + m, m = -l..l, m < 0 sine-type and m > 0 cosine-type; Y_0 = 1/sqrt(4 pi) and
 * degree 1 is sqrt(3/(4 pi)) (y, z, x).  Evaluated as Y_l^{+-m} = sqrt2 q_l^m(z) {Re, Im}(x+iy)^m
 * with q_l^m a polynomial in z from a three-term recurrence in l: no trigonometric call, no
 * division by sin(theta).  With g = Rz(a) Ry(b) Rz(c), Y_l(g x) = D_l(a, b, c) Y_l(x) for the D
 * of lv_wigner_d_fwd, so synthesis(D(a) F, x) = synthesis(F, g^T x).
 *
 * Points x (P,3) need not be unit vectors: they are normalised in the kernel (first by the
 * largest component, so no length overflows).  At +-z every m != 0 entry is exactly 0.  The
 * zero vector and a point with a non-finite component have no direction: every harmonic of
 * such a point is NaN (Y_0 too), hence its row of Y, its synthesis values, and -- a sum over
 * all points -- every coefficient the analysis returns for a batch that has a value there.
 * No address depends on a point's value.
 *
 * lv_s2_harmonics_fwd: x (P,3) -> Y (P,M).
 * lv_s2_synthesis_fwd: values[b,p,c] = sum_k Y_k(x_p) F[b,k,c].  F (B,M,C) with F_batch_stride
 * = M*C, or one shared (M,C) block with F_batch_stride = 0 (as lv_group_action_fwd takes its
 * spectrum); x is shared by the batch; values (B,P,C).  Y stays in registers; the (M, tile)
 * coefficient block of one batch element is staged once per block in LDS.  The two stride
 * forms of the same spectrum give the same bits.
 * lv_s2_analysis_fwd, the adjoint: F[b,k,c] = sum_p w_p Y_k(x_p) values[b,p,c]; w (P) or NULL
 * (ones); values (B,P,C) -> F (B,M,C).  No atomics: one wave per partial sums its points in a
 * fixed order into the workspace (lv_s2_analysis_workspace bytes), a second launch adds the
 * partials in ascending order; the same inputs give the same bits on every run.
 * B == 0 or P == 0 succeed and launch nothing (the analysis then leaves F unwritten: the
 * caller zeroes an empty sum).  L or C outside their ranges, a negative count, an
 * F_batch_stride other than 0 or M*C, a null pointer or a short workspace with a non-empty
 * problem, and sizes whose byte offsets or grid leave the int64 / 2^31-1 block range return
 * LV_ERR_ARG before any launch. */
int lv_s2_harmonics_fwd(const float* x, float* Y, int64_t P, int L, void* stream);
int lv_s2_synthesis_fwd(const float* F, int64_t F_batch_stride, const float* x, float* values,
                        int64_t B, int64_t P, int L, int C, void* stream);
size_t lv_s2_analysis_workspace(int64_t B, int64_t P, int L, int C);
int lv_s2_analysis_fwd(const float* values, const float* x, const float* w, float* F, int64_t B,
                       int64_t P, int L, int C, void* workspace, size_t workspace_bytes,
                       void* stream);
/* Host-only dispatch of the three calls above (B and C are ignored for the basis): plan[0]
 * channels a lane accumulates (the channel tile: 1, 2, 4, 8 or 16; 0 for the basis), [1] grid
 * blocks, [2] threads per block (synthesis: 64 while 256-thread blocks would number at most
 * 512, else 256; analysis: 64, one wave per partial), [3] LDS bytes per block (the
 * recurrence's tables, plus M * tile * 4 for the synthesis), [4] analysis: partial sums per
 * coefficient = min(ceil(P / 64), ceil(2048 / (B * ceil(C / tile)))), a function of the shape
 * alone, [5] analysis: blocks of the second launch. */
#define LV_S2_OP_HARMONICS 0
#define LV_S2_OP_SYNTHESIS 1
#define LV_S2_OP_ANALYSIS 2
#define LV_S2_PLAN_LEN 6
int lv_s2_plan(int op, int64_t B, int64_t P, int L, int C, int64_t* plan);

#ifdef __cplusplus
}
#endif
#endif /* LIEVAE_H_ */
