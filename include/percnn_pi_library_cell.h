/* C-ABI of the library cell: Stage-3 rollouts of any equation over the Stage-2 candidate library -- part of libpercnn_pi.so.
 *
 * The reference writes one fine_tuning_*.py per discovered equation (2D_Burgers_eqn/Stage-3, 2D_Lambda_Omega_eqn/stage-3);
 * this is the explicit Euler step of those scripts for ANY equation  percnn_pi_library_moments / STRidge  can return:
 *
 *   next_s = h_s + dt * sum_{k=0..6} psi_k * q_{s,k},      q_{s,k} = sum_{m=0..9} C[s][m][k] * phi_m       s = u, v
 *   phi = [1, u, v, u^2, uv, v^2, u^3, u^2 v, u v^2, v^3]     psi = [1, u_x, u_y, v_x, v_y, lap_u, lap_v]
 *
 * C[s][m][k] is the coefficient of library term 7m + k (percnn_pi_discovery.h: theta[7a + b] = A_a * B_b) in the equation of
 * species s, in physical units.  u_x is the 4th-order central first derivative along grid axis 0 (rows), u_y along axis 1,
 * lap the 4th-order star; the stencils wrap (periodic) and are evaluated with the expressions of the Stage-2 library:
 *   d   = ((f[-2] - f[+2]) + 8 (f[+1] - f[-1])) * (1 / (12 dx))
 *   lap = ((-1/12) ((a2 + b2) + (l2 + r2)) + (4/3) ((a1 + b1) + (l1 + r1)) - 5 c) * (1 / dx^2)     a/b: axis 0, l/r: axis 1
 * The forward step's operation order is fixed: u2 = u*u, uv = u*v, v2 = v*v, u3 = u2*u, u2v = u2*v, uv2 = u*v2, v3 = v2*v;
 * q summed over m = 0..9 in order; rhs summed over k = 0..6 in order; inc = dt*rhs; next = h + inc; plain multiplies and adds.
 * A column k whose ten coefficients are all zero is skipped (the same bits for finite inputs, up to the sign of a zero).
 *
 * The reference's Stage-3 cells also define a classical Runge-Kutta step (forward_rk4).  With f(y) the right-hand side above
 * (rhs, evaluated exactly as the Euler step evaluates it, skipped columns included), the percnn_pi_lib_rk4_* entry points take
 * one such step per launch in this fixed order:
 *   k1 = f(h)         y2 = h + (k1*dt)/2.0
 *   k2 = f(y2)        y3 = h + (k2*dt)/2.0
 *   k3 = f(y3)        y4 = h + k3*dt
 *   k4 = f(y4)        s  = ((k1 + 2.0*k2) + 2.0*k3) + k4
 *   next = h + (dt*s)/6.0                                     plain multiplies and adds, one true division by 6.0
 * Their backward walks the stages from 4 down to 1 with kappa_i = dL/dk_i and ybar_i = J(y_i)^T kappa_i:
 *   kappa4 = dt/6 lambda,  kappa3 = dt/3 lambda + dt ybar4,  kappa2 = dt/3 lambda + dt/2 ybar3,  kappa1 = dt/6 lambda + dt/2 ybar2
 *   lambda_out = lambda + inject + ybar1 + ybar2 + ybar3 + ybar4,      gC[s][m][k] += sum_i sum_p kappa_{i,s} phi_m(y_i) psi_k(y_i)
 *
 * float64, planar [2][H][W] states, dx = dy.  coef: DEVICE array double[2][10][7].
 * Two calls on the same input give the same bits (no floating-point atomics).
 *
 * Conventions as in percnn_pi.h: caller owns all buffers, asynchronous on `stream` (a hipStream_t), no allocation / host
 * synchronisation inside, returns 0 or hipError_t / PERCNN_PI_E*.  Every refusal happens before the first launch, in this
 * order: PERCNN_PI_EINVAL for a NULL pointer, for H or W < 5 (or beyond 2^20 rows / columns), for T_steps < 0, for dx or dt
 * not positive and finite, for an output that overlaps an input; then PERCNN_PI_EWORKSPACE for a missing, misaligned
 * (8 bytes) or short workspace.
 */
#ifndef PERCNN_PI_LIBRARY_CELL_H
#define PERCNN_PI_LIBRARY_CELL_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PERCNN_PI_LIB_COEFS 140

/* one time step; shape = {H, W};  h and h_next: [2][H][W], must not overlap */
int percnn_pi_lib_step_fwd_f64(const double* h, double* h_next, const double* coef, const int64_t* shape, double dx, double dt,
                               void* stream);

/* T steps: traj [T+1][2][H][W], frame 0 holds the initial state, frame t+1 is written from frame t */
int percnn_pi_lib_rollout_fwd_f64(double* traj, const double* coef, const int64_t* shape, int T_steps, double dx, double dt,
                                  void* stream);

/* workspace of the rollout backward (two adjoint states + one row of 140 partial sums per workgroup); 0 for arguments the
 * call refuses */
size_t percnn_pi_lib_rollout_bwd_workspace_bytes(const int64_t* shape, int T_steps);

/* backward of the T-step rollout:  g_traj = dL/dtraj [T+1][2][H][W] (frame_mask: host bytes, T+1 entries, 0 = frame carries
 * no gradient and is not read; NULL = all frames);  g_h0 [2][H][W] = dL/d(frame 0);  g_coef: double[140] = dL/dC, all 140
 * entries whatever the support (both overwritten).  g_h0 and g_coef must not overlap traj, g_traj, coef or each other. */
int percnn_pi_lib_rollout_bwd_f64(const double* traj, const double* g_traj, const unsigned char* frame_mask, double* g_h0,
                                  double* g_coef, void* workspace, size_t workspace_bytes, const double* coef,
                                  const int64_t* shape, int T_steps, double dx, double dt, void* stream);

/* The same four calls with the Runge-Kutta step: argument lists, refusals and frame_mask as above.  The forward calls need no
 * workspace.  The backward recomputes y2, y3, y4 of a step in one launch and runs one launch per stage; its workspace holds two
 * adjoint states (lambda), the three stage states, two ybar states and one row of 140 partial sums per 16 x 16 tile:
 *   (7 * 2 * H * W + ceil(H / 16) * ceil(W / 16) * 140) * sizeof(double) */
int percnn_pi_lib_rk4_step_fwd_f64(const double* h, double* h_next, const double* coef, const int64_t* shape, double dx, double dt,
                                   void* stream);
int percnn_pi_lib_rk4_rollout_fwd_f64(double* traj, const double* coef, const int64_t* shape, int T_steps, double dx, double dt,
                                      void* stream);
size_t percnn_pi_lib_rk4_rollout_bwd_workspace_bytes(const int64_t* shape, int T_steps);
int percnn_pi_lib_rk4_rollout_bwd_f64(const double* traj, const double* g_traj, const unsigned char* frame_mask, double* g_h0,
                                      double* g_coef, void* workspace, size_t workspace_bytes, const double* coef,
                                      const int64_t* shape, int T_steps, double dx, double dt, void* stream);

/* Ensembles: B trajectories in the launches of one, sample b with member b's 140 coefficients.  The eight calls above with
 * `int B` after `shape`; the members share dx, dt and the integrator.  Dense layouts:
 *   h, h_next, g_h0   [B][2][H][W]
 *   traj, g_traj      [T+1][B][2][H][W]   (frame-major, what percnn_pi_library_moments reads)
 *   coef, g_coef      double[B][140]
 * frame_mask stays one byte per frame.  The workspace is B times the single-trajectory workspace of the same integrator.
 * Refusals in the order above, with PERCNN_PI_EINVAL for B < 1 or B > 65535 right after the shape check and the overlap checks
 * on the B-fold extents.  Sample b's trajectory, g_h0[b] and g_coef[b] are bit for bit what the single-trajectory calls give for
 * that sample alone: those calls are B = 1 of the same code. */
int percnn_pi_lib_ensemble_step_fwd_f64(const double* h, double* h_next, const double* coef, const int64_t* shape, int B, double dx,
                                        double dt, void* stream);
int percnn_pi_lib_ensemble_rollout_fwd_f64(double* traj, const double* coef, const int64_t* shape, int B, int T_steps, double dx,
                                           double dt, void* stream);
size_t percnn_pi_lib_ensemble_rollout_bwd_workspace_bytes(const int64_t* shape, int B, int T_steps);
int percnn_pi_lib_ensemble_rollout_bwd_f64(const double* traj, const double* g_traj, const unsigned char* frame_mask, double* g_h0,
                                           double* g_coef, void* workspace, size_t workspace_bytes, const double* coef,
                                           const int64_t* shape, int B, int T_steps, double dx, double dt, void* stream);
int percnn_pi_lib_rk4_ensemble_step_fwd_f64(const double* h, double* h_next, const double* coef, const int64_t* shape, int B,
                                            double dx, double dt, void* stream);
int percnn_pi_lib_rk4_ensemble_rollout_fwd_f64(double* traj, const double* coef, const int64_t* shape, int B, int T_steps, double dx,
                                               double dt, void* stream);
size_t percnn_pi_lib_rk4_ensemble_rollout_bwd_workspace_bytes(const int64_t* shape, int B, int T_steps);
int percnn_pi_lib_rk4_ensemble_rollout_bwd_f64(const double* traj, const double* g_traj, const unsigned char* frame_mask,
                                               double* g_h0, double* g_coef, void* workspace, size_t workspace_bytes,
                                               const double* coef, const int64_t* shape, int B, int T_steps, double dx, double dt,
                                               void* stream);

#ifdef __cplusplus
}
#endif
#endif
