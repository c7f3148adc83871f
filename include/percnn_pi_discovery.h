/* C-ABI of Stage-2 equation discovery: second moments of the 70-term candidate library -- part of libpercnn_pi.so.
 *
 * Replaces the host side of
 *   Loss_generator.get_phy_residual   DataDrivenDiscoveryOfPDEs/2D_Burgers_eqn/Stage-2/derivatives.py:129-199
 *   the library / data matrix         DataDrivenDiscoveryOfPDEs/2D_Burgers_eqn/Stage-2/PDE_FIND_u.py:185-193, 245-260
 * (and the lambda-omega Stage-2, the same code with dx = 0.2, dt = 0.0125): the rows x 70 matrix Theta is never formed,
 * sequential-threshold ridge regression needs it only through  G = Theta^T Theta,  b = Theta^T y,  y^T y  and the row count.
 *
 * Rows are the points of frames f = 0 .. nframes-3 of a trajectory of 2-species planar states [2][H][W]:
 *   y        = (u_t, v_t),  u_t = (h[f+1] - h[f]) / dt
 *   theta[7a + b] = A_a * B_b,   A = [1, u, v, u^2, uv, v^2, u^3, u^2 v, u v^2, v^3],
 *                                B = [1, u_x, u_y, v_x, v_y, lap_u, lap_v]
 *   u_x: 4th-order central first derivative along grid axis 0 (rows), u_y along axis 1 (the reference's naming),
 *        (f[-2] - 8 f[-1] + 8 f[+1] - f[+2]) / (12 dx);   lap: 4th-order star (taps -1/12, 4/3 per axis, centre -5) / dx^2.
 * All arithmetic is float64 from the loaded values; the _f32 / _f64 suffix is the type of the trajectory only.
 *
 * region   PERCNN_PI_REGION_INTERIOR: points with 2 <= y <= H-3, 2 <= x <= W-3 (valid convolutions on the unpadded field:
 *          what the reference scripts evaluate);  PERCNN_PI_REGION_PERIODIC: all H*W points, stencils wrap.
 * classes  r = (f*H + y)*W + x (the full-grid index in both regions, per sample);  h = mix32((uint32)r + seed) with
 *          mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 *          class 0 (train) if h < t_train, class 1 (test) if t_train <= h < t_keep, otherwise the row is dropped.
 *          0 <= t_train <= t_keep <= 2^32; t_train = t_keep = 2^32 puts every row into class 0.
 * outputs  (float64, overwritten)  G [batch][2][70][70],  b [batch][2][70][2],  yy [batch][2][2],  n [batch][2]
 *          (the row count of each class, exact).  G is exactly symmetric; two calls on the same input give the same bits
 *          (no floating-point atomics: one partial row per workgroup in `workspace`, summed in a fixed order).
 *
 * Conventions as in percnn_pi.h: caller owns all buffers, asynchronous on `stream` (a hipStream_t), no allocation / host
 * synchronisation inside, returns 0 or hipError_t / PERCNN_PI_E*.
 */
#ifndef PERCNN_PI_DISCOVERY_H
#define PERCNN_PI_DISCOVERY_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PERCNN_PI_LIBRARY_TERMS 70
#define PERCNN_PI_REGION_INTERIOR 0
#define PERCNN_PI_REGION_PERIODIC 1

/* bytes of `workspace` for a call with this shape = {H, W}, frame count and batch (0 for arguments the call refuses) */
size_t percnn_pi_library_moments_workspace_bytes(const int64_t* shape, int nframes, int batch);

/* traj: frame f of sample s starts at traj + f*frame_stride + s*sample_stride (strides in elements; the [2][H][W] block
 * of a frame is contiguous).  PERCNN_PI_EINVAL for NULL pointers, nframes < 3, H or W < 5, batch outside 1..65535,
 * nframes*H*W > 2^32, t_train > t_keep, t_keep > 2^32, dx or dt not positive and finite, an unknown region, negative
 * strides, outputs or workspace that overlap the trajectory;  PERCNN_PI_EWORKSPACE for a short workspace. */
int percnn_pi_library_moments_f32(const float* traj, int64_t frame_stride, int64_t sample_stride, const int64_t* shape,
                                  int nframes, int batch, double dx, double dt, int region, uint32_t seed, uint64_t t_train,
                                  uint64_t t_keep, double* G, double* b, double* yy, double* n, void* workspace,
                                  size_t workspace_bytes, void* stream);
int percnn_pi_library_moments_f64(const double* traj, int64_t frame_stride, int64_t sample_stride, const int64_t* shape,
                                  int nframes, int batch, double dx, double dt, int region, uint32_t seed, uint64_t t_train,
                                  uint64_t t_keep, double* G, double* b, double* yy, double* n, void* workspace,
                                  size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
