// C-ABI of the library cell (include/percnn_pi_library_cell.h).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "../../include/percnn_pi.h"
#include "../../include/percnn_pi_library_cell.h"
#include "pi_lib.h"

namespace {

namespace Lb = pi::lib;

// B samples per launch (blockIdx.z): the single-trajectory entry points are B = 1 of the same host bodies
struct Plan {
    Lb::Geom g;
    unsigned B;
    unsigned tiles_x, tiles_y, nblocks;       // adjoint launch: tiles of one sample
    unsigned fwd_blocks;
    int rk4_tile;                             // Runge-Kutta forward launch: tile extent, tiles
    unsigned rk4_tiles_x, rk4_tiles_y;
    long frame;                               // doubles of one [B][2][H][W] state
    size_t state_bytes, coef_bytes;           // one [B][2][H][W] state, the [B][140] coefficients
    size_t ws_bytes[2];                       // rollout backward: Euler, Runge-Kutta
};

enum Integrator { EULER = 0, RK4 = 1 };

bool plan_shape(const int64_t* shape, int B, Plan& p)
{
    if (!shape) return false;
    const int64_t H = shape[0], W = shape[1];
    if (H < 5 || W < 5 || H > (1LL << 20) || W > (1LL << 20)) return false;
    if (H * W >= (1LL << 31)) return false;
    if (B < 1 || B > 65535) return false;                       // gridDim.z
    p.B = (unsigned)B;
    p.g.H = (int)H; p.g.W = (int)W;
    p.g.plane = (long)(H * W);
    p.tiles_x = (unsigned)((W + Lb::TS - 1) / Lb::TS);
    p.tiles_y = (unsigned)((H + Lb::TS - 1) / Lb::TS);
    p.nblocks = p.tiles_x * p.tiles_y;
    p.fwd_blocks = (unsigned)((H * W + Lb::NT - 1) / Lb::NT);
    p.frame = (long)B * 2 * H * W;
    p.state_bytes = (size_t)p.frame * sizeof(double);
    p.coef_bytes = (size_t)B * Lb::NCOEF * sizeof(double);
    p.rk4_tile = Lb::rk4_tile((int)H, (int)W, B);
    p.rk4_tiles_x = (unsigned)((W + p.rk4_tile - 1) / p.rk4_tile);
    p.rk4_tiles_y = (unsigned)((H + p.rk4_tile - 1) / p.rk4_tile);
    // two adjoint states; Runge-Kutta: y2 y3 y4, two ybar, two lambda.  Then the rows, nblocks per sample
    p.ws_bytes[EULER] = 2 * p.state_bytes + (size_t)p.nblocks * p.coef_bytes;
    p.ws_bytes[RK4] = 7 * p.state_bytes + (size_t)p.nblocks * p.coef_bytes;
    return true;
}

bool step_sizes(double dx, double dt, Lb::Geom& g)
{
    if (!(dx > 0.0) || !(dt > 0.0) || !std::isfinite(dx) || !std::isfinite(dt)) return false;
    g.dt = dt; g.inv_12dx = 1.0 / (12.0 * dx); g.inv_dx2 = 1.0 / (dx * dx);
    return true;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

// kernel<..., SAMPLES>: `many` for B > 1, `one` for the single trajectory, whose offsets are all zero (pi_lib.h)
template <class... P, class... A>
void launch(const Plan& p, void (*many)(P...), void (*one)(P...), dim3 grid, hipStream_t st, A... args)
{
    hipLaunchKernelGGL(p.B > 1 ? many : one, grid, dim3(Lb::NT), 0, st, static_cast<P>(args)...);
}

// one Runge-Kutta step: out = the next state, or (STAGES) y2 y3 y4
template <bool STAGES>
void launch_rk4(const double* h, double* out, const double* coef, const Plan& p, hipStream_t st)
{
    const dim3 grid(p.rk4_tiles_x, p.rk4_tiles_y, p.B);
    if (p.rk4_tile == 8)
        launch(p, Lb::rk4_kernel<8, STAGES, true>, Lb::rk4_kernel<8, STAGES, false>, grid, st, h, out, coef, p.g);
    else
        launch(p, Lb::rk4_kernel<16, STAGES, true>, Lb::rk4_kernel<16, STAGES, false>, grid, st, h, out, coef, p.g);
}

int launch_step(Integrator in, const double* h, double* out, const double* coef, const Plan& p, hipStream_t st)
{
    if (in == RK4)
        launch_rk4<false>(h, out, coef, p, st);
    else
        launch(p, Lb::step_kernel<true>, Lb::step_kernel<false>, dim3(p.fwd_blocks, 1, p.B), st, h, out, coef, p.g);
    return (int)hipGetLastError();
}

// the adjoint of one step: G = dL/d(frame t+1) -> out = dL/d(frame t), coefficient gradients added to the rows
int launch_adjoint(Integrator in, const double* h, const double* G, const double* inject, double* out, double* scratch,
                   const double* coef, double* rows, const Plan& p, hipStream_t st)
{
    const dim3 grid(p.tiles_x, p.tiles_y, p.B);
    if (in == EULER) {
        launch(p, Lb::adjoint_kernel<true>, Lb::adjoint_kernel<false>, grid, st, h, G, inject, out, coef, rows, p.g);
        return (int)hipGetLastError();
    }
    // scratch: y2 y3 y4, recomputed, then two ybar buffers.  Stage 4 starts the running sum in `out`, stage 1 completes it
    const long frame = p.frame;
    double *y2 = scratch, *y3 = scratch + frame, *y4 = scratch + 2 * frame, *yb0 = scratch + 3 * frame, *yb1 = scratch + 4 * frame;
    const double dt = p.g.dt;
    launch_rk4<true>(h, scratch, coef, p, st);
    if (hipError_t e = hipGetLastError()) return (int)e;
    const struct {
        const double *y, *prev; double a, b; const double *inject, *acc; double* ybar;
    } stages[4] = {{y4, nullptr, dt / 6.0, 0.0, inject, G, yb0},
                   {y3, yb0, dt / 3.0, dt, nullptr, out, yb1},
                   {y2, yb1, dt / 3.0, dt / 2.0, nullptr, out, yb0},
                   {h, yb0, dt / 6.0, dt / 2.0, nullptr, out, nullptr}};
    for (const auto& s : stages) {
        launch(p, Lb::rk4_stage_kernel<true>, Lb::rk4_stage_kernel<false>, grid, st, s.y, G, s.prev, s.a, s.b, s.inject, s.acc,
               s.ybar, out, coef, rows, p.g);
        if (hipError_t e = hipGetLastError()) return (int)e;
    }
    return 0;
}

int step_fwd(Integrator in, const double* h, double* h_next, const double* coef, const int64_t* shape, int B, double dx, double dt,
             void* stream)
{
    if (!h || !h_next || !coef) return PERCNN_PI_EINVAL;
    Plan p;
    if (!plan_shape(shape, B, p)) return PERCNN_PI_EINVAL;
    if (!step_sizes(dx, dt, p.g)) return PERCNN_PI_EINVAL;
    if (overlap(h_next, p.state_bytes, h, p.state_bytes) || overlap(h_next, p.state_bytes, coef, p.coef_bytes))
        return PERCNN_PI_EINVAL;
    return launch_step(in, h, h_next, coef, p, static_cast<hipStream_t>(stream));
}

int rollout_fwd(Integrator in, double* traj, const double* coef, const int64_t* shape, int B, int T_steps, double dx, double dt,
                void* stream)
{
    if (!traj || !coef) return PERCNN_PI_EINVAL;
    Plan p;
    if (!plan_shape(shape, B, p)) return PERCNN_PI_EINVAL;
    if (T_steps < 0) return PERCNN_PI_EINVAL;
    if (!step_sizes(dx, dt, p.g)) return PERCNN_PI_EINVAL;
    if (overlap(traj, ((size_t)T_steps + 1) * p.state_bytes, coef, p.coef_bytes)) return PERCNN_PI_EINVAL;
    const long frame = p.frame;
    for (int t = 0; t < T_steps; ++t)
        if (int rc = launch_step(in, traj + (long)t * frame, traj + (long)(t + 1) * frame, coef, p,
                                 static_cast<hipStream_t>(stream)))
            return rc;
    return 0;
}

size_t rollout_bwd_workspace_bytes(Integrator in, const int64_t* shape, int B, int T_steps)
{
    Plan p;
    if (!plan_shape(shape, B, p) || T_steps < 0) return 0;
    return p.ws_bytes[in];
}

int rollout_bwd(Integrator in, const double* traj, const double* g_traj, const unsigned char* frame_mask, double* g_h0,
                double* g_coef, void* workspace, size_t workspace_bytes, const double* coef, const int64_t* shape, int B,
                int T_steps, double dx, double dt, void* stream)
{
    if (!traj || !g_traj || !g_h0 || !g_coef || !coef) return PERCNN_PI_EINVAL;
    Plan p;
    if (!plan_shape(shape, B, p)) return PERCNN_PI_EINVAL;
    if (T_steps < 0) return PERCNN_PI_EINVAL;
    if (!step_sizes(dx, dt, p.g)) return PERCNN_PI_EINVAL;
    // nothing the call writes may overlap what it reads, or another output
    const size_t traj_bytes = ((size_t)T_steps + 1) * p.state_bytes, coef_bytes = p.coef_bytes;
    const size_t ws_bytes = p.ws_bytes[in];
    const struct { const void* p; size_t bytes; } ins[] = {{traj, traj_bytes}, {g_traj, traj_bytes}, {coef, coef_bytes}};
    for (const auto& in_ : ins)
        if (overlap(g_h0, p.state_bytes, in_.p, in_.bytes) || overlap(g_coef, coef_bytes, in_.p, in_.bytes)) return PERCNN_PI_EINVAL;
    if (overlap(g_h0, p.state_bytes, g_coef, coef_bytes)) return PERCNN_PI_EINVAL;
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < ws_bytes) return PERCNN_PI_EWORKSPACE;
    for (const auto& in_ : ins)
        if (overlap(workspace, ws_bytes, in_.p, in_.bytes)) return PERCNN_PI_EINVAL;
    if (overlap(workspace, ws_bytes, g_h0, p.state_bytes) || overlap(workspace, ws_bytes, g_coef, coef_bytes))
        return PERCNN_PI_EINVAL;

    auto st = static_cast<hipStream_t>(stream);
    const long frame = p.frame;
    // workspace: two adjoint states, [Runge-Kutta: the five states of launch_adjoint,] the rows; every state [B][2][H][W]
    double* buf[2] = {static_cast<double*>(workspace), static_cast<double*>(workspace) + frame};
    double* scratch = static_cast<double*>(workspace) + 2 * frame;
    double* rows = scratch + (in == RK4 ? 5 * frame : 0);
    auto carries = [&](int f) { return !frame_mask || frame_mask[f]; };
    if (hipError_t e = hipMemsetAsync(rows, 0, (size_t)p.nblocks * coef_bytes, st)) return (int)e;
    if (T_steps == 0) {
        if (hipError_t e = carries(0) ? hipMemcpyAsync(g_h0, g_traj, p.state_bytes, hipMemcpyDeviceToDevice, st)
                                      : hipMemsetAsync(g_h0, 0, p.state_bytes, st))
            return (int)e;
    }
    // the adjoint of frame T is its own gradient; step t turns the adjoint of frame t+1 into that of frame t
    const double* G = g_traj + (long)T_steps * frame;
    if (T_steps > 0 && !carries(T_steps)) {
        if (hipError_t e = hipMemsetAsync(buf[T_steps & 1], 0, p.state_bytes, st)) return (int)e;
        G = buf[T_steps & 1];
    }
    for (int t = T_steps - 1; t >= 0; --t) {
        double* out = t == 0 ? g_h0 : buf[t & 1];
        const double* inject = carries(t) ? g_traj + (long)t * frame : nullptr;
        if (int rc = launch_adjoint(in, traj + (long)t * frame, G, inject, out, scratch, coef, rows, p, st)) return rc;
        G = out;
    }
    hipLaunchKernelGGL(Lb::finish_kernel, dim3(1, 1, p.B), dim3(Lb::FIN_NT), 0, st, rows, (int)p.nblocks, g_coef);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int percnn_pi_lib_step_fwd_f64(const double* h, double* h_next, const double* coef, const int64_t* shape, double dx, double dt,
                               void* stream)
{
    return step_fwd(EULER, h, h_next, coef, shape, 1, dx, dt, stream);
}

int percnn_pi_lib_rk4_step_fwd_f64(const double* h, double* h_next, const double* coef, const int64_t* shape, double dx, double dt,
                                   void* stream)
{
    return step_fwd(RK4, h, h_next, coef, shape, 1, dx, dt, stream);
}

int percnn_pi_lib_rollout_fwd_f64(double* traj, const double* coef, const int64_t* shape, int T_steps, double dx, double dt,
                                  void* stream)
{
    return rollout_fwd(EULER, traj, coef, shape, 1, T_steps, dx, dt, stream);
}

int percnn_pi_lib_rk4_rollout_fwd_f64(double* traj, const double* coef, const int64_t* shape, int T_steps, double dx, double dt,
                                      void* stream)
{
    return rollout_fwd(RK4, traj, coef, shape, 1, T_steps, dx, dt, stream);
}

size_t percnn_pi_lib_rollout_bwd_workspace_bytes(const int64_t* shape, int T_steps)
{
    return rollout_bwd_workspace_bytes(EULER, shape, 1, T_steps);
}

size_t percnn_pi_lib_rk4_rollout_bwd_workspace_bytes(const int64_t* shape, int T_steps)
{
    return rollout_bwd_workspace_bytes(RK4, shape, 1, T_steps);
}

int percnn_pi_lib_rollout_bwd_f64(const double* traj, const double* g_traj, const unsigned char* frame_mask, double* g_h0,
                                  double* g_coef, void* workspace, size_t workspace_bytes, const double* coef, const int64_t* shape,
                                  int T_steps, double dx, double dt, void* stream)
{
    return rollout_bwd(EULER, traj, g_traj, frame_mask, g_h0, g_coef, workspace, workspace_bytes, coef, shape, 1, T_steps, dx, dt,
                       stream);
}

int percnn_pi_lib_rk4_rollout_bwd_f64(const double* traj, const double* g_traj, const unsigned char* frame_mask, double* g_h0,
                                      double* g_coef, void* workspace, size_t workspace_bytes, const double* coef,
                                      const int64_t* shape, int T_steps, double dx, double dt, void* stream)
{
    return rollout_bwd(RK4, traj, g_traj, frame_mask, g_h0, g_coef, workspace, workspace_bytes, coef, shape, 1, T_steps, dx, dt,
                       stream);
}

// B members per launch: the same calls with `int B` after `shape`

int percnn_pi_lib_ensemble_step_fwd_f64(const double* h, double* h_next, const double* coef, const int64_t* shape, int B, double dx,
                                        double dt, void* stream)
{
    return step_fwd(EULER, h, h_next, coef, shape, B, dx, dt, stream);
}

int percnn_pi_lib_rk4_ensemble_step_fwd_f64(const double* h, double* h_next, const double* coef, const int64_t* shape, int B,
                                            double dx, double dt, void* stream)
{
    return step_fwd(RK4, h, h_next, coef, shape, B, dx, dt, stream);
}

int percnn_pi_lib_ensemble_rollout_fwd_f64(double* traj, const double* coef, const int64_t* shape, int B, int T_steps, double dx,
                                           double dt, void* stream)
{
    return rollout_fwd(EULER, traj, coef, shape, B, T_steps, dx, dt, stream);
}

int percnn_pi_lib_rk4_ensemble_rollout_fwd_f64(double* traj, const double* coef, const int64_t* shape, int B, int T_steps,
                                               double dx, double dt, void* stream)
{
    return rollout_fwd(RK4, traj, coef, shape, B, T_steps, dx, dt, stream);
}

size_t percnn_pi_lib_ensemble_rollout_bwd_workspace_bytes(const int64_t* shape, int B, int T_steps)
{
    return rollout_bwd_workspace_bytes(EULER, shape, B, T_steps);
}

size_t percnn_pi_lib_rk4_ensemble_rollout_bwd_workspace_bytes(const int64_t* shape, int B, int T_steps)
{
    return rollout_bwd_workspace_bytes(RK4, shape, B, T_steps);
}

int percnn_pi_lib_ensemble_rollout_bwd_f64(const double* traj, const double* g_traj, const unsigned char* frame_mask, double* g_h0,
                                           double* g_coef, void* workspace, size_t workspace_bytes, const double* coef,
                                           const int64_t* shape, int B, int T_steps, double dx, double dt, void* stream)
{
    return rollout_bwd(EULER, traj, g_traj, frame_mask, g_h0, g_coef, workspace, workspace_bytes, coef, shape, B, T_steps, dx, dt,
                       stream);
}

int percnn_pi_lib_rk4_ensemble_rollout_bwd_f64(const double* traj, const double* g_traj, const unsigned char* frame_mask,
                                               double* g_h0, double* g_coef, void* workspace, size_t workspace_bytes,
                                               const double* coef, const int64_t* shape, int B, int T_steps, double dx, double dt,
                                               void* stream)
{
    return rollout_bwd(RK4, traj, g_traj, frame_mask, g_h0, g_coef, workspace, workspace_bytes, coef, shape, B, T_steps, dx, dt,
                       stream);
}

}  // extern "C"
