// C-ABI of the library cell (include/percnn_pi_library_cell.h).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "../../include/percnn_pi.h"
#include "../../include/percnn_pi_library_cell.h"
#include "pi_lib.h"

namespace {

namespace Lb = pi::lib;

struct Plan {
    Lb::Geom g;
    unsigned tiles_x, tiles_y, nblocks;       // adjoint launch
    unsigned fwd_blocks;
    size_t state_bytes;                       // one [2][H][W] state
    size_t ws_bytes;
};

bool plan_shape(const int64_t* shape, Plan& p)
{
    if (!shape) return false;
    const int64_t H = shape[0], W = shape[1];
    if (H < 5 || W < 5 || H > (1LL << 20) || W > (1LL << 20)) return false;
    if (H * W >= (1LL << 31)) return false;
    p.g.H = (int)H; p.g.W = (int)W;
    p.g.plane = (long)(H * W);
    p.tiles_x = (unsigned)((W + Lb::TS - 1) / Lb::TS);
    p.tiles_y = (unsigned)((H + Lb::TS - 1) / Lb::TS);
    p.nblocks = p.tiles_x * p.tiles_y;
    p.fwd_blocks = (unsigned)((H * W + Lb::NT - 1) / Lb::NT);
    p.state_bytes = (size_t)2 * H * W * sizeof(double);
    p.ws_bytes = 2 * p.state_bytes + (size_t)p.nblocks * Lb::NCOEF * sizeof(double);
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

int launch_step(const double* h, double* out, const double* coef, const Plan& p, hipStream_t st)
{
    hipLaunchKernelGGL(Lb::step_kernel, dim3(p.fwd_blocks), dim3(Lb::NT), 0, st, h, out, coef, p.g);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int percnn_pi_lib_step_fwd_f64(const double* h, double* h_next, const double* coef, const int64_t* shape, double dx, double dt,
                               void* stream)
{
    if (!h || !h_next || !coef) return PERCNN_PI_EINVAL;
    Plan p;
    if (!plan_shape(shape, p)) return PERCNN_PI_EINVAL;
    if (!step_sizes(dx, dt, p.g)) return PERCNN_PI_EINVAL;
    if (overlap(h_next, p.state_bytes, h, p.state_bytes) || overlap(h_next, p.state_bytes, coef, Lb::NCOEF * sizeof(double)))
        return PERCNN_PI_EINVAL;
    return launch_step(h, h_next, coef, p, static_cast<hipStream_t>(stream));
}

int percnn_pi_lib_rollout_fwd_f64(double* traj, const double* coef, const int64_t* shape, int T_steps, double dx, double dt,
                                  void* stream)
{
    if (!traj || !coef) return PERCNN_PI_EINVAL;
    Plan p;
    if (!plan_shape(shape, p)) return PERCNN_PI_EINVAL;
    if (T_steps < 0) return PERCNN_PI_EINVAL;
    if (!step_sizes(dx, dt, p.g)) return PERCNN_PI_EINVAL;
    if (overlap(traj, ((size_t)T_steps + 1) * p.state_bytes, coef, Lb::NCOEF * sizeof(double))) return PERCNN_PI_EINVAL;
    const long frame = 2 * p.g.plane;
    for (int t = 0; t < T_steps; ++t)
        if (int rc = launch_step(traj + (long)t * frame, traj + (long)(t + 1) * frame, coef, p, static_cast<hipStream_t>(stream)))
            return rc;
    return 0;
}

size_t percnn_pi_lib_rollout_bwd_workspace_bytes(const int64_t* shape, int T_steps)
{
    Plan p;
    if (!plan_shape(shape, p) || T_steps < 0) return 0;
    return p.ws_bytes;
}

int percnn_pi_lib_rollout_bwd_f64(const double* traj, const double* g_traj, const unsigned char* frame_mask, double* g_h0,
                                  double* g_coef, void* workspace, size_t workspace_bytes, const double* coef,
                                  const int64_t* shape, int T_steps, double dx, double dt, void* stream)
{
    if (!traj || !g_traj || !g_h0 || !g_coef || !coef) return PERCNN_PI_EINVAL;
    Plan p;
    if (!plan_shape(shape, p)) return PERCNN_PI_EINVAL;
    if (T_steps < 0) return PERCNN_PI_EINVAL;
    if (!step_sizes(dx, dt, p.g)) return PERCNN_PI_EINVAL;
    // nothing the call writes may overlap what it reads, or another output
    const size_t traj_bytes = ((size_t)T_steps + 1) * p.state_bytes, coef_bytes = Lb::NCOEF * sizeof(double);
    const struct { const void* p; size_t bytes; } ins[] = {{traj, traj_bytes}, {g_traj, traj_bytes}, {coef, coef_bytes}};
    for (const auto& in : ins)
        if (overlap(g_h0, p.state_bytes, in.p, in.bytes) || overlap(g_coef, coef_bytes, in.p, in.bytes)) return PERCNN_PI_EINVAL;
    if (overlap(g_h0, p.state_bytes, g_coef, coef_bytes)) return PERCNN_PI_EINVAL;
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < p.ws_bytes) return PERCNN_PI_EWORKSPACE;
    for (const auto& in : ins)
        if (overlap(workspace, p.ws_bytes, in.p, in.bytes)) return PERCNN_PI_EINVAL;
    if (overlap(workspace, p.ws_bytes, g_h0, p.state_bytes) || overlap(workspace, p.ws_bytes, g_coef, coef_bytes))
        return PERCNN_PI_EINVAL;

    auto st = static_cast<hipStream_t>(stream);
    const long frame = 2 * p.g.plane;
    double* buf[2] = {static_cast<double*>(workspace), static_cast<double*>(workspace) + frame};
    double* rows = static_cast<double*>(workspace) + 2 * frame;
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
        hipLaunchKernelGGL(Lb::adjoint_kernel, dim3(p.tiles_x, p.tiles_y), dim3(Lb::NT), 0, st, traj + (long)t * frame, G, inject,
                           out, coef, rows, p.g);
        if (hipError_t e = hipGetLastError()) return (int)e;
        G = out;
    }
    hipLaunchKernelGGL(Lb::finish_kernel, dim3(1), dim3(Lb::FIN_NT), 0, st, rows, (int)p.nblocks, g_coef);
    return (int)hipGetLastError();
}

}  // extern "C"
