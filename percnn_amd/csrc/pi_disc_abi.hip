// C-ABI of the Stage-2 library moments (include/percnn_pi_discovery.h).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "../../include/percnn_pi.h"
#include "../../include/percnn_pi_discovery.h"
#include "pi_disc.h"

namespace {

namespace D = pi::disc;

constexpr unsigned long long TWO32 = 1ULL << 32;

// workgroups per sample: 16 groups of 4 points per wave at least, at most one workgroup per CU.  The count depends on the
// full grid's point count only (not on the region, not on the batch), so a sample's sums are added in the same order in a
// batched and an unbatched call, and the workspace is the same for both regions.
bool plan(const int64_t* shape, int nframes, int batch, int region, D::Geom& g, unsigned& nblocks)
{
    if (!shape || nframes < 3 || batch < 1 || batch > 65535) return false;
    const int64_t H = shape[0], W = shape[1];
    if (H < 5 || W < 5 || H > (1LL << 30) || W > (1LL << 30)) return false;
    if ((unsigned long long)H * (unsigned long long)W > TWO32 / (unsigned long long)nframes) return false;
    if (region != PERCNN_PI_REGION_INTERIOR && region != PERCNN_PI_REGION_PERIODIC) return false;
    g.H = (int)H; g.W = (int)W;
    g.plane = (long)H * W;
    g.off = region == PERCNN_PI_REGION_INTERIOR ? 2 : 0;
    g.rh = (int)H - 2 * g.off; g.rw = (int)W - 2 * g.off;
    const unsigned long long np = (unsigned long long)(nframes - 2) * g.rh * g.rw;
    g.npoints = (unsigned)np;
    g.ngroups = (unsigned)((np + 3) / 4);
    const unsigned cap = 256;
    const unsigned long long full = ((unsigned long long)(nframes - 2) * H * W + 3) / 4;
    const unsigned long long want = (full + D::NWAVES * 16 - 1) / (D::NWAVES * 16);
    nblocks = want < 1 ? 1u : (want > cap ? cap : (unsigned)want);
    return true;
}

template <typename T>
int moments(const T* traj, int64_t frame_stride, int64_t sample_stride, const int64_t* shape, int nframes, int batch, double dx,
            double dt, int region, uint32_t seed, uint64_t t_train, uint64_t t_keep, double* G, double* b, double* yy,
            double* n, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!traj || !G || !b || !yy || !n) return PERCNN_PI_EINVAL;
    D::Geom g;
    unsigned nblocks = 0;
    if (!plan(shape, nframes, batch, region, g, nblocks)) return PERCNN_PI_EINVAL;
    if (t_train > t_keep || t_keep > TWO32) return PERCNN_PI_EINVAL;
    if (!(dx > 0.0) || !(dt > 0.0) || !std::isfinite(dx) || !std::isfinite(dt)) return PERCNN_PI_EINVAL;
    if (frame_stride < 0 || sample_stride < 0) return PERCNN_PI_EINVAL;
    const size_t need = (size_t)batch * nblocks * D::ROW * sizeof(double);
    if (!workspace || workspace_bytes < need) return PERCNN_PI_EWORKSPACE;
    // nothing the call writes may overlap what it reads
    const uintptr_t t0 = (uintptr_t)traj;
    const uintptr_t t1 = t0 + ((uintptr_t)(batch - 1) * (uintptr_t)sample_stride + (uintptr_t)(nframes - 1) * (uintptr_t)frame_stride +
                               2 * (uintptr_t)g.plane) * sizeof(T);
    const struct { const void* p; size_t bytes; } outs[] = {
        {G, (size_t)batch * 2 * D::NTERMS * D::NTERMS * sizeof(double)}, {b, (size_t)batch * 2 * D::NTERMS * 2 * sizeof(double)},
        {yy, (size_t)batch * 4 * sizeof(double)}, {n, (size_t)batch * 2 * sizeof(double)}, {workspace, need}};
    for (const auto& o : outs) {
        const uintptr_t o0 = (uintptr_t)o.p;
        if (o0 < t1 && t0 < o0 + o.bytes) return PERCNN_PI_EINVAL;
    }
    g.frame_stride = (long)frame_stride;
    g.sample_stride = (long)sample_stride;
    g.seed = seed;
    g.t_train = t_train; g.t_keep = t_keep;
    g.inv_dt = 1.0 / dt; g.inv_12dx = 1.0 / (12.0 * dx); g.inv_dx2 = 1.0 / (dx * dx);
    auto st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(D::moments_kernel<T>, dim3(nblocks, (unsigned)batch), dim3(D::NT), 0, st, traj, g, part);
    if (hipError_t e = hipGetLastError()) return (int)e;
    hipLaunchKernelGGL(D::finish_kernel, dim3(2, (unsigned)batch), dim3(D::FIN_NT), 0, st, part, (int)nblocks, G, b, yy, n);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t percnn_pi_library_moments_workspace_bytes(const int64_t* shape, int nframes, int batch)
{
    D::Geom g;
    unsigned nblocks = 0;
    if (!plan(shape, nframes, batch, PERCNN_PI_REGION_PERIODIC, g, nblocks)) return 0;
    return (size_t)batch * nblocks * D::ROW * sizeof(double);
}

int percnn_pi_library_moments_f32(const float* traj, int64_t frame_stride, int64_t sample_stride, const int64_t* shape,
                                  int nframes, int batch, double dx, double dt, int region, uint32_t seed, uint64_t t_train,
                                  uint64_t t_keep, double* G, double* b, double* yy, double* n, void* workspace,
                                  size_t workspace_bytes, void* stream)
{
    return moments(traj, frame_stride, sample_stride, shape, nframes, batch, dx, dt, region, seed, t_train, t_keep, G, b, yy, n,
                   workspace, workspace_bytes, stream);
}

int percnn_pi_library_moments_f64(const double* traj, int64_t frame_stride, int64_t sample_stride, const int64_t* shape,
                                  int nframes, int batch, double dx, double dt, int region, uint32_t seed, uint64_t t_train,
                                  uint64_t t_keep, double* G, double* b, double* yy, double* n, void* workspace,
                                  size_t workspace_bytes, void* stream)
{
    return moments(traj, frame_stride, sample_stride, shape, nframes, batch, dx, dt, region, seed, t_train, t_keep, G, b, yy, n,
                   workspace, workspace_bytes, stream);
}

}  // extern "C"
