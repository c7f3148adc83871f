// Stage-2 equation discovery: second moments of the 70-term candidate library (include/percnn_pi_discovery.h).
//
// theta = A (x) B with A = the 10 monomials of (u, v) up to degree 3 and B = [1, u_x, u_y, v_x, v_y, lap_u, lap_v], so
// theta theta^T, theta y^T and y y^T of one point are all entries of ONE outer product  m s^T :
//   m = the 28 monomials u^i v^j, i + j <= 6, index d(d+1)/2 + j with d = i + j   (A_a A_a' = m[index of the exponent sum];
//       A itself is m[0..9] in this order)
//   s = the 45 products c_p c_q, p <= q, of c = [B..., u_t, v_t], index p*9 - p(p-1)/2 + (q - p)
// The kernel accumulates S = sum over points of m s^T (28 x 45, padded to 32 x 48) per row class with
// v_mfma_f64_16x16x4_f64: 2 x 3 tiles, 4 points per instruction.  Lane l feeds row / column l & 15 of every tile for the
// point l >> 4 of its wave's group of 4; each lane evaluates the stencils of its own point (the 16 lanes of a point load the
// same addresses: one request).  The class mask is applied to the m operand, dropped and tail points feed zeros on both.
// f64 MFMA C/D lane map: D[row = (lane >> 4) + 4*reg][col = lane & 15]  (NOT the f32 map).
// One partial S per workgroup goes to the caller's workspace; finish_kernel sums them in a fixed order and expands to G, b,
// yy, n.  G[i][j] and G[j][i] read the same entry of S, so G is symmetric bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pi {
namespace disc {

constexpr int NTERMS = 70, NA = 10, NB = 7, NC = 9;
constexpr int NMONO = 28, NPROD = 45;
constexpr int MP = 32, NP = 48;                 // padded to whole 16 x 16 tiles
constexpr int MT = MP / 16, PT = NP / 16;
constexpr int CLS = MP * NP;                    // doubles of one class's S
constexpr int ROW = 2 * CLS;                    // doubles of one workgroup's partial (two classes)
constexpr int NT = 256, NWAVES = NT / 64;
constexpr int FIN_NT = 512;

typedef double d4 __attribute__((ext_vector_type(4)));

struct Geom {
    long frame_stride, sample_stride, plane;    // elements
    int H, W;
    int rh, rw, off;                            // extent of the region along each axis, its first row / column
    unsigned npoints, ngroups;                  // points of one sample, groups of 4
    unsigned seed;
    unsigned long long t_train, t_keep;
    double inv_dt, inv_12dx, inv_dx2;
};

__host__ __device__ inline unsigned mix32(unsigned x)
{
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}

// exponents (i, j) of monomial `idx` (u^i v^j)
__host__ __device__ inline void mono_exp(int idx, int& i, int& j)
{
    int d = 0;
    while ((d + 1) * (d + 2) / 2 <= idx) ++d;
    j = idx - d * (d + 1) / 2;
    i = d - j;
}
__host__ __device__ inline int mono_index(int i, int j) { const int d = i + j; return d * (d + 1) / 2 + j; }

// (p, q), p <= q, of product `idx`
__host__ __device__ inline void prod_pair(int idx, int& p, int& q)
{
    p = 0;
    while (p + 1 < NC && (p + 1) * NC - (p + 1) * p / 2 <= idx) ++p;
    q = p + idx - (p * NC - p * (p - 1) / 2);
}
__host__ __device__ inline int prod_index(int p, int q)
{
    if (p > q) { const int t = p; p = q; q = t; }
    return p * NC - p * (p - 1) / 2 + (q - p);
}

__device__ inline double ipow6(double x, int e)
{
    double r = 1.0;
#pragma unroll
    for (int t = 0; t < 6; ++t) r *= (t < e) ? x : 1.0;
    return r;
}

// c[i] of c = [1, c1 .. c8] for a lane-dependent i, by selects (no indexed registers)
__device__ inline double sel9(int i, double c1, double c2, double c3, double c4, double c5, double c6, double c7, double c8)
{
    double r = 1.0;
    r = (i == 1) ? c1 : r; r = (i == 2) ? c2 : r; r = (i == 3) ? c3 : r; r = (i == 4) ? c4 : r;
    r = (i == 5) ? c5 : r; r = (i == 6) ? c6 : r; r = (i == 7) ? c7 : r; r = (i == 8) ? c8 : r;
    return r;
}

// one species at one point: value, first derivatives along axis 0 / 1, Laplacian, forward time difference
template <typename T>
__device__ inline void point_fields(const T* __restrict__ p, const Geom& g, int y, int x, int ym2, int ym1, int yp1, int yp2,
                                    int xm2, int xm1, int xp1, int xp2, double& ce, double& d0, double& d1, double& lap,
                                    double& dtv)
{
    const long W = g.W, row = (long)y * W;
    ce = (double)p[row + x];
    const double a2 = (double)p[ym2 * W + x], a1 = (double)p[ym1 * W + x];
    const double b1 = (double)p[yp1 * W + x], b2 = (double)p[yp2 * W + x];
    const double l2 = (double)p[row + xm2], l1 = (double)p[row + xm1];
    const double r1 = (double)p[row + xp1], r2 = (double)p[row + xp2];
    const double nx = (double)p[g.frame_stride + row + x];
    d0 = ((a2 - b2) + 8.0 * (b1 - a1)) * g.inv_12dx;
    d1 = ((l2 - r2) + 8.0 * (r1 - l1)) * g.inv_12dx;
    lap = ((-1.0 / 12.0) * ((a2 + b2) + (l2 + r2)) + (4.0 / 3.0) * ((a1 + b1) + (l1 + r1)) - 5.0 * ce) * g.inv_dx2;
    dtv = (nx - ce) * g.inv_dt;
}

template <typename T>
__global__ __launch_bounds__(NT) void moments_kernel(const T* __restrict__ traj, Geom g, double* __restrict__ partial)
{
    __shared__ double red[ROW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = lane >> 4, jl = lane & 15;
    const T* base = traj + (long)blockIdx.y * g.sample_stride;

    // this lane's rows of the m operand and columns of the s operand (padding rows / columns feed zeros)
    int mi[MT], mj[MT], sp[PT], sq[PT];
    bool mok[MT], sok[PT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int idx = jl + 16 * t;
        mok[t] = idx < NMONO;
        mono_exp(mok[t] ? idx : 0, mi[t], mj[t]);
    }
#pragma unroll
    for (int t = 0; t < PT; ++t) {
        const int idx = jl + 16 * t;
        sok[t] = idx < NPROD;
        prod_pair(sok[t] ? idx : 0, sp[t], sq[t]);
    }

    d4 acc[2][MT][PT];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int b = 0; b < PT; ++b) acc[c][a][b] = d4{0.0, 0.0, 0.0, 0.0};

    const int H = g.H, W = g.W;
    const unsigned stride = gridDim.x * NWAVES;
    for (unsigned grp = blockIdx.x * NWAVES + wave; grp < g.ngroups; grp += stride) {
        const unsigned long long q64 = (unsigned long long)grp * 4 + k;
        const bool live = q64 < g.npoints;
        const unsigned q = live ? (unsigned)q64 : 0u;                  // tail lanes compute on point 0 and feed zeros
        const unsigned t = q / (unsigned)g.rw;
        const int x = (int)(q - t * (unsigned)g.rw) + g.off;
        const unsigned f = t / (unsigned)g.rh;
        const int y = (int)(t - f * (unsigned)g.rh) + g.off;
        const unsigned r = (f * (unsigned)H + (unsigned)y) * (unsigned)W + (unsigned)x;
        const unsigned hsh = mix32(r + g.seed);
        const int cls = !live ? 2 : (hsh < g.t_train ? 0 : (hsh < g.t_keep ? 1 : 2));
        if (__ballot(cls < 2) == 0) continue;                          // wave-uniform: nothing of this group is kept

        int ym2 = y - 2, ym1 = y - 1, yp1 = y + 1, yp2 = y + 2, xm2 = x - 2, xm1 = x - 1, xp1 = x + 1, xp2 = x + 2;
        ym2 += ym2 < 0 ? H : 0; ym1 += ym1 < 0 ? H : 0; yp1 -= yp1 >= H ? H : 0; yp2 -= yp2 >= H ? H : 0;
        xm2 += xm2 < 0 ? W : 0; xm1 += xm1 < 0 ? W : 0; xp1 -= xp1 >= W ? W : 0; xp2 -= xp2 >= W ? W : 0;

        const T* fr = base + (long)f * g.frame_stride;
        double u, v, ux, uy, vx, vy, lu, lv, ut, vt;
        point_fields(fr, g, y, x, ym2, ym1, yp1, yp2, xm2, xm1, xp1, xp2, u, ux, uy, lu, ut);
        point_fields(fr + g.plane, g, y, x, ym2, ym1, yp1, yp2, xm2, xm1, xp1, xp2, v, vx, vy, lv, vt);

        double av[2][MT], bv[PT];
#pragma unroll
        for (int tt = 0; tt < MT; ++tt) {
            const double m = ipow6(u, mi[tt]) * ipow6(v, mj[tt]);
            av[0][tt] = (mok[tt] && cls == 0) ? m : 0.0;
            av[1][tt] = (mok[tt] && cls == 1) ? m : 0.0;
        }
#pragma unroll
        for (int tt = 0; tt < PT; ++tt) {
            const double s = sel9(sp[tt], ux, uy, vx, vy, lu, lv, ut, vt) * sel9(sq[tt], ux, uy, vx, vy, lu, lv, ut, vt);
            bv[tt] = (sok[tt] && cls < 2) ? s : 0.0;
        }
#pragma unroll
        for (int cc = 0; cc < 2; ++cc)
#pragma unroll
            for (int a = 0; a < MT; ++a)
#pragma unroll
                for (int b = 0; b < PT; ++b)
                    acc[cc][a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[cc][a], bv[b], acc[cc][a][b], 0, 0, 0);
    }

    // the workgroup's waves in a fixed order: wave 0 stores, waves 1.. add
    for (int w = 0; w < NWAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int cc = 0; cc < 2; ++cc)
#pragma unroll
                for (int a = 0; a < MT; ++a)
#pragma unroll
                    for (int b = 0; b < PT; ++b)
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) {
                            const int m = 16 * a + k + 4 * reg, n = 16 * b + jl;
                            double* e = &red[cc * CLS + m * NP + n];
                            *e = (w == 0 ? 0.0 : *e) + acc[cc][a][b][reg];
                        }
        }
        __syncthreads();
    }
    double* out = partial + ((long)blockIdx.y * gridDim.x + blockIdx.x) * ROW;
    for (int e = threadIdx.x; e < ROW; e += NT) out[e] = red[e];
}

// grid (2 classes, batch): sums the `nrows` partials of a sample in row order, then expands S to G, b, yy, n
__global__ __launch_bounds__(FIN_NT) void finish_kernel(const double* __restrict__ partial, int nrows, double* __restrict__ G,
                                                        double* __restrict__ bvec, double* __restrict__ yy,
                                                        double* __restrict__ n)
{
    __shared__ double S[CLS];
    const int cls = blockIdx.x;
    const long smp = blockIdx.y;
    const double* src = partial + smp * nrows * (long)ROW + cls * CLS;
    for (int e = threadIdx.x; e < CLS; e += FIN_NT) {
        double s = 0.0;
        for (int r = 0; r < nrows; ++r) s += src[(long)r * ROW + e];
        S[e] = s;
    }
    __syncthreads();
    const long oc = smp * 2 + cls;
    for (int o = threadIdx.x; o < NTERMS * NTERMS; o += FIN_NT) {
        const int i = o / NTERMS, j = o - i * NTERMS;
        int ai, aj, bi, bj;
        mono_exp(i / NB, ai, aj);
        mono_exp(j / NB, bi, bj);
        G[oc * NTERMS * NTERMS + o] = S[mono_index(ai + bi, aj + bj) * NP + prod_index(i % NB, j % NB)];
    }
    for (int o = threadIdx.x; o < NTERMS * 2; o += FIN_NT) {
        const int i = o >> 1, sp = o & 1;
        bvec[oc * NTERMS * 2 + o] = S[(i / NB) * NP + prod_index(i % NB, NB + sp)];
    }
    if (threadIdx.x < 2) yy[oc * 2 + threadIdx.x] = S[prod_index(NB + threadIdx.x, NB + threadIdx.x)];
    if (threadIdx.x == 2) n[oc] = S[0];
}

}  // namespace disc
}  // namespace pi
