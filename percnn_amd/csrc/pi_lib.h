// Stage-3 rollouts of any equation over the Stage-2 candidate library (include/percnn_pi_library_cell.h).
//
//   next_s = h_s + dt * sum_{k<7} psi_k * q_{s,k},     q_{s,k} = sum_{m<10} C[s][m][k] * phi_m
//   phi = [1, u, v, u^2, uv, v^2, u^3, u^2 v, u v^2, v^3]        psi = [1, u_x, u_y, v_x, v_y, lap_u, lap_v]
// with the stencil expressions of disc::point_fields (pi_disc.h), so the library that discovers an equation and the cell
// that integrates it evaluate the same numbers.  float64, periodic, one launch per step and per adjoint step.
//
// step_kernel     one point per lane: the radius-2 star of both species (18 loads), psi, phi, both updates in the pinned
//                 order (plain multiplies and adds).  C is read with wave-uniform addresses (scalar loads); a column k whose ten
//                 coefficients of a species are all zero is skipped by a wave-uniform branch.  Which columns those are comes
//                 from one vote of the wave over the 140 entries (nonzero_mask): testing them one scalar load after the other
//                 cost 4 us per step pair on the sparse Burgers equation, more than the skipped arithmetic saves.
// adjoint_kernel  one 16 x 16 tile per workgroup, one point per lane.  With G the incoming adjoint state, a_s = dt G_s and
//                 w_k = sum_s a_s q_{s,k}, the outgoing state is
//                   G_s + inject_s + sum_{s',k} a_s' psi_k dq_{s',k}/dh_s  - D0 w_{s_x} - D1 w_{s_y} + Lap w_{lap_s}
//                 q depends on the point's own (u, v) only, so w is evaluated ONCE per point of the tile plus its 2-wide star
//                 halo into LDS (384 evaluations for 256 points) and the transposed stencils read it from there.
//                 The same launch accumulates gC[s][m][k] += sum_p a_s phi_m psi_k with v_mfma_f64_16x16x4_f64: rows (s, m)
//                 = 20 padded to two 16-row tiles, columns k = 7 padded to 16, K = 4 points per instruction.  Each lane
//                 stages phi, a and psi of its point in LDS; lane l then feeds row / column l & 15 for the point l >> 4 of a
//                 group of 4 (the operand map at the top of pi_disc.h; C/D: D[(lane >> 4) + 4 reg][lane & 15]).  Lanes
//                 outside the grid stage zeros for a and psi, padding rows and columns feed zeros.
// rk4_kernel      one classical Runge-Kutta step per launch, no workspace (the order of include/percnn_pi_library_cell.h).  A
//                 workgroup owns an FT x FT tile (FT = 8 or 16: rk4_tile) and loads it with an 8-wide wrapped halo into LDS,
//                 then evaluates k1 on tile + 6, k2 on tile + 4, k3 on tile + 2 and k4 on the tile: four right-hand sides, one
//                 launch boundary.  The stage
//                 states ping-pong between two LDS windows next to the window of h; k1 .. k4 of the tile's own points stay in
//                 registers for s.  A point's value is the same expression whichever tile evaluates it, so the redundant halo
//                 work changes no bit.  Window extents are no multiple of the workgroup, so lanes loop over window points;
//                 every lane reaches every barrier.  <STAGES>: writes y2, y3, y4 of the tile's points instead of the next
//                 state (what the backward recomputes per step; k4 is not needed for that).
// rk4_stage_kernel  adjoint_kernel's body for one Runge-Kutta stage: kappa = a lambda + b ybar_{i+1} pointwise (halo points
//                 included) takes the place of dt G, the stage state y_i that of h; writes ybar_i = J(y_i)^T kappa and adds it to
//                 the running sum that becomes the step's outgoing adjoint.
// Partial sums: one row of 140 doubles per workgroup, each workgroup adds only to its own row, launch after launch in stream
// order; finish_kernel sums the rows in a fixed order.  No floating-point atomics: the same call twice gives the same bits.
//
// Samples: every launch carries the sample index on blockIdx.z (B = gridDim.z members of an ensemble; one trajectory is B = 1 of
// the same bodies).  Sample z reads and writes its own [2][H][W] slice of a dense [B][2][H][W] state (`sample`), member z's 140
// coefficients (C + 140 z: blockIdx.z is uniform over the workgroup, so the coefficient reads stay scalar loads and nonzero_mask
// / the column skip work per member) and its own nblocks rows of partial sums.  finish_kernel runs one workgroup per sample, so
// sample z's results are the bits the B = 1 launch gives for that sample alone.  Every body exists twice, <SAMPLES> true for
// B > 1 and false for B = 1, where the offsets are zero: these launches wait for their first load, and the offset arithmetic in
// front of it cost the single-trajectory route 1 % (3.71 against 3.68 us per Euler step at 100^2); <false> is the code without it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pi {
namespace lib {

constexpr int NA = 10, NB = 7, NCOEF = 2 * NA * NB;
constexpr int NT = 256, NWAVES = NT / 64;
constexpr int TS = 16, HALO = 2, LW = TS + 2 * HALO;   // adjoint tile, its LDS extent with the star halo
constexpr int STG = 19;                                 // staged doubles per point: phi[10], a_u, a_v, psi[7]
constexpr int FIN_NT = 192;
constexpr int FH = 8;                                   // halo of the forward Runge-Kutta tile: four radius-2 stages
// The Runge-Kutta tile is FT x FT, FT = 8 or 16 (rk4_tile): a launch of a 100^2 step is bounded by its slowest workgroup, not by
// arithmetic, and a workgroup's time is its serial right-hand sides per lane -- 5 on the 8-wide tile (169 workgroups at 100^2,
// 3.4 x redundant evaluations), 10 on the 16-wide one (49 workgroups, 2.0 x).  The small tile while every workgroup still gets a
// compute unit of its own (256 on MI355X), the 16-wide tile beyond.
// An ensemble launch of B samples fills the chip, so its workgroups run in rounds of the resident ones -- LDS admits 5 workgroups
// of the 8-wide tile per compute unit (1280 on MI355X) and 3 of the 16-wide one (768) -- and a round costs the serial right-hand
// sides: the tile with fewer rounds x right-hand sides, the 16-wide one on a tie.  That is the faster tile at every measured
// B x 100^2 (profiles/library_cell_ensemble.json), where counting B x tiles against the 256 of one trajectory chose the slower
// one at B = 2, 4 and 16.  B = 1 is the rule above.
constexpr int RK4_SMALL_TILE_BLOCKS = 256;
constexpr int RK4_RESIDENT_8 = 1280, RK4_RESIDENT_16 = 768, RK4_SERIAL_8 = 5, RK4_SERIAL_16 = 10;

__host__ __device__ inline int rk4_tile(int H, int W, int B = 1)
{
#ifdef PERCNN_PI_LIB_RK4_TILE                               // measurement builds (tools/library_cell_bench.py): one tile everywhere
    return PERCNN_PI_LIB_RK4_TILE;
#endif
    const long n8 = (long)B * ((H + 7) / 8) * ((W + 7) / 8), n16 = (long)B * ((H + 15) / 16) * ((W + 15) / 16);
    if (B == 1) return n8 <= RK4_SMALL_TILE_BLOCKS ? 8 : 16;
    const long cost8 = (n8 + RK4_RESIDENT_8 - 1) / RK4_RESIDENT_8 * RK4_SERIAL_8;
    const long cost16 = (n16 + RK4_RESIDENT_16 - 1) / RK4_RESIDENT_16 * RK4_SERIAL_16;
    return cost8 < cost16 ? 8 : 16;
}

typedef double d4 __attribute__((ext_vector_type(4)));

struct Geom {
    int H, W;
    long plane;
    double dt, inv_12dx, inv_dx2;
};

__host__ __device__ inline int cidx(int s, int m, int k) { return (s * NA + m) * NB + k; }

// this workgroup's sample (blockIdx.z) of a dense [B][2][H][W] state; sample_opt: of a pointer that may be NULL
template <bool SAMPLES, class T>
__device__ inline T* sample(T* p, const Geom& g)
{
    if constexpr (!SAMPLES) return p;
    return p + (long)blockIdx.z * 2 * g.plane;
}

template <bool SAMPLES, class T>
__device__ inline T* sample_opt(T* p, const Geom& g)
{
    if constexpr (!SAMPLES) return p;
    return p ? p + (long)blockIdx.z * 2 * g.plane : nullptr;
}

// member z's coefficients of [B][140]
template <bool SAMPLES>
__device__ inline const double* sample_coef(const double* C)
{
    if constexpr (!SAMPLES) return C;
    return C + blockIdx.z * NCOEF;
}

__device__ inline int wrapi(int v, int n)
{
    v %= n;
    return v < 0 ? v + n : v;
}

// phi in the pinned operation order
__device__ inline void monomials(double u, double v, double* phi)
{
    const double u2 = u * u, uv = u * v, v2 = v * v;
    phi[0] = 1.0; phi[1] = u; phi[2] = v; phi[3] = u2; phi[4] = uv; phi[5] = v2;
    phi[6] = u2 * u; phi[7] = u2 * v; phi[8] = u * v2; phi[9] = v2 * v;
}

// which of the 140 coefficients are non-zero, as three wave-uniform 64-bit words: lane l looks at entries l, 64 + l, 128 + l
// and the wave votes (one round of loads instead of a chain of 140 dependent scalar loads).  Needs all 64 lanes of the wave.
struct NonZero {
    unsigned long long w[3];
};

__device__ inline NonZero nonzero_mask(const double* __restrict__ C)
{
    const int lane = threadIdx.x & 63;
    const bool tail = lane < NCOEF - 128;
    NonZero z;
    z.w[0] = __ballot(C[lane] != 0.0);
    z.w[1] = __ballot(C[64 + lane] != 0.0);
    z.w[2] = __ballot(tail && C[tail ? 128 + lane : 0] != 0.0);
    return z;
}

// wave-uniform: does column k of species s carry any coefficient?  (s, k compile-time: the three masks fold to constants)
__device__ inline bool column_live(const NonZero& z, int s, int k)
{
    unsigned long long m[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < NA; ++a) m[cidx(s, a, k) >> 6] |= 1ULL << (cidx(s, a, k) & 63);
    return ((z.w[0] & m[0]) | (z.w[1] & m[1]) | (z.w[2] & m[2])) != 0;
}

__device__ inline double column_q(const double* __restrict__ C, int s, int k, const double* phi)
{
    double q = C[cidx(s, 0, k)] * phi[0];
#pragma unroll
    for (int m = 1; m < NA; ++m) q = q + C[cidx(s, m, k)] * phi[m];
    return q;
}

// the pinned stencil expressions on the star a2 a1 [ce] b1 b2 (axis 0), l2 l1 [ce] r1 r2 (axis 1)
__device__ inline void star_fields(const Geom& g, double ce, double a2, double a1, double b1, double b2, double l2, double l1,
                                   double r1, double r2, double& d0, double& d1, double& lap)
{
    d0 = ((a2 - b2) + 8.0 * (b1 - a1)) * g.inv_12dx;
    d1 = ((l2 - r2) + 8.0 * (r1 - l1)) * g.inv_12dx;
    lap = ((-1.0 / 12.0) * ((a2 + b2) + (l2 + r2)) + (4.0 / 3.0) * ((a1 + b1) + (l1 + r1)) - 5.0 * ce) * g.inv_dx2;
}

// one species at the point (y, x): value, first derivatives along axis 0 / 1, Laplacian -- disc::point_fields' expressions
__device__ inline void point_fields(const double* __restrict__ p, const Geom& g, int y, int x, int ym2, int ym1, int yp1, int yp2,
                                    int xm2, int xm1, int xp1, int xp2, double& ce, double& d0, double& d1, double& lap)
{
    const long W = g.W, row = (long)y * W;
    ce = p[row + x];
    const double a2 = p[ym2 * W + x], a1 = p[ym1 * W + x];
    const double b1 = p[yp1 * W + x], b2 = p[yp2 * W + x];
    const double l2 = p[row + xm2], l1 = p[row + xm1];
    const double r1 = p[row + xp1], r2 = p[row + xp2];
    star_fields(g, ce, a2, a1, b1, b2, l2, l1, r1, r2, d0, d1, lap);
}

// psi of the point (y, x), 0 <= y < H, 0 <= x < W
__device__ inline void library_fields(const double* __restrict__ h, const Geom& g, int y, int x, double& u, double& v, double* psi)
{
    const int H = g.H, W = g.W;
    int ym2 = y - 2, ym1 = y - 1, yp1 = y + 1, yp2 = y + 2, xm2 = x - 2, xm1 = x - 1, xp1 = x + 1, xp2 = x + 2;
    ym2 += ym2 < 0 ? H : 0; ym1 += ym1 < 0 ? H : 0; yp1 -= yp1 >= H ? H : 0; yp2 -= yp2 >= H ? H : 0;
    xm2 += xm2 < 0 ? W : 0; xm1 += xm1 < 0 ? W : 0; xp1 -= xp1 >= W ? W : 0; xp2 -= xp2 >= W ? W : 0;
    psi[0] = 1.0;
    point_fields(h, g, y, x, ym2, ym1, yp1, yp2, xm2, xm1, xp1, xp2, u, psi[1], psi[2], psi[5]);
    point_fields(h + g.plane, g, y, x, ym2, ym1, yp1, yp2, xm2, xm1, xp1, xp2, v, psi[3], psi[4], psi[6]);
}

// the right-hand side of species s in the pinned order: live columns k = 0 .. 6 in turn, q summed over m = 0 .. 9
template <int S>
__device__ inline double rhs_of(const double* __restrict__ C, const NonZero& nz, const double* phi, const double* psi)
{
    double rhs = 0.0;
#pragma unroll
    for (int k = 0; k < NB; ++k)
        if (column_live(nz, S, k)) rhs = rhs + psi[k] * column_q(C, S, k, phi);
    return rhs;
}

template <bool SAMPLES>
__global__ __launch_bounds__(NT) void step_kernel(const double* __restrict__ h, double* __restrict__ out,
                                                  const double* __restrict__ C, Geom g)
{
    C = sample_coef<SAMPLES>(C); h = sample<SAMPLES>(h, g); out = sample<SAMPLES>(out, g);
    const NonZero nz = nonzero_mask(C);
    const long idx = (long)blockIdx.x * NT + threadIdx.x;
    if (idx >= g.plane) return;
    const int y = (int)(idx / g.W), x = (int)(idx - (long)y * g.W);
    double u, v, psi[NB], phi[NA];
    library_fields(h, g, y, x, u, v, psi);
    monomials(u, v, phi);
    const double inc_u = g.dt * rhs_of<0>(C, nz, phi, psi), inc_v = g.dt * rhs_of<1>(C, nz, phi, psi);
    out[idx] = u + inc_u;
    out[g.plane + idx] = v + inc_v;
}

// ---- one Runge-Kutta step per launch -------------------------------------------------------------------------------------------
// f(y) at slot c of an LDS window y [2][FW * FW]: point_fields' expressions on LDS neighbours
template <int FW>
__device__ inline void rhs_window(const double* y, int c, const double* __restrict__ C, const NonZero& nz, const Geom& g, double& ku,
                                  double& kv)
{
    double psi[NB], phi[NA];
    psi[0] = 1.0;
    const double *pu = y + c, *pv = y + FW * FW + c;
    star_fields(g, pu[0], pu[-2 * FW], pu[-FW], pu[FW], pu[2 * FW], pu[-2], pu[-1], pu[1], pu[2], psi[1], psi[2], psi[5]);
    star_fields(g, pv[0], pv[-2 * FW], pv[-FW], pv[FW], pv[2 * FW], pv[-2], pv[-1], pv[1], pv[2], psi[3], psi[4], psi[6]);
    monomials(pu[0], pv[0], phi);
    ku = rhs_of<0>(C, nz, phi, psi);
    kv = rhs_of<1>(C, nz, phi, psi);
}

// window slot of point i of the region tile + M: the tile's FT^2 points first (point i of the tile is i of every region, so it
// stays on one lane through the stages), then the ring of width M: two bands of M rows over the region's FT + 2M columns, then
// FT rows of 2M columns.  0 <= i < (FT + 2M)^2
template <int FT, int M>
__device__ inline int region_slot(int i)
{
    constexpr int R = FT + 2 * M, FW = FT + 2 * FH;
    if (i < FT * FT) return (i / FT + FH) * FW + i % FT + FH;
    if constexpr (M > 0) {
        i -= FT * FT;
        int row, col;
        if (i < 2 * M * R) {
            row = i / R; col = i - row * R;
            row += row >= M ? FT : 0;
        } else {
            const int j = i - 2 * M * R;
            row = j / (2 * M); col = j - row * (2 * M);
            row += M; col += col >= M ? FT : 0;
        }
        return (row + FH - M) * FW + col + FH - M;
    }
    return 0;
}

// k = f(y) on the region tile + M and, for M > 0, the next stage state h + (k dt) / DIV there.  Lanes loop over the region's
// points; k of a lane's tile points (the leading KPL rounds) is returned in ku, kv
template <int FT, int M, int DIV>
__device__ inline void rk4_stage(const double* y, const double* hb, double* nb, const double* __restrict__ C, const NonZero& nz,
                                 const Geom& g, double* ku, double* kv)
{
    constexpr int FW = FT + 2 * FH, FWIN = FW * FW, NPTS = (FT + 2 * M) * (FT + 2 * M), KPL = (FT * FT + NT - 1) / NT;
    auto point = [&](int i, double& ru, double& rv) {
        const int c = region_slot<FT, M>(i);
        rhs_window<FW>(y, c, C, nz, g, ru, rv);
        if constexpr (M > 0) {
            nb[c] = hb[c] + (ru * g.dt) / (double)DIV;
            nb[FWIN + c] = hb[FWIN + c] + (rv * g.dt) / (double)DIV;
        }
    };
#pragma unroll
    for (int j = 0; j < KPL; ++j)
        if ((int)threadIdx.x + j * NT < NPTS) point(threadIdx.x + j * NT, ku[j], kv[j]);
    for (int i = threadIdx.x + KPL * NT; i < NPTS; i += NT) {
        double ru, rv;
        point(i, ru, rv);
    }
}

// grid (ceil(W / FT), ceil(H / FT), B).  out: the next state [B][2][H][W]; STAGES: y2, y3, y4 as [3][B][2][H][W]
template <int FT, bool STAGES, bool SAMPLES>
__global__ __launch_bounds__(NT) void rk4_kernel(const double* __restrict__ h, double* __restrict__ out,
                                                 const double* __restrict__ C, Geom g)
{
    constexpr int FW = FT + 2 * FH, FWIN = FW * FW, KPL = (FT * FT + NT - 1) / NT;
    __shared__ double hb[2 * FWIN], pb[2 * FWIN], qb[2 * FWIN];
    const int tid = threadIdx.x;
    const int ty0 = blockIdx.y * FT, tx0 = blockIdx.x * FT;
    C = sample_coef<SAMPLES>(C); h = sample<SAMPLES>(h, g); out = sample<SAMPLES>(out, g);
    const long planes = SAMPLES ? (long)gridDim.z * g.plane : g.plane;      // 2 planes: from y_i to y_{i+1} of the same sample
    const NonZero nz = nonzero_mask(C);
    // the halo may wrap the grid more than once: a true modulo
    for (int i = tid; i < FWIN; i += NT) {
        const int wy = i / FW, wx = i - wy * FW;
        const long o = (long)wrapi(ty0 - FH + wy, g.H) * g.W + wrapi(tx0 - FH + wx, g.W);
        hb[i] = h[o];
        hb[FWIN + i] = h[g.plane + o];
    }
    __syncthreads();
    // where this lane's tile points live (-1: none, or outside the grid -- such a lane evaluates wrapped points and stores nothing)
    int slot[KPL];
    long at[KPL];
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
        const int p = tid + j * NT, ly = p / FT, lx = p % FT;
        slot[j] = p < FT * FT ? (ly + FH) * FW + lx + FH : 0;
        at[j] = p < FT * FT && ty0 + ly < g.H && tx0 + lx < g.W ? (long)(ty0 + ly) * g.W + tx0 + lx : -1;
    }
    auto store_stage = [&](const double* yb, int i) {
        if (!STAGES) return;
#pragma unroll
        for (int j = 0; j < KPL; ++j)
            if (at[j] >= 0) {
                out[(2 * i) * planes + at[j]] = yb[slot[j]];
                out[(SAMPLES ? (2 * i) * planes + g.plane : (2 * i + 1) * g.plane) + at[j]] = yb[FWIN + slot[j]];
            }
    };
    double ku[KPL] = {}, kv[KPL] = {}, su[KPL], sv[KPL];
    rk4_stage<FT, 6, 2>(hb, hb, pb, C, nz, g, ku, kv);               // k1, y2
#pragma unroll
    for (int j = 0; j < KPL; ++j) { su[j] = ku[j]; sv[j] = kv[j]; }
    __syncthreads();
    store_stage(pb, 0);
    rk4_stage<FT, 4, 2>(pb, hb, qb, C, nz, g, ku, kv);               // k2, y3
#pragma unroll
    for (int j = 0; j < KPL; ++j) { su[j] = su[j] + 2.0 * ku[j]; sv[j] = sv[j] + 2.0 * kv[j]; }
    __syncthreads();
    store_stage(qb, 1);
    rk4_stage<FT, 2, 1>(qb, hb, pb, C, nz, g, ku, kv);               // k3, y4 (the reads of y2 ended at the barrier above)
#pragma unroll
    for (int j = 0; j < KPL; ++j) { su[j] = su[j] + 2.0 * ku[j]; sv[j] = sv[j] + 2.0 * kv[j]; }
    __syncthreads();
    store_stage(pb, 2);
    if (STAGES) return;                                             // no barrier follows
    rk4_stage<FT, 0, 1>(pb, hb, nullptr, C, nz, g, ku, kv);          // k4
#pragma unroll
    for (int j = 0; j < KPL; ++j)
        if (at[j] >= 0) {
            out[at[j]] = hb[slot[j]] + (g.dt * (su[j] + ku[j])) / 6.0;
            out[g.plane + at[j]] = hb[FWIN + slot[j]] + (g.dt * (sv[j] + kv[j])) / 6.0;
        }
}

// what multiplies the right-hand side's Jacobian at a point: dt G for the Euler step (prev NULL, a = dt), and for a Runge-Kutta
// stage kappa_i = a lambda + b ybar_{i+1}
struct Kappa {
    const double* lam;
    const double* prev;
    double a, b;
    __device__ void at(long o, long plane, double& ku, double& kv) const
    {
        ku = a * lam[o]; kv = a * lam[plane + o];
        if (prev) { ku = ku + b * prev[o]; kv = kv + b * prev[plane + o]; }
    }
};

// w_k = sum_s a_s q_{s,k}, k = 1 .. 6, of the grid point (gy, gx) into LDS slot `slot`; returns the point's values and a = kappa
__device__ inline void eval_w(const double* __restrict__ h, const Kappa& kap, const double* __restrict__ C, const Geom& g,
                              const bool* live, int gy, int gx, double (*wl)[LW * LW], int slot, double& u, double& v, double& au,
                              double& av, double* phi)
{
    const long o = (long)gy * g.W + gx;
    u = h[o]; v = h[g.plane + o];
    kap.at(o, g.plane, au, av);
    monomials(u, v, phi);
#pragma unroll
    for (int k = 1; k < NB; ++k)
        if (live[k]) wl[k - 1][slot] = au * column_q(C, 0, k, phi) + av * column_q(C, 1, k, phi);
}

// One 16 x 16 tile of J(h)^T kappa and of the coefficient-gradient row, for the Euler adjoint step and for a Runge-Kutta stage.
//   Euler (STAGE false): out = lam + inject + J(h)^T kappa, summed onto lam + inject term by term.
//   STAGE:               ybar (may be NULL) = J(h)^T kappa summed from zero;  out = (acc + inject) + ybar.  out may be acc
//                        (each lane reads and writes its own point only); it is never lam or prev, which are read with a halo.
template <bool STAGE>
__device__ inline void adjoint_body(const double* __restrict__ h, const Kappa kap, const double* __restrict__ inject,
                                    const double* acc, double* __restrict__ ybar, double* out, const double* __restrict__ C,
                                    double* __restrict__ rows, const Geom& g)
{
    __shared__ double wl[NB - 1][LW * LW];
    __shared__ double stg[NWAVES][64 * STG];
    __shared__ double red[NCOEF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lx = tid & (TS - 1), ly = tid >> 4;
    const int ty0 = blockIdx.y * TS, tx0 = blockIdx.x * TS;

    const NonZero nz = nonzero_mask(C);
    bool live[NB];                                                  // wave-uniform: column k carries a coefficient
#pragma unroll
    for (int k = 0; k < NB; ++k) live[k] = column_live(nz, 0, k) || column_live(nz, 1, k);

    // w at the tile's points (lanes outside the grid evaluate the wrapped point: it is the halo of a lane inside) ...
    const bool inside = ty0 + ly < g.H && tx0 + lx < g.W;
    const int gy = wrapi(ty0 + ly, g.H), gx = wrapi(tx0 + lx, g.W);
    const int slot = (ly + HALO) * LW + lx + HALO;
    double u, v, au, av, phi[NA];
    eval_w(h, kap, C, g, live, gy, gx, wl, slot, u, v, au, av, phi);
    // ... and at the 4 x 32 points of the star halo
    if (tid < 128) {
        const int strip = tid >> 5, j = tid & 31;
        int py, px;
        if (strip < 2) { py = (j >> 4) + (strip ? TS + HALO : 0); px = (j & 15) + HALO; }
        else           { py = (j & 15) + HALO; px = (j >> 4) + (strip == 3 ? TS + HALO : 0); }
        double u_, v_, au_, av_, phi_[NA];
        eval_w(h, kap, C, g, live, wrapi(ty0 + py - HALO, g.H), wrapi(tx0 + px - HALO, g.W), wl, py * LW + px, u_, v_, au_, av_,
               phi_);
    }
    __syncthreads();

    double psi[NB], uc, vc;
    library_fields(h, g, gy, gx, uc, vc, psi);
    // pointwise part: sum_k psi_k sum_m (a_u C[u][m][k] + a_v C[v][m][k]) dphi_m/dh_s
    const double du_phi[NA] = {0.0, 1.0, 0.0, 2.0 * u, v, 0.0, 3.0 * phi[3], 2.0 * phi[4], phi[5], 0.0};
    const double dv_phi[NA] = {0.0, 0.0, 1.0, 0.0, u, 2.0 * v, 0.0, phi[3], 2.0 * phi[4], 3.0 * phi[5]};
    const long o = (long)gy * g.W + gx;
    double ou = 0.0, ov = 0.0;
    if (!STAGE) {
        ou = kap.lam[o]; ov = kap.lam[g.plane + o];
        if (inject) { ou += inject[o]; ov += inject[g.plane + o]; }
    }
#pragma unroll
    for (int k = 0; k < NB; ++k)
        if (live[k]) {
            double su = 0.0, sv = 0.0;
#pragma unroll
            for (int m = 1; m < NA; ++m) {
                const double r = au * C[cidx(0, m, k)] + av * C[cidx(1, m, k)];
                su += r * du_phi[m]; sv += r * dv_phi[m];
            }
            ou += psi[k] * su; ov += psi[k] * sv;
        }
    // transposed stencils on w: D0^T = -D0, D1^T = -D1, Lap^T = Lap
    auto d0 = [&](const double* f) {
        return ((f[slot - 2 * LW] - f[slot + 2 * LW]) + 8.0 * (f[slot + LW] - f[slot - LW])) * g.inv_12dx;
    };
    auto d1 = [&](const double* f) { return ((f[slot - 2] - f[slot + 2]) + 8.0 * (f[slot + 1] - f[slot - 1])) * g.inv_12dx; };
    auto lap = [&](const double* f) {
        return ((-1.0 / 12.0) * ((f[slot - 2 * LW] + f[slot + 2 * LW]) + (f[slot - 2] + f[slot + 2])) +
                (4.0 / 3.0) * ((f[slot - LW] + f[slot + LW]) + (f[slot - 1] + f[slot + 1])) - 5.0 * f[slot]) * g.inv_dx2;
    };
    if (live[1]) ou -= d0(wl[0]);
    if (live[2]) ou -= d1(wl[1]);
    if (live[5]) ou += lap(wl[4]);
    if (live[3]) ov -= d0(wl[2]);
    if (live[4]) ov -= d1(wl[3]);
    if (live[6]) ov += lap(wl[5]);
    if (inside) {
        if (STAGE) {
            if (ybar) { ybar[o] = ou; ybar[g.plane + o] = ov; }
            double bu = acc[o], bv = acc[g.plane + o];
            if (inject) { bu += inject[o]; bv += inject[g.plane + o]; }
            ou = bu + ou; ov = bv + ov;
        }
        out[o] = ou; out[g.plane + o] = ov;
    }

    // coefficient gradients: stage this lane's point, then 16 groups of 4 points through the matrix cores
    double* mine = &stg[wave][lane * STG];
#pragma unroll
    for (int m = 0; m < NA; ++m) mine[m] = phi[m];
    mine[NA] = inside ? au : 0.0;
    mine[NA + 1] = inside ? av : 0.0;
#pragma unroll
    for (int k = 0; k < NB; ++k) mine[NA + 2 + k] = inside ? psi[k] : 0.0;
    __syncthreads();
    const int r = lane & 15, kq = lane >> 4;
    const int s0 = r >= NA ? 1 : 0, m0 = r - NA * s0;               // row r of tile 0; row 16 + r of tile 1 is (v, 6 + r)
    d4 acc0 = d4{0.0, 0.0, 0.0, 0.0}, acc1 = d4{0.0, 0.0, 0.0, 0.0};
    for (int grp = 0; grp < 16; ++grp) {
        const double* P = &stg[wave][(grp * 4 + kq) * STG];
        const double a0 = P[NA + s0] * P[m0];
        const double a1 = r < 2 * NA - 16 ? P[NA + 1] * P[r + 16 - NA] : 0.0;
        const double b = r < NB ? P[NA + 2 + r] : 0.0;
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc1, 0, 0, 0);
    }
    // the workgroup's waves in a fixed order: wave 0 stores, waves 1.. add
    for (int w = 0; w < NWAVES; ++w) {
        if (wave == w && r < NB) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                double* e = &red[(kq + 4 * reg) * NB + r];
                *e = (w == 0 ? 0.0 : *e) + acc0[reg];
            }
            double* e = &red[(16 + kq) * NB + r];
            *e = (w == 0 ? 0.0 : *e) + acc1[0];
        }
        __syncthreads();
    }
    if (tid < NCOEF) {
        double* row = rows + ((long)blockIdx.y * gridDim.x + blockIdx.x) * NCOEF;
        row[tid] = row[tid] + red[tid];
    }
}

// the rows of partial sums of this workgroup's sample
template <bool SAMPLES>
__device__ inline double* sample_rows(double* rows)
{
    if constexpr (!SAMPLES) return rows;
    return rows + (long)blockIdx.z * gridDim.y * gridDim.x * NCOEF;
}

// grid (ceil(W / 16), ceil(H / 16), B); inject may be NULL (the frame carries no gradient); rows: [B][blocks][140], added to
template <bool SAMPLES>
__global__ __launch_bounds__(NT) void adjoint_kernel(const double* __restrict__ h, const double* __restrict__ G,
                                                     const double* __restrict__ inject, double* __restrict__ out,
                                                     const double* __restrict__ C, double* __restrict__ rows, Geom g)
{
    adjoint_body<false>(sample<SAMPLES>(h, g), Kappa{sample<SAMPLES>(G, g), nullptr, g.dt, 0.0}, sample_opt<SAMPLES>(inject, g),
                        nullptr, nullptr, sample<SAMPLES>(out, g), sample_coef<SAMPLES>(C), sample_rows<SAMPLES>(rows), g);
}

// one Runge-Kutta stage of the adjoint, same grid: y the stage state, kappa = a lam + b prev (prev NULL: a lam);
// ybar (may be NULL) = J(y)^T kappa;  out = (acc + inject) + ybar, out may be acc.  g.dt is not used: a and b carry it
template <bool SAMPLES>
__global__ __launch_bounds__(NT) void rk4_stage_kernel(const double* __restrict__ y, const double* __restrict__ lam,
                                                       const double* __restrict__ prev, double a, double b,
                                                       const double* __restrict__ inject, const double* acc,
                                                       double* __restrict__ ybar, double* out, const double* __restrict__ C,
                                                       double* __restrict__ rows, Geom g)
{
    adjoint_body<true>(sample<SAMPLES>(y, g), Kappa{sample<SAMPLES>(lam, g), sample_opt<SAMPLES>(prev, g), a, b},
                       sample_opt<SAMPLES>(inject, g), sample<SAMPLES>(acc, g), sample_opt<SAMPLES>(ybar, g), sample<SAMPLES>(out, g),
                       sample_coef<SAMPLES>(C), sample_rows<SAMPLES>(rows), g);
}

// one workgroup per sample (grid (1, 1, B)): sums the sample's `nrows` partial rows in row order into gC [B][140]
__global__ __launch_bounds__(FIN_NT) void finish_kernel(const double* __restrict__ rows, int nrows, double* __restrict__ gC)
{
    const int e = threadIdx.x;
    if (e >= NCOEF) return;
    rows += (long)blockIdx.z * nrows * NCOEF;
    double s = 0.0;
    for (int r = 0; r < nrows; ++r) s += rows[(long)r * NCOEF + e];
    gC[blockIdx.z * NCOEF + e] = s;
}

}  // namespace lib
}  // namespace pi
