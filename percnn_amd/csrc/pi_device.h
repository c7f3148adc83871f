// pi_device.h -- device-side helpers shared by the Pi-block kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pi {

// ---- parameter block layout (documented in include/percnn_pi.h) ------------------------------
constexpr int P_DT = 0, P_COEF = 1, P_C0 = 3, P_TAPS = 4, P_W = 16;
__host__ __device__ constexpr int species_block(int hc) { return 10 * hc + 1; }
// hc == 0 selects the pre-contracted polynomial reaction: 16 header slots + 2 x 10 cubic coefficients
constexpr int POLY = -1;          // template tag for that mode
constexpr int NPOLY = P_W + 20;
// hc == -1 selects the advective polynomial block of the Stage-3 physics-based cells (60 entries, pi_adv.h)
__host__ __device__ constexpr int nparams(int hc) { return hc == 0 ? NPOLY : (hc == -1 ? 60 : P_W + 2 * species_block(hc)); }

constexpr int WAVE = 64;          // CDNA wavefront
constexpr int NXCD = 8;           // MI355X: 8 XCDs, block b is dispatched to XCD b % 8

// Flavours of a step kernel (one state / B states, one block: "batched" / B states, B blocks: "ensemble") are ONE __global__
// template whose argument list carries parameter packs: empty for one state, `long sample` (+ one int) for the others, read
// with flavour_arg<I>(pack...) under `if constexpr`.  A kernel template and not a __device__ body behind three thin kernels:
// through a call the __restrict__ kernel arguments lose their meaning, and every kernel came out with another register
// allocation (instruction counts off by up to 9 %, SGPR spills 2 -> 25 in the RZ = 2 forward); with the packs each flavour's
// code is, instruction for instruction, what a hand-written kernel with that argument list gives (tools/compare_kernels.py).
template <int I, typename A, typename... R>
__device__ __forceinline__ auto flavour_arg(A a, R... r)
{
    if constexpr (I == 0) return a;
    else return flavour_arg<I - 1>(r...);
}

// 16-byte vector access: 4 x f32 or 2 x f64 per lane -> 1 KiB per wave-instruction
template <typename T> struct vec_width;
template <> struct vec_width<float>  { static constexpr int value = 4; };
template <> struct vec_width<double> { static constexpr int value = 2; };

template <typename T, int N> struct alignas(sizeof(T) * N) Pack { T v[N]; };

template <typename T, int N>
__device__ __forceinline__ Pack<T, N> ld(const T* p) { return *reinterpret_cast<const Pack<T, N>*>(p); }
template <typename T, int N>
__device__ __forceinline__ void st(T* p, const Pack<T, N>& x) { *reinterpret_cast<Pack<T, N>*>(p) = x; }

// Write-through (sc1, agent scope) 16-byte store for the frames the 2D tile kernels write.  Those frames are consumed by the
// NEXT launch (all XCDs) or much later by the backward, never again by the launch that wrote them, and a dependent kernel
// boundary costs + (dirty bytes / ~6 TB/s) for the L2 write-back at kernel end (MI355X_MICROARCH.md, row "boundary": a K = 4
// forward launch leaves 8 MiB dirty).  Written through while the kernel still computes, that drain is off the boundary:
// measured on MI355X 512^2 forward 2.00 -> 1.84 us per step, lambda-omega 512^2 fp64 3.0 -> 2.78, 2048^2 16.3 -> 15.4
// (profiles/r02_write_through_stores.txt); the direct 3D kernels do not gain (128^3 11.3 -> 11.7) and keep plain stores.
// The compiler only emits sc1 on <= 8-byte atomic stores (two 8-byte sc1 stores per lane were measured SLOWER than plain
// stores: 512^2 forward 2.28 us), hence inline asm; the s_nop covers the gfx9 hazard "VMEM store of more than 64 bits
// followed by a write of its data VGPRs", which the hazard recogniser cannot see through inline asm (without it: corrupted
// frames -- caught by the parity tests).
template <typename T, int N>
__device__ __forceinline__ void st_frame_wt(T* p, const Pack<T, N>& x)
{
    if constexpr (sizeof(T) * N == 16) {
        typedef unsigned v4u __attribute__((ext_vector_type(4)));
        const v4u v = __builtin_bit_cast(v4u, x);
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
    } else {
        *reinterpret_cast<Pack<T, N>*>(p) = x;
    }
}

// Explicit fused multiply-add; the translation unit is built with -ffp-contract=off so every
// other a*b+c keeps its two roundings (the reference rounds `coef*lap + react` and `h + res*dt`
// separately -- train_2drd.py:115-118).
__device__ __forceinline__ float  fma_(float a, float b, float c)    { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }

// the 10 wave-uniform scalars of one hidden channel {w1u,w1v,b1, w2u,w2v,b2, w3u,w3v,b3, w4}
template <typename T> struct W10 { T w[10]; };
template <typename T>
__device__ __forceinline__ W10<T> load_w10(const T* __restrict__ p)
{
    W10<T> r;
#pragma unroll
    for (int i = 0; i < 10; ++i) r.w[i] = p[i];
    return r;
}

// ---- pre-contracted reaction: r_s(u,v) = sum_m c[m] phi_m, phi = {1,u,v,u2,uv,v2,u3,u2v,uv2,v3} -------
// The Hadamard product of the three 1x1 branches followed by the 1x1 aggregation
// (train_2drd.py:115-116) IS this cubic; evaluating it in Horner form costs 9 FMAs per species
// instead of 72 VALU ops at Hc = 8, independent of Hc.
template <typename T>
__device__ __forceinline__ T poly_r(const T* __restrict__ c, T u, T v)
{
    const T A0 = fma_(v, fma_(v, fma_(v, c[9], c[5]), c[2]), c[0]);
    const T A1 = fma_(v, fma_(v, c[8], c[4]), c[1]);
    const T A2 = fma_(v, c[7], c[3]);
    return fma_(u, fma_(u, fma_(u, c[6], A2), A1), A0);
}
// dr/du and dr/dv
template <typename T>
__device__ __forceinline__ void poly_dr(const T* __restrict__ c, T u, T v, T& ru, T& rv)
{
    const T A1 = fma_(v, fma_(v, c[8], c[4]), c[1]);
    const T A2x2 = fma_(v, T(2) * c[7], T(2) * c[3]);
    ru = fma_(u, fma_(u, T(3) * c[6], A2x2), A1);
    const T B0 = fma_(v, fma_(v, T(3) * c[9], T(2) * c[5]), c[2]);
    const T B1 = fma_(v, T(2) * c[8], c[4]);
    rv = fma_(u, fma_(u, c[7], B1), B0);
}

// ---- loss gradient formed inside the adjoint sweep (round 3) -------------------------------------------------------------
// A sweep kernel is handed the frame to "inject" at step t-1 as a pointer.  mode 0: that frame IS dL/dh_{t-1} (the caller
// materialised it).  For the squared-error losses of the reference (train_2drd.py:397-407: MSE against data; SURVEY 8d:
// mean(traj^2)) the frame is a function of operands the sweep reads anyway, so the caller need not materialise it:
//   mode 1:  dL/dh_{t-1} = a * h_{t-1}                 (the pointer is the state frame itself, no extra bytes: 24 B / point)
//   mode 2:  dL/dh_{t-1} = a * (h_{t-1} - target_{t-1})  (the pointer is the target frame)
// with a = scale * (dev ? *dev : 1) -- the host factor (2 / N for a mean) times the scalar autograd hands the loss, read from
// device memory so that no host synchronisation is needed.  One subtraction and one multiplication, separately rounded:
// the same values ATen's mse_loss / pow backward writes into a materialised dL/dtraj.
// Sample flavours of the kernels (flavour_arg above): `dev` is a vector of B elements, one factor per sample -- each member of
// a batch or an ensemble has a loss and an upstream gradient of its own -- and workgroup (x, b) reads dev[b]: wave-uniform,
// so still a scalar load.
struct LossInj {
    double scale;
    const void* dev;        // nullable; one element of the compute type (sample flavours: B elements)
    int mode;               // 0, 1, 2
};
// S... = the sample index of this workgroup, passed by the sample flavours alone
template <typename T, typename... S>
__device__ __forceinline__ T loss_factor(const LossInj& l, S... sample)
{
    if constexpr (sizeof...(S) == 1)
        return (T)l.scale * (l.dev ? static_cast<const T*>(l.dev)[flavour_arg<0>(sample...)] : T(1));
    else
        return (T)l.scale * (l.dev ? *static_cast<const T*>(l.dev) : T(1));
}
// value to add to the adjoint state: j = the value loaded through the injection pointer, h = the state at that point
template <typename T>
__device__ __forceinline__ T loss_inject(int mode, T a, T h, T j)
{
    if (mode == 0) return j;
    const T d = mode == 2 ? h - j : h;
    return a * d;
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() makes hipcc drain the vector-memory
// counter (s_waitcnt vmcnt(0)) first, which would serialise every software-prefetched global load and
// every in-flight trajectory store behind the barrier; LDS visibility needs lgkmcnt(0) alone.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ int wrap(int i, int n) { i %= n; return i < 0 ? i + n : i; }
// stencil neighbours: i in [-2, n+1] and n >= 2, so one conditional add/sub is the periodic wrap.  The runtime `%`
// above is ~20 quarter-rate integer instructions; eight of them per point made the direct 3D kernels VALU-bound.
__device__ __forceinline__ int wrap_near(int i, int n) { return i < 0 ? i + n : (i >= n ? i - n : i); }

// exact x / d for 0 <= x < 2^31 from host-computed (m, s): d == 1 -> m = 0;  else l = ceil(log2 d),
// m = ceil(2^(31+l) / d) (< 2^32), s = l - 1 and  x / d == umulhi(x, m) >> s   (Granlund-Montgomery, N = 31)
struct FastDiv {
    unsigned m, s;
    __device__ __forceinline__ unsigned div(unsigned x) const { return m ? (__umulhi(x, m) >> s) : x; }
    // d >= 2 known: no test of m (a wave-uniform test becomes a scalar branch, i.e. a basic-block boundary that keeps the
    // scheduler from batching the loads on either side of it)
    __device__ __forceinline__ unsigned div_nz(unsigned x) const { return __umulhi(x, m) >> s; }
};

// ---- sparse-observation loss form (the reference's own data loss: mse_loss(output[::15, :, ::2, ::2, ::2], truth[...])) --------
// The loss lives on the sub-lattice x_d % s_d == 0 of the observed frames and the target is COMPACT: frame [B][2][*Sc],
// Sc_d = ceil(S_d / s_d), one frame per observed frame.  Axes are numbered slowest first and always three: a 2D grid is
// (1, H, W) with stride 1 on the leading axis.  floor(x / s) is a valid compact coordinate for EVERY x, so a target load at the
// floor index is always in bounds and can stay unconditional; the point is on the lattice iff q * s == x.
// The sweeps keep the mode-2 arithmetic a * (h - j) of loss_inject: their loaders hand it j = the target value (0 without a
// target) on the lattice and j = h off it, where it gives a * (h - h) = 0 -- what a materialised gradient holds there.
// Sample flavours only; the description travels as the LAST trailing kernel argument (ObsLat: direct kernel, top frame, loss
// value; ObsTile: 2D tile sweep).  No resident, brick or plane-streaming kernel is instantiated with it.
struct ObsLat {
    FastDiv d[3];           // x / s per axis
    int s[3];               // strides
    int sc[3];              // compact extents
    long cs;                // compact species stride = sc[0] * sc[1] * sc[2]; a compact sample is 2 * cs elements
    int has_target;         // 0: the target is zero and no target pointer is read
};
// the tile sweep injects up to K frames per launch, and the observed ones are not a uniform stride apart in the time-compact
// target: one element offset per sub-step (sub-step m injects frame t - 1 - m), relative to `target` = sample 0 of compact frame 0
struct ObsTile {
    ObsLat lat;
    const void* target;     // compact target [n][B][2][*Sc] of the compute type; nullptr <=> !lat.has_target
    long coff[8];
};
template <typename A, typename B> struct same_type { static constexpr bool value = false; };
template <typename A> struct same_type<A, A> { static constexpr bool value = true; };
// number of lattice descriptions in a flavour pack (0 or 1, the last argument)
template <typename... X> struct obs_args { static constexpr int value = 0; };
template <typename A, typename... X> struct obs_args<A, X...> {
    static constexpr int value = ((same_type<A, ObsLat>::value || same_type<A, ObsTile>::value) ? 1 : 0) + obs_args<X...>::value;
};
// compact coordinate of x on axis `a` and whether x is a lattice coordinate
__device__ __forceinline__ unsigned obs_q(const ObsLat& l, int a, unsigned x, bool& on)
{
    const unsigned q = l.d[a].div(x);
    on = q * (unsigned)l.s[a] == x;
    return q;
}

// XCD-aware block remap: hand each XCD (private 4 MiB L2) a contiguous range of the grid so the
// axis-0 neighbours of a block's rows are served by the same L2.  Pure speed; any mapping is correct.
// Any block count: XCD x (the blocks with bid % 8 == x) gets the contiguous range starting at x*q + min(x, r), q = n / 8,
// r = n % 8 -- the first r XCDs hold one block more.  (Was: identity unless n % 8 == 0, which cost a 1800^2 grid with a
// block count of 3165 a quarter of its speed against 3600 blocks.)
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nblocks)
{
    const unsigned q = nblocks / NXCD, r = nblocks % NXCD, x = bid % NXCD;
    return x * q + min(x, r) + bid / NXCD;
}

// ---- wave-level sum (all 64 lanes) -----------------------------------------------------------
// DPP row shifts + row broadcasts: 6 VALU adds, no LDS crossbar traffic. Total lands in lane 63.  (ds_bpermute butterflies are 6
// dependent LDS-crossbar round trips per sum: the two fp64 sums at the end of the tile adjoint kernel cost ~1 us that way.)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_mov(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, true));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_mov(double v)
{
    const long long b = __builtin_bit_cast(long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffLL), CTRL, ROW_MASK, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xF, true);
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}
template <typename T>
__device__ __forceinline__ T wave_sum_to_last(T v)
{
    v += dpp_mov<0x111, 0xF>(v);   // row_shr:1
    v += dpp_mov<0x112, 0xF>(v);   // row_shr:2
    v += dpp_mov<0x114, 0xF>(v);   // row_shr:4
    v += dpp_mov<0x118, 0xF>(v);   // row_shr:8   -> lane 15 of each row holds the row total
    v += dpp_mov<0x142, 0xA>(v);   // row_bcast:15 into rows 1,3
    v += dpp_mov<0x143, 0xC>(v);   // row_bcast:31 into rows 2,3 -> lane 63 holds the wave total
    return v;
}
constexpr int REDUCE_LANE = 63;

}  // namespace pi
