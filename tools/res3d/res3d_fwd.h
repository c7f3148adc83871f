// res3d_fwd.h -- the RESIDENT 3D FORWARD rollout (round 6): pi_fwd3d_resident_kernel and its strip, on the hand-over machinery of
// percnn_amd/csrc/pi_res3d.h (window layout, task schedule, Ring / publish / request / landed / unpack).  The library launches the
// resident reverse sweep only (launch_adj_res3d); this kernel is built by tools/res3d/res3d_dev.hip alone, which includes this
// header after pi_res3d.h.  It is kept as the starting point of a K = 2 forward.
#pragma once
#include "../../percnn_amd/csrc/pi_res3d.h"

namespace pi {
namespace r3d {

// one strip (4 points along x, both species) of one forward step, operands from the LDS window; pi::star's order: centre,
// axis 0 (-2, -1, +1, +2), axis 1, axis 2; coef * lap + react and h + res * dt keep their two roundings (train_3drd.py:123-139)
// `fr` (nullable, wave-uniform): frame of the state being READ -- the strip's own values are stored there on the way.  The frame
// of step t thus leaves during the strips of step t + 1, two stores at a time between arithmetic, instead of as one burst of 64 KB
// per CU that the ring request would queue behind (a CU drains ~12 B per clock to memory: 2.2 us of a step).
__device__ __forceinline__ void fwd_strip(const unsigned char* smem, unsigned lo, const float* __restrict__ P, v4f& ou, v4f& ov,
                                          float* fr, long ss, unsigned go)
{
    v4f c[2], lap[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const unsigned char* b = smem + s * SP + lo;
        c[s] = lds4(b);
        if (fr) *(gv4f*)((gchar*)(fr + s * ss) + go) = c[s];
        v4f l;
#pragma unroll
        for (int i = 0; i < 4; ++i) l[i] = P[P_C0] * c[s][i];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k = t < 2 ? t - 2 : t - 1;
            const v4f nb = lds4(b + k * ZS);
            const float w = P[P_TAPS + t];
#pragma unroll
            for (int i = 0; i < 4; ++i) l[i] = fma_(w, nb[i], l[i]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k = t < 2 ? t - 2 : t - 1;
            const v4f nb = lds4(b + k * YS);
            const float w = P[P_TAPS + 4 + t];
#pragma unroll
            for (int i = 0; i < 4; ++i) l[i] = fma_(w, nb[i], l[i]);
        }
        const v2f xl = lds2(b - 8), xr = lds2(b + 16);
        const float win[8] = {xl[0], xl[1], c[s][0], c[s][1], c[s][2], c[s][3], xr[0], xr[1]};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k = t < 2 ? t - 2 : t - 1;
            const float w = P[P_TAPS + 8 + t];
#pragma unroll
            for (int i = 0; i < 4; ++i) l[i] = fma_(w, win[2 + i + k], l[i]);
        }
        lap[s] = l;
    }
    const float dt = P[P_DT];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const float* cf = P + P_W + 10 * s;
        const float coef = P[P_COEF + s];
        v4f o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float rr = poly_r(cf, c[0][i], c[1][i]);
            const float res = coef * lap[s][i] + rr;
            const float inc = res * dt;
            o[i] = c[s][i] + inc;
        }
        if (s == 0) ou = o; else ov = o;
    }
}

// forward rollout: frames[0] is the initial state (read), frames[1 .. nsteps] are written.
// Per step:  S: the strips that read the halo, their faces staged | publish | I: the interior strips, the ring requested after the
// first of them | write-back | ring lands, halo unpacked -- publish to need is the whole of I + write-back (~2.5 us).
template <int NT>
__global__ void __launch_bounds__(NT, 1)
pi_fwd3d_resident_kernel(float* __restrict__ frames, const float* __restrict__ P, Args a, unsigned long long* stamps)
{
    using S = Shape<NT>;
    constexpr int SLOTS = S::SLOTS, NW = S::NW, BOX_BYTES = S::BOX_BYTES;
    constexpr int WS = NS / WAVE;                                       // wave-slots of phase S
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned char* smem = smem_raw + 8;                                 // the window (see ROWB)
    int* wg_abort = reinterpret_cast<int*>(smem + STG0 + NGRAN * 16);
    const int tid = (int)threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int nblk = a.gz * a.gy * a.gx;
    const int b = (int)blockIdx.x;
    int bx, by, bz;
    const unsigned local = locate_block(a, b, bz, by, bx);
    const unsigned skipf = ((a.skip & 1) ? local : 0u) | ((a.skip & 2) ? (~local & 63u) : 0u);
    const int me = (bz * a.gy + by) * a.gx + bx;                        // outbox slot = block number (not workgroup number)
    if (tid == 0) {
        *wg_abort = 0;
        const unsigned n = __hip_atomic_fetch_add(a.sync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
        if (n == (unsigned)nblk && a.host) __hip_atomic_store(a.host, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const int half_bytes = nblk * BOX_BYTES;
    const __amdgpu_buffer_rsrc_t box = __builtin_amdgcn_make_buffer_rsrc(a.outbox, 0, 2 * half_bytes, 0x00020000);

    // ---- fixed geometry of this lane -------------------------------------------------------------------------------------
    unsigned lo[SLOTS], go[SLOTS], tk[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        const Task t = task_of<NT>(s, tid);
        lo[s] = lds_of(t);
        tk[s] = (unsigned)t.z | (unsigned)t.y << 8 | (unsigned)t.xs << 16;
        go[s] = (unsigned)((((bz * BZ + t.z) * a.n1 + by * BY + t.y) * a.n2 + bx * BX + 4 * t.xs) * 4);
    }
    Ring<NT> R;
    ring_setup<NT>(R, a, bz, by, bx, local);

    // ---- the window of frame 0: own block and halo straight from memory ---------------------------------------------------
    for (int i = tid; i < 2 * (BZ + 4) * (BY + 4) * (BX + 4); i += NT) {
        const int x = i % (BX + 4), y = (i / (BX + 4)) % (BY + 4), z = (i / ((BX + 4) * (BY + 4))) % (BZ + 4), s = i / ((BX + 4) * (BY + 4) * (BZ + 4));
        const int g0 = (bz * BZ + z - 2 + a.n0) % a.n0, g1 = (by * BY + y - 2 + a.n1) % a.n1, g2 = (bx * BX + x - 2 + a.n2) % a.n2;
        const float v = frames[s * a.ss + ((long)g0 * a.n1 + g1) * a.n2 + g2];
        *reinterpret_cast<float*>(smem + s * SP + z * ZS + y * YS + OWN0 - 8 + 4 * x) = v;
    }
    __syncthreads();

    Landing<NT> L;
    bool failed = false;
    for (int t = 0; t < a.nsteps; ++t) {
        const unsigned ep = (unsigned)t + 1u;                           // the state this step produces
        const bool more = t + 1 < a.nsteps, ring = more && !(a.skip & 4);
        float* fr = t > 0 ? frames + (long)t * a.frame_stride : nullptr;      // frame 0 is the caller's
        v4f ou[SLOTS], ov[SLOTS];
        R3D_STAMP(0);
        // ---- phase S: the strips that read the halo; what the neighbours wait for goes to the staging area ----
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
            if (s * NW + wave < WS) {                                   // wave-uniform
                fwd_strip(smem, lo[s], P, ou[s], ov[s], fr, a.ss, go[s]);
                const Task tt = {(int)(tk[s] & 255u), (int)(tk[s] >> 8 & 255u), (int)(tk[s] >> 16)};
                stage_strip(smem, tt, ou[s], ov[s]);
            }
        R3D_STAMP(1);
        lds_barrier();                                                  // faces staged; nobody reads the halo of state t any more
        R3D_STAMP(2);
        if (ring) {
            const __amdgpu_buffer_rsrc_t mine = __builtin_amdgcn_make_buffer_rsrc(
                static_cast<char*>(a.outbox) + ((size_t)(ep & 1u) * (size_t)half_bytes + (size_t)me * BOX_BYTES), 0, BOX_BYTES, 0x00020000);
            publish<NT>(smem, R, mine, ep, skipf);
        }
        R3D_STAMP(3);
        // ---- phase I: interior strips; the ring of state t + 1 is requested after the first of them ----
        bool asked = !ring;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s)
            if (s * NW + wave >= WS) {
                fwd_strip(smem, lo[s], P, ou[s], ov[s], fr, a.ss, go[s]);
                if (!asked) {
                    for (int i = 0; i < a.pause; ++i) __builtin_amdgcn_s_sleep(1);
                    request<NT>(L, R, box, (int)(ep & 1u) * half_bytes, skipf);
                    asked = true;
                }
            }
        R3D_STAMP(4);
        lds_barrier();                                                  // every read of state t is done
        R3D_STAMP(5);
        // ---- state t + 1 into the window ----
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            *reinterpret_cast<v4f*>(smem + lo[s]) = ou[s];
            *reinterpret_cast<v4f*>(smem + SP + lo[s]) = ov[s];
        }
        if (!more) {                                                    // the last frame has no next step to carry it
            float* out = frames + (long)(t + 1) * a.frame_stride;
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                *(gv4f*)((gchar*)out + go[s]) = ou[s];
                *(gv4f*)((gchar*)(out + a.ss) + go[s]) = ov[s];
            }
            break;
        }
        R3D_STAMP(6);
        // ---- the halo of state t + 1 lands ----
        if (ring) {
            const int rd = (int)(ep & 1u) * half_bytes;
            const unsigned long long t0 = ticks();
            const unsigned long long bound = t == 0 ? a.first_timeout_ticks : a.timeout_ticks;
            while (!landed<NT>(L, R, box, rd, ep, skipf)) {
                if (ticks() - t0 > bound || __hip_atomic_load(a.sync + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) { failed = true; break; }
                __builtin_amdgcn_s_sleep(1);
            }
            if (failed) {
                if (tid % WAVE == 0) *wg_abort = 1;
            } else {
                unpack<NT>(smem, L, R, skipf);
            }
        }
        R3D_STAMP(7);
        lds_barrier();
        if (*wg_abort) {
            // ABORT: the host learns it from its status slot and runs the launch-per-step kernels instead; frames already
            // written are the correct ones, nothing of the ones not yet written is
            if (tid == 0) {
                __hip_atomic_fetch_add(a.sync + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__hip_atomic_exchange(a.sync + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u && a.host) {
                    __hip_atomic_store(a.host + 1, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(a.host + 2, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(a.host + 3, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
            return;
        }
    }
}

}  // namespace r3d
}  // namespace pi
