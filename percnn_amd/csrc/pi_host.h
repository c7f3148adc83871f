// pi_host.h -- the HOST runtime of libpercnn_pi.so, defined in pi_host.hip and shared by the translation units that launch
// kernels (pi_abi.hip, pi_s1_abi.hip).  Not part of the C-ABI.  Four things, none of which names a kernel:
//   Options     the table of tuning options, its process-wide defaults and the "key=value,..." parser
//   Problem     an entry point's validated shape + options, and the block decomposition of the direct kernels (pi::Geom)
//   SideStream  one side stream + event ring per host thread and device
//   residency   the host side of the protocol of the resident ("persistent") launches: slot claim, per-device scratch, the
//               "launched" step with the roll-call wait, the abort bookkeeping.  Its state (PersistGuard, one per process) and
//               the option defaults are objects of pi_host.hip alone: every unit reaches them through the functions below, so
//               there is one resident grid per device however many units launch one.
// pi_host.hip holds no kernel and compiles in seconds; this header is read by every unit, so an edit HERE (a default of
// Options, say) still rebuilds all of them.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "pi_device.h"

namespace pi { struct Geom; }     // pi_kernels.h

namespace pi_host {

struct Options {
    int block = 256;
    int vec = 0;            // 0 = widest legal (16 B per lane); 1/2/4 = cap (tuning aid)
    int wgrad_blocks = 1024;
    int tile = 1;           // 2D: temporally blocked LDS kernels where the shape allows
    int tile_k = 4;         // sub-steps per launch (2 or 4)
    int tile_nt = 512;      // workgroup size of the tile kernels (256 or 512)
    int stream3d = 1;       // 3D: plane-streaming kernels where the shape allows (W = 64*VEC)
    int tile_fuse = 1;      // 2D tile sweep (float32 poly, K = 4, 32x32 tiles, 512 threads): reduce the 20 coefficient moments
                            // inside the sweep launches and keep only the hand-over adjoint frames (no moments pass)
    int bwd_cpl = 2;        // direct adjoint kernel: chunks per lane (grid-stride) while >= 512 workgroups remain; measured
                            // 1 -> 2: 128^3 22.9 -> 21.6, 192^3 76.9 -> 64.7, 2048^2 43.8 -> 37.9 us per fused backward step
    int zc = 8;             // planes per workgroup of the streaming kernels
    int overlap = 0;        // 1: run the gradient reduction on a side stream, chunk by chunk, under the sweep (measured: no gain on MI355X)
    int overlap_chunk = 128; // time steps per chunk
    int fuse_wgrad = 2;     // rollout sweep with the fused per-step kernel (all gradients reduced in the sweep launches)
                            // instead of sweep + one time-parallel reduction: 0 never, 1 whenever the per-step direct kernels
                            // sweep, 2 = where it measured faster: float32 poly mode on the direct-kernel path (128^3:
                            // 26.0 -> 23.3 us per step, 2048^2: 45.4 -> 39.8; fp64 and the factored mode lose)
    int skip_wgrad = 0;     // diagnostics: rollout_bwd runs the adjoint sweep only (bench uses it to time the sweep alone)
    int tile_xcd = 1;       // XCD-aware block -> tile map of the 2D tile kernels (0 = identity)
    int handover_local = 1; // 32 x 32 resident FORWARD: band granules whose readers all run on the publisher's XCD (by that map,
                            // confirmed by the hardware's XCC ids at run time) are published with plain stores and stay in the
                            // XCD's L2; 0: every granule is written through (the resident sweeps always do: measured, no gain)
    int debug_handover_local = 0;   // per call, percnn_pi_debug_plan only: N > 0 = write the bitmaps of local band granules into
                                    // an `out` of N ints instead of the plan (the entry-point count is pinned, hence no entry of its own)
    int tile_by = 0;        // tile height of the 2D tile kernels: 32, 16, or 0 = by grid size (see tile_by_for)
    int slab_fused_put_adj = 0; // ... and the adjoint sweep's faces by the sweep launch (to self: no gain; across xGMI: bench.py decides)
    int peer_upb = 2048;    // mailbox put / take launches: 16-byte units per workgroup and species (peer_prepare)
    int peer_upb_take = 0;  // ... of the take alone (0 = as the put)
    int tile_persist = 2;   // float32 poly blocks on whole 32 x 32 tiles, <= one tile per CU: the whole tile sweep
                            // of a rollout in ONE launch of resident workgroups (pi_adj2d_persist_kernel).  2 = plain launch (one
                            // workgroup fills a CU's LDS, so a grid of <= #CUs is resident as long as no OTHER kernel holds whole
                            // CUs: calls on other streams of this process are detected and take the launch-per-group path;
                            // processes that share one GPU must set 0); 1 = cooperative launch (residency guaranteed by the
                            // runtime, but ~0.4 ms per launch on ROCm 7.2: slower than what it saves at T = 1000); 0 = off
    int persist_handshake = 1;  // persistent sweep: the entry point waits (host spin on a host-mapped word, no stream sync) until
                            // the launch reports that every workgroup is resident -- or that it aborted, in which case the
                            // launch-per-group sweep is enqueued in the same call and the persistent path is switched off for
                            // this device (percnn_pi_persist_status).  0: no wait; an aborted launch is reported by the NEXT
                            // entry point (PERCNN_PI_EASYNC) instead
    int fwd_small_half = 1;     // small-tile resident forward (32 x 8 tiles) on half-strips: 512 lanes, two waves per SIMD
    int adj_small_half = 1;     // small-tile resident sweep (32 x 8 tiles) on half-strips: 512 lanes, two waves per SIMD
    // small-tile resident kernels: 64-clock units between publish and the first ring request (PersistArgs::pause); -1 = by tile count.
    // Re-swept with the half-strip / pair-granule kernels of round 6 (us per step at pause 12 | 16 | 20 | 24 | 28 | 32):
    //   forward  100^2 (52 tiles) .873 .867 .821 .819 .843 .871 | 160^2 .921 .916 .901 .886 .874 .874 | 256^2 .978 .941 .921 .865 .851 .878
    //   sweep    100^2 1.159 1.145 1.123 1.130 1.155 1.182 | 160^2 1.216 1.206 1.201 1.183 1.179 1.206 | 256^2 1.539 1.517 1.480 1.432 1.373 1.377
    int adj_small_pause = -1;   // -> 20 up to 64 tiles, 28 above
    int fwd_small_pause = -1;   // -> 24 up to 64 tiles, 28 above
    int persist_small = 1;      // the 32 x 8-tile regime (grids below ~300^2, split schedule) as one persistent launch too
    int fwd_persist_per_cu = 1; // ... on grids of up to this many tiles per CU (1 or 2)
    int fwd_persist_f64 = 1;    // ... float64 too (lambda-omega; 16-byte granules)
    int adj_persist_f64 = 1;    // the float64 tile SWEEP as one resident launch as well (split flavour, moments in shared LDS rows)
    int fwd_persist = 1;        // the FORWARD rollout of such a grid as one launch of resident workgroups too (pi_fwd2d_persist_kernel;
                            // same residency check / abort / fallback; its granule outbox is a per-device scratch of the library)
    int persist_split = 1;      // persistent sweep: 1 = split flavour (pi_adj2d_persist_split_kernel: the halo-independent
                            // "pyramid" of the next group runs while the granules of the hand-over travel), 0 = round 3's kernel
    int persist_timeout_ms = 2000;       // bound of one hand-over wait inside the persistent sweep
    int persist_first_timeout_ms = 100;  // ... of the first one (residency check)
    int tile_wide = 3;      // float32 poly blocks: 3 = 32x40 / 40x40 tiles where they keep the grid in one round (tile_wide_for),
                            // 0 = never, 1 / 2 = force 32x40 / 40x40
    int fwd_blocks = 0;     // direct forward kernel: grid cap (0 = none; measured: a bounded persistent grid loses, 384^3 376 -> 416 us)
    int xcd_window = 0;     // direct forward kernel: XCD-contiguous block remap inside windows of this many blocks (0 = whole grid)
    int block_small = 1;    // direct kernels: 64-thread workgroups while 256-thread ones would leave CUs idle (small grids)
    int rz = 0;             // direct 3D kernels, pre-contracted blocks: planes per workgroup pass sharing their plane neighbours in
                            // registers (1, 2, 4; 0 = by size, see direct_rz)
    int l2_tile_kb = 128;   // direct 3D kernels: y-tile of a plane (both species, KiB) whose five stencil planes stay in the L2
                            // (0 = whole planes, the pre-round-2 order): see set_blockmap
    int l2_tile_min_kb = 1536;  // ... applied once four neighbour planes x two species exceed this many KiB (0: always; tests)
    int peer_wire_us = 0;   // MEASUREMENT AID: every put over the peer mailboxes holds its arrival flag back this many microseconds
                            // (pi_peer.h PeerXfer::wire_ticks): a stand-in for the link time of an xGMI hop when the ring runs to self
    int slab_put_blocks = 16; // ... workgroups per direction of that fused put (a multiple of 4)
    int slab_fused_put = 1; // native slab rollouts over the peer mailboxes: the step kernel that writes a frame about to be exchanged
                            // also carries its faces into the neighbours' mailboxes (pi_peer.h "put fused into the step kernel")
    int slab_local_index = 1;   // native slab rollouts of ONE rank (ring == NULL): 1 = the periodic wrap is resolved by index inside the
                            // step launches (no face copies, no recomputed halo planes: 32 x 256^2, us per fwd+bwd step: 34.6 with one
                            // copy launch per exchange -> see profiles/r05_slab_local_wrap.txt); 0 = by face copies into the halo
                            // planes -- the launches of a multi-rank run minus its transport (what bench.py's compute / exchange
                            // split times; also selected per call by bit 1 of the `overlap` argument)
    int slab_wide_adjoint = 0;  // native slab backward over RCCL: one exchange per TWO adjoint steps (4 adjoint planes + 2 dL/dtraj
                            // planes per side in one group call), the 2-plane strips next to the faces recomputed locally.
                            // Built for VERDICT r1 #3, measured SLOWER on MI355X (RCCL to self, 32 x 256^2 slab: 74.0 -> 79.6 us
                            // per fwd+bwd step): an ncclGroup costs per operation (~3 us each of its 8 sends / receives), not per
                            // call, so 16 operations every second step save nothing and the two strip launches come on top
    int lane_x = 0;         // direct kernels: log2 of the lanes along x per row segment (2..6), 0 = fewest idle lanes (set_blockmap),
                            // -1 = the pre-round-2 rule (next power of two >= chunks per row)
    int brick3d = 1;        // 3D: brick kernels (pi_brick3d.h) for one-step launches where the shape allows: 0 never, 1 by
                            // size (brick_ok), 2 whenever eligible
    int res3d = 1;          // 3D float32 pre-contracted blocks: the whole reverse sweep of a rollout as ONE launch of resident
                            // workgroups with the adjoint state in LDS (pi_res3d.h; round 6): 0 never, 1 where it measured faster than
                            // the brick sweep (whole 16 x 16 x 32 blocks, at least 7/8 of the CUs busy: 128^3, 112 x 128^2), 2 on
                            // every grid of whole blocks that fits the device (tests)
    int brick_rz = 0;       // planes per brick (1, 2, 4; 0 = by size)
    int brick_xcd = 1;      // brick kernels: XCD regions split in y as well as in z where the counts divide (BrickGeom::xny):
                            // 0 never, 1 where it measured no worse (make_brick_geom), 2 always
    int brick_xny = 0;      // ... 0 = regions sized by the L2 (make_brick_geom), 1 = contiguous plane ranges, 2 / 4 / 8 = force that many
                            // row strips (tuning aid); -1 = the round-4 rule for forward steps of >= 8 M points (contiguous)
    int brick_wide = 1;     // 3D rows of 65 .. 128 chunks on 512-lane bricks (0: the direct kernels, as before round 4)
    int brick_nt = 0;       // lanes per brick workgroup: 512 = the wide flavour (pre-contracted blocks; see brick_nt_for), else 256
    int brick_wgs = 0;      // adjoint brick kernel: resident workgroups per CU that walk the bricks (0 = 4 / 2 by planes per brick)
    int brick_wt = 1;       // brick kernels store their output frame write-through (BrickGeom::wt)
    int lds_pad = 0;        // extra dynamic LDS per workgroup (bytes): lowers workgroups/CU so that a
                            // small grid is spread over all CUs instead of being packed onto a few
};
// one option of the table (pi_host.hip, OPTION_ROWS: a row per field) / a whole "key=value,key=value" string (whitespace-free;
// empty / NULL = no overrides); 0 or PERCNN_PI_EINVAL
int apply_option(Options& o, const char* key, long value);
int apply_overrides(Options& o, const char* spec);

// One side stream + a small event ring per host thread and device for sweep || reduction overlap (created lazily, released when
// the thread ends: applications that churn worker threads do not accumulate streams; fork/join through events only -- no host
// synchronisation).
struct SideStream {
    hipStream_t stream = nullptr;
    hipEvent_t ev[8] = {};
    hipEvent_t done = nullptr;
    int next = 0;
    bool ok = false;
    SideStream() = default;
    SideStream(const SideStream&) = delete;
    SideStream& operator=(const SideStream&) = delete;
    ~SideStream();
};
SideStream* side_stream();

constexpr int MAX_BWD_BLOCKS = 4096;   // bounds the per-workgroup gradient partials (grid-stride beyond)

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct Problem {
    int ndim, hc;
    int64_t n0, n1, W;
    int64_t n;          // points per species (interior)
    bool slab;
    int halo = 2;       // slab layout: planes present on each side of axis 0 (even, >= 2)
    int skip = 0;       // slab layout: outermost planes per side that this call neither reads nor writes
    int lo = -1, hi = -1;   // slab layout, plane-range calls: padded plane indices [lo, hi) this call computes
    bool slab_periodic = false; // slab layout of ONE rank: the n0 interior planes are a periodic domain of their own -- the wrap is
                                // resolved by index inside the step launches (plane -1 = interior plane n0 - 1), the halo planes
                                // are neither read nor written
    Options opt;            // this call's tuning options: process defaults at entry + per-call overrides
    pi::LossInj loss{0.0, nullptr, 0};   // adjoint calls: what the injection pointer means (pi_device.h); mode 0 = dL/dout itself
};

int make_problem(int hc, int ndim, const int64_t* shape, bool slab, Problem& p, const char* overrides = nullptr,
                 bool launches = true);                     // launches = false: a pure size / plan query

pi::FastDiv make_fastdiv(unsigned d);
// chunk-id decomposition of the time-parallel / residual / advective kernels without integer division (vec = points per lane)
void set_fastdiv(pi::Geom& g, int vec);
// block-uniform decomposition of the direct step kernels; false if the grid is outside what they address
bool set_blockmap(pi::Geom& g, int ndim, int vec, int block, size_t elem, int l2_tile_bytes = 128 * 1024, int rz = 1,
                  long l2_tile_min_bytes = 3L << 19, int lane_x = 0);
pi::Geom make_geom(const Problem& p);
// workgroup size of the direct kernels
int direct_block(const Problem& p, const pi::Geom& g, int vec);

// ---- residency protocol: persist_enter -> [persist_fits] -> [persist_scratch] -> persist_claim -> the launch -> persist_launched
struct Resident {
    int dev = 0, slot = 0;
    volatile int* hs = nullptr;       // host-mapped status slot {roll call complete, step, task, aborted}
    unsigned char* scratch = nullptr; // per-device scratch, zeroed on the stream: 256 B of sync words | granule outbox |
                                      // what the caller counted into outbox_bytes behind its granules (2D forward: one
                                      // placement word per tile, option handover_local)
    unsigned long long timeout_ticks = 0, first_timeout_ticks = 0;   // bounds of a hand-over wait (100 MHz ticks): options persist_*_ms
};

int device_cu_count();
bool persist_disabled_here();
void persist_reset();
int persist_async_error();
bool persist_enter(hipStream_t st, int& dev);
// workgroups of `kernel` (NT lanes, `lds` bytes) that fit a CU of device `dev`, the current one; 0: none, or the runtime
// would not say.  Asked once per (device, kernel, lds) -- after allow_lds, which the answer depends on.
int persist_fits(const void* kernel, int NT, size_t lds, int dev);
hipError_t persist_scratch(size_t outbox_bytes, hipStream_t st, Resident& r);
void persist_claim(const Options& o, Resident& r);
hipError_t persist_launched(hipStream_t st, const Resident& r, int handshake, unsigned grid, const char* what);

// what the caller of a resident launcher does with its return value
enum class ResidentRun { ran, fall_back, fall_back_clear, fatal };
ResidentRun resident_outcome(hipError_t e);

// The same steps under the process-wide options, for launchers that take no per-call options (Stage-1, the resident 3D sweep):
// hipSuccess: go ahead and launch on `stream`; anything else: take the launch-per-step path (resident launches switched off or
// aborted earlier on this device, another stream holds a resident grid, the stream is being captured, no memory)
hipError_t resident_begin(void* stream, size_t outbox_bytes, Resident& r);
// after the launch: waits for the roll call (option persist_handshake).  hipSuccess: resident and running;
// hipErrorLaunchFailure: it aborted -- recompute launch by launch (the device keeps that path until persist_reset)
hipError_t resident_launched(void* stream, Resident& r, unsigned grid, const char* what);
// PERCNN_PI_EASYNC once if a resident launch nobody waited for has aborted since the last look, else 0
int resident_async_error();
int resident_cu_count();

}  // namespace pi_host
