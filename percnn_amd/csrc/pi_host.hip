// pi_host.hip -- the host runtime of libpercnn_pi.so (declared in pi_host.h): the option table, Problem and the block
// decomposition of the direct kernels, the side stream and the host side of the residency protocol.
// This unit holds no __global__ function and no __device__ variable and instantiates no kernel: its gfx950 code object is
// empty, it compiles in seconds, and it can be built under a host sanitizer (tests/host_unit_main.hip).  Of the kernel headers
// it reads pi_device.h and pi_kernels.h (FastDiv, LossInj, Geom) only.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>
#include <tuple>

#include "../../include/percnn_pi.h"
#include "pi_device.h"
#include "pi_kernels.h"
#include "pi_host.h"

namespace pi_host {

using pi::Geom;

// The ONLY process-wide mutable state of the library besides the residency guard below: the table of tuning defaults.  Every
// entry point copies it once, under the lock, into its Problem (p.opt), overlays the call's own overrides ("key=value,..." of
// the *_opt entry points) and reads nothing else afterwards -- concurrent calls with different options do not interact.
// (Defined here, once: a copy per translation unit would give each unit its own defaults.)
Options g_defaults;
std::mutex g_defaults_mu;

// ---- the option table: one row per field of Options ------------------------------------------------------------
// PI_OPT derives the key string and the member from ONE token, so a key cannot point at a neighbour's field; the
// static_assert below ties the number of rows to the number of fields.  A rule is a captureless predicate over the value --
// accepted values are stored as given -- or nullptr for a boolean: any value, stored as value != 0.
using Rule = bool (*)(long);
struct OptionRow {
    const char* key;
    int Options::* field;
    Rule ok;
};
template <long LO, long HI, long STEP = 1>
bool in_range(long v) { return v >= LO && v <= HI && v % STEP == 0; }       // (every stepped range starts at LO >= 0)
template <long... S>
bool one_of(long v) { return ((v == S) || ...); }
bool peer_upb_take_ok(long v) { return v == 0 || in_range<256, 65536>(v); }  // 0 = as the put
constexpr Rule boolean = nullptr;

#define PI_OPT(name, rule) {#name, &Options::name, rule}
constexpr OptionRow OPTION_ROWS[] = {
    PI_OPT(block, (in_range<64, 256, 64>)),
    PI_OPT(vec, (one_of<0, 1>)),
    PI_OPT(wgrad_blocks, (in_range<1, MAX_BWD_BLOCKS / 2>)),
    PI_OPT(tile, (in_range<0, 2>)),                              // 0 = never, 1 = size heuristic, 2 = whenever eligible
    PI_OPT(tile_k, (one_of<2, 4, 8>)),                           // 8: poly mode only (else 4)
    PI_OPT(tile_nt, (one_of<256, 512, 1024>)),                   // 1024: poly mode only
    PI_OPT(stream3d, (in_range<0, 2>)),                          // 0 = never, 1 = size heuristic, 2 = whenever eligible
    PI_OPT(tile_fuse, (in_range<0, 2>)),                         // 0 split, 1 fused for float32 (default), 2 fused for float64 too
    PI_OPT(bwd_cpl, (in_range<1, 16>)),
    PI_OPT(zc, (in_range<1, 1024>)),
    PI_OPT(overlap, boolean),
    PI_OPT(overlap_chunk, (in_range<1, 1 << 20>)),
    PI_OPT(fuse_wgrad, (in_range<0, 2>)),
    PI_OPT(skip_wgrad, boolean),
    PI_OPT(tile_xcd, boolean),
    PI_OPT(handover_local, boolean),
    PI_OPT(debug_handover_local, (in_range<0, 1 << 24>)),        // (per call only: set_option refuses it)
    PI_OPT(tile_by, (one_of<0, 8, 16, 32>)),
    PI_OPT(slab_fused_put_adj, boolean),
    PI_OPT(peer_upb, (in_range<256, 65536>)),
    PI_OPT(peer_upb_take, peer_upb_take_ok),
    PI_OPT(tile_persist, (in_range<0, 2>)),
    PI_OPT(persist_handshake, boolean),
    PI_OPT(fwd_small_half, (in_range<0, 1>)),
    PI_OPT(adj_small_half, (in_range<0, 1>)),
    PI_OPT(adj_small_pause, (in_range<-1, 200>)),
    PI_OPT(fwd_small_pause, (in_range<-1, 200>)),
    PI_OPT(persist_small, (in_range<0, 2>)),
    PI_OPT(fwd_persist_per_cu, (in_range<1, 2>)),
    PI_OPT(fwd_persist_f64, boolean),
    PI_OPT(adj_persist_f64, boolean),
    PI_OPT(fwd_persist, boolean),
    PI_OPT(persist_split, boolean),
    PI_OPT(persist_timeout_ms, (in_range<1, 600000>)),
    PI_OPT(persist_first_timeout_ms, (in_range<1, 600000>)),
    PI_OPT(tile_wide, (in_range<0, 3>)),
    PI_OPT(fwd_blocks, (in_range<0, 1 << 24>)),
    PI_OPT(xcd_window, (in_range<0, 1 << 24, 8>)),
    PI_OPT(block_small, boolean),
    PI_OPT(rz, (one_of<0, 1, 2, 4>)),
    PI_OPT(l2_tile_kb, (in_range<0, 16384>)),
    PI_OPT(l2_tile_min_kb, (in_range<0, 1 << 22>)),
    PI_OPT(peer_wire_us, (in_range<0, 100000>)),
    PI_OPT(slab_put_blocks, (in_range<4, 256, 4>)),
    PI_OPT(slab_fused_put, boolean),
    PI_OPT(slab_local_index, boolean),
    PI_OPT(slab_wide_adjoint, boolean),
    PI_OPT(lane_x, (one_of<-1, 0, 2, 3, 4, 5, 6, 7>)),           // 7 = flat
    PI_OPT(brick3d, (in_range<0, 2>)),                           // 0 = never, 1 = size heuristic, 2 = whenever eligible
    PI_OPT(res3d, (in_range<0, 2>)),                             // 0 = never, 1 = where it measured faster, 2 = whenever eligible
    PI_OPT(brick_rz, (one_of<0, 1, 2, 4>)),
    PI_OPT(brick_xcd, (in_range<0, 2>)),
    PI_OPT(brick_xny, (one_of<-1, 0, 1, 2, 4, 8>)),
    PI_OPT(brick_wide, boolean),
    PI_OPT(brick_nt, (one_of<0, 256, 512>)),
    PI_OPT(brick_wgs, (in_range<0, 16>)),
    PI_OPT(brick_wt, boolean),
    PI_OPT(lds_pad, (in_range<0, 80 * 1024, 16>)),
};
#undef PI_OPT
static_assert(sizeof(Options) == sizeof(OPTION_ROWS) / sizeof(OPTION_ROWS[0]) * sizeof(int),
              "one row of OPTION_ROWS per field of Options (all of them int)");

int apply_option(Options& o, const char* key, long value)
{
    if (!key) return PERCNN_PI_EINVAL;
    if (!std::strcmp(key, "persist_reset")) { persist_reset(); return 0; }
    if (!std::strcmp(key, "graph")) return value == 0 ? 0 : PERCNN_PI_EINVAL;   // reserved
    for (const OptionRow& r : OPTION_ROWS)
        if (!std::strcmp(key, r.key)) {
            if (r.ok && !r.ok(value)) return PERCNN_PI_EINVAL;
            o.*r.field = r.ok ? (int)value : value != 0;
            return 0;
        }
    return PERCNN_PI_EINVAL;
}

// "key=value,key=value" (whitespace-free); empty / NULL = no overrides
int apply_overrides(Options& o, const char* spec)
{
    if (!spec) return 0;
    char key[32];
    while (*spec) {
        const char* eq = std::strchr(spec, '=');
        if (!eq || eq == spec || (size_t)(eq - spec) >= sizeof(key)) return PERCNN_PI_EINVAL;
        std::memcpy(key, spec, (size_t)(eq - spec));
        key[eq - spec] = 0;
        char* end = nullptr;
        const long v = std::strtol(eq + 1, &end, 10);
        if (end == eq + 1 || (*end && *end != ',')) return PERCNN_PI_EINVAL;
        if (int rc = apply_option(o, key, v)) return rc;
        spec = *end ? end + 1 : end;
    }
    return 0;
}

// ---- side stream ----------------------------------------------------------------------------------------------------
SideStream::~SideStream()
{
    // (thread-local destructors of the main thread run inside exit() before the runtime's own teardown; errors are ignored --
    // work still queued on the stream completes, hipStreamDestroy only releases the handle)
    for (auto& e : ev)
        if (e) (void)hipEventDestroy(e);
    if (done) (void)hipEventDestroy(done);
    if (stream) (void)hipStreamDestroy(stream);
    (void)hipGetLastError();
}
SideStream* side_stream()
{
    // per host THREAD and device: two threads that drive two streams of one device must not share the event ring
    static thread_local SideStream per_dev[16];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
    SideStream& s = per_dev[dev];
    if (!s.ok) {
        if (hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess) return nullptr;
        for (auto& e : s.ev)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
        if (hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess) return nullptr;
        s.ok = true;
    }
    return &s;
}

// ---- Problem and the geometry of the direct kernels ------------------------------------------------------------
int make_problem(int hc, int ndim, const int64_t* shape, bool slab, Problem& p, const char* overrides, bool launches)
{
    {
        std::lock_guard<std::mutex> lk(g_defaults_mu);
        p.opt = g_defaults;
    }
    if (int rc = apply_overrides(p.opt, overrides)) return rc;
    if (launches)
        if (int rc = persist_async_error()) return rc;      // an earlier persistent sweep aborted and nobody has been told yet
    if (!shape || (ndim != 2 && ndim != 3) || hc < -1 || hc > 64) return PERCNN_PI_EINVAL;   // hc == 0: poly, -1: advective
    if (hc == -1 && slab) return PERCNN_PI_EINVAL;
    for (int a = 0; a < ndim; ++a)
        if (shape[a] < 2 || shape[a] > (1 << 30)) return PERCNN_PI_EINVAL;
    p.ndim = ndim; p.hc = hc; p.slab = slab;
    p.n0 = shape[0];
    p.n1 = ndim == 3 ? shape[1] : 1;
    p.W = shape[ndim - 1];
    // n = n0 * n1 * W <= 2^40, asked without forming a product that may not fit (n0 * n1 <= 2^60 does; times W, 48 x 2^30 x 2^30
    // wrapped to 0 and was let through).  Exact: for integers n0 * n1 <= floor(2^40 / W) <=> n0 * n1 * W <= 2^40
    if (p.n0 * p.n1 > (int64_t(1) << 40) / p.W) return PERCNN_PI_EINVAL;
    p.n = p.n0 * p.n1 * p.W;
    return 0;
}

pi::FastDiv make_fastdiv(unsigned d)
{
    pi::FastDiv f{0u, 0u};
    if (d <= 1) return f;
    unsigned l = 0;
    while ((1ull << l) < d) ++l;                                   // l = ceil(log2 d) >= 1
    f.m = (unsigned)((((unsigned long long)1 << (31 + l)) + d - 1) / d);
    f.s = l - 1;
    return f;
}

// chunk-id decomposition of the time-parallel / residual / advective kernels without integer division (vec = points per lane)
void set_fastdiv(Geom& g, int vec)
{
    const long nchunks = (long)g.rows * (g.W / vec);
    g.fastdiv = nchunks < (1L << 31) ? 1 : 0;
    g.dcpr = make_fastdiv((unsigned)(g.W / vec));
    g.dn1 = make_fastdiv((unsigned)g.n1);
}

// block-uniform decomposition of the direct step kernels (pi_kernels.h "Direct step kernels, addressing"): lanes along x
// = the power of two that wastes the fewest lanes on this row length; false if the grid is outside what 32-bit byte
// offsets / 31-bit block ids address (2D: the whole local field + 4 rows, 3D: one plane, must stay below 4 GiB)
bool set_blockmap(Geom& g, int ndim, int vec, int block, size_t elem, int l2_tile_bytes, int rz, long l2_tile_min_bytes,
                  int lane_x)
{
    const long cpr = g.W / vec;
    // lanes along x: 2^lxs consecutive chunks of a row per wave row-segment.  A row of cpr chunks is covered by
    // ceil(cpr / 2^lxs) segments, so a width that is not a power of two leaves lanes idle (cpr = 48 on 64 lanes: 25 %; the
    // reference's 48^3: 12 chunks on 16 lanes).  Pick the power of two with the most useful lanes, weighted by what a
    // narrower contiguous segment costs (fitted to 96^3 .. 224^3 on MI355X, profiles/r02_lanes_along_x.txt: 128-byte
    // segments run at ~0.8 of 1 KiB ones, 256 / 512-byte ones at ~0.95): 160^3 13.8 k -> 17.0 k, 192^3 8.4 k -> 10.6 k steps/s.
    static const double seg_weight[5] = {0.70, 0.82, 0.95, 0.95, 1.0};     // 2^lxs = 4, 8, 16, 32, 64 chunks of 16 bytes
    int lxs = 2;
    double best_pow2 = 1.0;                               // score of the chosen power of two (forced / old rule: never flat)
    if (lane_x >= 2 && lane_x <= 6) {
        lxs = lane_x;                                     // tuning aid / A-B tests
    } else if (lane_x == -1) {                            // the pre-round-2 rule
        if (cpr <= 64) { while ((1L << lxs) < cpr) ++lxs; }
        else {
            lxs = 6;
            double best = 0.0;
            for (int c = 6; c >= 4; --c) {
                const long lx = 1L << c;
                const double eff = (double)cpr / (double)(((cpr + lx - 1) / lx) * lx);
                if (eff > best + 1e-9) { best = eff; lxs = c; }
            }
        }
    } else {
        const long rows = ndim == 3 ? g.n1 : g.n0;
        double best = 0.0;
        for (int c = 6; c >= 2; --c) {
            const long lx = 1L << c, rb = block >> c;     // rb rows of lx chunks per workgroup
            if (lx > block) continue;
            double eff = (double)cpr / (double)(((cpr + lx - 1) / lx) * lx) *
                         (double)rows / (double)(((rows + rb - 1) / rb) * rb);
            eff *= seg_weight[c - 2];
            // a row pitch that is not a multiple of 128 bytes leaves the segments straddling cache lines: S bytes touch
            // (S + 128) / 128 lines on average instead of S / 128 (200^3 with 128-byte segments: forward 39 -> 66 us)
            const long seg = lx * 16;
            if (((long)g.W * (long)elem) % 128 != 0) eff *= (double)seg / (double)(seg + 128);
            if (eff > best + 1e-9) { best = eff; lxs = c; }
        }
        best_pow2 = best;
    }
    while ((1 << lxs) > block) --lxs;
    const long nrow = ndim == 3 ? g.n1 : g.n0;
    // ... or none of them: consecutive chunks of the plane across row ends (`flat`; one multiply-shift per lane, rows follow
    // each other in memory so a wave still moves 1 KiB pieces) -- taken where the best power of two leaves > ~10 % idle
    bool flat = lane_x == 7;
    if (lane_x == 0 && nrow * cpr < (1L << 31)) {
        const long total = nrow * cpr, nb = (total + block - 1) / block;
        double eff = 0.97 * (double)total / (double)(nb * block);
        if (((long)g.W * (long)elem) % 128 != 0) eff *= 1024.0 / (1024.0 + 128.0);
        // (not with four planes per pass: 208^3 forward 41 -> 51 us, 240^3 65 -> 69 us when forced, while the two-plane
        // adjoint of the same grids gains 7 %)
        // and only below 8 M points, where the kernels are latency-bound and idle lanes are what costs: beyond that the
        // outcome follows the DRAM access pattern instead (same-box A/B: 288^3 +10 %, 224^3 -3 %, 352^3 -5 %)
        const long npts = (long)g.n0 * g.n1 * g.W;
        flat = eff > best_pow2 + 0.08 && rz <= 2 && npts < (8L << 20);
    }
    if (flat && nrow * cpr >= (1L << 31)) return false;
    const long lx = flat ? block : 1L << lxs, rpb = flat ? 1 : block >> lxs;
    g.lxs = flat ? -1 : lxs;
    g.nxb = flat ? 1 : (int)((cpr + lx - 1) / lx);
    g.nrg = flat ? (int)((nrow * cpr + block - 1) / block) : (int)((nrow + rpb - 1) / rpb);
    if (flat) g.dcpr = make_fastdiv((unsigned)cpr);
    g.rz = ndim == 3 ? rz : 1;
    const long ngroups = ndim == 3 ? (g.n0 + g.rz - 1) / g.rz : 1;          // plane groups of rz planes
    const long nblk = (long)g.nxb * g.nrg * ngroups;
    const unsigned long long span = (unsigned long long)(ndim == 3 ? (long)g.n1 : (long)g.n0 + 4) * g.W * elem;
    if (nblk <= 0 || nblk >= (1L << 31) || span >= (1ull << 32)) return false;
    g.nblk = (unsigned)nblk;
    g.dnxb = make_fastdiv((unsigned)g.nxb);
    g.dnrg = make_fastdiv((unsigned)g.nrg);
    // 3D y-tiling for L2 residency (Geom::rgt): a tile's plane section, both species, is held to ~128 KiB so that the four
    // neighbour planes of everything in flight on an XCD (~2 MiB) fit its 4 MiB L2 next to the streams themselves
    g.rgt = 0; g.nlast = 0; g.per_tile = 0;
    // (only where whole planes do not fit anyway: four neighbour planes x two species above ~1.5 MiB; measured on
    // MI355X: 384^3 backward 726 -> 513 us, 256^3 171 -> 148 us per step, 192^3 -- 1.2 MB of neighbour planes -- loses 3-8 %)
    if (ndim == 3 && l2_tile_bytes > 0 && 8L * g.n1 * g.W * (long)elem > l2_tile_min_bytes) {
        const long tile_rows = (long)l2_tile_bytes / (2 * (long)g.W * (long)elem);
        long rgt = flat ? (long)l2_tile_bytes / (2 * (long)block * vec * (long)elem) : tile_rows / rpb;
        if (rgt < 1) rgt = 1;
        if (rgt < g.nrg && (long)rgt * ngroups < (1L << 31)) {
            const long ntile = (g.nrg + rgt - 1) / rgt;
            g.rgt = (int)rgt;
            g.nlast = (int)(g.nrg - (ntile - 1) * rgt);
            g.per_tile = (unsigned)(rgt * ngroups);
            g.dper = make_fastdiv(g.per_tile);
            g.drgt = make_fastdiv((unsigned)g.rgt);
            g.dlast = make_fastdiv((unsigned)g.nlast);
        }
    }
    return true;
}

Geom make_geom(const Problem& p)
{
    Geom g;
    g.fastdiv = 0; g.dcpr = pi::FastDiv{0u, 0u}; g.dn1 = pi::FastDiv{0u, 0u};
    g.lxs = 0; g.nxb = g.nrg = 0; g.nblk = 0; g.dnxb = pi::FastDiv{0u, 0u}; g.dnrg = pi::FastDiv{0u, 0u};
    g.rgt = g.nlast = 0; g.per_tile = 0; g.dper = g.drgt = g.dlast = pi::FastDiv{0u, 0u};
    g.xwin = 0; g.rz = 1;
    g.loss = p.loss;
    g.n0 = (int)p.n0; g.n1 = (int)p.n1; g.W = (int)p.W;
    g.rows = (int)(p.n0 * p.n1);
    g.s0 = (long)(p.n1 * p.W);
    if (p.slab && p.slab_periodic) {
        g.ss = (long)(p.n0 + 2 * p.halo) * g.s0;
        g.off = (long)p.halo * g.s0;
        g.wrap0 = 1;
    } else if (p.slab) {
        // local array: n0 + 2*halo planes; this call computes planes [skip+2, n0+2*halo-skip-2)
        g.ss = (long)(p.n0 + 2 * p.halo) * g.s0;
        if (p.lo >= 0) {                                   // explicit plane range (communication overlap: faces first)
            g.off = (long)p.lo * g.s0;
            g.n0 = p.hi - p.lo;
        } else {
            g.off = (long)(p.skip + 2) * g.s0;
            g.n0 = (int)(p.n0 + 2 * p.halo - 2 * p.skip - 4);
        }
        g.rows = g.n0 * (int)p.n1;
        g.wrap0 = 0;
    } else {
        g.ss = (long)p.n0 * g.s0; g.off = 0; g.wrap0 = 1;
    }
    return g;
}

// workgroup size of the direct kernels: the "block" option, or 128 threads while 256-thread workgroups would leave
// CUs idle (a 48^3 grid is 108 workgroups of 256 threads on 256 CUs)
int direct_block(const Problem& p, const Geom& g, int vec)
{
    const long chunks = (long)g.rows * (g.W / vec);
    if (p.opt.block_small && p.opt.block == 256 && chunks < 1024L * 256) return 128;   // measured 48^3 .. 96^3: +0-10 %
    return p.opt.block;
}

// ---- residency protocol ---------------------------------------------------------------------------------------------
int device_cu_count()
{
    static int cu_count[16] = {};                           // per device, asked once (benign race: same value)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 0;
    if (!cu_count[dev]) {
        int n = 0;
        cu_count[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : -1;
    }
    return cu_count[dev] > 0 ? cu_count[dev] : 0;
}

// Two persistent sweeps in flight on ONE device would each hold part of the CUs and wait for workgroups that cannot become
// resident.  Within a process: the last persistent launch per device leaves an event behind; a call on ANOTHER stream while that
// event is not ready takes the launch-per-group path (same stream: ordered behind it anyway).
// Anything ELSE that keeps workgroups from becoming resident -- another process on the GPU, a CU mask (HSA_CU_MASK, a CU-masked
// stream), a long kernel on another stream -- is caught by the launch itself: its workgroups give up within a bound, write
// nothing, and say so in a host-mapped status slot (pi_tile2d.h, PersistArgs::host).  With the handshake (default) the entry
// point waits for that word -- "all resident" normally arrives a few microseconds after the kernel starts -- and enqueues the
// launch-per-group sweep itself on an abort; the device then keeps the launch-per-group path until persist_reset.
// The host side of that protocol is the functions below, once for every resident launcher (2D tile sweeps and forwards, the
// 3D adjoint sweep, the Stage-1 unit): persist_enter -> [persist_fits] -> [persist_scratch] ->
// persist_claim -> the launch -> persist_launched.
constexpr int PERSIST_SLOTS = 32;
struct PersistHost {                                      // host-mapped (hipHostMalloc): written by the device, read here
    volatile int slot[PERSIST_SLOTS][4];                  // {roll call complete, group, tile, aborted}: see PersistArgs::host
};
struct PersistGuard {
    std::mutex mu;
    hipEvent_t ev[16] = {};
    hipStream_t st[16] = {};
    bool armed[16] = {};
    bool disabled[16] = {};                               // a launch aborted on this device: launch-per-group until persist_reset
    PersistHost* host = nullptr;
    bool host_tried = false;
    bool watch[PERSIST_SLOTS] = {};                       // slots of launches nobody has looked at since (no-handshake mode)
    int next_slot = 0;
    long launches = 0, aborts = 0;
    int last_group = -1, last_tile = -1;
    bool warned = false;
    void* fwd_scratch[16] = {};                           // per device: sync words + granule outbox (persist_scratch)
    size_t fwd_scratch_bytes[16] = {};
    std::map<std::tuple<int, const void*, size_t>, int> fits;   // (device, kernel, LDS bytes) -> workgroups per CU (persist_fits)
};
// (defined here, once, for every unit of the library: two guards would each admit a resident grid of their own)
PersistGuard g_persist;

bool persist_disabled_here()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return true;
    std::lock_guard<std::mutex> lk(g_persist.mu);
    return g_persist.disabled[dev];
}

void persist_reset()
{
    std::lock_guard<std::mutex> lk(g_persist.mu);
    for (bool& d : g_persist.disabled) d = false;
    for (bool& w : g_persist.watch) w = false;
    g_persist.warned = false;
}

// the launches of no-handshake callers: has one of them aborted since anybody looked?  (reads of cached host memory)
int persist_async_error()
{
    if (!g_persist.host) return 0;
    std::lock_guard<std::mutex> lk(g_persist.mu);
    int rc = 0;
    for (int i = 0; i < PERSIST_SLOTS; ++i)
        if (g_persist.watch[i] && g_persist.host->slot[i][3] != 0) {
            g_persist.watch[i] = false;
            g_persist.last_group = g_persist.host->slot[i][1];
            g_persist.last_tile = g_persist.host->slot[i][2];
            ++g_persist.aborts;
            for (bool& d : g_persist.disabled) d = true;
            rc = PERCNN_PI_EASYNC;
        }
    return rc;
}

bool persist_enter(hipStream_t st, int& dev)
{
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return false;
    std::lock_guard<std::mutex> lk(g_persist.mu);
    if (g_persist.disabled[dev]) return false;
    if (g_persist.armed[dev] && g_persist.st[dev] != st && hipEventQuery(g_persist.ev[dev]) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (!g_persist.host_tried) {
        g_persist.host_tried = true;
        void* hp = nullptr;
        if (hipHostMalloc(&hp, sizeof(PersistHost), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess && hp) {
            std::memset(hp, 0, sizeof(PersistHost));
            g_persist.host = static_cast<PersistHost*>(hp);
        } else (void)hipGetLastError();
    }
    return g_persist.host != nullptr;                      // no status word, no persistent launch
}
void persist_leave(hipStream_t st, int dev)
{
    std::lock_guard<std::mutex> lk(g_persist.mu);
    if (!g_persist.ev[dev] && hipEventCreateWithFlags(&g_persist.ev[dev], hipEventDisableTiming) != hipSuccess) return;
    if (hipEventRecord(g_persist.ev[dev], st) == hipSuccess) { g_persist.st[dev] = st; g_persist.armed[dev] = true; }
}

// workgroups of kernel `k` (NT lanes, `lds` bytes) that fit a CU of device `dev`, the current one; 0: none, or the runtime
// would not say.  Asked once per (device, kernel, lds) -- after allow_lds, which the answer depends on.
int persist_fits(const void* k, int NT, size_t lds, int dev)
{
    std::lock_guard<std::mutex> lk(g_persist.mu);
    auto [it, fresh] = g_persist.fits.try_emplace({dev, k, lds}, 0);
    if (fresh) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, NT, lds) != hipSuccess || nb < 1) { (void)hipGetLastError(); nb = 0; }
        it->second = nb;
    }
    return it->second;
}

// the per-device scratch of the launchers that bring no workspace: 256 B of sync words | outbox of `outbox_bytes` (the caller
// counts what it keeps behind its granules -- the resident forward's placement words, persist_xcc_bytes -- into them), allocated
// once (sized for this launch or larger) and zeroed on the stream
hipError_t persist_scratch(size_t outbox_bytes, hipStream_t st, Resident& r)
{
    const size_t need = 256 + outbox_bytes;
    {
        std::lock_guard<std::mutex> lk(g_persist.mu);
        if (g_persist.fwd_scratch_bytes[r.dev] < need) {
            if (g_persist.fwd_scratch[r.dev]) {             // (a launch that still uses the old one is ordered before this call's
                (void)hipFree(g_persist.fwd_scratch[r.dev]);// work only on its own stream: hipFree synchronises the device)
                g_persist.fwd_scratch[r.dev] = nullptr;
                g_persist.fwd_scratch_bytes[r.dev] = 0;
            }
            void* q = nullptr;
            if (hipMalloc(&q, need) != hipSuccess || !q) { (void)hipGetLastError(); return hipErrorOutOfMemory; }
            g_persist.fwd_scratch[r.dev] = q;
            g_persist.fwd_scratch_bytes[r.dev] = need;
        }
        r.scratch = static_cast<unsigned char*>(g_persist.fwd_scratch[r.dev]);
    }
    return hipMemsetAsync(r.scratch, 0, need, st);
}

// a status slot for the launch about to be made (r.dev: from persist_enter), reset, and the bounds of its hand-over waits
void persist_claim(const Options& o, Resident& r)
{
    {
        std::lock_guard<std::mutex> lk(g_persist.mu);
        r.slot = g_persist.next_slot++ % PERSIST_SLOTS;
        g_persist.watch[r.slot] = false;
    }
    r.hs = g_persist.host->slot[r.slot];
    r.hs[0] = 0; r.hs[1] = -1; r.hs[2] = -1; r.hs[3] = 0;
    r.timeout_ticks = (unsigned long long)o.persist_timeout_ms * 100000ull;                 // 100 MHz clock
    r.first_timeout_ticks = (unsigned long long)o.persist_first_timeout_ms * 100000ull;
}

// wait for the roll call of a resident launch (not for the launch itself): normally a few microseconds after the kernel
// starts, i.e. this returns when the stream has reached it.  The bound only guards against a device that never runs the
// launch at all.  An abort is dealt with here -- the caller recomputes launch by launch.
hipError_t persist_wait_roll_call(volatile int* hs, int slot, int dev, unsigned grid, const char* what)
{
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (hs[0] == 0 && hs[3] == 0) {
        if ((++spins & 0x3ff) == 0) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(600)) return hipErrorLaunchTimeOut;
            std::this_thread::yield();
        }
    }
    if (hs[3] != 0) {
        std::lock_guard<std::mutex> lk(g_persist.mu);
        g_persist.watch[slot] = false;
        ++g_persist.aborts;
        g_persist.last_group = hs[1];
        g_persist.last_tile = hs[2];
        g_persist.disabled[dev] = true;
        if (!g_persist.warned) {
            g_persist.warned = true;
            std::fprintf(stderr, "percnn_pi: %s could not keep all %u workgroups resident on device %d (group %d, tile %d: another "
                                 "process / kernel holds CUs, or a CU mask is set); using one launch per group of steps from now on "
                                 "(percnn_pi_set_option(\"persist_reset\", 1) re-arms it)\n", what, grid, dev, (int)hs[1], (int)hs[2]);
        }
        return hipErrorLaunchFailure;
    }
    return hipSuccess;
}

// after a launch that was enqueued without error.  hipSuccess: resident and running (handshake), or fire and forget (an abort
// nobody has dealt with surfaces at the next entry point: PERCNN_PI_EASYNC); hipErrorLaunchFailure: it ran and ABORTED;
// hipErrorLaunchTimeOut: fatal.  In the first two cases the launch is on the stream: persist_leave records it for persist_enter.
hipError_t persist_launched(hipStream_t st, const Resident& r, int handshake, unsigned grid, const char* what)
{
    {
        std::lock_guard<std::mutex> lk(g_persist.mu);
        g_persist.watch[r.slot] = true;
        ++g_persist.launches;
    }
    const hipError_t e = handshake ? persist_wait_roll_call(r.hs, r.slot, r.dev, grid, what) : hipSuccess;
    if (e == hipSuccess || e == hipErrorLaunchFailure) persist_leave(st, r.dev);
    return e;
}

// what the caller of a resident launcher does with its return value
ResidentRun resident_outcome(hipError_t e)
{
    if (e == hipSuccess) return ResidentRun::ran;
    if (e == hipErrorLaunchTimeOut) return ResidentRun::fatal;       // the device never ran the launch: the stream is stuck behind it
    (void)hipGetLastError();                                      // not resident / not supported / aborted: launch by launch
    // it RAN and gave up: workgroups that were already through may have added to their partial rows -- start the rows over
    return e == hipErrorLaunchFailure ? ResidentRun::fall_back_clear : ResidentRun::fall_back;
}

// ---- resident launches under the process-wide options (the Stage-1 unit, the resident 3D sweep) ------------------------------
// They share the residency guard of the 2D resident kernels: one resident grid per device at a time (calls on other streams
// are detected and refused), host-mapped status slots, a per-device scratch (sync words + granule outbox), the handshake on the
// roll call and the "disabled after an abort" state (percnn_pi_persist_status / persist_reset report and re-arm both).
// No step of the protocol is written here: these are the functions at PersistGuard, under the process-wide options (the 2D
// launchers take a call's own).
int resident_async_error() { return persist_async_error(); }
int resident_cu_count() { return device_cu_count(); }
// hipSuccess: launch; anything else: take the launch-per-step path (nothing has been enqueued but the memset)
hipError_t resident_begin(void* stream, size_t outbox_bytes, Resident& r)
{
    auto st = static_cast<hipStream_t>(stream);
    Options o;
    { std::lock_guard<std::mutex> lk(g_defaults_mu); o = g_defaults; }
    if (!o.tile_persist || !o.fwd_persist) return hipErrorNotSupported;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return hipErrorNotSupported; }
    if (!persist_enter(st, r.dev)) return hipErrorNotSupported;
    if (hipError_t e = persist_scratch(outbox_bytes, st, r)) return e;
    persist_claim(o, r);
    return hipSuccess;
}
// after the launch: hipSuccess = resident and running; hipErrorLaunchFailure = it aborted (the caller recomputes launch by launch)
hipError_t resident_launched(void* stream, Resident& r, unsigned grid, const char* what)
{
    int handshake;
    { std::lock_guard<std::mutex> lk(g_defaults_mu); handshake = g_defaults.persist_handshake; }
    return persist_launched(static_cast<hipStream_t>(stream), r, handshake, grid, what);
}

}  // namespace pi_host

// ---- exported symbols ---------------------------------------------------------------------------
using namespace pi_host;

extern "C" {

int percnn_pi_set_option(const char* key, long value)
{
    if (key && !std::strcmp(key, "debug_handover_local")) return PERCNN_PI_EINVAL;       // a query of one call, never a default
    std::lock_guard<std::mutex> lk(g_defaults_mu);
    return apply_option(g_defaults, key, value);
}

// host-mapped words the device can write and the host can read without synchronising (pack guard slots)
int percnn_pi_host_words_alloc(void** p, size_t bytes)
{
    if (!p || bytes == 0) return PERCNN_PI_EINVAL;
    void* hp = nullptr;
    if (hipError_t e = hipHostMalloc(&hp, bytes, hipHostMallocMapped | hipHostMallocCoherent)) return (int)e;
    std::memset(hp, 0, bytes);
    *p = hp;
    return 0;
}
int percnn_pi_host_words_free(void* p) { return p ? (int)hipHostFree(p) : 0; }

int percnn_pi_persist_status(long* info)
{
    if (!info) return PERCNN_PI_EINVAL;
    int dev = 0;
    const bool have_dev = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 16;
    if (!have_dev) (void)hipGetLastError();
    std::lock_guard<std::mutex> lk(g_persist.mu);
    info[0] = g_persist.launches;
    info[1] = g_persist.aborts;
    info[2] = have_dev && g_persist.disabled[dev] ? 1 : 0;
    info[3] = g_persist.last_group;
    info[4] = g_persist.last_tile;
    // state word of the most recent launch as the device left it: 0 not started, 1 every workgroup resident, 2 aborted
    if (g_persist.host && g_persist.next_slot > 0) {
        volatile int* hs = g_persist.host->slot[(g_persist.next_slot - 1) % PERSIST_SLOTS];
        info[5] = hs[3] ? 2 : hs[0];
    } else info[5] = -1;
    return 0;
}

// Fence for callers that run the resident launches fire-and-forget (persist_handshake = 0) and hand their outputs to code
// that is not this library: waits for `stream`, then reports -- once -- whether a resident launch aborted since anybody looked
int percnn_pi_persist_fence(void* stream)
{
    if (hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(stream))) return (int)e;
    return persist_async_error();
}

}  // extern "C"
