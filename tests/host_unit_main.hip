// host_unit_main.hip -- stand-alone driver of the library's host runtime (percnn_amd/csrc/pi_host.hip), built together with it
// under the host's address and undefined-behaviour sanitizers by tests/test_host_unit_cpu.py and run without a GPU: it calls no
// HIP API.  Three parts: the option-string parser on malformed and over-long strings; every option key with accepted values,
// checked by the field the value lands in; make_problem -> make_geom -> set_blockmap over a fixed grid of arguments, with the
// invariants of the block decomposition checked.  Exit status 0 and a last line "host unit ok: ..." when everything held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../include/percnn_pi.h"
#include "../percnn_amd/csrc/pi_kernels.h"
#include "../percnn_amd/csrc/pi_host.h"

using namespace pi_host;

static int failures = 0;
#define EXPECT(cond, ...)                                                                          \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            ++failures;                                                                            \
            std::fprintf(stderr, "host_unit_main.hip:%d: %s: ", __LINE__, #cond);                  \
            std::fprintf(stderr, __VA_ARGS__);                                                     \
            std::fprintf(stderr, "\n");                                                            \
        }                                                                                          \
    } while (0)

constexpr size_t NFIELDS = sizeof(Options) / sizeof(int);

static bool same(const Options& a, const Options& b) { return !std::memcmp(&a, &b, sizeof(Options)); }

// ---- 1. the parser ----------------------------------------------------------------------------------------------------
static void parser()
{
    const std::string a31(31, 'a'), a32(32, 'a'), a4096(4096, 'a'), pad32 = "tile_k" + std::string(26, 'x');
    const std::string bad[] = {"nonsense=1", "tile_k=3", "tile_k", "=4", "tile_k=4;tile=0", "tile_k=x", "tile_k=", "tile_k=,tile=0",
                               "tile_k=4,,tile=0", ",tile_k=4", ",", "tile_k=4 ", "tile_k=4x", "tile_k=0x4", " tile_k=4",
                               "tile_k =4", "TILE_K=4", "tile_k=4,nonsense=1", "tile_k=4,tile", "tile_k=99999999999999999999",
                               a31 + "=1", a32 + "=1", a32 + "a=1", a4096 + "=1", pad32 + "=4", a4096, "tile_k=2," + a4096 + "=1",
                               "a=1,,b=2", "graph=1"};
    for (const std::string& s : bad) {
        // (an exactly-sized heap copy: a read past the string's end is the sanitizer's to report)
        std::vector<char> spec(s.begin(), s.end());
        spec.push_back(0);
        Options o;
        EXPECT(apply_overrides(o, spec.data()) == PERCNN_PI_EINVAL, "\"%.40s\" was accepted", s.c_str());
    }
    const std::string ok[] = {"", "tile_k=4", "tile_k=4,skip_wgrad=1", "tile_k=4,", "tile_k= 4", "tile_k=+4", "tile_k=04",
                              "adj_small_pause=-1", "tile_k=2,tile_k=4", "graph=0", "persist_reset=1",
                              "persist_first_timeout_ms=600000"};
    for (const std::string& s : ok) {
        std::vector<char> spec(s.begin(), s.end());
        spec.push_back(0);
        Options o;
        EXPECT(apply_overrides(o, spec.data()) == 0, "\"%s\" was refused", s.c_str());
    }
    Options o, d;
    EXPECT(apply_overrides(o, nullptr) == 0 && same(o, d), "NULL string");
    EXPECT(apply_option(o, nullptr, 1) == PERCNN_PI_EINVAL && same(o, d), "NULL key");
    EXPECT(apply_overrides(o, "tile_k=2,zc=16,overlap=5") == 0 && o.tile_k == 2 && o.zc == 16 && o.overlap == 1, "three keys");
    // what precedes a refused key of the string has been applied to the CALL's copy -- which the entry point then drops
    Options q;
    EXPECT(apply_overrides(q, "tile=0,tile_k=3") == PERCNN_PI_EINVAL && q.tile == 0 && q.tile_k == d.tile_k, "refused in the middle");
}

// ---- 2. every key, by the field it lands in ------------------------------------------------------------------------------
struct KeyCase {
    const char* key;
    int Options::* field;
    bool boolean;
    std::vector<long> accepted, refused;
};
#define K(name, boolean, ...) {#name, &Options::name, boolean, __VA_ARGS__}
static const long M24 = 1L << 24, M22 = 1L << 22, M20 = 1L << 20, BIG = 1L << 40;
static const std::vector<long> ANY = {0, 1, 2, -1, -BIG, BIG};
static const KeyCase CASES[] = {
    K(block, false, {64, 128, 192, 256}, {63, 65, 0, 257, 320}),
    K(vec, false, {0, 1}, {-1, 2}),
    K(wgrad_blocks, false, {1, 1024, 2048}, {0, 2049}),
    K(tile, false, {0, 1, 2}, {-1, 3}),
    K(tile_k, false, {2, 4, 8}, {1, 3, 6, 9}),
    K(tile_nt, false, {256, 512, 1024}, {255, 257, 768, 2048}),
    K(stream3d, false, {0, 1, 2}, {-1, 3}),
    K(tile_fuse, false, {0, 1, 2}, {-1, 3}),
    K(bwd_cpl, false, {1, 16}, {0, 17}),
    K(zc, false, {1, 1024}, {0, 1025}),
    K(overlap, true, ANY, {}),
    K(overlap_chunk, false, {1, M20}, {0, M20 + 1}),
    K(fuse_wgrad, false, {0, 1, 2}, {-1, 3}),
    K(skip_wgrad, true, ANY, {}),
    K(tile_xcd, true, ANY, {}),
    K(handover_local, true, ANY, {}),
    K(debug_handover_local, false, {0, 1, 96, M24}, {-1, M24 + 1}),
    K(tile_by, false, {0, 8, 16, 32}, {-1, 7, 24, 33}),
    K(slab_fused_put_adj, true, ANY, {}),
    K(peer_upb, false, {256, 65536}, {255, 0, 65537}),
    K(peer_upb_take, false, {0, 256, 65536}, {-1, 1, 255, 65537}),
    K(tile_persist, false, {0, 1, 2}, {-1, 3}),
    K(persist_handshake, true, ANY, {}),
    K(fwd_small_half, false, {0, 1}, {-1, 2}),
    K(adj_small_half, false, {0, 1}, {-1, 2}),
    K(adj_small_pause, false, {-1, 0, 200}, {-2, 201}),
    K(fwd_small_pause, false, {-1, 0, 200}, {-2, 201}),
    K(persist_small, false, {0, 1, 2}, {-1, 3}),
    K(fwd_persist_per_cu, false, {1, 2}, {0, 3}),
    K(fwd_persist_f64, true, ANY, {}),
    K(adj_persist_f64, true, ANY, {}),
    K(fwd_persist, true, ANY, {}),
    K(persist_split, true, ANY, {}),
    K(persist_timeout_ms, false, {1, 600000}, {0, 600001}),
    K(persist_first_timeout_ms, false, {1, 600000}, {0, 600001}),
    K(tile_wide, false, {0, 1, 2, 3}, {-1, 4}),
    K(fwd_blocks, false, {0, M24}, {-1, M24 + 1}),
    K(xcd_window, false, {0, 8, M24}, {-8, 4, M24 + 8}),
    K(block_small, true, ANY, {}),
    K(rz, false, {0, 1, 2, 4}, {-1, 3, 8}),
    K(l2_tile_kb, false, {0, 16384}, {-1, 16385}),
    K(l2_tile_min_kb, false, {0, M22}, {-1, M22 + 1}),
    K(peer_wire_us, false, {0, 100000}, {-1, 100001}),
    K(slab_put_blocks, false, {4, 8, 256}, {0, 6, 260}),
    K(slab_fused_put, true, ANY, {}),
    K(slab_local_index, true, ANY, {}),
    K(slab_wide_adjoint, true, ANY, {}),
    K(lane_x, false, {-1, 0, 2, 3, 4, 5, 6, 7}, {-2, 1, 8}),
    K(brick3d, false, {0, 1, 2}, {-1, 3}),
    K(res3d, false, {0, 1, 2}, {-1, 3}),
    K(brick_rz, false, {0, 1, 2, 4}, {-1, 3, 8}),
    K(brick_xcd, false, {0, 1, 2}, {-1, 3}),
    K(brick_xny, false, {-1, 0, 1, 2, 4, 8}, {-2, 3, 5, 6, 7, 9}),
    K(brick_wide, true, ANY, {}),
    K(brick_nt, false, {0, 256, 512}, {-1, 128, 1024}),
    K(brick_wgs, false, {0, 16}, {-1, 17}),
    K(brick_wt, true, ANY, {}),
    K(lds_pad, false, {0, 16, 80 * 1024}, {-16, 8, 80 * 1024 + 16}),
};
#undef K
static_assert(sizeof(CASES) / sizeof(CASES[0]) == NFIELDS, "one case per field of Options");

static void keys()
{
    const Options d;
    bool seen[NFIELDS] = {};
    for (const KeyCase& c : CASES) {
        const size_t at = (size_t)(reinterpret_cast<const char*>(&(d.*c.field)) - reinterpret_cast<const char*>(&d)) / sizeof(int);
        EXPECT(at < NFIELDS && !seen[at], "%s: field taken twice", c.key);
        seen[at] = true;
        for (long v : c.accepted) {
            Options o;
            EXPECT(apply_option(o, c.key, v) == 0, "%s=%ld refused", c.key, v);
            const int want = c.boolean ? (v != 0) : (int)v;
            EXPECT(o.*c.field == want, "%s=%ld stored %d", c.key, v, o.*c.field);
            o.*c.field = d.*c.field;
            EXPECT(same(o, d), "%s=%ld wrote another field", c.key, v);
        }
        for (long v : c.refused) {
            Options o;
            EXPECT(apply_option(o, c.key, v) == PERCNN_PI_EINVAL && same(o, d), "%s=%ld accepted", c.key, v);
        }
    }
}

// ---- 3. Problem -> Geom -> block decomposition ---------------------------------------------------------------------------
static unsigned fastdiv(const pi::FastDiv& f, unsigned x) { return f.m ? (unsigned)(((unsigned long long)x * f.m) >> 32) >> f.s : x; }
static void check_div(const pi::FastDiv& f, unsigned d, const char* what)
{
    if (d == 0) return;
    for (unsigned x : {0u, 1u, d - 1, d, d + 1, 2 * d - 1, 2 * d, 12345677u, (1u << 30) + 1, (1u << 31) - 1})
        if (x < (1u << 31)) EXPECT(fastdiv(f, x) == x / d, "%s: %u / %u", what, x, d);
}

static long geometry()
{
    const int64_t extents[] = {2, 3, 48, 100, 512, 70000, int64_t(1) << 30};
    long admitted = 0, maps = 0;
    unsigned long long sum = 0;
    std::vector<std::vector<int64_t>> shapes;
    for (int64_t a : extents)
        for (int64_t b : extents) {
            shapes.push_back({a, b});
            for (int64_t c : extents) shapes.push_back({a, b, c});
        }
    shapes.push_back({1, 8}); shapes.push_back({8, (int64_t(1) << 30) + 1}); shapes.push_back({8, 8, 0});      // refused
    for (const auto& sh : shapes) {
        const int ndim = (int)sh.size();
        Problem p;
        const int rc = make_problem(0, ndim, sh.data(), false, p, nullptr, false);
        bool admit = true;
        double n = 1;
        for (int64_t e : sh) { admit = admit && e >= 2 && e <= (int64_t(1) << 30); n *= (double)e; }
        admit = admit && n <= 1099511627776.0;
        EXPECT((rc == 0) == admit, "make_problem of %d extents from %ld: %d", ndim, (long)sh[0], rc);
        if (rc) continue;
        ++admitted;
        for (size_t elem : {(size_t)4, (size_t)8}) {
            const int widest = 16 / (int)elem;
            for (int vec : {1, widest}) {
                if (p.W % vec) continue;
                for (int block = 64; block <= 256; block += 64)
                    for (int lane_x = -1; lane_x <= 7; ++lane_x) {
                        if (lane_x == 1) continue;                       // no value of the option
                        for (int rz : {1, 2, 4}) {
                            pi::Geom g = make_geom(p);
                            set_fastdiv(g, vec);
                            const pi::FastDiv dcpr0 = g.dcpr;
                            const bool ok = set_blockmap(g, ndim, vec, block, elem, p.opt.l2_tile_kb * 1024, rz,
                                                         (long)p.opt.l2_tile_min_kb * 1024, lane_x);
                            ++maps;
                            if (!ok) continue;
                            const long cpr = g.W / vec, nrow = ndim == 3 ? g.n1 : g.n0;
                            const long groups = ndim == 3 ? (g.n0 + g.rz - 1) / g.rz : 1;
                            EXPECT(g.nblk > 0 && g.nblk < (1u << 31) && (long)g.nblk == (long)g.nxb * g.nrg * groups, "nblk");
                            if (g.lxs < 0) {                             // flat: consecutive chunks of the plane
                                EXPECT(g.nxb == 1 && (long)g.nrg * block >= nrow * cpr && (long)(g.nrg - 1) * block < nrow * cpr, "flat cover");
                                check_div(g.dcpr, (unsigned)cpr, "dcpr (flat)");
                            } else {
                                const long lx = 1L << g.lxs, rpb = block >> g.lxs;
                                EXPECT(lx <= block && rpb >= 1, "lanes along x");
                                EXPECT((long)g.nxb * lx >= cpr && (long)(g.nxb - 1) * lx < cpr, "x cover");
                                EXPECT((long)g.nrg * rpb >= nrow && (long)(g.nrg - 1) * rpb < nrow, "row cover");
                                EXPECT(g.dcpr.m == dcpr0.m && g.dcpr.s == dcpr0.s, "dcpr kept");
                            }
                            check_div(g.dnxb, (unsigned)g.nxb, "dnxb");
                            check_div(g.dnrg, (unsigned)g.nrg, "dnrg");
                            if (g.rgt) {
                                const long ntile = (g.nrg + g.rgt - 1) / g.rgt;
                                EXPECT(ndim == 3 && g.rgt < g.nrg && g.nlast >= 1 && g.nlast <= g.rgt &&
                                       (ntile - 1) * g.rgt + g.nlast == g.nrg && (long)g.per_tile == g.rgt * groups, "y tiles");
                                check_div(g.dper, g.per_tile, "dper");
                                check_div(g.drgt, (unsigned)g.rgt, "drgt");
                                check_div(g.dlast, (unsigned)g.nlast, "dlast");
                            }
                            sum = sum * 1000003ull + (unsigned long long)(g.lxs + 2) + 7ull * g.nxb + 31ull * g.nrg + 127ull * g.nblk +
                                  8191ull * g.rgt + (unsigned long long)direct_block(p, g, vec);
                        }
                    }
            }
        }
    }
    std::printf("geometry: %zu shapes, %ld admitted, %ld block maps, checksum %016llx\n", shapes.size(), admitted, maps, sum);
    return maps;
}

int main()
{
    parser();
    keys();
    const long maps = geometry();
    if (failures) {
        std::fprintf(stderr, "host unit FAILED: %d expectations\n", failures);
        return 1;
    }
    std::printf("host unit ok: %zu option keys, %ld block maps\n", NFIELDS, maps);
    return 0;
}
