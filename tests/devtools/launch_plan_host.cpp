// The launch planner of libprhf.so (pyrayhf_amd/csrc/prhf_plan.h, plan_launch) on the host, without a GPU
// (tests/test_launch_plan_host.py).  Two uses:
//   launch_plan_host check      the invariants of launch_plan_checks.h over a table of shapes, two anchors worked out by
//                               hand from plan_slice, and what each launch-shaping option changes; prints
//                               "launch_plan_host: ok"
//   launch_plan_host predict    reads shapes from stdin, one per line -
//                                 name n_prof n_freq n_alt lds_levels tall n_segs {prof_begin prof_end mode n_points}...
//                               - and prints the kernels the plan launches, in the order run() enqueues them:
//                                 name kernel grid workgroup dynamic_lds_bytes
#include <cstdio>
#include <cstring>
#include <string>

#include "prhf_plan.h"
#include "launch_plan_checks.h"

static const int kCus = 256;

struct Case {
    std::string name;
    LaunchShape sh;
    int n_segs;
    prhf_segment seg[PRHF_MAX_SEGMENTS];
};
struct Slice { long long begin, end; int mode, n_points; };

// the work list the Python wrappers make: grids one behind the other, a slice's rows at its profiles' rows
static Case make_case(const char* name, long long n_prof, long long n_freq, long long n_alt, long long lds_levels, bool tall,
                      const Slice* sl, int n) {
    Case c;
    c.name = name;
    c.n_segs = n;
    long long off = 0;
    for (int i = 0; i < n; ++i) {
        c.seg[i] = prhf_segment{sl[i].begin, sl[i].end, sl[i].mode, sl[i].n_points, off, sl[i].begin * n_freq};
        off += sl[i].n_points;
    }
    c.sh = LaunchShape{n_prof, n_freq, n_alt, lds_levels, tall, off, kCus, PRHF_MATH_AUTO};
    return c;
}
static Case one_slice(const char* name, long long n_prof, long long n_freq, int mode, int n_points, long long n_alt = 620,
                      long long lds_levels = 620, bool tall = false) {
    const Slice s = {0, n_prof, mode, n_points};
    return make_case(name, n_prof, n_freq, n_alt, lds_levels, tall, &s, 1);
}

static const Slice kMixed[] = {{0, 300, PRHF_MODE_O, 200}, {300, 500, PRHF_MODE_X, 2000}, {500, 700, PRHF_MODE_O, 500}};
static const Slice kEmptyInside[] = {{0, 300, PRHF_MODE_O, 200}, {300, 300, PRHF_MODE_X, 2000}, {300, 700, PRHF_MODE_X, 2000}};
static const Slice kEight[] = {{0, 100, PRHF_MODE_O, 200}, {100, 200, PRHF_MODE_X, 200}, {200, 300, PRHF_MODE_O, 500},
                               {300, 400, PRHF_MODE_X, 2000}, {400, 400, PRHF_MODE_O, 50}, {400, 500, PRHF_MODE_X, 8192},
                               {500, 600, PRHF_MODE_O, 1000}, {600, 700, PRHF_MODE_X, 500}};

static int failures = 0;
#define CHECK(cond, ...)                                               \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::fprintf(stderr, "CHECK failed: %s: ", #cond);         \
            std::fprintf(stderr, __VA_ARGS__);                         \
            std::fprintf(stderr, "\n");                                \
            ++failures;                                                \
        }                                                              \
    } while (0)

static LaunchPlan plan_of(const Case& c, const Knobs& kn) {
    LaunchPlan pl;
    char why[160] = "";
    const int rc = plan_launch(c.sh, c.seg, c.n_segs, kn, pl, why, sizeof why);
    CHECK(rc == PRHF_OK, "%s: %s", c.name.c_str(), why);
    failures += check_plan(c.name.c_str(), c.sh, c.seg, c.n_segs, kn, pl);
    return pl;
}

// ---- comparisons for the option cases: which part of a plan an option moved
static auto geometry(const prhf::SegDev& s) {
    return std::make_tuple(s.prof_begin, s.prof_end, s.mult_off, s.out_off, s.block_begin, s.partial_off, s.altmin_off, s.mode, s.n_points,
                           s.chunks, s.chunk_len, s.slots, s.blocks_per_prof, s.tier, s.tail_prof, s.tail_bpp, s.well_conditioned, s.lean,
                           s.prio, s.thread_scan);
}
static auto tables(const prhf::SegDev& s) { return std::make_tuple(s.sp_off, s.strided_lower, s.panel_lower, s.pair_plan); }
static auto fields(const ShortLaunch& l) {
    return std::make_tuple(l.lds_levels, l.threads, l.queue_entries, l.short_queue, l.lds_bytes, l.slots, l.grid, l.queue);
}
static bool same_kind(const ShortKind& a, const ShortKind& b) {
    if (a.n_segs != b.n_segs || a.blocks != b.blocks) return false;
    for (int i = 0; i < a.n_segs; ++i)
        if (geometry(a.seg[i]) != geometry(b.seg[i]) || tables(a.seg[i]) != tables(b.seg[i])) return false;
    if (a.blocks == 0) return true;
    return a.second == b.second && a.lanes == b.lanes && a.follow_grid == b.follow_grid && a.list_bytes == b.list_bytes &&
           fields(a.first) == fields(b.first) && (!a.second || fields(a.full) == fields(b.full));
}
static bool same_general(const LaunchPlan& a, const LaunchPlan& b) {        // slices, blocks and scratch; not grid and queue
    if (a.n_segs != b.n_segs || a.blocks != b.blocks || a.launch_tier != b.launch_tier || a.wg_slots != b.wg_slots ||
        a.lds_bytes != b.lds_bytes || a.partial_elems != b.partial_elems || a.altmin_elems != b.altmin_elems || a.out_rows != b.out_rows ||
        a.tall_stride != b.tall_stride || a.tall_slabs != b.tall_slabs)
        return false;
    for (int i = 0; i < a.n_segs; ++i)
        if (geometry(a.seg[i]) != geometry(b.seg[i])) return false;
    return true;
}
static bool same_grid(const LaunchPlan& a, const LaunchPlan& b) { return a.grid == b.grid && a.queue == b.queue; }
static bool same_tables(const LaunchPlan& a, const LaunchPlan& b) {
    if (a.n_segs != b.n_segs || a.want_pairs != b.want_pairs || a.table_entries != b.table_entries || a.any_plan != b.any_plan ||
        a.freq_table != b.freq_table || a.short_order != b.short_order || a.zero_queues != b.zero_queues ||
        std::memcmp(&a.pieces, &b.pieces, sizeof a.pieces) != 0)
        return false;
    for (int i = 0; i < a.n_segs; ++i)
        if (tables(a.seg[i]) != tables(b.seg[i])) return false;
    return true;
}

static void table_of_shapes() {
    const Knobs kn;
    const Case cases[] = {
        one_slice("single profile x 174, X/20000", 1, 174, PRHF_MODE_X, 20000),
        one_slice("12500 x 256, X/20000", 12500, 256, PRHF_MODE_X, 20000),
        one_slice("10000 x 174, O/200", 10000, 174, PRHF_MODE_O, 200),
        one_slice("700 x 44, X/2000", 700, 44, PRHF_MODE_X, 2000),
        one_slice("200 x 44, O/200", 200, 44, PRHF_MODE_O, 200),
        one_slice("700 x 64, X/500", 700, 64, PRHF_MODE_X, 500),
        make_case("the mixed list of test_gpu_launch_knobs.py", 700, 64, 620, 620, false, kMixed, 3),
        one_slice("tall column, X/2000", 8, 44, PRHF_MODE_X, 2000, 2000, 2000, true),
        one_slice("tall column, O/200", 8, 44, PRHF_MODE_O, 200, 2000, 2000, true),
        one_slice("tall column, 20000 x 44 O/200", 20000, 44, PRHF_MODE_O, 200, 2000, 2000, true),
        one_slice("trimmed column, X/2000", 8, 44, PRHF_MODE_X, 2000, 2000, 1097, false),
        one_slice("trimmed column, 700 x 44 O/200", 700, 44, PRHF_MODE_O, 200, 2000, 1097, false),
        one_slice("trimmed column, 700 x 64 X/500", 700, 64, PRHF_MODE_X, 500, 2000, 1399, false),
        one_slice("no profiles", 0, 44, PRHF_MODE_X, 2000),
        make_case("an empty slice inside a list", 700, 64, 620, 620, false, kEmptyInside, 3),
        make_case("eight segments", 700, 64, 620, 620, false, kEight, 8),
        one_slice("64 x 256, X/8192", 64, 256, PRHF_MODE_X, 8192),
    };
    for (const Case& c : cases) (void)plan_of(c, kn);
    // every input slice of the mixed list where it belongs
    const LaunchPlan mixed = plan_of(cases[6], kn);
    CHECK(mixed.n_segs == 1 && mixed.o.n_segs == 2 && mixed.x.n_segs == 0 && mixed.o.blocks == 500 && mixed.forked, "the mixed list");
    const LaunchPlan eight = plan_of(cases[15], kn);
    CHECK(eight.n_segs == 3 && eight.o.n_segs == 3 && eight.x.n_segs == 2 && eight.o.blocks == 300 && eight.x.blocks == 200, "eight segments");
    CHECK(eight.o.lanes == 16 && mixed.o.lanes == 16 && plan_of(cases[2], kn).o.lanes == 8, "lanes per pair");
    const LaunchPlan tall = plan_of(cases[9], kn);
    CHECK(tall.tall && tall.queue && tall.grid == 2 * kCus && tall.tall_slabs == 2 * kCus && tall.o.n_segs == 0 && tall.no_candidates == 1, "tall launch");
    const LaunchPlan none = plan_of(cases[13], kn);
    CHECK(none.blocks == 0 && none.grid == 0 && !none.queue && !none.forked && none.o.blocks == 0 && none.x.blocks == 0, "no profiles");
    // planner errors carry a message
    LaunchPlan pl;
    char why[160] = "";
    Case bad = cases[3];
    bad.seg[0].prof_end = 701;
    CHECK(plan_launch(bad.sh, bad.seg, 1, kn, pl, why, sizeof why) == PRHF_EINVAL && why[0], "a profile range outside the batch was planned");
    Case huge = one_slice("too large", 3000000000LL, 174, PRHF_MODE_O, 200);
    why[0] = 0;
    CHECK(plan_launch(huge.sh, huge.seg, 1, kn, pl, why, sizeof why) == PRHF_EINVAL && !std::strcmp(why, "launch too large"), "3e9 blocks: %s", why);
}

// Two plans that follow from plan_slice by hand
static void anchors() {
    const Knobs kn;
    // One profile x 174 frequencies x 20000 points: 174 pairs < 4096 waves; min(ceil(4096 / 174) = 24, ceil(20000 / 256) = 79, 8
    // waves) -> S = 8 slots of ceil(20000 / 8 = 2500 -> 2560) points: 8 chunks; 174 x 8 / 8 = 174 workgroups on 512 slots
    const LaunchPlan a = plan_of(one_slice("anchor: single profile", 1, 174, PRHF_MODE_X, 20000), kn);
    CHECK(a.n_segs == 1 && a.seg[0].slots == 8 && a.seg[0].chunks == 8 && a.seg[0].chunk_len == 2560, "slots %d chunks %d x %d",
          a.seg[0].slots, a.seg[0].chunks, a.seg[0].chunk_len);
    CHECK(a.blocks == 174 && a.grid == 174 && !a.queue && a.wg_slots == 512, "%lld blocks, grid %lld", a.blocks, a.grid);
    CHECK(!a.freq_table && !a.zero_queues && a.want_pairs && a.seg[0].lean == 1 && a.partial_elems == 0, "tables of the single profile");
    CHECK(a.launch_tier == 1 && a.o.n_segs == 0 && a.x.n_segs == 0 && !a.forked, "one fast-tier launch");
    // 12500 x 256 x 20000: one workgroup per profile, the last round of 512 slots cut into 4 workgroups per profile:
    // 11988 + 512 x 4 = 14036 blocks on a queue of 512 workgroups
    const LaunchPlan h = plan_of(one_slice("anchor: headline", 12500, 256, PRHF_MODE_X, 20000), kn);
    CHECK(h.n_segs == 1 && h.seg[0].tail_prof == 11988 && h.seg[0].tail_bpp == 4 && h.seg[0].blocks_per_prof == 1, "tail %lld x %d",
          h.seg[0].tail_prof, h.seg[0].tail_bpp);
    CHECK(h.blocks == 14036 && h.queue && h.grid == 512, "%lld blocks, grid %lld", h.blocks, h.grid);
    CHECK(h.pieces.n == 1 && h.pieces.sp_off[0] == 20000 + PRHF_PAIR_PAD && h.seg[0].sp_off == 20000 + PRHF_PAIR_PAD, "piece at %lld", h.pieces.sp_off[0]);
    CHECK(h.seg[0].pair_plan == 1 && h.any_plan && h.freq_table && !h.short_order && h.seg[0].strided_lower == 1 && h.seg[0].panel_lower == 1, "planning pass");
    CHECK(h.table_entries == 20000 + PRHF_PAIR_PAD + prhf::strided_piece_entries(20000), "table of %lld entries", h.table_entries);
}

// What each launch-shaping option changes in a plan - and what it leaves alone
static void options() {
    const Knobs base;
    const Case eight = make_case("options: eight segments", 700, 64, 620, 620, false, kEight, 8);
    const Case headline = one_slice("options: headline", 12500, 256, PRHF_MODE_X, 20000);
    const Case config3 = one_slice("options: 10000 x 174 O/200", 10000, 174, PRHF_MODE_O, 200);
    const LaunchPlan b8 = plan_of(eight, base), bh = plan_of(headline, base), b3 = plan_of(config3, base);
    CHECK(b8.o.first.threads == PRHF_COMPACT_THREADS && b8.x.first.threads == PRHF_COMPACT_THREADS && b8.o.second && b8.x.second, "default: compact");
    CHECK(b3.short_order && b3.o.first.queue && b3.o.blocks == 10000 && b3.n_segs == 0 && !b3.forked, "default: config 3");
    Knobs kn = base;
    kn.short_kernel = 0;
    LaunchPlan p = plan_of(eight, kn);
    CHECK(p.o.n_segs == 0 && p.o.blocks == 0 && p.n_segs == b8.n_segs + b8.o.n_segs && same_kind(p.x, b8.x) && p.forked &&
          std::memcmp(&p.pieces, &b8.pieces, sizeof p.pieces) == 0 && p.freq_table && !p.short_order, "short_kernel = 0");
    kn = base;
    kn.shortx_kernel = 0;
    p = plan_of(eight, kn);
    CHECK(p.x.n_segs == 0 && p.x.blocks == 0 && p.n_segs == b8.n_segs + b8.x.n_segs && same_kind(p.o, b8.o) && p.forked &&
          std::memcmp(&p.pieces, &b8.pieces, sizeof p.pieces) == 0, "shortx_kernel = 0");
    kn = base;
    kn.short_compact = 0;
    p = plan_of(eight, kn);
    CHECK(p.o.first.threads == PRHF_SHORT_THREADS && p.x.first.threads == PRHF_SHORT_THREADS && !p.o.second && !p.x.second &&
          p.o.first.lds_levels == 620 && p.o.n_segs == b8.o.n_segs && p.x.blocks == b8.x.blocks && p.o.lanes == b8.o.lanes &&
          same_general(p, b8) && same_grid(p, b8) && same_tables(p, b8) && p.forked == b8.forked, "short_compact = 0");
    kn = base;
    kn.short_concurrent = 0;
    p = plan_of(eight, kn);
    CHECK(!p.forked && b8.forked && same_general(p, b8) && same_grid(p, b8) && same_tables(p, b8) && same_kind(p.o, b8.o) && same_kind(p.x, b8.x),
          "short_concurrent = 0");
    kn = base;
    kn.persistent = 0;
    p = plan_of(headline, kn);
    CHECK(!p.queue && bh.queue && p.grid == p.blocks && same_general(p, bh) && p.any_plan == bh.any_plan && p.freq_table == bh.freq_table &&
          std::memcmp(&p.pieces, &bh.pieces, sizeof p.pieces) == 0 && tables(p.seg[0]) == tables(bh.seg[0]), "persistent = 0");
    p = plan_of(config3, kn);                                           // (the short-grid kernels keep their queues)
    CHECK(same_kind(p.o, b3.o) && same_tables(p, b3), "persistent = 0 and the short grids");
    for (const Case* c : {&eight, &headline}) {
        const LaunchPlan& b = c == &eight ? b8 : bh;
        kn = base;
        kn.strided_top = 0;
        p = plan_of(*c, kn);
        bool clean = p.pieces.n == 0 && p.table_entries == c->sh.mult_len + PRHF_PAIR_PAD && !p.any_plan;
        for (int i = 0; i < p.n_segs; ++i) clean = clean && tables(p.seg[i]) == std::make_tuple(0LL, 0, 0, 0);
        CHECK(clean && b.pieces.n == 1 && same_general(p, b) && same_grid(p, b) && same_kind(p.o, b.o) && same_kind(p.x, b.x) &&
              p.want_pairs == b.want_pairs && p.forked == b.forked, "strided_top = 0: %s", c->name.c_str());
        kn = base;
        kn.pair_plan = 0;
        p = plan_of(*c, kn);
        bool off = !p.any_plan && b.any_plan && std::memcmp(&p.pieces, &b.pieces, sizeof p.pieces) == 0 && p.table_entries == b.table_entries;
        for (int i = 0; i < p.n_segs; ++i)
            off = off && p.seg[i].pair_plan == 0 && p.seg[i].sp_off == b.seg[i].sp_off && p.seg[i].strided_lower == b.seg[i].strided_lower &&
                  p.seg[i].panel_lower == b.seg[i].panel_lower;
        CHECK(off && same_general(p, b) && same_grid(p, b) && same_kind(p.o, b.o) && same_kind(p.x, b.x) && p.freq_table == b.freq_table,
              "pair_plan = 0: %s", c->name.c_str());
    }
    kn = base;
    kn.short_queue = 16;
    p = plan_of(eight, kn);
    ShortKind o16 = p.o;
    CHECK(o16.first.short_queue == -16 && o16.second && o16.full.short_queue == -16, "short_queue = 16: %d / %d", o16.first.short_queue, o16.full.short_queue);
    o16.first.short_queue = b8.o.first.short_queue;
    o16.full.short_queue = b8.o.full.short_queue;
    CHECK(same_kind(o16, b8.o) && same_kind(p.x, b8.x) && same_general(p, b8) && same_grid(p, b8) && same_tables(p, b8) && p.forked == b8.forked,
          "short_queue = 16 moved something else");
    kn = base;
    kn.no_candidates = 1;
    p = plan_of(eight, kn);
    CHECK(p.no_candidates == 1 && b8.no_candidates == 0 && p.o.n_segs == 0 && p.x.n_segs == 0 && p.n_segs == 8 && !p.any_plan && !p.forked &&
          std::memcmp(&p.pieces, &b8.pieces, sizeof p.pieces) == 0, "no_candidates = 1");
    p = plan_of(headline, kn);
    CHECK(p.no_candidates == 1 && p.seg[0].pair_plan == 0 && !p.any_plan && same_general(p, bh) && same_grid(p, bh) &&
          p.seg[0].sp_off == bh.seg[0].sp_off, "no_candidates = 1: headline");
}

static void print_launch(const char* name, const char* kernel, long long grid, int threads, size_t lds) {
    if (grid > 0) std::printf("%s %s %lld %d %zu\n", name, kernel, grid, threads, lds);
}

static void predict_kind(const char* name, const LaunchPlan& pl, const ShortKind& k, bool xmode) {
    if (k.blocks == 0) return;
    char kernel[64];
    for (int second = 0; second <= (k.second ? 1 : 0); ++second) {
        const ShortLaunch& l = second ? k.full : k.first;
        if (xmode) std::snprintf(kernel, sizeof kernel, "vfo_shortx_kernel<%d>", l.threads);
        else std::snprintf(kernel, sizeof kernel, "vfo_short_kernel<%d,%d>", l.threads, k.lanes);
        print_launch(name, kernel, l.grid, l.threads, l.lds_bytes);
    }
    std::snprintf(kernel, sizeof kernel, "vfo_kernel<%d,%d>", xmode ? 1 : 0, PRHF_BLOCK_THREADS);
    print_launch(name, kernel, k.follow_grid, PRHF_BLOCK_THREADS, pl.lds_bytes);
}

static int predict() {
    char name[128];
    long long n_prof, n_freq, n_alt, lds_levels;
    int tall, n;
    const Knobs kn;
    while (std::scanf("%127s %lld %lld %lld %lld %d %d", name, &n_prof, &n_freq, &n_alt, &lds_levels, &tall, &n) == 7) {
        Slice sl[PRHF_MAX_SEGMENTS];
        if (n < 1 || n > PRHF_MAX_SEGMENTS) return 2;
        for (int i = 0; i < n; ++i) {
            char mode[8];
            if (std::scanf("%lld %lld %7s %d", &sl[i].begin, &sl[i].end, mode, &sl[i].n_points) != 4) return 2;
            sl[i].mode = mode[0] == 'O' ? PRHF_MODE_O : PRHF_MODE_X;
        }
        const Case c = make_case(name, n_prof, n_freq, n_alt, lds_levels, tall != 0, sl, n);
        const LaunchPlan pl = plan_of(c, kn);
        if (pl.freq_table) print_launch(name, pl.short_order ? "short_order_kernel" : "freq_table_kernel", 1, 0, 0);
        char kernel[64];
        if (pl.tall) std::snprintf(kernel, sizeof kernel, "vfo_tall_kernel<%d>", PRHF_BLOCK_THREADS);
        else std::snprintf(kernel, sizeof kernel, "vfo_kernel<%d,%d>", pl.launch_tier, PRHF_BLOCK_THREADS);
        if (pl.forked) print_launch(name, kernel, pl.grid, PRHF_BLOCK_THREADS, pl.lds_bytes);
        predict_kind(name, pl, pl.x, true);
        predict_kind(name, pl, pl.o, false);
        if (!pl.forked) print_launch(name, kernel, pl.grid, PRHF_BLOCK_THREADS, pl.lds_bytes);
    }
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "predict")) return predict();
    table_of_shapes();
    anchors();
    options();
    if (failures) {
        std::fprintf(stderr, "launch_plan_host: %d checks failed\n", failures);
        return 1;
    }
    std::printf("launch_plan_host: ok\n");
    return 0;
}
