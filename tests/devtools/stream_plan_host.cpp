// plan_launch's decision for the streaming form of the persistent launch (pyrayhf_amd/csrc/prhf_plan.h, LaunchPlan::stream,
// options stream_blocks and stream_grid - the very code prhf_api.cpp compiles) on the host, without a GPU
// (tests/test_stream_plan_host.py).  Stand-alone: builds with g++ alone, also under -fsanitize=address,undefined.
//   stream_plan_host check       the decision against its conditions over the benchmark's shapes; prints "stream_plan_host: ok"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "prhf_plan.h"

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); \
                                             std::printf("\n"); ++failures; } } while (0)

static const int kCus = 256;
struct Slice { long long begin, end; int mode, n_points; };

static LaunchPlan plan_of(long long n_prof, long long n_freq, long long levels, const Slice* sl, int n, const Knobs& kn,
                          bool tall = false) {
    prhf_segment seg[PRHF_MAX_SEGMENTS];
    long long off = 0;
    for (int i = 0; i < n; ++i) {
        seg[i] = prhf_segment{sl[i].begin, sl[i].end, sl[i].mode, sl[i].n_points, off, sl[i].begin * n_freq};
        off += sl[i].n_points;
    }
    const LaunchShape sh = {n_prof, n_freq, levels, levels, tall, off, kCus, PRHF_MATH_AUTO};
    LaunchPlan pl;
    char why[256] = "";
    const int rc = plan_launch(sh, seg, n, kn, pl, why, sizeof why);
    EXPECT(rc == PRHF_OK, "refused: %s", why);
    return pl;
}
static LaunchPlan one(long long n_prof, long long n_freq, int mode, int n_points, const Knobs& kn, long long levels = 620,
                      bool tall = false) {
    const Slice s = {0, n_prof, mode, n_points};
    return plan_of(n_prof, n_freq, levels, &s, 1, kn, tall);
}

// What a streaming plan must look like, and what every other plan must not
static void expect_stream(const LaunchPlan& pl, long long grid, const char* what) {
    EXPECT(pl.stream, "%s must take the streaming form", what);
    EXPECT(pl.queue, "%s: the streaming form draws its blocks from the queue word", what);
    EXPECT(pl.stream_grid == grid, "%s: %lld workgroups, expected %lld", what, pl.stream_grid, grid);
    EXPECT(pl.stream_blocks > 0 && pl.stream_blocks <= pl.blocks && pl.stream_tail_bpp >= 1 && pl.stream_tail_bpp <= pl.seg[0].tail_bpp,
           "%s: the form's blocks", what);
    EXPECT(pl.stream_lds_bytes == 2 * pl.lds_bytes && pl.stream_lds_bytes <= kLdsFull, "%s: two slots: %zu", what, pl.stream_lds_bytes);
    EXPECT(pl.n_segs == 1 && pl.o.n_segs == 0 && pl.x.n_segs == 0 && !pl.tall && !pl.forked, "%s: one slice, alone", what);
    const prhf::SegDev& s = pl.seg[0];
    EXPECT(s.mode == PRHF_KMODE_X && s.tier == 1 && s.chunks == 1 && s.slots == 0 && s.lean && s.sp_off > 0 && s.thread_scan,
           "%s: X mode, fast tier, whole pairs through the strided sum, heights per thread", what);
    EXPECT(pl.freq_table || !s.pair_plan, "%s: a planned slice reads the per-frequency table", what);
    EXPECT(pl.wg_slots == 2 * kCus, "%s: the general kernel's occupancy keeps its meaning", what);
}
static void expect_general(const LaunchPlan& pl, const char* what) {
    EXPECT(!pl.stream && pl.stream_grid == 0 && pl.stream_lds_bytes == 0 && pl.stream_blocks == 0, "%s must keep the general kernel", what);
}

static void check() {
    const Knobs base;
    EXPECT(base.stream_blocks == 1 && base.stream_grid == 0, "defaults");
    // ---- eligible: the config-4 shard and config 4 in full (256 frequencies, X mode, 20000 points, 620 levels) ----
    const LaunchPlan shard = one(12500, 256, PRHF_MODE_X, 20000, base);
    expect_stream(shard, kCus, "config-4 shard");
    // the tail: the last resident round of profiles in half as many pieces as the general kernel's (sixteen waves a block)
    EXPECT(shard.stream_blocks == 12500 - 512 + 2 * 512, "the tail: %lld blocks", shard.stream_blocks);
    EXPECT(shard.stream_tail_bpp == 2 && shard.stream_tail_prof == 12500 - 512, "the form's tail_bpp / tail_prof");
    // ... while the slice's own decomposition stays the general kernel's
    EXPECT(shard.blocks == 12500 - 512 + 4 * 512 && shard.seg[0].tail_bpp == 4 && shard.seg[0].tail_prof == 12500 - 512, "the slice's tail");
    EXPECT(shard.grid == shard.wg_slots, "the general launch's geometry is still planned: %lld", shard.grid);
    expect_stream(one(100000, 256, PRHF_MODE_X, 20000, base), kCus, "config 4 in full");
    // the same slice with 512 frequencies (the limit) and at 8192 points (the strided sum's first size)
    expect_stream(one(12500, 512, PRHF_MODE_X, 8192, base), kCus, "512 frequencies");
    // ---- not eligible ----
    expect_general(one(10000, 174, PRHF_MODE_O, 200, base), "config 3 (short-grid O)");
    {
        const Slice c5[] = {{0, 2500, PRHF_MODE_O, 200}, {2500, 4375, PRHF_MODE_X, 2000}, {4375, 5625, PRHF_MODE_O, 2000},
                            {5625, 6250, PRHF_MODE_X, 20000}};
        expect_general(plan_of(6250, 512, 620, c5, 4, base), "config 5 (mixed list)");
        // ... and its X/20000 slice together with one short-grid slice only: still not alone on the device
        const Slice two[] = {{0, 2500, PRHF_MODE_O, 200}, {2500, 6250, PRHF_MODE_X, 20000}};
        expect_general(plan_of(6250, 512, 620, two, 2, base), "a long slice beside a short-grid launch");
    }
    expect_general(one(1, 174, PRHF_MODE_X, 20000, base), "config 2 (one profile, chunked pairs)");
    expect_general(one(12500, 256, PRHF_MODE_O, 20000, base), "O mode");
    expect_general(one(12500, 256, PRHF_MODE_X, 4096, base), "a grid below the strided sum");
    expect_general(one(12500, 600, PRHF_MODE_X, 20000, base), "600 frequencies");
    expect_general(one(10, 256, PRHF_MODE_X, 20000, base), "few profiles (160 blocks on 512 slots): not persistent");
    expect_general(one(12500, 256, PRHF_MODE_X, 20000, base, 3000, true), "a tall column");
    // 700 levels: one slot fits a workgroup, two do not
    EXPECT(prhf::lds_bytes_for(700) <= kLdsFull && 2 * prhf::lds_bytes_for(700) > kLdsFull, "700 levels: the anchor");
    expect_general(one(12500, 256, PRHF_MODE_X, 20000, base, 700), "700 levels");
    // the most levels two slots hold
    long long most = 1;
    while (2 * prhf::lds_bytes_for(most + 1) <= kLdsFull) ++most;
    expect_stream(one(12500, 256, PRHF_MODE_X, 20000, base, most), kCus, "the most levels of two slots");
    expect_general(one(12500, 256, PRHF_MODE_X, 20000, base, most + 1), "one level more");
    // ---- options ----
    Knobs kn = base;
    kn.stream_blocks = 0;
    const LaunchPlan off = one(12500, 256, PRHF_MODE_X, 20000, kn);
    expect_general(off, "stream_blocks = 0");
    EXPECT(off.queue && off.grid == shard.grid && off.blocks == 12500 - 512 + 4 * 512 && off.lds_bytes == shard.lds_bytes &&
           off.seg[0].tail_bpp == 4 && off.seg[0].tail_prof == shard.seg[0].tail_prof, "the general kernel's tail is quartered");
    EXPECT(std::memcmp(&off.seg[0], &shard.seg[0], sizeof off.seg[0]) == 0 && off.blocks == shard.blocks,
           "the slice's decomposition does not depend on the option");
    kn = base;
    kn.tail_bpp = 2;                           // a tail of two pieces becomes none
    LaunchPlan t2 = one(12500, 256, PRHF_MODE_X, 20000, kn);
    expect_stream(t2, kCus, "tail_bpp = 2");
    EXPECT(t2.stream_blocks == 12500 && t2.stream_tail_bpp == 1 && t2.stream_tail_prof == 12500, "tail_bpp = 2: %lld blocks", t2.stream_blocks);
    kn.tail_bpp = 1;
    t2 = one(12500, 256, PRHF_MODE_X, 20000, kn);
    expect_stream(t2, kCus, "tail_bpp = 1");
    EXPECT(t2.stream_blocks == 12500 && t2.stream_tail_bpp == 1, "tail_bpp = 1");
    kn = base;
    kn.persistent = 0;
    expect_general(one(12500, 256, PRHF_MODE_X, 20000, kn), "persistent = 0");
    kn = base;
    kn.no_candidates = 1;
    expect_general(one(12500, 256, PRHF_MODE_X, 20000, kn), "no_candidates = 1");
    kn = base;
    kn.pair_plan = 0;                          // (without plans every pair plans itself; the form does not depend on it)
    expect_stream(one(12500, 256, PRHF_MODE_X, 20000, kn), kCus, "pair_plan = 0");
    kn = base;
    kn.stream_grid = 7;
    expect_stream(one(12500, 256, PRHF_MODE_X, 20000, kn), 7, "stream_grid = 7");
    kn.stream_grid = 100000;
    expect_stream(one(12500, 256, PRHF_MODE_X, 20000, kn), kCus, "stream_grid above the CUs");
    // fewer blocks than slots: option 2 only; one workgroup for every two blocks
    kn = base;
    kn.target_waves = 64;                      // (the tests' contexts: 24 x 48 pairs are whole work items)
    expect_general(one(24, 48, PRHF_MODE_X, 8192, kn), "24 profiles, stream_blocks = 1");
    kn.stream_blocks = 2;
    // (a slice of few profiles is cut into several blocks per profile: 24 profiles of 48 whole pairs into three each)
    LaunchPlan small = one(24, 48, PRHF_MODE_X, 8192, kn);
    expect_stream(small, 36, "24 profiles, stream_blocks = 2");
    EXPECT(small.blocks == 72 && small.seg[0].blocks_per_prof == 3, "24 x 3 blocks: %lld", small.blocks);
    EXPECT(small.zero_queues != small.freq_table, "the queue word is zeroed by the table's kernel or a memset");
    kn.stream_grid = 1;
    expect_stream(one(24, 48, PRHF_MODE_X, 8192, kn), 1, "stream_grid = 1");
    kn.stream_grid = 2;
    expect_stream(one(24, 48, PRHF_MODE_X, 8192, kn), 2, "stream_grid = 2");
    kn.stream_grid = 0;
    // one workgroup for every two blocks: 1 x 80 whole pairs are eight blocks, 3 x 48 nine
    LaunchPlan few = one(1, 80, PRHF_MODE_X, 8192, kn);
    expect_stream(few, 4, "one profile of whole pairs");
    EXPECT(few.blocks == 8, "one profile in %lld blocks", few.blocks);
    few = one(2, 100, PRHF_MODE_X, 8192, kn);
    expect_stream(few, (few.blocks + 1) / 2, "two profiles");
    few = one(3, 48, PRHF_MODE_X, 8192, kn);
    expect_stream(few, 5, "three profiles");
    EXPECT(few.blocks == 9, "three profiles in %lld blocks", few.blocks);
    expect_general(one(1, 48, PRHF_MODE_X, 8192, kn), "one profile whose pairs are cut into chunks");
    expect_general(one(24, 48, PRHF_MODE_O, 8192, kn), "O mode, stream_blocks = 2");
    // the option table knows both names, with their ranges
    int seen = 0;
    for (const KnobName& k : kKnobNames) {
        if (std::strcmp(k.name, "stream_blocks") == 0) { ++seen; EXPECT(k.lo == 0 && k.hi == 2 && k.field == &Knobs::stream_blocks, "range"); }
        if (std::strcmp(k.name, "stream_grid") == 0) { ++seen; EXPECT(k.lo == 0 && k.field == &Knobs::stream_grid, "range"); }
    }
    EXPECT(seen == 2, "option names");
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::strcmp(argv[1], "check") == 0) {
        check();
        if (failures) return 1;
        std::printf("stream_plan_host: ok\n");
        return 0;
    }
    std::fprintf(stderr, "usage: stream_plan_host check\n");
    return 2;
}
