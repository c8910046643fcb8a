// The structural invariants of a launch plan (pyrayhf_amd/csrc/prhf_plan.h, plan_launch), shared by the host test of
// the planner (launch_plan_host.cpp, tests/test_launch_plan_host.py) and the sanitizer sweep (sanitize_host.cpp).
// Include after prhf_plan.h.  check_plan() prints every broken invariant to stderr and returns their number.
#ifndef LAUNCH_PLAN_CHECKS_H
#define LAUNCH_PLAN_CHECKS_H

#include <cstdio>
#include <tuple>

#define PLAN_CHECK(cond, ...)                                          \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::fprintf(stderr, "%s: broken: %s: ", what, #cond);     \
            std::fprintf(stderr, __VA_ARGS__);                         \
            std::fprintf(stderr, "\n");                                \
            ++bad;                                                     \
        }                                                              \
    } while (0)

static inline bool same_slice(const prhf::SegDev& s, const prhf_segment& u) {
    return s.prof_begin == u.prof_begin && s.prof_end == u.prof_end && s.mult_off == u.mult_offset && s.out_off == u.out_offset &&
           s.n_points == u.n_points && s.mode == (u.mode == PRHF_MODE_O ? PRHF_KMODE_O : PRHF_KMODE_X);
}

// one short-grid launch against the kernel header's formulas
static inline int check_short_launch(const char* what, const ShortLaunch& l, bool xmode, bool from_list, long long blocks,
                                     const LaunchShape& sh, const Knobs& kn) {
    int bad = 0;
    const bool compact = l.threads == PRHF_COMPACT_THREADS;
    PLAN_CHECK(compact || l.threads == PRHF_SHORT_THREADS, "threads %d", l.threads);
    PLAN_CHECK(l.lds_levels >= 1 && l.lds_levels <= sh.lds_levels, "levels %lld of %lld", l.lds_levels, sh.lds_levels);
    const size_t want = xmode ? prhf::shortx_lds_bytes(l.lds_levels, sh.n_freq)
                              : prhf::short_lds_fixed(l.lds_levels, sh.n_freq, l.threads) + 8 * (size_t)l.queue_entries;
    PLAN_CHECK(l.lds_bytes == want, "LDS %zu, the kernel's formula gives %zu", l.lds_bytes, want);
    PLAN_CHECK(l.lds_bytes <= 160 * 1024, "LDS %zu", l.lds_bytes);
    if (compact) PLAN_CHECK(l.lds_bytes <= (160 * 1024) / 4 - PRHF_COMPACT_RESERVE, "compact LDS %zu", l.lds_bytes);
    if (compact) PLAN_CHECK(l.slots == 4LL * sh.cu_count, "compact slots %lld", l.slots);
    else PLAN_CHECK(l.slots == sh.cu_count * (l.lds_bytes <= 80 * 1024 - 512 ? 2 : 1), "slots %lld for %zu bytes", l.slots, l.lds_bytes);
    if (xmode) PLAN_CHECK(l.queue_entries == 0 && l.short_queue == 0, "X mode has no LDS queue");
    else {
        PLAN_CHECK(l.queue_entries >= (compact ? PRHF_COMPACT_MIN_QUEUE : 64) && l.queue_entries <= PRHF_SHORT_MAX_QUEUE, "queue of %d entries", l.queue_entries);
        if (kn.short_queue > 0) PLAN_CHECK(l.short_queue == -std::min((int)kn.short_queue, l.queue_entries), "fixed queue %d", l.short_queue);
        else PLAN_CHECK(l.short_queue == l.queue_entries, "queue argument %d for %d entries", l.short_queue, l.queue_entries);
    }
    PLAN_CHECK(l.queue == (from_list || blocks > l.slots), "queue %d: %lld blocks on %lld slots", (int)l.queue, blocks, l.slots);
    PLAN_CHECK(l.grid == std::min(blocks, l.slots) && l.grid >= 1, "grid %lld", l.grid);
    return bad;
}

static inline int check_short_kind(const char* what, const ShortKind& k, bool xmode, const LaunchShape& sh, const Knobs& kn,
                                   const LaunchPlan& pl) {
    int bad = 0;
    long long blocks = 0;
    for (int i = 0; i < k.n_segs; ++i) {
        const prhf::SegDev& s = k.seg[i];
        PLAN_CHECK(s.block_begin == blocks, "slice %d begins at block %lld, not %lld", i, s.block_begin, blocks);
        blocks += s.prof_end - s.prof_begin;
        PLAN_CHECK(s.blocks_per_prof == 1 && s.tail_bpp == 1 && s.chunks == 1 && s.slots == 0 && s.lean == 1, "slice %d is not one block per profile", i);
        PLAN_CHECK(s.mode == (xmode ? PRHF_KMODE_X : PRHF_KMODE_O) && s.tier == (xmode ? 1 : 0), "slice %d: mode %d tier %d", i, s.mode, s.tier);
        PLAN_CHECK(s.n_points >= PRHF_SHORT_MIN_POINTS && s.n_points <= (xmode ? PRHF_SHORTX_MAX_POINTS : PRHF_SHORT_MAX_POINTS), "slice %d: %d points", i, s.n_points);
        PLAN_CHECK(s.pair_plan == 0 && s.sp_off == 0, "slice %d plans pairs", i);
    }
    PLAN_CHECK(k.blocks == blocks, "%lld blocks, slices hold %lld", k.blocks, blocks);
    if (k.n_segs > 0) PLAN_CHECK(!sh.tall && pl.want_pairs && pl.freq_table, "short grids without their tables");
    if (k.blocks == 0) return bad;
    PLAN_CHECK(k.list_bytes == (size_t)(k.blocks + 1) * sizeof(unsigned), "list of %zu bytes", k.list_bytes);
    PLAN_CHECK(k.follow_grid == std::min(k.blocks, pl.wg_slots), "follow-up grid %lld", k.follow_grid);
    bad += check_short_launch(what, k.first, xmode, false, k.blocks, sh, kn);
    // a second launch exactly when the compact arrays hold fewer levels than the column
    PLAN_CHECK(k.second == (k.first.threads == PRHF_COMPACT_THREADS && k.first.lds_levels < sh.lds_levels), "second %d", (int)k.second);
    if (k.first.threads == PRHF_COMPACT_THREADS) PLAN_CHECK(2 * k.first.lds_levels >= sh.lds_levels, "compact arrays hold %lld of %lld", k.first.lds_levels, sh.lds_levels);
    else PLAN_CHECK(k.first.lds_levels == sh.lds_levels, "full-size arrays of %lld levels", k.first.lds_levels);
    if (k.second) {
        bad += check_short_launch(what, k.full, xmode, true, k.blocks, sh, kn);
        PLAN_CHECK(k.full.threads == PRHF_SHORT_THREADS && k.full.lds_levels == sh.lds_levels, "second launch is not full-size");
    }
    if (!xmode) PLAN_CHECK(k.lanes == 8 || k.lanes == 16, "%d lanes", k.lanes);
    return bad;
}

static inline int check_plan(const char* what, const LaunchShape& sh, const prhf_segment* segs, int n_segs, const Knobs& kn,
                             const LaunchPlan& pl) {
    int bad = 0;
    // every input slice lands in exactly one of general, short O, short X
    PLAN_CHECK(pl.n_segs + pl.o.n_segs + pl.x.n_segs == n_segs, "%d + %d + %d slices of %d", pl.n_segs, pl.o.n_segs, pl.x.n_segs, n_segs);
    for (int i = 0; i < n_segs; ++i) {
        int found = 0;
        for (int k = 0; k < pl.n_segs; ++k) found += same_slice(pl.seg[k], segs[i]);
        for (int k = 0; k < pl.o.n_segs; ++k) found += same_slice(pl.o.seg[k], segs[i]);
        for (int k = 0; k < pl.x.n_segs; ++k) found += same_slice(pl.x.seg[k], segs[i]);
        PLAN_CHECK(found == 1, "input slice %d found %d times", i, found);
    }
    // block ranges contiguous, ascending, disjoint; scratch offsets disjoint
    long long blocks = 0, partial = 0, altmin = 0, rows = 0;
    int tier = 0;
    for (int i = 0; i < pl.n_segs; ++i) {
        const prhf::SegDev& s = pl.seg[i];
        const long long P = s.prof_end - s.prof_begin;
        PLAN_CHECK(s.block_begin == blocks, "slice %d begins at block %lld, not %lld", i, s.block_begin, blocks);
        PLAN_CHECK(s.tail_prof >= 0 && s.tail_prof <= P && s.blocks_per_prof >= 1 && s.tail_bpp >= 1, "slice %d: tail", i);
        blocks += s.tail_prof * s.blocks_per_prof + (P - s.tail_prof) * s.tail_bpp;
        if (s.chunks > 1 && s.slots == 0) {
            PLAN_CHECK(s.partial_off == partial && s.altmin_off == altmin, "slice %d: scratch at %lld / %lld", i, s.partial_off, s.altmin_off);
            partial += P * sh.n_freq * s.chunks;
            altmin += P;
        }
        PLAN_CHECK(s.prio == std::max(0, 3 - i), "slice %d: priority %d", i, s.prio);
        tier = (i == 0 || tier == s.tier) ? s.tier : 2;
        if (sh.tall) PLAN_CHECK(s.thread_scan == 0 && s.sp_off == 0 && s.pair_plan == 0, "tall slice %d on an LDS path", i);
        // the planning pass only where slice_plans_pairs holds, the strided flags only with a piece
        if (s.pair_plan) PLAN_CHECK(slice_plans_pairs(s, sh.tall, sh.n_freq, sh.lds_levels, kn), "slice %d plans pairs", i);
        if (s.sp_off == 0) PLAN_CHECK(!s.strided_lower && !s.panel_lower && !s.pair_plan, "slice %d: strided flags without a piece", i);
        if (s.sp_off > 0) {
            int hits = 0;
            for (int p = 0; p < pl.pieces.n; ++p)
                hits += pl.pieces.sp_off[p] == s.sp_off && pl.pieces.mult_off[p] == s.mult_off && pl.pieces.n_points[p] == s.n_points;
            PLAN_CHECK(hits == 1, "slice %d: piece at %lld found %d times", i, s.sp_off, hits);
        }
        if (s.lean) PLAN_CHECK(pl.want_pairs, "slice %d takes the main loop without a pair table", i);
    }
    for (int i = 0; i < n_segs; ++i) rows = std::max<long long>(rows, segs[i].out_offset / sh.n_freq + (segs[i].prof_end - segs[i].prof_begin));
    PLAN_CHECK(pl.blocks == blocks && pl.partial_elems == partial && pl.altmin_elems == altmin && pl.out_rows == rows,
               "%lld blocks, %lld + %lld scratch, %lld rows", pl.blocks, pl.partial_elems, pl.altmin_elems, pl.out_rows);
    PLAN_CHECK(pl.launch_tier == tier && pl.tall == sh.tall, "tier %d", pl.launch_tier);
    // the general launch: a queue exactly when its blocks exceed its resident slots (and the option allows it)
    const size_t lds = sh.tall ? prhf::lds_bytes_tall() : prhf::lds_bytes_for(sh.lds_levels);
    PLAN_CHECK(pl.lds_bytes == lds && pl.wg_slots == sh.cu_count * (lds <= 80 * 1024 ? 2 : 1), "LDS %zu, %lld slots", pl.lds_bytes, pl.wg_slots);
    PLAN_CHECK(pl.queue == ((kn.persistent != 0 || sh.tall) && pl.blocks > pl.wg_slots), "queue %d", (int)pl.queue);
    PLAN_CHECK(pl.grid == (pl.queue ? pl.wg_slots : pl.blocks), "grid %lld", pl.grid);
    if (sh.tall && pl.blocks > 0) PLAN_CHECK(pl.tall_stride >= prhf::tall_slab_bytes(sh.n_alt) && pl.tall_slabs == pl.grid, "slabs %lld x %llu", pl.tall_slabs, pl.tall_stride);
    else PLAN_CHECK(pl.tall_stride == 0, "slabs without a tall launch");
    PLAN_CHECK(pl.no_candidates == (kn.no_candidates != 0 || sh.tall), "no_candidates %d", pl.no_candidates);
    bad += check_short_kind(what, pl.o, false, sh, kn, pl);
    bad += check_short_kind(what, pl.x, true, sh, kn, pl);
    // tables: the per-frequency table whenever a slice plans its pairs; pieces deduplicated, behind the pair table, disjoint
    bool any_plan = false;
    for (int i = 0; i < pl.n_segs; ++i) any_plan = any_plan || pl.seg[i].pair_plan != 0;
    PLAN_CHECK(pl.any_plan == any_plan, "any_plan %d", (int)pl.any_plan);
    if (pl.any_plan) PLAN_CHECK(pl.freq_table, "a slice plans its pairs without the per-frequency table");
    if (pl.freq_table) PLAN_CHECK(pl.want_pairs, "per-frequency table without the pair table");
    if (pl.short_order) PLAN_CHECK(pl.freq_table && pl.o.blocks >= 4 * pl.o.first.slots, "block order for %lld blocks", pl.o.blocks);
    long long end = sh.mult_len + PRHF_PAIR_PAD;
    PLAN_CHECK(pl.pieces.n >= 0 && pl.pieces.n <= PRHF_MAX_SEGMENTS, "%d pieces", pl.pieces.n);
    for (int p = 0; p < pl.pieces.n && p < PRHF_MAX_SEGMENTS; ++p) {
        PLAN_CHECK(pl.pieces.sp_off[p] == end, "piece %d at %lld, table ends at %lld", p, pl.pieces.sp_off[p], end);
        end += prhf::strided_piece_entries(pl.pieces.n_points[p]);
        for (int q = 0; q < p; ++q)
            PLAN_CHECK(!(pl.pieces.mult_off[q] == pl.pieces.mult_off[p] && pl.pieces.n_points[q] == pl.pieces.n_points[p]), "pieces %d and %d are one grid", q, p);
    }
    PLAN_CHECK(pl.table_entries == end && end * 16 < 0x7fffffffLL + (pl.pieces.n ? 0 : (1LL << 40)), "table of %lld entries", pl.table_entries);
    const bool any_short = pl.o.n_segs > 0 || pl.x.n_segs > 0;
    PLAN_CHECK(pl.forked == (any_short && pl.blocks > 0 && kn.short_concurrent != 0), "forked %d", (int)pl.forked);
    PLAN_CHECK(pl.zero_queues == (!pl.freq_table && (any_short || pl.queue)), "zero_queues %d", (int)pl.zero_queues);
    return bad;
}

#endif  // LAUNCH_PLAN_CHECKS_H
