// prhf_plan.h - the host-side launch planner of libprhf.so: the context options (Knobs), the validation of a work list
// (validate_work_list), the decomposition of a slice into wave-sized items and blocks (plan_slice) and, on top of them,
// plan_launch: every decision of one operator call - which slices go to the general kernel and which to the short-grid
// kernels, the geometry, LDS size and block queue of each launch, the strided table's pieces, the tables to build, the
// second stream - as one LaunchPlan of plain data, which run() in prhf_api.cpp executes.  The names of the context's
// control words (StatusWord) live here too.  No HIP call and no device state in here - plain arithmetic on the
// caller's descriptors - so that the same code is compiled into prhf_api.cpp and into the host tests
// (tests/test_launch_plan_host.py; under -fsanitize=address,undefined tests/devtools/sanitize_host.cpp,
// tests/test_sanitizers_host.py).  Everything lives in an anonymous namespace: internal to the including file.

#ifndef PRHF_PLAN_H
#define PRHF_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "prhf.h"
#include "prhf_kernels.h"

namespace {

// Launch-shaping and arithmetic settings of one context (prhf_ctx_set_option).  The defaults are
// the measured best; tests and A/B runs change them per context.  Only a -DPRHF_DIAG build reads them from the
// environment as well (PRHF_<NAME>, at context creation).
struct Knobs {
    double target_waves = 4096;        // waves resident at two 8-wave workgroups per CU: few-pair launches are chunked up to this
    double lean_min_points = 65;       // shorter grids skip the pair table and the main loop
    double well_conditioned = 1e-5;    // default O-mode arithmetic: the reference's operation order where 1 - X <= this
    double thread_scan_min = 0.0;      // n_freq x n_points from which X mode settles reflection heights per thread
    double no_candidates = 0;          // 1: no per-profile candidate list, every frequency is a work item
    double persistent = 1;             // 0: one workgroup per block, hardware dispatch order
    double tail_rounds = 1.0;          // resident rounds of workgroups at the end of a long slice that are cut finer
    double tail_bpp = 4;               // ... into this many workgroups per profile (1: no tail refinement)
    double split_min_points = 1024;    // few-profile slices are cut into several workgroups per profile from this grid size
    double split_few_profiles = 1;     // 0: one workgroup per profile whatever their number
    double short_kernel = 1;           // 0: short O-mode grids stay in the general kernel
    double shortx_kernel = 1;          // 0: X-mode grids of up to 4096 points stay in the general kernel
    double short_concurrent = 1;       // 0: short-grid and general launch of a mixed list one after the other
    double short_queue = 0;            // > 0: the short-grid kernel's queue holds exactly this many entries (tests)
    double direct_upload = 1;          // small host-buffer calls on a large-BAR device: the CPU writes the inputs straight into
                                       // device memory (0: pinned staging buffer + hipMemcpyAsync)
    double timing = 0;                 // 1: synchronous host-buffer operator calls record timing events too (device-pointer
                                       // launches always do).  Off by default: the two event records cost 3.5 us of a
                                       // 41 us single-profile call, and nothing is left on the stream when such a call
                                       // returns; prhf_last_kernel_ms keeps reporting the last launch that was timed
    double trim_lds = 1;               // columns of more than 1400 levels: stage only up to the highest peak of the launch and
                                       // stay on the LDS kernels when that fits (0: always the global-memory slabs)
    double short_compact = 1;          // short O-mode grids: four 4-wave workgroups per CU whose staged arrays hold as many
                                       // levels as a quarter of the LDS allows; a profile whose peak lies higher goes to a
                                       // second launch with full-size arrays (0: two 8-wave workgroups per CU only)
    double short_prio = 4;             // short-grid O kernel, bits: wave priority of a block's items by age (1: the blocks of the last
                                       // three resident rounds rank below everything pulled before them - config 3 -2.7 %),
                                       // by cost (2: a profile with many reflecting frequencies outranks its neighbours), both (3);
                                       // by phase (4, the default since round 5: staging, lists, the queue and the final sums -
                                       // latency chains of few instructions - run above every main loop of the CU, whose other
                                       // workgroups' loops fill the issue slots: config 3 -1.5 %, the O/200 slice of config 5
                                       // -1.8 % against 1; with the age rule on top, 5: -1.9 % / +1.4 %)
    double short_order = 1;            // long short-grid O launches draw their blocks in descending order of a cost estimate
                                       // (a pre-pass over sixteen samples of every density column; 0: index order)
    double short_lanes = 0;            // short-grid O kernel: lanes per pair, 16 (four pairs per work item) or 8 (eight: half the
                                       // items and their set-up per profile, no half-empty last wave-iteration on 200 points;
                                       // but eight pairs' nodes per LDS read: more bank conflicts).  0: eight on grids of up
                                       // to 256 points, sixteen beyond (measured: -12 % at 50 points, -4 % at 200, -1 % at 256,
                                       // +1 % at 400, +22 % at 1000)
    double host_slabs = 3;             // large host-buffer batches are uploaded, evaluated and returned in this many slabs of
                                       // profiles (10 % / 30 % / 60 %) so that the transfers of one overlap the kernel of
                                       // another (1: one upload, one launch, one download)
    double local_chunks = 1;           // few-pair launches: a pair's chunks are waves of ONE workgroup, which adds them up
                                       // itself (0: chunks anywhere in the launch, sums through scratch + vfo_finalize_kernel)
    double tall_lean = 1;              // profiles staged in global memory (more than 1400 levels below the highest peak): the
                                       // main loop on the slab's nodes (0: the generic loop)
    double snell_table = 4;            // tracers: the frequency-independent parts of every level's mu, mu' (f_N^2, g_p |B|,
                                       // sin psi, cos psi) once per profile when the rays (groups) number at least this
                                       // many times the profiles - a ray stops at its turning point, after a third to a
                                       // half of the column, the table covers all of it - and the table stays under
                                       // 1 GiB (0: never; values do not depend on it)
    double strided_top = 1;            // X mode, fast tier, whole pairs of at least 8192 points on the reference's stretch:
                                       // the top segments are summed from every eighth point plus end corrections
                                       // (0: every point, the launch of before bit for bit)
    double strided_lower = 1;          // ... and on a uniform altitude grid the segments of at least
                                       // PRHF_STRIDED_MIN_SEGMENT points below those three as well, in one strided pass
                                       // and one pass over the segment boundaries (0: the launch of strided_top alone,
                                       // bit for bit; strided_top = 0 switches both off)
    double panel_lower = 1;            // ... and where strided_lower applies, the region below the top three segments is cut
                                       // at every segment's first point, a segment's run into pieces of at most
                                       // PRHF_PANEL_BLOCK points, each summed from nodes at real-valued indices (DESIGN.md 4.1;
                                       // a pair with a piece too close to X + Y = 1 keeps strided_lower's sum; 0: the launch
                                       // of before, bit for bit)
    double panel_nodes = 4;            // ... every piece from the four nodes of the Gauss rule of the counting measure on four
                                       // lanes, sixteen per wave-iteration; the pieces of a run whose segment's continuation
                                       // reaches X + Y = 1 within 16 piece lengths are halved until it does not, or until
                                       // they hold at most four points (8, or anything but 4: no halving,
                                       // eight Gauss-Legendre nodes on eight lanes for every piece - the same cuts and the
                                       // same guard, not the bits of the launch before the cuts changed)
    double panel_upper = 1;            // ... and the region of the panel sum ends at the top segment's first point, not at the
                                       // third segment's from the top, in every pair whose runs from the third segment below
                                       // the top one upwards pass the tests of the panel sum's runs; the other pairs keep the lower region and
                                       // the strided sums of those two segments (0: the launch of before, bit
                                       // for bit)
    double panel_quick = 1;            // ... and a list of the panel sum's runs whose every run passes a bound from 1 - X - Y at
                                       // its segment's two levels - X + Y = 1 at least 16 L + 10 indices beyond the run,
                                       // both levels at 1e-3 or more - skips the runs' exact tests, which would find
                                       // nothing (0: the exact tests for every list; values never depend
                                       // on it)
    double strided_grade = 1;          // ... and the strided stretch of each of the top three segments is cut into zones:
                                       // every 32nd point at least 1024 indices below the index where the segment's
                                       // continuation reaches X + Y = 1 and where 1 - X - Y >= 1.6e-4, every 16th at
                                       // least 512 below it and where 1 - X - Y >= 1e-5, in multiples of 2048 and 1024
                                       // indices (whole wave-iterations), every eighth next to it as before (DESIGN.md
                                       // 4.1; 0: every eighth point throughout, the launch of before, bit for bit)
    double pair_plan = 1;              // ... and the integers that steer such a pair's sum - first points of the top three
                                       // segments, the strided stretch of each - are computed once per pair, by one thread
                                       // while the workgroup makes its candidate list, instead of by all 64 lanes of the
                                       // pair's wave (0: the launch of before, bit for bit; values never
                                       // depend on it)
    double pair_plan_cap = 0;          // > 0: a workgroup keeps at most this many plans, the other pairs plan themselves (tests)
    double stream_blocks = 1;          // a persistent launch of one X-mode fast-tier slice whose workgroups settle reflection
                                       // heights per thread (what slice_plans_pairs asks of the shape) and whose staged
                                       // profile fits half of a CU's LDS takes the streaming form: one 16-wave workgroup
                                       // per CU with two slots, the next profile staged by one wave beside the sums of the
                                       // current one, no barrier per profile (vfo_stream_kernel).  0: the
                                       // launch of before, instruction for instruction; 2: also a launch of fewer blocks
                                       // than resident slots (tests).  Values never depend on it
    double stream_grid = 0;            // > 0: the streaming form launches at most this many workgroups (tests, A/B runs)
};
struct KnobName {
    const char* name;
    double Knobs::*field;
    double lo, hi;
};
const KnobName kKnobNames[] = {
    {"target_waves", &Knobs::target_waves, 64, 1e9},
    {"lean_min_points", &Knobs::lean_min_points, 2, 1e9},
    {"well_conditioned", &Knobs::well_conditioned, 0, 1},
    {"thread_scan_min", &Knobs::thread_scan_min, 0, 1e300},
    {"no_candidates", &Knobs::no_candidates, 0, 1},
    {"persistent", &Knobs::persistent, 0, 1},
    {"tail_rounds", &Knobs::tail_rounds, 0, 1e6},
    {"tail_bpp", &Knobs::tail_bpp, 1, 64},
    {"split_min_points", &Knobs::split_min_points, 1, 1e9},
    {"split_few_profiles", &Knobs::split_few_profiles, 0, 1},
    {"short_kernel", &Knobs::short_kernel, 0, 1},
    {"shortx_kernel", &Knobs::shortx_kernel, 0, 1},
    {"short_concurrent", &Knobs::short_concurrent, 0, 1},
    {"short_queue", &Knobs::short_queue, 0, PRHF_SHORT_MAX_QUEUE},
    {"local_chunks", &Knobs::local_chunks, 0, 1},
    {"direct_upload", &Knobs::direct_upload, 0, 1},
    {"timing", &Knobs::timing, 0, 1},
    {"trim_lds", &Knobs::trim_lds, 0, 1},
    {"short_compact", &Knobs::short_compact, 0, 1},
    {"short_prio", &Knobs::short_prio, 0, 7},
    {"host_slabs", &Knobs::host_slabs, 1, 3},
    {"short_order", &Knobs::short_order, 0, 1},
    {"short_lanes", &Knobs::short_lanes, 0, 16},
    {"snell_table", &Knobs::snell_table, 0, 1e9},
    {"tall_lean", &Knobs::tall_lean, 0, 1},
    {"strided_top", &Knobs::strided_top, 0, 1},
    {"strided_lower", &Knobs::strided_lower, 0, 1},
    {"panel_lower", &Knobs::panel_lower, 0, 1},
    {"panel_nodes", &Knobs::panel_nodes, 4, 8},
    {"panel_upper", &Knobs::panel_upper, 0, 1},
    {"panel_quick", &Knobs::panel_quick, 0, 1},
    {"strided_grade", &Knobs::strided_grade, 0, 1},
    {"pair_plan", &Knobs::pair_plan, 0, 1},
    {"pair_plan_cap", &Knobs::pair_plan_cap, 0, 1024},
    {"stream_blocks", &Knobs::stream_blocks, 0, 2},
    {"stream_grid", &Knobs::stream_grid, 0, 65536},
};
constexpr int kWavesPerBlock = PRHF_BLOCK_THREADS / 64;

// Decompose one slice into wave-sized items and blocks ("Launch geometry").
inline void plan_slice(prhf::SegDev& s, long long n_freq, long long wg_slots, const Knobs& kn) {
    const long long kTargetWaves = (long long)kn.target_waves;
    const bool kSplitFewProfiles = kn.split_few_profiles != 0;
    const long long kSplitMinPoints = (long long)kn.split_min_points;
    const double kTailRounds = kn.tail_rounds;
    const int kTailBpp = (int)kn.tail_bpp;
    const long long P = s.prof_end - s.prof_begin;
    const long long pairs = P * n_freq;
    const long long N = s.n_points;
    long long chunks = 1, chunk_len = ((N + 63) / 64) * 64;
    if (pairs > 0 && pairs < kTargetWaves && N > 256) {
        long long want = std::min((kTargetWaves + pairs - 1) / pairs, (N + 255) / 256);
        chunk_len = (((N + want - 1) / want + 63) / 64) * 64;
        chunks = (N + chunk_len - 1) / chunk_len;
    }
    s.slots = 0;
    if (chunks > 1 && kn.local_chunks != 0) {
        // Block-local chunks: S = 2, 4 or 8 slots per pair (the power of two at or below what the waves target asks
        // for), the pair's <= S chunks on consecutive waves of one workgroup, 8 / S pairs per workgroup.  One profile x
        // 174 frequencies x 20000 points: 174 workgroups of 8 chunks instead of 501 workgroups + a second kernel.
        long long want = std::min<long long>(std::min((kTargetWaves + pairs - 1) / pairs, (N + 255) / 256), kWavesPerBlock);
        long long S = 1;
        while (S * 2 <= want) S *= 2;
        if (S > 1) {
            chunk_len = (((N + S - 1) / S + 63) / 64) * 64;
            chunks = (N + chunk_len - 1) / chunk_len;          // <= S
            s.slots = (int)S;
        }
    }
    s.chunks = (int)chunks;
    s.chunk_len = (int)chunk_len;
    if (s.slots > 0) {
        s.blocks_per_prof = (int)((n_freq * s.slots + kWavesPerBlock - 1) / kWavesPerBlock);
        s.tail_prof = P;
        s.tail_bpp = s.blocks_per_prof;
        return;
    }
    const long long items = n_freq * chunks;
    long long waves = std::max<long long>(1, std::min(items, (kTargetWaves + std::max<long long>(P, 1) - 1) /
                                                                 std::max<long long>(P, 1)));
    s.blocks_per_prof = (int)((waves + kWavesPerBlock - 1) / kWavesPerBlock);
    // A long slice with few profiles - fewer than four resident rounds of one-workgroup profiles - is a launch of one
    // or two rounds whose last one is mostly empty slots (625 profiles of 20000 points on 512 slots: 7.8 ms for
    // 4.4 ms of work, tools/slice_cost5.py).  Cut every profile of such a slice into several workgroups (up to 32), each
    // with its share of the frequencies (it stages the profile again: ~13 us against milliseconds of items).
    if (kSplitFewProfiles && chunks == 1 && N >= kSplitMinPoints && P > 0 && P * s.blocks_per_prof < 4 * wg_slots) {
        long long bpp = std::min<long long>(32, (4 * wg_slots + P - 1) / P);
        while (bpp > 1 && items < bpp * kWavesPerBlock * 2) --bpp;     // at least two items per wave
        if (bpp > s.blocks_per_prof) s.blocks_per_prof = (int)bpp;
    }
    // A long slice of one-workgroup profiles ends on whole workgroups (milliseconds each at n_points = 20000)
    // while most of the chip has already drained.  Cut the profiles of the last kTailRounds rounds of
    // workgroup slots into kTailBpp workgroups each: the launch then drains in a fraction of a workgroup time.
    s.tail_prof = P;
    s.tail_bpp = s.blocks_per_prof;
    const long long tail = (long long)(kTailRounds * (double)wg_slots);
    if (kTailBpp > 1 && s.blocks_per_prof == 1 && chunks == 1 && N >= 1024 && P >= 4 * tail && tail > 0 &&
        n_freq >= (long long)kTailBpp * kWavesPerBlock) {
        s.tail_prof = P - tail;
        s.tail_bpp = kTailBpp;
    }
}

// Does a slice take the planning pass (SegDev::pair_plan)?  Only where the strided sum is on (a piece of the strided
// table: X mode, fast tier, whole pairs of at least PRHF_TOP3_MIN_POINTS points, profiles staged in LDS) and a workgroup
// settles its reflection heights one frequency per thread (one round of frequencies that fits the staged arrays); the
// plan's fields are 16 bits wide.  Tall and chunked slices never do.
inline bool slice_plans_pairs(const prhf::SegDev& s, bool tall, long long n_freq, long long lds_levels, const Knobs& kn) {
    return kn.pair_plan != 0 && !tall && s.sp_off > 0 && s.chunks == 1 && s.slots == 0 && s.lean != 0 && s.tier == 1 &&
           s.mode == PRHF_KMODE_X && s.thread_scan != 0 && kn.no_candidates == 0 && n_freq <= PRHF_BLOCK_THREADS &&
           n_freq <= lds_levels && s.n_points >= PRHF_TOP3_MIN_POINTS && s.n_points < 65536;
}

// The stretched grid must not decrease (smooth_nonuniform_grid never does): the top-segment search of the main loop
// relies on it.  Returns the first index i with mult[i] < mult[i - 1] inside a slice's range, -1 when there is none
// (ranges that do not lie inside the array are validate_work_list's to report).
inline long long first_decreasing_grid_entry(const double* mult, int64_t mult_len, const prhf_segment* segs, int32_t n_segs) {
    for (int32_t g = 0; g < n_segs; ++g)
        if (segs[g].mult_offset >= 0 && segs[g].n_points >= 1 && segs[g].mult_offset + segs[g].n_points <= mult_len)
            for (int64_t i = segs[g].mult_offset + 1; i < segs[g].mult_offset + segs[g].n_points; ++i)
                if (mult[i] < mult[i - 1]) return (long long)i;
    return -1;
}

// The caller's work list against the shapes of its arrays (include/prhf.h, prhf_vfo_worklist_f64): profile ranges inside
// [0, n_prof], a mode, a grid of at least one point that lies inside the multiplier array, output rows that start on
// a row boundary and that no two slices share.  PRHF_OK, or PRHF_EINVAL with the reason in `msg`.
inline int validate_work_list(const prhf_segment* segs, int32_t n_segs, int64_t n_prof, int64_t n_freq, int64_t mult_len,
                              char* msg, size_t msg_len) {
    for (int i = 0; i < n_segs; ++i) {
        const prhf_segment& u = segs[i];
        if (u.prof_begin < 0 || u.prof_end < u.prof_begin || u.prof_end > n_prof) {
            std::snprintf(msg, msg_len, "segment %d: profile range outside [0, n_prof]", i);
            return PRHF_EINVAL;
        }
        if (u.mode != PRHF_MODE_O && u.mode != PRHF_MODE_X) {
            std::snprintf(msg, msg_len, "mode must be 'O' or 'X'");
            return PRHF_EINVAL;
        }
        if (u.n_points < 1) {
            std::snprintf(msg, msg_len, "n_points must be >= 1");
            return PRHF_EINVAL;
        }
        if (u.mult_offset < 0 || u.mult_offset + u.n_points > mult_len) {
            std::snprintf(msg, msg_len, "segment %d: multiplier range outside the array", i);
            return PRHF_EINVAL;
        }
        if (u.out_offset < 0 || u.out_offset % n_freq != 0) {
            std::snprintf(msg, msg_len, "segment %d: output offset must be a non-negative multiple of n_freq", i);
            return PRHF_EINVAL;
        }
        for (int k = 0; k < i; ++k) {          // rows [out_offset / n_freq, + profiles) of two segments must not overlap
            const long long a0 = segs[k].out_offset / n_freq, a1 = a0 + (segs[k].prof_end - segs[k].prof_begin);
            const long long b0 = u.out_offset / n_freq, b1 = b0 + (u.prof_end - u.prof_begin);
            if (a0 < b1 && b0 < a1 && a0 < a1 && b0 < b1) {
                std::snprintf(msg, msg_len, "segments %d and %d write the same output rows", k, i);
                return PRHF_EINVAL;
            }
        }
    }
    return PRHF_OK;
}

// The control words of a context (prhf_ctx::d_status, kStatusWords device words).  A persistent launch counts the blocks
// it has handed out in its queue word, which must be zero when the launch starts; every launch of one operator call
// has a word of its own, because they may run side by side.
enum StatusWord : int {
    kWordShortOFull = 0,      // short-grid O: the second launch, with full-size arrays
    kWordGeneral = 1,         // the general launch (vfo_kernel, vfo_tall_kernel)
    kWordShortO = 2,          // short-grid O: the first launch
    kWordShortOFollow = 3,    // ... and the general kernel over the profiles it left
    kWordShortX = 4,          // short-grid X: the first launch
    kWordShortXFollow = 5,    // ... and the general kernel over the profiles it left
    kLaunchQueueWords = 6,    // words [0, this) are zeroed in one piece in front of a launch with a queue
    kWordRayQueue = 6,        // kept for the tracers (their per-ray launch now keeps its queue behind the per-profile scalars)
    kWordPeak = 7,            // the peak pre-pass of a tall column: the highest peak index (launch_peak_levels)
    kWordShortXFull = 8,      // short-grid X: the second launch, with full-size arrays
    kStatusWords = 12,
};

// LDS of one CU and the budgets of a short-grid workgroup: two per CU where its nodes allow that, else one, or - the
// compact geometry - PRHF_COMPACT_WGS_PER_CU; a few hundred bytes of static LDS (tickets, counters) come on top.
#ifndef PRHF_COMPACT_RESERVE
#define PRHF_COMPACT_RESERVE 512    // bytes kept back per workgroup for its static LDS (tickets, counters)
#endif
constexpr size_t kLdsPerCu = 160 * 1024;
constexpr size_t kShortReserve = 512;
constexpr size_t kLdsHalf = kLdsPerCu / 2 - kShortReserve, kLdsFull = kLdsPerCu - kShortReserve;
constexpr size_t kLdsQuarter = kLdsPerCu / PRHF_COMPACT_WGS_PER_CU - PRHF_COMPACT_RESERVE;

// LDS of a workgroup that stages `levels` levels of a profile: the general kernel's launches, the regrid kernel's, and
// - at the most levels LDS holds - what the kernels are configured for.  The one name the API uses for it.
inline size_t staged_lds_bytes(long long levels) { return prhf::lds_bytes_for(levels); }

// Resident workgroups of a launch: LDS admits two per CU up to half of it each (less `reserve` bytes of static LDS), else one
inline long long resident_slots(int cu_count, size_t lds_bytes, size_t reserve) {
    return (long long)cu_count * (lds_bytes + reserve <= kLdsPerCu / 2 ? 2 : 1);
}

// The compact geometry of the short-grid kernels: four 4-wave workgroups per CU instead of two 8-wave
// ones - four independent profiles in flight per CU, so that one workgroup's staging and barrier waits are covered by
// three others' items (config 3: -10 %).  A quarter of the LDS holds the lists and fewer levels than the column has; a
// profile whose peak lies above them goes to a second launch with full-size arrays.  Taken when those arrays hold at
// least half of the column (PyIRI columns peak at 25 - 50 % of their height).  Returns the levels the compact arrays
// hold - the most for which lds_of(levels) fits a quarter of the LDS - or 0: no compact launch.
template <class LdsOf>
inline long long compact_levels_for(long long lds_levels, LdsOf lds_of) {
    long long L = lds_levels;
    while (L > 1 && lds_of(L) > kLdsQuarter) --L;
    return (2 * L >= lds_levels && L >= 8 && lds_of(L) <= kLdsQuarter) ? L : 0;
}

// The shape of one operator call, as far as the plan depends on it
struct LaunchShape {
    long long n_prof, n_freq, n_alt;
    long long lds_levels;     // levels the staged arrays have room for: n_alt, or the highest peak index of a tall column + 1
    bool tall;                // profiles staged in global memory (vfo_tall_kernel); decided by run()'s peak pre-pass
    long long mult_len;
    int cu_count;
    int math;                 // PRHF_MATH_*
};

// One launch of a short-grid kernel
struct ShortLaunch {
    long long lds_levels;     // levels its staged arrays hold (KArgs::lds_levels)
    int threads;              // PRHF_COMPACT_THREADS or PRHF_SHORT_THREADS
    int queue_entries;        // O mode: entries of the LDS queue of ill-conditioned points (X mode has none: 0)
    int short_queue;          // KArgs::short_queue: those entries, or - option short_queue - minus the fixed number
    size_t lds_bytes;
    long long slots;          // resident workgroups
    long long grid;           // workgroups launched: one per block, or `slots` persistent ones
    bool queue;               // ... which pull their blocks from a queue word
};

// The short-grid slices of one mode: vfo_short_kernel (O) / vfo_shortx_kernel (X) over one-profile blocks, a second
// launch with full-size arrays over the profiles the compact one left, and the general kernel over what both left
// (non-uniform altitude grid, fast-turning or vanishing field, negative density, peak at level 0 or 1, a sum that is
// not finite)
struct ShortKind {
    int n_segs;
    long long blocks;         // 0: nothing is launched
    ShortLaunch first;
    bool second;              // compact launch whose arrays hold fewer levels than the column: `full` follows
    ShortLaunch full;
    int lanes;                // O mode: lanes per pair (Knobs::short_lanes)
    long long follow_grid;    // the follow-up general launch: persistent workgroups that read their list from the device
    size_t list_bytes;        // each leftover list: a count and `blocks` block indices
    prhf::SegDev seg[PRHF_MAX_SEGMENTS];
};

// Everything one operator call decides before it touches the device
struct LaunchPlan {
    // the general launch (vfo_kernel<launch_tier> or vfo_tall_kernel): its slices, longest workgroups first
    int n_segs;
    bool tall;                // vfo_tall_kernel: profiles staged in global memory (LaunchShape::tall)
    int launch_tier;          // else vfo_kernel's: 0 faithful, 1 fast, 2 per slice
    long long blocks;
    long long wg_slots;       // resident workgroups
    long long grid;           // workgroups launched: `blocks`, or `wg_slots` persistent ones
    bool queue;               // ... which pull their blocks from kWordGeneral
    size_t lds_bytes;
    int no_candidates;        // KArgs::no_candidates
    long long partial_elems, altmin_elems;   // scratch of the chunked slices, in doubles
    long long out_rows;
    unsigned long long tall_stride;          // tall launch: bytes of one workgroup's slab, and the slabs
    long long tall_slabs;
    // tables
    bool want_pairs;          // a slice takes the main loop: the pair table
    long long table_entries;  // ... with the strided table's pieces behind it
    bool any_plan;            // a slice takes the planning pass (SegDev::pair_plan)
    bool freq_table;          // the per-frequency table is built; its kernel zeroes the control words on the way
    bool short_order;         // ... by short_order_kernel, which sorts the short-grid O launch's blocks by cost as well
    bool zero_queues;         // without that table: the queue words are zeroed by a memset
    bool forked;              // short-grid launches on the second stream, beside the general launch
    bool stream;              // the general launch takes the streaming form (vfo_stream_kernel; option stream_blocks):
    long long stream_grid;    // ... this many workgroups of PRHF_STREAM_THREADS, which pull their blocks from kWordGeneral,
    size_t stream_lds_bytes;  // ... with two slots of lds_bytes each,
    long long stream_blocks;  // ... over this many blocks: the slice's, with its tail cut into
    int stream_tail_bpp;      // ... this many blocks per profile (seg[0].tail_bpp and `blocks` stay the general kernel's)
    long long stream_tail_prof;
    prhf::StridedPieces pieces;
    prhf::SegDev seg[PRHF_MAX_SEGMENTS];
    ShortKind o, x;
};

// The one place that sizes a short-grid launch: `levels` staged levels in the compact or the full-size geometry,
// `queue_entries` of LDS queue (O mode), over `blocks` blocks - or over a device-side list of at most as many
inline ShortLaunch size_short_launch(bool xmode, bool compact, long long levels, int queue_entries, bool from_list,
                                     long long blocks, const LaunchShape& sh, const Knobs& kn) {
    ShortLaunch l;
    l.lds_levels = levels;
    l.threads = compact ? PRHF_COMPACT_THREADS : PRHF_SHORT_THREADS;
    l.queue_entries = xmode ? 0 : queue_entries;
    const int fixed = (int)kn.short_queue;
    l.short_queue = fixed > 0 && !xmode ? -std::min(fixed, queue_entries) : l.queue_entries;
    l.lds_bytes = xmode ? prhf::shortx_lds_bytes(levels, sh.n_freq)
                        : prhf::short_lds_fixed(levels, sh.n_freq, l.threads) + 8 * (size_t)queue_entries;
    l.slots = compact ? (long long)sh.cu_count * PRHF_COMPACT_WGS_PER_CU : resident_slots(sh.cu_count, l.lds_bytes, kShortReserve);
    l.queue = from_list || blocks > l.slots;
    l.grid = std::min(blocks, l.slots);
    return l;
}

// Number the blocks of one kind's slices and size its launches.  full_queue: queue entries of the full-size O geometry.
inline void plan_short_kind(ShortKind& k, bool xmode, int full_queue, long long wg_slots, const LaunchShape& sh, const Knobs& kn) {
    k.blocks = 0;
    for (int i = 0; i < k.n_segs; ++i) {
        k.seg[i].block_begin = k.blocks;
        k.blocks += k.seg[i].prof_end - k.seg[i].prof_begin;
    }
    k.second = false;
    k.lanes = 0;
    k.follow_grid = std::min(k.blocks, wg_slots);
    k.list_bytes = (size_t)(k.blocks + 1) * sizeof(unsigned);
    k.first = k.full = ShortLaunch();
    if (k.blocks == 0) return;
    long long compact = 0;
    int compact_queue = 0;
    if (kn.short_compact != 0) {
        if (xmode) {
            compact = compact_levels_for(sh.lds_levels, [&](long long L) { return prhf::shortx_lds_bytes(L, sh.n_freq); });
        } else {
            compact = compact_levels_for(sh.lds_levels, [&](long long L) {
                return prhf::short_lds_fixed(L, sh.n_freq, PRHF_COMPACT_THREADS) + 8 * PRHF_COMPACT_MIN_QUEUE;
            });
            if (compact) compact_queue = prhf::short_queue_entries(compact, sh.n_freq, kLdsQuarter, PRHF_COMPACT_THREADS);
        }
    }
    k.first = size_short_launch(xmode, compact > 0, compact ? compact : sh.lds_levels, compact ? compact_queue : full_queue,
                                false, k.blocks, sh, kn);
    k.second = compact > 0 && compact < sh.lds_levels;        // some bottomsides may not fit the compact arrays
    if (k.second) k.full = size_short_launch(xmode, false, sh.lds_levels, full_queue, true, k.blocks, sh, kn);
    if (!xmode) {
        // lanes per pair: eight on grids of up to 256 points (the launch's longest), sixteen beyond (Knobs::short_lanes)
        int longest = 0;
        for (int i = 0; i < k.n_segs; ++i) longest = std::max(longest, k.seg[i].n_points);
        k.lanes = kn.short_lanes == 0 ? (longest <= 256 ? 8 : 16) : (kn.short_lanes < 12 ? 8 : 16);
    }
}

// Plan one operator call ("Launch geometry"): PRHF_OK and the plan in `pl`, or PRHF_EINVAL with the
// reason in `msg`.  Nothing is allocated; of the plan's slice arrays only the entries in use are written.
inline int plan_launch(const LaunchShape& sh, const prhf_segment* segs, int32_t n_user_segs, const Knobs& kn, LaunchPlan& pl,
                       char* msg, size_t msg_len) {
    const long long n_freq = sh.n_freq, n_prof = sh.n_prof, lds_levels = sh.lds_levels;
    const bool tall = sh.tall;
    const int kLeanMinPoints = (int)kn.lean_min_points;
    const bool kNoCandidates = kn.no_candidates != 0, kPersistent = kn.persistent != 0;
    if (validate_work_list(segs, n_user_segs, n_prof, n_freq, sh.mult_len, msg, msg_len) != PRHF_OK) return PRHF_EINVAL;
    // (a tall launch keeps its profile in a slab of global memory: its LDS always admits two workgroups per CU)
    pl.tall = tall;
    pl.lds_bytes = tall ? prhf::lds_bytes_tall() : staged_lds_bytes(lds_levels);
    pl.wg_slots = resident_slots(sh.cu_count, pl.lds_bytes, 0);
    // queue entries of a full-size short-grid O workgroup (0: the kernel cannot run)
    const size_t short_budget = prhf::short_queue_entries(lds_levels, n_freq, kLdsHalf, PRHF_SHORT_THREADS) ? kLdsHalf : kLdsFull;
    const int full_queue = prhf::short_queue_entries(lds_levels, n_freq, short_budget, PRHF_SHORT_THREADS);

    pl.n_segs = pl.o.n_segs = pl.x.n_segs = 0;
    pl.want_pairs = false;
    pl.out_rows = 0;
    for (int i = 0; i < n_user_segs; ++i) {
        const prhf_segment& u = segs[i];
        prhf::SegDev s;
        std::memset(&s, 0, sizeof s);
        s.prof_begin = u.prof_begin;
        s.prof_end = u.prof_end;
        s.mult_off = u.mult_offset;
        s.out_off = u.out_offset;
        s.mode = u.mode == PRHF_MODE_O ? PRHF_KMODE_O : PRHF_KMODE_X;
        s.n_points = u.n_points;
        s.tier = sh.math == PRHF_MATH_AUTO ? (u.mode == PRHF_MODE_O ? 0 : 1) : (sh.math == PRHF_MATH_FAST ? 1 : 0);
        // AUTO, O mode: the reference's operation order where it decides the answer (1 - X <= well_conditioned = 1e-5), the
        // reduced algebra elsewhere; PRHF_MATH_FAITHFUL keeps the reference's order everywhere
        s.well_conditioned = (sh.math == PRHF_MATH_AUTO && s.tier == 0) ? kn.well_conditioned : HUGE_VAL;
        // the main loop needs the pair table: one more (small) kernel unless the caller's grid is cached - not
        // worth it for a handful of pairs on a short grid, where the launch itself is the cost
        const long long seg_pairs = (u.prof_end - u.prof_begin) * n_freq;
        // (decided from the slice's shape alone: host and device callers must get the same arithmetic)
        const bool table_is_cheap = seg_pairs >= 4096 || u.n_points >= 2048;
        // (a profile staged in global memory - `tall` - takes the main loop too: it reads the nodes from the workgroup's
        //  slab through a buffer resource, NodeSpace<true>; option tall_lean = 0: the generic loop, as up to round 4)
        s.lean = ((!tall || kn.tall_lean != 0) && (s.tier == 1 || s.well_conditioned < 1.0) && u.n_points >= kLeanMinPoints &&
                  seg_pairs > 0 && table_is_cheap) ? 1 : 0;
        s.thread_scan = (!tall && (double)n_freq * (double)u.n_points >= kn.thread_scan_min) ? 1 : 0;
        plan_slice(s, n_freq, pl.wg_slots, kn);
        pl.out_rows = std::max<long long>(pl.out_rows, u.out_offset / n_freq + (u.prof_end - u.prof_begin));
        // Slices of short grids leave for a launch of their own.  The short-grid kernels read the per-frequency table
        // (launches of >= 4096 pairs) and list at most PRHF_MAX_CAND frequencies per profile
        // (grids shorter than the general kernel's main loop takes - lean_min_points - are theirs too: the pair
        //  table is built for them)
        const bool table = !tall && (s.lean || (seg_pairs >= 4096 && s.n_points < kLeanMinPoints));
        const bool fits_short = table && s.chunks == 1 && s.n_points >= PRHF_SHORT_MIN_POINTS && n_freq <= PRHF_MAX_CAND &&
                                n_prof * n_freq >= 4096 && !kNoCandidates;
        const bool is_short = kn.short_kernel != 0 && fits_short && s.tier == 0 && s.well_conditioned < 1.0 &&
                              s.n_points <= PRHF_SHORT_MAX_POINTS && full_queue > 0;
        // ... and its X-mode variant (fast tier, reflection heights per thread, no top-segment phase)
        const bool is_shortx = kn.shortx_kernel != 0 && fits_short && s.tier == 1 && s.mode == PRHF_KMODE_X &&
                               s.n_points <= PRHF_SHORTX_MAX_POINTS && s.thread_scan &&
                               prhf::shortx_lds_bytes(lds_levels, n_freq) <= kLdsFull;
        if (is_short || is_shortx) {
            ShortKind& k = is_short ? pl.o : pl.x;
            prhf::SegDev& t = k.seg[k.n_segs++];
            t = s;
            t.lean = 1;
            t.blocks_per_prof = 1;
            t.tail_prof = t.prof_end - t.prof_begin;
            t.tail_bpp = 1;
            pl.want_pairs = true;
        } else {
            pl.want_pairs = pl.want_pairs || s.lean != 0;
            pl.seg[pl.n_segs++] = s;
        }
    }
    pl.launch_tier = 0;
    for (int i = 0; i < pl.n_segs; ++i) pl.launch_tier = (i == 0 || pl.launch_tier == pl.seg[i].tier) ? pl.seg[i].tier : 2;
    // Workgroups are dispatched roughly in index order: give the slices with the most work per workgroup
    // the lowest indices so that a mixed launch does not end on its longest workgroups.  (A stable insertion sort: at
    // most PRHF_MAX_SEGMENTS entries, and nothing is allocated.)
    auto cost = [](const prhf::SegDev& s) {
        const double per_point = s.tier == 1 ? 1.0 : (s.well_conditioned < 1.0 ? 1.8 : 3.5);
        return (double)s.n_points / s.chunks / s.blocks_per_prof * per_point;   // head workgroups
    };
    for (int i = 1; i < pl.n_segs; ++i)
        for (int k = i; k > 0 && cost(pl.seg[k]) > cost(pl.seg[k - 1]); --k) std::swap(pl.seg[k], pl.seg[k - 1]);
    pl.blocks = pl.partial_elems = pl.altmin_elems = 0;
    for (int i = 0; i < pl.n_segs; ++i) {
        prhf::SegDev& s = pl.seg[i];
        const long long P = s.prof_end - s.prof_begin;
        s.prio = std::max(0, 3 - i);               // (sorted: the slice with the longest workgroups first)
        s.block_begin = pl.blocks;
        pl.blocks += s.tail_prof * s.blocks_per_prof + (P - s.tail_prof) * s.tail_bpp;
        if (s.chunks > 1 && s.slots == 0) {
            s.partial_off = pl.partial_elems;
            s.altmin_off = pl.altmin_elems;
            pl.partial_elems += P * n_freq * s.chunks;
            pl.altmin_elems += P;
        }
    }
    // persistent workgroups pulling blocks from a queue (vfo_kernel) once the launch has more blocks than slots
    pl.queue = (kPersistent || tall) && pl.blocks > pl.wg_slots;
    pl.grid = pl.queue ? pl.wg_slots : pl.blocks;
    pl.no_candidates = kNoCandidates || tall;
    pl.tall_stride = tall && pl.blocks > 0 ? prhf::tall_slab_bytes(sh.n_alt) : 0;
    pl.tall_slabs = tall ? std::min(pl.blocks, pl.wg_slots) : 0;
    plan_short_kind(pl.x, true, full_queue, pl.wg_slots, sh, kn);
    plan_short_kind(pl.o, false, full_queue, pl.wg_slots, sh, kn);
    if (pl.blocks > 0x7fffffffLL || pl.o.blocks > 0x7fffffffLL || pl.x.blocks > 0x7fffffffLL) {
        std::snprintf(msg, msg_len, "launch too large");
        return PRHF_EINVAL;
    }

    // The strided table (option strided_top): one piece behind the pair table for every distinct grid of
    // the X-mode fast-tier slices that take whole pairs of at least PRHF_TOP3_MIN_POINTS points through the main loop.
    std::memset(&pl.pieces, 0, sizeof pl.pieces);
    pl.table_entries = sh.mult_len + PRHF_PAIR_PAD;
    pl.any_plan = false;                       // a slice takes the planning pass: it needs the candidate list
    if (pl.want_pairs && kn.strided_top != 0 && !tall) {
        prhf::StridedPieces& pieces = pl.pieces;
        for (int i = 0; i < pl.n_segs; ++i) {
            prhf::SegDev& s = pl.seg[i];
            if (!(s.lean && s.tier == 1 && s.mode == PRHF_KMODE_X && s.chunks == 1 && s.n_points >= PRHF_TOP3_MIN_POINTS)) continue;
            int p = 0;
            while (p < pieces.n && !(pieces.mult_off[p] == s.mult_off && pieces.n_points[p] == s.n_points)) ++p;
            if (p == pieces.n) {
                const long long len = prhf::strided_piece_entries(s.n_points);
                // (the main loop addresses the table through a 31-bit byte offset)
                if ((pl.table_entries + len) * 16 >= 0x7fffffffLL) continue;
                pieces.mult_off[p] = s.mult_off;
                pieces.n_points[p] = s.n_points;
                pieces.sp_off[p] = pl.table_entries;
                pl.table_entries += len;
                ++pieces.n;
            }
            s.sp_off = pieces.sp_off[p];
            s.strided_lower = kn.strided_lower != 0;
            s.panel_lower = s.strided_lower && kn.panel_lower != 0;
            s.panel_nodes = s.panel_lower && kn.panel_nodes == 4 ? 4 : 8;
            // (bit 1: option panel_quick.  The main loop's instance for panel_upper reads that option in bit 26 of the
            //  piece's offset from the slice's grid: a piece 2^26 entries - 1 GiB - or more away keeps the lower region)
            s.panel_upper = s.panel_lower && kn.panel_upper != 0 && s.sp_off - s.mult_off < (1LL << 26)
                                ? 1 | (kn.panel_quick != 0 ? 2 : 0) : 0;
            s.strided_grade = kn.strided_grade != 0;
            s.pair_plan = slice_plans_pairs(s, tall, n_freq, lds_levels, kn) ? 1 : 0;
            pl.any_plan = pl.any_plan || s.pair_plan != 0;
        }
    }
    // The streaming form (option stream_blocks): the launch is one slice, alone on the device - no
    // short-grid launch beside it - and persistent today (option 2: or would be with more blocks); the slice is what
    // slice_plans_pairs asks for, whatever option pair_plan says (without plans every pair plans itself, as in the
    // general kernel); two slots fit one workgroup's LDS.  One workgroup per CU; a launch of few blocks, fewer.
    pl.stream = false;
    pl.stream_grid = 0;
    pl.stream_lds_bytes = 0;
    pl.stream_blocks = 0;
    pl.stream_tail_bpp = 0;
    pl.stream_tail_prof = 0;
    if (kn.stream_blocks != 0 && kPersistent && !tall && pl.n_segs == 1 && pl.o.n_segs == 0 && pl.x.n_segs == 0 && pl.blocks > 0 &&
        (pl.queue || kn.stream_blocks == 2) && 2 * pl.lds_bytes <= kLdsFull) {
        Knobs with_plans = kn;
        with_plans.pair_plan = 1;
        if (slice_plans_pairs(pl.seg[0], tall, n_freq, lds_levels, with_plans)) {
            pl.stream = true;
            pl.queue = true;                   // (the queue word is zeroed and handed to the kernel)
            // The tail (plan_slice): a block of this form is summed by sixteen waves, not eight, and staged by ONE wave,
            // which takes three times as long as eight do.  Pieces of the general kernel's duration are half as many per
            // profile: with tail_bpp = 4 as it stands the CU's one stager was what the last round waited for (+3 %
            // against the general kernel), with 2 the form gains (profiles/ab_stream_blocks.txt).
            const prhf::SegDev& s = pl.seg[0];
            const long long P = s.prof_end - s.prof_begin;
            pl.stream_blocks = pl.blocks;
            pl.stream_tail_bpp = s.tail_bpp;
            pl.stream_tail_prof = s.tail_prof;
            if (s.tail_prof < P && s.tail_bpp > s.blocks_per_prof) {
                const int bpp = std::max(s.blocks_per_prof, s.tail_bpp / (PRHF_STREAM_THREADS / PRHF_BLOCK_THREADS));
                pl.stream_blocks -= (P - s.tail_prof) * (s.tail_bpp - bpp);
                pl.stream_tail_bpp = bpp;
                if (bpp == s.blocks_per_prof) pl.stream_tail_prof = P;
            }
            pl.stream_lds_bytes = 2 * pl.lds_bytes;
            pl.stream_grid = std::min<long long>(sh.cu_count, (pl.stream_blocks + 1) / 2);
            if (kn.stream_grid > 0) pl.stream_grid = std::min(pl.stream_grid, (long long)kn.stream_grid);
        }
    }
    // per-frequency scalars: long launches read them from a table instead of dividing once per pair (a short
    // launch - one profile - is latency bound: it does without the extra kernel)
    // (... and so does a launch with a slice that plans its pairs: the heights that pass starts from are settled with
    //  the candidate list, which reads the table.  By default such a slice has 4096 pairs anyway - fewer are chunked)
    pl.freq_table = pl.want_pairs && (n_prof * n_freq >= 4096 || pl.any_plan);
    // A short-grid O launch of four resident rounds and more draws its blocks in descending order of a cost
    // estimate: the kernel that sorts them makes the table as well (short_order_kernel)
    pl.short_order = pl.freq_table && pl.o.blocks > 0 && kn.short_order != 0 && pl.o.blocks >= 4 * pl.o.first.slots;
    const bool any_short = pl.o.n_segs > 0 || pl.x.n_segs > 0;
    pl.zero_queues = !pl.freq_table && (any_short || pl.queue);
    // A list with both kinds of slices: the general launch goes first, on the caller's stream, and takes every
    // workgroup slot; the short-grid launch runs on a second stream and its workgroups move in as the general
    // launch's persistent workgroups leave - its 30 - 100 us blocks fill the end of the launch, which otherwise drains
    // on a few long blocks.  (One after the other on one stream the config-5 shard took 8.04 ms, general kernel alone
    // 7.94 ms.)  A launch of one kind stays on the caller's stream.
    pl.forked = any_short && pl.blocks > 0 && kn.short_concurrent != 0;
    return PRHF_OK;
}

// The launch of the Jacobian / VJP kernels (prhf_vjp.inc): one workgroup per profile, the staged bottomside plus one
// (Jacobian) or two (VJP) rows of lds_levels doubles per wave that takes frequencies.  Four such waves where LDS holds
// their rows, else two, else one - and never more than there are frequencies; a bottomside that leaves no room for one
// wave's rows is refused (staging it in global memory, as vfo_tall_kernel does, is not implemented for the derivative).
// The bits of a VJP depend on the number of waves (the order its frequencies are added in): it changes only where
// the rows stop fitting, from vjp_max_levels(.., 4) levels on.
struct VjpPlan {
    long long blocks;
    int threads, waves;
    size_t lds_bytes;
};
inline long long vjp_max_levels(bool jacobian, int waves) {
    long long L = 1;
    while (prhf::vjp_lds_bytes(L + 1, waves, jacobian) <= kLdsFull) ++L;
    return L;
}
inline int plan_vjp(long long n_prof, long long n_freq, long long lds_levels, bool jacobian, VjpPlan& pl, char* why,
                    size_t why_len) {
    std::memset(&pl, 0, sizeof pl);
    if (n_prof < 0 || n_freq < 1 || lds_levels < 1) {
        std::snprintf(why, why_len, "bad shape");
        return PRHF_EINVAL;
    }
    int waves = PRHF_VJP_THREADS / 64;
    while (waves > 1 && (waves / 2 >= n_freq || prhf::vjp_lds_bytes(lds_levels, waves, jacobian) > kLdsFull)) waves /= 2;
    if (prhf::vjp_lds_bytes(lds_levels, waves, jacobian) > kLdsFull) {
        std::snprintf(why, why_len, "the %s stages at most %lld levels up to the density peak in LDS; this launch needs %lld "
                      "(tall bottomsides are not supported by the derivative kernels)", jacobian ? "Jacobian" : "VJP",
                      vjp_max_levels(jacobian, 1), lds_levels);
        return PRHF_EINVAL;
    }
    pl.blocks = n_prof;
    pl.threads = PRHF_VJP_THREADS;
    pl.waves = waves;
    pl.lds_bytes = prhf::vjp_lds_bytes(lds_levels, waves, jacobian);
    return PRHF_OK;
}

// The launches of the JVP kernel (prhf_jvp.inc): one workgroup per profile, the staged bottomside plus the tangent
// columns of one chunk.  Nothing in LDS is per wave, so every wave takes frequencies at every height (`waves`: those that
// get one), and a workgroup may as well have eight of them where there are frequencies for more than four: the LDS of a
// tall bottomside admits one or two workgroups per CU, and 512 threads then put twice the waves on its SIMDs
// (PRHF_JVP_WIDE = 0 builds keep 256, to measure against).  A result's bits do not depend on the workgroup's size.  The T tangents of a call go in chunks of `chunk` - 8 where LDS holds eight columns
// beside the bottomside (up to jvp_max_levels(8) = 908 levels), else 4, 2 or 1 - one launch per chunk, the last one with
// what remains, on the smallest instantiation that holds it (jvp_chunk).  A result's bits do not depend on the chunking.
// Limit: jvp_max_levels(1) = 1332 levels up to the highest density peak; beyond it the call is refused.
#ifndef PRHF_JVP_WIDE
#define PRHF_JVP_WIDE 1
#endif
struct JvpPlan {
    long long blocks;
    int threads, waves;
    int chunk;                // tangents of a full launch (= its instantiation's NT)
    long long n_chunks;       // launches
    long long lds_levels;
};
inline long long jvp_max_levels(int nt) {
    long long L = 1;
    while (prhf::jvp_lds_bytes(L + 1, nt) <= kLdsFull) ++L;
    return L;
}
inline int plan_jvp(long long n_prof, long long n_freq, long long lds_levels, long long n_tan, JvpPlan& pl, char* why,
                    size_t why_len) {
    std::memset(&pl, 0, sizeof pl);
    if (n_prof < 0 || n_freq < 1 || lds_levels < 1 || n_tan < 0) {
        std::snprintf(why, why_len, "bad shape");
        return PRHF_EINVAL;
    }
    int chunk = PRHF_JVP_MAX_NT;
    while (chunk > 1 && (chunk / 2 >= n_tan || prhf::jvp_lds_bytes(lds_levels, chunk) > kLdsFull)) chunk /= 2;
    if (prhf::jvp_lds_bytes(lds_levels, chunk) > kLdsFull) {
        std::snprintf(why, why_len, "the JVP stages at most %lld levels up to the density peak in LDS; this launch needs %lld "
                      "(tall bottomsides are not supported by the derivative kernels)", jvp_max_levels(1), lds_levels);
        return PRHF_EINVAL;
    }
    pl.blocks = n_prof;
    pl.threads = (PRHF_JVP_WIDE && n_freq > PRHF_VJP_THREADS / 64) ? PRHF_JVP_THREADS_WIDE : PRHF_VJP_THREADS;
    pl.waves = (int)std::min<long long>(pl.threads / 64, n_freq);
    pl.chunk = chunk;
    pl.n_chunks = (n_tan + chunk - 1) / chunk;
    pl.lds_levels = lds_levels;
    return PRHF_OK;
}
// Launch i of the plan: its first tangent, how many it takes, the instantiation (1, 2, 4, 8 >= count) and its LDS
struct JvpChunk {
    long long first;
    int count, nt;
    size_t lds_bytes;
};
inline JvpChunk jvp_chunk(const JvpPlan& pl, long long n_tan, long long i) {
    JvpChunk ch;
    ch.first = i * pl.chunk;
    ch.count = (int)std::min<long long>(pl.chunk, n_tan - ch.first);
    ch.nt = 1;
    while (ch.nt < ch.count) ch.nt *= 2;
    ch.lds_bytes = prhf::jvp_lds_bytes(pl.lds_levels, ch.nt);
    return ch;
}

}  // namespace

#endif  // PRHF_PLAN_H
