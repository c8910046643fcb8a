// prhf_kernels.h - launch interface between the C ABI (prhf_api.cpp) and the HIP kernels.
#ifndef PRHF_KERNELS_H
#define PRHF_KERNELS_H

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#define PRHF_KMODE_O 0
#define PRHF_KMODE_X 1

#define PRHF_STATUS_NEGDEN 0x1
#define PRHF_STATUS_PEAK0  0x2
#define PRHF_STATUS_BADINDEX 0x4    // a ray's profile_index outside [0, n_prof) (tracers)
#define PRHF_STATUS_BADFIELD 0x20   // a point's / ray's field index outside [0, n_fields) (prhf_gradient.inc)
#define PRHF_STATUS_PATHLEN 0x40    // a ray of the gradient tracer has more nodes than path_stride
#define PRHF_STATUS_WORDS 8         // one word of host-visible memory per status bit (post_status)
#define PRHF_STATUS_NANINPUT 0x10   // NaN in a profile's altitude column, or in |B| / psi below its peak
#define PRHF_STATUS_BADGROUP 0x8    // a ray's ray_group outside [0, n_groups) (grouped tracer launch)
#define PRHF_STATUS_STALL 0x80      // streaming launch: a wave waited for a slot of its workgroup beyond the bound and gave up

#ifndef PRHF_BLOCK_THREADS
#define PRHF_BLOCK_THREADS 512      // 8 wavefronts share one staged profile
#endif
#ifndef PRHF_SHORT_THREADS
#define PRHF_SHORT_THREADS 512      // workgroup of the short-grid kernels (vfo_short_kernel, vfo_shortx_kernel)
#endif
#ifndef PRHF_SHORT_WAVES_PER_SIMD
#define PRHF_SHORT_WAVES_PER_SIMD 4 // ... and the occupancy their register budget is set for
#endif
#define PRHF_STREAM_THREADS 1024    // the streaming form of the persistent launch: sixteen waves share two staged profiles
#define PRHF_HINT_BUCKETS 1024      // uint16 segment hints, 2 KiB of LDS (non-uniform altitude grids)
#define PRHF_MAX_CAND 1024          // uint16 list of the frequencies that may reflect, 2 KiB of LDS
#define PRHF_MAX_SEGMENTS 8
#define PRHF_RED_DOUBLES 160        // block-reduction scratch (9 rows x up to 16 waves) + per-profile scalars
#define PRHF_NODE_BYTES 96          // one staged bottomside level
#define PRHF_SNODE_BYTES 80         // ... of the short-grid kernel (20 dwords: conflict-free under ds_read_b128)
#define PRHF_SHORT_MIN_POINTS 2     // grids of 2 .. 1024 points in the default O-mode arithmetic: vfo_short_kernel
#define PRHF_SHORT_MAX_POINTS 1024  // (16 wave-iterations: one violation mask each, per wave)
#define PRHF_SHORTX_MAX_POINTS 1024  // X mode (fast tier) up to this many points: vfo_shortx_kernel (no top-segment phase;
                                    // measured against the general kernel: -38 % at 200 points, -21 % at 500, -7 % at 1000, +6 % at 2000)
#define PRHF_SHORT_MASKS 32         // violation masks a wave keeps per work item: wave-iterations of the item that hold
                                    // ill-conditioned points (more: every point of the item's pairs in the reference's order)
#define PRHF_SHORT_MAX_QUEUE 4096   // entries of the LDS queue of ill-conditioned points, at most
#define PRHF_ORDER_CLASSES 16       // cost classes of the short-grid launch's block order (short_order_kernel)
#ifndef PRHF_COMPACT_THREADS
#define PRHF_COMPACT_THREADS 256    // the compact geometry of the short-grid O kernel: four 4-wave workgroups per CU, staged
#endif
#ifndef PRHF_COMPACT_WGS_PER_CU
#define PRHF_COMPACT_WGS_PER_CU 4   // arrays for as many levels as a quarter of the LDS holds
#endif
#ifndef PRHF_COMPACT_MIN_QUEUE
#define PRHF_COMPACT_MIN_QUEUE 256  // queue entries such a workgroup has at least (a profile's unused nodes come on top)
#endif
#define PRHF_PAIR_PAD 256           // entries behind the pair table that the main loop's prefetch may touch (127; 63 x 4 = 252
                                    // behind a stride-32 zone of the strided table: static_assert in strided_run)
#ifndef PRHF_TOP_MIN_POINTS
#define PRHF_TOP_MIN_POINTS 1024    // grids from this many points on give their top segment a loop of its own
#endif
#ifndef PRHF_TOP3_MIN_POINTS
#define PRHF_TOP3_MIN_POINTS 8192   // ... and from this many on, the two segments below it as well
#endif
#ifndef PRHF_STRIDED_MIN_SEGMENT
#define PRHF_STRIDED_MIN_SEGMENT 64 // segments below the top three take the strided sum while they hold this many points
#endif
#ifndef PRHF_PANEL_BLOCK
#define PRHF_PANEL_BLOCK 128        // the panel sum below the top three segments cuts its region at every multiple of this (64 or 128)
#endif
#ifndef PRHF_PANEL_MIN_SEGMENT
#define PRHF_PANEL_MIN_SEGMENT 8    // ... and begins at the lowest segment that holds this many points
#endif
#ifndef PRHF_MIN_WAVES_PER_SIMD
#define PRHF_MIN_WAVES_PER_SIMD 4   // two 8-wave workgroups per CU: caps VGPRs at 128
#endif

namespace prhf {

// waves per SIMD the short-grid kernels' register budget is set for: the compact geometry keeps PRHF_COMPACT_WGS_PER_CU
// workgroups of `threads` per CU resident (256 threads: 4 x 4 waves = 4 per SIMD; 320: 5), the full-size one two of 512
constexpr int short_waves_per_simd(int threads) {
    return threads < PRHF_SHORT_THREADS && threads * PRHF_COMPACT_WGS_PER_CU / 256 > PRHF_SHORT_WAVES_PER_SIMD
               ? threads * PRHF_COMPACT_WGS_PER_CU / 256 : PRHF_SHORT_WAVES_PER_SIMD;
}

// One homogeneous slice of a launch, with its decomposition into blocks.
struct SegDev {
    long long prof_begin, prof_end;  // profile rows [begin, end)
    long long mult_off;              // first element of this slice's multiplier grid
    long long out_off;               // first element of this slice's output rows
    long long block_begin;           // first block index of this slice
    long long partial_off;           // chunk-sum scratch offset (chunks > 1)
    long long altmin_off;            // per-profile min(alt) scratch offset (chunks > 1)
    int mode, n_points;
    int chunks;                      // wave-sized work items per pair
    int chunk_len;                   // grid points per chunk (multiple of 64)
    int slots;                       // > 0: block-local chunks - a pair's chunks (<= slots, a power of two <= 8) are the
                                     // consecutive waves of ONE workgroup, which adds them up itself (run_items)
    int blocks_per_prof;
    int tier;                        // 0 faithful, 1 fast (read by the mixed-tier kernel)
    // The last profiles of a long slice may be cut into more, shorter workgroups so that the launch
    // drains quickly: profiles [tail_prof, P) of the slice use tail_bpp blocks each (tail_prof = P: none).
    long long tail_prof;
    int tail_bpp;
    int panel_upper;                 // with panel_lower (below): the panel sum's region reaches up to the top segment's first
                                     // point where the two segments below it pass the runs' tests (option panel_upper; it sits
                                     // here, in what was padding: the kernels' argument layout is the one of before).
                                     // Bit 1, set beside bit 0 only: a list of the panel sum whose runs all pass the quick
                                     // bound skips the runs' exact tests (option panel_quick)
    // Faithful tier only: where 1 - X exceeds this at all 64 points of a wave-iteration the reduced
    // algebra is used instead of the reference's operation order (+inf: never).
    double well_conditioned;
    int lean;                        // this slice uses the main loop (and KArgs::pairs); decided per slice so that a
                                     // slice gets the same arithmetic alone and inside a mixed launch
    int prio;                        // wave priority (0..3) of this slice's workgroups in a mixed launch: see vfo_kernel
    long long sp_off;                // > 0: this slice's piece of the strided table, in entries from KArgs::pairs
                                     // (launch_grid_strided; the main loop's strided sum); 0: none
    int strided_lower;               // with sp_off > 0: the segments below the top three take the strided sum too
                                     // (option strided_lower)
    int panel_lower;                 // with strided_lower: those segments are summed from eight nodes per piece where the
                                     // pair's guard allows it (option panel_lower)
    int panel_nodes;                 // with panel_lower: 4 - pieces far from X + Y = 1 take four nodes on four lanes; 8 - every
                                     // piece takes eight lanes (option panel_nodes)
    int strided_grade;               // with sp_off > 0: a strided stretch of the top three segments is cut into zones of
                                     // stride 32, 16 and 8 by the distance to X + Y = 1 (option strided_grade)
    int pair_plan;                   // with sp_off > 0: the workgroup plans its pairs' sums one pair per thread (option
                                     // pair_plan; plan_pairs in prhf_kernels.hip)
    int thread_scan;                 // X mode: reflection heights settled one frequency per thread while the candidate
                                     // list is made (on by default; PRHF_THREAD_SCAN_MIN turns it off for A/B runs.
                                     // O mode always does, by binary search)
};

// KArgs::plan_counters: seven words and one of padding, then kQuickSlots slots of kQuickSlotWords words (a cache line)
// whose first two words count the list passes of the panel sum that took the quick path and the exact tests; the
// host adds the slots up (prhf_panel_quick_counters)
constexpr int kQuickSlots = 64, kQuickSlotWords = 8, kQuickSlotBase = 8;
constexpr int kPlanCounterWords = kQuickSlotBase + kQuickSlots * kQuickSlotWords;

struct KArgs {
    const double* freq;
    const double* den;
    const double* bmag;
    const double* bpsi;
    const double* alt;
    const double* mult;
    const double* pairs;             // (m_i, m_i+1 - m_i) interleaved, same indexing as mult; may be null
    const double* ftab;              // (n_freq, 8) per-frequency scalars (freq_table_kernel); null: computed per pair
    double* out;
    double* partial;
    double* altmin;
    unsigned* status;
    unsigned* queue;                 // persistent launch: next block index - gridDim.x, zero at launch; null = one block per workgroup
    long long n_blocks;              // blocks of work in this launch
    unsigned long long* trace;       // -DPRHF_TRACE builds: (start, end) wall clock of every wave, else unused
    long long n_freq, n_alt, prof_stride, alt_stride;
    long long field_stride;          // row stride of bmag and bpsi: prof_stride, or 0 when one row serves every profile
    int n_segs;
    int no_candidates;               // PRHF_NO_CANDIDATES=1 (A/B runs): every frequency is a work item, none is pre-filtered
    // Short-grid launches (vfo_short_kernel) and their follow-up:
    unsigned* leftover;              // [0] count, [1..] block indices of the profiles the short-grid kernel does not take
    unsigned* leftover_tall;         // compact short-grid launch: ... of the profiles whose bottomside its staged arrays do not
                                     // hold (they go to the short-grid launch with full-size arrays); null: `leftover`
    const unsigned* block_list;      // follow-up launches: evaluate blocks block_list[1 .. block_list[0]] instead of 0 .. n_blocks
    int short_queue;                 // entries of the short-grid kernel's LDS queue
    int short_prio;                  // wave priorities of the short-grid O kernel's blocks (vfo_short_kernel)
    const unsigned* order;           // short-grid O launch: its blocks by cost class (short_order_kernel), or null: index order
    unsigned* zero_after;            // general kernel, follow-up of such a launch: the class counters to leave at zero (or null)
    // Profiles taller than LDS holds (vfo_tall_kernel): one slab of tall_stride bytes per workgroup of the launch
    unsigned char* tall;
    unsigned long long tall_stride;
    // Levels the staged arrays (nodes, f_N^2, g_p |B|) have room for: n_alt, or - a column of more than 1400 levels
    // whose bottomsides all fit LDS (launch_peak_levels) - the highest peak index of the launch + 1
    long long lds_levels;
    // The planning pass (SegDev::pair_plan): [0] pairs that ran from a plan, [1] eligible pairs that planned themselves;
    // plan_cap > 0 caps the records per workgroup (tests).  [2] pairs whose lower segments took the panel sum, [3] eligible
    // pairs that fell back (SegDev::panel_lower), [4] the pairs of [2] in slices with SegDev::panel_upper, [5] those of
    // them whose panel region stayed the lower one (the others' region reached the top segment), [6] the pairs of [0] whose
    // plan carries the panel region's set-up (the record's second form); from kQuickSlotBase the slots of the panel sum's
    // list passes in slices with SegDev::panel_upper - quick path (option panel_quick), exact tests.  A workgroup counts
    // in its LDS (WgCounts in prhf_kernels.hip) and adds its words here once, when it leaves the kernel: the words are
    // complete when the launch has finished.  Null: nothing is added
    unsigned long long* plan_counters;
    int plan_cap;
    SegDev seg[PRHF_MAX_SEGMENTS];
};

// n_alt + 1 nodes (the last one may be the +inf sentinel), f_N^2 and g_p*B per level,
// segment hints, candidate frequencies, block-reduction scratch
inline __host__ __device__ size_t lds_bytes_for(long long n_alt) {
    return (size_t)(n_alt + 1) * PRHF_NODE_BYTES + (size_t)n_alt * 16 + PRHF_HINT_BUCKETS * 2 + PRHF_MAX_CAND * 2 +
           PRHF_RED_DOUBLES * 8;
}

// ... of a tall launch (vfo_tall_kernel): hints, candidate list (unused), reduction scratch; the staged profile
// itself - the first two terms of lds_bytes_for - is a slab of global memory per workgroup
inline size_t lds_bytes_tall() { return PRHF_HINT_BUCKETS * 2 + PRHF_MAX_CAND * 2 + PRHF_RED_DOUBLES * 8; }
inline size_t tall_slab_bytes(long long n_alt) {
    return (((size_t)(n_alt + 1) * PRHF_NODE_BYTES + (size_t)n_alt * 16) + 255) & ~(size_t)255;
}

// LDS of one short-grid workgroup (vfo_short_kernel): the per-frequency lists and scratch in front, then n_alt + 1
// nodes, then `queue` entries of 8 bytes (a profile with K < n_alt levels adds its unused nodes to the queue).
inline __host__ __device__ size_t short_lds_lists(long long n_alt, long long n_freq, int threads) {
    const size_t b = (size_t)(n_alt > n_freq ? n_alt : n_freq) * 8 + (size_t)n_freq * 24 + (size_t)(threads / 64) * PRHF_SHORT_MASKS * 12 +
                     PRHF_RED_DOUBLES * 8 + (size_t)n_freq * 4 + (size_t)n_freq * 2;
    return (b + 15) & ~(size_t)15;
}
inline size_t short_lds_fixed(long long n_alt, long long n_freq, int threads) {
    return short_lds_lists(n_alt, n_freq, threads) + (size_t)(n_alt + 1) * PRHF_SNODE_BYTES;
}
// ... of the X-mode variant (vfo_shortx_kernel): no queue; f_N^2 and g_p |B| per level, three doubles and an index
// per frequency, scratch, nodes
inline __host__ __device__ size_t shortx_lds_lists(long long n_alt, long long n_freq) {
    const size_t b = (size_t)n_alt * 16 + (size_t)n_freq * 24 + PRHF_RED_DOUBLES * 8 + (size_t)n_freq * 2;
    return (b + 15) & ~(size_t)15;
}
inline size_t shortx_lds_bytes(long long n_alt, long long n_freq) {
    return shortx_lds_lists(n_alt, n_freq) + (size_t)(n_alt + 1) * PRHF_SNODE_BYTES;
}
// queue entries that fit `budget` bytes beside a full node table (0: the kernel cannot run)
inline int short_queue_entries(long long n_alt, long long n_freq, size_t budget, int threads) {
    const size_t fixed = short_lds_fixed(n_alt, n_freq, threads);
    if (fixed + 8 * 64 > budget) return 0;
    const size_t q = (budget - fixed) / 8;
    return (int)(q > PRHF_SHORT_MAX_QUEUE ? PRHF_SHORT_MAX_QUEUE : q);
}

hipError_t configure_kernels(size_t max_lds_bytes, size_t max_stream_lds_bytes);
hipError_t query_occupancy(int tier, size_t lds_bytes, int* blocks_per_cu);
// pairs[2 i], pairs[2 i + 1] = mult[i], mult[i + 1] - mult[i]; `pairs` holds n + PRHF_PAIR_PAD entries
hipError_t launch_grid_pairs(const double* mult, long long n, double* pairs, hipStream_t stream);
// The strided table's pieces (grid_strided_kernel): grid p is n_points[p] multipliers from mult + mult_off[p], its
// piece starts sp_off[p] entries into `pairs` and holds strided_piece_entries(n_points[p]) entries
struct StridedPieces {
    int n;
    int n_points[PRHF_MAX_SEGMENTS];
    long long mult_off[PRHF_MAX_SEGMENTS];
    long long sp_off[PRHF_MAX_SEGMENTS];
};
inline long long strided_piece_entries(long long n_points) { return 1 + ((n_points + 7) / 8 + 1) + PRHF_PAIR_PAD; }
hipError_t launch_grid_strided(const double* mult, double* pairs, const StridedPieces& pc, hipStream_t stream);
// tab[8 f ..] = f_hz, f2, cp^2/f2, (g_p/f)^2, 1/f2, 1/f_hz, 0, 0; row n_freq: min |freq_mhz| (tab holds n_freq + 1 rows)
// Control words that the per-frequency table's kernel zeroes on the way (its workgroup 0): the block queues and list
// heads of the launches that follow it on the stream.
struct ZeroWords {
    unsigned* p[8];
    int words[8];
    int n;
};
hipError_t launch_freq_table(const double* freq_mhz, long long n_freq, double* tab, const ZeroWords& zero, hipStream_t stream);
// tier: 0 faithful, 1 fast, 2 per slice (SegDev::tier)
// a.n_blocks blocks of work; with a.queue set the grid is `grid_blocks` persistent workgroups that pull
// block indices from the queue, else grid_blocks must equal a.n_blocks
hipError_t launch_vfo(const KArgs& a, long long grid_blocks, int tier, size_t lds_bytes, hipStream_t stream);
// the streaming form (vfo_stream_kernel): grid_blocks workgroups of PRHF_STREAM_THREADS, each with two slots of
// lds_bytes_for(a.lds_levels) bytes; a.queue set; one X-mode fast-tier slice of whole pairs (LaunchPlan::stream)
hipError_t launch_vfo_stream(const KArgs& a, long long grid_blocks, hipStream_t stream);
// profiles of more than 1400 levels: a.tall holds grid_blocks slabs of a.tall_stride >= tall_slab_bytes(n_alt) bytes
hipError_t launch_vfo_tall(const KArgs& a, long long grid_blocks, hipStream_t stream);
// *max_peak (one device word, zeroed by the caller) = the highest density-peak index - np.argmax, the first NaN
// ranking highest, exactly stage_profile's rule - over n_prof profiles: a column of more levels than LDS holds can
// still take the LDS kernels when every bottomside fits
hipError_t launch_peak_levels(const double* den, long long n_prof, long long n_alt, long long prof_stride,
                              unsigned* max_peak, hipStream_t stream);
// the short-grid kernel over a.n_blocks one-profile blocks (a.queue set: `grid_blocks` persistent workgroups);
// lds_bytes = short_lds_fixed + 8 a.short_queue; threads: PRHF_SHORT_THREADS or PRHF_COMPACT_THREADS
hipError_t launch_vfo_short(const KArgs& a, long long grid_blocks, size_t lds_bytes, int threads, int lanes, hipStream_t stream);
// the blocks of the short-grid launch `a` sorted into cost classes: order[0 .. CLASSES) counts (zero when the launch
// starts), then CLASSES lists of a.n_blocks entries; the same launch makes the per-frequency table `tab` of
// launch_freq_table and zeroes `zero`'s control words
hipError_t launch_short_order(const KArgs& a, unsigned* order, const double* freq_mhz, double* tab, const ZeroWords& zero,
                              hipStream_t stream);
// the X-mode variant; lds_bytes = shortx_lds_bytes(a.lds_levels, n_freq); threads: PRHF_SHORT_THREADS or PRHF_COMPACT_THREADS
hipError_t launch_vfo_shortx(const KArgs& a, long long grid_blocks, size_t lds_bytes, int threads, hipStream_t stream);
// absmax_scratch: 2 x u64 device words, absmax_host: 2 x u64 pinned host words
hipError_t launch_mu_mup(const double* X, const double* Y, const double* psi, long long n, int mode, int tier,
                         unsigned long long* absmax_scratch, unsigned long long* absmax_host,
                         double* mu, double* mup, hipStream_t stream);
hipError_t launch_find_vh(const double* X, const double* Y, const double* psi, const double* dh, long long n_rows,
                          long long n_cols, double alt_min, int mode, int tier,
                          unsigned long long* absmax_scratch, unsigned long long* absmax_host, double* vh,
                          hipStream_t stream);

// Standalone regrid of one profile (library.py:324-438); all pointers are device memory.
struct RegridArgs {
    const double* freq_hz;
    const double* den;
    const double* bmag;
    const double* bpsi;
    const double* alt;
    const double* mult;
    double* out_freq;
    double* out_den;
    double* out_bmag;
    double* out_bpsi;
    double* out_dist;
    double* out_alt;
    double* out_crit;
    long long* out_ind;
    unsigned* status;
    long long n_freq, n_alt;
    long long lds_levels;     // levels the staged arrays hold: n_alt, or - a taller column - its peak index + 1 (<= 1400)
    int n_points, mode;
};
hipError_t launch_regrid(const RegridArgs& a, size_t lds_bytes, hipStream_t stream);
// Derivative of the operator with respect to the density column (prhf_vjp.inc): Jacobian rows or the vector-Jacobian
// product, one workgroup of PRHF_VJP_THREADS per profile; all pointers are device memory.
#define PRHF_VJP_THREADS 256
struct VjpArgs {
    const double* freq;       // MHz, (n_freq)
    const double* den;
    const double* bmag;
    const double* bpsi;
    const double* alt;
    const double* mult;       // the stretched grid, (n_points)
    const double* grad_vh;    // VJP: upstream gradient (n_prof, n_freq); not read where a pair has no value
    double* out;              // Jacobian: (n_prof, n_freq, n_alt); VJP: (n_prof, n_alt)
    unsigned* status;
    long long n_prof, n_freq, n_alt;
    long long prof_stride, field_stride, alt_stride;
    long long lds_levels;     // levels the staged arrays hold (> every bottomside of the launch)
    int n_points, mode;       // PRHF_KMODE_*
    int waves;                // waves of the workgroup that take frequencies (each owns rows in LDS): 1, 2 or 4
};
// LDS of one workgroup: the operator's staged profile (without its candidate list), then per frequency-taking wave
// one row of lds_levels doubles (Jacobian) or two (VJP: the current row and the wave's accumulated product)
inline size_t vjp_lds_bytes(long long levels, int waves, bool jacobian) {
    return (size_t)(levels + 1) * PRHF_NODE_BYTES + (size_t)levels * 16 + PRHF_HINT_BUCKETS * 2 + PRHF_RED_DOUBLES * 8 +
           (size_t)waves * (jacobian ? 1 : 2) * (size_t)levels * 8;
}
hipError_t launch_vfo_vjp(const VjpArgs& a, bool jacobian, size_t lds_bytes, hipStream_t stream);
// Jacobian-vector product of the operator (prhf_jvp.inc): dvh[p, f, t] = sum_k J[p, f, k] tan[p, t, k] for up to
// PRHF_JVP_MAX_NT tangents per launch, one workgroup of PRHF_VJP_THREADS or PRHF_JVP_THREADS_WIDE per profile; all pointers
// are device memory.
#define PRHF_JVP_MAX_NT 8
#define PRHF_JVP_THREADS_WIDE 512
struct JvpArgs {
    const double* freq;       // MHz, (n_freq)
    const double* den;
    const double* bmag;
    const double* bpsi;
    const double* alt;
    const double* mult;       // the stretched grid, (n_points)
    const double* tan;        // the launch's first tangent: rows of n_alt doubles, tan_prof_stride between profiles (0: shared)
    double* out;              // the launch's first column of dvh (n_prof, n_freq, out_stride)
    unsigned* status;
    long long n_prof, n_freq, n_alt;
    long long prof_stride, field_stride, alt_stride, tan_prof_stride;
    long long out_stride;     // tangents of the whole call: doubles between two frequencies in dvh
    long long lds_levels;     // levels the staged arrays hold (> every bottomside of the launch)
    int n_points, mode;       // PRHF_KMODE_*
    int n_tan;                // tangents of this launch, 1 ... NT of the instantiation that runs
};
// LDS of one workgroup: the operator's staged profile (without its candidate list), then nt tangent columns of
// lds_levels doubles.  No per-wave rows: every wave takes frequencies whatever the bottomside's height.
inline size_t jvp_lds_bytes(long long levels, int nt) {
    return (size_t)(levels + 1) * PRHF_NODE_BYTES + (size_t)levels * 16 + PRHF_HINT_BUCKETS * 2 + PRHF_RED_DOUBLES * 8 +
           (size_t)nt * (size_t)levels * 8;
}
// nt: accumulators per lane of the instantiation, 1, 2, 4 or 8 (>= a.n_tan); threads: PRHF_VJP_THREADS or PRHF_JVP_THREADS_WIDE
hipError_t launch_vfo_jvp(const JvpArgs& a, int nt, int threads, size_t lds_bytes, hipStream_t stream);
// Stratified Snell's-law tracer (library.py:1096-1268), one wavefront per ray; device pointers.
#define PRHF_SNELL_OUTPUTS 8   // path km, delay s, x_mid, z_mid, ground range, x_turn, z_turn, n_path
struct SnellArgs {
    const double* den;
    const double* bmag;
    const double* bpsi;
    const double* alt;
    const double* freq_hz;       // (n_rays)
    const double* elev_deg;      // (n_rays)
    const long long* prof_idx;   // (n_rays) or null: every ray uses profile 0
    // Grouped launch (prhf_snell_fan_f64): rays that share (profile, frequency) read their levels from a table
    // computed once per group instead of evaluating the Appleton-Hartree index level by level themselves.
    const long long* ray_group;  // (n_rays) group of each ray, or null: ungrouped (freq_hz / prof_idx per ray)
    const double* group_freq;    // (n_groups) [Hz]
    const long long* group_prof; // (n_groups) or null: profile 0
    long long n_groups;
    double* levels;              // (n_groups, n_alt + 1) mu' of every level (ground level first when inserted)
    // ... and, made beside it once per group (snell_tables_kernel), what every ray of the group would otherwise make itself:
    double* group_entries;       // (n_groups, n_alt + 1, 4) the levels with a finite mu, compacted: altitude, mu, mu', running
                                 // minimum of the bracket criterion (mu, or mu r on a spherical Earth) over the entries 1 .. i
    int* group_kidx;             // (n_groups, n_alt + 1) grid level of each entry
    int* group_info;             // (n_groups, 4) entries, "ground level inserted", error bits (1 profile index, 2 negative
                                 // density), profile
    // Per-ray launch: persistent wavefronts drawing rays from queues (snell_queue_bytes() of counters, zeroed by the launch's first kernel)
    unsigned* ray_queue;
    int resident_cus;            // multiprocessors of the device (sizes the persistent grid)
    double* prof_info;           // (n_prof, 4) scratch: max|B|, "has a negative density", the level of the largest density (a
                                 // hint: where a ray that escapes would have come closest to turning), filled by launch_snell
    // Per-profile level table (or null), filled by launch_snell: what a level's mu and mu' need that does not depend on
    // the frequency - f_N^2 = (sqrt(den) c_p)^2, g_p |B|, sin(psi), cos(psi) - so that a ray pays two quotients and
    // the Appleton-Hartree algebra per level instead of a square root and a correctly rounded sine / cosine on top
    // (the same operations on the same values: bit-identical).  Worth it when the rays outnumber the profiles.
    double* ptab;                // (n_prof, n_alt, 4)
    long long n_prof;
    double* out;                 // (n_rays, PRHF_SNELL_OUTPUTS)
    double* path_x;              // (n_rays, path_stride) or null
    double* path_z;
    unsigned* status;
    long long n_rays, n_alt, prof_stride, alt_stride, path_stride;
    int mode;
    int reduced;                 // per-ray launch: levels far from reflection and from the ray's turning point in the reduced
                                 // algebra (the default; 0: every level in the reference's operation order) - prhf_snell.inc
    int geometry;                // 0 flat Earth, 1 spherical Earth
    double earth_radius_km;      // spherical only (library.py:1473, :1552-1553)
    double dz_target_km;         // spherical sub-step controls (library.py:1470-1472)
    double apex_boost;
    int max_substeps;
};
size_t snell_queue_bytes();            // the per-ray launch's queue counters (SnellArgs::ray_queue, 128-byte aligned)
hipError_t launch_snell(const SnellArgs& a, hipStream_t stream);   // with a.ray_group: level table kernel first
// wavefronts of the per-ray kernel that one device keeps resident; cu_count: multiprocessors of the device
hipError_t snell_resident_waves(long long n_alt, int cu_count, long long* waves, bool ptab = false, bool reduced = false,
                                int geometry = 0);

// Point-to-point homing for the grouped tracer (prhf_homing.inc): the rays of a group that land at a link's range.
#define PRHF_HOME_OUTPUTS (3 + PRHF_SNELL_OUTPUTS)   // elevation_deg, status, scan_index, then the tracer's eight
struct HomeArgs {
    SnellArgs s;                 // a grouped launch's arguments (tables, columns, controls); elev_deg, ray_group, out unused
    const double* scan_elev;     // (n_scan) scan grid [deg], strictly increasing
    const long long* link_group; // (n_links) group of each link
    const double* link_range;    // (n_links) target ground range [km]
    long long n_links;
    int n_scan;
    double range_tol;            // [km]
    int max_iter, max_roots;
    // D(e) is the landing x of hop g.n_hops - 1 (1: the tracer's ray).  row_width: PRHF_GRAD_HOME_OUTPUTS for the one-hop
    // call; 3 + PRHF_GRAD_HOP_OUTPUTS g.n_hops for the multi-hop call, whose rows hold every hop's row with its launch.
    int row_width;
    double* scan_d;              // (n_groups, n_scan) scratch: ground range of every scan ray
    int* work;                   // (n_links max_roots, 4) scratch: (link, rank, interval, 0) of the brackets to refine; 16-byte aligned
    unsigned* queue;             // home_queue_bytes() of scratch: the refine launch's counters, the work list's length
    double* out;                 // (n_links, max_roots, PRHF_HOME_OUTPUTS)
    long long* n_brackets;       // (n_links)
};
size_t home_queue_bytes();
hipError_t launch_snell_home(const HomeArgs& h, hipStream_t stream);   // tables, scan, brackets, refinement: five kernels

// Skip distance of a group and MUF of a link for the grouped tracer (prhf_skip.inc).
#define PRHF_SKIP_OUTPUTS (5 + PRHF_SNELL_OUTPUTS)   // elevation_deg, status, scan_index, bracket_deg, n_evals, then the tracer's eight
#define PRHF_MUF_OUTPUTS (3 + PRHF_SKIP_OUTPUTS)     // muf_hz, f_above_hz, status, then the skip row at muf_hz
struct SkipArgs {
    SnellArgs s;                 // a grouped launch's arguments (tables, columns, controls); elev_deg, ray_group, out unused
    const double* scan_elev;     // (n_scan) scan grid [deg], strictly increasing
    int n_scan;
    double elev_tol;             // [deg]
    int max_iter;
    const int* active;           // (n_groups) or null: groups with a 0 here are left alone (the MUF search's settled links)
    double* scan_d;              // (n_groups, n_scan) scratch: ground range of every scan ray
    double* out;                 // (n_groups, PRHF_SKIP_OUTPUTS)
};
hipError_t launch_snell_skip(const SkipArgs& h, hipStream_t stream);   // tables, scan, refinement: four kernels
struct MufArgs {
    SkipArgs k;                  // a link is a group: k.s.n_groups == n_links, k.s.group_freq == group_freq, k.active == active,
                                 // k.out (n_links, PRHF_SKIP_OUTPUTS) scratch: the skip rows of the trip
    const double* link_range;    // (n_links) target ground range [km]
    long long n_links;
    double f_lo, f_hi;           // [Hz]
    int n_bisect;
    double* group_freq;          // (n_links) scratch: the device-side group table's frequencies, written once per trip
    int* active;                 // (n_links) scratch
    double* state;               // (n_links, 4) scratch: lo, hi, status, 0
    double* best;                // (n_links, PRHF_SKIP_OUTPUTS) scratch: the skip row at lo
    double* out;                 // (n_links, PRHF_MUF_OUTPUTS)
};
hipError_t launch_snell_muf(const MufArgs& m, hipStream_t stream);     // (2 + n_bisect) x (set, tables, scan, refine, decide)

// 2-D refractive-index fields and the gradient tracers (prhf_gradient.inc); device pointers throughout.
struct FieldPackArgs {
    const double* mu;            // (n_fields, n0, n1)
    const double* mup;
    const double* a0;            // (n0), (n1): the axes
    const double* a1;
    double* rec;                 // (n_fields, n0, n1, 4): mu, d/da1, d/da0, mu'
    long long n_fields;
    int n0, n1;
    int uniform0, uniform1;      // all np.diff(axis) are equal: np.gradient's scalar-spacing branch
    int edge_order;
};
struct FieldSampleArgs {
    const double* rec;
    const double* a0;
    const double* a1;
    const double* p0;            // (n) coordinates along a0 and a1
    const double* p1;
    const long long* field;      // (n) or null: field 0
    double* out_n;               // (n) each, or null
    double* out_d1;
    double* out_d0;
    double* out_mup;
    unsigned* status;
    long long n, n_fields;
    int n0, n1;
    double fill_n, fill_grad, fill_mup;
};
#define PRHF_GRAD_OUTPUTS 12     // path km, delay s, x_mid, z_mid, ground range, x_apex, z_apex, status, nodes, RHS calls, rejected steps, 0
#define PRHF_GEO_CARTESIAN 0     // state (x, z, vx, vz) on (z, x) axes
#define PRHF_GEO_SPHERICAL 1     // state (r, phi, v_r, v_phi) on (r, phi) axes
struct GradTraceArgs {
    const double* rec;
    const double* a0;            // z axis (n0), x axis (n1); spherical: r axis, phi axis
    const double* a1;
    const double* x0;            // (n_rays) each
    const double* z0;
    const double* elev;
    const long long* ray_field;  // (n_rays) or null: field 0
    double* out;                 // (n_rays, PRHF_GRAD_OUTPUTS)
    double* path_t;              // (n_rays, path_stride) each, or all null: t and the four state components
    double* path_x;
    double* path_z;
    double* path_vx;
    double* path_vz;
    unsigned* status;
    long long n_rays, n_fields, path_stride;
    int n0, n1;
    int renormalize_every;       // (Cartesian only: the spherical right-hand side has nothing that depends on it)
    int geometry;                // PRHF_GEO_*
    // spherical: z_ground = R_E + z_ground_km, z_max = r_max_km, x_min / x_max = phi_min / phi_max
    double s_max, rtol, atol, max_step, z_ground, z_max, x_min, x_max;
    double fill_n, fill_grad, fill_mup;
    double earth_radius;         // spherical only
    // multi-hop calls only (prhf_gradient_hops.inc): hops per ray, and z_ground_km as the caller gave it (the launch
    // altitude of every hop after the first; z_ground above carries R_E + z_ground_km in a spherical call)
    int n_hops;
    double hop_z0;
};
#define PRHF_FIELD_MAX_AXES 8000   // n0 + n1 at most: both axes are staged in 64 KiB of LDS
inline size_t field_axes_lds_bytes(int n0, int n1) { return (size_t)(n0 + n1) * 8; }
hipError_t launch_field_pack(const FieldPackArgs& a, hipStream_t stream);
hipError_t launch_field_sample(const FieldSampleArgs& a, hipStream_t stream);
hipError_t launch_grad_trace(const GradTraceArgs& a, hipStream_t stream);
#define PRHF_GRAD_MAX_HOPS 16
#define PRHF_GRAD_HOP_OUTPUTS (3 + PRHF_GRAD_OUTPUTS)    // launch x, launch z, launch elevation, then the tracer's twelve
// Chains of a.n_hops rays: a.out is (n_rays, n_hops, PRHF_GRAD_HOP_OUTPUTS), the paths
// (n_rays n_hops, path_stride).
hipError_t launch_grad_hop_trace(const GradTraceArgs& a, hipStream_t stream);

// Point-to-point homing for the gradient tracers (prhf_gradient_homing.inc): the rays of a transmitter that land at a
// link's target coordinate.
#define PRHF_GRAD_HOME_OUTPUTS (3 + PRHF_GRAD_OUTPUTS)   // elevation_deg, status, scan_index, then the tracer's twelve
#define PRHF_GRAD_HOME_COUNTERS 4                        // records, rays refined, ray slots of the refine waves, refine waves
struct GradHomeArgs {
    GradTraceArgs g;             // records, axes, controls, fills, geometry, status; the per-ray arrays and the paths are null
    const long long* group_field;   // (n_groups) field, launch point of each group
    const double* group_x0;
    const double* group_z0;
    long long n_groups;
    const long long* link_group; // (n_links) group of each link
    const double* link_target;   // (n_links) target ground_range_km
    long long n_links;
    const double* scan_elev;     // (n_scan) scan grid [deg], strictly increasing
    int n_scan;
    double range_tol;            // [km]
    int max_iter, max_roots;
    // D(e) is the landing x of hop g.n_hops - 1 (1: the tracer's ray).  row_width: PRHF_GRAD_HOME_OUTPUTS for the one-hop
    // call; 3 + PRHF_GRAD_HOP_OUTPUTS g.n_hops for the multi-hop call, whose rows hold every hop's row with its launch.
    int row_width;
    double* scan_d;              // (n_groups, n_scan) scratch: ground range of every scan ray
    int* work;                   // (n_links max_roots, 4) scratch: (link, rank, interval, 0) of the brackets to refine; 16-byte aligned
    unsigned* queue;             // PRHF_GRAD_HOME_COUNTERS words of scratch, zeroed by the scan kernel
    double* out;                 // (n_links, max_roots, row_width)
    long long* n_brackets;       // (n_links)
};
hipError_t launch_grad_home(const GradHomeArgs& h, hipStream_t stream);   // scan, brackets, refinement, result rays: four kernels

// Fields of many frequencies built on the device, skip distance of a transmitter and MUF of a link for the gradient
// tracers (prhf_gradient_skip.inc).
struct FieldBuildArgs {
    const double* den;           // (plane) each: one 2-D ionosphere
    const double* bmag;
    const double* bpsi;
    const double* freq;          // (n_freq) [Hz]
    const int* active;           // (n_freq) or null: frequencies with a 0 here are left alone (the MUF search's settled links)
    const unsigned long long* bmax;   // 2 words (launch_field_bmax): nanmax|B| as a bit pattern, != 0 when any B is not NaN
    double* mu;                  // (n_freq, plane) each
    double* mup;
    long long n_freq, plane;
    int mode;                    // PRHF_KMODE_*
};
hipError_t launch_field_bmax(const double* bmag, long long plane, unsigned long long* words, hipStream_t stream);
hipError_t launch_field_build(const FieldBuildArgs& a, hipStream_t stream);

#define PRHF_GRAD_SKIP_OUTPUTS (6 + PRHF_GRAD_OUTPUTS)       // skip_km, elevation_deg, status, scan_index, bracket_deg, n_evals, then the tracer's twelve
#define PRHF_GRAD_MUF_OUTPUTS (3 + PRHF_GRAD_SKIP_OUTPUTS)   // muf_hz, f_above_hz, status, then the skip row at muf_hz
#define PRHF_GRAD_SKIP_COUNTERS 4                            // groups refined, rays refined, ray slots of the refine waves, refine waves
#define PRHF_GRAD_SKIP_QUEUE_WORDS 8                         // [0] the work list's length, [1..3] counters 1..3, [4] counter 0, [5] hop rays
// Multi-hop rows: the six head values, then the g.n_hops hop rows of launch_grad_hop_trace
#define PRHF_GRAD_HOP_SKIP_OUTPUTS(n_hops) (6 + PRHF_GRAD_HOP_OUTPUTS * (n_hops))
struct GradSkipArgs {
    GradTraceArgs g;             // records, axes, controls, fills, geometry, status; the per-ray arrays and the paths are null
    const long long* group_field;   // (n_groups) field, launch point of each group
    const double* group_x0;
    const double* group_z0;
    long long n_groups;
    const double* scan_elev;     // (n_scan) scan grid [deg], strictly increasing
    int n_scan;
    double elev_tol;             // [deg]
    int max_iter;
    const int* active;           // (n_groups) or null: groups with a 0 here are left alone (the MUF search's settled links)
    double* scan_d;              // (n_groups, n_scan) scratch: ground range of every scan ray
    int* work;                   // (n_groups, 2) scratch: (group, scan node) of the groups to refine; 8-byte aligned
    unsigned* queue;             // PRHF_GRAD_SKIP_QUEUE_WORDS words of scratch, zero when the call's first kernel starts
    // the doubles of a row of `out`: PRHF_GRAD_SKIP_OUTPUTS for the one-hop call (g.n_hops is not read);
    // PRHF_GRAD_HOP_SKIP_OUTPUTS(g.n_hops) for the chain call, where D(e) is the landing x of hop g.n_hops - 1
    int row_width;
    double* out;                 // (n_groups, row_width)
};
// scan, node, refinement, result rays: four kernels.  chain: the multi-hop instantiations (rows of row_width doubles)
hipError_t launch_grad_skip(const GradSkipArgs& h, bool chain, hipStream_t stream);
struct GradMufArgs {
    GradSkipArgs k;              // a link is a group: k.n_groups == n_links, k.group_field == group_field, k.active == active,
                                 // k.g.rec == p.rec, k.out (n_links, k.row_width) scratch: the skip rows of the trip
    FieldBuildArgs b;            // b.freq == group_freq, b.active == active, b.n_freq == n_links
    FieldPackArgs p;             // p.mu == b.mu, p.mup == b.mup, p.n_fields == n_links
    const double* link_target;   // (n_links) target ground_range_km
    long long n_links;
    double f_lo, f_hi;           // [Hz]
    int n_bisect;
    double* group_freq;          // (n_links) scratch: every link's frequency of the trip
    long long* group_field;      // (n_links) scratch: 0 .. n_links - 1
    int* active;                 // (n_links) scratch
    double* state;               // (n_links, 4) scratch: lo, hi, status, 0
    double* best;                // (n_links, 6) scratch: the head of the skip row at lo
    double* out;                 // (n_links, 3 + k.row_width)
};
// Bmax, then (2 + n_bisect) x (set, build, pack, scan, node, refine, decide), then set, build, pack, result, decide
hipError_t launch_grad_muf(const GradMufArgs& m, bool chain, hipStream_t stream);

// residual / cost may be null
hipError_t launch_residual(const double* vh_model, const double* vh_obs, long long n_prof, int n_freq,
                           double* residual, double* cost, hipStream_t stream);

// Many ionograms on one frequency grid (prhf_residual_many.inc): an item is a (candidate row, ionogram) pair
#define PRHF_MANY_MAX_FREQ 4096          // grid frequencies: a wave keeps 12 bytes of LDS for each
#define PRHF_MANY_ITEMS_PER_WAVE 16
struct ResidualManyArgs {
    const double* vh_model;              // (n_rows, n_freq)
    const double* vh_obs;                // (n_iono, n_freq), NaN: no observation
    const int* ionogram_of_row;          // (n_rows), or null: shared candidates - every row against every ionogram
    long long n_rows;
    long long n_items;                   // n_rows, or n_iono n_rows with shared candidates (item q = i n_rows + row)
    int n_iono, n_freq, items_per_wave;
    double* residual;                    // (n_rows, n_freq) or null; own candidates only
    double* cost;                        // (n_items)
};
hipError_t launch_residual_many(const ResidualManyArgs& a, hipStream_t stream);
// best (n_iono): the first row of the smallest finite cost (a global row; shared candidates: the candidate), -1: none
hipError_t launch_residual_best(const double* cost, const int* ionogram_of_row, long long n_rows, int n_iono, long long* best,
                                double* best_cost, hipStream_t stream);

// Levenberg-Marquardt fits of many ionograms in a reduced basis (prhf_lm.inc); device pointers.
struct LmSynthArgs {
    const double* den0;      // background columns, den0_stride doubles apart (0: one column for every ionogram)
    const double* basis;     // n_tan rows of n_alt, basis_stride doubles between ionograms (0: one set)
    const double* c;         // (n_iono, n_tan) coefficients
    const int* status;       // (n_iono) or null; given: an ionogram whose status is PRHF_LM_NO_DATA gets a NaN column
    const int* frozen;       // (n_iono) statuses or null; given: an ionogram that is not PRHF_LM_RUNNING is left as it stands
    double* den;             // (n_iono, n_alt): den0 exp(sum_t c_t B_t)
    double* tan;             // (n_iono, n_tan, n_alt): den B_t, or null
    long long n_iono, n_alt, den0_stride, basis_stride;
    int n_tan;
};
hipError_t launch_lm_synth(const LmSynthArgs& a, hipStream_t stream);
struct LmStepArgs {
    const double* vh_obs;    // (n_iono, n_freq), NaN: no observation
    const double* vh_eval;   // (n_iono, n_freq): the operator at c_eval
    const double* dvh;       // (n_iono, n_freq, n_tan): its JVP along den B_t
    const double* prior;     // (n_tan) or null
    // one ionogram's state (prhf_lm_step.h); at k = 0 only c_eval is read (the start)
    double *c, *c_eval, *A, *g, *delta, *cost, *lambda;    // (n_iono, n_tan) x 2, (n_iono, n_tan (n_tan + 1) / 2), (n_iono, n_tan) x 2, (n_iono) x 2
    int *status, *n_eval, *n_accept;
    double* vh_fit;          // (n_iono, n_freq): the trace of the accepted point
    double* history;         // (n_iono, max_iter) accepted cost after every evaluation, or null
    double* state_out;       // (n_iono, n_tan^2 + 2 n_tan): A in full, g, delta, of every ionogram still running, or null
    long long n_iono;
    int n_freq, n_tan, k;    // k: the evaluation, 0 ... max_iter - 1
    int max_iter;
    double lambda0, lambda_up, lambda_down, step_max, ftol, xtol;
};
hipError_t launch_lm_step(const LmStepArgs& a, hipStream_t stream);

}  // namespace prhf

#endif
