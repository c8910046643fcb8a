/*
 * prhf.h - C ABI of libprhf.so, the MI355X (gfx950) vertical-ionogram forward operator.
 *
 * Drop-in boundary.  The reference has no FFI layer: its boundary is the Python function
 *     PyRayHF.library.vertical_forward_operator(freq, den, bmag, bpsi, alt, mode='O', n_points=200)
 * (reference PyRayHF/library.py:459-509).  The entry points below are what a ctypes binding
 * for that function calls; pyrayhf_amd/library.py is that binding.
 *
 * Conventions
 *   - plain pointers and sizes only; all arrays are float64, C-contiguous rows;
 *   - every function returns 0 (PRHF_OK) or a negative PRHF_E* code; prhf_last_error()
 *     returns a thread-local message for the last failure on the calling thread;
 *   - the library borrows caller buffers for the duration of a call (or, with
 *     PRHF_FLAG_ASYNC, until the next prhf_sync on that context) and owns nothing but its
 *     context (stream, scratch, events);
 *   - a context is bound to one device and is not thread-safe; different contexts are
 *     independent and may be used from different threads;
 *   - every entry point runs on its context's device and restores the calling thread's current
 *     HIP device before it returns (a process that drives several GPUs keeps its own current device).
 *
 * Units are the reference's (library.py:465-474): freq MHz, den m^-3, bmag Tesla,
 * bpsi degrees, alt km; the result is virtual height in km, NaN where the sounder
 * frequency is not reflected below the density peak.
 */
#ifndef PRHF_H
#define PRHF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRHF_ABI_VERSION 4   /* 2: + prhf_snell_fan_f64, prhf_recent_kernel_ms, PRHF_FLAG_SHARED_FIELD (round 2)
                              * 3: + prhf_ctx_set_option (round 3)
                              * 4: + prhf_field_pack_f64, prhf_field_sample_f64, prhf_trace_gradient_f64;
                              *    prhf_trace_gradient_spherical_f64 and prhf_snell_home_f64 joined later without a new
                              *    number: a new symbol changes nothing for a caller of the others (so did
                              *    prhf_gradient_home_f64, prhf_snell_skip_f64, prhf_snell_muf_f64 and
                              *    prhf_pair_plan_counters, prhf_panel_counters, and prhf_field_build_f64,
                              *    prhf_gradient_skip_f64, prhf_gradient_muf_f64, prhf_gradient_skip_counters,
                              *    prhf_trace_gradient_hops_f64, prhf_gradient_hop_home_f64, and
                              *    prhf_residual_many_f64, prhf_vfo_residual_many_f64, and
                              *    prhf_gradient_hop_skip_f64, prhf_gradient_hop_muf_f64,
                              *    prhf_gradient_hop_skip_counters, and prhf_panel_upper_counters,
                              *    and prhf_stream_launches, and prhf_panel_plan_counters, and
                              *    prhf_panel_quick_counters, and prhf_vfo_lm_fit_f64, prhf_lm_fit_counters) */

/* return codes */
#define PRHF_OK        0
#define PRHF_EINVAL   -1   /* null pointer, bad shape, n_points < 1, bad mode, bad flag combination, bad segment or index,
                            * a host-buffer multiplier grid that decreases, an unknown option */
#define PRHF_ENEGDEN  -2   /* a density below the peak is negative (reference library.py:93-94 raises ValueError) */
#define PRHF_EPEAK0   -3   /* density peak at index 0: empty bottomside (the reference raises IndexError) */
#define PRHF_EHIP     -4   /* HIP runtime failure; message carries hipGetErrorString */
#define PRHF_ENOMEM   -5   /* scratch allocation failed */

/* wave modes: reference 'O' and 'X' (library.py:391-396, :221-226) */
#define PRHF_MODE_O 0
#define PRHF_MODE_X 1

/* flags of prhf_vfo_batch_f64 / prhf_vfo_worklist_f64 */
#define PRHF_FLAG_DEVICE_PTRS 0x1u  /* every array pointer (inputs, multiplier, output) is device memory */
#define PRHF_FLAG_ASYNC       0x2u  /* device pointers only: enqueue and return; data errors surface at prhf_sync */
#define PRHF_FLAG_GRID_STABLE 0x4u  /* the multiplier array at this address (device or host) keeps its contents for as
                                     * long as the context lives, so the table the library derives from it (grid steps,
                                     * one small kernel) - and, for a host array, its device copy - is made once per
                                     * (address, length) and reused (at most 16 host grids are remembered) */
#define PRHF_FLAG_SHARED_FIELD 0x8u /* bmag and bpsi are ONE row of n_alt values each, shared by every profile (a fit's
                                     * candidates differ in their density only, library.py:589-591): a third of the
                                     * bytes to upload and to read */

/* arithmetic tiers, prhf_ctx_set_math (see DESIGN.md "Arithmetic tiers") */
#define PRHF_MATH_FAITHFUL 0  /* reference operation order, IEEE divide/sqrt, no contraction */
#define PRHF_MATH_FAST     1  /* reduced algebra, rsqrt + Newton, contracted; X-mode error <= 1e-9 relative */
#define PRHF_MATH_AUTO     2  /* the default, per slice.  X mode: fast.  O mode (ill conditioned near X = 1): the
                               * reference's operation order at every grid point with 1 - X <= 1e-5, the reduced
                               * algebra where the order cannot matter; reproduces the reference to 1e-10 */

typedef struct prhf_ctx prhf_ctx;

/* One homogeneous slice of a mixed launch (BASELINE config 5): profiles [prof_begin, prof_end)
 * are evaluated with one mode and one grid size.  mult_offset indexes the concatenated
 * multiplier array; the slice's output rows start at vh_out + out_offset (row-major
 * (prof_end - prof_begin, n_freq)).  out_offset must be a non-negative multiple of n_freq and the
 * output rows of two segments must not overlap (PRHF_EINVAL otherwise).  With host buffers, output rows
 * below the highest written row that no segment covers come back as NaN; with device pointers the
 * library writes only the rows its segments cover. */
typedef struct prhf_segment {
    int64_t prof_begin;
    int64_t prof_end;
    int32_t mode;
    int32_t n_points;
    int64_t mult_offset;
    int64_t out_offset;
} prhf_segment;

int prhf_abi_version(void);
const char* prhf_last_error(void);
int prhf_device_count(int* n);

int prhf_ctx_create(int device, prhf_ctx** out);
int prhf_ctx_destroy(prhf_ctx* ctx);

/* borrow != 0: launch on the caller's hipStream_t (e.g. torch's current stream; a NULL handle is the legacy
 * default stream, which is what torch reports for its default stream).  borrow == 0: return to the context's
 * own non-blocking stream (hip_stream is ignored). */
int prhf_ctx_set_stream(prhf_ctx* ctx, void* hip_stream, int32_t borrow);

/* Select the arithmetic tier (PRHF_MATH_*), default PRHF_MATH_AUTO. */
int prhf_ctx_set_math(prhf_ctx* ctx, int level);

/* Launch-shaping and arithmetic settings of this context, by name (tests and A/B measurements; the defaults are
 * the measured best and no caller needs to touch them).  The library reads no environment variable: only a
 * -DPRHF_DIAG build presets these from PRHF_<NAME> at context creation.  PRHF_EINVAL for an unknown name or a
 * value outside the option's range.
 *   "well_conditioned"   default O-mode arithmetic: the reference's operation order where 1 - X <= this (1e-5)
 *   "short_kernel"       0: short O-mode grids (2 .. 1024 points) stay in the general kernel (1)
 *   "shortx_kernel"      0: X-mode grids of 2 .. 1024 points (fast tier) stay in the general kernel (1)
 *   "short_concurrent"   0: a mixed list runs its short-grid and general launches one after the other (1)
 *   "short_queue"        > 0: the short-grid kernel's queue of ill-conditioned points holds exactly this many entries (0)
 *   "persistent", "tail_bpp", "tail_rounds", "split_few_profiles", "split_min_points", "target_waves"
 *                        how a launch is cut into workgroups (never the value of a pair)
 *   "no_candidates", "thread_scan_min", "lean_min_points"
 *                        which of the equivalent search / loop paths a pair takes
 *   "local_chunks"       0: the chunks of a few-pair launch on a long grid are spread over the launch and added by a
 *                        second kernel (1: a pair's chunks are waves of one workgroup, which adds them up itself)
 *   "direct_upload"      0: a small host-buffer call stages its inputs in pinned memory and copies them (1: on a
 *                        large-BAR device the CPU writes them straight into device memory)
 *   "timing"             1: synchronous host-buffer operator calls record timing events too (0; see prhf_last_kernel_ms)
 *   "trim_lds"           0: a column of more than 1400 levels is always staged in global memory (1: when every
 *                        bottomside of the launch fits LDS, only the levels up to the highest peak are staged)
 *   "tall_lean"          0: a profile staged in global memory takes the generic loop (1: the main loop reads its nodes
 *                        from the slab)
 *   "strided_top"        0: every grid point of a long X-mode grid is evaluated, the launch of ABI 4 before this option bit
 *                        for bit (1: whole pairs of at least 8192 points in X mode, fast tier, on a grid that is the
 *                        reference's stretch: the top three altitude segments are summed from every eighth point plus
 *                        Euler-Maclaurin end corrections, within 1e-12 of the full sum; any other grid is detected on
 *                        the device and keeps the full sum)
 *   "strided_lower"      0: only those three segments take the strided sum, the launch of before this option bit for
 *                        bit (1: on a uniform altitude grid the segments of at least 64 points below them do too - one
 *                        strided pass plus one pass over the points around the segment boundaries; a pair with a
 *                        segment too close to X + Y = 1 keeps the sum of before; "strided_top" = 0 switches both off)
 *   "panel_lower"        0: the segments below the top three are summed as "strided_lower" says, the launch of before this
 *                        option bit for bit (1: where "strided_lower" applies, the region below the top three segments is
 *                        cut at every segment's first point, and a segment's run of n points into ceil(n / 128) pieces
 *                        of equal length; a piece is summed from nodes at real-valued indices ("panel_nodes") with
 *                        weights that make the rule exact for the discrete sum of polynomials of degree 7 - within 1e-12
 *                        of the full sum; a pair with a piece of more than 8 points too close to X + Y = 1 keeps the sum
 *                        of before)
 *   "panel_nodes"        8: every piece of the panel sum takes eight lanes - its own points up to eight, else eight
 *                        Gauss-Legendre nodes.  Since the region is cut at segments' first points alone, and a segment's
 *                        run into ceil(n / 128) equal pieces, this setting no longer gives the bits of the launch before
 *                        the option existed
 *                        (4: a piece takes four lanes - its own points up to four, else the four nodes of the Gauss rule
 *                        of the counting measure on its points, exact for the same polynomials; the pieces of a run
 *                        whose segment's continuation reaches X + Y = 1 within 16 piece lengths of it are halved until
 *                        it does not, or until they hold at most four points.  Both settings use the same cuts and the
 *                        same guard: the same pairs take the rule and the same pairs fall back; with 4 values stay
 *                        within 1e-12 of "panel_lower" = 0.  Values between 4 and 8 count as 8)
 *   "panel_upper"        0: the region of the panel sum ends below the third segment from the top, the launch of before
 *                        this option bit for bit (1: where "panel_lower" applies, under either setting of "panel_nodes",
 *                        the region ends at the top segment's first point, rounded down to a multiple of 64 from four
 *                        points above it: the two segments below the top one are runs of the panel sum like any other,
 *                        and only the top segment keeps its strided sum.  A pair does so if the runs whose extent
 *                        changes - from the third segment below the top one upwards - pass the tests every run passes,
 *                        which is settled from the pair alone before any of them is summed; a pair where one fails
 *                        keeps the lower region and the strided sums of those two segments, it does not fall back as a
 *                        whole on their account.  Values stay within 1e-12 of the full sum.  A grid whose piece of the
 *                        strided table lies 2^26 entries - 1 GiB of pair table - or more behind the grid itself keeps
 *                        the lower region as with 0: the main loop reads option "panel_quick" in that bit of the offset)
 *   "panel_quick"        0: every list of the panel sum's runs puts every run to the exact tests (1: where "panel_upper"
 *                        applies, a list - up to 63 runs of a pair's region - whose every run passes a bound from
 *                        1 - X - Y at the two levels of its segment skips them: both levels at 1e-3 or more, and the
 *                        index where the segment's continuation reaches X + Y = 1 at least 16 L + 10 indices beyond the
 *                        run, L the points of the run's pieces.  The bound implies what the exact tests would find, so
 *                        values, fall-backs and every other counter are the same under both settings;
 *                        prhf_panel_quick_counters counts the lists of both kinds)
 *   "strided_grade"      0: the strided stretch of each of the top three segments takes every eighth point throughout, the
 *                        launch of before this option bit for bit (1: the stretch is cut into zones by the distance to
 *                        the index where the segment's continuation reaches X + Y = 1 - every 32nd point at least 1024
 *                        indices below it and only where 1 - X - Y >= 1.6e-4, every 16th at least 512 below it and only
 *                        where 1 - X - Y >= 1e-5, every eighth next to it as before - with Euler-Maclaurin corrections
 *                        of both zones at each junction.  A coarse zone holds whole wavefront iterations: a multiple of
 *                        2048 indices at stride 32, of 1024 at stride 16; the last 64 indices stay at stride 8.  Values
 *                        stay within 1e-12 of the full sum.  A segment that has that index below it is not cut)
 *   "pair_plan"          0: every wavefront computes the integers that steer its pair's strided sum itself, the launch of
 *                        before this option bit for bit (1: where "strided_lower" applies and a workgroup settles its
 *                        reflection heights one frequency per thread - at most 512 frequencies, grids of fewer than 65536
 *                        points - one thread per pair computes them beforehand; a pair whose plan finds no room, or whose
 *                        closed-form guess of a segment's first point does not bracket it, still computes its own.  The
 *                        integers are the same either way: no value depends on this option)
 *   "pair_plan_cap"      > 0: a workgroup keeps at most this many plans (0: as many as fit; tests)
 *   "stream_blocks"      0: every persistent launch is the general kernel's, the launch of before this option instruction
 *                        for instruction (1: a persistent launch of ONE X-mode fast-tier slice of whole pairs whose
 *                        workgroups settle reflection heights per thread - at most 512 frequencies, a uniform altitude
 *                        grid still decided per profile - and whose staged profile fits half of a CU's LDS runs as one
 *                        16-wave workgroup per CU with two staged profiles: one wave stages the next profile while the
 *                        others sum the current one, and no barrier separates two profiles.  2: also when the launch has
 *                        fewer blocks than the device keeps resident; tests.  No value depends on this option.  A wave
 *                        that waits seconds for a slot of its own workgroup gives the launch up: PRHF_EHIP)
 *   "stream_grid"        > 0: the streaming form launches at most this many workgroups (0: one per CU; tests, A/B runs)
 *   "short_compact", "short_prio", "short_order", "short_lanes"
 *                        geometry of the short-grid kernels: four 4-wave workgroups per CU (1), wave priorities by age (1),
 *                        blocks in descending cost order (1), lanes per pair in the O kernel (8; 16: four pairs per work
 *                        item instead of eight - another order of additions in a pair's sum, 1e-16 apart)
 *   "host_slabs"         large host-buffer batches go in this many slabs so that transfers overlap the kernel (3; 1: none)
 *   "snell_table"        tracers: the frequency-independent parts of a level's mu, mu' (f_N^2, g_p |B|, sin psi, cos psi)
 *                        are tabulated once per profile when the rays (groups) number at least this many times the
 *                        profiles and the table stays under 1 GiB (4; 0: never) */
int prhf_ctx_set_option(prhf_ctx* ctx, const char* name, double value);

/*
 * Virtual heights of n_prof profiles x n_freq sounder frequencies.
 *
 * Replaces: vertical_forward_operator (reference library.py:459-509) and everything below it
 * (regrid_to_nonuniform_grid :324-438, find_X :120-137, find_Y :140-158, find_mu_mup :161-256,
 * find_vh :259-293), evaluated once per profile row; semantics are a loop of single-profile
 * reference calls.
 *
 *   freq_mhz    (n_freq)                       sounder frequencies, MHz
 *   den,bmag,bpsi  n_prof rows of n_alt values, row p at ptr + p*prof_stride_elems
 *   alt         (n_alt) shared by all profiles when alt_stride_elems == 0, else row p at
 *               alt + p*alt_stride_elems; ascending
 *   multiplier  (n_points) stretched unit grid, smooth_nonuniform_grid(0,1,n_points,10.)
 *               (library.py:296-321, :361-364) computed by the host in float64; values in [0, 1] and
 *               NON-DECREASING (the main loop's top-segment search relies on it: PRHF_EINVAL for a host
 *               buffer that decreases; a device-resident grid is the caller's responsibility)
 *   A frequency that is not a positive finite number gives a NaN column (the reference: NaN for 0 and NaN).
 *   vh_out      (n_prof, n_freq) row-major
 *   NaN inputs are not errors; they behave as in the reference: a NaN in den ranks as the column's maximum, the
 *   first one wins (np.argmax, library.py:371: a density column padded with NaN is cut at the padding); a NaN in alt
 *   makes the profile's row NaN (:507), and so does a NaN in bmag below the peak in X mode (:389); in O mode, and for
 *   a NaN in bpsi, the grid points of the two segments next to that level drop out of the sum (:288).
 *   (prhf_regrid_f64 refuses a NaN in alt, bmag or bpsi below the peak: PRHF_EINVAL.)
 * Limits: n_alt <= 65535, n_freq <= 2^20, n_points >= 1.  A profile's bottomside - the levels below its density
 * peak - is held in LDS when it has at most 1400 levels (for n_alt > 1400 a pre-pass finds the highest peak of the
 * launch: one synchronisation); taller bottomsides are staged in global memory (one slab per resident workgroup,
 * allocated by the context) and run the same main loop on the slab's nodes - 1.1 to 1.4 times the time per grid point
 * of a profile held in LDS (option "tall_lean" 0: the generic loop, about three times).
 */
int prhf_vfo_batch_f64(prhf_ctx* ctx,
                       const double* freq_mhz, int64_t n_freq,
                       const double* den, const double* bmag, const double* bpsi,
                       const double* alt,
                       int64_t n_prof, int64_t n_alt,
                       int64_t prof_stride_elems, int64_t alt_stride_elems,
                       const double* multiplier, int32_t n_points, int32_t mode,
                       double* vh_out, uint32_t flags);

/* Mixed O/X and mixed n_points in one launch.  multiplier is the concatenation of the
 * segments' grids; segs is host memory in every flag combination. */
int prhf_vfo_worklist_f64(prhf_ctx* ctx,
                          const double* freq_mhz, int64_t n_freq,
                          const double* den, const double* bmag, const double* bpsi,
                          const double* alt,
                          int64_t n_prof, int64_t n_alt,
                          int64_t prof_stride_elems, int64_t alt_stride_elems,
                          const double* multiplier, int64_t multiplier_len,
                          const prhf_segment* segs, int32_t n_segs,
                          double* vh_out, uint32_t flags);

/*
 * The derivative of prhf_vfo_batch_f64's virtual heights with respect to the density column: the dense Jacobian
 * jac_out[p, f, k] = d vh[p, f] / d den[p, k], or its product with an upstream gradient,
 * grad_den_out[p, k] = sum_f grad_vh[p, f] * d vh[p, f] / d den[p, k]  (what reverse-mode differentiation of a loss
 * needs; H^T of data assimilation).  The function differentiated is the reference's discrete sum exactly
 * (library.py:324-438, :259-293): vh = min(alt) + sum_i mu'(z_i) dz_i on the stretched grid z_i = alt_0 + m_i (h - alt_0)
 * below the reflection height h, np.interp's crossing of the running maximum of X (O mode) or X + Y (X mode) minus
 * 1e-6 km - the grid moves with h, and h with the two levels of its bracket.  Analytic (forward-mode dual numbers
 * through the group index), not finite differences.
 *
 * Arguments as prhf_vfo_batch_f64.  vh_out (n_prof, n_freq) may be NULL; when given it is written by the operator's own
 * launch and equals prhf_vfo_batch_f64's output bit for bit.  jac_out is (n_prof, n_freq, n_alt), grad_vh (n_prof, n_freq),
 * grad_den_out (n_prof, n_alt), all row-major.  Flags: PRHF_FLAG_DEVICE_PTRS, PRHF_FLAG_ASYNC (device pointers only),
 * PRHF_FLAG_GRID_STABLE (accepted; these kernels keep no table of the grid), PRHF_FLAG_SHARED_FIELD.
 *
 * Conventions:
 *   - a pair that has no virtual height (vh NaN: the frequency is not reflected - or a NaN altitude, a NaN |B| below the
 *     peak in X mode, every term skipped) has a row of zeros; grad_vh is not read at such a pair, so a NaN there does no
 *     harm;
 *   - levels at and above the density peak (k >= argmax den, the first NaN density ranking highest) get 0;
 *   - a one-level bottomside (the peak at level 1) whose frequency escapes also has a row of zeros: the value np.interp's
 *     one-node rule gives such a pair in the reference, mu'(level 0) * 1e-6, is not differentiated;
 *   - grid points whose term the reference's sum skips (NaN, library.py:288: a NaN |B| or psi next to the point,
 *     mu^2 < 0, mu > 1 - library.py:233, :238) are constants;
 *   - the unmagnetised branch (library.py:201-207, decided per profile as in prhf_vfo_batch_f64) is differentiated as
 *     mu' = (1 - X)^(-1/2);
 *   - the operator has kinks - a grid point exactly on a level, a tie in the density's argmax or in the running maximum,
 *     a running maximum of exactly 1 at a level; there the result is one of the one-sided derivatives, which one is
 *     unspecified.
 * The arithmetic is the same in every math tier (IEEE divide and square root).  Results are reproducible bit for bit:
 * they do not depend on scheduling, on the other profiles of the launch, or on repetition; no atomics are used.  (One
 * exception: the VJP adds its frequencies on four waves up to 908 staged levels, on two or one above, and the levels
 * staged are those of the launch's highest peak - above 908 a profile's grad_den_out row depends on the launch in the
 * rounding of that sum.  Jacobian rows do not.)
 * Limits: the levels below the highest density peak of the launch, plus the per-wave accumulator rows, must fit in LDS:
 * about 1200 levels up to the peak (n_alt itself may be larger: a pre-pass then finds the peak, one synchronisation).
 * A taller bottomside is refused with PRHF_EINVAL ("... stages at most N levels ...").  Mixed work lists are not
 * supported.  Data errors (negative density, peak at level 0) are those of prhf_vfo_batch_f64.
 */
int prhf_vfo_jacobian_f64(prhf_ctx* ctx,
                          const double* freq_mhz, int64_t n_freq,
                          const double* den, const double* bmag, const double* bpsi,
                          const double* alt,
                          int64_t n_prof, int64_t n_alt,
                          int64_t prof_stride_elems, int64_t alt_stride_elems,
                          const double* multiplier, int32_t n_points, int32_t mode,
                          double* vh_out, double* jac_out, uint32_t flags);
int prhf_vfo_vjp_f64(prhf_ctx* ctx,
                     const double* freq_mhz, int64_t n_freq,
                     const double* den, const double* bmag, const double* bpsi,
                     const double* alt,
                     int64_t n_prof, int64_t n_alt,
                     int64_t prof_stride_elems, int64_t alt_stride_elems,
                     const double* multiplier, int32_t n_points, int32_t mode,
                     const double* grad_vh, double* vh_out, double* grad_den_out, uint32_t flags);

/*
 * The Jacobian-vector product of the same derivative - the tangent-linear operator, H dx of data assimilation, what
 * forward-mode differentiation needs:  dvh_out[p, f, t] = sum_k (d vh[p, f] / d den[p, k]) * tangents[p, t, k]  for n_tan
 * directions per profile, without forming the Jacobian: what is written is n_prof * n_freq * n_tan doubles.  The matrix
 * is exactly the one prhf_vfo_jacobian_f64 returns, with its conventions; the product is formed per grid point (the
 * node's total dX along the tangent - interpolated tangent plus the node's motion with the reflection height - before
 * it meets d mu'/dX), so it agrees with jac_out times the tangent to rounding, not bit for bit.
 *
 * Arguments as prhf_vfo_vjp_f64, with: tangents, n_tan rows of n_alt doubles per profile; tan_prof_stride_elems, the
 * distance between two profiles' sets in doubles (>= n_tan * n_alt), or 0 for ONE set (n_tan, n_alt) applied to every
 * profile; vh_out (n_prof, n_freq), may be NULL - when given it is written by the operator's own launch and equals
 * prhf_vfo_batch_f64's output bit for bit; dvh_out (n_prof, n_freq, n_tan), row-major.  Flags as for the VJP.
 * n_tan == 0 is PRHF_OK and writes nothing to dvh_out (vh_out, when given, is still written).
 *
 * Conventions, beyond those of the Jacobian:
 *   - a pair that has no virtual height has dvh = 0 for every tangent, as its Jacobian row is zero: the adjoint identity
 *     sum_f g_f dvh_f = sum_k (J^T g)_k t_k holds exactly there;
 *   - tangent entries at levels k >= argmax den are not read, so a NaN there does no harm;
 *   - at a kink of the operator the result is one of the one-sided derivatives, the one the Jacobian gives.
 * The bits of dvh_out[p, f, t] depend on profile p, the frequency, n_points, mode and tangent t only: not on n_tan, on the
 * other tangents, profiles or frequencies of the call, or on repetition.  No atomics.
 * Tangents go through the kernel eight at a time - one launch per eight, the rest in a last one - while the bottomside
 * and eight tangent columns fit in LDS (908 levels up to the highest density peak of the call), four, two or one at a
 * time above that.  Limit: 1332 levels up to the peak (n_alt itself may be larger: the peak pre-pass, one
 * synchronisation); a taller bottomside is refused with PRHF_EINVAL ("the JVP stages at most 1332 levels ...").
 */
int prhf_vfo_jvp_f64(prhf_ctx* ctx,
                     const double* freq_mhz, int64_t n_freq,
                     const double* den, const double* bmag, const double* bpsi,
                     const double* alt,
                     int64_t n_prof, int64_t n_alt,
                     int64_t prof_stride_elems, int64_t alt_stride_elems,
                     const double* multiplier, int32_t n_points, int32_t mode,
                     const double* tangents, int64_t n_tan, int64_t tan_prof_stride_elems,
                     double* vh_out, double* dvh_out, uint32_t flags);

/*
 * Levenberg-Marquardt fits of n_iono ionograms on one common frequency grid, each in a small basis of log-density
 * perturbations, in one call; the first consumer of the JVP inside the library:
 *     den_i(c) = den0_i * exp(sum_t c_t * B_t),   t < n_tan,   1 <= n_tan <= PRHF_LM_MAX_TANGENTS
 * so every trial column is positive where its background is, and d vh / d c_t is prhf_vfo_jvp_f64 along den_i * B_t.
 * Per ionogram i the cost is  sum over K_i of (vh_obs - vh_model)^2 + sum_t prior_weight_t c_t^2,  K_i the frequencies
 * where vh_obs[i] is finite, a modelled NaN filled as prhf_vfo_residual_many_f64 fills it (the mean of the finite
 * |vh_model| over K_i, at least 100 km).  A pair without a virtual height has a zero JVP row: it counts in the cost and
 * not in the step.
 *
 * The rule, per ionogram (pyrayhf_amd/csrc/prhf_lm_step.h holds it, operation by operation): evaluation k = 0 is made at
 * c0 and accepted; a later one is accepted where its cost is strictly smaller (lambda / lambda_down), else rejected
 * (lambda * lambda_up; lambda stays within [1e-12, 1e12]).  An accepted evaluation whose gain is at most ftol times the
 * cost before ends with PRHF_LM_CONVERGED_F.  The step solves (A + lambda diag(max(A_tt, 1e-30))) delta = g by Cholesky,
 * A = sum d d^T + diag(w), g = sum d r - w c of the accepted point; a pivot that is not positive raises lambda, at most 8
 * times, then PRHF_LM_SINGULAR.  delta is scaled to max|delta_t| <= step_max; max|delta_t| <= xtol (max|c_t| + xtol)
 * ends with PRHF_LM_CONVERGED_X.  An ionogram with a final status is frozen: it rides along in the later launches and
 * nothing of its outputs changes.  PRHF_LM_RUNNING: max_iter evaluations were made.  PRHF_LM_NO_DATA: K_i is empty -
 * c_out is c0, cost_out, den_out and vh_out are NaN.  PRHF_LM_NO_COST: the cost at c0 is not finite.
 *
 * Arguments: the operator's, with den0 in place of den - den0_stride_elems doubles between two ionograms' columns, 0
 * for ONE background column; bmag and bpsi are one row each with PRHF_FLAG_SHARED_FIELD, else n_iono packed rows of n_alt
 * doubles; alt_stride_elems as for the operator.  basis: n_tan rows of n_alt doubles, basis_prof_stride_elems between
 * two ionograms' sets (>= n_tan * n_alt), 0 for ONE set.  vh_obs (n_iono, n_freq).  c0 (n_iono, n_tan) or NULL: zeros.
 * prior_weight (n_tan), finite, >= 0, or NULL: none.  options or NULL: the defaults of prhf_lm_options below.
 * Outputs: c_out (n_iono, n_tan), cost_out, lambda_out (n_iono) doubles; status_out, n_eval_out, n_accept_out (n_iono)
 * int32; den_out (n_iono, n_alt), the column at c_out; vh_out (n_iono, n_freq), the operator's trace of that column,
 * bit for bit; cost_history_out (n_iono, max_iter) or NULL: the accepted cost after every evaluation (a frozen
 * ionogram's entries repeat its last); state_out (n_iono, n_tan^2 + 2 n_tan) or NULL: A and g of the accepted point, A in
 * full, and the last step that was computed (zeros where none was).
 * Flags as for the JVP.  Host arrays are uploaded once and downloaded once.  With device pointers nothing visits the
 * host, and a prior_weight on the device is not checked.
 *
 * Every evaluation is four launches on the context's stream - trial columns, operator, JVP, step - enqueued back to
 * back: while the whole column fits the JVP's plan (n_alt <= 1332; above 908 levels the tangents go through in chunks of
 * fewer than eight) the call synchronises once, at its end (never with PRHF_FLAG_ASYNC).  A taller column needs the peak
 * pre-pass, whose answer can move with c: one synchronisation per evaluation.  prhf_lm_fit_counters reports what the last call did.
 * Reproducible: every output row of ionogram i depends on that ionogram's inputs and the options only - not on the
 * other ionograms, their number, or repetition; no atomics, every sum in a fixed order.  Data errors of den0 surface as
 * in the operator.  PRHF_EINVAL before any device call: null context or array, n_tan outside [1, 8], a stride shorter
 * than its row, max_iter < 1 or an option outside its range, a negative or non-finite prior_weight in host memory.
 * The cost is discontinuous where a grid frequency crosses a layer's critical frequency (E-layer cusp, foF2) between
 * two trial columns: the rule then stalls at the jump - it rejects until lambda is large - and reports what it reached.
 */
#define PRHF_LM_RUNNING     0
#define PRHF_LM_CONVERGED_F 1
#define PRHF_LM_CONVERGED_X 2
#define PRHF_LM_SINGULAR    3
#define PRHF_LM_NO_DATA     4
#define PRHF_LM_NO_COST     5
#define PRHF_LM_MAX_TANGENTS 8
typedef struct prhf_lm_options {
    int32_t max_iter;      /* evaluations, 1 ... 1048576 (2^20); default 20 */
    int32_t reserved;      /* 0 */
    double lambda0;        /* > 0; 1e-3 */
    double lambda_up;      /* > 1; 10 */
    double lambda_down;    /* >= 1; 10 */
    double step_max;       /* > 0: cap on max_t |delta_t|; 1.0 */
    double ftol;           /* >= 0; 1e-10 */
    double xtol;           /* >= 0; 1e-10 */
} prhf_lm_options;
int prhf_vfo_lm_fit_f64(prhf_ctx* ctx,
                        const double* freq_mhz, int64_t n_freq,
                        const double* den0, const double* bmag, const double* bpsi,
                        const double* alt,
                        int64_t n_iono, int64_t n_alt,
                        int64_t den0_stride_elems, int64_t alt_stride_elems,
                        const double* multiplier, int32_t n_points, int32_t mode,
                        const double* basis, int64_t n_tan, int64_t basis_prof_stride_elems,
                        const double* vh_obs, const double* c0, const double* prior_weight,
                        const prhf_lm_options* options,
                        double* c_out, double* cost_out, int32_t* status_out, int32_t* n_eval_out,
                        int32_t* n_accept_out, double* lambda_out, double* den_out, double* vh_out,
                        double* cost_history_out, double* state_out, uint32_t flags);
/* counters[0 .. PRHF_LM_FIT_COUNTERS) of the last prhf_vfo_lm_fit_f64 on this context: evaluations enqueued, timed
 * launches enqueued (see prhf_recent_kernel_ms: four per evaluation and the last column's), and the times the call made
 * the host wait for the stream - synchronisations and buffers that had to grow. */
#define PRHF_LM_FIT_COUNTERS 3
int prhf_lm_fit_counters(prhf_ctx* ctx, uint64_t* counters);

/*
 * Appleton-Hartree phase index mu and group index mu' on flat arrays of n elements.
 * Replaces: find_mu_mup (reference library.py:161-256); psi_deg in degrees.  As in the reference,
 * the isotropic formulas are used when max|Y| over the whole array is below 1e-12 (:201-207).
 * Synchronous (one device->host word decides the branch).
 */
int prhf_mu_mup_f64(prhf_ctx* ctx, const double* X, const double* Y, const double* psi_deg, int64_t n,
                    int32_t mode, double* mu_out, double* mup_out, uint32_t flags);

/*
 * Virtual heights from already-regridded arrays.  Replaces: find_vh (reference library.py:259-293):
 * vh[r] = nansum_c(mu'(X,Y,psi)[r,c] * dh[r,c]), exact 0 -> NaN, + alt_min.  X, Y, psi_deg, dh are
 * (n_rows, n_cols) row-major; the isotropic test spans the whole array as in find_mu_mup.  Synchronous.
 */
int prhf_find_vh_f64(prhf_ctx* ctx, const double* X, const double* Y, const double* psi_deg, const double* dh,
                     int64_t n_rows, int64_t n_cols, double alt_min, int32_t mode, double* vh_out,
                     uint32_t flags);

/*
 * The un-fused first half of the operator for ONE profile.  Replaces: regrid_to_nonuniform_grid
 * (reference library.py:324-438): peak truncation, reflection heights, stretched altitudes and the
 * profile sampled on them.  freq_hz in Hz (as the reference's function takes it); every output is
 * (n_freq, n_points) row-major: the reference's dict entries 'freq', 'den', 'bmag', 'bpsi', 'dist',
 * 'alt', 'crit_height' (float64) and 'ind' (int64).  IEEE arithmetic in the reference's order: the
 * outputs are bit-identical to NumPy's.  Synchronous; returns PRHF_ENEGDEN / PRHF_EPEAK0 on bad input.
 * As in the reference only the levels below the density peak (np.argmax, the first NaN ranking highest) are used:
 * at and above it only den is read, and a NaN in alt, bmag or bpsi there changes nothing; below it such a NaN is
 * PRHF_EINVAL.  n_alt <= 65535.  Bottomside limit: the levels up to the peak are held in LDS, at most 1400 of them
 * (the peak at level 1399 or lower); a column whose peak lies higher is PRHF_EINVAL.  For n_alt > 1400 the peak is
 * found first (host scan; device buffers: one small kernel and one synchronisation).
 */
int prhf_regrid_f64(prhf_ctx* ctx, const double* freq_hz, int64_t n_freq, const double* den, const double* bmag,
                    const double* bpsi, const double* alt, int64_t n_alt, const double* multiplier,
                    int32_t n_points, int32_t mode, double* out_freq, double* out_den, double* out_bmag,
                    double* out_bpsi, double* out_dist, double* out_alt, double* out_crit, int64_t* out_ind,
                    uint32_t flags);

/*
 * Residual rows of the fitting driver for n_prof candidate profiles against one observed trace.
 * Replaces: the arithmetic of residual_VH (reference library.py:660-669) applied to a batch: modeled
 * NaNs are replaced by max(nanmean|vh_model row|, 100), residual = vh_obs - vh_model, and
 * cost[p] = sum_f residual[p,f]^2 (the objective of the brute-force search, library.py:794-798).
 * vh_model (n_prof, n_freq) is normally the output of prhf_vfo_batch_f64 left on the device;
 * residual_out or cost_out may be NULL.
 */
int prhf_residual_f64(prhf_ctx* ctx, const double* vh_model, const double* vh_obs, int64_t n_prof, int64_t n_freq,
                      double* residual_out, double* cost_out, uint32_t flags);

/*
 * prhf_vfo_batch_f64 followed by prhf_residual_f64 in one call: the candidate profiles are staged once,
 * the modeled traces never leave HBM between the two kernels.  vh_out may be NULL (only residuals / costs
 * wanted); residual_out or cost_out may be NULL.  This is the whole inner loop of the reference's
 * brute-force fit (minimize_parameters, library.py:794-798: one residual_VH call per grid node) as one launch.
 */
int prhf_vfo_residual_f64(prhf_ctx* ctx, const double* freq_mhz, int64_t n_freq, const double* den,
                          const double* bmag, const double* bpsi, const double* alt, int64_t n_prof,
                          int64_t n_alt, int64_t prof_stride_elems, int64_t alt_stride_elems,
                          const double* multiplier, int32_t n_points, int32_t mode, const double* vh_obs,
                          double* vh_out, double* residual_out, double* cost_out, uint32_t flags);

/*
 * The residual stage for MANY ionograms on one common frequency grid, and the winning candidate of each, in one launch.
 * vh_obs is (n_iono, n_freq); NaN (any non-finite value) means "ionogram i has no observation at grid frequency f".
 * Per ionogram i and candidate row p of that ionogram, with K_i = { f : vh_obs[i, f] finite } and m = vh_model[p, :]:
 * the rule of prhf_residual_f64 (residual_VH, reference library.py:660-669) on the compacted pair
 * (vh_model[p, K_i], vh_obs[i, K_i]), i.e. after minimize_parameters' filter (:741-745) -
 *     fill    = max(mean of |m[f]| over f in K_i with m[f] not NaN, 100), NaN when there is no such f;
 *     r[p, f] = vh_obs[i, f] - (m[f], or fill where m[f] is NaN)   for f in K_i;   NaN for f outside K_i;
 *     cost    = sum of r^2 over K_i;   NaN when K_i is empty
 * - bit for bit what prhf_residual_f64 returns for that compacted pair.
 * best[i] is the first row with the smallest finite cost among the rows of ionogram i and best_cost[i] that cost;
 * -1 and NaN when no cost of the ionogram is finite (or it has no row).
 * Two layouts:
 *   own candidates     ionogram_of_row (n_rows) int32, non-decreasing, values in [0, n_iono): row p belongs to that
 *                      ionogram (groups may be ragged or empty).  residual_out (n_rows, n_freq) or NULL, cost_out
 *                      (n_rows), best_out (n_iono) GLOBAL row indices, best_cost_out (n_iono).
 *   shared candidates  ionogram_of_row == NULL: every row is a candidate of every ionogram.  residual_out must be
 *                      NULL, cost_out is (n_iono, n_rows), best_out (n_iono) candidate indices.
 * cost_out, best_out and best_cost_out are required.  n_freq <= 4096; n_rows, n_iono < 2^31; at most 2^36 pairs.
 * Host buffers: an ionogram_of_row entry outside [0, n_iono) or below its predecessor is PRHF_EINVAL.  Device buffers
 * (PRHF_FLAG_DEVICE_PTRS) are not inspected by the host: a row whose entry is out of range gets a NaN cost (and NaN
 * residuals) and nothing outside vh_obs is read; no error is raised for it.  Flags: PRHF_FLAG_DEVICE_PTRS,
 * PRHF_FLAG_ASYNC (device pointers only).
 */
int prhf_residual_many_f64(prhf_ctx* ctx, const double* vh_model, int64_t n_rows, const double* vh_obs, int64_t n_iono,
                           int64_t n_freq, const int32_t* ionogram_of_row, double* residual_out, double* cost_out,
                           int64_t* best_out, double* best_cost_out, uint32_t flags);

/*
 * prhf_vfo_batch_f64 followed by prhf_residual_many_f64 in one call, the twin of prhf_vfo_residual_f64: the operator
 * runs once on the n_prof profiles and the n_freq grid frequencies (with shared candidates: once for all ionograms),
 * the modeled traces never leave HBM.  freq_mhz is the common grid: finite (PRHF_EINVAL otherwise, host buffers),
 * and positive and ascending if the traces are to mean anything.  vh_out (n_prof, n_freq) may be NULL.  The other
 * arguments and flags (PRHF_FLAG_DEVICE_PTRS, PRHF_FLAG_ASYNC, PRHF_FLAG_GRID_STABLE, PRHF_FLAG_SHARED_FIELD) are
 * those of prhf_vfo_residual_f64 and prhf_residual_many_f64 (n_rows = n_prof).  The operator's values are those of
 * prhf_vfo_batch_f64 on the same arguments.
 */
int prhf_vfo_residual_many_f64(prhf_ctx* ctx, const double* freq_mhz, int64_t n_freq, const double* den,
                               const double* bmag, const double* bpsi, const double* alt, int64_t n_prof,
                               int64_t n_alt, int64_t prof_stride_elems, int64_t alt_stride_elems,
                               const double* multiplier, int32_t n_points, int32_t mode, const double* vh_obs,
                               int64_t n_iono, const int32_t* ionogram_of_row, double* vh_out, double* residual_out,
                               double* cost_out, int64_t* best_out, double* best_cost_out, uint32_t flags);

/*
 * Stratified Snell's-law ray tracing over a flat Earth for n_rays rays (one wavefront each).
 * Replaces: trace_ray_cartesian_snells (reference library.py:1096-1268) with tan_from_mu_scalar
 * (:1034-1062) and find_turning_point (:1065-1093).  Ray r has frequency freq_hz[r] [Hz], launch elevation
 * elevation_deg[r] above the horizon and uses profile profile_index[r] (NULL: profile 0) of the
 * (n_prof, n_alt) columns; a ground level at z = 0 is inserted when alt[0] > 0, as in the reference.
 * out is (n_rays, 8): group_path_km, group_delay_sec, x_midpoint, z_midpoint, ground_range_km (the
 * reference's dict entries; its x_apex_km / z_apex_km equal the midpoint), then x and z of the turning
 * point and the number of path nodes.  The midpoint is the path node before the apex: the exact-arithmetic answer of
 * the reference's search (library.py:1248-1252), whose own rounding lands there for two rays in three and on the apex
 * for the third.  Arithmetic (prhf_ctx_set_math): PRHF_MATH_FAITHFUL evaluates mu and mu' of every level in the
 * reference's operation order (reference-run rays to 1e-12); the default evaluates levels far from reflection and from
 * the ray's turning point in the reduced algebra (within 1e-10 of the former; spherical rays at the edge of a skip zone, one
 * in a few million of a random set: up to 3e-10).  Rays that never turn give NaN (node count 0).  path_x / path_z
 * (optional, (n_rays, path_stride), path_stride >= 2 n_alt + 1) receive the reference's 'x' and 'z'
 * arrays padded with NaN.  Synchronous; PRHF_ENEGDEN on a negative density; PRHF_EINVAL when a
 * profile_index lies outside [0, n_prof) - checked on the host for host buffers and by the kernel for
 * device-resident ones (that ray's outputs are NaN, no memory outside the columns is read).
 */
int prhf_snell_cartesian_f64(prhf_ctx* ctx, const double* freq_hz, const double* elevation_deg,
                             const int64_t* profile_index, int64_t n_rays, const double* den, const double* bmag,
                             const double* bpsi, const double* alt, int64_t n_prof, int64_t n_alt,
                             int64_t alt_stride_elems, int32_t mode, double* out, double* path_x, double* path_z,
                             int64_t path_stride, uint32_t flags);

/*
 * The same over a spherical Earth (Bouguer's law mu r sin(theta) = const, adaptive midpoint sub-steps towards
 * the apex).  Replaces: trace_ray_spherical_snells (reference library.py:1460-1713); the four controls are
 * its R_E (6371 km), dz_target_km (1.0), apex_boost (200.0) and max_substeps (400).  Outputs as for the
 * flat-Earth tracer, with x = R_E * phi.
 */
int prhf_snell_spherical_f64(prhf_ctx* ctx, const double* freq_hz, const double* elevation_deg,
                             const int64_t* profile_index, int64_t n_rays, const double* den, const double* bmag,
                             const double* bpsi, const double* alt, int64_t n_prof, int64_t n_alt,
                             int64_t alt_stride_elems, int32_t mode, double earth_radius_km, double dz_target_km,
                             double apex_boost, int32_t max_substeps, double* out, double* path_x, double* path_z,
                             int64_t path_stride, uint32_t flags);

/*
 * Fans of rays: many elevations per (profile, frequency).  The tracers above evaluate the Appleton-Hartree index
 * level by level for every ray (library.py:1184-1189 / :1566-1571) although it depends on the profile and the
 * frequency only; here the n_groups (profile, frequency) groups get their tables once - mu and mu' of every level
 * (one thread per group and level, the reference's operation order) and the list of the levels with a finite mu,
 * compacted, with the running minimum of the turning-point criterion, so that a ray finds its bracket
 * (library.py:1085-1093 / :1598-1603: the first pair of consecutive finite levels the invariant falls between) with
 * two loads - and every ray reads the tables of its group: group_freq_hz[g] [Hz], group_profile_index[g] (NULL:
 * profile 0), ray_group[r] in [0, n_groups), elevation_deg[r].  geometry 0: flat Earth (the four controls are
 * ignored), 1: spherical Earth.  Outputs, paths, flags and errors as for the per-ray calls; the results are those of
 * the per-ray calls on the same rays in PRHF_MATH_FAITHFUL to 1e-15 (other orders of summation).  PRHF_EINVAL when the
 * tables (n_groups x (n_alt + 1) x 44 bytes in the context's scratch) would exceed 64 GiB, and - checked on the host
 * for host buffers, by the kernel for device-resident arrays (reported at the synchronisation) - when a ray_group or
 * a profile index is out of range.
 */
int prhf_snell_fan_f64(prhf_ctx* ctx, int32_t geometry, const double* group_freq_hz,
                       const int64_t* group_profile_index, int64_t n_groups, const int64_t* ray_group,
                       const double* elevation_deg, int64_t n_rays, const double* den, const double* bmag,
                       const double* bpsi, const double* alt, int64_t n_prof, int64_t n_alt,
                       int64_t alt_stride_elems, int32_t mode, double earth_radius_km, double dz_target_km,
                       double apex_boost, int32_t max_substeps, double* out, double* path_x, double* path_z,
                       int64_t path_stride, uint32_t flags);

/*
 * Point-to-point homing (oblique ionograms): the rays of a (profile, frequency) group that land at a given ground
 * range.  No counterpart in the reference; the definition is DESIGN.md section 4.8.  Groups as for
 * prhf_snell_fan_f64 (group_freq_hz[g], group_profile_index[g] or NULL); link l is the pair (link_group[l] in
 * [0, n_groups), link_range_km[l]); scan_elevation_deg holds n_scan >= 2 strictly increasing elevations.  Scan: D_i,
 * the ground range of the group's fan ray at scan node i - the bits prhf_snell_fan_f64 gives for that ray.  Brackets
 * of a link with target t, numbered in ascending elevation: the intervals i with D_i and D_i+1 finite and (D_i - t),
 * (D_i+1 - t) of opposite signs or D_i == t; D_(n_scan-1) == t is a bracket of no width; a NaN target has none.
 * Tangential contacts without a sign change on the scan grid are not found: what is found is a function of the grid.
 * Each of the first max_roots (1 .. 64) brackets is narrowed by at most max_iter (1 .. 128) rays of the group that
 * never leave it (Illinois steps, a bisection whenever a step did not halve the bracket) and gets row
 * (l, rank) of out (n_links, max_roots, 11): elevation_deg, status, scan_index (the interval), then the eight outputs
 * of prhf_snell_cartesian_f64 for the result ray.  status 0: a ray with |D - t| <= range_tol_km (>= 0, finite) was
 * found - a scan node counts - and is the result; 1: the bracket cannot be split any further in float64, or max_iter
 * is spent (a jump of D(e), not a crossing); 2: a ray inside the bracket does not turn; for 1 and 2 the result is the
 * ray with the smallest miss among the bracket's two scan nodes and the rays tried.  Rows without a bracket are NaN
 * with status -1; n_brackets[l] counts every bracket of the link, those beyond max_roots included.  The rows do not
 * depend on scheduling.  geometry, the four spherical controls, mode, flags and errors as for prhf_snell_fan_f64;
 * synchronous.  PRHF_EINVAL for a control outside the ranges above, for tables beyond 64 GiB, for a host scan grid
 * that does not increase strictly and for a link_group or profile index out of range - checked on the host for host
 * buffers, by the kernels for device-resident arrays (those links get NaN rows and no bracket; no memory outside the
 * columns is read).
 */
int prhf_snell_home_f64(prhf_ctx* ctx, int32_t geometry, const double* group_freq_hz,
                        const int64_t* group_profile_index, int64_t n_groups, const int64_t* link_group,
                        const double* link_range_km, int64_t n_links, const double* scan_elevation_deg, int64_t n_scan,
                        const double* den, const double* bmag, const double* bpsi, const double* alt, int64_t n_prof,
                        int64_t n_alt, int64_t alt_stride_elems, int32_t mode, double earth_radius_km,
                        double dz_target_km, double apex_boost, int32_t max_substeps, double range_tol_km,
                        int32_t max_iter, int32_t max_roots, double* out, int64_t* n_brackets, uint32_t flags);

/*
 * Skip distance: the smallest ground range any ray of a (profile, frequency) group reaches on a scan grid.  No
 * counterpart in the reference; the definition is DESIGN.md section 4.10.  Groups, columns, geometry, the four spherical
 * controls, mode, flags and errors as for prhf_snell_home_f64; scan_elevation_deg holds n_scan >= 1 strictly increasing
 * elevations.  Per group, in float64 without contraction:
 *   Scan: D_i, ground_range_km of the group's fan ray at scan node i (the bits prhf_snell_fan_f64 gives), NaN for a ray
 *   that does not turn.
 *   Node: i* = the FIRST index that attains the minimum over the finite D_i.  None finite: status -1, every output NaN
 *   (scan_index -1, n_evals and the node count 0).
 *   Edge: i* == 0, i* == n_scan - 1, or a neighbour of i* that is not finite: status 1, the result is the scan node's
 *   own ray, bracket_deg NaN ("no skip zone inside the scan", or "the minimum sits beside penetration").
 *   Refine otherwise: a = e_(i*-1), b = e_(i*), c = e_(i*+1), Db = D_(i*), g = 0.3819660112501051; per trip, in this order:
 *     c - a <= elev_tol_deg: status 0, stop;
 *     right = (c - b) >= (b - a); x = right ? b + g * (c - b) : b - g * (b - a) (difference, product, sum: one rounding each);
 *     unless a < x < c and x != b: status 0, stop (the doubles are exhausted);
 *     max_iter (1 .. 128) rays traced already: status 3, stop;
 *     Dx = ground_range_km of the group's ray at x; not finite: status 2, stop (a ray inside the bracket escapes);
 *     Dx < Db: the old b becomes a (right) or c (left), b = x, Db = Dx; otherwise x becomes c (right) or a (left): a tie keeps b.
 *   The result is the ray at b for every status; a b that is still the scan node is traced once more for its outputs
 *   and that ray is not counted.
 * out is (n_groups, 13): elevation_deg (b), status, scan_index (i*), bracket_deg (c - a at the end), n_evals (rays
 * traced by the search, an escaping one included), then the eight outputs of prhf_snell_cartesian_f64 for the result ray -
 * the skip distance is its ground_range_km, out[.., 9].  No result depends on how many groups share the call or on
 * scheduling.  elev_tol_deg is finite and >= 0.  Synchronous; one call, no host round trip between its kernels.
 */
int prhf_snell_skip_f64(prhf_ctx* ctx, int32_t geometry, const double* group_freq_hz,
                        const int64_t* group_profile_index, int64_t n_groups, const double* scan_elevation_deg,
                        int64_t n_scan, const double* den, const double* bmag, const double* bpsi, const double* alt,
                        int64_t n_prof, int64_t n_alt, int64_t alt_stride_elems, int32_t mode, double earth_radius_km,
                        double dz_target_km, double apex_boost, int32_t max_substeps, double elev_tol_deg,
                        int32_t max_iter, double* out, uint32_t flags);

/*
 * MUF of a link (junction frequency, the nose of the oblique ionogram): the frequency at which the skip distance
 * reaches the link's ground range.  DESIGN.md section 4.10.  Link l is the pair (link_profile_index[l] in [0, n_prof), or
 * profile 0 for a NULL array; link_range_km[l] = t).  S(f) is the skip distance of prhf_snell_skip_f64 for that column,
 * frequency f, mode, scan grid and controls, +inf when its status is -1.  0 < f_lo_hz < f_hi_hz, both finite.
 *   status -1: t is NaN.  2: S(f_lo) > t, unreachable even at f_lo.  Both: every other output NaN.
 *   status 1: S(f_hi) <= t, the link is open at f_hi: muf_hz = f_hi with its skip row, f_above_hz NaN.
 *   status 0: S(f_lo) <= t < S(f_hi); lo = f_lo, hi = f_hi, then n_bisect (1 .. 64) trips: m = lo + 0.5 * (hi - lo);
 *   a trip whose m is not strictly inside (lo, hi) changes nothing; S(m) <= t: lo = m, otherwise hi = m.
 *   muf_hz = lo, f_above_hz = hi: S(muf_hz) <= t < S(f_above_hz) whether or not S is monotone - the rule says which
 *   crossing is found.
 * out is (n_links, 16): muf_hz, f_above_hz, status, then the 13 values of the skip row at muf_hz.  The per-trip
 * kernels (the links' next frequencies into the device-side group table, tables, scan, refine, decide) are enqueued on
 * one stream and the call waits once, at its end.  Arrays are host memory, or device memory with PRHF_FLAG_DEVICE_PTRS.
 */
int prhf_snell_muf_f64(prhf_ctx* ctx, int32_t geometry, const int64_t* link_profile_index, const double* link_range_km,
                       int64_t n_links, double f_lo_hz, double f_hi_hz, int32_t n_bisect,
                       const double* scan_elevation_deg, int64_t n_scan, const double* den, const double* bmag,
                       const double* bpsi, const double* alt, int64_t n_prof, int64_t n_alt, int64_t alt_stride_elems,
                       int32_t mode, double earth_radius_km, double dz_target_km, double apex_boost, int32_t max_substeps,
                       double elev_tol_deg, int32_t max_iter, double* out, uint32_t flags);

/*
 * 2-D refractive-index fields mu(a0, a1) for the gradient tracer: node records.
 * Replaces: the grid half of build_refractive_index_interpolator_cartesian / _spherical (reference library.py:1801-1835,
 * :1879-1921) and of build_mup_function (:1978-2014).  mu and mup are n_fields planes of (n0, n1) values each,
 * row-major (host memory, or device memory with PRHF_FLAG_DEVICE_PTRS); axis0 (n0) and axis1 (n1) are HOST memory in
 * every flag combination and strictly increasing - altitude z and distance x of a Cartesian field, r = R_E + z and
 * phi = x / R_E of a spherical one (:1887-1888).  records is DEVICE memory in every flag combination,
 * (n_fields, n0, n1, 4) doubles: {mu, d mu / d a1, d mu / d a0, mu'} per node, the derivatives
 * np.gradient(mu, axis0, axis1, edge_order = 1 or 2) (:1823, :1908) in NumPy's formulas and operation order - its
 * scalar-spacing branch along an axis whose np.diff values are all equal, its three-point branch otherwise -
 * bit-identical to NumPy, NaNs included.  An axis needs edge_order + 1 values; n0 + n1 <= 8000.  Synchronous.
 */
int prhf_field_pack_f64(prhf_ctx* ctx, const double* mu, const double* mup, int64_t n_fields, int64_t n0, int64_t n1,
                        const double* axis0, const double* axis1, int32_t edge_order, double* records, uint32_t flags);

/*
 * The fields at n points (p0[i], p1[i]) along (axis0, axis1); field_index[i] (NULL: field 0) chooses the field.
 * Replaces: the RegularGridInterpolator calls behind eval_refractive_index_and_grad, n_and_grad_rphi and mup_func
 * (reference library.py:939-950, :1716-1752, :1987-2013) with method="linear", bounds_error=False: the cell i with
 * g[i] <= v < g[i + 1] (the last cell for v = g[n - 1]); all four corner products are formed, so a NaN corner gives
 * NaN even at weight 0; a point outside the hull gets fill_n (mu), fill_grad (both derivatives), fill_mup; a NaN
 * coordinate gives NaN.  Any of the four outputs (n each) may be NULL.  records, axes and limits as for
 * prhf_field_pack_f64; the point arrays and outputs are host memory, or device memory with PRHF_FLAG_DEVICE_PTRS.
 * PRHF_EINVAL for a field_index outside [0, n_fields): checked on the host for host buffers, by the kernel for
 * device-resident ones (that point's outputs are NaN, no memory outside the records is read).  Synchronous.
 */
int prhf_field_sample_f64(prhf_ctx* ctx, const double* records, int64_t n_fields, int64_t n0, int64_t n1,
                          const double* axis0, const double* axis1, const double* p0, const double* p1,
                          const int64_t* field_index, int64_t n, double fill_n, double fill_grad, double fill_mup,
                          double* out_n, double* out_d1, double* out_d0, double* out_mup, uint32_t flags);

/*
 * Ray tracing through a horizontally varying mu(x, z) over a flat Earth, n_rays rays in one launch (one per lane).
 * Replaces: trace_ray_cartesian_gradient (reference library.py:1270-1457) with ray_rhs_cartesian (:953-1006) and the
 * event helpers (:1009-1031).  records: Cartesian records of prhf_field_pack_f64 on (z_axis (nz), x_axis (nx)).  Ray r
 * starts at (x0_km[r], z0_km[r]) with elevation_deg[r] above the horizon in field ray_field[r] (NULL: field 0).  The
 * controls are the reference's (:1278-1291; max_step_km = +inf for None; z_min_km is unused there and absent here);
 * fill_n / fill_grad / fill_mup are the interpolators' fill values outside the grid (:1764-1766, :1938).  The system
 * dr/ds = v, dv/ds = (grad mu - (grad mu . v) v) / mu is integrated by the Dormand-Prince 5(4) pair with the
 * controller solve_ivp(method="RK45") documents; the four terminal events (+ -> -) are located on the step's dense
 * output and the event point is the last node.
 * out is (n_rays, 12): group_path_km, group_delay_sec, x_midpoint, z_midpoint, ground_range_km, x_apex_km, z_apex_km
 * (the reference's dict entries, :1405-1441), status (0 ground, 1 domain, 2 length, 3 failure: the step fell below
 * 10 ulp of s, :1391-1398), nodes, right-hand-side calls, rejected steps, 0.  path_t .. path_vz (all five or none,
 * (n_rays, path_stride) each) receive the reference's 't', 'x', 'z', 'vx', 'vz' padded with NaN; PRHF_EINVAL when a
 * ray has more nodes than path_stride (nothing is truncated: ask again with out[.., 8] nodes).  Ray arrays, out and
 * paths are host memory, or device memory with PRHF_FLAG_DEVICE_PTRS.  PRHF_EINVAL for a ray_field outside
 * [0, n_fields): on the host for host buffers, by the kernel for device-resident ones (NaN outputs, no memory outside
 * the records is read).  Synchronous.
 */
int prhf_trace_gradient_f64(prhf_ctx* ctx, const double* records, int64_t n_fields, int64_t nz, int64_t nx,
                            const double* z_axis, const double* x_axis, const double* x0_km, const double* z0_km,
                            const double* elevation_deg, const int64_t* ray_field, int64_t n_rays, double s_max_km,
                            double rtol, double atol, double max_step_km, double z_ground_km, double z_max_km,
                            double x_min_km, double x_max_km, int32_t renormalize_every, double fill_n, double fill_grad,
                            double fill_mup, double* out, double* path_t, double* path_x, double* path_z, double* path_vx,
                            double* path_vz, int64_t path_stride, uint32_t flags);

/*
 * The same over a spherical Earth: mu(r, phi), n_rays rays in one launch (one per lane).
 * Replaces: trace_ray_spherical_gradient (reference library.py:2128-2337) with rhs_spherical (:2094-2125), except its
 * stop conditions: the reference hands the Cartesian event helpers the state [r, phi, v_r, v_phi] (:2239-2243 with
 * :1009-1031), which tests phi against radii and r against angles, so that none can fire.  The four terminal events
 * (+ -> -) here are ground r - (earth_radius_km + z_ground_km) - 1e-3, top r_max_km - r, left phi - phi_min, right
 * phi_max - phi.  records: spherical records of prhf_field_pack_f64 on (r_axis (nr) =
 * R_E + z, phi_axis (nphi) = x / R_E).  Ray r starts at r = earth_radius_km + z0_km[r], phi = x0_km[r] / earth_radius_km
 * with (v_r, v_phi) = (sin, cos)(elevation_deg[r]) (:2230-2234).  The system is dr/ds = v_r, dphi/ds = v_phi / r,
 * dv_r/ds = (mu_r - g v_r) / mu + v_phi^2 / r, dv_phi/ds = (mu_phi / r - g v_phi) / mu - v_r v_phi / r with
 * g = mu_r v_r + (mu_phi / r) v_phi, zero for a non-finite or non-positive mu; renormalize_every is accepted and, as in
 * the reference - whose renormalisation rebinds local names after the derivatives are formed -, changes nothing.
 * Integrator, controller, event location, out (n_rays, 12), status codes, path_stride rule, flags and PRHF_EINVAL rules
 * are those of prhf_trace_gradient_f64, with x = earth_radius_km * phi and z = r - earth_radius_km in x_midpoint,
 * z_midpoint, ground_range_km, x_apex_km and z_apex_km; a chord is sqrt(dr^2 + (r_mid dphi)^2) (:2291-2294), mu' is
 * sampled at (earth_radius_km + z_mid, x_mid / earth_radius_km) of the chord's x and z midpoints (:2299-2301), and the
 * midpoint is the node searchsorted(cumsum(ds), group_path_km / 2) (:2309-2313; NaN for a path of length 0), the sums
 * taken in node order.  path_t, path_r, path_phi, path_v_r, path_v_phi (all five or none) receive the reference's 't',
 * 'r', 'phi', 'v_r', 'v_phi'.  PRHF_EINVAL also for an earth_radius_km that is not positive and finite.  Synchronous.
 */
int prhf_trace_gradient_spherical_f64(prhf_ctx* ctx, const double* records, int64_t n_fields, int64_t nr, int64_t nphi,
                                      const double* r_axis, const double* phi_axis, const double* x0_km,
                                      const double* z0_km, const double* elevation_deg, const int64_t* ray_field,
                                      int64_t n_rays, double earth_radius_km, double s_max_km, double rtol, double atol,
                                      double max_step_km, double z_ground_km, double r_max_km, double phi_min,
                                      double phi_max, int32_t renormalize_every, double fill_n, double fill_grad,
                                      double fill_mup, double* out, double* path_t, double* path_r, double* path_phi,
                                      double* path_v_r, double* path_v_phi, int64_t path_stride, uint32_t flags);

/*
 * Point-to-point homing through a horizontally varying mu (oblique ionograms of a tilted ionosphere): the rays of a
 * transmitter that land at a given coordinate, for the gradient tracers of both geometries.  No counterpart in the
 * reference; the definition is DESIGN.md section 4.9, which carries section 4.8's semantics over.  geometry 0: the
 * rays of prhf_trace_gradient_f64 (top, left, right = z_max_km, x_min_km, x_max_km; earth_radius_km ignored), 1: those
 * of prhf_trace_gradient_spherical_f64 (top, left, right = r_max_km, phi_min, phi_max).  records, n_fields, n0, n1,
 * axis0, axis1 (HOST memory), the controls s_max_km .. renormalize_every and the fills are that tracer's.
 * Group g is a transmitter: field group_field[g] in [0, n_fields), launch point (group_x0_km[g], group_z0_km[g]).  Link l
 * is the pair (link_group[l] in [0, n_groups), link_target_km[l]); the target is compared with the tracer's own
 * ground_range_km (x of the landing node, earth_radius_km * phi in the spherical case; finite only for status ground).
 * scan_elevation_deg holds n_scan >= 2 strictly increasing elevations (beyond 90 degrees is legal, as in the tracers).
 *   Scan: D_i, ground_range_km of the group's ray at scan node i under the call's controls - the bits the tracer
 * gives for that ray.  One scan serves all targets of a group.
 *   Brackets of a link with target t, ranked in ascending elevation: the intervals i with D_i and D_i+1 finite and
 * (D_i - t), (D_i+1 - t) of opposite signs, or D_i == t; D_(n_scan-1) == t is a bracket of no width; a NaN target has
 * none.  What is found is a function of the scan grid.  n_brackets[l] counts every bracket of the link.
 *   Refine: each of the first max_roots (1 .. 64) brackets, in float64 without contraction:
 *     lo = e_i, hi = e_i+1, f_lo = D_i - t, f_hi = D_i+1 - t (no width: hi = lo, f_hi = f_lo); g_lo = f_lo, g_hi = f_hi;
 *     best = the end with the smaller |f| (lo on a tie), best_miss = min(|f_lo|, |f_hi|); side = 0, bisect = false;
 *     best_miss <= range_tol_km: status 0, no ray is traced.  Else at most max_iter (1 .. 128) times:
 *       mid = lo + 0.5 * (hi - lo); unless lo < mid < hi: status 1, stop;
 *       x = mid; if not bisect: xs = lo - g_lo * ((hi - lo) / (g_hi - g_lo)), and x = xs if lo < xs < hi;
 *       D = ground_range_km of the group's ray at x; not finite: status 2, stop;
 *       f = D - t; |f| < best_miss: best = x, best_miss = |f|; |f| <= range_tol_km: status 0, stop;
 *       width = hi - lo; if (f < 0) == (f_lo < 0): lo = x, f_lo = g_lo = f, and g_hi = 0.5 * g_hi if side == -1; side = -1;
 *       else: hi = x, g_hi = f, and g_lo = 0.5 * g_lo if side == +1; side = +1;
 *       bisect = (hi - lo) > 0.5 * width;
 *     max_iter rays traced without a stop: status 1.
 * A bracket stops as soon as its status is decided.  status 0: a ray with |D - t| <= range_tol_km (>= 0, finite) was
 * found, a scan node counts; 1: the bracket cannot be split further in float64 or max_iter is spent (a jump of D(e));
 * 2: a ray inside the bracket does not land.  The result of a bracket is `best`: for 1 and 2 the ray with the smallest
 * miss among the bracket's two scan nodes and the rays tried.
 *   out is (n_links, max_roots, 15); row (l, rank): elevation_deg, status, scan_index (the interval i), then the twelve
 * outputs of the tracer for the result ray, bit-identical to what the tracer returns for that elevation, launch point,
 * field and controls (the full ray: midpoint, apex and delay included).  Rows without a bracket are NaN with status -1.
 * No result depends on scheduling.  D(e) of these tracers is not continuous down to rounding (the step controller
 * turns last-bit differences into other step sequences: about 3e-3 km at the default tolerances), so a range_tol_km
 * below that yields status 1, not a better ray.
 * Group, link and scan arrays, out and n_brackets are host memory, or device memory with PRHF_FLAG_DEVICE_PTRS.
 * PRHF_EINVAL for a null context (before anything else), a control outside its range, a host scan grid that does not
 * increase strictly, a range_tol_km that is negative or not finite, an earth_radius_km that is not positive and finite
 * (geometry 1), and a link_group or group_field out of range - checked on the host for host buffers, by the kernels
 * for device-resident arrays (those links get NaN rows and no bracket, no memory outside the records is read, and the
 * error is reported at the synchronisation).  Synchronous.
 */
int prhf_gradient_home_f64(prhf_ctx* ctx, int32_t geometry, const double* records, int64_t n_fields, int64_t n0,
                           int64_t n1, const double* axis0, const double* axis1, const int64_t* group_field,
                           const double* group_x0_km, const double* group_z0_km, int64_t n_groups,
                           const int64_t* link_group, const double* link_target_km, int64_t n_links,
                           const double* scan_elevation_deg, int64_t n_scan, double earth_radius_km, double s_max_km,
                           double rtol, double atol, double max_step_km, double z_ground_km, double top, double left,
                           double right, int32_t renormalize_every, double fill_n, double fill_grad, double fill_mup,
                           double range_tol_km, int32_t max_iter, int32_t max_roots, double* out, int64_t* n_brackets,
                           uint32_t flags);

/* Diagnostics of the context's last prhf_gradient_home_f64: counters[0] brackets refined (used rows), [1] rays the
 * refine lanes traced, [2] ray slots (64 per trip of a refine wavefront's loop), [3] refine wavefronts with work.
 * Lane utilisation of the refinement = [1] / [2].  No device call. */
int prhf_gradient_home_counters(prhf_ctx* ctx, uint64_t* counters);

/*
 * Multi-hop rays through a horizontally varying mu: a ray that lands is reflected off the ground and traced on, n_rays
 * chains of n_hops (1 .. 16) hops in one launch, a chain per lane.  No counterpart in the reference (over a stratified
 * ionosphere n hops are n copies of one hop; through a tilt they are not); the definition is DESIGN.md section 4.12.
 * geometry, records .. axis1, the ray arrays, earth_radius_km, the controls s_max_km .. renormalize_every (top, left,
 * right as in prhf_gradient_home_f64) and the fills are the tracer's of that geometry.  The chain of ray r, every hop
 * under the call's controls:
 *   hop 0 launches at (x0_km[r], z0_km[r]) with elevation_deg[r];
 *   hop h + 1 exists only if h + 1 < n_hops and hop h ended with status 0 (ground);
 *   it launches at x = ground_range_km of hop h (the x of its landing node, those bits), z = z_ground_km, with the
 *   elevation atan2(-v_vert, v_horiz) * (180.0 / 3.141592653589793) - one multiplication by that constant -, where
 *   (v_horiz, v_vert) = (vx, vz) of hop h's last path node in a Cartesian call and (v_phi, v_r) in a spherical one: the
 *   bits the tracer stores in path_vx / path_vz (path_v_r / path_v_phi).  This is specular reflection off the ground;
 *   the launch normalises the direction again.  An elevation beyond 90 degrees (a ray travelling backwards) is legal.
 *   Every hop has the whole s_max_km and starts the step controller and the right-hand-side counter afresh, as a tracer
 *   call does.  The ground event sits at z_ground_km + 1e-3: a hop launched at z_ground_km starts below it, rising.
 * out is (n_rays, n_hops, 15): launch x, launch z, launch elevation, then the tracer's twelve.  Every used hop row is
 * bit for bit what prhf_trace_gradient_f64 / prhf_trace_gradient_spherical_f64 returns for that row's launch point,
 * elevation, field and controls.  Rows behind the first hop that does not land are unused: NaN, status -1, nodes,
 * right-hand-side calls, rejected steps and the last column 0.  path_t .. path_vb (all five or none) are
 * (n_rays * n_hops, path_stride): row r * n_hops + h holds the tracer's path of hop h, NaN where unused; PRHF_EINVAL when
 * a hop has more nodes than path_stride, as in the tracers.  Host memory, or device memory with PRHF_FLAG_DEVICE_PTRS.
 * PRHF_EINVAL for a null context (before anything else), n_hops outside 1 .. 16, a geometry other than 0 or 1, and
 * whatever the tracer of that geometry refuses - a ray_field out of range on the host for host buffers, by the kernel
 * for device-resident ones (NaN rows, no memory outside the records is read).  Synchronous.
 */
int prhf_trace_gradient_hops_f64(prhf_ctx* ctx, int32_t geometry, const double* records, int64_t n_fields, int64_t n0,
                                 int64_t n1, const double* axis0, const double* axis1, const double* x0_km,
                                 const double* z0_km, const double* elevation_deg, const int64_t* ray_field, int64_t n_rays,
                                 double earth_radius_km, double s_max_km, double rtol, double atol, double max_step_km,
                                 double z_ground_km, double top, double left, double right, int32_t renormalize_every,
                                 double fill_n, double fill_grad, double fill_mup, int32_t n_hops, double* out,
                                 double* path_t, double* path_a, double* path_b, double* path_va, double* path_vb,
                                 int64_t path_stride, uint32_t flags);

/*
 * Homing on the landing of hop n_hops - 1 (2F, 3F .. modes of a long link): prhf_gradient_home_f64 with D(e) the
 * ground_range_km of the last hop of prhf_trace_gradient_hops_f64's chain at elevation e, NaN unless all n_hops
 * (1 .. 16) hops land.  Scan, brackets, the refine rule, statuses, n_brackets, flags and every PRHF_EINVAL rule are
 * that call's, unchanged; so are all arguments before n_hops.  out is (n_links, max_roots, 3 + 15 * n_hops):
 * elevation_deg, status, scan_index, then the n_hops hop rows of prhf_trace_gradient_hops_f64 for the result chain, bit
 * for bit what that call returns at elevation_deg.  Rows without a bracket: elevation and scan_index NaN, status -1, hop
 * rows unused as that call writes them.  With n_hops = 1 the call finds what prhf_gradient_home_f64 finds.
 * prhf_gradient_home_counters reports this call as well.  PRHF_EINVAL also for n_hops outside 1 .. 16.  Synchronous.
 */
int prhf_gradient_hop_home_f64(prhf_ctx* ctx, int32_t geometry, const double* records, int64_t n_fields, int64_t n0,
                               int64_t n1, const double* axis0, const double* axis1, const int64_t* group_field,
                               const double* group_x0_km, const double* group_z0_km, int64_t n_groups,
                               const int64_t* link_group, const double* link_target_km, int64_t n_links,
                               const double* scan_elevation_deg, int64_t n_scan, double earth_radius_km, double s_max_km,
                               double rtol, double atol, double max_step_km, double z_ground_km, double top, double left,
                               double right, int32_t renormalize_every, double fill_n, double fill_grad, double fill_mup,
                               double range_tol_km, int32_t max_iter, int32_t max_roots, int32_t n_hops, double* out,
                               int64_t* n_brackets, uint32_t flags);

/*
 * Fields of many frequencies built on the device: the records (n_freq, n0, n1, 4) of
 * prhf_field_pack_f64 for the frequencies freq_hz (n_freq) of ONE 2-D ionosphere den, bmag, bpsi (n0, n1) - electron
 * density [m^-3], |B| [T], angle [deg] - with no host round trip inside the call.  Per node and frequency, in float64
 * without contraction, each operation rounded once: f_N = sqrt(den) c_p, X = (f_N f_N) / (f f), Y = (g_p |B|) / f, then mu
 * and mu' in the faithful tier's arithmetic, or the isotropic formulas when that frequency's field is isotropic:
 * nanmax|Y| < 1e-12 (an all-NaN Y counts as magnetised), prhf_mu_mup_f64's decision on that frequency's Y array, taken
 * here from nanmax|B|, found once per call.  f squared is the PRODUCT f f - what the reference's find_X gives for an
 * array of frequencies; its scalar f ** 2 (libm pow) differs in the last bit for about one frequency in a thousand.
 * Then np.gradient as prhf_field_pack_f64 computes it (edge_order 1 or 2).  A negative density gives NaN as sqrt does.
 * den, bmag, bpsi, freq_hz and, when given, mu_out and mup_out (n_freq, n0, n1; both or neither) are host memory, or
 * device memory with PRHF_FLAG_DEVICE_PTRS; axis0 and axis1 are host memory; records is device memory.
 * PRHF_EINVAL for a null context (before anything else), a null array, a bad mode, edge_order, shape or axis;
 * PRHF_ENEGDEN for a negative density in a host array.  Synchronous.
 */
int prhf_field_build_f64(prhf_ctx* ctx, const double* den, const double* bmag, const double* bpsi, int64_t n0, int64_t n1,
                         const double* axis0, const double* axis1, const double* freq_hz, int64_t n_freq, int32_t mode,
                         int32_t edge_order, double* records, double* mu_out, double* mup_out, uint32_t flags);

/*
 * Skip distance through a horizontally varying mu: the least ground_range_km over the elevations of a transmitter's
 * rays, for the gradient tracers of both geometries.  No counterpart in the reference; DESIGN.md section 4.11 carries the
 * rule of section 4.10 (prhf_snell_skip_f64) over unchanged.  geometry, records .. axis1, the groups (field, launch
 * point), the controls s_max_km .. renormalize_every and the fills are prhf_gradient_home_f64's.  scan_elevation_deg
 * holds n_scan >= 1 strictly increasing elevations.
 *   Scan: D_i = ground_range_km of the group's ray at scan node i (the landing coordinate: x, or earth_radius_km * phi;
 * finite only for status ground) - the bits the tracer gives.  i* = the first index that attains the minimum over the
 * finite D_i.  No finite D_i: status -1, a NaN row, scan_index -1, n_evals 0.  i* at either end of the scan or beside a
 * node whose D is not finite: status 1, the node as it stands, no further ray.  Otherwise, in float64 without contraction,
 * with a = e_(i*-1), b = e_i*, c = e_(i*+1), D_b = D_i*, n = 0, g = 0.3819660112501051, at most max_iter + 1 times:
 *     c - a <= elev_tol_deg: status 0, stop;
 *     right = (c - b) >= (b - a); x = right ? b + g * (c - b) : b - g * (b - a);
 *     unless a < x < c and x != b: status 0, stop (the doubles are exhausted);
 *     n >= max_iter (1 .. 128): status 3, stop;
 *     D = ground_range_km of the group's ray at x; n = n + 1; D not finite: status 2, stop;
 *     D < D_b: (right ? a : c) = b, b = x, D_b = D; else (right ? c : a) = x.
 * There is no early stop: n_evals = n is part of the result.
 *   out is (n_groups, 18): skip_km (D_b), elevation_deg (b), status, scan_index (i*), bracket_deg (c - a; NaN for status
 * 1), n_evals, then the tracer's twelve outputs for the ray at elevation_deg, bit-identical to what the tracer returns
 * for that elevation, field, launch point and controls.  For a scan that looks forward the skip distance is skip_km -
 * x0_km.  D(e) of these tracers carries the step controller's sawtooth (section 4.9): skip_km is robust against it, the
 * elevation of a flat minimum is not.  No result depends on scheduling.
 * Group and scan arrays and out are host memory, or device memory with PRHF_FLAG_DEVICE_PTRS.  PRHF_EINVAL for a null
 * context (before anything else), a control outside its range, a host scan grid that does not increase strictly, an
 * elev_tol_deg that is negative or not finite, an earth_radius_km that is not positive and finite (geometry 1), and a
 * group_field out of range - checked on the host for host buffers, by the kernels for device-resident arrays (those
 * groups get NaN rows, no memory outside the records is read, and the error is reported at the synchronisation).
 * Synchronous.
 */
int prhf_gradient_skip_f64(prhf_ctx* ctx, int32_t geometry, const double* records, int64_t n_fields, int64_t n0,
                           int64_t n1, const double* axis0, const double* axis1, const int64_t* group_field,
                           const double* group_x0_km, const double* group_z0_km, int64_t n_groups,
                           const double* scan_elevation_deg, int64_t n_scan, double earth_radius_km, double s_max_km,
                           double rtol, double atol, double max_step_km, double z_ground_km, double top, double left,
                           double right, int32_t renormalize_every, double fill_n, double fill_grad, double fill_mup,
                           double elev_tol_deg, int32_t max_iter, double* out, uint32_t flags);

/*
 * MUF of a link through a tilted ionosphere: link l is (link_x0_km[l], link_z0_km[l], link_target_km[l]) over the one
 * ionosphere den, bmag, bpsi (n0, n1) on axis0, axis1 (prhf_field_build_f64's inputs; mode, edge_order likewise).
 * S(f) = skip_km of prhf_gradient_skip_f64 on prhf_field_build_f64's field at f (+inf at status -1).  Semantics,
 * statuses and the bisection are prhf_snell_muf_f64's: a NaN target: status -1; S(f_lo_hz) > t:
 * 2; S(f_hi_hz) <= t: 1 with muf_hz = f_hi_hz; else lo = f_lo_hz, hi = f_hi_hz and n_bisect (1 .. 64) times m = lo + 0.5 *
 * (hi - lo), a trip whose m is not strictly inside (lo, hi) changes nothing, S(m) <= t ? lo = m : hi = m: status 0 with
 * S(muf_hz = lo) <= t < S(f_above_hz = hi).
 *   out is (n_links, 21): muf_hz, f_above_hz, status, then the 18 values prhf_gradient_skip_f64 gives on
 * prhf_field_build_f64's field at muf_hz, bit for bit (NaN for status -1 and 2; f_above_hz is NaN for status 1).
 * One synchronisation at the end; the call is latency-bound: 3 + n_bisect dependent rounds of seven short kernels.
 * Scratch is 48 * n0 * n1 bytes per link (mu, mu' and the records of the link's field): PRHF_ENOMEM when it cannot be
 * allocated - search in batches of links; no result depends on the batching.
 * The ionosphere, the link and scan arrays and out are host memory, or device memory with PRHF_FLAG_DEVICE_PTRS; the axes
 * are host memory.  PRHF_EINVAL for a null context (before anything else) and as in the two calls above, for n_bisect
 * outside 1 .. 64 and unless 0 < f_lo_hz < f_hi_hz, both finite; PRHF_ENEGDEN for a negative density in a host array.
 * Synchronous.
 */
int prhf_gradient_muf_f64(prhf_ctx* ctx, int32_t geometry, const double* den, const double* bmag, const double* bpsi,
                          int64_t n0, int64_t n1, const double* axis0, const double* axis1, int32_t mode, int32_t edge_order,
                          const double* link_x0_km, const double* link_z0_km, const double* link_target_km, int64_t n_links,
                          double f_lo_hz, double f_hi_hz, int32_t n_bisect, const double* scan_elevation_deg, int64_t n_scan,
                          double earth_radius_km, double s_max_km, double rtol, double atol, double max_step_km,
                          double z_ground_km, double top, double left, double right, int32_t renormalize_every,
                          double fill_n, double fill_grad, double fill_mup, double elev_tol_deg, int32_t max_iter,
                          double* out, uint32_t flags);

/* Diagnostics of the context's last prhf_gradient_skip_f64 or prhf_gradient_muf_f64 (all its trips): counters[0] groups
 * refined, [1] rays the refine lanes traced, [2] ray slots (64 per trip of a refine wavefront's loop), [3] refine
 * wavefronts with work.  Lane utilisation of the refinement = [1] / [2].  No device call. */
int prhf_gradient_skip_counters(prhf_ctx* ctx, uint64_t* counters);

/*
 * Skip distance of the n_hops-hop mode (2F, 3F ..) through a horizontally varying mu: prhf_gradient_skip_f64 with D(e)
 * the ground_range_km of hop n_hops - 1 of prhf_trace_gradient_hops_f64's chain launched at elevation e, NaN unless all
 * n_hops (1 .. 16) hops land.  All arguments before n_hops are that call's.  Written out:
 *   Scan: D_i = D(e_i) for every scan node, a node whose chain fails on any hop has a D that is not finite.  i* = the
 * first index that attains the minimum over the finite D_i (D(e) of a chain is not unimodal: the first index is part of
 * the definition).  No finite D_i: status -1.  i* at either end of the scan or beside a node whose D is not finite:
 * status 1, the node as it stands, no further chain.  Otherwise, in float64 without contraction, with a = e_(i*-1),
 * b = e_i*, c = e_(i*+1), D_b = D_i*, n = 0, g = 0.3819660112501051, at most max_iter + 1 times:
 *     c - a <= elev_tol_deg: status 0, stop;
 *     right = (c - b) >= (b - a); x = right ? b + g * (c - b) : b - g * (b - a);
 *     unless a < x < c and x != b: status 0, stop (the doubles are exhausted);
 *     n >= max_iter (1 .. 128): status 3, stop;
 *     D = D(x); n = n + 1; D not finite: status 2, stop;
 *     D < D_b: (right ? a : c) = b, b = x, D_b = D; else (right ? c : a) = x.
 *   out is (n_groups, 6 + 15 * n_hops): skip_km (D_b), elevation_deg (b), status, scan_index (i*), bracket_deg (c - a;
 * NaN for status 1), n_evals (n: chains, not hops), then the n_hops hop rows of prhf_trace_gradient_hops_f64 for the
 * chain at elevation_deg, bit for bit what that call returns there; skip_km has the bits of the last hop's
 * ground_range_km.  Status -1: skip_km, elevation_deg and bracket_deg NaN, scan_index -1, n_evals 0, and the hop rows
 * unused as prhf_trace_gradient_hops_f64 writes them.  With n_hops = 1 the call finds what prhf_gradient_skip_f64 finds.
 * Memory, flags, the handling of a device-resident group_field out of range and every PRHF_EINVAL rule are
 * prhf_gradient_skip_f64's; PRHF_EINVAL also for n_hops outside 1 .. 16 (after the null context, before the rest).
 * Synchronous.
 */
int prhf_gradient_hop_skip_f64(prhf_ctx* ctx, int32_t geometry, const double* records, int64_t n_fields, int64_t n0,
                               int64_t n1, const double* axis0, const double* axis1, const int64_t* group_field,
                               const double* group_x0_km, const double* group_z0_km, int64_t n_groups,
                               const double* scan_elevation_deg, int64_t n_scan, double earth_radius_km, double s_max_km,
                               double rtol, double atol, double max_step_km, double z_ground_km, double top, double left,
                               double right, int32_t renormalize_every, double fill_n, double fill_grad, double fill_mup,
                               double elev_tol_deg, int32_t max_iter, int32_t n_hops, double* out, uint32_t flags);

/*
 * MUF of the n_hops-hop mode of a link through a tilted ionosphere: prhf_gradient_muf_f64 with S(f) = skip_km of
 * prhf_gradient_hop_skip_f64 on prhf_field_build_f64's field at f (+inf at status -1).  All arguments before n_hops,
 * the statuses -1, 0, 1, 2, the bisection m = lo + 0.5 * (hi - lo), n_bisect (1 .. 64) and the trip that does not move
 * are that call's.
 *   out is (n_links, 3 + 6 + 15 * n_hops): muf_hz, f_above_hz, status, then the row prhf_gradient_hop_skip_f64 gives on
 * prhf_field_build_f64's field at muf_hz, bit for bit (NaN throughout for status -1 and 2; f_above_hz is NaN for status
 * 1).  Scratch is 48 * n0 * n1 bytes per link, as in prhf_gradient_muf_f64: PRHF_ENOMEM when it cannot be allocated.
 * With n_hops = 1 the call finds what prhf_gradient_muf_f64 finds.  PRHF_EINVAL for a null context (before anything
 * else), n_hops outside 1 .. 16 and whatever prhf_gradient_muf_f64 refuses; PRHF_ENEGDEN likewise.  Synchronous.
 */
int prhf_gradient_hop_muf_f64(prhf_ctx* ctx, int32_t geometry, const double* den, const double* bmag, const double* bpsi,
                              int64_t n0, int64_t n1, const double* axis0, const double* axis1, int32_t mode,
                              int32_t edge_order, const double* link_x0_km, const double* link_z0_km,
                              const double* link_target_km, int64_t n_links, double f_lo_hz, double f_hi_hz, int32_t n_bisect,
                              const double* scan_elevation_deg, int64_t n_scan, double earth_radius_km, double s_max_km,
                              double rtol, double atol, double max_step_km, double z_ground_km, double top, double left,
                              double right, int32_t renormalize_every, double fill_n, double fill_grad, double fill_mup,
                              double elev_tol_deg, int32_t max_iter, int32_t n_hops, double* out, uint32_t flags);

/* prhf_gradient_skip_counters with a fifth word, for the context's last skip or MUF call of the gradient tracers,
 * one-hop or multi-hop: counters[0 .. 3] as there - prhf_gradient_skip_counters reports the multi-hop calls too, a ray
 * being a chain and a ray slot one lane-trip whatever the hops -, [4] hop rays: the hops of the refine lanes' chains
 * that landed, n_hops each (a chain that does not land ends its group's search; it counts under [1] alone); 0 after a
 * one-hop call.  Per slot a lane traced [4] / [2] hops.  No device call. */
int prhf_gradient_hop_skip_counters(prhf_ctx* ctx, uint64_t* counters);

/* The five diagnostics below (prhf_pair_plan_counters, prhf_panel_counters, prhf_panel_upper_counters,
 * prhf_panel_plan_counters, prhf_panel_quick_counters) read words that the operator's kernels add to once per workgroup,
 * when the workgroup leaves the kernel: a launch's counts are complete once the launch has finished - each of the five
 * waits for the context's stream, so what it returns is - and a launch in flight has added only the workgroups that
 * have left.  A call that returns a data error (a status of the profiles) has counted its other profiles all the same. */

/* Diagnostics of option "pair_plan", summed over every launch since the context was made: counters[0] reflecting pairs
 * whose sum ran from a plan made by one thread, [1] pairs of the same slices that computed their plan themselves (no
 * room for the plan, or a guess that did not bracket).  Pairs of slices that are not eligible count in neither.
 * Waits for the context's stream. */
int prhf_pair_plan_counters(prhf_ctx* ctx, uint64_t* counters);

/* Diagnostics of option "panel_lower", summed over every launch since the context was made: counters[0] reflecting pairs
 * whose segments below the top three took the panel sum, [1] pairs that were eligible for it and kept the sum of before
 * (a piece too close to X + Y = 1, a region of fewer than 256 points, a guess that did not bracket).  Waits for the
 * context's stream. */
int prhf_panel_counters(prhf_ctx* ctx, uint64_t* counters);

/* Diagnostics of option "panel_upper", summed over every launch since the context was made: of the pairs that
 * prhf_panel_counters counts under [0], counters[0] those whose panel region reached the top segment's first point, [1]
 * those that kept the lower region and the strided sums of the two segments below the top one.  Both stay 0 with the
 * option off.  (prhf_panel_counters itself counts with the option what it counts without it, except for a pair whose run
 * next below those segments fails the tests when it ends at the lower region's end and passes when it reaches its
 * segment's end: such a pair takes the panel sum with the option and falls back without.)  Waits for the context's stream. */
int prhf_panel_upper_counters(prhf_ctx* ctx, uint64_t* counters);

/* Diagnostics of the panel region's set-up, summed over every launch since the context was made: counters[0] the pairs
 * among those of prhf_pair_plan_counters' first word whose plan carries the panel sum's region - its first point, the
 * segments of its ends, whether it reaches the top segment - so that their waves read it instead of computing it.
 * Stays 0 with option "pair_plan", "panel_lower" or "panel_upper" off, and wherever no pair is planned.  Waits for the
 * context's stream. */
int prhf_panel_plan_counters(prhf_ctx* ctx, uint64_t* counters);

/* Diagnostics of option "panel_quick", summed over every launch since the context was made: the list passes of the panel
 * sum - one pass lists up to 63 runs of a pair's region, a pair makes two or three - in slices with option "panel_upper":
 * counters[0] the passes whose runs all passed the quick bound and skipped the runs' exact tests, [1] the passes that
 * took the exact tests.  [0] stays 0 with the option off; both stay 0 with option "panel_upper", "panel_lower" or
 * "strided_lower" off and wherever no pair comes to the panel sum.  (A pair with more than 63 passes of one kind counts
 * 63 of them; a grid of fewer than 65536 points on a profile that fits the kernel's staged arrays does not come
 * near.)  Waits for the context's stream. */
int prhf_panel_quick_counters(prhf_ctx* ctx, uint64_t* counters);

/* Diagnostics of option "stream_blocks": *count = the operator launches of this context that took the streaming form
 * since the context was made (a launch that keeps the general kernel does not count).  Host-side; does not synchronize. */
int prhf_stream_launches(prhf_ctx* ctx, uint64_t* count);

/* Diagnostics: workgroups of the fused kernel the runtime expects to keep resident per CU for
 * profiles of n_alt levels (LDS-limited) in arithmetic tier `math`. */
int prhf_occupancy(prhf_ctx* ctx, int64_t n_alt, int32_t math, int32_t* workgroups_per_cu);

/* Wait for everything enqueued on the context; returns PRHF_ENEGDEN / PRHF_EPEAK0 if a
 * kernel flagged bad input since the last sync. */
int prhf_sync(prhf_ctx* ctx);

/* Device time of the most recent TIMED launch (all kernels of that call), from HIP events on the
 * context's stream.  Synchronises on the stop event.  Every launch on device pointers is timed; a synchronous
 * host-buffer call of the operator (prhf_vfo_batch_f64 / _worklist / _residual without PRHF_FLAG_DEVICE_PTRS) is
 * timed only after prhf_ctx_set_option(ctx, "timing", 1): its two event records are 3.5 us of a 41 us call. */
int prhf_last_kernel_ms(prhf_ctx* ctx, double* ms);

/* The same for the most recent launches, oldest first: at most `capacity` of them (the context remembers 64);
 * *n = how many were written.  One synchronisation, on the newest launch - what a caller needs that enqueues a
 * series of launches and wants every one's device time without a host round trip between them (bench.py). */
int prhf_recent_kernel_ms(prhf_ctx* ctx, double* ms, int32_t capacity, int32_t* n);

#ifdef __cplusplus
}
#endif
#endif /* PRHF_H */
