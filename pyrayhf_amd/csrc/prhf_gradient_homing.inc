// prhf_gradient_homing.inc - point-to-point homing for the gradient ray tracers of both geometries: the rays of a
// transmitter (field, x0, z0) that land at a given ground_range_km.  Included by prhf_kernels.hip behind
// prhf_gradient.inc, inside namespace prhf.  Every ray here is grad_ray<GEO, FULL> of that file: FULL = false (the
// range-only ray: same steps, same landing node, no second pass) for the scan and the refinement, FULL = true for the
// result rows, so that a ray of a given field, launch point, elevation and controls has the bits
// prhf_trace_gradient_f64 / prhf_trace_gradient_spherical_f64 give it.  The reference has no homing function;
// DESIGN.md section 4.9 defines this one and include/prhf.h writes the refine step out operation by operation.
//
// A GROUP is a transmitter, a LINK a (group, target t) pair, the SCAN GRID a strictly increasing list of E elevations.
// Four kernels, no host round trip in between (launch_grad_home):
//   scan     grad_home_scan_kernel<GEO>: one ray per lane, ceil(E / 64) wavefronts per group, so that a wavefront
//            shares a field and neighbouring lanes have neighbouring elevations: D_i = ground_range_km of the group's
//            ray at e_i, and nothing else, into scan_d (n_groups, E); a group's scan serves all of its targets.
//   bracket  grad_home_bracket_kernel: home_bracket_kernel's twin for rows of 15 (the rule itself is the shared
//            home_is_bracket of prhf_homing.inc): one wavefront per link, 64 intervals a trip, ranks in ascending
//            elevation from the ballots' running popcount; n_brackets counts all brackets, the first max_roots go to
//            the work list as (link, rank, interval); every row of the link is preset to "unused" (NaN, status -1).
//   refine   grad_home_refine_kernel<GEO>: one record of the work list per LANE (a gradient ray is a lane's work).  A
//            lane narrows its bracket with range-only rays - Illinois steps, a bisection whenever the step before did
//            not halve the bracket - and stops as soon as its status is decided; the wavefront loops until a ballot
//            finds no lane at work.  The bracket's state (nine doubles, four ints) stays in registers across a ray:
//            the kernels need no scratch and no LDS beyond the staged axes.  It writes elevation, status and interval
//            to row (link, rank): the slot is the bracket's rank, whichever lane of whichever wavefront refines it,
//            and the order of the work list (the bracket kernel's atomic) decides nothing but that.
//   result   grad_home_result_kernel<GEO>: one record per lane again: the full two-pass ray at the row's elevation,
//            its twelve outputs behind the row's first three.  Only the records of the work list become rays.
// The refine and result launches are sized for n_links max_roots records; wavefronts beyond the list's length leave.
// MULTI-HOP HOMING (prhf_gradient_hop_home_f64, DESIGN.md section 4.12) is these four kernels with g.n_hops > 1 or a
// row_width other than PRHF_GRAD_HOME_OUTPUTS: D(e) is grad_hops<GEO, false> of prhf_gradient_hops.inc - the landing x
// of hop n_hops - 1, for one hop grad_ray itself - and a result row holds the row of every hop behind its first three.
// Counters (queue[]): 0 records, 1 rays traced by the refine lanes, 2 ray slots (64 per trip of a refine wavefront's
// loop), 3 refine wavefronts with work: lane utilisation = [1] / [2].

namespace {

constexpr int kGradHomeOutputs = PRHF_GRAD_HOME_OUTPUTS;

// (prhf_gradient_hops.inc)
template <int GEO, bool FULL>
__device__ __forceinline__ double grad_hops(const GradTraceArgs& a, const double* g0, const double* g1, long long r,
                                            long long field, double elev_deg, double x0_km, double z0_km, double* out);
// Column j of an unused hop row (launch x, z, elevation, then the tracer's twelve): NaN, status -1, the counters and the pad 0
__device__ __forceinline__ double grad_hop_unused(int j) { return j < 10 ? qnan() : j == 10 ? -1.0 : 0.0; }
__device__ __forceinline__ void grad_hop_unused_row(double* row) {
    for (int j = 0; j < PRHF_GRAD_HOP_OUTPUTS; ++j) row[j] = grad_hop_unused(j);
}

__device__ __forceinline__ void grad_home_stage_axes(const GradTraceArgs& a, double* axes) {
    for (int i = threadIdx.x; i < a.n0 + a.n1; i += blockDim.x) axes[i] = i < a.n0 ? a.a0[i] : a.a1[i - a.n0];
    __syncthreads();
}

template <int GEO>
__global__ __launch_bounds__(PRHF_GRAD_TRACE_THREADS) void grad_home_scan_kernel(const GradHomeArgs h) {
    extern __shared__ __attribute__((aligned(16))) double grad_axes[];
    grad_home_stage_axes(h.g, grad_axes);
    if (blockIdx.x == 0 && threadIdx.x < PRHF_GRAD_HOME_COUNTERS) h.queue[threadIdx.x] = 0u;   // (read two kernels on)
    const unsigned per_group = (unsigned)((h.n_scan + 63) / 64);
    const long long grp = blockIdx.x / per_group;
    const int i = (int)(blockIdx.x - grp * per_group) * 64 + (int)threadIdx.x;
    if (i >= h.n_scan) return;
    const long long f = h.group_field[grp];
    double d = qnan();
    if (f < 0 || f >= h.g.n_fields)       // (device-resident group_field: not checked by the host) no ray, no bracket
        post_status(h.g.status, (unsigned)PRHF_STATUS_BADFIELD);
    else
        d = grad_hops<GEO, false>(h.g, grad_axes, grad_axes + h.g.n0, 0, f, h.scan_elev[i], h.group_x0[grp], h.group_z0[grp],
                                  nullptr);
    h.scan_d[grp * h.n_scan + i] = d;
}

__global__ __launch_bounds__(64) void grad_home_bracket_kernel(const GradHomeArgs h) {
    const int lane = threadIdx.x & 63;
    const long long link = blockIdx.x;
    const long long g_given = h.link_group[link];
    const bool bad = g_given < 0 || g_given >= h.n_groups;         // (device-resident link_group: not checked by the host)
    const long long g = bad ? 0 : g_given;
    const double t = bad ? qnan() : h.link_target[link];            // (a NaN target brackets nothing)
    const double* d = h.scan_d + g * h.n_scan;
    double* rows = h.out + link * ((long long)h.max_roots * h.row_width);
    if (bad && lane == 0) post_status(h.g.status, (unsigned)PRHF_STATUS_BADGROUP);
    const bool hop_rows = h.row_width != kGradHomeOutputs;          // (the one-hop call's unused rows are NaN throughout)
    for (int k = lane; k < h.max_roots * h.row_width; k += 64) {
        const int col = k % h.row_width;
        rows[k] = col == 1 ? -1.0 : (hop_rows && col >= 3) ? grad_hop_unused((col - 3) % PRHF_GRAD_HOP_OUTPUTS) : qnan();
    }
    int found = 0;
    for (int base = 0; base < h.n_scan; base += 64) {
        const int i = base + lane;
        const bool is = i < h.n_scan && home_is_bracket(d, h.n_scan, i, t);
        const unsigned long long mask = __ballot(is);
        const int cnt = __popcll(mask);
        const int rank = found + __popcll(mask & ((1ull << lane) - 1ull));
        const int take = min(max(h.max_roots - found, 0), cnt);     // brackets of this trip that get a row
        if (take > 0) {
            unsigned at = 0;
            if (lane == 0) at = atomicAdd(h.queue, (unsigned)take);
            at = (unsigned)__builtin_amdgcn_readfirstlane((int)at);
            if (is && rank < h.max_roots) reinterpret_cast<int4*>(h.work)[at + (unsigned)(rank - found)] = make_int4((int)link, rank, i, 0);
        }
        found += cnt;
    }
    if (lane == 0) h.n_brackets[link] = found;
}

template <int GEO>
__global__ __launch_bounds__(PRHF_GRAD_TRACE_THREADS) void grad_home_refine_kernel(const GradHomeArgs h) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double grad_axes[];
    const unsigned n_work = h.queue[0];
    if ((unsigned long long)blockIdx.x * 64ull >= n_work) return;
    grad_home_stage_axes(h.g, grad_axes);
    const int lane = threadIdx.x & 63;
    const unsigned long long w = (unsigned long long)blockIdx.x * 64ull + (unsigned)lane;
    const bool mine = w < n_work;
    // The bracket [lo, hi] with f = D - t at its ends; an end within the tolerance (D_i == t among them) is the root.
    long long link = 0, f = 0;
    int rank = 0, i = 0, status = 1, last_side = 0, bisect = 0, it = 0;
    double t = 0.0, x0 = 0.0, z0 = 0.0, lo = 0.0, hi = 0.0, f_lo = 0.0, g_lo = 0.0, g_hi = 0.0, best_e = 0.0, best_miss = 0.0;
    if (mine) {
        const int4 rec = reinterpret_cast<const int4*>(h.work)[w];
        link = rec.x; rank = rec.y; i = rec.z;
        const long long g = h.link_group[link];                     // (in range: grad_home_bracket_kernel lists no other,
        f = h.group_field[g];                                       //  and a group with a bad field has no finite D)
        x0 = h.group_x0[g]; z0 = h.group_z0[g];
        const double* d = h.scan_d + g * h.n_scan;
        t = h.link_target[link];
        lo = h.scan_elev[i]; f_lo = d[i] - t;
        const bool wide = i + 1 < h.n_scan;
        hi = wide ? h.scan_elev[i + 1] : lo;
        const double f_hi = wide ? d[i + 1] - t : f_lo;
        best_e = (fabs(f_hi) < fabs(f_lo)) ? hi : lo;
        best_miss = fmin(fabs(f_lo), fabs(f_hi));
        status = best_miss <= h.range_tol ? 0 : 1;
        g_lo = f_lo; g_hi = f_hi;                                   // the secant's ordinates (Illinois halves a stale one)
    }
    bool busy = mine && status != 0;
    unsigned rays = 0, trips = 0;
    while (__ballot(busy) != 0) {
        ++trips;
        if (busy) {
            const double mid = lo + 0.5 * (hi - lo);
            if (!(mid > lo && mid < hi)) {
                busy = false;                                        // no float64 left between the ends: status 1
            } else {
                double x = mid;
                if (!bisect) {
                    const double xs = lo - g_lo * ((hi - lo) / (g_hi - g_lo));
                    if (xs > lo && xs < hi) x = xs;
                }
                const double dx = grad_hops<GEO, false>(h.g, grad_axes, grad_axes + h.g.n0, 0, f, x, x0, z0, nullptr);
                ++rays;
                if (!finite64(dx)) {
                    status = 2;                                      // the ray does not land inside the bracket
                    busy = false;
                } else {
                    const double fx = dx - t, miss = fabs(fx);
                    if (miss < best_miss) { best_miss = miss; best_e = x; }
                    if (miss <= h.range_tol) {
                        status = 0;
                        busy = false;
                    } else {
                        const double width = hi - lo;
                        if ((fx < 0.0) == (f_lo < 0.0)) {
                            lo = x; f_lo = fx; g_lo = fx;
                            if (last_side == -1) g_hi = 0.5 * g_hi;
                            last_side = -1;
                        } else {
                            hi = x; g_hi = fx;
                            if (last_side == 1) g_lo = 0.5 * g_lo;
                            last_side = 1;
                        }
                        bisect = ((hi - lo) > 0.5 * width) ? 1 : 0;
                        if (++it >= h.max_iter) busy = false;       // max_iter rays traced: status 1
                    }
                }
            }
        }
    }
    if (mine) {
        double* row = h.out + (link * h.max_roots + rank) * h.row_width;
        row[0] = best_e;
        row[1] = (double)status;
        row[2] = (double)i;
        if (rays) atomicAdd(h.queue + 1, rays);
    }
    if (lane == 0) {
        atomicAdd(h.queue + 2, 64u * trips);
        atomicAdd(h.queue + 3, 1u);
    }
}

template <int GEO>
__global__ __launch_bounds__(PRHF_GRAD_TRACE_THREADS) void grad_home_result_kernel(const GradHomeArgs h) {
    extern __shared__ __attribute__((aligned(16))) double grad_axes[];
    const unsigned n_work = h.queue[0];
    if ((unsigned long long)blockIdx.x * 64ull >= n_work) return;
    grad_home_stage_axes(h.g, grad_axes);
    const unsigned long long w = (unsigned long long)blockIdx.x * 64ull + threadIdx.x;
    if (w >= n_work) return;
    const int4 rec = reinterpret_cast<const int4*>(h.work)[w];
    const long long link = rec.x;
    const long long g = h.link_group[link];
    double* row = h.out + (link * h.max_roots + rec.y) * h.row_width;
    if (h.row_width == kGradHomeOutputs)
        (void)grad_ray<GEO, true>(h.g, grad_axes, grad_axes + h.g.n0, 0, h.group_field[g], row[0], h.group_x0[g], h.group_z0[g], row + 3);
    else
        (void)grad_hops<GEO, true>(h.g, grad_axes, grad_axes + h.g.n0, 0, h.group_field[g], row[0], h.group_x0[g], h.group_z0[g], row + 3);
}

}  // namespace

hipError_t launch_grad_home(const GradHomeArgs& h, hipStream_t stream) {
    if (h.n_links <= 0) return hipSuccess;
    const long long per_group = (h.n_scan + 63) / 64;
    const long long rows = h.n_links * (long long)h.max_roots;
    if (h.n_groups * per_group > 0x7fffffffLL || h.n_links > 0x7fffffffLL || rows > 0x7fffffffLL) return hipErrorInvalidValue;
    const size_t lds = field_axes_lds_bytes(h.g.n0, h.g.n1);
    const dim3 threads(PRHF_GRAD_TRACE_THREADS), scan_grid((unsigned)(h.n_groups * per_group)),
        row_grid((unsigned)((rows + 63) / 64));
    const bool sph = h.g.geometry == PRHF_GEO_SPHERICAL;
    if (sph) hipLaunchKernelGGL(grad_home_scan_kernel<PRHF_GEO_SPHERICAL>, scan_grid, threads, lds, stream, h);
    else hipLaunchKernelGGL(grad_home_scan_kernel<PRHF_GEO_CARTESIAN>, scan_grid, threads, lds, stream, h);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(grad_home_bracket_kernel, dim3((unsigned)h.n_links), dim3(64), 0, stream, h);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (sph) hipLaunchKernelGGL(grad_home_refine_kernel<PRHF_GEO_SPHERICAL>, row_grid, threads, lds, stream, h);
    else hipLaunchKernelGGL(grad_home_refine_kernel<PRHF_GEO_CARTESIAN>, row_grid, threads, lds, stream, h);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (sph) hipLaunchKernelGGL(grad_home_result_kernel<PRHF_GEO_SPHERICAL>, row_grid, threads, lds, stream, h);
    else hipLaunchKernelGGL(grad_home_result_kernel<PRHF_GEO_CARTESIAN>, row_grid, threads, lds, stream, h);
    return hipGetLastError();
}
