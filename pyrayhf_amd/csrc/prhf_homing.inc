// prhf_homing.inc - point-to-point homing for the stratified Snell tracers: the rays of a (profile, frequency) group
// that land at a given ground range.  Included by prhf_kernels.hip behind prhf_snell.inc, inside namespace prhf: every
// ray here is snell_ray_table<GEOM> itself (prhf_snell.inc, not edited), reading the group tables of
// snell_tables_kernel - the two-load bracket search and the up-leg - so that a ray of a given group and elevation has
// the bits prhf_snell_fan_f64 gives it.  The reference has no homing function; DESIGN.md section 4.8 defines this one.
//
// A LINK is a (group, target range t) pair, the SCAN GRID a strictly increasing list of E elevations.  Four steps
// behind the tables' prologue, no host round trip in between (launch_snell_home):
//   scan     home_scan_kernel<GEOM>: one wavefront per (group, scan node): D_i = ground_range_km of the fan ray at
//            e_i, and nothing else, into scan_d (n_groups, E); a group's scan serves all of its targets.
//   bracket  home_bracket_kernel: one wavefront per link, 64 intervals a trip: interval i is a bracket when D_i and
//            D_i+1 are finite and (D_i - t), (D_i+1 - t) have opposite signs or D_i == t; D_E-1 == t is a bracket of
//            no width.  Ranks in ascending elevation from the ballots' running popcount; n_brackets counts all of them,
//            the first max_roots go to the work list as (link, rank, interval); every row of the link is preset to
//            "unused" (NaN, status -1).
//   refine   home_refine_kernel<GEOM>: persistent wavefronts draw the records from eight sliced counters (as the
//            per-ray launch draws rays); one wavefront narrows one bracket with rays of the group - Illinois steps, a
//            bisection whenever the last step did not halve the bracket, so max_iter evaluations always halve it
//            max_iter / 2 times - and writes row (link, rank): the slot is the bracket's rank, whoever refines it.
// How snell_ray_table is called for ONE ray without per-ray arrays in global memory: a copy of the launch's SnellArgs
// whose elev_deg, ray_group and out point at a 16-double slot of the wavefront's LDS behind the up-leg array (a generic
// pointer may address LDS); ray 0 of that copy is the ray, path_x is null (no path stores), and the eight outputs come
// back through LDS, which a wavefront reads in the order it wrote.

namespace {

constexpr int kHomeOutputs = 3 + PRHF_SNELL_OUTPUTS;     // elevation, status, scan index, then the tracer's eight
constexpr int kHomeSlot = 32;                             // doubles of LDS behind u_up: elevation, group, the eight outputs, and ...
constexpr int kHomeState = 10;                            // ... the refine kernel's bracket state (st[]), the best ray's outputs behind it
constexpr int kHomeSlices = 8;                            // queues of the refine launch (one per XCD)
constexpr int kHomeQueueStride = 32;                      // unsigned words between two queues' counters (128 B)
constexpr int kHomeQueueWords = (kHomeSlices + 1) * kHomeQueueStride;   // ... and behind them the number of records

// One ray of group `grp` at `elev` through snell_ray_table; its ground range; the eight outputs stay in slot[2 .. 9].
template <int GEOM>
__device__ __forceinline__ double home_eval(const SnellArgs& b, double* lds, double* slot, long long grp, double elev) {
    const int lane = threadIdx.x & 63;
    __syncthreads();                                      // (one wavefront: the last ray's LDS reads before these writes)
    if (lane == 0) {
        slot[0] = elev;
        *reinterpret_cast<long long*>(slot + 1) = grp;
    }
    __syncthreads();
    snell_ray_table<GEOM>(b, 0, lds);
    __syncthreads();
    return slot[2 + 4];                                   // ground_range_km, NaN for a ray that does not turn
}

__device__ __forceinline__ SnellArgs home_ray_args(const SnellArgs& s, double* slot) {
    SnellArgs b = s;
    b.elev_deg = slot;
    b.ray_group = reinterpret_cast<const long long*>(slot + 1);
    b.out = slot + 2;
    b.path_x = nullptr;
    b.path_z = nullptr;
    b.path_stride = 0;
    b.n_rays = 1;
    return b;
}

// The bracket rule of both homing calls (this file's, and prhf_gradient_homing.inc's): is interval i of the scan
// d[0 .. n_scan) a bracket of the target t?  "Interval" n_scan - 1 stands for the bracket of no width at the last node.
__device__ __forceinline__ bool home_is_bracket(const double* d, int n_scan, int i, double t) {
    const double d0 = d[i];
    if (i == n_scan - 1) return d0 == t;
    const double d1 = d[i + 1];
    const double f0 = d0 - t, f1 = d1 - t;
    return finite64(d0) && finite64(d1) && ((f0 < 0.0 && f1 > 0.0) || (f0 > 0.0 && f1 < 0.0) || d0 == t);
}

}  // namespace

#ifndef PRHF_HOME_WAVES
#define PRHF_HOME_WAVES (GEOM == 0 ? 8 : 6)   // register budget of the refine kernels in waves per SIMD (DESIGN.md 4.8)
#endif

template <int GEOM>
__global__ __launch_bounds__(64, PRHF_FAN_WAVES) void home_scan_kernel(const HomeArgs h) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* lds = reinterpret_cast<double*>(smem);
    double* slot = lds + (h.s.n_alt + 2);
    const int lane = threadIdx.x & 63;
    // the refine launch's counters and the work list's length (read two kernels on)
    if (blockIdx.x == 0 && lane <= kHomeSlices) h.queue[lane * kHomeQueueStride] = 0u;
    const long long grp = blockIdx.x / (unsigned)h.n_scan;
    const int i = (int)(blockIdx.x - grp * h.n_scan);
    const SnellArgs b = home_ray_args(h.s, slot);
    const double d = home_eval<GEOM>(b, lds, slot, grp, h.scan_elev[i]);
    if (lane == 0) h.scan_d[grp * h.n_scan + i] = d;
}

__global__ __launch_bounds__(64) void home_bracket_kernel(const HomeArgs h) {
    const int lane = threadIdx.x & 63;
    const long long link = blockIdx.x;
    const long long g_given = h.link_group[link];
    const bool bad = g_given < 0 || g_given >= h.s.n_groups;       // (device-resident link_group: not checked by the host)
    const long long g = bad ? 0 : g_given;
    const double t = bad ? qnan() : h.link_range[link];             // (a NaN target brackets nothing)
    const double* d = h.scan_d + g * h.n_scan;
    double* rows = h.out + link * ((long long)h.max_roots * kHomeOutputs);
    if (bad && lane == 0) post_status(h.s.status, (unsigned)PRHF_STATUS_BADGROUP);
    for (int k = lane; k < h.max_roots * kHomeOutputs; k += 64) rows[k] = (k % kHomeOutputs == 1) ? -1.0 : qnan();
    int found = 0;
    // "interval" E - 1 stands for the bracket of no width at the last node
    for (int base = 0; base < h.n_scan; base += 64) {
        const int i = base + lane;
        const bool is = i < h.n_scan && home_is_bracket(d, h.n_scan, i, t);
        const unsigned long long mask = __ballot(is);
        const int cnt = __popcll(mask);
        const int rank = found + __popcll(mask & ((1ull << lane) - 1ull));
        const int take = min(max(h.max_roots - found, 0), cnt);     // brackets of this trip that get a row
        if (take > 0) {
            unsigned at = 0;
            if (lane == 0) at = atomicAdd(h.queue + kHomeSlices * kHomeQueueStride, (unsigned)take);
            at = (unsigned)__builtin_amdgcn_readfirstlane((int)at);
            if (is && rank < h.max_roots) reinterpret_cast<int4*>(h.work)[at + (unsigned)(rank - found)] = make_int4((int)link, rank, i, 0);
        }
        found += cnt;
    }
    if (lane == 0) h.n_brackets[link] = found;
}

template <int GEOM>
__global__ __launch_bounds__(64, PRHF_HOME_WAVES) void home_refine_kernel(const HomeArgs h) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* lds = reinterpret_cast<double*>(smem);
    double* slot = lds + (h.s.n_alt + 2);
    const int lane = threadIdx.x & 63;
    double* st = slot + 10;
    const SnellArgs b = home_ray_args(h.s, slot);
    const unsigned n_work = h.queue[kHomeSlices * kHomeQueueStride];
    const unsigned per_slice = (n_work + kHomeSlices - 1) / kHomeSlices;
    int slice = (int)(blockIdx.x % kHomeSlices);
    // a draw yields a record or moves the wavefront on to the next slice; after kHomeSlices moves it leaves
    for (int moves = 0; moves < kHomeSlices;) {
        unsigned next = 0;
        if (lane == 0) next = atomicAdd(h.queue + slice * kHomeQueueStride, 1u);
        next = (unsigned)__builtin_amdgcn_readfirstlane((int)next);
        const unsigned long long w = (unsigned long long)slice * per_slice + next;
        if (next >= per_slice || w >= n_work) {
            slice = (slice + 1) % kHomeSlices;
            ++moves;
            continue;
        }
        const int4 rec = reinterpret_cast<const int4*>(h.work)[w];
        const long long link = uniform(rec.x);
        const int rank = uniform(rec.y), i = uniform(rec.z);
        const long long g = h.link_group[link];                     // (in range: home_bracket_kernel lists no other)
        const double tol = h.range_tol;
        const double* d = h.scan_d + g * h.n_scan;
        // The bracket [lo, hi] with f = D - t at its ends; an end within the tolerance (D_i == t among them) is the root.
        // While a ray is traced the bracket's state waits in LDS (st[]: the wavefront's own words, written by lane 0 and
        // read back by every lane - the same bits), so that the ray has the registers the fan kernel's ray has.
        double t = h.link_range[link];
        double lo = h.scan_elev[i], f_lo = d[i] - t;
        const bool wide = i + 1 < h.n_scan;
        double hi = wide ? h.scan_elev[i + 1] : lo, f_hi = wide ? d[i + 1] - t : f_lo;
        double best_e = (fabs(f_hi) < fabs(f_lo)) ? hi : lo;
        double best_miss = fmin(fabs(f_lo), fabs(f_hi));
        int best_is_node = 1;                                        // the best ray so far is a scan node: not traced here yet
        int status = best_miss <= tol ? 0 : 1;
        if (status != 0) {
            double g_lo = f_lo, g_hi = f_hi;                         // the secant's ordinates (Illinois halves a stale one)
            int last_side = 0, bisect = 0;
            for (int it = 0; it < h.max_iter; ++it) {
                const double mid = lo + 0.5 * (hi - lo);
                if (!(mid > lo && mid < hi)) break;                  // no float64 left between the ends
                double x = mid;
                if (!bisect) {
                    const double xs = lo - g_lo * ((hi - lo) / (g_hi - g_lo));
                    if (xs > lo && xs < hi) x = xs;
                }
                if (lane == 0) {
                    st[0] = lo; st[1] = hi; st[2] = f_lo; st[3] = g_lo; st[4] = g_hi; st[5] = best_e; st[6] = best_miss;
                    st[7] = x; st[8] = t;
                }
                const double dx = home_eval<GEOM>(b, lds, slot, g, x);
                lo = st[0]; hi = st[1]; f_lo = st[2]; g_lo = st[3]; g_hi = st[4]; best_e = st[5]; best_miss = st[6];
                x = st[7]; t = st[8];
                if (!finite64(dx)) { status = 2; break; }            // the ray escapes inside the bracket
                const double f = dx - t, miss = fabs(f);
                if (miss < best_miss) {
                    best_miss = miss;
                    best_e = x;
                    best_is_node = 0;
                    if (lane < PRHF_SNELL_OUTPUTS) st[kHomeState + lane] = slot[2 + lane];
                }
                if (miss <= tol) { status = 0; break; }
                const double width = hi - lo;
                if ((f < 0.0) == (f_lo < 0.0)) {
                    lo = x; f_lo = f; g_lo = f;
                    if (last_side == -1) g_hi = 0.5 * g_hi;
                    last_side = -1;
                } else {
                    hi = x; g_hi = f;
                    if (last_side == 1) g_lo = 0.5 * g_lo;
                    last_side = 1;
                }
                bisect = ((hi - lo) > 0.5 * width) ? 1 : 0;
            }
        }
        if (best_is_node) {
            if (lane == 0) st[5] = best_e;
            (void)home_eval<GEOM>(b, lds, slot, g, best_e);
            best_e = st[5];
            if (lane < PRHF_SNELL_OUTPUTS) st[kHomeState + lane] = slot[2 + lane];
        }
        __syncthreads();
        double* row = h.out + (link * h.max_roots + rank) * kHomeOutputs;
        if (lane < PRHF_SNELL_OUTPUTS) row[3 + lane] = st[kHomeState + lane];
        if (lane == 0) {
            row[0] = best_e;
            row[1] = (double)status;
            row[2] = (double)i;
        }
    }
}

size_t home_lds_bytes(long long n_alt) { return (size_t)(n_alt + 2 + kHomeSlot) * sizeof(double); }
size_t home_queue_bytes() { return (size_t)kHomeQueueWords * sizeof(unsigned); }

hipError_t launch_snell_home(const HomeArgs& h, hipStream_t stream) {
    const SnellArgs& a = h.s;
    if (h.n_links <= 0) return hipSuccess;
    if (a.n_alt + 2 > 65535 || a.n_groups * (long long)h.n_scan > 0x7fffffffLL || h.n_links > 0x7fffffffLL ||
        h.n_links * (long long)h.max_roots > 0x7fffffffLL)
        return hipErrorInvalidValue;
    const size_t lds_bytes = home_lds_bytes(a.n_alt);
    const void* scan = a.geometry == 0 ? reinterpret_cast<const void*>(&home_scan_kernel<0>)
                                       : reinterpret_cast<const void*>(&home_scan_kernel<1>);
    const void* refine = a.geometry == 0 ? reinterpret_cast<const void*>(&home_refine_kernel<0>)
                                         : reinterpret_cast<const void*>(&home_refine_kernel<1>);
    hipError_t e = hipFuncSetAttribute(scan, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(refine, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    // the tables' prologue of a grouped launch (launch_snell)
    const int n_chunk = a.ptab ? (int)((a.n_alt + 63) / 64) : 1;
    if (a.n_prof * n_chunk > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(snell_profile_kernel, dim3((unsigned)(a.n_prof * n_chunk)), dim3(64), 0, stream, a, n_chunk);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int n_lev = (int)a.n_alt + 1;
    const int trips = (n_lev + kTableThreads - 1) / kTableThreads;
    const int threads = 64 * ((n_lev + 64 * trips - 1) / (64 * trips));
    hipLaunchKernelGGL(snell_tables_kernel, dim3((unsigned)a.n_groups), dim3((unsigned)threads), 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    void* params[] = {const_cast<HomeArgs*>(&h)};
    e = hipLaunchKernel(scan, dim3((unsigned)(a.n_groups * h.n_scan)), dim3(64), params, lds_bytes, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(home_bracket_kernel, dim3((unsigned)h.n_links), dim3(64), 0, stream, h);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    int per_cu = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, refine, 64, lds_bytes);
    if (e != hipSuccess) return e;
    if (per_cu < 1) per_cu = 1;
    const long long waves = (long long)per_cu * (long long)(a.resident_cus > 0 ? a.resident_cus : 256);
    const long long records = h.n_links * (long long)h.max_roots;   // at most: the list's length is the device's
    e = hipLaunchKernel(refine, dim3((unsigned)(records < waves ? records : waves)), dim3(64), params, lds_bytes, stream);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}
