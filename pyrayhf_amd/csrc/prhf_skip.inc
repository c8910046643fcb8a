// prhf_skip.inc - skip distance of a (profile, frequency) group of the stratified Snell tracers, and the MUF of a link:
// the frequency at which the skip distance reaches the link's range.  Included by prhf_kernels.hip behind
// prhf_homing.inc, inside namespace prhf: every ray here is snell_ray_table<GEOM> through home_eval / home_ray_args
// (prhf_homing.inc, not edited), so that a ray of a given group and elevation has the bits prhf_snell_fan_f64 gives it.
// The reference has neither function; DESIGN.md section 4.10 defines both.
//
// Skip distance, behind the tables' prologue and with no host round trip in between (launch_snell_skip):
//   scan     skip_scan_kernel<GEOM>: one wavefront per (group, scan node): D_i = ground_range_km of the fan ray at e_i,
//            8 bytes per ray into scan_d (n_groups, E).
//   refine   skip_refine_kernel<GEOM>: one wavefront per group.  i* = the first index that attains the minimum over the
//            finite D_i, 64 nodes a trip (the wavefront's minimum, then the first lane that holds it).  An i* at either
//            end of the scan or beside a node that does not land is the answer as it stands (status 1); otherwise a
//            golden-section search on the triple (e_i*-1, e_i*, e_i*+1), a dependent chain of rays of the group.  While
//            a ray is traced the triple and the best row wait in the wavefront's LDS slot, as in home_refine_kernel.
// MUF (launch_snell_muf): a link is its own group, whose frequency lives in the device-side group table.  Per trip
// muf_set_kernel writes every link's next frequency there, the tables, the scan and the refine run on it, and
// muf_decide_kernel moves the link's frequency bracket; everything is enqueued on one stream, the host waits once.

namespace {

constexpr int kSkipOutputs = PRHF_SKIP_OUTPUTS;           // elevation, status, scan index, bracket, rays traced, then the tracer's eight
constexpr int kMufOutputs = PRHF_MUF_OUTPUTS;             // muf, the frequency above, status, then the skip row at the muf
constexpr int kSkipState = 8;                            // doubles of the refine kernel's parked triple; the best ray's outputs behind it

}  // namespace

#ifndef PRHF_SKIP_WAVES
#define PRHF_SKIP_WAVES PRHF_HOME_WAVES       // register budget of the refine kernels in waves per SIMD (DESIGN.md 4.10)
#endif

template <int GEOM>
__global__ __launch_bounds__(64, PRHF_FAN_WAVES) void skip_scan_kernel(const SkipArgs h) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* lds = reinterpret_cast<double*>(smem);
    double* slot = lds + (h.s.n_alt + 2);
    const int lane = threadIdx.x & 63;
    const long long grp = blockIdx.x / (unsigned)h.n_scan;
    const int i = (int)(blockIdx.x - grp * h.n_scan);
    if (h.active && h.active[grp] == 0) return;                     // (MUF: a link whose frequency bracket is settled)
    const SnellArgs b = home_ray_args(h.s, slot);
    const double d = home_eval<GEOM>(b, lds, slot, grp, h.scan_elev[i]);
    if (lane == 0) h.scan_d[grp * h.n_scan + i] = d;
}

template <int GEOM>
__global__ __launch_bounds__(64, PRHF_SKIP_WAVES) void skip_refine_kernel(const SkipArgs h) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* lds = reinterpret_cast<double*>(smem);
    double* slot = lds + (h.s.n_alt + 2);
    const int lane = threadIdx.x & 63;
    double* st = slot + 10;
    const long long g = blockIdx.x;
    if (h.active && h.active[g] == 0) return;
    const SnellArgs b = home_ray_args(h.s, slot);
    const double* d = h.scan_d + g * h.n_scan;
    double* row = h.out + g * kSkipOutputs;
    const double inf = __builtin_inf();
    // ---- the node: first index of the minimum over the finite D_i ------------------------------------------------
    double d_min = inf;
    int i_min = -1;
    for (int base = 0; base < h.n_scan; base += 64) {
        const int i = base + lane;
        const double raw = i < h.n_scan ? d[i] : inf;
        const double v = finite64(raw) ? raw : inf;
        const double m = uniform(wave_min(v));
        const unsigned long long at = __ballot(v == m);
        // (a later trip wins only with a smaller value: the first index keeps a tie)
        if (m < d_min) {
            d_min = m;
            i_min = base + __ffsll((long long)at) - 1;
        }
    }
    if (i_min < 0) {                                                // no ray of the scan lands
        if (lane < kSkipOutputs) row[lane] = (lane == 1 || lane == 2) ? -1.0 : (lane == 4 || lane == 12) ? 0.0 : qnan();
        return;
    }
    const bool edge = i_min == 0 || i_min == h.n_scan - 1 || !finite64(d[max(i_min - 1, 0)]) ||
                      !finite64(d[min(i_min + 1, h.n_scan - 1)]);
    double e_a = qnan(), e_b = h.scan_elev[i_min], e_c = qnan(), d_b = d_min;
    int status = 1, n_evals = 0, b_is_node = 1;
    if (!edge) {
        // ---- golden-section search on (a, b, c): D_b is the least ground range seen; at most max_iter rays ----------
        const double gold = 0.3819660112501051;
        const double tol = h.elev_tol;
        e_a = h.scan_elev[i_min - 1];
        e_c = h.scan_elev[i_min + 1];
        status = 3;
        for (int trip = 0; trip <= h.max_iter; ++trip) {
            if (e_c - e_a <= tol) { status = 0; break; }
            const bool right = (e_c - e_b) >= (e_b - e_a);
            const double x = right ? e_b + gold * (e_c - e_b) : e_b - gold * (e_b - e_a);
            if (!(x > e_a && x < e_c) || x == e_b) { status = 0; break; }      // the doubles are exhausted
            if (n_evals >= h.max_iter) { status = 3; break; }
            if (lane == 0) { st[0] = e_a; st[1] = e_b; st[2] = e_c; st[3] = d_b; st[4] = x; }
            const double dx = home_eval<GEOM>(b, lds, slot, g, x);
            e_a = st[0]; e_b = st[1]; e_c = st[2]; d_b = st[3];
            const double xr = st[4];
            ++n_evals;
            if (!finite64(dx)) { status = 2; break; }              // the ray escapes inside the bracket
            const bool rt = (e_c - e_b) >= (e_b - e_a);
            if (dx < d_b) {
                if (rt) e_a = e_b; else e_c = e_b;
                e_b = xr;
                d_b = dx;
                b_is_node = 0;
                if (lane < PRHF_SNELL_OUTPUTS) st[kSkipState + lane] = slot[2 + lane];
            } else {                                                // (a tie keeps b)
                if (rt) e_c = xr; else e_a = xr;
            }
        }
    }
    if (b_is_node) {                                                // the scan node's own ray, for its eight outputs: not counted
        if (lane == 0) { st[0] = e_a; st[1] = e_b; st[2] = e_c; }
        (void)home_eval<GEOM>(b, lds, slot, g, e_b);
        e_a = st[0]; e_b = st[1]; e_c = st[2];
        if (lane < PRHF_SNELL_OUTPUTS) st[kSkipState + lane] = slot[2 + lane];
    }
    __syncthreads();
    if (lane < PRHF_SNELL_OUTPUTS) row[5 + lane] = st[kSkipState + lane];
    if (lane == 0) {
        row[0] = e_b;
        row[1] = (double)status;
        row[2] = (double)i_min;
        row[3] = e_c - e_a;                                         // (NaN for an edge node)
        row[4] = (double)n_evals;
    }
}

// ---- MUF: one thread per link ---------------------------------------------------------------------------------------
// state (n_links, 4): lo, hi, link status, 0.  phase 0: f_lo, 1: f_hi, 2: a bisection trip.
__global__ __launch_bounds__(64) void muf_set_kernel(const MufArgs m, int phase) {
#pragma clang fp contract(off)
    const long long l = (long long)blockIdx.x * 64 + threadIdx.x;
    if (l >= m.n_links) return;
    double f = phase == 0 ? m.f_lo : m.f_hi;
    int on = 1;
    if (phase == 2) {
        const double lo = m.state[4 * l], hi = m.state[4 * l + 1];
        const double mid = lo + 0.5 * (hi - lo);
        on = (m.state[4 * l + 2] == 0.0 && mid > lo && mid < hi) ? 1 : 0;   // (a trip that cannot split changes nothing)
        f = on ? mid : m.f_lo;
    }
    m.group_freq[l] = f;
    m.active[l] = on;
}

__global__ __launch_bounds__(64) void muf_decide_kernel(const MufArgs m, int phase, int last) {
    const long long l = (long long)blockIdx.x * 64 + threadIdx.x;
    if (l >= m.n_links) return;
    const double* cur = m.k.out + l * kSkipOutputs;
    double* best = m.best + l * kSkipOutputs;
    double* s = m.state + 4 * l;
    const double t = m.link_range[l];
    const bool on = m.active[l] != 0;
    // S(f): the skip distance, +inf when no ray of the scan lands
    const double sf = cur[1] == -1.0 ? __builtin_inf() : cur[5 + 4];
    bool take = false;
    if (phase == 0) {
        s[0] = m.f_lo; s[1] = m.f_hi; s[3] = 0.0;
        s[2] = (t != t) ? -1.0 : (sf > t) ? 2.0 : 0.0;
        take = true;
    } else if (phase == 1) {
        if (s[2] == 0.0 && sf <= t) { s[2] = 1.0; s[0] = m.f_hi; s[1] = qnan(); take = true; }
    } else if (on) {
        if (sf <= t) { s[0] = m.group_freq[l]; take = true; }
        else s[1] = m.group_freq[l];
    }
    if (take)
        for (int k = 0; k < kSkipOutputs; ++k) best[k] = cur[k];
    if (last) {
        double* row = m.out + l * kMufOutputs;
        const bool none = s[2] == -1.0 || s[2] == 2.0;
        row[0] = none ? qnan() : s[0];
        row[1] = none ? qnan() : s[1];
        row[2] = s[2];
        for (int k = 0; k < kSkipOutputs; ++k) row[3 + k] = none ? qnan() : best[k];
    }
}

namespace {

hipError_t skip_tables(const SnellArgs& a, bool profiles, hipStream_t stream) {
    // the tables' prologue of a grouped launch (launch_snell)
    hipError_t e;
    if (profiles) {
        const int n_chunk = a.ptab ? (int)((a.n_alt + 63) / 64) : 1;
        if (a.n_prof * n_chunk > 0x7fffffffLL) return hipErrorInvalidValue;
        hipLaunchKernelGGL(snell_profile_kernel, dim3((unsigned)(a.n_prof * n_chunk)), dim3(64), 0, stream, a, n_chunk);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int n_lev = (int)a.n_alt + 1;
    const int trips = (n_lev + kTableThreads - 1) / kTableThreads;
    const int threads = 64 * ((n_lev + 64 * trips - 1) / (64 * trips));
    hipLaunchKernelGGL(snell_tables_kernel, dim3((unsigned)a.n_groups), dim3((unsigned)threads), 0, stream, a);
    return hipGetLastError();
}

hipError_t skip_kernels(const SkipArgs& h, const void** scan, const void** refine, size_t* lds_bytes) {
    const SnellArgs& a = h.s;
    if (a.n_alt + 2 > 65535 || a.n_groups * (long long)h.n_scan > 0x7fffffffLL) return hipErrorInvalidValue;
    *lds_bytes = home_lds_bytes(a.n_alt);
    *scan = a.geometry == 0 ? reinterpret_cast<const void*>(&skip_scan_kernel<0>)
                            : reinterpret_cast<const void*>(&skip_scan_kernel<1>);
    *refine = a.geometry == 0 ? reinterpret_cast<const void*>(&skip_refine_kernel<0>)
                              : reinterpret_cast<const void*>(&skip_refine_kernel<1>);
    hipError_t e = hipFuncSetAttribute(*scan, hipFuncAttributeMaxDynamicSharedMemorySize, (int)*lds_bytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(*refine, hipFuncAttributeMaxDynamicSharedMemorySize, (int)*lds_bytes);
}

hipError_t skip_enqueue(const SkipArgs& h, const void* scan, const void* refine, size_t lds_bytes, hipStream_t stream) {
    void* params[] = {const_cast<SkipArgs*>(&h)};
    hipError_t e = hipLaunchKernel(scan, dim3((unsigned)(h.s.n_groups * h.n_scan)), dim3(64), params, lds_bytes, stream);
    if (e != hipSuccess) return e;
    return hipLaunchKernel(refine, dim3((unsigned)h.s.n_groups), dim3(64), params, lds_bytes, stream);
}

}  // namespace

hipError_t launch_snell_skip(const SkipArgs& h, hipStream_t stream) {
    if (h.s.n_groups <= 0) return hipSuccess;
    const void *scan, *refine;
    size_t lds_bytes;
    hipError_t e = skip_kernels(h, &scan, &refine, &lds_bytes);
    if (e != hipSuccess) return e;
    e = skip_tables(h.s, true, stream);
    if (e != hipSuccess) return e;
    e = skip_enqueue(h, scan, refine, lds_bytes, stream);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

hipError_t launch_snell_muf(const MufArgs& m, hipStream_t stream) {
    if (m.n_links <= 0) return hipSuccess;
    const void *scan, *refine;
    size_t lds_bytes;
    hipError_t e = skip_kernels(m.k, &scan, &refine, &lds_bytes);
    if (e != hipSuccess) return e;
    const dim3 links((unsigned)((m.n_links + 63) / 64));
    // S(f_lo), S(f_hi), then n_bisect trips: set the frequencies, tables, scan, refine, decide
    for (int trip = 0; trip < 2 + m.n_bisect; ++trip) {
        const int phase = trip < 2 ? trip : 2;
        hipLaunchKernelGGL(muf_set_kernel, links, dim3(64), 0, stream, m, phase);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = skip_tables(m.k.s, trip == 0, stream);                  // (the per-profile scalars do not depend on the frequency)
        if (e != hipSuccess) return e;
        e = skip_enqueue(m.k, scan, refine, lds_bytes, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(muf_decide_kernel, links, dim3(64), 0, stream, m, phase, trip == 1 + m.n_bisect ? 1 : 0);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}
