// prhf_gradient_skip.inc - for the gradient ray tracers of both geometries: the fields of many frequencies built on the
// device from one 2-D ionosphere, the skip distance of a transmitter (field, x0, z0), and the MUF of a link through that
// ionosphere - the frequency at which the skip distance reaches the link's target.  Included by prhf_kernels.hip behind
// prhf_gradient_homing.inc and prhf_gradient_hops.inc, inside namespace prhf.  Every ray here is grad_ray<GEO, FULL> of
// prhf_gradient.inc: FULL = false (the range-only ray) for the scan and the refinement, FULL = true for the result rows,
// so that a ray of a given field, launch point, elevation and controls has the bits prhf_trace_gradient_f64 /
// prhf_trace_gradient_spherical_f64 give it.  The reference has none of the three; DESIGN.md section 4.11 defines them:
// the rule is section 4.10's.
//
// Fields (launch_field_bmax, launch_field_build): per node and frequency f_N = sqrt(Ne) c_p, X = (f_N f_N) / (f f),
// Y = (g_p B) / f, each operation rounded once, then index_faithful<mode> - or index_unmagnetised when that frequency's
// field is isotropic: nanmax|Y| < 1e-12 with at least one Y that is not NaN, prhf_mu_mup_f64's decision on that
// frequency's Y array.  Rounding is monotone, so nanmax|Y| = |(g_p Bmax) / f| with Bmax = nanmax|B|: one reduction per
// call (field_bmax_kernel) leaves Bmax in two device words and the build needs no pass over Y and no host round trip.
// The records come from field_pack_kernel as it is.
//
// Skip distance (launch_grad_skip), four kernels and no host round trip in between:
//   scan     grad_skip_scan_kernel<GEO>: grad_home_scan_kernel's body: one range-only ray per lane, ceil(E / 64)
//            wavefronts per group: D_i = ground_range_km of the group's ray at e_i into scan_d (n_groups, E).
//   node     grad_skip_node_kernel: one wavefront per group, 64 scan nodes a trip: i* = the first index that attains the
//            minimum over the finite D_i (the wavefront's minimum, then the first lane that holds it, as
//            skip_refine_kernel finds it).  It writes the row's head: NaN and status -1 when no ray lands, the node as it
//            stands (status 1) when i* is at either end of the scan or beside a node that does not land; every other group
//            goes to the work list as (group, i*), one atomic per wavefront.
//   refine   grad_skip_refine_kernel<GEO>: one record of the work list per LANE (a gradient ray is a lane's work): the
//            golden-section search of section 4.10 on (e_i*-1, e_i*, e_i*+1) with range-only rays.  The state (a, b, c,
//            D_b, x and three ints) stays in registers across a ray; the wavefront loops until a ballot finds no lane at
//            work, at most max_iter + 1 trips.  The order of the work list decides which lane refines a group and nothing
//            else.
//   result   grad_skip_result_kernel<GEO>: one group per lane: the full two-pass ray at the row's elevation, its twelve
//            outputs behind the row's head - edge groups too; a row without a ray (status -1) never reaches the tracer.
// MUF (launch_grad_muf): a link is its own group on its own field.  Per trip grad_muf_set_kernel writes every link's
// next frequency and its "is searching" word, the fields of those frequencies are built and packed, the scan, the node
// kernel and the refinement run on them and grad_muf_decide_kernel moves the link's frequency bracket and keeps the head
// of the search's row at lo; settled links are skipped by the build and by every tracer kernel.  After the last trip the
// fields at the result frequencies are built once more and the result kernel traces the rows' rays.  Everything is
// enqueued on one stream; the host waits once.
// queue[]: 0 the work list's length (zeroed by every scan launch), 1 rays traced by the refine lanes, 2 ray slots (64
// per trip of a refine wavefront's loop), 3 refine wavefronts with work, 4 groups refined: lane utilisation = [1] / [2].
//
// Multi-hop (DESIGN.md section 4.13, prhf_gradient_hop_skip_f64 / prhf_gradient_hop_muf_f64): the same rule with D(e)
// the landing x of hop g.n_hops - 1 of the chain launched at e - grad_hops<GEO, false> of prhf_gradient_hops.inc, NaN
// unless every hop lands - and a row of 6 + PRHF_GRAD_HOP_OUTPUTS g.n_hops doubles: the head, then grad_hops<GEO, true>
// at the row's elevation.  The scan, refine and result kernels are instantiated on a compile-time CHAIN flag: false is
// the one-hop call as it was (the direct grad_ray, rows of 18), true the chain; the entry point chooses.  The node and
// the MUF kernels take the row's stride from h.row_width.  A ray slot is still one lane-trip, whatever the hops;
// queue[5] counts the hops of the refine lanes' chains that landed (n_hops each; a chain that does not land ends its
// group's search and is counted under [1] alone).

namespace {

constexpr int kGradSkipOutputs = PRHF_GRAD_SKIP_OUTPUTS;
constexpr int kGradSkipHead = PRHF_GRAD_SKIP_OUTPUTS - PRHF_GRAD_OUTPUTS;   // skip_km .. n_evals

// ---- fields -----------------------------------------------------------------------------------------------------------
// words[0] = nanmax|B| as a bit pattern (it orders like the double for non-negative values), words[1] != 0 when any B is
// not NaN: mu_mup_kernel's pair of words for |Y|.  The words are zero when the kernel starts.
__global__ __launch_bounds__(256) void field_bmax_kernel(const double* __restrict__ bmag, long long plane,
                                                         unsigned long long* words) {
    double bmax = 0.0;
    int seen = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += (long long)gridDim.x * blockDim.x) {
        const double ab = fabs(bmag[i]);
        bmax = fmax(bmax, ab);
        seen |= (ab == ab) ? 1 : 0;
    }
    __shared__ double wg_max[4];
    __shared__ int wg_seen[4];
    bmax = wave_max(bmax);
    seen = __any(seen) ? 1 : 0;
    if ((threadIdx.x & 63) == 0) { wg_max[threadIdx.x >> 6] = bmax; wg_seen[threadIdx.x >> 6] = seen; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) { bmax = fmax(bmax, wg_max[w]); seen |= wg_seen[w]; }
        atomicMax(words, (unsigned long long)__double_as_longlong(bmax));
        if (seen) atomicOr(words + 1, 1ull);
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void field_build_kernel(const FieldBuildArgs a) {
#pragma clang fp contract(off)
    const long long total = a.n_freq * a.plane;
    const double bmax = __longlong_as_double((long long)a.bmax[0]);
    const bool seen = a.bmax[1] != 0;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long f = t / a.plane, node = t - f * a.plane;
        if (a.active && a.active[f] == 0) continue;
        const double fr = a.freq[f];
        const double fn = sqrt(a.den[node]) * kPlasma;             // library.py:96
        const double X = (fn * fn) / (fr * fr);                     // :137 on arrays: both squares are products
        const double Y = (kGyro * a.bmag[node]) / fr;               // :157
        // :201 on this frequency's Y array: nanmax|Y| is the image of nanmax|B| (an all-NaN B, or a NaN frequency: magnetised)
        const double ymax = fabs((kGyro * bmax) / fr);
        double mu, mup;
        if (seen && ymax < kUnmagTol) index_unmagnetised(X, &mu, &mup);
        else index_faithful<MODE>(X, Y, a.bpsi[node], &mu, &mup);
        a.mu[t] = mu;
        a.mup[t] = mup;
    }
}

// ---- skip distance ----------------------------------------------------------------------------------------------------
// D(e): the range-only ray, or the range-only chain of a.n_hops hops
template <int GEO, bool CHAIN>
__device__ __forceinline__ double grad_skip_range(const GradTraceArgs& a, const double* axes, long long field, double elev_deg,
                                                  double x0_km, double z0_km) {
    if (CHAIN) return grad_hops<GEO, false>(a, axes, axes + a.n0, 0, field, elev_deg, x0_km, z0_km, nullptr);
    return grad_ray<GEO, false>(a, axes, axes + a.n0, 0, field, elev_deg, x0_km, z0_km, nullptr);
}

template <int GEO, bool CHAIN>
__global__ __launch_bounds__(PRHF_GRAD_TRACE_THREADS) void grad_skip_scan_kernel(const GradSkipArgs h) {
    extern __shared__ __attribute__((aligned(16))) double grad_axes[];
    if (blockIdx.x == 0 && threadIdx.x == 0) h.queue[0] = 0u;      // (the work list's length: read two kernels on)
    const unsigned per_group = (unsigned)((h.n_scan + 63) / 64);
    const long long grp = blockIdx.x / per_group;
    if (h.active && h.active[grp] == 0) return;                     // (the whole workgroup: one group)
    grad_home_stage_axes(h.g, grad_axes);
    const int i = (int)(blockIdx.x - grp * per_group) * 64 + (int)threadIdx.x;
    if (i >= h.n_scan) return;
    const long long f = h.group_field[grp];
    double d = qnan();
    if (f < 0 || f >= h.g.n_fields)       // (device-resident group_field: not checked by the host) no ray, a NaN row
        post_status(h.g.status, (unsigned)PRHF_STATUS_BADFIELD);
    else
        d = grad_skip_range<GEO, CHAIN>(h.g, grad_axes, f, h.scan_elev[i], h.group_x0[grp], h.group_z0[grp]);
    h.scan_d[grp * h.n_scan + i] = d;
}

__global__ __launch_bounds__(64) void grad_skip_node_kernel(const GradSkipArgs h) {
    const int lane = threadIdx.x & 63;
    const long long g = blockIdx.x;
    if (h.active && h.active[g] == 0) return;
    const double* d = h.scan_d + g * h.n_scan;
    double* row = h.out + g * h.row_width;
    const double inf = __builtin_inf();
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
        // (behind the head: NaN for the one-hop call, the chain call's hop rows unused as grad_hops writes them)
        const bool hop_rows = h.row_width != kGradSkipOutputs;
        for (int k = lane; k < h.row_width; k += 64)
            row[k] = (k == 2 || k == 3) ? -1.0 : (k == 5) ? 0.0
                     : (hop_rows && k >= kGradSkipHead) ? grad_hop_unused((k - kGradSkipHead) % PRHF_GRAD_HOP_OUTPUTS) : qnan();
        return;
    }
    const bool edge = i_min == 0 || i_min == h.n_scan - 1 || !finite64(d[max(i_min - 1, 0)]) ||
                      !finite64(d[min(i_min + 1, h.n_scan - 1)]);
    if (lane != 0) return;
    if (edge) {
        row[0] = d_min;
        row[1] = h.scan_elev[i_min];
        row[2] = 1.0;
        row[3] = (double)i_min;
        row[4] = qnan();
        row[5] = 0.0;
    } else {
        const unsigned at = atomicAdd(h.queue, 1u);                // at < n_groups: one entry per group at most
        reinterpret_cast<int2*>(h.work)[at] = make_int2((int)g, i_min);
    }
}

template <int GEO, bool CHAIN>
__global__ __launch_bounds__(PRHF_GRAD_TRACE_THREADS) void grad_skip_refine_kernel(const GradSkipArgs h) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double grad_axes[];
    const unsigned n_work = h.queue[0];
    if ((unsigned long long)blockIdx.x * 64ull >= n_work) return;
    grad_home_stage_axes(h.g, grad_axes);
    const int lane = threadIdx.x & 63;
    const unsigned long long w = (unsigned long long)blockIdx.x * 64ull + (unsigned)lane;
    const bool mine = w < n_work;
    const double gold = 0.3819660112501051;
    long long g = 0, f = 0;
    int i = 0, status = 3, n_evals = 0;
    double x0 = 0.0, z0 = 0.0, e_a = 0.0, e_b = 0.0, e_c = 0.0, d_b = 0.0;
    if (mine) {
        const int2 rec = reinterpret_cast<const int2*>(h.work)[w];
        g = rec.x; i = rec.y;                                       // (0 < i < n_scan - 1, D finite at i - 1, i, i + 1: the node kernel)
        f = h.group_field[g];                                       // (in range: a group with a bad field has no finite D)
        x0 = h.group_x0[g]; z0 = h.group_z0[g];
        e_a = h.scan_elev[i - 1]; e_b = h.scan_elev[i]; e_c = h.scan_elev[i + 1];
        d_b = h.scan_d[g * h.n_scan + i];
    }
    bool busy = mine;
    unsigned rays = 0, trips = 0, landed = 0;
    // golden-section search on (a, b, c): D_b is the least ground range seen; at most max_iter rays, one per trip
    for (int trip = 0; trip <= h.max_iter && __ballot(busy) != 0; ++trip) {
        ++trips;
        if (busy) {
            const bool right = (e_c - e_b) >= (e_b - e_a);
            const double x = right ? e_b + gold * (e_c - e_b) : e_b - gold * (e_b - e_a);
            if (e_c - e_a <= h.elev_tol) {
                status = 0; busy = false;
            } else if (!(x > e_a && x < e_c) || x == e_b) {
                status = 0; busy = false;                           // the doubles are exhausted
            } else if (n_evals >= h.max_iter) {
                status = 3; busy = false;
            } else {
                const double dx = grad_skip_range<GEO, CHAIN>(h.g, grad_axes, f, x, x0, z0);
                ++n_evals;
                ++rays;
                if (CHAIN && finite64(dx)) ++landed;
                if (!finite64(dx)) {
                    status = 2; busy = false;                       // the ray does not land inside the bracket
                } else if (dx < d_b) {
                    if (right) e_a = e_b; else e_c = e_b;
                    e_b = x;
                    d_b = dx;
                } else {                                            // (a tie keeps b)
                    if (right) e_c = x; else e_a = x;
                }
            }
        }
    }
    if (mine) {
        double* row = h.out + g * h.row_width;
        row[0] = d_b;
        row[1] = e_b;
        row[2] = (double)status;
        row[3] = (double)i;
        row[4] = e_c - e_a;
        row[5] = (double)n_evals;
        if (rays) atomicAdd(h.queue + 1, rays);
        if (CHAIN && landed) atomicAdd(h.queue + 5, landed * (unsigned)h.g.n_hops);
    }
    if (lane == 0) {
        atomicAdd(h.queue + 2, 64u * trips);
        atomicAdd(h.queue + 3, 1u);
        if (blockIdx.x == 0) atomicAdd(h.queue + 4, n_work);
    }
}

template <int GEO, bool CHAIN>
__global__ __launch_bounds__(PRHF_GRAD_TRACE_THREADS) void grad_skip_result_kernel(const GradSkipArgs h) {
    extern __shared__ __attribute__((aligned(16))) double grad_axes[];
    grad_home_stage_axes(h.g, grad_axes);
    const long long g = (long long)blockIdx.x * 64 + threadIdx.x;
    if (g >= h.n_groups) return;
    if (h.active && h.active[g] == 0) return;
    double* row = h.out + g * h.row_width;
    if (row[2] == -1.0) return;                                     // no ray of the scan lands (or a bad field): NaN row
    if (CHAIN)
        (void)grad_hops<GEO, true>(h.g, grad_axes, grad_axes + h.g.n0, 0, h.group_field[g], row[1], h.group_x0[g],
                                   h.group_z0[g], row + kGradSkipHead);
    else
        (void)grad_ray<GEO, true>(h.g, grad_axes, grad_axes + h.g.n0, 0, h.group_field[g], row[1], h.group_x0[g],
                                  h.group_z0[g], row + kGradSkipHead);
}

// ---- MUF: one thread per link -----------------------------------------------------------------------------------------
// state (n_links, 4): lo, hi, link status, 0.  phase 0: f_lo, 1: f_hi, 2: a bisection trip, 3: the result frequency.
__global__ __launch_bounds__(64) void grad_muf_set_kernel(const GradMufArgs m, int phase) {
#pragma clang fp contract(off)
    const long long l = (long long)blockIdx.x * 64 + threadIdx.x;
    if (l >= m.n_links) return;
    double f = m.f_lo;
    int on = 1;
    if (phase == 0) {
        m.group_field[l] = l;
    } else if (phase == 1) {
        on = m.state[4 * l + 2] == 0.0 ? 1 : 0;                     // (a NaN target, or S(f_lo) beyond it: settled)
        f = m.f_hi;
    } else if (phase == 2) {
        const double lo = m.state[4 * l], hi = m.state[4 * l + 1];
        const double mid = lo + 0.5 * (hi - lo);
        on = (m.state[4 * l + 2] == 0.0 && mid > lo && mid < hi) ? 1 : 0;   // (a trip that cannot split changes nothing)
        if (on) f = mid;
    } else {
        const double st = m.state[4 * l + 2];
        on = (st == 0.0 || st == 1.0) ? 1 : 0;
        if (on) {
            f = m.state[4 * l];
            for (int k = 0; k < kGradSkipHead; ++k) m.k.out[l * m.k.row_width + k] = m.best[l * kGradSkipHead + k];
        }
    }
    m.group_freq[l] = f;
    m.active[l] = on;
}

__global__ __launch_bounds__(64) void grad_muf_decide_kernel(const GradMufArgs m, int phase) {
    const long long l = (long long)blockIdx.x * 64 + threadIdx.x;
    if (l >= m.n_links) return;
    const double* cur = m.k.out + l * m.k.row_width;
    double* s = m.state + 4 * l;
    if (phase == 3) {
        double* row = m.out + l * (3 + m.k.row_width);
        const bool none = s[2] == -1.0 || s[2] == 2.0;
        row[0] = none ? qnan() : s[0];
        row[1] = none ? qnan() : s[1];
        row[2] = s[2];
        for (int k = 0; k < m.k.row_width; ++k) row[3 + k] = none ? qnan() : cur[k];
        return;
    }
    if (m.active[l] == 0) return;
    double* best = m.best + l * kGradSkipHead;
    const double t = m.link_target[l];
    // S(f): the skip distance, +inf when no ray of the scan lands
    const double sf = cur[2] == -1.0 ? __builtin_inf() : cur[0];
    bool take = false;
    if (phase == 0) {
        s[0] = m.f_lo; s[1] = m.f_hi; s[3] = 0.0;
        s[2] = (t != t) ? -1.0 : (sf > t) ? 2.0 : 0.0;
        take = true;
    } else if (phase == 1) {
        if (sf <= t) { s[2] = 1.0; s[0] = m.f_hi; s[1] = qnan(); take = true; }
    } else {
        if (sf <= t) { s[0] = m.group_freq[l]; take = true; }
        else s[1] = m.group_freq[l];
    }
    if (take)
        for (int k = 0; k < kGradSkipHead; ++k) best[k] = cur[k];
}

// One launch of kernel<GEO, CHAIN> for the call's geometry and kind
#define PRHF_GRAD_SKIP_LAUNCH(kernel, grid)                                                                        \
    do {                                                                                                           \
        if (sph && chain) hipLaunchKernelGGL((kernel<PRHF_GEO_SPHERICAL, true>), grid, threads, lds, stream, h);   \
        else if (sph) hipLaunchKernelGGL((kernel<PRHF_GEO_SPHERICAL, false>), grid, threads, lds, stream, h);      \
        else if (chain) hipLaunchKernelGGL((kernel<PRHF_GEO_CARTESIAN, true>), grid, threads, lds, stream, h);     \
        else hipLaunchKernelGGL((kernel<PRHF_GEO_CARTESIAN, false>), grid, threads, lds, stream, h);               \
    } while (0)

hipError_t grad_skip_enqueue(const GradSkipArgs& h, bool chain, bool search, bool result, hipStream_t stream) {
    const long long per_group = (h.n_scan + 63) / 64;
    const size_t lds = field_axes_lds_bytes(h.g.n0, h.g.n1);
    const dim3 threads(PRHF_GRAD_TRACE_THREADS), scan_grid((unsigned)(h.n_groups * per_group)),
        row_grid((unsigned)((h.n_groups + 63) / 64));
    const bool sph = h.g.geometry == PRHF_GEO_SPHERICAL;
    hipError_t e;
    if (search) {
        PRHF_GRAD_SKIP_LAUNCH(grad_skip_scan_kernel, scan_grid);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(grad_skip_node_kernel, dim3((unsigned)h.n_groups), dim3(64), 0, stream, h);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        PRHF_GRAD_SKIP_LAUNCH(grad_skip_refine_kernel, row_grid);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (result) PRHF_GRAD_SKIP_LAUNCH(grad_skip_result_kernel, row_grid);
    return hipGetLastError();
}
#undef PRHF_GRAD_SKIP_LAUNCH

// (a chain call: 1 .. PRHF_GRAD_MAX_HOPS hops and the row that holds them; the one-hop call: rows of 18)
bool grad_skip_rows_fit(const GradSkipArgs& h, bool chain) {
    if (!chain) return h.row_width == kGradSkipOutputs;
    return h.g.n_hops >= 1 && h.g.n_hops <= PRHF_GRAD_MAX_HOPS && h.row_width == kGradSkipHead + PRHF_GRAD_HOP_OUTPUTS * h.g.n_hops;
}

bool grad_skip_fits(const GradSkipArgs& h) {
    return h.n_groups <= 0x7fffffffLL && h.n_groups * (long long)((h.n_scan + 63) / 64) <= 0x7fffffffLL;
}

}  // namespace

hipError_t launch_field_bmax(const double* bmag, long long plane, unsigned long long* words, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(words, 0, 2 * sizeof(unsigned long long), stream);
    if (e != hipSuccess || plane <= 0) return e;
    const unsigned blocks = (unsigned)((plane + 255) / 256 < 1024 ? (plane + 255) / 256 : 1024);
    hipLaunchKernelGGL(field_bmax_kernel, dim3(blocks), dim3(256), 0, stream, bmag, plane, words);
    return hipGetLastError();
}

hipError_t launch_field_build(const FieldBuildArgs& a, hipStream_t stream) {
    const long long total = a.n_freq * a.plane;
    if (total <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
    if (a.mode == PRHF_KMODE_O) hipLaunchKernelGGL(field_build_kernel<PRHF_KMODE_O>, dim3(blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(field_build_kernel<PRHF_KMODE_X>, dim3(blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_grad_skip(const GradSkipArgs& h, bool chain, hipStream_t stream) {
    if (h.n_groups <= 0) return hipSuccess;
    if (!grad_skip_fits(h) || !grad_skip_rows_fit(h, chain)) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(h.queue, 0, PRHF_GRAD_SKIP_QUEUE_WORDS * sizeof(unsigned), stream);
    if (e != hipSuccess) return e;
    return grad_skip_enqueue(h, chain, true, true, stream);
}

hipError_t launch_grad_muf(const GradMufArgs& m, bool chain, hipStream_t stream) {
    if (m.n_links <= 0) return hipSuccess;
    if (!grad_skip_fits(m.k) || !grad_skip_rows_fit(m.k, chain)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(m.k.queue, 0, PRHF_GRAD_SKIP_QUEUE_WORDS * sizeof(unsigned), stream);
    if (e != hipSuccess) return e;
    e = launch_field_bmax(m.b.bmag, m.b.plane, const_cast<unsigned long long*>(m.b.bmax), stream);
    if (e != hipSuccess) return e;
    const dim3 links((unsigned)((m.n_links + 63) / 64));
    // S(f_lo), S(f_hi), n_bisect trips, then the rows at the result frequencies
    for (int trip = 0; trip < 3 + m.n_bisect; ++trip) {
        const int phase = trip < 2 ? trip : trip < 2 + m.n_bisect ? 2 : 3;
        hipLaunchKernelGGL(grad_muf_set_kernel, links, dim3(64), 0, stream, m, phase);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = launch_field_build(m.b, stream);
        if (e != hipSuccess) return e;
        e = launch_field_pack(m.p, stream);
        if (e != hipSuccess) return e;
        e = grad_skip_enqueue(m.k, chain, phase != 3, phase == 3, stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(grad_muf_decide_kernel, links, dim3(64), 0, stream, m, phase);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
