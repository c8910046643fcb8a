// prhf_gradient_hops.inc - multi-hop rays for the gradient tracers of both geometries: a ray that lands is reflected off
// the ground and traced on, up to n_hops times, as one lane's work.  Included by prhf_kernels.hip behind
// prhf_gradient_homing.inc (whose kernels take D(e) from grad_hops, declared there), inside namespace prhf.  The
// reference has no such call; DESIGN.md section 4.12 defines the chain and include/prhf.h writes it out.  Every hop is
// grad_ray<GEO, FULL> of prhf_gradient.inc: a used hop row has the bits prhf_trace_gradient_f64 /
// prhf_trace_gradient_spherical_f64 give for that row's launch point, elevation, field and controls.

namespace {

// The chain of a.n_hops hops of field `field` from (x0_km, z0_km) at `elev_deg`.  Hop h + 1 exists while hop h ends on
// the ground (status 0); it launches at x = that hop's ground_range_km, z = a.hop_z0 (z_ground_km as the caller gave
// it) with the elevation atan2(-v_vert, v_horiz) (180 / pi) of that hop's last path node - (vx, vz) of a Cartesian
// state, (v_phi, v_r) of a spherical one -: specular reflection, the direction normalised again by the launch.
// Returns the landing x of the last hop, NaN unless every hop lands.
// FULL: `out` is (n_hops, PRHF_GRAD_HOP_OUTPUTS) - launch x, launch z, launch elevation, then the tracer's twelve -,
// the path of hop h goes to row r * n_hops + h of a.path_*; rows behind the first hop that does not land are unused:
// NaN, status -1, the three counters and the pad 0.  !FULL: range-only hops, `r` and `out` are not used.
template <int GEO, bool FULL>
__device__ __forceinline__ double grad_hops(const GradTraceArgs& a, const double* g0, const double* g1, long long r,
                                            long long field, double elev_deg, double x0_km, double z0_km, double* out) {
    double x = x0_km, z = z0_km, e = elev_deg, d = qnan();
    int h = 0;
#pragma nounroll
    for (; h < a.n_hops; ++h) {
        double* row = FULL ? out + h * PRHF_GRAD_HOP_OUTPUTS : nullptr;
        if (FULL) { row[0] = x; row[1] = z; row[2] = e; }
        double v[2];
        d = grad_ray<GEO, FULL>(a, g0, g1, r * a.n_hops + h, field, e, x, z, FULL ? row + 3 : nullptr, v);
        // (range-only: a hop that does not land returns NaN, and a chain through a NaN landing x ends in NaN anyway)
        const bool landed = FULL ? row[3 + 7] == 0.0 : d == d;
        if (!landed) { d = qnan(); ++h; break; }
        const double v_horiz = GEO == PRHF_GEO_SPHERICAL ? v[1] : v[0], v_vert = GEO == PRHF_GEO_SPHERICAL ? v[0] : v[1];
        x = d;
        z = a.hop_z0;
        e = atan2(-v_vert, v_horiz) * (180.0 / 3.141592653589793);
    }
    if (FULL)
        for (; h < a.n_hops; ++h) grad_hop_unused_row(out + h * PRHF_GRAD_HOP_OUTPUTS);
    return d;
}

template <int GEO>
__global__ __launch_bounds__(PRHF_GRAD_TRACE_THREADS) void grad_hop_trace_kernel(const GradTraceArgs a) {
    extern __shared__ __attribute__((aligned(16))) double grad_axes[];
    const double* g0 = grad_axes;
    const double* g1 = grad_axes + a.n0;
    for (int i = threadIdx.x; i < a.n0 + a.n1; i += blockDim.x) grad_axes[i] = i < a.n0 ? a.a0[i] : a.a1[i - a.n0];
    __syncthreads();
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_rays) return;
    double* out = a.out + r * ((long long)a.n_hops * PRHF_GRAD_HOP_OUTPUTS);
    const long long f = a.ray_field ? a.ray_field[r] : 0;
    if (f < 0 || f >= a.n_fields) {
        post_status(a.status, (unsigned)PRHF_STATUS_BADFIELD);
        for (int k = 0; k < a.n_hops * PRHF_GRAD_HOP_OUTPUTS; ++k) out[k] = qnan();
        return;
    }
    (void)grad_hops<GEO, true>(a, g0, g1, r, f, a.elev[r], a.x0[r], a.z0[r], out);
}

}  // namespace

hipError_t launch_grad_hop_trace(const GradTraceArgs& a, hipStream_t stream) {
    if (a.n_rays <= 0) return hipSuccess;
    const long long blocks = (a.n_rays + PRHF_GRAD_TRACE_THREADS - 1) / PRHF_GRAD_TRACE_THREADS;
    if (blocks > 0x7fffffffLL || a.n_hops < 1 || a.n_hops > PRHF_GRAD_MAX_HOPS) return hipErrorInvalidValue;
    if (a.geometry == PRHF_GEO_SPHERICAL)
        hipLaunchKernelGGL(grad_hop_trace_kernel<PRHF_GEO_SPHERICAL>, dim3((unsigned)blocks), dim3(PRHF_GRAD_TRACE_THREADS),
                           field_axes_lds_bytes(a.n0, a.n1), stream, a);
    else
        hipLaunchKernelGGL(grad_hop_trace_kernel<PRHF_GEO_CARTESIAN>, dim3((unsigned)blocks), dim3(PRHF_GRAD_TRACE_THREADS),
                           field_axes_lds_bytes(a.n0, a.n1), stream, a);
    return hipGetLastError();
}
