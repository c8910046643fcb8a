// prhf_gradient.inc - 2-D refractive-index fields mu(a0, a1) and the gradient ray tracers of both geometries.
// Included by prhf_kernels.hip inside namespace prhf.
//
// Replaces: build_refractive_index_interpolator_cartesian / _spherical (reference PyRayHF/library.py:1755-1927),
// build_mup_function (:1930-2017), ray_rhs_cartesian (:953-1006), the event helpers (:1009-1031),
// trace_ray_cartesian_gradient (:1270-1457), rhs_spherical (:2094-2125) and trace_ray_spherical_gradient (:2128-2337,
// with the stop conditions of DESIGN.md section 4.7).  Line numbers below are that file.
//
// FIELD RECORDS (field_pack_kernel): node (f, i0, i1) of a field is four doubles {mu, d mu/d a1, d mu/d a0, mu'}, the
// derivatives np.gradient(mu, a0, a1, edge_order) in NumPy's formulas and operation order (IEEE + - x /, no
// contraction: bit-identical).  The two a1-neighbours of a cell are 64 contiguous bytes.
//
// SAMPLER (field_sample_kernel, field_locate / field_blend): scipy.interpolate.RegularGridInterpolator(method="linear",
// bounds_error=False): cell i with g[i] <= v < g[i + 1] (v = g[n - 1]: the last cell), normalised distances
// (v - g[i]) / (g[i + 1] - g[i]), the four products formed left to right and added left to right (a NaN corner
// poisons the sum at weight 0), fill values outside the hull, NaN for a NaN coordinate.
//
// TRACER (grad_trace_kernel<GEO>): one ray per lane.  Dormand-Prince 5(4) with the step controller that
// scipy.integrate.solve_ivp(method="RK45") documents; the state y = (x, z, vx, vz) - (r, phi, v_r, v_phi) for
// GEO = PRHF_GEO_SPHERICAL -, the seven stage vectors and the controller live in registers, accept / reject is per lane
// and a wave loops until a ballot shows no active lane.  The two axes are staged in LDS; a lane remembers its last cell
// and hunts +-1 from it before it searches.  The geometry is a template parameter: the spherical instantiation differs
// in the right-hand side, in the state component an event looks at, in a chord's length, in the point mu' is sampled
// at and in the midpoint rule; stepper, controller, event location and path writer are shared text.

namespace {

#define PRHF_GRAD_THREADS 256        // pack and sampler: one node / one point per thread
#define PRHF_GRAD_TRACE_THREADS 64   // tracer: one wave per workgroup, so that a fan of a few thousand rays reaches every CU

// np.gradient along one axis: f[k * s] is the value at axis index k of n, x the axis coordinates.  `uniform`: all
// np.diff(x) are equal (NumPy then divides by the scalar x[1] - x[0]).
__device__ __forceinline__ double np_gradient_1d(const double* f, long long s, long long i, long long n, const double* x,
                                                 int uniform, int edge_order) {
    if (i > 0 && i < n - 1) {
        if (uniform) {
            const double dx = x[1] - x[0];
            return (f[(i + 1) * s] - f[(i - 1) * s]) / (2. * dx);
        }
        const double dx1 = x[i] - x[i - 1], dx2 = x[i + 1] - x[i];
        const double a = -(dx2) / (dx1 * (dx1 + dx2));
        const double b = (dx2 - dx1) / (dx1 * dx2);
        const double c = dx1 / (dx2 * (dx1 + dx2));
        return a * f[(i - 1) * s] + b * f[i * s] + c * f[(i + 1) * s];
    }
    if (edge_order == 1) {
        if (i == 0) return (f[s] - f[0]) / (x[1] - x[0]);
        const double dxn = uniform ? x[1] - x[0] : x[n - 1] - x[n - 2];
        return (f[(n - 1) * s] - f[(n - 2) * s]) / dxn;
    }
    double a, b, c;
    if (i == 0) {
        if (uniform) {
            const double dx = x[1] - x[0];
            a = -1.5 / dx; b = 2. / dx; c = -0.5 / dx;
        } else {
            const double dx1 = x[1] - x[0], dx2 = x[2] - x[1];
            a = -(2. * dx1 + dx2) / (dx1 * (dx1 + dx2));
            b = (dx1 + dx2) / (dx1 * dx2);
            c = -dx1 / (dx2 * (dx1 + dx2));
        }
        return a * f[0] + b * f[s] + c * f[2 * s];
    }
    if (uniform) {
        const double dx = x[1] - x[0];
        a = 0.5 / dx; b = -2. / dx; c = 1.5 / dx;
    } else {
        const double dx1 = x[n - 2] - x[n - 3], dx2 = x[n - 1] - x[n - 2];
        a = (dx2) / (dx1 * (dx1 + dx2));
        b = -(dx2 + dx1) / (dx1 * dx2);
        c = (2. * dx2 + dx1) / (dx2 * (dx1 + dx2));
    }
    return a * f[(n - 3) * s] + b * f[(n - 2) * s] + c * f[(n - 1) * s];
}

__global__ __launch_bounds__(PRHF_GRAD_THREADS) void field_pack_kernel(const FieldPackArgs a) {
    const long long plane = (long long)a.n0 * a.n1, total = plane * a.n_fields;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long f = t / plane, node = t - f * plane, i0 = node / a.n1, i1 = node - i0 * a.n1;
        const double* mu = a.mu + f * plane;
        double2 lo, hi;
        lo.x = mu[node];
        lo.y = np_gradient_1d(mu + i0 * a.n1, 1, i1, a.n1, a.a1, a.uniform1, a.edge_order);
        hi.x = np_gradient_1d(mu + i1, a.n1, i0, a.n0, a.a0, a.uniform0, a.edge_order);
        hi.y = a.mup[t];
        double2* rec = reinterpret_cast<double2*>(a.rec + 4 * t);
        rec[0] = lo;
        rec[1] = hi;
    }
}

// The cell of v on the axis g[0 .. n), g[0] <= v <= g[n - 1]: i with g[i] <= v < g[i + 1], the last cell for
// v = g[n - 1] (SciPy's find_interval_ascending).  `last`: the lane's previous cell, in [0, n - 2].
__device__ __forceinline__ int field_cell(const double* g, int n, double v, int last) {
    int i = last;
    if (v >= g[i] && v < g[i + 1]) return i;
    if (i + 2 < n && v >= g[i + 1] && v < g[i + 2]) return i + 1;
    if (i > 0 && v >= g[i - 1] && v < g[i]) return i - 1;
    int lo = 0, hi = n - 2;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (v >= g[mid]) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// 0: inside the hull (c0, c1, y0, y1 set), 1: outside, 2: a NaN coordinate
__device__ __forceinline__ int field_locate(const double* g0, int n0, const double* g1, int n1, double a0, double a1,
                                            int& c0, int& c1, double& y0, double& y1) {
    if (a0 != a0 || a1 != a1) return 2;
    if (a0 < g0[0] || a0 > g0[n0 - 1] || a1 < g1[0] || a1 > g1[n1 - 1]) return 1;
    c0 = field_cell(g0, n0, a0, c0);
    c1 = field_cell(g1, n1, a1, c1);
    y0 = (a0 - g0[c0]) / (g0[c0 + 1] - g0[c0]);
    y1 = (a1 - g1[c1]) / (g1[c1 + 1] - g1[c1]);
    return 0;
}

__device__ __forceinline__ double field_blend(double v00, double v01, double v10, double v11, double y0, double y1) {
    return v00 * (1 - y0) * (1 - y1) + v01 * (1 - y0) * y1 + v10 * y0 * (1 - y1) + v11 * y0 * y1;
}

// The four corner records of cell (c0, c1) of field f: r[0], r[1] = node (c0, c1), r[2], r[3] = (c0, c1 + 1), then row c0 + 1.
struct FieldCorners {
    double2 r[8];
};
template <bool LOW, bool HIGH>
__device__ __forceinline__ void field_corners(const double* rec, long long f, int n0, int n1, int c0, int c1, FieldCorners& q) {
    const double2* p = reinterpret_cast<const double2*>(rec + 4 * ((f * n0 + c0) * (long long)n1 + c1));
    const double2* p1 = p + 2 * (long long)n1;
    if (LOW) { q.r[0] = p[0]; q.r[2] = p[2]; q.r[4] = p1[0]; q.r[6] = p1[2]; }
    if (HIGH) { q.r[1] = p[1]; q.r[3] = p[3]; q.r[5] = p1[1]; q.r[7] = p1[3]; }
}

__global__ __launch_bounds__(PRHF_GRAD_THREADS) void field_sample_kernel(const FieldSampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) double grad_axes[];
    double* g0 = grad_axes;
    double* g1 = grad_axes + a.n0;
    for (int i = threadIdx.x; i < a.n0 + a.n1; i += blockDim.x) grad_axes[i] = i < a.n0 ? a.a0[i] : a.a1[i - a.n0];
    __syncthreads();
    int c0 = 0, c1 = 0;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < a.n; t += (long long)gridDim.x * blockDim.x) {
        const long long f = a.field ? a.field[t] : 0;
        double y0 = 0, y1 = 0;
        double o0, o1, o2, o3;
        int where = field_locate(g0, a.n0, g1, a.n1, a.p0[t], a.p1[t], c0, c1, y0, y1);
        if (f < 0 || f >= a.n_fields) {          // device-resident indices: NaN, nothing outside the records is read
            post_status(a.status, (unsigned)PRHF_STATUS_BADFIELD);
            where = 2;
        }
        if (where == 0) {
            FieldCorners q;
            field_corners<true, true>(a.rec, f, a.n0, a.n1, c0, c1, q);
            o0 = field_blend(q.r[0].x, q.r[2].x, q.r[4].x, q.r[6].x, y0, y1);
            o1 = field_blend(q.r[0].y, q.r[2].y, q.r[4].y, q.r[6].y, y0, y1);
            o2 = field_blend(q.r[1].x, q.r[3].x, q.r[5].x, q.r[7].x, y0, y1);
            o3 = field_blend(q.r[1].y, q.r[3].y, q.r[5].y, q.r[7].y, y0, y1);
        } else if (where == 1) {
            o0 = a.fill_n; o1 = o2 = a.fill_grad; o3 = a.fill_mup;
        } else {
            o0 = o1 = o2 = o3 = qnan();
        }
        if (a.out_n) a.out_n[t] = o0;
        if (a.out_d1) a.out_d1[t] = o1;
        if (a.out_d0) a.out_d0[t] = o2;
        if (a.out_mup) a.out_mup[t] = o3;
    }
}

// ---- tracer ----------------------------------------------------------------------------------------------------

// Python's max(a, b) / min(a, b) on floats (the second argument wins only when it compares greater / less: a NaN in
// second place is dropped, as in the controller solve_ivp runs)
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }
// np.maximum: a NaN wins
__device__ __forceinline__ double np_maximum(double a, double b) { return (a > b || a != a) ? a : b; }

struct GradLane {
    long long f;        // field of the ray
    int c0, c1;         // last cell
    unsigned valid;     // RHS calls with a usable mu so far (the reference's eval_counter, :996)
    unsigned n_rhs;     // all RHS calls
};

// The right-hand side on the sampled field.  Cartesian: ray_rhs_cartesian (:983-1006), y = (x, z, vx, vz).
// Spherical: rhs_spherical (:2094-2125), y = (r, phi, v_r, v_phi), records on (r, phi) axes, so that slot 1 is
// d mu / d phi and slot 2 d mu / d r.
template <int GEO>
__device__ __forceinline__ void grad_rhs(const GradTraceArgs& a, const double* g0, const double* g1, GradLane& L, double x,
                                         double z, double vx, double vz, double& k0, double& k1, double& k2, double& k3) {
    ++L.n_rhs;
    double n, dndx, dndz, y0 = 0, y1 = 0;
    // (a spherical state's first component runs along axis 0, a Cartesian state's second)
    const int where = GEO == PRHF_GEO_SPHERICAL ? field_locate(g0, a.n0, g1, a.n1, x, z, L.c0, L.c1, y0, y1)
                                                : field_locate(g0, a.n0, g1, a.n1, z, x, L.c0, L.c1, y0, y1);
    if (where == 0) {
        FieldCorners q;
        field_corners<true, true>(a.rec, L.f, a.n0, a.n1, L.c0, L.c1, q);
        n = field_blend(q.r[0].x, q.r[2].x, q.r[4].x, q.r[6].x, y0, y1);
        dndx = field_blend(q.r[0].y, q.r[2].y, q.r[4].y, q.r[6].y, y0, y1);
        dndz = field_blend(q.r[1].x, q.r[3].x, q.r[5].x, q.r[7].x, y0, y1);
    } else if (where == 1) {
        n = a.fill_n; dndx = dndz = a.fill_grad;
    } else {
        n = dndx = dndz = qnan();
    }
    if (!(fabs(n) < __builtin_inf()) || n <= 0.0) {      // :986-987
        k0 = k1 = k2 = k3 = 0.0;
        return;
    }
    if (GEO == PRHF_GEO_SPHERICAL) {
        // :2106-2114 with r = x, v_r = vx, v_phi = vz, mu_phi = dndx, mu_r = dndz.  The reference's renormalisation
        // (:2117-2122) rebinds its local v_r and v_phi after the four derivatives have been formed from the old ones:
        // it changes nothing in the vector it returns, so there is nothing to do here on any call.
        const double r = x, gv = dndz * vx + (dndx / r) * vz;
        k0 = vx;
        k1 = vz / r;
        k2 = (dndz - gv * vx) / n + (vz * vz) / r;
        k3 = ((dndx / r) - gv * vz) / n - (vx * vz) / r;
        return;
    }
    double dxds = vx, dzds = vz;
    double gv = dndx * vx + dndz * vz;
    double dvx = (dndx - gv * vx) / n;
    double dvz = (dndz - gv * vz) / n;
    ++L.valid;
    if (a.renormalize_every > 0 && L.valid % (unsigned)a.renormalize_every == 0) {      // :996-1004
        const double vmag = hypot(vx, vz);
        if (vmag > 0.0) {
            const double scale = 1.0 / vmag;
            dxds = dxds * scale; dzds = dzds * scale;
            gv = dndx * dxds + dndz * dzds;
            dvx = (dndx - gv * dxds) / n;
            dvz = (dndz - gv * dzds) / n;
        }
    }
    k0 = dxds; k1 = dzds; k2 = dvx; k3 = dvz;
}

// mu' at the point (p0, p1) along (axis 0, axis 1): a chord's midpoint (:1419-1424, :2299-2301)
__device__ __forceinline__ double grad_mup(const GradTraceArgs& a, const double* g0, const double* g1, GradLane& L, double p0, double p1) {
    double y0 = 0, y1 = 0;
    int c0 = L.c0, c1 = L.c1;
    const int where = field_locate(g0, a.n0, g1, a.n1, p0, p1, c0, c1, y0, y1);
    if (where == 1) return a.fill_mup;
    if (where == 2) return qnan();
    FieldCorners q;
    field_corners<false, true>(a.rec, L.f, a.n0, a.n1, c0, c1, q);
    return field_blend(q.r[1].y, q.r[3].y, q.r[5].y, q.r[7].y, y0, y1);
}

// 10 |nextafter(t, inf) - t|, t >= 0 (the smallest step solve_ivp takes)
__device__ __forceinline__ double grad_min_step(double t) {
    const double up = __longlong_as_double(__double_as_longlong(t) + 1);
    return 10.0 * fabs(up - t);
}

// Dormand-Prince 5(4): nodes, weights, error weights and the dense-output matrix of solve_ivp's RK45 (the published
// tableau; Shampine's quartic interpolant)
#define DP_A21 (1. / 5)
#define DP_A31 (3. / 40)
#define DP_A32 (9. / 40)
#define DP_A41 (44. / 45)
#define DP_A42 (-56. / 15)
#define DP_A43 (32. / 9)
#define DP_A51 (19372. / 6561)
#define DP_A52 (-25360. / 2187)
#define DP_A53 (64448. / 6561)
#define DP_A54 (-212. / 729)
#define DP_A61 (9017. / 3168)
#define DP_A62 (-355. / 33)
#define DP_A63 (46732. / 5247)
#define DP_A64 (49. / 176)
#define DP_A65 (-5103. / 18656)
#define DP_B1 (35. / 384)
#define DP_B3 (500. / 1113)
#define DP_B4 (125. / 192)
#define DP_B5 (-2187. / 6784)
#define DP_B6 (11. / 84)
#define DP_E1 (-71. / 57600)
#define DP_E3 (71. / 16695)
#define DP_E4 (-71. / 1920)
#define DP_E5 (17253. / 339200)
#define DP_E6 (-22. / 525)
#define DP_E7 (1. / 40)

// One component of Q = K^T P (rows of P for the stages 1, 3 .. 7; the second stage's row is zero)
__device__ __forceinline__ void dp_dense_row(double k1, double k3, double k4, double k5, double k6, double k7, double (&q)[4]) {
    q[0] = k1;
    q[1] = k1 * (-8048581381. / 2820520608) + k3 * (131558114200. / 32700410799) + k4 * (-1754552775. / 470086768) +
           k5 * (127303824393. / 49829197408) + k6 * (-282668133. / 205662961) + k7 * (40617522. / 29380423);
    q[2] = k1 * (8663915743. / 2820520608) + k3 * (-68118460800. / 10900136933) + k4 * (14199869525. / 1410260304) +
           k5 * (-318862633887. / 49829197408) + k6 * (2019193451. / 616988883) + k7 * (-110615467. / 29380423);
    q[3] = k1 * (-12715105075. / 11282082432) + k3 * (87487479700. / 32700410799) + k4 * (-10690763975. / 1880347072) +
           k5 * (701980252875. / 199316789632) + k6 * (-1453857185. / 822651844) + k7 * (69997945. / 29380423);
}
// y(t) on the step [t_old, t_old + h]
__device__ __forceinline__ double dp_dense(const double (&q)[4], double y_old, double t_old, double h, double t) {
    const double x = (t - t_old) / h, x2 = x * x, x3 = x2 * x, x4 = x3 * x;
    return h * (q[0] * x + q[1] * x2 + q[2] * x3 + q[3] * x4) + y_old;
}

// Event functions (:1009-1031 as trace_ray_cartesian_gradient wires them, :1370-1373): 0 ground (with its 1e-3 km
// offset), 1 top, 2 left, 3 right; all terminal, direction + -> -.  EV & 2: the event looks at x, else at z.  A
// spherical launch carries R_E + z_ground_km, r_max_km, phi_min and phi_max in the same four places, and events 0 and 1
// look at r, 2 and 3 at phi (DESIGN.md section 4.7; the reference's own wiring, :2239-2243, tests phi against radii).
template <int EV>
__device__ __forceinline__ double grad_event(const GradTraceArgs& a, double v) {
    if (EV == 0) return v - a.z_ground - 1e-3;
    if (EV == 1) return a.z_max - v;
    if (EV == 2) return v - a.x_min;
    return a.x_max - v;
}
// The zero of event EV on the step's dense output, to the last place of s: bisection on [t_old, t_new] between a
// value >= 0 and a value <= 0, the end with the smaller |g| returned.
template <int EV>
__device__ __forceinline__ double grad_event_root(const GradTraceArgs& a, const double (&q)[4], double y_old, double t_old,
                                                  double h, double t_new, double g_old, double g_new) {
    if (g_old == 0.0) return t_old;
    if (g_new == 0.0) return t_new;
    double lo = t_old, hi = t_new, glo = g_old, ghi = g_new;
    for (int it = 0; it < 200; ++it) {
        const double mid = lo + 0.5 * (hi - lo);
        if (!(mid > lo && mid < hi)) break;
        const double gm = grad_event<EV>(a, dp_dense(q, y_old, t_old, h, mid));
        if (gm > 0.0) { lo = mid; glo = gm; }
        else if (gm < 0.0) { hi = mid; ghi = gm; }
        else return mid;
    }
    return fabs(glo) <= fabs(ghi) ? lo : hi;
}

#define PRHF_GRAD_MAX_ATTEMPTS (1 << 24)     // steps a lane may attempt before it gives up with status "failure"

// One ray of field `field` from (x0_km, z0_km) at `elev_deg` under the controls of `a`, on the axes g0, g1 staged in LDS:
// the whole of a lane's work in grad_trace_kernel.  Returns the ray's ground_range_km (NaN unless it ends on the
// ground).  FULL: the ray as the tracers return it - the twelve outputs to `out`, the path of ray `r` to a.path_* when
// those are set.  !FULL: the range-only ray of the homing kernels (prhf_gradient_homing.inc) - the same stepper,
// controller, events and dense-output bisection, hence the same steps and the same landing node to the bit, without mu'
// sampling, chord lengths, the apex, path stores and the second pass that replays the steps up to the midpoint; `r` and
// `out` are not used.  Both are this one text: what !FULL leaves out stands behind `if (FULL)`.  `v_land` (optional):
// the last path node's two velocity components of pass 0, the bits path_vx / path_vz get (prhf_gradient_hops.inc).
template <int GEO, bool FULL>
__device__ __forceinline__ double grad_ray(const GradTraceArgs& a, const double* g0, const double* g1, long long r,
                                           long long field, double elev_deg, double x0_km, double z0_km, double* out,
                                           double* v_land = nullptr) {
    constexpr bool SPH = GEO == PRHF_GEO_SPHERICAL;
    GradLane L;
    L.f = field;
    // :1354-1357; :2230-2234: (r, phi, v_r, v_phi) = (R_E + z0, x0 / R_E, sin, cos), not normalised
    const double elev = elev_deg * (3.141592653589793 / 180.0);
    const double vx0 = cos(elev), vz0 = sin(elev), vnorm = hypot(vx0, vz0);
    const double xs = SPH ? a.earth_radius + z0_km : x0_km, zs = SPH ? x0_km / a.earth_radius : z0_km,
                 vxs = SPH ? vz0 : vx0 / vnorm, vzs = SPH ? vx0 : vz0 / vnorm;

    // results of pass 0 (x and z of a spherical node: R_E phi and r - R_E, :2277-2278)
    double path_km = 0.0, delay = 0.0, x_apex = SPH ? a.earth_radius * zs : xs, z_apex = SPH ? xs - a.earth_radius : zs,
           x_last = x_apex;
    double x_mid = SPH ? qnan() : xs, z_mid = SPH ? qnan() : zs;
    if (v_land) { v_land[0] = vxs; v_land[1] = vzs; }
    int n_nodes = 1, status = 3, n_rej = 0;
    unsigned n_rhs = 0;
    bool too_long = false;

    // pass 0: the ray.  pass 1: the same steps again up to node n_nodes / 2 (:1428-1430), which no lane can know
    // before its ray has ended and which is not kept anywhere unless the caller asked for the path.  Spherical
    // (:2309-2313): up to node searchsorted(cumsum(ds), path / 2), the start of the first chord at whose end the lane's
    // own running sum - the one that gave path_km - reaches half of it; no midpoint (NaN) for a path of length 0.
#pragma nounroll
    for (int pass = 0; pass < (FULL ? 2 : 1); ++pass) {
        const int target = (pass == 0 || SPH) ? 0x7fffffff : n_nodes / 2;
        const double half_km = 0.5 * path_km;
        double cum_km = 0.0;
        L.c0 = L.c1 = 0; L.valid = 0; L.n_rhs = 0;
        double t = 0.0, y0 = xs, y1 = zs, y2 = vxs, y3 = vzs;
        double ka0, ka1, ka2, ka3;          // K1: f(t, y), first same as last
        grad_rhs<GEO>(a, g0, g1, L, y0, y1, y2, y3, ka0, ka1, ka2, ka3);
        double h_abs;
        {   // the initial step (Hairer, Norsett & Wanner II.4, as solve_ivp applies it; error order 4)
            const double s0 = a.atol + fabs(y0) * a.rtol, s1 = a.atol + fabs(y1) * a.rtol, s2 = a.atol + fabs(y2) * a.rtol,
                         s3 = a.atol + fabs(y3) * a.rtol;
            const double d0 = sqrt((y0 / s0) * (y0 / s0) + (y1 / s1) * (y1 / s1) + (y2 / s2) * (y2 / s2) + (y3 / s3) * (y3 / s3)) / 2.0;
            const double d1 = sqrt((ka0 / s0) * (ka0 / s0) + (ka1 / s1) * (ka1 / s1) + (ka2 / s2) * (ka2 / s2) + (ka3 / s3) * (ka3 / s3)) / 2.0;
            double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
            h0 = py_min(h0, a.s_max);
            double f0, f1, f2, f3;
            grad_rhs<GEO>(a, g0, g1, L, y0 + h0 * ka0, y1 + h0 * ka1, y2 + h0 * ka2, y3 + h0 * ka3, f0, f1, f2, f3);
            const double e0 = (f0 - ka0) / s0, e1 = (f1 - ka1) / s1, e2 = (f2 - ka2) / s2, e3 = (f3 - ka3) / s3;
            const double d2 = sqrt(e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3) / 2.0 / h0;
            double h1;
            if (d1 <= 1e-15 && d2 <= 1e-15) h1 = py_max(1e-6, h0 * 1e-3);
            else h1 = pow(0.01 / py_max(d1, d2), 0.2);
            h_abs = py_min(py_min(py_min(100 * h0, h1), a.s_max), a.max_step);
        }
        int nodes = 1, attempts = 0;
        bool active = nodes <= target && !(SPH && pass == 1 && !(path_km > 0.0)), new_step = true, rejected = false;
        double min_step = 0.0;
        if (!SPH && !active) { x_mid = y0; z_mid = y1; }          // (target 0: the launch point)
        if (FULL && pass == 0 && a.path_t) {
            if (a.path_stride > 0) {
                const long long o = r * a.path_stride;
                a.path_t[o] = t; a.path_x[o] = y0; a.path_z[o] = y1; a.path_vx[o] = y2; a.path_vz[o] = y3;
            } else too_long = true;
        }
        while (__ballot(active) != 0) {
            if (active) {
                if (new_step) {
                    min_step = grad_min_step(t);
                    if (h_abs > a.max_step) h_abs = a.max_step;
                    else if (h_abs < min_step) h_abs = min_step;
                    new_step = false;
                    rejected = false;
                }
                if (h_abs < min_step || ++attempts > PRHF_GRAD_MAX_ATTEMPTS) {
                    active = false;                       // status "failure": the step fell below 10 ulp of s
                    if (pass == 0) status = 3;
                } else {
                    double t_new = t + h_abs;
                    if (t_new - a.s_max > 0) t_new = a.s_max;
                    const double h = t_new - t;
                    h_abs = fabs(h);
                    double kb0, kb1, kb2, kb3, kc0, kc1, kc2, kc3, kd0, kd1, kd2, kd3, ke0, ke1, ke2, ke3, kf0, kf1, kf2, kf3,
                           kg0, kg1, kg2, kg3;
                    grad_rhs<GEO>(a, g0, g1, L, y0 + (DP_A21 * ka0) * h, y1 + (DP_A21 * ka1) * h, y2 + (DP_A21 * ka2) * h,
                             y3 + (DP_A21 * ka3) * h, kb0, kb1, kb2, kb3);
                    grad_rhs<GEO>(a, g0, g1, L, y0 + (DP_A31 * ka0 + DP_A32 * kb0) * h, y1 + (DP_A31 * ka1 + DP_A32 * kb1) * h,
                             y2 + (DP_A31 * ka2 + DP_A32 * kb2) * h, y3 + (DP_A31 * ka3 + DP_A32 * kb3) * h, kc0, kc1, kc2, kc3);
                    grad_rhs<GEO>(a, g0, g1, L, y0 + (DP_A41 * ka0 + DP_A42 * kb0 + DP_A43 * kc0) * h,
                             y1 + (DP_A41 * ka1 + DP_A42 * kb1 + DP_A43 * kc1) * h,
                             y2 + (DP_A41 * ka2 + DP_A42 * kb2 + DP_A43 * kc2) * h,
                             y3 + (DP_A41 * ka3 + DP_A42 * kb3 + DP_A43 * kc3) * h, kd0, kd1, kd2, kd3);
                    grad_rhs<GEO>(a, g0, g1, L, y0 + (DP_A51 * ka0 + DP_A52 * kb0 + DP_A53 * kc0 + DP_A54 * kd0) * h,
                             y1 + (DP_A51 * ka1 + DP_A52 * kb1 + DP_A53 * kc1 + DP_A54 * kd1) * h,
                             y2 + (DP_A51 * ka2 + DP_A52 * kb2 + DP_A53 * kc2 + DP_A54 * kd2) * h,
                             y3 + (DP_A51 * ka3 + DP_A52 * kb3 + DP_A53 * kc3 + DP_A54 * kd3) * h, ke0, ke1, ke2, ke3);
                    grad_rhs<GEO>(a, g0, g1, L, y0 + (DP_A61 * ka0 + DP_A62 * kb0 + DP_A63 * kc0 + DP_A64 * kd0 + DP_A65 * ke0) * h,
                             y1 + (DP_A61 * ka1 + DP_A62 * kb1 + DP_A63 * kc1 + DP_A64 * kd1 + DP_A65 * ke1) * h,
                             y2 + (DP_A61 * ka2 + DP_A62 * kb2 + DP_A63 * kc2 + DP_A64 * kd2 + DP_A65 * ke2) * h,
                             y3 + (DP_A61 * ka3 + DP_A62 * kb3 + DP_A63 * kc3 + DP_A64 * kd3 + DP_A65 * ke3) * h, kf0, kf1, kf2, kf3);
                    // (the second stage has weight 0 in the solution and in the error: 0 x NaN keeps a NaN stage visible)
                    const double n0 = y0 + h * (DP_B1 * ka0 + 0.0 * kb0 + DP_B3 * kc0 + DP_B4 * kd0 + DP_B5 * ke0 + DP_B6 * kf0);
                    const double n1 = y1 + h * (DP_B1 * ka1 + 0.0 * kb1 + DP_B3 * kc1 + DP_B4 * kd1 + DP_B5 * ke1 + DP_B6 * kf1);
                    const double n2 = y2 + h * (DP_B1 * ka2 + 0.0 * kb2 + DP_B3 * kc2 + DP_B4 * kd2 + DP_B5 * ke2 + DP_B6 * kf2);
                    const double n3 = y3 + h * (DP_B1 * ka3 + 0.0 * kb3 + DP_B3 * kc3 + DP_B4 * kd3 + DP_B5 * ke3 + DP_B6 * kf3);
                    grad_rhs<GEO>(a, g0, g1, L, n0, n1, n2, n3, kg0, kg1, kg2, kg3);
                    const double r0 = (DP_E1 * ka0 + 0.0 * kb0 + DP_E3 * kc0 + DP_E4 * kd0 + DP_E5 * ke0 + DP_E6 * kf0 + DP_E7 * kg0) * h /
                                      (a.atol + np_maximum(fabs(y0), fabs(n0)) * a.rtol);
                    const double r1 = (DP_E1 * ka1 + 0.0 * kb1 + DP_E3 * kc1 + DP_E4 * kd1 + DP_E5 * ke1 + DP_E6 * kf1 + DP_E7 * kg1) * h /
                                      (a.atol + np_maximum(fabs(y1), fabs(n1)) * a.rtol);
                    const double r2 = (DP_E1 * ka2 + 0.0 * kb2 + DP_E3 * kc2 + DP_E4 * kd2 + DP_E5 * ke2 + DP_E6 * kf2 + DP_E7 * kg2) * h /
                                      (a.atol + np_maximum(fabs(y2), fabs(n2)) * a.rtol);
                    const double r3 = (DP_E1 * ka3 + 0.0 * kb3 + DP_E3 * kc3 + DP_E4 * kd3 + DP_E5 * ke3 + DP_E6 * kf3 + DP_E7 * kg3) * h /
                                      (a.atol + np_maximum(fabs(y3), fabs(n3)) * a.rtol);
                    const double err = sqrt(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3) / 2.0;
                    // Spherical only: r = R_E + z resolves 9e-13 km, more than the 10 ulp of s below which a step counts
                    // as failed while s < 1024 km.  A ray that meets the underside of the NaN cap comes to rest one ulp
                    // of r below it: a step that would move r is rejected on the NaN beyond, a shorter one is accepted and
                    // moves nothing but s and phi, 1e-12 km at a time (the reference does just that, to no end).  A step
                    // short of s_max that would be accepted and leaves r where it was although dr/ds is not zero is
                    // below the resolution of the state as well: status "failure", no node (DESIGN.md section 4.7).
                    const bool stalled = SPH && err < 1.0 && n0 == y0 && ka0 != 0.0 && t_new - a.s_max < 0;
                    if (stalled) {
                        active = false;
                        if (pass == 0) status = 3;
                    } else if (err < 1.0) {
                        double factor = err == 0.0 ? 10.0 : py_min(10.0, 0.9 * pow(err, -0.2));
                        if (rejected) factor = py_min(1.0, factor);
                        h_abs *= factor;
                        // the node this step ends on: (t_new, y_new), or the first terminal event on the way
                        double tn = t_new, e0 = n0, e1 = n1, e2 = n2, e3 = n3;
                        int ended = -1;                      // 0 ground, 1 domain, 2 length
                        // the component the ground and top events look at, and the one left and right look at
                        const double yv = SPH ? y0 : y1, nv = SPH ? n0 : n1, yh = SPH ? y1 : y0, nh = SPH ? n1 : n0;
                        const double ga0 = grad_event<0>(a, yv), gb0 = grad_event<0>(a, nv);
                        const double ga1 = grad_event<1>(a, yv), gb1 = grad_event<1>(a, nv);
                        const double ga2 = grad_event<2>(a, yh), gb2 = grad_event<2>(a, nh);
                        const double ga3 = grad_event<3>(a, yh), gb3 = grad_event<3>(a, nh);
                        const bool hit0 = ga0 >= 0 && gb0 <= 0, hit1 = ga1 >= 0 && gb1 <= 0, hit2 = ga2 >= 0 && gb2 <= 0,
                                   hit3 = ga3 >= 0 && gb3 <= 0;
                        if (hit0 || hit1 || hit2 || hit3) {
                            double q0[4], q1[4];
                            dp_dense_row(ka0, kc0, kd0, ke0, kf0, kg0, q0);
                            dp_dense_row(ka1, kc1, kd1, ke1, kf1, kg1, q1);
                            const double(&qz)[4] = SPH ? q0 : q1;
                            const double(&qx)[4] = SPH ? q1 : q0;
                            double root = __builtin_inf();
                            if (hit0) { root = grad_event_root<0>(a, qz, yv, t, h, t_new, ga0, gb0); ended = 0; }
                            if (hit1) {
                                const double s = grad_event_root<1>(a, qz, yv, t, h, t_new, ga1, gb1);
                                if (s < root) { root = s; ended = 1; }
                            }
                            if (hit2) {
                                const double s = grad_event_root<2>(a, qx, yh, t, h, t_new, ga2, gb2);
                                if (s < root) { root = s; ended = 1; }
                            }
                            if (hit3) {
                                const double s = grad_event_root<3>(a, qx, yh, t, h, t_new, ga3, gb3);
                                if (s < root) { root = s; ended = 1; }
                            }
                            double qv[4];
                            tn = root;
                            e0 = dp_dense(q0, y0, t, h, root);
                            e1 = dp_dense(q1, y1, t, h, root);
                            dp_dense_row(ka2, kc2, kd2, ke2, kf2, kg2, qv);
                            e2 = dp_dense(qv, y2, t, h, root);
                            dp_dense_row(ka3, kc3, kd3, ke3, kf3, kg3, qv);
                            e3 = dp_dense(qv, y3, t, h, root);
                        } else if (t_new - a.s_max >= 0) {
                            ended = 2;
                        }
                        // solve_ivp does not append an event node that coincides with the node before it
                        if (!(ended >= 0 && ended < 2 && tn == t && nodes > 1)) {
                            double ds = 0.0;                 // the chord to this node (the spherical replay needs it too)
                            if (FULL && SPH) {               // :2291-2294
                                const double dr = e0 - y0, rdphi = (0.5 * (y0 + e0)) * (e1 - y1);
                                ds = sqrt(dr * dr + rdphi * rdphi);
                            } else if (FULL && pass == 0) {
                                ds = hypot(e0 - y0, e1 - y1);                                 // :1413-1415
                            }
                            if (pass == 0) {
                                // this node's x and z
                                const double ex = SPH ? a.earth_radius * e1 : e0, ez = SPH ? e0 - a.earth_radius : e1;
                                if (FULL && ds == ds) {
                                    path_km += ds;
                                    double mup;
                                    if (SPH) {
                                        // :2299-2301 and build_mup_function's way back to (r, phi) (:2009-2010): the
                                        // midpoints of the x and z paths, not of r and phi
                                        const double xm = 0.5 * (a.earth_radius * y1 + ex), zm = 0.5 * ((y0 - a.earth_radius) + ez);
                                        mup = grad_mup(a, g0, g1, L, a.earth_radius + zm, xm / a.earth_radius);
                                    } else {
                                        mup = grad_mup(a, g0, g1, L, 0.5 * (y1 + e1), 0.5 * (y0 + e0));
                                    }
                                    if (fabs(mup) < __builtin_inf()) delay += (mup / 299792.458) * ds;      // :1418-1425
                                }
                                if (FULL && ez > z_apex) { z_apex = ez; x_apex = ex; }         // np.nanargmax: the first maximum
                                x_last = ex;
                                if (v_land) { v_land[0] = e2; v_land[1] = e3; }
                                if (FULL && a.path_t) {
                                    if (nodes < a.path_stride) {
                                        const long long o = r * a.path_stride + nodes;
                                        a.path_t[o] = tn; a.path_x[o] = e0; a.path_z[o] = e1; a.path_vx[o] = e2; a.path_vz[o] = e3;
                                    } else too_long = true;
                                }
                            } else if (SPH) {
                                if (ds == ds) cum_km += ds;
                                if (cum_km >= half_km) {      // the chord's first node
                                    x_mid = a.earth_radius * y1; z_mid = y0 - a.earth_radius;
                                    active = false;
                                }
                            } else if (nodes == target) {
                                x_mid = e0; z_mid = e1;
                            }
                            ++nodes;
                        }
                        t = t_new; y0 = n0; y1 = n1; y2 = n2; y3 = n3;
                        ka0 = kg0; ka1 = kg1; ka2 = kg2; ka3 = kg3;
                        new_step = true;
                        if (ended >= 0) {
                            active = false;
                            if (pass == 0) status = ended;
                        }
                        if (nodes > target) active = false;
                    } else {
                        h_abs *= py_max(0.2, 0.9 * pow(err, -0.2));
                        rejected = true;
                        if (pass == 0) ++n_rej;
                    }
                }
            }
        }
        if (pass == 0) { n_nodes = nodes; n_rhs = L.n_rhs; }
    }
    if (!FULL) return status == 0 ? x_last : qnan();
    if (too_long) post_status(a.status, (unsigned)PRHF_STATUS_PATHLEN);
    out[0] = path_km;
    out[1] = delay;
    out[2] = x_mid;
    out[3] = z_mid;
    out[4] = status == 0 ? x_last : qnan();          // :1438
    out[5] = x_apex;
    out[6] = z_apex;
    out[7] = (double)status;
    out[8] = (double)n_nodes;
    out[9] = (double)n_rhs;
    out[10] = (double)n_rej;
    out[11] = 0.0;
    return status == 0 ? x_last : qnan();
}

template <int GEO>
__global__ __launch_bounds__(PRHF_GRAD_TRACE_THREADS) void grad_trace_kernel(const GradTraceArgs a) {
    extern __shared__ __attribute__((aligned(16))) double grad_axes[];
    const double* g0 = grad_axes;
    const double* g1 = grad_axes + a.n0;
    for (int i = threadIdx.x; i < a.n0 + a.n1; i += blockDim.x) grad_axes[i] = i < a.n0 ? a.a0[i] : a.a1[i - a.n0];
    __syncthreads();
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_rays) return;
    double* out = a.out + r * PRHF_GRAD_OUTPUTS;
    const long long f = a.ray_field ? a.ray_field[r] : 0;
    if (f < 0 || f >= a.n_fields) {
        post_status(a.status, (unsigned)PRHF_STATUS_BADFIELD);
        for (int k = 0; k < PRHF_GRAD_OUTPUTS; ++k) out[k] = qnan();
        return;
    }
    (void)grad_ray<GEO, true>(a, g0, g1, r, f, a.elev[r], a.x0[r], a.z0[r], out);
}

}  // namespace

hipError_t launch_field_pack(const FieldPackArgs& a, hipStream_t stream) {
    const long long total = (long long)a.n_fields * a.n0 * a.n1;
    if (total <= 0) return hipSuccess;
    long long blocks = (total + PRHF_GRAD_THREADS - 1) / PRHF_GRAD_THREADS;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(field_pack_kernel, dim3((unsigned)blocks), dim3(PRHF_GRAD_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_field_sample(const FieldSampleArgs& a, hipStream_t stream) {
    if (a.n <= 0) return hipSuccess;
    long long blocks = (a.n + PRHF_GRAD_THREADS - 1) / PRHF_GRAD_THREADS;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(field_sample_kernel, dim3((unsigned)blocks), dim3(PRHF_GRAD_THREADS), field_axes_lds_bytes(a.n0, a.n1),
                       stream, a);
    return hipGetLastError();
}

hipError_t launch_grad_trace(const GradTraceArgs& a, hipStream_t stream) {
    if (a.n_rays <= 0) return hipSuccess;
    const long long blocks = (a.n_rays + PRHF_GRAD_TRACE_THREADS - 1) / PRHF_GRAD_TRACE_THREADS;
    if (a.geometry == PRHF_GEO_SPHERICAL)
        hipLaunchKernelGGL(grad_trace_kernel<PRHF_GEO_SPHERICAL>, dim3((unsigned)blocks), dim3(PRHF_GRAD_TRACE_THREADS),
                           field_axes_lds_bytes(a.n0, a.n1), stream, a);
    else
        hipLaunchKernelGGL(grad_trace_kernel<PRHF_GEO_CARTESIAN>, dim3((unsigned)blocks), dim3(PRHF_GRAD_TRACE_THREADS),
                           field_axes_lds_bytes(a.n0, a.n1), stream, a);
    return hipGetLastError();
}
