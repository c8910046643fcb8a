// prhf_snell.inc - stratified Snell's-law ray tracers (flat and spherical Earth), one wavefront
// per ray.  Included by prhf_kernels.hip inside namespace prhf (it reuses the Appleton-Hartree
// device functions and wave primitives defined there).
//
// Replaces: trace_ray_cartesian_snells (reference PyRayHF/library.py:1096-1268) with
// tan_from_mu_scalar (:1034-1062) and find_turning_point (:1065-1093), and
// trace_ray_spherical_snells (:1460-1713).  Line numbers below are that file.
//
// Two launches.  PER RAY (snell_kernel<GEOM, PTAB, REDUCED>, snell_ray): every ray has its own frequency, elevation and
// profile.  Phase and group index level by level from the ground up, 64 levels at a time, stream-compacting the levels
// with a finite mu and looking (by ballot) for the first bracket where mu (flat) or mu r (spherical, Bouguer) falls
// through the invariant p - the levels above that bracket cannot change any output, so they are never evaluated (the
// reference evaluates them all) - with the up-leg x(z) / phi(z) by a wave prefix sum, the path length, the group delay
// and the midpoint while a chunk is in registers; the mirrored half of the path by symmetry.  Persistent wavefronts
// draw the rays from eight queues (snell_dispatch).  GROUPED (snell_fan_kernel<GEOM>, snell_ray_table): rays that
// share (profile, frequency) read tables made once per group (snell_tables_kernel) - mu, mu' of every level and the
// compacted list of the finite levels with the running minimum of the bracket criterion, which turns the bracket
// search into two loads.
//
// mu and mu' of the levels are the reference's operations in the reference's order (index_faithful_sc) - in the
// per-ray launch's default arithmetic only where that can move a result (REDUCED, in front of snell_ray); what does
// not decide an answer - tan(theta) = p / sqrt(...), the spherical sub-steps' integrand, hypot - is evaluated to
// ~1.5 ulp without IEEE square roots and divisions (hypot_km, dphi_integrand).  The frequency-independent parts of a
// level (f_N^2, g_p |B|, sin / cos of the field angle) come from a per-profile table when the rays outnumber the
// profiles (SnellArgs::ptab, snell_profile_kernel).

namespace {

// Inclusive running sum over the lanes: DPP row shifts inside the rows of 16, row_bcast:15 / :31 across them (the pattern
// of wave_scan_max; a lane without a source adds 0).  Six dependent steps of three vector instructions - the shuffle
// version's six steps were two ds_bpermute round trips each.
#define PRHF_DPP_ADD(v, ctrl, rows) do {                                                                            \
        const int lo_ = __builtin_amdgcn_update_dpp(0, __double2loint(v), ctrl, rows, 0xf, (rows) == 0xf);          \
        const int hi_ = __builtin_amdgcn_update_dpp(0, __double2hiint(v), ctrl, rows, 0xf, (rows) == 0xf);          \
        v = v + __hiloint2double(hi_, lo_);                                                                         \
    } while (0)
__device__ __forceinline__ double wave_inclusive_scan(double v, int lane) {
    (void)lane;
    PRHF_DPP_ADD(v, 0x111, 0xf);    // row_shr:1
    PRHF_DPP_ADD(v, 0x112, 0xf);    // row_shr:2
    PRHF_DPP_ADD(v, 0x114, 0xf);    // row_shr:4
    PRHF_DPP_ADD(v, 0x118, 0xf);    // row_shr:8
    PRHF_DPP_ADD(v, 0x142, 0xa);    // row_bcast:15 into rows 1 and 3
    PRHF_DPP_ADD(v, 0x143, 0xc);    // row_bcast:31 into rows 2 and 3
    return v;
}

__device__ __forceinline__ bool finite64(double v) { return (v - v) == 0.0; }

// sqrt(a^2 + b^2) of kilometre-sized operands to ~1.5 ulp (np.hypot, :1240 / :1683, rounds to ~1): no scaling against
// overflow or underflow - path increments are 1e-9 .. 1e4 km - one v_rsq_f64 and its third-order step instead of the
// device library's hypot (~45 instructions).  0 for (0, 0), NaN for a NaN operand.
__device__ __forceinline__ double hypot_km(double a, double b) {
    const double s = __builtin_fma(a, a, b * b);
    const double r = s * rsqrt_cubic(s);
    return s > 0.0 ? r : s;
}
// The integrand of the spherical up-leg, p / (r sqrt(den)) (:1629-1632), as p rsqrt(r^2 den): the same smooth function
// of the same operands (den = max((mu r)^2 - p^2, 1e-16) is formed exactly as the reference forms it) to ~1.5 ulp,
// without the IEEE square root and division (~45 instructions of the ~110 a sub-step took).
__device__ __forceinline__ double dphi_integrand(double p, double r_m, double den) {
    return p * rsqrt_cubic((r_m * r_m) * den);
}
// t0 = j / N and t1 = (j + 1) / N of the sub-steps (:1656-1657) are IEEE quotients; 0 / N = 0 and N / N = 1 exactly, so
// the two ends need no division (an interval of ONE sub-step - most of them - needs none).  In between, the quotient of
// two small integers from the correctly rounded reciprocal rN = 1 / N and one correction (Markstein): q0 = j rN is
// within an ulp of j / N, r = j - q0 N is exact in an fma, and fl(q0 + r rN) is the correctly rounded quotient - checked
// against the division for every 0 <= j <= N <= 8192 (tests/test_host_substep_quotient.py); three instructions instead
// of the ~14 and the v_rcp_f64 of a division, twice per sub-step where an interval is shared out.  Beyond 8192 sub-steps
// (max_substeps is the caller's; the reference's default is 400): the division.
constexpr int kQuotientProven = 8192;
#ifndef PRHF_SNELL_SHARED
#define PRHF_SNELL_SHARED 16
#endif
constexpr int kShared = PRHF_SNELL_SHARED;      // sub-steps from which an interval is shared out over the wavefront
__device__ __forceinline__ double substep_node(int j, int n_sub, double dN, double rN) {
    const double a = (double)j;
    if (n_sub > kQuotientProven) return j == 0 ? 0.0 : (j == n_sub ? 1.0 : a / dN);
    const double q0 = a * rN;                                       // (0 / N = 0 and N / N = 1 come out of it exactly too)
    return __builtin_fma(__builtin_fma(-q0, dN, a), rN, q0);
}

// v of lane l (l wave-uniform) as a wave-uniform value: two v_readlane_b32, the result lives in scalar registers
__device__ __forceinline__ double lane_value(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// The spherical up-leg behind an interval without height.  The reference's loop leaves such an interval with
// `if dz <= 0: continue` (:1641-1642) and so never reaches phi_up[k + 1] = phi_up[k] + dphi_sum (:1669): that node keeps
// the 0 it was made with and the running angle starts again from there (a column with a repeated altitude; fixture
// G29).  `incl`: the chunk's running sum of `du` with the carry in it; `restart`: this lane's interval is such a one
// (its du is 0).  Every lane from the last such lane below it on gets the sum of what lies behind that lane alone.  One
// ballot where there is none - every column but a degenerate one.  Every lane calls this.
__device__ __forceinline__ double restart_behind_empty_intervals(double incl, double du, bool restart, int lane) {
    unsigned long long m = __ballot(restart);
    while (m) {
        const int r = __ffsll((long long)m) - 1;
        m &= m - 1;
        const double behind = wave_inclusive_scan(lane > r ? du : 0.0, lane);
        if (lane >= r) incl = behind;
    }
    return incl;
}

// np.interp(x, xp, fp) for one abscissa on a grid that may carry NaN ordinates (numpy arr_interp).
__device__ __forceinline__ double interp_nan_aware(double x, int j, int n, double xj, double xj1, double fj,
                                                   double fj1) {
#pragma clang fp contract(off)
    if (j >= n - 1) return fj;                       // last node (or beyond: right value)
    if (xj == x) return fj;
    const double slope = (fj1 - fj) / (xj1 - xj);
    double r = slope * (x - xj) + fj;
    if (r != r) {
        r = slope * (x - xj1) + fj1;
        if (r != r && fj == fj1) r = fj;
    }
    return r;
}

// mu and mu' of profile level s at frequency f0 (:1184-1189 without the blanking): from the columns, or - a.ptab given -
// from the per-profile table of the frequency-independent parts (snell_profile_kernel); the same operations either way
template <int MODE, bool PTAB>
__device__ __forceinline__ void snell_level_index(const SnellArgs& a, long long pi, int s, const double* den,
                                                  const double* bmag, const double* bpsi, double f0, double f2,
                                                  int unmag, double* mu_out, double* mup_out) {
#pragma clang fp contract(off)
    if (PTAB) {
        typedef double vec2 __attribute__((ext_vector_type(2)));
        const vec2* e = reinterpret_cast<const vec2*>(a.ptab + 4 * (pi * a.n_alt + s));
        const vec2 e0 = e[0], e1 = e[1];
        const double X = e0.x / f2;
        const double Y = e0.y / f0;
        if (unmag) index_unmagnetised(X, mu_out, mup_out);
        else index_faithful_sc<MODE>(X, Y, e1.x, e1.y, mu_out, mup_out);
        return;
    }
    const double fn = sqrt(den[s]) * kPlasma;
    const double X = (fn * fn) / f2;
    const double Y = (kGyro * bmag[s]) / f0;
    if (unmag) index_unmagnetised(X, mu_out, mup_out);
    else index_faithful<MODE>(X, Y, bpsi[s], mu_out, mup_out);
}

}  // namespace

// The ray of a GROUPED launch (a.ray_group).  What does not depend on the ray is made once per (profile, frequency)
// group, before the rays run (snell_tables_kernel): mu and mu' of every level (the reference's operations in its
// order, :1184-1189) and the list of the levels with a finite mu (:1204-1205), compacted, each
// entry carrying its altitude, mu, mu' and the running minimum of the bracket criterion (mu flat, mu r spherical) over
// the entries 1 .. i.  The reference's turning-point search (:1085-1093 / :1598-1603) returns the FIRST pair of
// consecutive finite levels with crit[i] >= p >= crit[i + 1]; crit[0] >= p always (p = crit[0] sin(theta0)), so that
// pair is (j - 1, j) with j the first entry >= 1 whose criterion is <= p - the first entry whose running minimum is
// <= p, and a running minimum is monotone: the search is two dependent loads (64 samples of it, then the 64 entries
// between two samples) instead of a walk over all levels below the turning point with a compaction, an LDS round trip
// and a gather per chunk of 64 (rounds 3 - 5, 57 % VALU-busy: latency-bound).  The pair found is checked against the
// reference's own condition and a plain walk takes over if it fails (a criterion that is NaN at entry j - 1, an Earth
// radius that makes crit[0] negative).  Then the up-leg, the path length, the group delay and the midpoint over
// contiguous entries: lane l of a chunk loads the upper node of its interval and takes the lower one from lane l - 1.
// Same operations on the same values as the per-ray launch's reference-order tier: the two agree to 1e-15
// (tests/test_gpu_tracers.py).
struct GroupEntry { double z, mu, mup, run_min; };                  // 32 bytes: two b128 loads

template <int GEOM>
__device__ __forceinline__ void snell_ray_table(const SnellArgs& a, long long ray, double* lds) {
#pragma clang fp contract(off)
    typedef double vec2 __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x & 63;
    const int n_alt = (int)a.n_alt;
    long long grp = a.ray_group[ray];
    const bool bad_group = grp < 0 || grp >= a.n_groups;
    if (bad_group) grp = 0;
    // per group (snell_tables_kernel): entries, "a ground level was inserted", error bits, profile
    const int4 info = *reinterpret_cast<const int4*>(a.group_info + 4 * grp);
    const int nv = info.x, ground = info.y & 1, group_bad = info.z;
    const long long pi = info.w;
    const double* alt = a.alt + pi * a.alt_stride;
    const int n = n_alt + ground;
    const vec2* entries = reinterpret_cast<const vec2*>(a.group_entries + grp * (4 * (a.n_alt + 1)));
    const int* kidx = a.group_kidx + grp * (a.n_alt + 1);           // grid level of each entry
    const double* lev = a.levels + grp * (a.n_alt + 1);             // mu' of every grid level, blanked ones included (the apex needs it)
    double* u_up = lds;                  // up-leg horizontal coordinate (x or phi), n_alt + 2 entries
    double* out = a.out + ray * PRHF_SNELL_OUTPUTS;
    const double RE = a.earth_radius_km;
    const double nan = qnan();
    const double inf = __builtin_inf();

    auto fail = [&]() {
        if (lane < PRHF_SNELL_OUTPUTS) out[lane] = (lane == 7) ? 0.0 : nan;
        if (a.path_x)
            for (long long k = lane; k < a.path_stride; k += 64) {
                a.path_x[ray * a.path_stride + k] = nan;
                a.path_z[ray * a.path_stride + k] = nan;
            }
    };
    auto level_alt = [&](int k) { return (ground && k == 0) ? 0.0 : alt[k - ground]; };
    if (bad_group || (group_bad & 1)) {
        if (lane == 0) post_status(a.status, (unsigned)(bad_group ? PRHF_STATUS_BADGROUP : PRHF_STATUS_BADINDEX));
        fail();
        return;
    }
    if (group_bad & 2) {                                            // a negative density in the column (:93-94 raises)
        if (lane == 0) post_status(a.status, (unsigned)PRHF_STATUS_NEGDEN);
        fail();
        return;
    }
    const double theta0 = (90.0 - a.elev_deg[ray]) * kDegToRad;     // :1192 / :1573
    const double s0 = sin(theta0);
    // (nv = 0: level 0 has no finite mu; one entry: the reference's "fewer than 2 levels" exit)
    if (nv < 2 || (GEOM == 0 && !finite64(s0))) { fail(); return; }
    auto crit_of = [&](double z, double mu) { return (GEOM == 0) ? mu : mu * (RE + z); };                 // :1598
    const vec2 e0 = entries[0];                                     // entry 0 is grid level 0
    const double z_first = e0.x, mu_first = e0.y;
    const double p = (GEOM == 0) ? mu_first * s0 : (mu_first * (RE + z_first)) * s0;        // :1201 / :1584

    // ---- the bracket (:1085-1093 / :1598-1603): first entry j >= 1 with run_min[j] <= p ----------------------------
    int it = -1;
    {
        const int seg = (nv + 63) >> 6;                             // entries per sample (<= 47 at 3000 levels)
        const int j1 = min((lane + 1) * seg - 1, nv - 1);
        const double m1 = entries[2 * j1 + 1].y;
        const unsigned long long h1 = __ballot(m1 <= p);
        if (h1 == 0ull) { fail(); return; }                         // mu (mu r) stays above p: the ray escapes
        const int first = (__ffsll((long long)h1) - 1) * seg;
        const int j2 = first + lane;
        const double m2 = (lane < seg && j2 < nv) ? entries[2 * j2 + 1].y : inf;
        const unsigned long long h2 = __ballot(m2 <= p);
        it = first + __ffsll((long long)h2) - 2;                    // (h2 != 0: the sample that ends this stretch is in it)
        if (it < 0) { fail(); return; }                             // (entry 0 itself: only with an infinite invariant)
    }
    double za, zb, ca, cb;
    auto load_bracket = [&]() {
        const vec2 e = entries[2 * (it + (lane & 1))];
        za = lane_value(e.x, 0); zb = lane_value(e.x, 1);
        ca = crit_of(za, lane_value(e.y, 0)); cb = crit_of(zb, lane_value(e.y, 1));
    };
    load_bracket();
    if (!(ca >= p && cb <= p)) {                                    // the reference's own walk
        it = -1;
        for (int sb = 0; sb < nv - 1 && it < 0; sb += 64) {
            const int i = sb + lane;
            bool hit = false;
            if (i < nv - 1) {
                const vec2 lo = entries[2 * i], hi = entries[2 * i + 2];
                hit = (crit_of(lo.x, lo.y) >= p) && (crit_of(hi.x, hi.y) <= p);
            }
            const unsigned long long found = __ballot(hit);
            if (found) it = sb + __ffsll((long long)found) - 1;
        }
        if (it < 0) { fail(); return; }
        load_bracket();
    }
    double z_turn;
    int n_grid;                                                     // up-leg nodes taken from the grid
    if (GEOM == 0) {
        z_turn = za;                                                // :1089-1092
        if (ca != cb) z_turn = za + ((ca - p) / (ca - cb)) * (zb - za);
        n_grid = (z_turn == za) ? it : it + 1;                      // np.searchsorted(zv, z_turn), :1219
    } else {
        double t = (ca != cb) ? (ca - p) / (ca - cb) : 0.0;         // :1617-1619
        t = fmin(fmax(t, 0.0), 1.0);
        z_turn = za + t * (zb - za);
        n_grid = it + 1;                                            // zv[:i0 + 1], :1622
    }
    const int n_up = n_grid + 1;
    const double mu_apex = (GEOM == 0) ? p : p / (RE + z_turn);     // :1221 / :1624

    // ---- mu' at the apex: np.interp on the full grid, NaN-aware (:1244 / :1686) --------------------------
    // number of grid levels at or below z_turn: all those up to the bracket's lower level, plus the
    // (blanked) ones between the bracket's two levels that z_turn has passed
    const int k_pair = kidx[it + (lane & 1)];
    const int k_lo = __builtin_amdgcn_readlane(k_pair, 0), k_hi = __builtin_amdgcn_readlane(k_pair, 1);
    int below = 0;
    for (int k = k_lo + 1 + lane; k <= k_hi; k += 64) below += (level_alt(k) <= z_turn) ? 1 : 0;
    below = k_lo + 1 + (int)(wave_sum((double)below) + 0.5);
    const int j = below - 1;
    double mup_j = nan;                                             // mu' on grid levels j and j + 1 (lanes 0 and 1)
    {
        const int kk = (j < 0 ? 0 : j) + (lane & 1);
        if (kk < n) mup_j = lev[kk];
    }
    const double mup_lo = lane_value(mup_j, 0), mup_hi = lane_value(mup_j, 1);
    double mup_apex;
    if (j < 0) mup_apex = mup_lo;
    else mup_apex = interp_nan_aware(z_turn, j, n, level_alt(j), (j + 1 < n) ? level_alt(j + 1) : 0.0, mup_lo,
                                     (j + 1 < n) ? mup_hi : 0.0);

    // ---- up-leg: x(z) = cumsum(dz tan(theta_mid)) (:1224-1230) or phi(z) with adaptive sub-steps (:1634-1669), and
    // beside it the intervals' lengths and their shares of the group delay (:1240-1246 / :1680-1689).  Lane l of a chunk:
    // the interval between nodes base + l and base + l + 1; node n_grid is the apex
    double carry = 0.0;
    double path = 0.0, delay = 0.0;      // this lane's share of the up-leg's length and group delay
    double z_carry = z_first, mu_carry = mu_first, mup_carry = entries[1].x;     // node 0
    double u_before = 0.0, u_turn = 0.0; // u of node n_up - 2 - the midpoint, almost always - and of the apex
    if (lane == 0) u_up[0] = 0.0;
    auto upper_node = [&](int s, double* z, double* mu, double* mup) {      // node s + 1 of interval s
        *z = z_turn; *mu = mu_apex; *mup = mup_apex;
        if (s + 1 < n_grid) {
            const vec2 q0 = entries[2 * (s + 1)];
            *z = q0.x; *mu = q0.y;
            *mup = entries[2 * (s + 1) + 1].x;
        }
    };
    // flat Earth: the next chunk's upper nodes are requested before this chunk is worked on (a chunk is ~60 instructions,
    // a load's latency several times that); spherical: a chunk is sub-steps by the hundred, and the six registers would
    // be the ones that take the kernel from seven waves per SIMD to six
    constexpr bool kAhead = GEOM == 0;
    double z1n = 0.0, mu1n = 0.0, mup1n = 0.0;
    if (kAhead) upper_node(lane, &z1n, &mu1n, &mup1n);
    for (int base = 0; base < n_up - 1; base += 64) {
        const int s = base + lane;
        double z1 = z1n, mu1 = mu1n, mup1 = mup1n;
        if (kAhead) {
            if (base + 64 < n_up - 1) upper_node(s + 64, &z1n, &mu1n, &mup1n);
        } else {
            upper_node(s, &z1, &mu1, &mup1);
        }
        const double z0 = wave_shift_up_1(z1, z_carry), mu0 = wave_shift_up_1(mu1, mu_carry);
        const double mup0 = wave_shift_up_1(mup1, mup_carry);
        double du = 0.0;
        bool empty = false;                                         // spherical: an interval with dz <= 0 (:1641)
        if (GEOM == 0 && s < n_up - 1) {
            const double dz = z1 - z0;
            double mm = 0.5 * (mu0 + mu1);
            if (s == n_up - 2) mm = fmax(mm, p + 1e-8);            // :1228
            double arg = mm * mm - p * p;                           // :1057-1061
            if (arg < 1e-10) arg = 1e-10;
            du = dz * (p * rsqrt_cubic(arg));                      // tan(theta) = p / sqrt(arg), :1061, to ~1 ulp
        }
        if (GEOM == 1) {
            // adaptive midpoint sub-steps of one interval (:1634-1669).  The number of sub-steps is very
            // uneven - up to max_substeps (400) in the intervals next to the apex, a handful elsewhere - so
            // an interval with many of them is shared out over the 64 lanes instead of keeping one lane busy
            // (the partial sums are added in another order than the reference's loop: 1e-16 relative).
            double dz = 0.0;
            int N = 0;
            if (s < n_up - 1) {
                dz = z1 - z0;
                empty = dz <= 0.0;
                if (dz > 0.0) {
                    const double gap_a = fmax(mu0 * (RE + z0) - p, 1e-12);
                    const double gap_b = fmax(mu1 * (RE + (z0 + dz)) - p, 1e-12);
                    const double sharp = 1.0 / fmin(gap_a, gap_b);
                    double nd = fmax(1.0, ceil(fabs(dz) / a.dz_target_km));                       // :1645
                    nd = fmin((double)a.max_substeps, nd * (1.0 + a.apex_boost * sharp));         // :1651
                    N = (int)nd;                                                                  // int() truncates
                }
            }
            auto substeps = [&](double z0_, double dz_, double ma, double mb, int n_sub, int first, int stride) {
                const double dN = (double)n_sub;
                const double rN = 1.0 / dN;
                const double h = dz_ / dN;
                double sum = 0.0;
                double t0 = substep_node(first, n_sub, dN, rN);
                for (int jj = first; jj < n_sub; jj += stride) {
                    const double t1 = substep_node(jj + 1, n_sub, dN, rN);
                    const double half = 0.5 * (t0 + t1);
                    const double r_m = RE + (z0_ + half * dz_);
                    double mr = (ma + (mb - ma) * half) * r_m;
                    if (mr <= p) mr = p + 1e-8;                                                   // :1664-1665
                    const double den_ = fmax(mr * mr - p * p, 1e-16);                             // :1631
                    sum = sum + dphi_integrand(p, r_m, den_) * h;
                    t0 = (stride == 1) ? t1 : substep_node(jj + stride, n_sub, dN, rN);               // the next sub-step's left node
                }
                return sum;
            };
            unsigned long long heavy = __ballot(N >= kShared);
            while (heavy) {
                const int owner = __ffsll((long long)heavy) - 1;
                heavy &= heavy - 1;
                const double part = substeps(lane_value(z0, owner), lane_value(dz, owner), lane_value(mu0, owner),
                                             lane_value(mu1, owner), __builtin_amdgcn_readlane(N, owner), lane, 64);
                const double total = wave_sum(part);
                if (lane == owner) du = total;
            }
            if (N > 0 && N < kShared) du = substeps(z0, dz, mu0, mu1, N, 0, 1);
        }
        double incl = wave_inclusive_scan(du, lane) + carry;
        if (GEOM == 1) incl = restart_behind_empty_intervals(incl, du, empty, lane);
        const double u_lo = wave_shift_up_1(incl, carry);           // the node below is the lane below's (lane 0: the carry)
        if (s < n_up - 1) {
            u_up[s + 1] = incl;
            const double dzs = z1 - z0, dus = incl - u_lo;
            const double ds = (GEOM == 0) ? hypot_km(dus, dzs) : hypot_km((RE + 0.5 * (z0 + z1)) * dus, dzs);
            const double mseg = 0.5 * (mup0 + mup1);
            const double tt = (mseg / kLightKmS) * ds;
            if (ds == ds) path += ds;
            if (tt == tt) delay += tt;
        }
        const int last = n_up - 2 - base;                           // lane of the last interval, if it is in this chunk
        if (last >= 0 && last < 64) {
            u_before = lane_value(u_lo, last);
            u_turn = lane_value(incl, last);
        }
        carry = lane_value(incl, 63);
        z_carry = lane_value(z1, 63); mu_carry = lane_value(mu1, 63); mup_carry = lane_value(mup1, 63);
    }
    __syncthreads();                     // (one wavefront: u_up, for the path arrays and a midpoint below node n_up - 2)
    auto z_node = [&](int s) { return s < n_grid ? entries[2 * s].x : z_turn; };
    auto u_path = [&](int k) { return (k < n_up) ? u_up[k] : 2.0 * u_turn - u_up[2 * n_up - 2 - k]; };
    auto z_path = [&](int k) { return (k < n_up) ? z_node(k) : z_node(2 * n_up - 2 - k); };
    // ---- path length and group delay (:1239-1246 / :1685-1689).  The path is the up-leg mirrored about the apex
    // (:1232-1237 / :1671-1676): its segment n_seg - 1 - k has the length and the mu' ends of segment k, so the sums
    // over the mirrored path are twice the up-leg's (1e-16 relative apart from the reference's, which adds the mirrored
    // coordinates' differences) - added up beside the up-leg itself.
    path = 2.0 * wave_sum(path);
    delay = 2.0 * wave_sum(delay);
    // midpoint (:1248-1252 / :1691-1695): x_full[searchsorted(cumsum(ds), path / 2)] - see the note on snell_ray below
    double x_mid = nan, z_mid = nan;
    if (path > 0.0) {
        int km = n_up - 2;
        double u_km = u_before, z_km = (km < n_grid) ? ((km == it) ? za : ((km == it + 1) ? zb : z_node(km))) : z_turn;
        if (u_turn == u_km && z_turn == z_km) {                     // (segments without a length before the apex: rare)
            while (km > 0 && u_up[km + 1] == u_up[km] && z_node(km + 1) == z_node(km)) --km;
            u_km = u_up[km];
            z_km = z_node(km);
        }
        x_mid = (GEOM == 0) ? u_km : RE * u_km;                     // x = R_E phi, :1678
        z_mid = z_km;
    }
    const double x_end = (GEOM == 0) ? 2.0 * u_turn : RE * (2.0 * u_turn);       // the mirror image of node 0 (u = 0)
    const double landed = (fabs(z_first) <= 1e-3) ? x_end : nan;                    // :1256-1258 / :1699-1701

    if (lane == 0) {
        out[0] = path; out[1] = delay; out[2] = x_mid; out[3] = z_mid; out[4] = landed;
        out[5] = (GEOM == 0) ? u_turn : RE * u_turn; out[6] = z_turn; out[7] = (double)(2 * n_up - 1);
    }
    if (a.path_x) {
        const int n_path = 2 * n_up - 1;
        for (long long k = lane; k < a.path_stride; k += 64) {
            double xv = nan, zz = nan;
            if (k < n_path) {
                xv = (GEOM == 0) ? u_path((int)k) : RE * u_path((int)k);
                zz = z_path((int)k);
            }
            a.path_x[ray * a.path_stride + k] = xv;
            a.path_z[ray * a.path_stride + k] = zz;
        }
    }
}

// The ray of a PER-RAY launch: its own frequency, elevation and profile.
// GEOM 0: flat Earth, horizontal coordinate x [km]; GEOM 1: spherical Earth, central angle phi [rad].
//
// One pass over the levels (round 4).  Rounds 1 - 3 compacted mu and mu' of the finite levels into an array - in LDS,
// then (round 3) in a slab of global memory per resident wavefront, 929 MB of writes per 200 000 rays - and came
// back to them for the up-leg, the path length, the group delay and the midpoint search: three more loops over the
// path.  Now everything that needs mu or mu' is computed while a chunk of 64 levels is in registers: the chunk's
// finite levels are compacted into a 64-entry staging area in LDS (grouped launch: they are read from the group's
// table instead), lane j owns the interval between compacted levels nv - 1 + j and nv + j - the bracket test
// (:1085-1093 / :1598-1603), the up-leg increment (:1224-1230 / :1634-1669), the interval's length and its share of
// the group delay (:1240-1246 / :1680-1689) - and the last two compacted levels travel to the next chunk in
// registers.  The path is mirrored about the apex (:1232-1237 / :1671-1676): its length and delay are twice the
// up-leg's (the reference forms these from the mirrored coordinates: 1e-16 relative apart).  What stays in LDS
// is the up-leg coordinate (8 bytes per level) and the 16-bit level index, for the path arrays.
//
// The midpoint (:1248-1252 / :1691-1695) is x_full[k], z_full[k] with k = searchsorted(cumsum(ds), path / 2): the first
// segment whose running length reaches half the path.  On a path that is its own mirror image the running length
// behind the last up-leg segment IS half the path, so in exact arithmetic k is that segment, n_up - 2, and the node
// returned is its first one: the node BEFORE the apex (or an earlier one when the segments in between have no length).
// That is what both kernels return.  The reference compares a sequential running sum with half a pairwise total, two
// roundings of the same number: its own answer is that node for two rays in three and the apex for the third
// (fixture G8: 84 / 43 of 127), decided by the last bits of every segment length - re-running its very search on node
// coordinates that are 2e-16 apart reproduces 72 % of its choices, the exact-arithmetic rule 66 %
// (tests/test_gpu_tracers.py counts them).  Rounds 3 - 4 returned the apex; the turning point itself is out[5], out[6].
// REDUCED (the per-ray launch's default arithmetic, SnellArgs::reduced): mu and mu' of a level in the reduced algebra
// (index_fast_core: ~45 vector instructions, two v_rsq_f64) wherever that cannot move an output, the reference's
// operation order (index_faithful_sc: ~310 with its IEEE divisions and square roots, exactly rounded YT^3, YT^4)
// elsewhere - decided per level and ray, after the cheap evaluation:
//   * mu^2 <= kReducedMinMu2 or mu' <= 1/2 or anything not finite: towards reflection mu^2 = 1 - q cancels and the two
//     formulations drift apart (above 0.1 they agree to 7e-16 absolute in mu^2, both as far from the exact value);
//   * mu^2 - p^2 <= kReducedApex mu^2 ((mu r)^2 on a spherical Earth): next to the turning point the up-leg's
//     tan(theta) = p / sqrt(mu^2 - p^2) amplifies a change of mu^2 by mu^2 / (mu^2 - p^2) <= 1000 here, so what the
//     reduced levels can move is 7e-16 x 1000 / 2 = 4e-13 of an interval's horizontal step (X mode, whose rsqrt takes one
//     Newton step: 4e-12), and the bracket that decides the turning point always lies among the re-evaluated levels.
// A chunk of 64 levels none of which needs the reference order costs a seventh of what it cost; a ray pays the full
// price for its last chunk only, and a ray that escapes - all 620 levels, a third of the rays of a random fan and half
// of its time - for none.  Measured against the reference-order tier: tests/test_gpu_tracers.py.
constexpr double kReducedMinMu2 = 0.1;
constexpr double kReducedApex = 1e-3;

template <int MODE, int GEOM, bool PTAB, bool REDUCED>
__device__ __forceinline__ void snell_ray(const SnellArgs& a, long long ray, double* lds) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int n_alt = (int)a.n_alt;
    const long long pi_given = a.prof_idx ? a.prof_idx[ray] : 0;
    const bool bad_index = pi_given < 0 || pi_given >= a.n_prof;    // device-resident index arrays cannot be checked by the host
    const long long pi = bad_index ? 0 : pi_given;
    const double* den = a.den + pi * a.prof_stride;
    const double* bmag = a.bmag + pi * a.prof_stride;
    const double* bpsi = a.bpsi + pi * a.prof_stride;
    const double* alt = a.alt + pi * a.alt_stride;
    const int ground = (alt[0] > 0.0) ? 1 : 0;                       // :1175-1182 / :1556-1563 ground level
    const int n = n_alt + ground;
    // LDS per ray (one wavefront): the up-leg coordinate and the 16-bit grid index of each compacted level (10 bytes
    // per level), mu and mu' of the chunk in flight (64 compacted levels at most)
    double* u_up = lds;                  // up-leg horizontal coordinate (x or phi), n_alt + 2 entries
    double* stg_mu = u_up + (n_alt + 2);
    double* stg_mup = stg_mu + 64;
    double* stg_z = stg_mup + 64;
    unsigned short* kidx = reinterpret_cast<unsigned short*>(stg_z + 64);       // grid level of each compacted level
    double* out = a.out + ray * PRHF_SNELL_OUTPUTS;
    const double f0 = a.freq_hz[ray];
    const double f2 = f0 * f0;
    const double RE = a.earth_radius_km;
    const double nan = qnan();

    auto fail = [&]() {
        if (lane < PRHF_SNELL_OUTPUTS) out[lane] = (lane == 7) ? 0.0 : nan;
        if (a.path_x)
            for (long long k = lane; k < a.path_stride; k += 64) {
                a.path_x[ray * a.path_stride + k] = nan;
                a.path_z[ray * a.path_stride + k] = nan;
            }
    };
    auto level_alt = [&](int k) { return (ground && k == 0) ? 0.0 : alt[k - ground]; };
    auto zv = [&](int i) { return level_alt((int)kidx[i]); };       // altitude of compacted level i
    if (bad_index) {
        if (lane == 0) post_status(a.status, (unsigned)PRHF_STATUS_BADINDEX);
        fail();
        return;
    }

    // ---- levels: isotropic test over the whole column (:201), then mu and mu' (:1184-1189) -------
    // per profile, not per ray (snell_profile_kernel): the isotropic test looks at the whole column (:201),
    // and a negative density anywhere in it is an error (:93-94 raises in the reference)
    const double bmax = a.prof_info[4 * pi];
    if (a.prof_info[4 * pi + 1] != 0.0) {
        if (lane == 0) post_status(a.status, (unsigned)PRHF_STATUS_NEGDEN);
        fail();
        return;
    }
    const int unmag = ((kGyro * bmax) / f0 < kUnmagTol) ? 1 : 0;
    // mu and mu' of grid level k (:1184-1189); NaN where the reference blanks them
    auto level_index = [&](int k, double* mu_out, double* mup_out) {
        const int s = (ground && k > 0) ? k - 1 : k;                // np.interp(0, alt, .) left value = level 0
        double mu, mup;
        snell_level_index<MODE, PTAB>(a, pi, s, den, bmag, bpsi, f0, f2, unmag, &mu, &mup);
        if (!finite64(mu) || mu <= 0.0) mu = nan;                   // :1188
        if (!finite64(mup) || mup <= 0.0) mup = nan;                // :1189
        *mu_out = mu;
        *mup_out = mup;
    };
    // ... the same two numbers in the reduced algebra (REDUCED): X and Y through the reciprocals of f^2 and f
    const double rf = REDUCED ? 1.0 / f0 : 0.0;
    const double rf2 = rf * rf;
    auto level_reduced = [&](int k, double* mu_out, double* mup_out) {
        const int s = (ground && k > 0) ? k - 1 : k;
        double X, y, S2;
        if (PTAB) {
            typedef double vec2 __attribute__((ext_vector_type(2)));
            const vec2* e = reinterpret_cast<const vec2*>(a.ptab + 4 * (pi * a.n_alt + s));
            const vec2 e0 = e[0], e1 = e[1];
            X = e0.x * rf2;
            y = e0.y * rf;
            S2 = e1.x * e1.x;
        } else {
            X = (den[s] * (kPlasma * kPlasma)) * rf2;
            y = (kGyro * bmag[s]) * rf;
            S2 = sin_sq_deg(bpsi[s]);
        }
        double mu, mup, q = 0.0;
        if (unmag) index_unmagnetised(X, &mu, &mup);
        // (third-order step behind both v_rsq_f64, 7e-16 instead of the Newton step's 3.5e-15: the invariant p is made
        //  from level 0's mu, and on rays at the edge of the skip zone - one in a million of a random set - the ground
        //  range moves 1e5 times as far as p does, relatively; tests/devtools/random_sweep_rays.py)
        else index_fast_core<MODE, true>(X, y * y, S2, &mu, &mup, &q);
        if (!(q > kQCliff) || !finite64(mu) || mu <= 0.0) mu = nan;  // :233, :238, :1188
        if (!finite64(mup) || mup <= 0.0) mup = nan;                // :1189
        *mu_out = mu;
        *mup_out = mup;
    };
    const double theta0 = (90.0 - a.elev_deg[ray]) * kDegToRad;     // :1192 / :1573
    const double s0 = sin(theta0);
    auto wave_sync = [&]() {                                        // this wave's LDS writes before its reads
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    // up-leg increment of one interval, flat Earth (:1057-1061, :1224-1230); `last`: the interval that ends at the apex
    auto du_flat = [&](double dz, double mu_a, double mu_b, double p_, bool last) {
        double mm = 0.5 * (mu_a + mu_b);
        if (last) mm = fmax(mm, p_ + 1e-8);                         // :1228
        double arg = mm * mm - p_ * p_;
        if (arg < 1e-10) arg = 1e-10;
        return dz * (p_ * rsqrt_cubic(arg));                      // tan(theta) = p / sqrt(arg), :1061, to ~1 ulp
    };
    // ... spherical Earth: adaptive midpoint sub-steps of the intervals the lanes hold (:1634-1669).  The number of
    // sub-steps is very uneven - up to max_substeps (400) in the intervals next to the apex, a handful elsewhere - so
    // an interval with many of them is shared out over the 64 lanes instead of keeping one lane busy (the partial
    // sums are added in another order than the reference's loop: 1e-16 relative).  Every lane calls this.
    auto du_sphere = [&](bool have, double z0, double dz, double mu_a, double mu_b, double p_) {
        int N = 0;
        if (have && dz > 0.0) {
            const double gap_a = fmax(mu_a * (RE + z0) - p_, 1e-12);
            const double gap_b = fmax(mu_b * (RE + (z0 + dz)) - p_, 1e-12);
            const double sharp = 1.0 / fmin(gap_a, gap_b);
            double nd = fmax(1.0, ceil(fabs(dz) / a.dz_target_km));                       // :1645
            nd = fmin((double)a.max_substeps, nd * (1.0 + a.apex_boost * sharp));         // :1651
            N = (int)nd;                                                                  // int() truncates
        }
        auto substeps = [&](double z0_, double dz_, double ma, double mb, int n_sub, int first, int stride) {
            const double dN = (double)n_sub;
            const double rN = 1.0 / dN;
            const double h = dz_ / dN;
            double sum = 0.0;
            double t0 = substep_node(first, n_sub, dN, rN);
            for (int jj = first; jj < n_sub; jj += stride) {
                const double t1 = substep_node(jj + 1, n_sub, dN, rN);
                const double half = 0.5 * (t0 + t1);
                const double r_m = RE + (z0_ + half * dz_);
                double mr = (ma + (mb - ma) * half) * r_m;
                if (mr <= p_) mr = p_ + 1e-8;                                                 // :1664-1665
                const double den_ = fmax(mr * mr - p_ * p_, 1e-16);                           // :1631
                sum = sum + dphi_integrand(p_, r_m, den_) * h;
                t0 = (stride == 1) ? t1 : substep_node(jj + stride, n_sub, dN, rN);               // the next sub-step's left node
            }
            return sum;
        };
        double du = 0.0;
        unsigned long long heavy = __ballot(N >= kShared);
        while (heavy) {
            const int owner = __ffsll((long long)heavy) - 1;
            heavy &= heavy - 1;
            const double part = substeps(lane_value(z0, owner), lane_value(dz, owner), lane_value(mu_a, owner),
                                         lane_value(mu_b, owner), __builtin_amdgcn_readlane(N, owner), lane, 64);
            const double total = wave_sum(part);
            if (lane == owner) du = total;
        }
        if (N > 0 && N < kShared) du = substeps(z0, dz, mu_a, mu_b, N, 0, 1);
        return du;
    };
    // length of the path segment between (u0, z0) and (u1, z1), :1240-1241 / :1680-1683
    auto seg_len_of = [&](double u0, double z0, double u1, double z1) {
        const double du = u1 - u0, dz = z1 - z0;
        if (GEOM == 0) return hypot_km(du, dz);
        const double r_mid = RE + 0.5 * (z0 + z1);
        return hypot_km(r_mid * du, dz);
    };

    // mu and mu' of the levels base .. base + 63 (lane l: level base + l), in the launch's arithmetic: the reference's
    // order, or (REDUCED) the reduced algebra with the levels that need it evaluated again in the reference's order
    auto chunk_levels = [&](int base, double p_now, double* m_out, double* mp_out) {
        const int k = base + lane;
        double m = nan, mp = nan;
        if (REDUCED) {
            if (k < n) level_reduced(k, &m, &mp);
            double p_c = p_now;                                      // (the first chunk makes p: from its level 0)
            if (base == 0) {
                const double mu0 = lane_value(m, 0);
                p_c = (GEOM == 0) ? mu0 * s0 : (mu0 * (RE + level_alt(0))) * s0;
            }
            const double cr = (GEOM == 0) ? m : m * (RE + level_alt(k < n ? k : n - 1));
            const bool keep = (m * m > kReducedMinMu2) && (mp > 0.5) && (cr * cr - p_c * p_c > kReducedApex * (cr * cr));
            const bool redo = k < n && !keep;                        // (a NaN anywhere fails `keep`)
            if (__any(redo)) {
                if (redo) level_index(k, &m, &mp);
            }
        } else if (k < n) {
            level_index(k, &m, &mp);
        }
        *m_out = m;
        *mp_out = mp;
    };
    // ---- A ray that never turns pays for its levels only (REDUCED).  Such a ray - a third of a random fan - walks all
    // 621 levels, and two thirds of what a chunk costs is the interval work (compaction, up-leg increment, running sum,
    // segment length, delay) that its NaN result never uses.  Where mu at the level of the largest density (a hint from
    // snell_profile_kernel) stays above p - the ray probably escapes - the levels are scanned first for the bracket alone:
    // the same level values and the same test as below, chunk by chunk; nothing found means the ray escapes, anything
    // else - a bracket, or a chunk with a blanked level between finite ones - hands the ray to the full pass below, from
    // the start.  The hint only chooses the order of work: every result is the full pass's or the scan's identical verdict.
    if (REDUCED) {
        const int k_peak = min((int)a.prof_info[4 * pi + 2] + ground, n - 1);
        double m_h = nan, mp_h = nan;
        level_reduced(lane == 0 ? 0 : k_peak, &m_h, &mp_h);
        const double mu0_h = lane_value(m_h, 0), mu_pk = lane_value(m_h, 1);
        const double p_h = (GEOM == 0) ? mu0_h * s0 : (mu0_h * (RE + level_alt(0))) * s0;
        const double c_pk = (GEOM == 0) ? mu_pk : mu_pk * (RE + level_alt(k_peak));
        if (c_pk > p_h * (1.0 + 1e-9)) {
            bool escapes = true;                                     // (so far)
            double p_s = nan, c_prev = nan;
            int seen = 0;                                            // finite levels so far
            for (int base = 0; base < n && escapes; base += 64) {
                double m, mp;
                chunk_levels(base, p_s, &m, &mp);
                if (base == 0) {
                    const double mu0 = lane_value(m, 0);
                    if (!finite64(mu0) || (GEOM == 0 && !finite64(s0))) { fail(); return; }
                    p_s = (GEOM == 0) ? mu0 * s0 : (mu0 * (RE + level_alt(0))) * s0;     // :1201 / :1584
                }
                const int kk = base + lane;
                const unsigned long long mask = __ballot(m == m);
                const int cnt = __popcll(mask);
                if ((mask & (mask + 1ull)) != 0ull) { escapes = false; break; }          // a blanked level in between
                const double cb = (GEOM == 0) ? m : m * (RE + ((kk < n) ? level_alt(kk) : 0.0));      // :1598
                const double ca = wave_shift_up_1(cb, c_prev);
                const bool have = lane < cnt && (seen > 0 || lane > 0);
                if (__ballot(have && ca >= p_s && cb <= p_s)) { escapes = false; break; }
                if (cnt > 0) {
                    c_prev = lane_value(cb, cnt - 1);
                    seen += cnt;
                }
            }
            if (escapes) { fail(); return; }
        }
    }

    // ---- levels from the ground up, 64 at a time: the finite ones (:1204-1205) are compacted, their intervals tested
    // for the bracket where mu (flat) or mu r (spherical, Bouguer) falls through p (:1085-1093 / :1598-1603) and - up
    // to that bracket - integrated; the levels above the bracket cannot change any output and are never evaluated ---
    double p = nan;
    int nv = 0, it = -1;
    double u_carry = 0.0;                // up-leg coordinate of compacted level nv - 1
    double len_acc = 0.0, delay_acc = 0.0;         // this lane's share of the up-leg length and group delay
    double z_turn = 0.0;
    int n_grid = 0;                      // up-leg nodes taken from the grid
    // the compacted level in front of the chunk in flight (nv - 1): mu, mu', altitude; wave-uniform, in scalar registers
    double c1_mu = nan, c1_mup = nan, c1_z = 0.0;
    double lo_mu = nan, lo_mup = nan, lo_z = 0.0;  // ... and compacted level n_grid - 1, the foot of the apex interval
    bool foot_again = false;
    // mu' of the last chunk's levels (lane l: grid level base_chunk + l) stays in registers behind the loop: the two grid
    // levels around the turning point, which the apex needs (:1244 / :1686), are almost always among them
    double mp_chunk = nan;
    int base_chunk = 0;
    if (lane == 0) u_up[0] = 0.0;
    for (int base = 0; base < n && it < 0; base += 64) {
        const int k = base + lane;
        double m = nan, mp = nan;
        chunk_levels(base, p, &m, &mp);
        mp_chunk = mp;
        base_chunk = base;
        if (base == 0) {
            const double mu0 = lane_value(m, 0);
            if (!finite64(mu0) || (GEOM == 0 && !finite64(s0))) { fail(); return; }
            p = (GEOM == 0) ? mu0 * s0 : (mu0 * (RE + level_alt(0))) * s0;         // :1201 / :1584
        }
        const bool ok = m == m;
        const unsigned long long mask = __ballot(ok);
        const int cnt = __popcll(mask);
        // The finite levels of a chunk are almost always its lanes 0 .. cnt - 1 (no blanked level in between): compaction
        // is then the identity, a lane's level is its own and the level below it its neighbour's - a DPP shift, with the
        // level carried over from the chunk before into lane 0 - and nothing but the level index goes through LDS
        const bool in_place = (mask & (mask + 1ull)) == 0ull;
        const double z_own = (k < n) ? level_alt(k) : 0.0;
        if (ok) {
            const int rank = __popcll(mask & ((1ull << lane) - 1ull));
            kidx[nv + rank] = (unsigned short)k;
            if (!in_place) {
                stg_mu[rank] = m;
                stg_mup[rank] = mp;
                stg_z[rank] = z_own;
            }
        }
        if (!in_place) wave_sync();
        // lane j: the interval between compacted levels nv - 1 + j (the carry for j = 0) and nv + j (rank j of this chunk)
        const bool have = lane < cnt && (nv > 0 || lane > 0);
        double mu_a = c1_mu, mup_a = c1_mup, z0 = c1_z, mu_b = nan, mup_b = nan, z1 = 0.0;
        if (in_place) {
            z1 = z_own; mu_b = m; mup_b = mp;                        // (lanes at and beyond cnt: not used)
            z0 = wave_shift_up_1(z_own, c1_z);
            mu_a = wave_shift_up_1(m, c1_mu);
            mup_a = wave_shift_up_1(mp, c1_mup);
        } else if (lane < cnt) {
            z1 = stg_z[lane]; mu_b = stg_mu[lane]; mup_b = stg_mup[lane];
            if (lane > 0) { z0 = stg_z[lane - 1]; mu_a = stg_mu[lane - 1]; mup_a = stg_mup[lane - 1]; }
        }
        const double ca = (GEOM == 0) ? mu_a : mu_a * (RE + z0), cb = (GEOM == 0) ? mu_b : mu_b * (RE + z1);     // :1598
        const unsigned long long found = __ballot(have && ca >= p && cb <= p);
        int n_int = cnt;                 // intervals of this chunk that belong to the up-leg whole: lanes [.., n_int)
        if (found) {
            const int js = __ffsll((long long)found) - 1;
            it = nv - 1 + js;
            const double za = lane_value(z0, js), zb = lane_value(z1, js), cas = lane_value(ca, js), cbs = lane_value(cb, js);
            if (GEOM == 0) {
                z_turn = za;                                                // :1089-1092
                if (cas != cbs) z_turn = za + ((cas - p) / (cas - cbs)) * (zb - za);
                n_grid = (z_turn == za) ? it : it + 1;                      // np.searchsorted(zv, z_turn), :1219
            } else {
                double t = (cas != cbs) ? (cas - p) / (cas - cbs) : 0.0;    // :1617-1619
                t = fmin(fmax(t, 0.0), 1.0);
                z_turn = za + t * (zb - za);
                n_grid = it + 1;                                            // zv[:i0 + 1], :1622
            }
            n_int = n_grid - nv;         // the intervals whose upper end is a grid node of the up-leg: s + 1 <= n_grid - 1
            // compacted level n_grid - 1: rank r of this chunk (the upper node of lane r's interval) or a carried one
            const int r = n_grid - 1 - nv;
            if (r >= 0) { lo_mu = lane_value(mu_b, r); lo_mup = lane_value(mup_b, r); lo_z = lane_value(z1, r); }
            else if (r == -1) { lo_mu = c1_mu; lo_mup = c1_mup; lo_z = c1_z; }
            else foot_again = true;      // (flat Earth, the turning point ON the level in front of this chunk: the foot is
                                         //  the level before that one, which nothing holds any more - evaluated again below)
        }
        const bool up = have && lane < n_int;
        const double dz = z1 - z0;
        double du = 0.0;
        if (GEOM == 0) {
            if (up) du = du_flat(dz, mu_a, mu_b, p, false);
        } else {
            du = du_sphere(up, z0, dz, mu_a, mu_b, p);
        }
        double incl = wave_inclusive_scan(up ? du : 0.0, lane) + u_carry;
        if (GEOM == 1) incl = restart_behind_empty_intervals(incl, up ? du : 0.0, up && dz <= 0.0, lane);
        const double u_lo = wave_shift_up_1(incl, u_carry);          // the lane below's sum; lane 0: the carry
        if (up) {
            u_up[nv + lane] = incl;                                  // compacted level nv + lane, the interval's upper node
            // the interval's length and its share of the group delay: half the sum of mu' at its ends times the
            // length (:1240-1246)
            const double ds = seg_len_of(u_lo, z0, incl, z1);
            const double half_mup = 0.5 * (mup_a + mup_b);
            const double tt = (REDUCED ? half_mup * (1.0 / kLightKmS) : half_mup / kLightKmS) * ds;    // :1245-1246
            if (ds == ds) len_acc += ds;
            if (tt == tt) delay_acc += tt;
        }
        // the coordinate of the last node written - the lane of the chunk's last up-leg interval (the lanes behind it add
        // zeros, but in another order of additions: their sums are an ulp apart from the node in the path array)
        u_carry = lane_value(incl, n_int > 0 ? n_int - 1 : 63);
        if (it < 0 && cnt > 0) {         // the chunk's last compacted level leads the next chunk
            const int l1 = 63 - __builtin_clzll(mask);
            c1_mu = lane_value(m, l1);
            c1_mup = lane_value(mp, l1);
            c1_z = level_alt(base + l1);
            nv += cnt;
        }
    }
    if (it < 0) { fail(); return; }                                 // also the reference's "fewer than 2 levels" exit
    // ---- the interval that ends at the apex: from compacted level n_grid - 1 to z_turn ---------------------------
    const int n_up = n_grid + 1;
    const double mu_apex = (GEOM == 0) ? p : p / (RE + z_turn);     // :1221 / :1624
    // mu' at the apex: np.interp on the full grid, NaN-aware (:1244 / :1686).  Number of grid levels at or below z_turn:
    // all those up to the bracket's lower level, plus the (blanked) ones between the bracket's two levels that z_turn
    // has passed
    wave_sync();
    const int k_lo = kidx[it], k_hi = kidx[it + 1];
    int below = 0;
    for (int k = k_lo + 1 + lane; k <= k_hi; k += 64) below += (level_alt(k) <= z_turn) ? 1 : 0;
    below = k_lo + 1 + (int)(wave_sum((double)below) + 0.5);
    const int j = below - 1;
    // mu' on grid levels j and j + 1 (lanes 0 and 1 evaluate them; nothing is stored for the full grid); lane 2: the
    // foot of the apex interval where no register holds it any more
    double mup_lo, mup_hi;
    double u_foot = u_carry;             // up-leg coordinate of compacted level n_grid - 1: the last chunk's scan ends there
    const int kj = j < 0 ? 0 : j;
    if (!foot_again && kj >= base_chunk && kj + 1 < base_chunk + 64) {
        // both levels were evaluated with the last chunk (a level past the grid's end: NaN there, as below)
        mup_lo = lane_value(mp_chunk, kj - base_chunk);
        mup_hi = lane_value(mp_chunk, kj + 1 - base_chunk);
    } else {
        double mu_j = nan, mup_j = nan;
        const int kf = (foot_again && n_grid >= 1) ? (int)kidx[n_grid - 1] : 0;
        const int kk = (lane == 2) ? kf : kj + (lane & 1);
        if (kk < n) level_index(kk, &mu_j, &mup_j);
        if (foot_again && n_grid >= 1) {
            lo_mu = lane_value(mu_j, 2);
            lo_mup = lane_value(mup_j, 2);
            lo_z = level_alt(kf);
            u_foot = u_up[n_grid - 1];   // (an earlier chunk wrote it; u_carry is one level further up here)
        }
        mup_lo = lane_value(mup_j, 0);
        mup_hi = lane_value(mup_j, 1);
    }
    double mup_apex;
    if (j < 0) mup_apex = mup_lo;
    else mup_apex = interp_nan_aware(z_turn, j, n, level_alt(j), (j + 1 < n) ? level_alt(j + 1) : 0.0, mup_lo,
                                     (j + 1 < n) ? mup_hi : 0.0);
    double u_turn = 0.0;
    double ds_last = 0.0;                                           // length of the segment that ends at the apex
    if (n_grid >= 1) {
        const double u_l = u_foot;                                  // = u_up[n_grid - 1]
        const double dz = z_turn - lo_z;
        double du;
        if (GEOM == 0) du = du_flat(dz, lo_mu, mu_apex, p, true);
        else du = lane_value(du_sphere(lane == 0, lo_z, dz, lo_mu, mu_apex, p), 0);
        u_turn = u_l + du;
        if (GEOM == 1 && dz <= 0.0) u_turn = 0.0;                   // (restart_behind_empty_intervals: the apex interval's turn)
        const double ds = seg_len_of(u_l, lo_z, u_turn, z_turn);
        const double tt = ((0.5 * (lo_mup + mup_apex)) / kLightKmS) * ds;
        if (lane == 0 && ds == ds) len_acc += ds;
        if (lane == 0 && tt == tt) delay_acc += tt;
        ds_last = ds;
    }
    if (lane == 0) u_up[n_up - 1] = u_turn;
    // the path mirrored about the apex: twice the up-leg (:1232-1246 / :1671-1689)
    const double path = 2.0 * wave_sum(len_acc);
    const double delay = 2.0 * wave_sum(delay_acc);
    const int n_seg = 2 * (n_up - 1);
    // midpoint (:1248-1252 / :1691-1695): the first node of the last up-leg segment that has a length (the comment in
    // front of this function) - the foot of the apex interval, which the registers still hold, unless that interval
    // is empty (spherical Earth, the turning point ON a level, :1617-1622)
    double x_mid = nan, z_mid = nan;
    if (path > 0.0) {
        double um = u_foot, zm = lo_z;
        if (!(ds_last > 0.0)) {
            wave_sync();
            auto z_at = [&](int s) { return s < n_grid ? zv(s) : z_turn; };
            int km = n_up - 2;
            while (km > 0 && u_up[km + 1] == u_up[km] && z_at(km + 1) == z_at(km)) --km;
            um = u_up[km];
            zm = z_at(km);
        }
        x_mid = (GEOM == 0) ? um : RE * um;                         // x = R_E phi, :1678
        z_mid = zm;
    }
    const double z_first = (n_grid >= 1) ? zv(0) : z_turn;          // the path ends where it began
    const double u_end = 2.0 * u_turn - 0.0;
    const double x_end = (GEOM == 0) ? u_end : RE * u_end;
    const double landed = (fabs(z_first) <= 1e-3) ? x_end : nan;                    // :1256-1258 / :1699-1701

    if (lane == 0) {
        out[0] = path; out[1] = delay; out[2] = x_mid; out[3] = z_mid; out[4] = landed;
        out[5] = (GEOM == 0) ? u_turn : RE * u_turn; out[6] = z_turn; out[7] = (double)(2 * n_up - 1);
    }
    (void)n_seg;
    if (a.path_x) {
        wave_sync();
        auto z_node = [&](int s) { return s < n_grid ? zv(s) : z_turn; };
        auto u_path = [&](int k) { return (k < n_up) ? u_up[k] : 2.0 * u_turn - u_up[2 * n_up - 2 - k]; };
        auto z_path = [&](int k) { return (k < n_up) ? z_node(k) : z_node(2 * n_up - 2 - k); };
        const int n_path = 2 * n_up - 1;
        for (long long k = lane; k < a.path_stride; k += 64) {
            double xv = nan, zz = nan;
            if (k < n_path) {
                xv = (GEOM == 0) ? u_path((int)k) : RE * u_path((int)k);
                zz = z_path((int)k);
            }
            a.path_x[ray * a.path_stride + k] = xv;
            a.path_z[ray * a.path_stride + k] = zz;
        }
    }
}

// mu and mu' of level k of group g (:1184-1189), NaN where the reference blanks them: exactly the per-ray evaluation
template <int MODE>
__device__ __forceinline__ void snell_level(const SnellArgs& a, long long g, long long pi, int ground, int n, int k,
                                            double* mu_out, double* mup_out) {
#pragma clang fp contract(off)
    const double* den = a.den + pi * a.prof_stride;
    const double* bmag = a.bmag + pi * a.prof_stride;
    const double* bpsi = a.bpsi + pi * a.prof_stride;
    double mu = qnan(), mup = qnan();
    if (k < n) {
        const double f0 = a.group_freq[g];
        const double f2 = f0 * f0;
        const int unmag = ((kGyro * a.prof_info[4 * pi]) / f0 < kUnmagTol) ? 1 : 0;
        const int s = (ground && k > 0) ? k - 1 : k;
        if (a.ptab) snell_level_index<MODE, true>(a, pi, s, den, bmag, bpsi, f0, f2, unmag, &mu, &mup);
        else snell_level_index<MODE, false>(a, pi, s, den, bmag, bpsi, f0, f2, unmag, &mu, &mup);
        if (!finite64(mu) || mu <= 0.0) mu = qnan();                 // :1188
        if (!finite64(mup) || mup <= 0.0) mup = qnan();              // :1189
    }
    *mu_out = mu;
    *mup_out = mup;
}

// The tables of a grouped launch, one workgroup per (profile, frequency) group - the rays of the group then share them:
//   * mu' of every level, exactly the per-ray evaluation of snell_ray (:1184-1189): a.levels (the apex needs mu'
//     of grid levels, blanked ones included);
//   * the levels with a finite mu (:1204-1205) as a compacted list - altitude, mu, mu' and the running minimum of the
//     bracket criterion over the entries 1 .. i (snell_ray_table) - the grid level of each entry, the group's scalars.
// A thread per level and trip (the workgroup is sized so that the trips are full: 320 threads x 2 for 621 levels); the
// list positions come from the wavefronts' ballots and a prefix over their counts in LDS.  (Rounds 2 - 5 made the level
// tables with a thread per (group, level) and - round 5 - the lists in a kernel of their own that read them back: one
// launch and 16 B per level of traffic more, in front of launches that take a fifth of a millisecond.)
constexpr int kTableThreads = 512;
template <int MODE>
__device__ __forceinline__ void snell_group_tables(const SnellArgs& a) {
#pragma clang fp contract(off)
    constexpr int kWaves = kTableThreads / 64;
    __shared__ int s_count[kWaves];
    __shared__ double s_least[kWaves];
    __shared__ int s_level0;
    const long long g = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = (int)blockDim.x >> 6;
    const long long pi_given = a.group_prof ? a.group_prof[g] : 0;
    const bool bad_index = pi_given < 0 || pi_given >= a.n_prof;
    const long long pi = bad_index ? 0 : pi_given;                   // (such rays fail in snell_ray_table)
    const double* alt = a.alt + pi * a.alt_stride;
    const int ground = (alt[0] > 0.0) ? 1 : 0;                       // :1175-1182 / :1556-1563 ground level
    const int n = (int)a.n_alt + ground;
    const int n_lev = (int)a.n_alt + 1;
    double* lev = a.levels + g * (a.n_alt + 1);
    double* ent = a.group_entries + g * (4 * (a.n_alt + 1));
    int* kid = a.group_kidx + g * (a.n_alt + 1);
    const double RE = a.earth_radius_km;
    const double inf = __builtin_inf();
    int nv = 0;
    double run = inf;
    bool level0 = true;
    for (int base = 0; base < n_lev; base += (int)blockDim.x) {
        const int k = base + (int)threadIdx.x;
        double m = qnan(), mp = qnan(), z = 0.0;
        if (k < n_lev) {
            snell_level<MODE>(a, g, pi, ground, n, k, &m, &mp);
            lev[k] = mp;
            if (k < n) z = (ground && k == 0) ? 0.0 : alt[k - ground];
        }
        const bool ok = m == m;
        const unsigned long long mask = __ballot(ok);
        const double crit = (a.geometry == 0) ? m : m * (RE + z);   // :1598
        const double v = (ok && k >= 1 && crit == crit) ? crit : inf;        // (entry 0 is level 0: not part of the minimum)
        double sc = -wave_scan_max(-v);
        if (lane == 63) s_least[wave] = sc;
        if (lane == 0) s_count[wave] = __popcll(mask);
        if (k == 0) s_level0 = ok ? 1 : 0;
        __syncthreads();
        if (base == 0) level0 = s_level0 != 0;                       // level 0 blanked: no entries, the group's rays fail
        int pos = nv + __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
        double least = inf;
        for (int w = 0; w < waves; ++w) {
            const int c = s_count[w];
            const double l = s_least[w];
            if (w < wave) { pos += c; sc = fmin(sc, l); }
            total += c;
            least = fmin(least, l);
        }
        sc = fmin(sc, run);
        if (ok && level0) {
            double* e = ent + 4 * pos;
            e[0] = z; e[1] = m; e[2] = mp; e[3] = sc;
            kid[pos] = k;
        }
        nv += total;
        run = fmin(run, least);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int* info = a.group_info + 4 * g;
        info[0] = level0 ? nv : 0;
        info[1] = ground;
        info[2] = (bad_index ? 1 : 0) | ((a.prof_info[4 * pi + 1] != 0.0) ? 2 : 0);
        info[3] = (int)pi;
    }
}
__global__ __launch_bounds__(kTableThreads) void snell_tables_kernel(const SnellArgs a) {
    if (a.mode == PRHF_KMODE_O) snell_group_tables<PRHF_KMODE_O>(a);
    else snell_group_tables<PRHF_KMODE_X>(a);
}

constexpr int kRaySlices = 8;                   // queues of a per-ray launch (one per XCD), each over its own slice of the rays
constexpr int kRayQueueStride = 32;             // unsigned words between two queues' counters (128 B: separate channels)
// max|B| and "some density is negative" per profile, read by every ray (the first wavefront of a profile's n_chunk).
// With a.ptab: the frequency-independent parts of every level's mu and mu' as well (SnellArgs::ptab), 64 levels per
// wavefront - one wavefront per profile walked its 620 levels through the double-double sine and cosine ten at a time,
// 19 us in front of a launch of 16 or 256 profiles (a tenth of what a fan of 200 000 rays takes).
__global__ __launch_bounds__(64) void snell_profile_kernel(const SnellArgs a, int n_chunk) {
#pragma clang fp contract(off)
    const long long p = blockIdx.x / n_chunk;
    const int chunk = (int)(blockIdx.x - p * n_chunk);
    const int lane = threadIdx.x;
    const double* den = a.den + p * a.prof_stride;
    const double* bmag = a.bmag + p * a.prof_stride;
    const double* bpsi = a.bpsi + p * a.prof_stride;
    if (a.ptab) {
        const int k = chunk * 64 + lane;
        if (k < (int)a.n_alt) {
            double* e = a.ptab + 4 * (p * a.n_alt + k);
            const double fn = sqrt(den[k]) * kPlasma;          // :96 (NaN for a negative density: such rays fail)
            double sn, cs;
            faithful_sincos(bpsi[k], &sn, &cs);
            e[0] = fn * fn;                                    // :136 numerator
            e[1] = kGyro * bmag[k];                            // :157 numerator
            e[2] = sn;
            e[3] = cs;
        }
    }
    if (blockIdx.x == 0 && a.ray_queue && lane < kRaySlices) a.ray_queue[lane * kRayQueueStride] = 0u;   // (the per-ray launch's queues)
    if (chunk != 0) return;
    double bmax = 0.0, dmax = -1.0;
    int neg = 0, kmax = 0;
    // (four trips' loads in flight: this wavefront's ten dependent trips were the kernel's length)
    for (int k0 = lane; k0 < (int)a.n_alt; k0 += 256) {
        double bv[4], dv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 64 * u;
            bv[u] = (k < (int)a.n_alt) ? bmag[k] : 0.0;
            dv[u] = (k < (int)a.n_alt) ? den[k] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 64 * u;
            if (k >= (int)a.n_alt) continue;
            bmax = fmax(bmax, fabs(bv[u]));
            neg |= (dv[u] < 0.0) ? 1 : 0;
            if (dv[u] > dmax) { dmax = dv[u]; kmax = k; }       // (a hint for the rays - where mu is smallest - never a result)
        }
    }
    bmax = wave_max(bmax);
    neg = __any(neg) ? 1 : 0;
    const double dtop = wave_max(dmax);
    const unsigned long long at = __ballot(dmax == dtop);
    const int ktop = __builtin_amdgcn_readlane(kmax, at ? __ffsll((long long)at) - 1 : 0);
    if (lane == 0) {
        a.prof_info[4 * p] = bmax;
        a.prof_info[4 * p + 1] = (double)neg;
        a.prof_info[4 * p + 2] = (double)ktop;             // level of the largest density (any of them on a tie)
        a.prof_info[4 * p + 3] = 0.0;
    }
}

#ifndef PRHF_SNELL_BATCH
#define PRHF_SNELL_BATCH 4
#endif
constexpr int kRayBatch = PRHF_SNELL_BATCH;     // rays a persistent wavefront draws from the queue at a time
template <int GEOM, bool PTAB, bool REDUCED>
__device__ __forceinline__ void snell_dispatch(const SnellArgs& a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* lds = reinterpret_cast<double*>(smem);
    // The per-ray launch is persistent: as many wavefronts as the device keeps resident, every one drawing its next
    // rays from a queue - rays differ a lot in cost (the early stop).  One counter for the whole launch took ~12 ns a
    // draw (an atomic that every XCD must see is served one at a time, memory-side): 8 rays had to be drawn at a time
    // to keep the draws (25 000 x 12 ns) below the rays' own time - at 4 the flat launch ran at the counter's pace, at 2
    // both ran at half speed - and a wavefront's last batch of 8 was the launch's tail.  Now the rays are cut into kRaySlices slices with a counter each, 128 B apart; a wavefront draws
    // kRayBatch rays from the slice of its XCD (workgroups go round the XCDs: blockIdx.x mod 8) and, when that one is
    // exhausted, from the next ones in turn.  A draw either yields rays or moves the wavefront on to the next slice,
    // and after kRaySlices moves it leaves: the grid always drains.
    const long long per_slice = ((a.n_rays + kRaySlices * kRayBatch - 1) / (kRaySlices * kRayBatch)) * kRayBatch;
    int slice = (int)(blockIdx.x % kRaySlices);
    // (the draw for the following batch in flight while this one's rays are traced: measured, no gain - one more live
    //  register for a round trip that the other wavefronts of the SIMD cover)
    for (int moves = 0; moves < kRaySlices;) {
        unsigned next = 0;
        if (threadIdx.x == 0) next = atomicAdd(a.ray_queue + slice * kRayQueueStride, 1u);
        const long long offset = (long long)(unsigned)__builtin_amdgcn_readfirstlane((int)next) * kRayBatch;
        const long long first = slice * per_slice + offset;
        if (offset >= per_slice || first >= a.n_rays) {              // this slice has no rays left
            slice = (slice + 1) % kRaySlices;
            ++moves;
            continue;
        }
        long long last = first + kRayBatch;
        if (last > a.n_rays) last = a.n_rays;
        for (long long ray = first; ray < last; ++ray) {
            if (a.mode == PRHF_KMODE_O) snell_ray<PRHF_KMODE_O, GEOM, PTAB, REDUCED>(a, ray, lds);
            else snell_ray<PRHF_KMODE_X, GEOM, PTAB, REDUCED>(a, ray, lds);
            __syncthreads();                           // (one wavefront: this ray's LDS reads before the next one's writes)
        }
    }
}
// PTAB: the levels' frequency-independent parts come from the per-profile table (SnellArgs::ptab) - a kernel of its own,
// so that neither variant carries the other's registers
#ifndef PRHF_SNELL_WAVES
#define PRHF_SNELL_WAVES 4          // register budget of the per-ray kernel in waves per SIMD
#endif
// ... and one per geometry: the flat-Earth ray carries none of the sub-steps' registers
template <int GEOM, bool PTAB, bool REDUCED>
__global__ __launch_bounds__(64, PRHF_SNELL_WAVES) void snell_kernel(const SnellArgs a) { snell_dispatch<GEOM, PTAB, REDUCED>(a); }
// grouped launch: every ray reads its levels from its group's table (a.ray_group, a.levels set)
#ifndef PRHF_FAN_WAVES
#define PRHF_FAN_WAVES (GEOM == 0 ? 8 : 7)   // register budget of the fan kernels in waves per SIMD (flat: 46 VGPRs; spherical: 72)
#endif
// (one kernel per geometry: the flat-Earth ray needs a third fewer registers than the spherical one with its sub-steps)
template <int GEOM>
__global__ __launch_bounds__(64, PRHF_FAN_WAVES) void snell_fan_kernel(const SnellArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const long long ray = blockIdx.x;
    if (ray < a.n_rays) snell_ray_table<GEOM>(a, ray, reinterpret_cast<double*>(smem));
}

static size_t snell_lds_bytes(long long n_alt, bool table) {   // up-leg coordinate; per-ray launch: level indices, mu, mu' of a chunk
    if (table) return (size_t)(n_alt + 2) * sizeof(double);
    return (size_t)(n_alt + 2) * sizeof(double) + 3 * 64 * sizeof(double) + (size_t)(n_alt + 2) * sizeof(unsigned short);
}

template <int GEOM>
static const void* snell_kernel_of(bool ptab, bool reduced) {
    if (ptab) return reduced ? reinterpret_cast<const void*>(&snell_kernel<GEOM, true, true>) : reinterpret_cast<const void*>(&snell_kernel<GEOM, true, false>);
    return reduced ? reinterpret_cast<const void*>(&snell_kernel<GEOM, false, true>) : reinterpret_cast<const void*>(&snell_kernel<GEOM, false, false>);
}
static const void* snell_kernel_for(int geometry, bool ptab, bool reduced) {
    return geometry == 0 ? snell_kernel_of<0>(ptab, reduced) : snell_kernel_of<1>(ptab, reduced);
}

size_t snell_queue_bytes() { return (size_t)kRaySlices * kRayQueueStride * sizeof(unsigned); }

hipError_t snell_resident_waves(long long n_alt, int cu_count, long long* waves, bool ptab, bool reduced, int geometry) {
    int per_cu = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, snell_kernel_for(geometry, ptab, reduced), 64, snell_lds_bytes(n_alt, false));
    if (e != hipSuccess) return e;
    if (per_cu < 1) per_cu = 1;
    *waves = (long long)per_cu * (long long)(cu_count > 0 ? cu_count : 256);
    return hipSuccess;
}

hipError_t launch_snell(const SnellArgs& a, hipStream_t stream) {
    if (a.n_rays <= 0) return hipSuccess;
    // the up-leg coordinate and the 16-bit level index of every compacted level, the chunk's staging area
    if (a.n_alt + 2 > 65535) return hipErrorInvalidValue;
    const size_t lds_bytes = snell_lds_bytes(a.n_alt, a.ray_group != nullptr);
    const void* kernel = a.ray_group ? (a.geometry == 0 ? reinterpret_cast<const void*>(&snell_fan_kernel<0>)
                                                        : reinterpret_cast<const void*>(&snell_fan_kernel<1>))
                                     : snell_kernel_for(a.geometry, a.ptab != nullptr, a.reduced != 0);
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    const int n_chunk = a.ptab ? (int)((a.n_alt + 63) / 64) : 1;
    if (a.n_prof * n_chunk > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(snell_profile_kernel, dim3((unsigned)(a.n_prof * n_chunk)), dim3(64), 0, stream, a, n_chunk);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.ray_group) {
        // trips of a workgroup over the n_alt + 1 levels, and the wavefronts that fill them
        const int n_lev = (int)a.n_alt + 1;
        const int trips = (n_lev + kTableThreads - 1) / kTableThreads;
        const int threads = 64 * ((n_lev + 64 * trips - 1) / (64 * trips));
        hipLaunchKernelGGL(snell_tables_kernel, dim3((unsigned)a.n_groups), dim3((unsigned)threads), 0, stream, a);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (a.ray_group) {
        void* params[] = {const_cast<SnellArgs*>(&a)};
        e = hipLaunchKernel(kernel, dim3((unsigned)a.n_rays), dim3(64), params, lds_bytes, stream);
        if (e != hipSuccess) return e;
    } else {
        if (!a.ray_queue || a.n_rays > 0x7fffffffLL) return hipErrorInvalidValue;
        long long waves = 0;
        e = snell_resident_waves(a.n_alt, a.resident_cus, &waves, a.ptab != nullptr, a.reduced != 0, a.geometry);
        if (e != hipSuccess) return e;
        const long long batches = (a.n_rays + kRayBatch - 1) / kRayBatch;      // draws that yield rays (snell_dispatch)
        const dim3 grid((unsigned)(batches < waves ? batches : waves));
        void* params[] = {const_cast<SnellArgs*>(&a)};
        e = hipLaunchKernel(kernel, grid, dim3(64), params, lds_bytes, stream);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}
