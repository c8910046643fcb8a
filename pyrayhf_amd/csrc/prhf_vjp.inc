// prhf_vjp.inc - the derivative of the vertical forward operator with respect to the density column (DESIGN.md
// section 4.14): dense Jacobian rows (vfo_jacobian_kernel) and the vector-Jacobian product (vfo_vjp_kernel).
// Included from prhf_kernels.hip, inside namespace prhf.
//
// The function differentiated is the reference's discrete sum (library.py:324-438, :259-293) as oracle/vfo_numpy.py
// restates it:  vh = min(alt) + sum_i mu'(X(z_i), Y(z_i), psi(z_i)) D_i,  z_i = alt_0 + m_i H,  D_i = (m_i+1 - m_i) H
// (the last one 1e-6),  H = h - alt_0 with h np.interp's crossing of the running maximum of X (O) / X + Y (X) minus
// 1e-6.  Per reflecting pair
//   d vh / d den_k = sum_i D_i (dmu'/dX)_i cX [w_ik + m_i sden_i dH/dden_k]  +  S_H dH/dden_k
//   S_H = sum_{i<n-1} mu'_i (m_i+1 - m_i) + sum_i D_i m_i (dmu'/dz along Y and psi)_i
// where w_ik is the interpolation weight of level k at z_i and dH/dden_k is non-zero at two levels only: the level jm
// where the running maximum below the crossing was FIRST attained and the level j + 1 above it.  The bracket - the
// total dX of a node - is formed per node before it meets dmu'/dX ~ (1 - X)^-3/2: at the last grid points the two
// parts cancel, 1 - X there being pinned at X' 1e-6.
// mu' and its two tangents (d/dX; d/dz through Y and psi) are forward-mode dual numbers pushed through the algebra of
// group_index_lean around a = 1 - X, with IEEE sqrt and divide, in every tier.  O mode forms G = beta - h as
// t a / (beta + h): no cancellation at reflection.
//
// One workgroup per profile: the bottomside is staged once (stage_profile), waves take frequencies, lanes take grid
// points.  A trip's points lie in non-decreasing segments; the two sums of each run of equal segment are reduced by
// a segmented scan and added by the run's last lane to the wave's row in LDS.  Nothing is accumulated in global
// memory, every order of addition is fixed: the bits depend on the profile and the launch's shape only.

namespace {

struct Dual {
    double v, a, b;          // value, d/dX, d/dz (Y and psi only)
};
__device__ __forceinline__ Dual dual(double v) { return Dual{v, 0.0, 0.0}; }
__device__ __forceinline__ Dual operator+(Dual x, Dual y) { return Dual{x.v + y.v, x.a + y.a, x.b + y.b}; }
__device__ __forceinline__ Dual operator-(Dual x, Dual y) { return Dual{x.v - y.v, x.a - y.a, x.b - y.b}; }
__device__ __forceinline__ Dual operator-(Dual x) { return Dual{-x.v, -x.a, -x.b}; }
__device__ __forceinline__ Dual operator*(Dual x, Dual y) {
    return Dual{x.v * y.v, x.a * y.v + x.v * y.a, x.b * y.v + x.v * y.b};
}
__device__ __forceinline__ Dual operator/(Dual x, Dual y) {
    const double q = x.v / y.v;
    return Dual{q, (x.a - q * y.a) / y.v, (x.b - q * y.b) / y.v};
}
__device__ __forceinline__ Dual operator-(double s, Dual x) { return Dual{s - x.v, -x.a, -x.b}; }
__device__ __forceinline__ Dual operator+(double s, Dual x) { return Dual{s + x.v, x.a, x.b}; }
__device__ __forceinline__ Dual operator*(double s, Dual x) { return Dual{s * x.v, s * x.a, s * x.b}; }
__device__ __forceinline__ Dual dual_sqrt(Dual x) {
    const double r = sqrt(x.v);
    return Dual{r, x.a / (2.0 * r), x.b / (2.0 * r)};
}

// One wave's LDS operations complete in order; this keeps the compiler from moving them across (lanes of the wave
// read and add to words that other lanes of it wrote)
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// mu' below the reflection height from X, Y^2, sin^2 psi, cos^2 psi; *ok: D > 0 and 0 < mu^2 <= 1 (library.py:233, :238)
template <int MODE>
__device__ __forceinline__ Dual group_index_dual(Dual X, Dual Y2, Dual S2, Dual C2, bool* ok) {
#pragma clang fp contract(off)
    constexpr double sgn = (MODE == PRHF_KMODE_O) ? 1.0 : -1.0;
    const Dual a = 1.0 - X;
    const Dual YL2 = Y2 * C2;
    const Dual h = 0.5 * (Y2 * S2);
    const Dual t = YL2 * a;
    const Dual ta = t * a;
    const Dual beta = dual_sqrt(h * h + ta);
    const Dual G = (MODE == PRHF_KMODE_O) ? ta / (beta + h) : -(beta + h);      // s beta - h
    const Dual D = a + G;
    const Dual N = G + a * a;
    const Dual w = dual(1.0) / dual_sqrt(N * D);
    const Dual v = t * (1.0 - 0.5 * a);                        // t (1 + X) / 2
    const Dual Sp1 = 1.0 + sgn * (v / beta);
    const Dual Nw = N * w;
    const Dual q = 1.0 - Nw * Nw;                              // 1 - mu^2
    const Dual U = Sp1 * q + (D - X);
    // (mu^2 = N / D; with D, N > 0 it exceeds 1 exactly where a < 0: X > 1 on a grid collapsed onto level 0 below the
    //  gyrofrequency - the reference makes such a term NaN, library.py:238)
    *ok = D.v > 0.0 && N.v * D.v > 0.0 && a.v >= 0.0;
    return w * U;
}

// np.interp's bracket of 1.0 in the running maximum (reflection_height's rules, library.py:388-407) with what the
// derivative needs besides the height: kstar = j + 1 (first level above the cutoff), jm (first level that attains the
// running maximum at level j) and the two values r_j, r_j+1.  moves: h depends on the density (a proper bracket).
// pf2: f_N^2 per level in X mode, its running maximum in O mode.  Wave-uniform results.
struct VjpBracket {
    double h, rj, rj1;
    int kstar, jm, moves;
};
template <int MODE>
__device__ __forceinline__ bool vjp_bracket(const Node* __restrict__ nodes, const double* __restrict__ pf2,
                                            const double* __restrict__ gb, int K, double f_hz, double f2, int lane,
                                            VjpBracket* out) {
#pragma clang fp contract(off)
    int kstar = K;
    for (int base = 0; base < K; base += 64) {
        const int k = base + lane;
        double col = -__builtin_inf();
        if (k < K) col = (MODE == PRHF_KMODE_O) ? pf2[k] / f2 : pf2[k] / f2 + gb[k] / f_hz;      // :136, :157, :389
        const unsigned long long hit = __ballot(col > 1.0);
        if (hit) {
            kstar = base + __ffsll((long long)hit) - 1;
            break;
        }
    }
    kstar = uniform(kstar);
    // running maximum below kstar and the first level that attains it
    double best = -__builtin_inf();
    int arg = 0x7fffffff;
    for (int k = lane; k < kstar; k += 64) {
        const double col = (MODE == PRHF_KMODE_O) ? pf2[k] / f2 : pf2[k] / f2 + gb[k] / f_hz;
        if (col > best) { best = col; arg = k; }
    }
    {
        double v0, v1;
        int i0, i1;
        halves(best, &v0, &v1);
        halves(arg, &i0, &i1);
        const bool second = v1 > v0 || (v1 == v0 && i1 < i0);
        best = second ? v1 : v0;
        arg = second ? i1 : i0;
#define PRHF_VJP_ARGMAX(OFF) do {                                                   \
            const double ov = lane_xor<OFF>(best);                                  \
            const int oi = lane_xor<OFF>(arg);                                      \
            if (ov > best || (ov == best && oi < arg)) { best = ov; arg = oi; }     \
        } while (0)
        PRHF_VJP_ARGMAX(16); PRHF_VJP_ARGMAX(8); PRHF_VJP_ARGMAX(4); PRHF_VJP_ARGMAX(2); PRHF_VJP_ARGMAX(1);
#undef PRHF_VJP_ARGMAX
    }
    best = uniform(best);
    arg = uniform(arg);
    out->kstar = kstar;
    out->jm = -1;
    out->moves = 0;
    out->rj = best;
    out->rj1 = 0.0;
    double h;
    if (kstar == K) {
        if (!(best >= 1.0)) return false;                      // never reaches the cutoff (:399)
        h = nodes[K - 1].alt;
    } else if (kstar == 0) {
        h = nodes[0].alt;                                      // left clamp
    } else {
        const int j = kstar - 1;
        const double aj = nodes[j].alt;
        if (best == 1.0) {
            h = aj;
        } else {
            const double col_star = uniform((MODE == PRHF_KMODE_O) ? pf2[kstar] / f2 : pf2[kstar] / f2 + gb[kstar] / f_hz);
            const double slope = (nodes[j + 1].alt - aj) / (col_star - best);
            h = slope * (1.0 - best) + aj;
            out->rj1 = col_star;
            out->jm = arg;
            out->moves = 1;
        }
    }
    out->h = h - kBackoff;                                     // :407
    return true;
}

// One grid point of a reflecting pair, shared by the Jacobian, VJP and JVP kernels: point i of the stretched grid below
// H = h - alt_0, its segment, and mu' with its two tangents there.
//   GX    D_i (dmu'/dX)_i cX, 0 where the reference's sum skips the term
//   term  mu'_i D_i, the point's share of the virtual height
//   sh    its share of S_H
//   msd   m_i sden_i: dX of the node per unit of dH;  tt: the interpolation weight of level s + 1
struct VjpPoint {
    double GX, term, sh, msd, tt;
    int s;
    bool active;
};
template <int MODE>
__device__ __forceinline__ VjpPoint vjp_point(const double* __restrict__ mult, int n, int i, double H, double a0, double cX,
                                              double cY, const Node* nodes, const unsigned short* hint,
                                              const BlockInfo& info, int K) {
#pragma clang fp contract(off)
    const bool active = i < n;
    const double m = active ? mult[i] : 0.0;
    const bool last = i + 1 >= n;
    const double m1 = last ? m : mult[i + 1];
    const double z = m * H + a0;                               // :413
    const double dist = !active ? 0.0 : (last ? kBackoff : (m1 * H + a0) - z);   // :415-416
    const double wgt = m1 - m;
    int s = guess_segment(hint, info, z);                      // np.interp's segment, at most K - 2
    if (s > K - 2) s = K > 1 ? K - 2 : 0;
    while (s > 0 && z < nodes[s].alt) --s;
    while (s + 2 < K && z >= nodes[s + 1].alt) ++s;
    const Node nd = nodes[s];
    double dz = z > a0 ? z - nd.alt : 0.0;
    const bool inside = dz > 0.0 && K > 1;
    if (!inside) dz = 0.0;
    const double seg_len = nodes[s + 1].alt - nd.alt;          // (level K is the +inf sentinel)
    const double sden = inside ? nd.sden : 0.0, sb = inside ? nd.sb : 0.0, sp = inside ? nd.spsi : 0.0;
    const double tt = inside ? dz / seg_len : 0.0;
    const double den = sden * dz + nd.den;
    const Dual X = Dual{cX * den, 1.0, 0.0};
    Dual mup;
    bool ok;
    if (info.unmag) {
        const Dual am = 1.0 - X;                               // :201-207 as mu' = (1 - X)^-1/2
        mup = dual(1.0) / dual_sqrt(am);
        ok = am.v > 0.0;
    } else {
        const double Y = cY * (sb * dz + nd.b);
        const double psi = (sp * dz + nd.psi) * kDegToRad;
        double sn, cs;
        sincos(psi, &sn, &cs);
        const double s2p = 2.0 * (sn * cs) * (sp * kDegToRad);
        const Dual Y2 = Dual{Y * Y, 0.0, 2.0 * Y * (cY * sb)};
        const Dual S2 = Dual{sn * sn, 0.0, s2p};
        const Dual C2 = Dual{cs * cs, 0.0, -s2p};
        mup = group_index_dual<MODE>(X, Y2, S2, C2, &ok);
    }
    const double inf = __builtin_inf();
    ok = ok && active && __builtin_fabs(mup.v) < inf && __builtin_fabs(mup.a) < inf && __builtin_fabs(mup.b) < inf;
    // (a NaN term is skipped by the reference's nansum, :288: a constant)
    VjpPoint pt;
    pt.GX = ok ? dist * mup.a * cX : 0.0;
    pt.term = ok ? mup.v * dist : 0.0;
    pt.sh = (ok ? mup.v * wgt : 0.0) + (ok ? dist * m * mup.b : 0.0);
    pt.msd = m * sden;
    pt.tt = tt;
    pt.s = s;
    pt.active = active;
    return pt;
}

// Dynamic LDS: the staged profile of the operator's kernels (nodes, f_N^2, g_p |B|), the hint table, the reduction
// scratch, then `rows` rows of lds_levels doubles for each of the `waves` waves that take frequencies
// (vjp_lds_bytes, prhf_kernels.h).  JAC: one row per wave - the Jacobian row of the wave's current frequency, written
// out and cleared after each.  VJP: two - that row, and the wave's sum of g[p, f] * row over its frequencies.
template <int MODE, bool JAC>
__device__ __forceinline__ void vjp_body(const VjpArgs& a) {
#pragma clang fp contract(off)
    constexpr int THREADS = PRHF_VJP_THREADS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int L = (int)a.lds_levels;
    Node* nodes = reinterpret_cast<Node*>(smem);
    double* pf2 = reinterpret_cast<double*>(smem + (size_t)(L + 1) * sizeof(Node));
    double* gb = pf2 + L;
    unsigned short* hint = reinterpret_cast<unsigned short*>(gb + L);
    double* red = reinterpret_cast<double*>(hint + kHintBuckets);
    double* rows = red + PRHF_RED_DOUBLES;
    constexpr int R = JAC ? 1 : 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = a.waves;
    const long long p = blockIdx.x;
    const int n_alt = (int)a.n_alt, n_freq = (int)a.n_freq, n = a.n_points;

    for (int i = tid; i < W * R * L; i += THREADS) rows[i] = 0.0;
    BlockInfo info = stage_profile<0, THREADS>(
        a.den + p * a.prof_stride, a.bmag + p * a.field_stride, a.bpsi + p * a.field_stride, a.alt + p * a.alt_stride,
        a.freq, n_freq, n_alt, nodes, pf2, gb, hint, red, L);
    if (MODE == PRHF_KMODE_X && info.nan_b && !info.bad) info.bad = kNanRow;          // the whole trace is NaN (run_block)
    if (MODE == PRHF_KMODE_O && !info.bad) prefix_max_in_place<THREADS>(pf2, info.K, red);
    if (tid == 0 && info.bad) post_status(a.status, (unsigned)info.bad);
    __syncthreads();
    const int K = info.bad ? 0 : info.K;
    const double a0 = info.a0;
    double* row = rows + (size_t)wave * R * L;
    double* acc = row + L;                                     // (VJP only)

    if (wave < W) {
        for (int f = wave; f < n_freq; f += W) {
            double* jrow = JAC ? a.out + ((size_t)p * n_freq + f) * n_alt : nullptr;
            const double fm = a.freq[f];
            const double f_hz = (fm > 0.0 && fm < __builtin_inf()) ? fm * 1e6 : qnan();
            const double f2 = f_hz * f_hz;
            const double cX = (kPlasma * kPlasma) / f2;
            const double cY = kGyro / f_hz;
            VjpBracket br;
            bool has = K > 0 && f_hz == f_hz && vjp_bracket<MODE>(nodes, pf2, gb, K, f_hz, f2, lane, &br);
            double HA = 0.0, HB = 0.0;
            int jm = -1, kstar = -1;
            double total = 0.0, SH = 0.0, EA = 0.0, EB = 0.0;
            if (has) {
                if (br.moves) {
                    const int j = br.kstar - 1;
                    const double da = nodes[j + 1].alt - nodes[j].alt, dr = br.rj1 - br.rj;
                    HA = -da * (br.rj1 - 1.0) / (dr * dr) * cX;
                    HB = -da * (1.0 - br.rj) / (dr * dr) * cX;
                    jm = br.jm;
                    kstar = br.kstar;
                }
                const double H = br.h - a0;
                for (int base = 0; base < n; base += 64) {
                    const VjpPoint pt = vjp_point<MODE>(a.mult, n, base + lane, H, a0, cX, cY, nodes, hint, info, K);
                    const bool active = pt.active;
                    const int s = pt.s;
                    const double GX = pt.GX, tt = pt.tt;
                    total += pt.term;
                    SH += pt.sh;
                    // total dX of this node per unit of den at its two levels: weight + the node's own motion with h
                    const double msd = pt.msd;
                    double c_lo = 1.0 - tt, c_hi = tt;
                    if (s == jm) c_lo += msd * HA;
                    if (s + 1 == jm) c_hi += msd * HA;
                    if (s + 1 == kstar) c_hi += msd * HB;
                    if (jm >= 0 && s != jm && s + 1 != jm) EA += GX * (msd * HA);
                    if (kstar >= 0 && s + 1 != kstar) EB += GX * (msd * HB);
                    double v_lo = GX * c_lo, v_hi = GX * c_hi;
                    // sums over each run of equal segment (segments do not decrease along a trip; idle lanes: their own run)
                    const int key = active ? s : 0x7fffffff;
#pragma unroll
                    for (int off = 1; off < 64; off <<= 1) {
                        const double o_lo = __shfl_up(v_lo, off), o_hi = __shfl_up(v_hi, off);
                        const int o_key = __shfl_up(key, off);
                        if (lane >= off && o_key == key) { v_lo += o_lo; v_hi += o_hi; }
                    }
                    const int next_key = __shfl_down(key, 1);
                    const bool tail = active && (lane == 63 || next_key != key);
                    if (tail) row[s] += v_lo;                  // (one run per segment and trip: no two lanes meet)
                    wave_lds_order();                          // segment s's upper level is segment s + 1's lower one
                    if (tail && s + 1 < K) row[s + 1] += v_hi;
                }
                total = wave_sum(total);
                SH = wave_sum(SH);
                EA = wave_sum(EA);
                EB = wave_sum(EB);
                has = total != 0.0 && total == total;                          // sum == 0 -> NaN (:290)
                wave_lds_order();
                if (has && lane == 0 && jm >= 0) {
                    row[jm] += EA + SH * HA;
                    row[kstar] += EB + SH * HB;
                }
            }
            wave_lds_order();
            // a pair without a value: a row of zeros, and its upstream gradient is not read
            const double g = (!JAC && has) ? a.grad_vh[(size_t)p * n_freq + f] : 0.0;
            for (int k = lane; k < (JAC ? n_alt : K); k += 64) {
                const double v = (has && k < K) ? row[k] : 0.0;
                if (JAC) jrow[k] = v;
                else if (has) acc[k] += g * v;
                if (k < K) row[k] = 0.0;
            }
        }
    }
    if (!JAC) {
        __syncthreads();
        // the waves' rows in wave order
        for (int k = tid; k < n_alt; k += THREADS) {
            double sum = 0.0;
            if (k < K)
                for (int w = 0; w < W; ++w) sum += rows[(size_t)w * R * L + L + k];
            a.out[(size_t)p * n_alt + k] = sum;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(PRHF_VJP_THREADS) void vfo_jacobian_kernel(const VjpArgs a) {
    vjp_body<MODE, true>(a);
}
template <int MODE>
__global__ __launch_bounds__(PRHF_VJP_THREADS) void vfo_vjp_kernel(const VjpArgs a) {
    vjp_body<MODE, false>(a);
}

}  // namespace

hipError_t launch_vfo_vjp(const VjpArgs& a, bool jacobian, size_t lds_bytes, hipStream_t stream) {
    if (a.n_prof <= 0) return hipSuccess;
    if (a.waves < 1 || a.waves > PRHF_VJP_THREADS / 64 || lds_bytes < vjp_lds_bytes(a.lds_levels, a.waves, jacobian))
        return hipErrorInvalidValue;
    const void* kernel = jacobian
        ? (a.mode == PRHF_KMODE_O ? reinterpret_cast<const void*>(&vfo_jacobian_kernel<PRHF_KMODE_O>)
                                  : reinterpret_cast<const void*>(&vfo_jacobian_kernel<PRHF_KMODE_X>))
        : (a.mode == PRHF_KMODE_O ? reinterpret_cast<const void*>(&vfo_vjp_kernel<PRHF_KMODE_O>)
                                  : reinterpret_cast<const void*>(&vfo_vjp_kernel<PRHF_KMODE_X>));
    if (lds_bytes > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    void* params[] = {const_cast<VjpArgs*>(&a)};
    return hipLaunchKernel(kernel, dim3((unsigned)a.n_prof), dim3(PRHF_VJP_THREADS), params, lds_bytes, stream);
}
