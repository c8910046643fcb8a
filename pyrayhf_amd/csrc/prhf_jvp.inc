// prhf_jvp.inc - the Jacobian-vector product of the vertical forward operator (DESIGN.md section 4.15): the
// tangent-linear operator dvh[p, f, t] = sum_k J[p, f, k] tan[p, t, k], J the matrix of prhf_vjp.inc, formed per grid
// point without its rows.  Included from prhf_kernels.hip after prhf_vjp.inc, inside namespace prhf.
//
// With dH_t = HA tan_t[jm] + HB tan_t[kstar] the motion of the reflection height along tangent t (once per pair; 0 where
// the bracket does not move), a grid point in segment s sees
//   dX_t = (1 - tt) tan_t[s] + tt tan_t[s + 1] + m_i sden_i dH_t         (the node's total dX, formed before dmu'/dX)
// and  dvh_t = sum_i GX_i dX_t + S_H dH_t.  The point's evaluation, the bracket and the staging are the VJP's
// (vjp_point, vjp_bracket, stage_profile); what a tangent adds per point is two LDS reads and three multiply-adds.
//
// One workgroup of THREADS (256, or 512 where there are frequencies for more than four waves: plan_jvp) per profile, waves
// take frequencies, lanes take grid points, NT accumulators per lane.  The tangent
// columns of the launch lie in LDS behind the reduction scratch, level-major (tans[k * NT + t]): the 2 NT words a point
// reads are contiguous.  Only levels below the density peak are staged or read.  Every addition's order is fixed by
// (profile, n_points): per lane over the trips, then wave_sum - the bits of a column depend on nothing else.

namespace {

template <int MODE, int NT, int THREADS>
__global__ __launch_bounds__(THREADS) void vfo_jvp_kernel(const JvpArgs a) {
#pragma clang fp contract(off)
    constexpr int W = THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int L = (int)a.lds_levels;
    Node* nodes = reinterpret_cast<Node*>(smem);
    double* pf2 = reinterpret_cast<double*>(smem + (size_t)(L + 1) * sizeof(Node));
    double* gb = pf2 + L;
    unsigned short* hint = reinterpret_cast<unsigned short*>(gb + L);
    double* red = reinterpret_cast<double*>(hint + kHintBuckets);
    double* tans = red + PRHF_RED_DOUBLES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long p = blockIdx.x;
    const int n_alt = (int)a.n_alt, n_freq = (int)a.n_freq, n = a.n_points;

    BlockInfo info = stage_profile<0, THREADS>(
        a.den + p * a.prof_stride, a.bmag + p * a.field_stride, a.bpsi + p * a.field_stride, a.alt + p * a.alt_stride,
        a.freq, n_freq, n_alt, nodes, pf2, gb, hint, red, L);
    if (MODE == PRHF_KMODE_X && info.nan_b && !info.bad) info.bad = kNanRow;          // the whole trace is NaN (run_block)
    if (MODE == PRHF_KMODE_O && !info.bad) prefix_max_in_place<THREADS>(pf2, info.K, red);
    if (tid == 0 && info.bad) post_status(a.status, (unsigned)info.bad);
    const int K = info.bad ? 0 : info.K;               // (K < L: stage_profile refuses a peak at or above the capacity)
    {
        const double* tg = a.tan + p * a.tan_prof_stride;
#pragma unroll
        for (int t = 0; t < NT; ++t)
            for (int k = tid; k < K; k += THREADS) tans[k * NT + t] = t < a.n_tan ? tg[(size_t)t * n_alt + k] : 0.0;
    }
    __syncthreads();
    const double a0 = info.a0;

    for (int f = wave; f < n_freq; f += W) {
        const double fm = a.freq[f];
        const double f_hz = (fm > 0.0 && fm < __builtin_inf()) ? fm * 1e6 : qnan();
        const double f2 = f_hz * f_hz;
        const double cX = (kPlasma * kPlasma) / f2;
        const double cY = kGyro / f_hz;
        VjpBracket br;
        bool has = K > 0 && f_hz == f_hz && vjp_bracket<MODE>(nodes, pf2, gb, K, f_hz, f2, lane, &br);
        double dH[NT], acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) dH[t] = acc[t] = 0.0;
        double total = 0.0, SH = 0.0;
        double mine = 0.0;                             // lane t keeps tangent t's result and writes it
        if (has) {
            if (br.moves) {
                const int j = br.kstar - 1;
                const double da = nodes[j + 1].alt - nodes[j].alt, dr = br.rj1 - br.rj;
                const double HA = -da * (br.rj1 - 1.0) / (dr * dr) * cX;
                const double HB = -da * (1.0 - br.rj) / (dr * dr) * cX;
#pragma unroll
                for (int t = 0; t < NT; ++t) dH[t] = uniform(HA * tans[br.jm * NT + t] + HB * tans[br.kstar * NT + t]);
            }
            const double H = br.h - a0;
            for (int base = 0; base < n; base += 64) {
                const VjpPoint pt = vjp_point<MODE>(a.mult, n, base + lane, H, a0, cX, cY, nodes, hint, info, K);
                total += pt.term;
                SH += pt.sh;
                const double* tp = tans + pt.s * NT;
                const bool upper = pt.s + 1 < K;           // (a one-level bottomside has no level above its segment)
                const double w_lo = 1.0 - pt.tt;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const double lo = tp[t], hi = upper ? tp[NT + t] : 0.0;
                    const double dX = (w_lo * lo + pt.tt * hi) + pt.msd * dH[t];
                    acc[t] += pt.GX * dX;
                }
            }
            total = wave_sum(total);
            SH = wave_sum(SH);
            // sum == 0 -> NaN (:290): a pair without a value keeps zeros, as its Jacobian row
            if (total != 0.0 && total == total) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const double v = wave_sum(acc[t]) + (br.moves ? SH * dH[t] : 0.0);
                    if (lane == t) mine = v;
                }
            }
        }
        if (lane < a.n_tan) a.out[((size_t)p * n_freq + f) * a.out_stride + lane] = mine;
    }
}

}  // namespace

hipError_t launch_vfo_jvp(const JvpArgs& a, int nt, int threads, size_t lds_bytes, hipStream_t stream) {
    if (a.n_prof <= 0 || a.n_tan <= 0) return hipSuccess;
    if (a.n_tan > nt || lds_bytes < jvp_lds_bytes(a.lds_levels, nt)) return hipErrorInvalidValue;
    if (threads != PRHF_VJP_THREADS && threads != PRHF_JVP_THREADS_WIDE) return hipErrorInvalidValue;
    const bool o = a.mode == PRHF_KMODE_O, wide = threads == PRHF_JVP_THREADS_WIDE;
    const void* kernel = nullptr;
#define PRHF_JVP_KERNEL(M, NT, T) reinterpret_cast<const void*>(&vfo_jvp_kernel<M, NT, T>)
#define PRHF_JVP_PICK(NT)                                                                                                      \
    case NT:                                                                                                                   \
        kernel = wide ? (o ? PRHF_JVP_KERNEL(PRHF_KMODE_O, NT, PRHF_JVP_THREADS_WIDE) : PRHF_JVP_KERNEL(PRHF_KMODE_X, NT, PRHF_JVP_THREADS_WIDE)) \
                      : (o ? PRHF_JVP_KERNEL(PRHF_KMODE_O, NT, PRHF_VJP_THREADS) : PRHF_JVP_KERNEL(PRHF_KMODE_X, NT, PRHF_VJP_THREADS));         \
        break
    switch (nt) {
        PRHF_JVP_PICK(1);
        PRHF_JVP_PICK(2);
        PRHF_JVP_PICK(4);
        PRHF_JVP_PICK(8);
        default: return hipErrorInvalidValue;
    }
#undef PRHF_JVP_PICK
#undef PRHF_JVP_KERNEL
    if (lds_bytes > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    void* params[] = {const_cast<JvpArgs*>(&a)};
    return hipLaunchKernel(kernel, dim3((unsigned)a.n_prof), dim3((unsigned)threads), params, lds_bytes, stream);
}
