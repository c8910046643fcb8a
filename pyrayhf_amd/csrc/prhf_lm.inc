// prhf_lm.inc - Levenberg-Marquardt fits of many ionograms in a reduced basis of log-density perturbations
// (DESIGN.md section 4.16): den_i(c) = den0_i exp(sum_t c_t B_t).  Included from prhf_kernels.hip after prhf_jvp.inc,
// inside namespace prhf.  One evaluation of prhf_vfo_lm_fit_f64 is four launches: lm_synth_kernel (the trial columns
// and the tangents den B_t), the operator, the JVP (dvh[i, f, t] = d vh / d c_t), lm_step_kernel (cost, normal
// equations, accept or reject, the damped step) - the rule itself is prhf_lm_step.h, which a host test program
// includes too.  No atomics; an ionogram's bits depend on its own inputs only.

namespace {

// One thread per (ionogram, level)
__global__ void __launch_bounds__(256) lm_synth_kernel(const LmSynthArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.n_iono * a.n_alt) return;
    const long long i = idx / a.n_alt, k = idx - i * a.n_alt;
    if (a.frozen && a.frozen[i] != prhf_lm::kRunning) return;     // its trial point has not moved: the rows stand
    const double* B = a.basis + i * a.basis_stride + k;
    const double* c = a.c + i * a.n_tan;
    double s = 0.0;
    for (int t = 0; t < a.n_tan; ++t) s = fma(c[t], B[(long long)t * a.n_alt], s);
    double den = a.den0[i * a.den0_stride + k] * exp(s);
    if (a.status && a.status[i] == prhf_lm::kNoData) den = qnan();
    a.den[idx] = den;
    if (a.tan)
        for (int t = 0; t < a.n_tan; ++t) a.tan[(i * a.n_tan + t) * a.n_alt + k] = den * B[(long long)t * a.n_alt];
}

// One wavefront per ionogram; lanes stride over the grid frequencies, every lane keeps its partial sums in registers,
// wave_sum adds them in its fixed order; then every lane runs the rule (the values are uniform) and lane 0 stores.
template <int NT>
__global__ void __launch_bounds__(256) lm_step_kernel(const LmStepArgs a) {
#pragma clang fp contract(off)
    using namespace prhf_lm;
    constexpr int NA = NT * (NT + 1) / 2;
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= a.n_iono) return;
    const int F = a.n_freq, k = a.k;
    if (k > 0 && uniform(a.status[i]) != kRunning) {         // frozen: it rides along, nothing of it changes
        if (a.history && lane == 0) a.history[i * a.max_iter + k] = a.cost[i];
        return;
    }
    const double* obs = a.vh_obs + i * F;
    const double* vh = a.vh_eval + i * F;
    const double* dvh = a.dvh + i * F * NT;

    double sum = 0.0, cnt = 0.0, kept = 0.0;
    for (int f = lane; f < F; f += 64) {
        if (!many_finite(obs[f])) continue;
        kept += 1.0;
        const double m = fabs(vh[f]);
        if (m == m) { sum += m; cnt += 1.0; }
    }
    sum = wave_sum(sum);
    cnt = wave_sum(cnt);
    kept = wave_sum(kept);
    const double fill = lm_fill(sum, cnt);
    Sums<NT> e;
    sums_zero(e);
    for (int f = lane; f < F; f += 64) {
        const double o = obs[f];
        if (!many_finite(o)) continue;
        double m = vh[f];
        if (!(m == m)) m = fill;
        double d[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) d[t] = dvh[(long long)f * NT + t];
        sums_add(e, d, o - m);
    }
#pragma unroll
    for (int p = 0; p < NA; ++p) e.A[p] = wave_sum(e.A[p]);
#pragma unroll
    for (int t = 0; t < NT; ++t) e.g[t] = wave_sum(e.g[t]);
    e.cost = wave_sum(e.cost);

    const Options opt = {a.max_iter, a.lambda0, a.lambda_up, a.lambda_down, a.step_max, a.ftol, a.xtol};
    State<NT> s;
    if (k == 0) {
        state_init(s, opt, a.c_eval + i * NT);
    } else {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            s.c[t] = a.c[i * NT + t];
            s.c_eval[t] = a.c_eval[i * NT + t];
        }
        s.cost = a.cost[i];
        s.lambda = a.lambda[i];
        s.status = kRunning;
        s.n_eval = a.n_eval[i];
        s.n_accept = a.n_accept[i];
    }
    const bool accept = lm_judge(s, opt, k, kept, e, a.prior);
    const bool step = s.status == kRunning;
    bool stepped = false;                                    // s.delta is this evaluation's (it is not carried in s)
    if (step) {
        if (!accept) {                                       // (k > 0: the accepted point's, from its own evaluation)
#pragma unroll
            for (int p = 0; p < NA; ++p) s.A[p] = a.A[i * NA + p];
#pragma unroll
            for (int t = 0; t < NT; ++t) s.g[t] = a.g[i * NT + t];
        }
        stepped = lm_step(s, opt);
    }

    if (accept)
        for (int f = lane; f < F; f += 64) a.vh_fit[i * F + f] = vh[f];
    else if (k == 0)                                         // no data: no trace
        for (int f = lane; f < F; f += 64) a.vh_fit[i * F + f] = qnan();
    if (lane != 0) return;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        a.c[i * NT + t] = s.c[t];
        a.c_eval[i * NT + t] = s.c_eval[t];
    }
    a.cost[i] = s.cost;
    a.lambda[i] = s.lambda;
    a.status[i] = s.status;
    a.n_eval[i] = s.n_eval;
    a.n_accept[i] = s.n_accept;
    if (accept || k == 0) {
#pragma unroll
        for (int p = 0; p < NA; ++p) a.A[i * NA + p] = s.A[p];
#pragma unroll
        for (int t = 0; t < NT; ++t) a.g[i * NT + t] = s.g[t];
    }
    if (stepped || k == 0) {                                 // else the step before stands (k = 0: zeros)
#pragma unroll
        for (int t = 0; t < NT; ++t) a.delta[i * NT + t] = s.delta[t];
    }
    if (a.history) a.history[i * a.max_iter + k] = s.cost;
    if (a.state_out) {
        double* out = a.state_out + i * (NT * NT + 2 * NT);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int u = 0; u < NT; ++u) out[t * NT + u] = (u <= t) ? s.A[t * (t + 1) / 2 + u] : s.A[u * (u + 1) / 2 + t];
            out[NT * NT + t] = s.g[t];
            if (stepped || k == 0) out[NT * NT + NT + t] = s.delta[t];
        }
    }
}

}  // namespace

hipError_t launch_lm_synth(const LmSynthArgs& a, hipStream_t stream) {
    if (a.n_tan < 1 || a.n_tan > prhf_lm::kMaxT || a.n_alt < 1 || a.n_iono < 0) return hipErrorInvalidValue;
    if (a.n_iono == 0) return hipSuccess;
    const long long blocks = (a.n_iono * a.n_alt + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lm_synth_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_lm_step(const LmStepArgs& a, hipStream_t stream) {
    if (a.n_freq < 1 || a.n_iono < 0 || a.k < 0 || a.k >= a.max_iter) return hipErrorInvalidValue;
    if (a.n_iono == 0) return hipSuccess;
    const long long blocks = (a.n_iono + 3) / 4;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(256);
    switch (a.n_tan) {
#define PRHF_LM_PICK(NT) case NT: hipLaunchKernelGGL(lm_step_kernel<NT>, grid, block, 0, stream, a); break
        PRHF_LM_PICK(1);
        PRHF_LM_PICK(2);
        PRHF_LM_PICK(3);
        PRHF_LM_PICK(4);
        PRHF_LM_PICK(5);
        PRHF_LM_PICK(6);
        PRHF_LM_PICK(7);
        PRHF_LM_PICK(8);
#undef PRHF_LM_PICK
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
