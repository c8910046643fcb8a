// prhf_lm_step.h - the Levenberg-Marquardt rule of prhf_vfo_lm_fit_f64, without HIP: the per-frequency
// additions, the accept / reject state machine and the damped Cholesky step of ONE ionogram.  lm_step_kernel
// (prhf_lm.inc) runs it on every lane of the ionogram's wavefront; tests/devtools/lm_step_host.cpp runs it on the host;
// tests/lm_rule.py restates it in NumPy.  The three agree bit for bit on the same inputs, because the arithmetic is
// fixed here completely:
//   - every operation is one IEEE float64 operation: no fused multiply-add anywhere (a * b + c is a rounded product and
//     a rounded sum; the library and the host program are built with contraction off), sqrt and / correctly rounded;
//   - sums over the tangents t run in index order; A is kept as its lower triangle, entry (t, s), s <= t, at t (t + 1) / 2 + s;
//   - sums over the frequencies: lane l of 64 adds the grid frequencies l, l + 64, l + 128, ... in that order (those of
//     K_i only), then the 64 partial sums are added pairwise: v[l] + v[l ^ 32], then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1 - the
//     tree of wave_sum (prhf_kernels.hip), restated for a host by wave_order_sum below;
//   - the prior's terms join behind the data's: cost + (w_t c_t) c_t for t = 0, 1, ...; A_tt + w_t; g_t - w_t c_t.
#ifndef PRHF_LM_STEP_H
#define PRHF_LM_STEP_H

#if defined(__HIPCC__)
#define PRHF_LM_HD __host__ __device__ __forceinline__
#else
#define PRHF_LM_HD inline
#endif
#if defined(__clang__)
#define PRHF_LM_UNROLL _Pragma("unroll")
#else
#define PRHF_LM_UNROLL
#endif

namespace prhf_lm {

// the values of PRHF_LM_* in include/prhf.h
enum Status { kRunning = 0, kConvergedF = 1, kConvergedX = 2, kSingular = 3, kNoData = 4, kNoCost = 5 };

constexpr int kMaxT = 8;             // tangents: one pass of the JVP kernel
constexpr int kRetries = 8;          // further factorisations, each with lambda * lambda_up, before kSingular
constexpr double kLambdaMin = 1e-12, kLambdaMax = 1e12;
constexpr double kTiny = 1e-30;      // floor of the damping's scale: a direction without sensitivity (A_tt = 0) is still damped

struct Options {
    int max_iter;
    double lambda0, lambda_up, lambda_down, step_max, ftol, xtol;
};

PRHF_LM_HD double lm_nan() { return __builtin_nan(""); }
PRHF_LM_HD bool lm_finite(double v) { return __builtin_fabs(v) < __builtin_inf(); }
PRHF_LM_HD double lm_clamp(double lambda) {
    return lambda < kLambdaMin ? kLambdaMin : (lambda > kLambdaMax ? kLambdaMax : lambda);    // (a NaN stays a NaN)
}
// The value that stands for a modelled NaN (residual_many_kernel's rule): the mean of |vh_model| over the kept
// frequencies where the model is finite, at least 100 km; NaN where there is none.
PRHF_LM_HD double lm_fill(double sum_abs, double count) {
    const double mean = (count > 0.0) ? sum_abs / count : lm_nan();
    return (mean == mean) ? (mean > 100.0 ? mean : 100.0) : lm_nan();
}

// What one evaluation adds up over the kept frequencies: sum d d^T (lower triangle), sum d r, sum r^2
template <int NT>
struct Sums {
    double A[NT * (NT + 1) / 2];
    double g[NT];
    double cost;
};

template <int NT>
PRHF_LM_HD void sums_zero(Sums<NT>& s) {
    PRHF_LM_UNROLL
    for (int p = 0; p < NT * (NT + 1) / 2; ++p) s.A[p] = 0.0;
    PRHF_LM_UNROLL
    for (int t = 0; t < NT; ++t) s.g[t] = 0.0;
    s.cost = 0.0;
}

// one kept frequency: its row d of dvh and its residual r
template <int NT>
PRHF_LM_HD void sums_add(Sums<NT>& s, const double* d, double r) {
    PRHF_LM_UNROLL
    for (int t = 0; t < NT; ++t) {
        PRHF_LM_UNROLL
        for (int u = 0; u <= t; ++u) s.A[t * (t + 1) / 2 + u] = s.A[t * (t + 1) / 2 + u] + d[t] * d[u];
        s.g[t] = s.g[t] + d[t] * r;
    }
    s.cost = s.cost + r * r;
}

// One ionogram between two evaluations
template <int NT>
struct State {
    double c[NT];        // the accepted point
    double c_eval[NT];   // the point the next evaluation is made at
    double A[NT * (NT + 1) / 2], g[NT];   // of the accepted point, prior included
    double delta[NT];    // the last step taken from c
    double cost;         // of the accepted point
    double lambda;
    int status, n_eval, n_accept;
};

template <int NT>
PRHF_LM_HD void state_init(State<NT>& s, const Options& o, const double* c0) {
    PRHF_LM_UNROLL
    for (int t = 0; t < NT; ++t) {
        s.c[t] = s.c_eval[t] = c0 ? c0[t] : 0.0;
        s.g[t] = s.delta[t] = 0.0;
    }
    PRHF_LM_UNROLL
    for (int p = 0; p < NT * (NT + 1) / 2; ++p) s.A[p] = 0.0;
    s.cost = lm_nan();
    s.lambda = lm_clamp(o.lambda0);
    s.status = kRunning;
    s.n_eval = s.n_accept = 0;
}

// Evaluation k has been made at s.c_eval: e holds the data's sums there, n_kept = |K_i|, w the prior's weights or null.
// Accepts or rejects the point (s.c, s.cost, s.lambda; on acceptance s.A and s.g, which are not read here) and sets a
// final status where the rule ends.  Returns whether the point was accepted: the caller then keeps the trace.  The
// caller goes on with lm_step while s.status is kRunning - after restoring s.A and s.g where it left them elsewhere.
template <int NT>
PRHF_LM_HD bool lm_judge(State<NT>& s, const Options& o, int k, double n_kept, const Sums<NT>& e, const double* w) {
    s.n_eval = k + 1;
    if (!(n_kept > 0.0)) {                  // nothing to fit: c stays c0
        s.status = kNoData;
        s.cost = lm_nan();
        return false;
    }
    double cost_eval = e.cost;
    if (w) {
        PRHF_LM_UNROLL
        for (int t = 0; t < NT; ++t) cost_eval = cost_eval + (w[t] * s.c_eval[t]) * s.c_eval[t];
    }
    const double cost_prev = s.cost;
    bool accept = true;
    if (k > 0) {
        accept = cost_eval < cost_prev;     // strictly; a cost that is not finite is rejected
        s.lambda = lm_clamp(accept ? s.lambda / o.lambda_down : s.lambda * o.lambda_up);
    }
    if (accept) {
        ++s.n_accept;
        s.cost = cost_eval;
        PRHF_LM_UNROLL
        for (int t = 0; t < NT; ++t) s.c[t] = s.c_eval[t];
        PRHF_LM_UNROLL
        for (int p = 0; p < NT * (NT + 1) / 2; ++p) s.A[p] = e.A[p];
        PRHF_LM_UNROLL
        for (int t = 0; t < NT; ++t) {
            s.g[t] = e.g[t];
            if (w) {
                s.A[t * (t + 1) / 2 + t] = s.A[t * (t + 1) / 2 + t] + w[t];
                s.g[t] = s.g[t] - w[t] * s.c[t];
            }
        }
    }
    if (k == 0 && !lm_finite(s.cost)) {
        s.status = kNoCost;
        return true;
    }
    if (k > 0 && accept && cost_prev - s.cost <= o.ftol * cost_prev) s.status = kConvergedF;
    return accept;
}

// The damped step from the accepted point: (A + lambda diag(max(A_tt, kTiny))) delta = g by Cholesky (lower triangle,
// column by column, the subtractions in index order; forward then backward substitution), lambda raised while a pivot is
// not positive; delta scaled to max |delta_t| <= step_max; then the xtol test, or the next trial point.  Returns whether
// s.delta was set: where the rule ends with kSingular it keeps the step before (a caller that does not carry s.delta
// from one evaluation to the next leaves its stored copy alone then).
template <int NT>
PRHF_LM_HD bool lm_step(State<NT>& s, const Options& o) {
    double L[NT * (NT + 1) / 2];
    bool ok = false;
    for (int attempt = 0; attempt <= kRetries && !ok; ++attempt) {
        if (attempt > 0) s.lambda = lm_clamp(s.lambda * o.lambda_up);
        ok = true;
        PRHF_LM_UNROLL
        for (int j = 0; j < NT; ++j) {
            const double ajj = s.A[j * (j + 1) / 2 + j];
            double v = ajj + s.lambda * (ajj > kTiny ? ajj : kTiny);
            PRHF_LM_UNROLL
            for (int m = 0; m < j; ++m) v = v - L[j * (j + 1) / 2 + m] * L[j * (j + 1) / 2 + m];
            if (!(v > 0.0)) ok = false;                    // (also a NaN; the rest of this attempt is not used)
            const double ljj = __builtin_sqrt(v);
            L[j * (j + 1) / 2 + j] = ljj;
            PRHF_LM_UNROLL
            for (int i = j + 1; i < NT; ++i) {
                double u = s.A[i * (i + 1) / 2 + j];
                PRHF_LM_UNROLL
                for (int m = 0; m < j; ++m) u = u - L[i * (i + 1) / 2 + m] * L[j * (j + 1) / 2 + m];
                L[i * (i + 1) / 2 + j] = u / ljj;
            }
        }
    }
    if (!ok) {
        s.status = kSingular;
        return false;
    }
    double y[NT], d[NT];
    PRHF_LM_UNROLL
    for (int i = 0; i < NT; ++i) {
        double v = s.g[i];
        PRHF_LM_UNROLL
        for (int m = 0; m < i; ++m) v = v - L[i * (i + 1) / 2 + m] * y[m];
        y[i] = v / L[i * (i + 1) / 2 + i];
    }
    PRHF_LM_UNROLL
    for (int i = NT - 1; i >= 0; --i) {
        double v = y[i];
        PRHF_LM_UNROLL
        for (int m = i + 1; m < NT; ++m) v = v - L[m * (m + 1) / 2 + i] * d[m];
        d[i] = v / L[i * (i + 1) / 2 + i];
    }
    double dmax = 0.0, cmax = 0.0;
    bool bad = false;
    PRHF_LM_UNROLL
    for (int t = 0; t < NT; ++t) {
        const double ad = __builtin_fabs(d[t]), ac = __builtin_fabs(s.c[t]);
        if (ad > dmax) dmax = ad;
        if (!(ad == ad)) bad = true;
        if (ac > cmax) cmax = ac;
    }
    if (bad || !lm_finite(dmax)) {                         // a step that is not a number: nothing to go on with
        s.status = kSingular;
        return false;
    }
    if (dmax > o.step_max) {
        const double scale = o.step_max / dmax;
        PRHF_LM_UNROLL
        for (int t = 0; t < NT; ++t) d[t] = d[t] * scale;
        dmax = o.step_max;
    }
    PRHF_LM_UNROLL
    for (int t = 0; t < NT; ++t) s.delta[t] = d[t];
    if (dmax <= o.xtol * (cmax + o.xtol)) {
        s.status = kConvergedX;
        return true;
    }
    PRHF_LM_UNROLL
    for (int t = 0; t < NT; ++t) s.c_eval[t] = s.c[t] + s.delta[t];
    return true;
}

#if !defined(__HIPCC__)
// ---- For a host: the wavefront's order of additions, and one whole evaluation of one ionogram ----

// the sum of 64 lane values in wave_sum's order
inline double wave_order_sum(const double* lanes) {
    double v[64], n[64];
    for (int l = 0; l < 64; ++l) v[l] = lanes[l];
    for (int off = 32; off >= 1; off >>= 1) {
        for (int l = 0; l < 64; ++l) n[l] = v[l] + v[l ^ off];
        for (int l = 0; l < 64; ++l) v[l] = n[l];
    }
    return v[0];
}

// lm_step_kernel's sums for one ionogram: vh_obs, vh_model (n_freq), dvh (n_freq, NT).  Returns |K_i|.
template <int NT>
inline double eval_sums(int n_freq, const double* vh_obs, const double* vh_model, const double* dvh, Sums<NT>& out) {
    double sum[64], cnt[64], kept[64];
    for (int l = 0; l < 64; ++l) {
        sum[l] = cnt[l] = kept[l] = 0.0;
        for (int f = l; f < n_freq; f += 64) {
            if (!lm_finite(vh_obs[f])) continue;
            kept[l] = kept[l] + 1.0;
            const double m = __builtin_fabs(vh_model[f]);
            if (m == m) { sum[l] = sum[l] + m; cnt[l] = cnt[l] + 1.0; }
        }
    }
    const double fill = lm_fill(wave_order_sum(sum), wave_order_sum(cnt));
    static Sums<NT> lane[64];                              // (a test program: one thread)
    for (int l = 0; l < 64; ++l) {
        sums_zero(lane[l]);
        for (int f = l; f < n_freq; f += 64) {
            if (!lm_finite(vh_obs[f])) continue;
            double m = vh_model[f];
            if (!(m == m)) m = fill;
            sums_add(lane[l], dvh + (long long)f * NT, vh_obs[f] - m);
        }
    }
    double col[64];
    for (int p = 0; p < NT * (NT + 1) / 2; ++p) {
        for (int l = 0; l < 64; ++l) col[l] = lane[l].A[p];
        out.A[p] = wave_order_sum(col);
    }
    for (int t = 0; t < NT; ++t) {
        for (int l = 0; l < 64; ++l) col[l] = lane[l].g[t];
        out.g[t] = wave_order_sum(col);
    }
    for (int l = 0; l < 64; ++l) col[l] = lane[l].cost;
    out.cost = wave_order_sum(col);
    return wave_order_sum(kept);
}
#endif

}  // namespace prhf_lm

#endif
