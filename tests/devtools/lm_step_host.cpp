// lm_step_host.cpp - the Levenberg-Marquardt rule of pyrayhf_amd/csrc/prhf_lm_step.h on a host, without HIP or Python
// (tests/test_lm_fit_host.py builds it with g++ -fsanitize=address,undefined and compares its output, bit for bit,
// with tests/lm_rule.py).  The model is linear: vh(c) = vh0 + D c, added in index order, dvh = D.
//
//   lm_step_host CASES.bin
// CASES.bin, float64: n_cases, T, F, max_iter, lambda0, lambda_up, lambda_down, step_max, ftol, xtol, has_prior; then
// per case vh_obs (F), vh0 (F), D (F, T), c0 (T), w (T).  Output, per case and evaluation, one line of 64-bit patterns in
// hex: c (T), c_eval (T), cost, lambda, then the status in decimal; per case a last line "end status n_eval n_accept"
// with A (T, T, from the lower triangle), g (T) and delta (T) behind it.

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "prhf_lm_step.h"

namespace {

unsigned long long bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return (unsigned long long)u;
}

template <int NT>
int run_case(int F, const prhf_lm::Options& o, const double* obs, const double* vh0, const double* D, const double* c0,
             const double* w) {
    using namespace prhf_lm;
    State<NT> s;
    state_init(s, o, c0);
    std::vector<double> vh((size_t)F);
    for (int k = 0; k < o.max_iter; ++k) {
        if (s.status == kRunning) {
            for (int f = 0; f < F; ++f) {
                double v = vh0[f];
                for (int t = 0; t < NT; ++t) v = v + D[(size_t)f * NT + t] * s.c_eval[t];
                vh[(size_t)f] = v;
            }
            Sums<NT> e;
            const double n_kept = eval_sums<NT>(F, obs, vh.data(), D, e);
            lm_judge(s, o, k, n_kept, e, w);
            if (s.status == kRunning) lm_step(s, o);
        }
        for (int t = 0; t < NT; ++t) std::printf("%016llx ", bits(s.c[t]));
        for (int t = 0; t < NT; ++t) std::printf("%016llx ", bits(s.c_eval[t]));
        std::printf("%016llx %016llx %d\n", bits(s.cost), bits(s.lambda), s.status);
    }
    std::printf("end %d %d %d", s.status, s.n_eval, s.n_accept);
    for (int t = 0; t < NT; ++t)
        for (int u = 0; u < NT; ++u) std::printf(" %016llx", bits(u <= t ? s.A[t * (t + 1) / 2 + u] : s.A[u * (u + 1) / 2 + t]));
    for (int t = 0; t < NT; ++t) std::printf(" %016llx", bits(s.g[t]));
    for (int t = 0; t < NT; ++t) std::printf(" %016llx", bits(s.delta[t]));
    std::printf("\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: lm_step_host CASES.bin\n");
        return 2;
    }
    std::FILE* fp = std::fopen(argv[1], "rb");
    if (!fp) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    std::vector<double> in;
    double buf[512];
    size_t n;
    while ((n = std::fread(buf, 8, 512, fp)) > 0) in.insert(in.end(), buf, buf + n);
    std::fclose(fp);
    if (in.size() < 11) {
        std::fprintf(stderr, "short header\n");
        return 2;
    }
    const int n_cases = (int)in[0], T = (int)in[1], F = (int)in[2];
    const prhf_lm::Options o = {(int)in[3], in[4], in[5], in[6], in[7], in[8], in[9]};
    const bool has_prior = in[10] != 0.0;
    if (n_cases < 0 || T < 1 || T > prhf_lm::kMaxT || F < 1 || o.max_iter < 1) {
        std::fprintf(stderr, "bad header\n");
        return 2;
    }
    const size_t per_case = (size_t)F * 2 + (size_t)F * (size_t)T + 2 * (size_t)T;
    if (in.size() != 11 + (size_t)n_cases * per_case) {
        std::fprintf(stderr, "bad length\n");
        return 2;
    }
    for (int q = 0; q < n_cases; ++q) {
        const double* p = in.data() + 11 + (size_t)q * per_case;
        const double *obs = p, *vh0 = p + F, *D = p + 2 * (size_t)F, *c0 = D + (size_t)F * (size_t)T, *w = c0 + T;
        const double* prior = has_prior ? w : nullptr;
        switch (T) {
            case 1: run_case<1>(F, o, obs, vh0, D, c0, prior); break;
            case 2: run_case<2>(F, o, obs, vh0, D, c0, prior); break;
            case 3: run_case<3>(F, o, obs, vh0, D, c0, prior); break;
            case 4: run_case<4>(F, o, obs, vh0, D, c0, prior); break;
            case 5: run_case<5>(F, o, obs, vh0, D, c0, prior); break;
            case 6: run_case<6>(F, o, obs, vh0, D, c0, prior); break;
            case 7: run_case<7>(F, o, obs, vh0, D, c0, prior); break;
            default: run_case<8>(F, o, obs, vh0, D, c0, prior); break;
        }
    }
    return 0;
}
