// The launch planning of the Jacobian / VJP kernels (pyrayhf_amd/csrc/prhf_plan.h, plan_vjp - the very code
// prhf_api.cpp compiles) on the host, without a GPU (tests/test_jacobian_host.py).  Stand-alone: builds with g++ alone,
// also under -fsanitize=address,undefined.
//   vjp_plan_host check                              invariants over a table of shapes; prints "vjp_plan_host: ok"
//   vjp_plan_host plan n_prof n_freq levels jac      prints "blocks threads waves lds_bytes", or "refused: <message>"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "prhf_plan.h"

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); \
                                             std::printf("\n"); ++failures; } } while (0)

static void check() {
    char why[256];
    VjpPlan pl;
    for (int jac = 0; jac < 2; ++jac) {
        const long long most1 = vjp_max_levels(jac != 0, 1), most4 = vjp_max_levels(jac != 0, 4);
        EXPECT(most4 < most1, "four waves' rows must need more room than one's");
        EXPECT(prhf::vjp_lds_bytes(most1, 1, jac != 0) <= kLdsFull && prhf::vjp_lds_bytes(most1 + 1, 1, jac != 0) > kLdsFull,
               "vjp_max_levels(1) = %lld is not the last level count that fits", most1);
        for (long long levels : {1LL, 2LL, 20LL, 78LL, 620LL, most4, most4 + 1, most1, most1 + 1, 1400LL, 3000LL, 65535LL})
            for (long long n_freq : {1LL, 2LL, 3LL, 4LL, 65LL, 174LL, 1LL << 20})
                for (long long n_prof : {0LL, 1LL, 3LL, 12500LL}) {
                    why[0] = 0;
                    const int rc = plan_vjp(n_prof, n_freq, levels, jac != 0, pl, why, sizeof why);
                    if (levels > most1) {
                        EXPECT(rc == PRHF_EINVAL && std::strstr(why, "stages at most") && pl.blocks == 0 && pl.lds_bytes == 0,
                               "levels %lld must be refused with the documented message, got %d '%s'", levels, rc, why);
                        continue;
                    }
                    EXPECT(rc == PRHF_OK, "levels %lld n_freq %lld refused: %s", levels, n_freq, why);
                    EXPECT(pl.blocks == n_prof && pl.threads == PRHF_VJP_THREADS, "one workgroup per profile");
                    EXPECT(pl.waves == 1 || pl.waves == 2 || pl.waves == 4, "waves %d", pl.waves);
                    EXPECT(pl.waves <= PRHF_VJP_THREADS / 64, "more frequency waves than the workgroup has");
                    EXPECT(pl.waves == 1 || pl.waves / 2 < n_freq, "idle accumulator rows: %d waves for %lld frequencies", pl.waves, n_freq);
                    EXPECT(pl.lds_bytes == prhf::vjp_lds_bytes(levels, pl.waves, jac != 0) && pl.lds_bytes <= kLdsFull,
                           "LDS %zu for %lld levels", pl.lds_bytes, levels);
                    // the rows lie behind the operator's staged arrays and must cover levels doubles per wave and row
                    EXPECT(pl.lds_bytes >= (size_t)(levels + 1) * PRHF_NODE_BYTES + (size_t)levels * 16 +
                                               (size_t)pl.waves * (jac ? 1 : 2) * (size_t)levels * 8, "rows do not fit");
                    if (n_freq >= 3 && levels <= most4) EXPECT(pl.waves == 4, "four waves where they fit (levels %lld)", levels);
                    if (levels > most4) EXPECT(pl.waves < 4, "levels %lld cannot hold four waves' rows", levels);
                }
        EXPECT(plan_vjp(1, 0, 10, jac != 0, pl, why, sizeof why) == PRHF_EINVAL, "n_freq = 0");
        EXPECT(plan_vjp(-1, 1, 10, jac != 0, pl, why, sizeof why) == PRHF_EINVAL, "n_prof < 0");
        EXPECT(plan_vjp(1, 1, 0, jac != 0, pl, why, sizeof why) == PRHF_EINVAL, "no levels");
    }
    // anchors worked out by hand from vjp_lds_bytes: 78 levels, VJP, 4 waves: 79*96 + 78*16 + 2048 + 1280 + 4*2*78*8
    EXPECT(plan_vjp(3, 5, 78, false, pl, why, sizeof why) == PRHF_OK && pl.lds_bytes == 7584 + 1248 + 2048 + 1280 + 4992,
           "78-level anchor: %zu", pl.lds_bytes);
    EXPECT(plan_vjp(3, 5, 620, true, pl, why, sizeof why) == PRHF_OK && pl.lds_bytes == 621 * 96 + 620 * 16 + 2048 + 1280 + 4 * 620 * 8,
           "620-level Jacobian anchor: %zu", pl.lds_bytes);
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::strcmp(argv[1], "check") == 0) {
        check();
        if (failures) return 1;
        std::printf("vjp_plan_host: ok\n");
        return 0;
    }
    if (argc == 6 && std::strcmp(argv[1], "plan") == 0) {
        VjpPlan pl;
        char why[256];
        if (plan_vjp(std::atoll(argv[2]), std::atoll(argv[3]), std::atoll(argv[4]), std::atoi(argv[5]) != 0, pl, why, sizeof why) != PRHF_OK) {
            std::printf("refused: %s\n", why);
            return 0;
        }
        std::printf("%lld %d %d %zu\n", pl.blocks, pl.threads, pl.waves, pl.lds_bytes);
        return 0;
    }
    std::fprintf(stderr, "usage: vjp_plan_host check | plan n_prof n_freq levels jacobian\n");
    return 2;
}
