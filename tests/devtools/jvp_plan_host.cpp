// The launch planning of the JVP kernel (pyrayhf_amd/csrc/prhf_plan.h, plan_jvp and jvp_chunk - the very code
// prhf_api.cpp compiles) on the host, without a GPU (tests/test_jvp_host.py).  Stand-alone: builds with g++ alone,
// also under -fsanitize=address,undefined.
//   jvp_plan_host check                              invariants over every shape below; prints "jvp_plan_host: ok"
//   jvp_plan_host plan n_prof n_freq levels n_tan    prints "blocks threads waves chunk n_chunks" and one line
//                                                    "first count nt lds_bytes" per launch, or "refused: <message>"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "prhf_plan.h"

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); \
                                             std::printf("\n"); ++failures; } } while (0)

static void check() {
    char why[256];
    JvpPlan pl;
    const long long limit = jvp_max_levels(1), most8 = jvp_max_levels(PRHF_JVP_MAX_NT);
    EXPECT(most8 < limit, "eight columns must need more room than one");
    EXPECT(prhf::jvp_lds_bytes(limit, 1) <= kLdsFull && prhf::jvp_lds_bytes(limit + 1, 1) > kLdsFull,
           "jvp_max_levels(1) = %lld is not the last level count that fits", limit);
    // the figures the header, the docstring and DESIGN.md state
    EXPECT(limit == 1332 && most8 == 908, "documented limits 1332 / 908, computed %lld / %lld", limit, most8);
    for (long long levels = 1; levels <= limit + 1; ++levels)
        for (long long n_freq = 1; n_freq <= 9; ++n_freq)
            for (long long n_tan : {1LL, 2LL, 3LL, 8LL, 9LL, 64LL}) {
                why[0] = 0;
                const int rc = plan_jvp(3, n_freq, levels, n_tan, pl, why, sizeof why);
                if (levels > limit) {
                    EXPECT(rc == PRHF_EINVAL && std::strstr(why, "stages at most") && pl.blocks == 0 && pl.n_chunks == 0,
                           "levels %lld must be refused with the documented message, got %d '%s'", levels, rc, why);
                    continue;
                }
                EXPECT(rc == PRHF_OK, "levels %lld n_freq %lld n_tan %lld refused: %s", levels, n_freq, n_tan, why);
                EXPECT(pl.blocks == 3 && pl.threads == (n_freq > 4 ? PRHF_JVP_THREADS_WIDE : PRHF_VJP_THREADS),
                       "one workgroup per profile, eight waves where more than four get a frequency: %d threads", pl.threads);
                EXPECT(pl.waves >= 1 && pl.waves == std::min<long long>(pl.threads / 64, n_freq), "waves %d", pl.waves);
                EXPECT(pl.chunk == 1 || pl.chunk == 2 || pl.chunk == 4 || pl.chunk == 8, "chunk %d", pl.chunk);
                EXPECT(pl.chunk == 1 || pl.chunk / 2 < n_tan, "chunk %d for %lld tangents", pl.chunk, n_tan);
                if (levels <= most8 && n_tan >= 8) EXPECT(pl.chunk == 8, "eight at a time where they fit (levels %lld)", levels);
                if (levels > most8) EXPECT(pl.chunk < 8, "levels %lld cannot hold eight columns", levels);
                long long covered = 0;
                for (long long i = 0; i < pl.n_chunks; ++i) {
                    const JvpChunk ch = jvp_chunk(pl, n_tan, i);
                    EXPECT(ch.first == covered && ch.count >= 1 && ch.count <= ch.nt && ch.nt <= pl.chunk, "launch %lld: first %lld count %d nt %d",
                           i, ch.first, ch.count, ch.nt);
                    EXPECT(ch.nt == 1 || ch.nt == 2 || ch.nt == 4 || ch.nt == 8, "nt %d", ch.nt);
                    EXPECT(ch.nt == 1 || ch.nt / 2 < ch.count, "nt %d for %d tangents", ch.nt, ch.count);
                    EXPECT(ch.lds_bytes == prhf::jvp_lds_bytes(levels, ch.nt) && ch.lds_bytes <= kLdsFull, "LDS %zu for %lld levels, nt %d",
                           ch.lds_bytes, levels, ch.nt);
                    // the columns lie behind the operator's staged arrays and must cover levels doubles per tangent
                    EXPECT(ch.lds_bytes >= (size_t)(levels + 1) * PRHF_NODE_BYTES + (size_t)levels * 16 + (size_t)ch.nt * (size_t)levels * 8,
                           "columns do not fit");
                    covered += ch.count;
                }
                EXPECT(covered == n_tan, "chunks cover %lld of %lld tangents", covered, n_tan);
            }
    EXPECT(plan_jvp(3, 5, 78, 0, pl, why, sizeof why) == PRHF_OK && pl.n_chunks == 0, "no tangents: no launches");
    EXPECT(plan_jvp(0, 5, 78, 3, pl, why, sizeof why) == PRHF_OK && pl.blocks == 0, "no profiles");
    EXPECT(plan_jvp(1, 0, 10, 1, pl, why, sizeof why) == PRHF_EINVAL, "n_freq = 0");
    EXPECT(plan_jvp(-1, 1, 10, 1, pl, why, sizeof why) == PRHF_EINVAL, "n_prof < 0");
    EXPECT(plan_jvp(1, 1, 0, 1, pl, why, sizeof why) == PRHF_EINVAL, "no levels");
    EXPECT(plan_jvp(1, 1, 10, -1, pl, why, sizeof why) == PRHF_EINVAL, "n_tan < 0");
    // anchor worked out by hand from jvp_lds_bytes: 78 levels, 8 columns: 79*96 + 78*16 + 2048 + 1280 + 8*78*8
    EXPECT(plan_jvp(3, 5, 78, 9, pl, why, sizeof why) == PRHF_OK && pl.n_chunks == 2 &&
           jvp_chunk(pl, 9, 0).lds_bytes == 7584 + 1248 + 2048 + 1280 + 4992 && jvp_chunk(pl, 9, 1).nt == 1, "78-level anchor");
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::strcmp(argv[1], "check") == 0) {
        check();
        if (failures) return 1;
        std::printf("jvp_plan_host: ok\n");
        return 0;
    }
    if (argc == 6 && std::strcmp(argv[1], "plan") == 0) {
        JvpPlan pl;
        char why[256];
        const long long n_tan = std::atoll(argv[5]);
        if (plan_jvp(std::atoll(argv[2]), std::atoll(argv[3]), std::atoll(argv[4]), n_tan, pl, why, sizeof why) != PRHF_OK) {
            std::printf("refused: %s\n", why);
            return 0;
        }
        std::printf("%lld %d %d %d %lld\n", pl.blocks, pl.threads, pl.waves, pl.chunk, pl.n_chunks);
        for (long long i = 0; i < pl.n_chunks; ++i) {
            const JvpChunk ch = jvp_chunk(pl, n_tan, i);
            std::printf("%lld %d %d %zu\n", ch.first, ch.count, ch.nt, ch.lds_bytes);
        }
        return 0;
    }
    std::fprintf(stderr, "usage: jvp_plan_host check | plan n_prof n_freq levels n_tan\n");
    return 2;
}
