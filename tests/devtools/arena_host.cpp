// Host check of the scratch-buffer carver (pyrayhf_amd/csrc/prhf_arena.h) and of the arena's blocks of the operator and the
// stage ops (prhf_layouts.h, the functions the library compiles): stand-alone, standard library only.
//   g++ -std=c++17 -Wall -I pyrayhf_amd/csrc tests/devtools/arena_host.cpp -o arena_host && ./arena_host
// (tests/test_arena_host.py builds it plain and with -fsanitize=address,undefined).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "prhf_arena.h"
#include "prhf_layouts.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// What the MUF call of the gradient tracers keeps in the context's chunk scratch (grad_muf_run, prhf_api.cpp)
struct MufScratch {
    unsigned* queue;
    int* work;
    double* scan_d;
    double* group_freq;
    long long* group_field;
    double* state;
    double* best;
    double* out;
    int* active;
};
constexpr size_t kGradOutputs = 12, kGradSkipOutputs = 6 + kGradOutputs;       // PRHF_GRAD_OUTPUTS, PRHF_GRAD_SKIP_OUTPUTS
MufScratch muf_layout(Carver& k, size_t L, size_t E, size_t row_width) {
    MufScratch s;
    s.queue = k.take<unsigned>(128 / sizeof(unsigned));
    s.work = k.take<int>(2 * L);
    s.scan_d = k.take<double>(L * E);
    s.group_freq = k.take<double>(L);
    s.group_field = k.take<long long>(L);
    s.state = k.take<double>(4 * L);
    s.best = k.take<double>(L * (kGradSkipOutputs - kGradOutputs));
    s.out = k.take<double>(L * row_width);
    s.active = k.take<int>(L);
    return s;
}

size_t at(const void* p, const void* base) { return (size_t)(static_cast<const char*>(p) - static_cast<const char*>(base)); }

// One layout run twice: over a null base for its size, over a buffer of exactly that size for its pointers.  `check`
// gets the buffer's address and compares every offset with the hand arithmetic of the code the layout replaced
// (prhf_api.cpp of the commit before: stage_inputs :340-503, run_host_slabs :899-916, the stage ops :1525-1776 and
// :2271-2357), stated as numbers; it ends with a write to the last element of the last array, which the sanitized build
// checks against the buffer's end.  `bytes`: the parent's size formula.
template <class Layout, class Check>
void twice(const char* what, size_t bytes, size_t padding, Layout layout, Check check) {
    Carver sizing(nullptr);
    layout(sizing);
    if (sizing.used() + padding != bytes) {
        std::printf("FAILED %s: %zu bytes + %zu of padding, the parent asked for %zu\n", what, sizing.used(), padding, bytes);
        ++failures;
    }
    std::vector<char> buf(sizing.used());
    Carver k(buf.data());
    layout(k);
    CHECK(k.used() == sizing.used());
    const int before = failures;
    check(buf.data());
    if (failures != before) std::printf("  (in %s)\n", what);
}

// 3 profiles, 5 levels, 2 frequencies, a grid of 7 points, 2 ionograms: odd sizes, so that rounding shows
constexpr size_t P = 3, A = 5, F = 2, M = 7, I = 2, OUT = P * F;

void layouts() {
    OperatorBlock b;
    double* out = nullptr;
    ResidualBlock one;
    ManyBlock many;
    // the operator's inputs, a field and an altitude row per profile, the grid in the arena, no residual stage:
    // elems = n_freq + (n_prof + 2 * 3) * n_alt + 3 * n_alt + 7 + out_elems = 2 + 45 + 15 + 7 + 6 = 75
    const OperatorShape per_profile = {F, P, A, P, P, M};
    twice("operator, rows per profile", 75 * 8, 0, [&](Carver& k) { b = operator_block(k, per_profile); out = k.take<double>(OUT); },
          [&](char* base) {
              CHECK(at(b.freq, base) == 0 && at(b.den, base) == 16 && at(b.bmag, base) == 136 && at(b.bpsi, base) == 256);
              CHECK(at(b.alt, base) == 376 && at(b.mult, base) == 496 && at(out, base) == 552);      // in_elems = 69
              out[OUT - 1] = 1.0;
          });
    // a shared field (one row), one altitude row (alt_stride 0), the grid cached outside the arena, one observed trace:
    // elems = 2 + (3 + 2) * 5 + 5 + 0 + 6 + post_elems, post_elems = n_freq + out_elems + n_prof = 11: 49
    const OperatorShape shared = {F, P, A, 1, 1, 0};
    twice("operator, shared rows, cached grid, one trace", 49 * 8, 0,
          [&](Carver& k) { b = operator_block(k, shared); out = k.take<double>(OUT); one = residual_block(k, F, OUT, P); },
          [&](char* base) {
              CHECK(at(b.freq, base) == 0 && at(b.den, base) == 16 && at(b.bmag, base) == 136 && at(b.bpsi, base) == 176);
              CHECK(at(b.alt, base) == 216 && at(b.mult, base) == 256 && at(out, base) == 256);      // in_elems = 32
              CHECK(at(one.obs, base) == 304 && at(one.residual, base) == 320 && at(one.cost, base) == 368);
              one.cost[P - 1] = 1.0;
          });
    // run_host_slabs' chain, shared rows: elems = n_freq + (n_prof + 2 + 1) * n_alt + n_points + n_prof * n_freq = 45
    const OperatorShape slabs = {F, P, A, 1, 1, M};
    twice("run_host_slabs", 45 * 8, 0, [&](Carver& k) { b = operator_block(k, slabs); out = k.take<double>(OUT); },
          [&](char* base) {
              CHECK(at(b.den, base) == 16 && at(b.bmag, base) == 136 && at(b.bpsi, base) == 176 && at(b.alt, base) == 216);
              CHECK(at(b.mult, base) == 256 && at(out, base) == 312);
              out[OUT - 1] = 1.0;
          });
    // ... and with rows per profile: the first case's 75 elements
    twice("run_host_slabs, rows per profile", 75 * 8, 0, [&](Carver& k) { b = operator_block(k, per_profile); out = k.take<double>(OUT); },
          [&](char* base) { CHECK(at(b.alt, base) == 376 && at(b.mult, base) == 496 && at(out, base) == 552); });
    // The many-ionogram block behind the first case's 552 + 48 bytes.  post_elems = n_iono * (n_freq + 2) + [out_elems] +
    // cost_elems + (n_prof + 1) / 2; the int32 tail, carved as int32, ends 4 bytes before the parent's two doubles.
    // rows named by ionogram_of_row, residual rows: 8 + 6 + 3 + 2 = 19
    const auto fused = [&](size_t residual_elems, bool by_row) {
        return [&, residual_elems, by_row](Carver& k) {
            b = operator_block(k, per_profile);
            out = k.take<double>(OUT);
            many = many_block(k, I, F, P, residual_elems, by_row);
        };
    };
    twice("many ionograms: rows named, residual", (75 + 19) * 8, 4, fused(OUT, true), [&](char* base) {
        CHECK(at(many.obs, base) == 600 && at(many.residual, base) == 632 && at(many.cost, base) == 680);
        CHECK(at(many.best_cost, base) == 704 && at(many.best, base) == 720 && at(many.ionogram_of_row, base) == 736);
        many.ionogram_of_row[P - 1] = 1;
    });
    // rows named, no residual array: 8 + 0 + 3 + 2 = 13
    twice("many ionograms: rows named, no residual", (75 + 13) * 8, 4, fused(0, true), [&](char* base) {
        CHECK(at(many.obs, base) == 600 && at(many.residual, base) == 632 && at(many.cost, base) == 632);
        CHECK(at(many.best_cost, base) == 656 && at(many.best, base) == 672 && at(many.ionogram_of_row, base) == 688);
        many.ionogram_of_row[P - 1] = 1;
    });
    // shared candidates (ionogram_of_row null: its room is kept), a cost per ionogram and row: 8 + 0 + 6 + 2 = 16
    twice("many ionograms: shared candidates", (75 + 16) * 8, 4, fused(0, false), [&](char* base) {
        CHECK(at(many.obs, base) == 600 && at(many.cost, base) == 632 && at(many.best_cost, base) == 680);
        CHECK(at(many.best, base) == 696 && at(many.ionogram_of_row, base) == 712);
        many.ionogram_of_row[P - 1] = 1;
    });
    // ... and with residual rows (the entry points refuse the combination; the layout has no say): 8 + 6 + 6 + 2 = 22
    twice("many ionograms: shared candidates, residual", (75 + 22) * 8, 4, fused(OUT, false), [&](char* base) {
        CHECK(at(many.residual, base) == 632 && at(many.cost, base) == 680 && at(many.best_cost, base) == 728);
        CHECK(at(many.best, base) == 744 && at(many.ionogram_of_row, base) == 760);
        many.ionogram_of_row[P - 1] = 1;
    });
    // prhf_residual_many_f64: the model rows in front.  elems = pf + obs + pf + cost + 2 n_iono + (n_rows + 1) / 2 =
    // 6 + 4 + 6 + 3 + 4 + 2 = 25
    double* model = nullptr;
    twice("residual_many", 25 * 8, 4, [&](Carver& k) { model = k.take<double>(P * F); many = many_block(k, I, F, P, P * F, true); },
          [&](char* base) {
              CHECK(at(model, base) == 0 && at(many.obs, base) == 48 && at(many.residual, base) == 80 && at(many.cost, base) == 128);
              CHECK(at(many.best_cost, base) == 152 && at(many.best, base) == 168 && at(many.ionogram_of_row, base) == 184);
              many.ionogram_of_row[P - 1] = 1;
          });
    // prhf_residual_f64: (2 pf + n_freq + n_prof) = 12 + 2 + 3 = 17
    twice("residual", 17 * 8, 0, [&](Carver& k) { model = k.take<double>(P * F); one = residual_block(k, F, P * F, P); },
          [&](char* base) {
              CHECK(at(one.obs, base) == 48 && at(one.residual, base) == 64 && at(one.cost, base) == 112);
              one.cost[P - 1] = 1.0;
          });
    // prhf_regrid_f64: in_elems = n_freq + 4 n_alt + n_points = 29, then eight arrays of fn = 14: (29 + 112) * 8
    RegridBlock g;
    twice("regrid", (29 + 8 * 14) * 8, 0, [&](Carver& k) { g = regrid_block(k, F, A, M); }, [&](char* base) {
        CHECK(at(g.freq, base) == 0 && at(g.col[0], base) == 16 && at(g.col[1], base) == 56 && at(g.col[2], base) == 96);
        CHECK(at(g.col[3], base) == 136 && at(g.mult, base) == 176);
        for (size_t i = 0; i < 7; ++i) CHECK(at(g.out[i], base) == 232 + i * 112);
        CHECK(at(g.ind, base) == 1016);
        g.ind[F * M - 1] = 1;
    });
    // prhf_field_sample_f64, axes of 3 and 5 values, 7 points: (n0 + n1 + 7 n) * 8; device pointers: the axes alone
    FieldSampleBlock s;
    twice("field_sample", (3 + 5 + 7 * 7) * 8, 0, [&](Carver& k) { s = field_sample_block(k, 3, 5, 7); }, [&](char* base) {
        CHECK(at(s.a0, base) == 0 && at(s.a1, base) == 24 && at(s.p0, base) == 64 && at(s.p1, base) == 120 && at(s.field, base) == 176);
        for (size_t i = 0; i < 4; ++i) CHECK(at(s.out[i], base) == 64 + (3 + i) * 56);
        s.out[3][6] = 1.0;
    });
    twice("field_sample, device pointers", (3 + 5) * 8, 0, [&](Carver& k) { s = field_sample_block(k, 3, 5, 0); },
          [&](char* base) { CHECK(at(s.a1, base) == 24); s.a1[4] = 1.0; });
    // prhf_field_pack_f64, 2 fields of 3 x 5 nodes: (n0 + n1 + 2 cells) * 8
    FieldPackBlock f;
    twice("field_pack", (3 + 5 + 2 * 30) * 8, 0, [&](Carver& k) { f = field_pack_block(k, 3, 5, 30); }, [&](char* base) {
        CHECK(at(f.a0, base) == 0 && at(f.a1, base) == 24 && at(f.mu, base) == 64 && at(f.mup, base) == 304);
        f.mup[29] = 1.0;
    });
    // prhf_mu_mup_f64: 5 n; prhf_find_vh_f64 on 3 rows of 5: 4 n + n_rows
    MuMupBlock m;
    twice("mu_mup", 5 * 7 * 8, 0, [&](Carver& k) { m = mu_mup_block(k, 7); }, [&](char* base) {
        CHECK(at(m.in[0], base) == 0 && at(m.in[1], base) == 56 && at(m.in[2], base) == 112);
        CHECK(at(m.out[0], base) == 168 && at(m.out[1], base) == 224);
        m.out[1][6] = 1.0;
    });
    FindVhBlock v;
    twice("find_vh", (4 * 15 + 3) * 8, 0, [&](Carver& k) { v = find_vh_block(k, 3, 5); }, [&](char* base) {
        for (size_t i = 0; i < 4; ++i) CHECK(at(v.in[i], base) == i * 120);
        CHECK(at(v.vh, base) == 480);
        v.vh[2] = 1.0;
    });
}

}  // namespace

int main() {
    // a null base: null pointers, the same running sum
    {
        Carver k(nullptr);
        CHECK(k.used() == 0);
        CHECK(k.take<double>(3) == nullptr && k.used() == 24);
        CHECK(k.take<int>(5) == nullptr && k.used() == 44);
        CHECK(k.take<char>(0) == nullptr && k.used() == 44);
    }
    // a real base: base plus the running sum; a zero count gives the cursor and does not move it
    {
        std::vector<double> buf(64);
        Carver k(buf.data());
        double* a = k.take<double>(3);
        long long* b = k.take<long long>(2);
        int* z = k.take<int>(0);
        int* i = k.take<int>(3);
        unsigned* u = k.take<unsigned>(1);
        CHECK(at(a, buf.data()) == 0 && at(b, buf.data()) == 24 && at(z, buf.data()) == 40 && at(i, buf.data()) == 40);
        CHECK(at(u, buf.data()) == 52 && k.used() == 56);
        a[2] = 1.0; b[1] = 2; i[2] = 3; *u = 4u;                 // (inside the buffer: the sanitized build checks it)
    }
    // align rounds up, and once is enough
    {
        Carver k(nullptr);
        k.align(128);
        CHECK(k.used() == 0);
        k.take<double>(4 * 5);                                   // five profiles' scalars: 160 bytes
        k.align(128);
        CHECK(k.used() == 256);
        k.align(128);
        CHECK(k.used() == 256);
        k.take<char>(1);
        k.align(16);
        CHECK(k.used() == 272);
    }
    // the level tables' even-cell rounding: an odd number of cells leaves the entries 16-byte aligned
    {
        Carver k(nullptr);
        const size_t cells = 3 * 7;
        k.take<double>((cells + 1) & ~(size_t)1);
        CHECK(k.used() == 176 && k.used() % 16 == 0);
    }
    // The MUF block for L = 3 links, E = 5 scan elevations, rows of PRHF_GRAD_SKIP_OUTPUTS = 18: the offsets of the
    // hand-carved block this layout replaced (prhf_api.cpp of the commit before, lines 2966-2980): queue_bytes 128,
    // work_bytes L * 8 = 24, scan_bytes L * E * 8 = 120, then r += L, L, 4 L, L * 6, L * 18 doubles and L ints;
    // 128 + 24 + 120 + 8 * L * (1 + 1 + 4 + 6 + 18) + 4 * L = 1004 bytes.
    {
        const size_t L = 3, E = 5;
        Carver sizing(nullptr);
        muf_layout(sizing, L, E, kGradSkipOutputs);
        CHECK(sizing.used() == 1004);
        std::vector<char> buf(sizing.used());
        Carver k(buf.data());
        const MufScratch s = muf_layout(k, L, E, kGradSkipOutputs);
        CHECK(k.used() == sizing.used());
        CHECK(at(s.queue, buf.data()) == 0);
        CHECK(at(s.work, buf.data()) == 128);
        CHECK(at(s.scan_d, buf.data()) == 152);
        CHECK(at(s.group_freq, buf.data()) == 272);
        CHECK(at(s.group_field, buf.data()) == 296);
        CHECK(at(s.state, buf.data()) == 320);
        CHECK(at(s.best, buf.data()) == 416);
        CHECK(at(s.out, buf.data()) == 560);
        CHECK(at(s.active, buf.data()) == 992);
        s.active[L - 1] = 1;                                     // the last word of the block
        s.queue[0] = 0u;
    }
    layouts();
    if (failures) return 1;
    std::printf("arena_host: ok\n");
    return 0;
}
