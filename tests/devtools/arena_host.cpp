// Host check of the scratch-buffer carver (pyrayhf_amd/csrc/prhf_arena.h): stand-alone, standard library only.
//   g++ -std=c++17 -Wall -I pyrayhf_amd/csrc tests/devtools/arena_host.cpp -o arena_host && ./arena_host
// (tests/test_arena_host.py builds it plain and with -fsanitize=address,undefined).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "prhf_arena.h"

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
    if (failures) return 1;
    std::printf("arena_host: ok\n");
    return 0;
}
