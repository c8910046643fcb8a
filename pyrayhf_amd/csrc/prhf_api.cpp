// prhf_api.cpp - the C ABI of libprhf.so (include/prhf.h): contexts, host<->device staging, the
// execution of a launch plan, timing and error reporting.  What an operator call launches is decided
// in prhf_plan.h (plan_launch), without HIP; run() here carries the plan out in named steps.  No
// compute happens on the host; there is no CPU fallback: without a GPU every compute entry point
// fails with PRHF_EHIP.

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>
#include <xmmintrin.h>

#include "prhf.h"
#include "prhf_kernels.h"
#include "prhf_arena.h"       // Carver: a scratch buffer's layout stated once, for its size and its pointers
#include "prhf_layouts.h"     // ... the arena's blocks of the operator and the stage ops
#include "prhf_plan.h"        // Knobs, plan_launch, StatusWord: the launch planning, HIP-free
#include "prhf_lm_step.h"     // the Levenberg-Marquardt rule's statuses and limits (prhf_vfo_lm_fit_f64)

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(PRHF_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));      \
    } while (0)

constexpr size_t kPackBytes = 1u << 20;
constexpr size_t kSlabMinBytes = 16u << 20;    // host-buffer batches from this many input bytes on go in slabs (run_host_slabs)
constexpr size_t kDirectBytes = 128u << 10;   // inputs up to this size are written by the CPU through the BAR (direct_upload)

constexpr long long kMaxAlt = 1400;        // nodes + hints must fit 160 KiB of LDS
constexpr long long kMaxAltTall = 65535;   // taller profiles are staged in global memory (vfo_tall_kernel); level
                                           // indices travel as uint16 in the hint table

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

// Every entry point works on its context's device and leaves the calling thread's current HIP device as it
// found it (torch's current device is the same per-thread state: a library call must not move it).
class DeviceScope {
  public:
    explicit DeviceScope(int device) {
        err_ = hipGetDevice(&prev_);
        if (err_ == hipSuccess && prev_ != device) {
            err_ = hipSetDevice(device);
            switched_ = err_ == hipSuccess;
        }
    }
    ~DeviceScope() {
        if (switched_) (void)hipSetDevice(prev_);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
    hipError_t error() const { return err_; }

  private:
    int prev_ = -1;
    bool switched_ = false;
    hipError_t err_ = hipSuccess;
};
#define ENTER_DEVICE(dev)            \
    DeviceScope device_scope_(dev);  \
    HIP_TRY(device_scope_.error())

hipError_t create_events_untimed(hipEvent_t* ev, int n) {
    for (int i = 0; i < n; ++i) {
        const hipError_t e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t create_events(hipEvent_t* ev, int n) {
    for (int i = 0; i < n; ++i) {
        const hipError_t e = hipEventCreate(&ev[i]);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

struct prhf_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t aux_stream = nullptr;  // mixed lists: the short-grid launch runs beside the general one (fork / join by events)
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    hipStream_t up_stream = nullptr, down_stream = nullptr;   // host-buffer batches in slabs: uploads / downloads beside the kernels
    hipEvent_t slab_up[3] = {}, slab_done[3] = {}, slab_free = nullptr;
    hipStream_t stream = nullptr;
    // start / stop events of the most recent launches, a ring: a caller that enqueues many launches without
    // synchronising can still read every one's device time afterwards (prhf_recent_kernel_ms)
    static constexpr int kTimingRing = 64;
    hipEvent_t ring0[kTimingRing] = {}, ring1[kTimingRing] = {};
    unsigned long long n_timed = 0;    // launches timed so far
    int slot = 0;                      // ring slot of the last launch that was enqueued completely
    int pending = 0;                   // ring slot of the launch being enqueued: published by mark_timed() only, so that
                                       // a launch that fails half way leaves `slot` on the last good pair of events
    bool timed = false;
    hipEvent_t begin_ev() { pending = (int)(n_timed % kTimingRing); return ring0[pending]; }
    hipEvent_t pending_end_ev() const { return ring1[pending]; }
    hipEvent_t end_ev() const { return ring1[slot]; }
    void mark_timed() { slot = pending; ++n_timed; timed = true; }
    int math = PRHF_MATH_AUTO;
    Knobs knobs;
    int cu_count = 256;
    int large_bar = 0;   // hipDeviceAttributeIsLargeBar: device memory is mapped into the host's address space
    DevBuf arena;     // staged host inputs + output
    DevBuf partial;   // chunk sums
    DevBuf altmin;    // per-profile min(alt) for chunked slices
    DevBuf pairs;     // (m_i, m_i+1 - m_i) table of the fast tier's main loop
    DevBuf ftab;      // per-frequency scalars of a long launch
    DevBuf levels;    // level table of a grouped tracer launch
    DevBuf ptab;      // tracers: per-profile table of the frequency-independent parts of a level's mu, mu'
    DevBuf leftover;  // short-grid launches: the profiles left to the general kernel (count + block indices)
    DevBuf leftover_x;   // ... of the X-mode short-grid launch
    DevBuf leftover_tall;   // compact short-grid launch: the profiles whose bottomside needs the full-size arrays
    DevBuf leftover_tall_x; // ... of the X-mode short-grid launch
    DevBuf order;           // short-grid launch: its blocks by cost class (short_order_kernel)
    DevBuf tall;         // profiles of more than kMaxAlt levels: one slab of staged levels per resident workgroup
    DevBuf vjp;          // prhf_vfo_jacobian_f64 / prhf_vfo_vjp_f64 on host buffers: their inputs and result
    const double* pairs_src = nullptr;   // PRHF_FLAG_GRID_STABLE: multiplier array the table was built from
    int64_t pairs_len = 0;
    prhf::StridedPieces pairs_pieces = {};   // ... and the strided table's pieces that were built behind it
    // PRHF_FLAG_GRID_STABLE with HOST buffers: the stretched grid at a host address that keeps its contents is
    // uploaded, and its pair table built, once (a 20 000-point grid is 160 KB: more than the rest of a
    // single-profile call's inputs together)
    struct HostGrid {
        const double* host = nullptr;
        int64_t len = 0;
        DevBuf mult, pairs;
        bool pairs_ready = false;
        prhf::StridedPieces pieces = {};     // the strided table's pieces behind the pair table
    };
    static constexpr int kHostGrids = 16;
    HostGrid host_grid[kHostGrids];
    int n_host_grids = 0;
    bool order_clean = false;       // the class counters at the head of `order` are zero (short_order_kernel needs them so; the
                                    // follow-up kernel of the launch that used them leaves them so)
    unsigned* d_status = nullptr;   // kStatusWords device words, named by StatusWord (prhf_plan.h): the block queues of the
                                    // operator's persistent launches and the word of the peak pre-pass
    unsigned* h_status = nullptr;   // PRHF_STATUS_WORDS words of pinned host memory mapped into the device: word b = status
    unsigned* h_status_dev = nullptr;   // bit b (post_status) - nothing to copy back or reset on the device; its device address
    double* h_pack = nullptr;       // pinned, kPackBytes: inputs of a small host-buffer call, sent in one piece; its upper
    double* h_pack_dev = nullptr;   // half, mapped into the device (h_pack_dev), takes a small result straight from the kernel
    unsigned long long* d_words = nullptr;   // 2 words: nanmax|Y| bits, any-not-NaN
    unsigned long long* h_words = nullptr;   // pinned
    uint64_t stream_launches = 0;   // operator launches that took the streaming form since the context was made (prhf_stream_launches)
    unsigned long long* d_plan_counters = nullptr;   // prhf::kPlanCounterWords words, since the context was made (prhf_pair_plan_counters, prhf_panel_counters, prhf_panel_upper_counters, prhf_panel_plan_counters, prhf_panel_quick_counters)
    bool status_pending = false;
    uint64_t grad_home_counters[PRHF_GRAD_HOME_COUNTERS] = {};   // of the last prhf_gradient_home_f64 (prhf_gradient_home_counters)
    DevBuf fields;    // prhf_gradient_muf_f64: mu, mu' and the records of every link's field (48 bytes per node and link)
    uint64_t grad_skip_counters[PRHF_GRAD_SKIP_COUNTERS + 1] = {};   // of the last skip / MUF call of the gradient tracers, one-hop or chain; [4]: hop rays
    uint64_t host_waits = 0;        // times the host waited for the stream: prhf_sync, the peak pre-pass, a buffer that grew (ensure)
    uint64_t lm_counters[PRHF_LM_FIT_COUNTERS] = {};   // of the last prhf_vfo_lm_fit_f64 (prhf_lm_fit_counters)
};

namespace {

int ensure(prhf_ctx* c, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap) return PRHF_OK;
    if (b.p) {
        ++c->host_waits;
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    size_t want = bytes + bytes / 4 + 4096;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(PRHF_ENOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    }
    b.cap = want;
    return PRHF_OK;
}

// ---- The steps every entry point is assembled from: checks, carve, stage, tail ----

#define PRHF_TRY(expr)                     \
    do {                                   \
        const int rc_ = (expr);            \
        if (rc_ != PRHF_OK) return rc_;    \
    } while (0)

hipError_t upload(prhf_ctx* c, void* dst, const void* src, size_t bytes) {
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream);
}
hipError_t download(prhf_ctx* c, void* dst, const void* src, size_t bytes) {
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
}
// rows of row_elems doubles, `stride` elements apart at the source (0: a single row, as it stands), packed at dst
hipError_t upload_rows(prhf_ctx* c, double* dst, const double* src, size_t row_elems, size_t rows, int64_t stride) {
    return hipMemcpy2DAsync(dst, row_elems * 8, src, (stride ? (size_t)stride : row_elems) * 8, row_elems * 8, rows,
                            hipMemcpyHostToDevice, c->stream);
}

// A Carver (prhf_arena.h) that also stages: put() enqueues, on the pass over the buffer, the upload of a host array
// into its room - room it takes itself, or room that a layout of prhf_layouts.h took (null on the sizing pass).  A
// null array takes its room and gives a null pointer.
class Stager : public Carver {
  public:
    // pack: host memory that mirrors the buffer - put() copies there instead, for the caller to send in one piece
    Stager(prhf_ctx* c, void* base, void* pack = nullptr)
        : Carver(base), c_(c), base_(static_cast<char*>(base)), pack_(static_cast<char*>(pack)) {}
    template <class T>
    T* put(const void* src, size_t count) {
        T* d = take<T>(count);
        if (!src) return nullptr;
        put(d, src, count);
        return d;
    }
    template <class T>
    void put(T* d, const void* src, size_t count) {
        if (!d || !src) return;
        if (pack_) std::memcpy(mirror(d), src, count * sizeof(T));
        else if (err_ == hipSuccess) err_ = upload(c_, d, src, count * sizeof(T));
    }
    // row-wise, for a strided source (upload_rows); no rows: nothing
    void put_rows(double* d, const double* src, size_t row_elems, size_t rows, int64_t stride) {
        if (!d || !rows) return;
        if (pack_)
            for (size_t r = 0; r < rows; ++r) std::memcpy(mirror(d + r * row_elems), src + r * (size_t)stride, row_elems * 8);
        else if (err_ == hipSuccess) err_ = upload_rows(c_, d, src, row_elems, rows, stride);
    }
    hipError_t error() const { return err_; }

  private:
    char* mirror(const void* d) const { return pack_ + (static_cast<const char*>(d) - base_); }
    prhf_ctx* c_;
    char *base_, *pack_;
    hipError_t err_ = hipSuccess;
};

// A buffer of the context laid out by `layout`, a function of a Stager: the pass over a null base gives the bytes the
// buffer must hold, the pass over the buffer gives the pointers and sends the uploads.  No size is written down beside
// its carving.
template <class Layout>
int carve(prhf_ctx* c, DevBuf& b, Layout layout) {
    Stager sizing(c, nullptr);
    layout(sizing);
    PRHF_TRY(ensure(c, b, sizing.used()));
    Stager k(c, b.p);
    layout(k);
    HIP_TRY(k.error());
    return PRHF_OK;
}

// The tail of a launch: the two timing events around `launch` (one launch or a body of several, the first error
// returned), the ring slot published and - posts_status - the status words read at the next prhf_sync.
template <class Launch>
int timed_launch(prhf_ctx* c, bool posts_status, Launch launch) {
    HIP_TRY(hipEventRecord(c->begin_ev(), c->stream));
    HIP_TRY(launch());
    HIP_TRY(hipEventRecord(c->pending_end_ev(), c->stream));
    c->mark_timed();
    if (posts_status) c->status_pending = true;
    return PRHF_OK;
}

// Optional second stage of a launch: residual rows against one observed trace (prhf_vfo_residual_f64), or - n_iono > 0 -
// against the traces of many ionograms on the launch's frequency grid (prhf_vfo_residual_many_f64).
struct Residual {
    const double* vh_obs;   // (n_freq); many ionograms: (n_iono, n_freq), NaN where there is no observation
    double* residual;       // (n_prof, n_freq) or null
    double* cost;           // (n_prof) or null; many ionograms: (n_prof), shared candidates (n_iono, n_prof), never null
    // many ionograms only:
    int64_t n_iono = 0;
    const int32_t* ionogram_of_row = nullptr;   // (n_prof), or null: shared candidates
    int64_t* best = nullptr;                    // (n_iono)
    double* best_cost = nullptr;                // (n_iono)
    size_t cost_elems(int64_t n_prof) const {
        return n_iono ? many_cost_elems((size_t)n_prof, (size_t)n_iono, ionogram_of_row != nullptr) : (size_t)n_prof;
    }
};

// The most dynamic LDS of a streaming workgroup (two slots; plan_launch admits what fits kLdsFull).  A -DPRHF_TRACE build
// keeps a kilobyte of marks in static LDS on top of the slots' headers: the launches it is made for leave that room.
#ifdef PRHF_TRACE
constexpr size_t kStreamLdsMax = kLdsFull - 2048;
#else
constexpr size_t kStreamLdsMax = kLdsFull;
#endif

int status_to_code(unsigned bits) {
    if (bits & PRHF_STATUS_PEAK0)
        return fail(PRHF_EPEAK0, "density peak at index 0: no bottomside levels below the peak");
    if (bits & PRHF_STATUS_NANINPUT)
        return fail(PRHF_EINVAL, "NaN in a profile (alt, bmag or bpsi below the density peak)");
    if (bits & PRHF_STATUS_NEGDEN) return fail(PRHF_ENEGDEN, "Density must be non-negative");
    if (bits & PRHF_STATUS_BADGROUP) return fail(PRHF_EINVAL, "ray_group outside [0, n_groups)");
    if (bits & PRHF_STATUS_BADINDEX) return fail(PRHF_EINVAL, "profile_index outside [0, n_prof)");
    if (bits & PRHF_STATUS_BADFIELD) return fail(PRHF_EINVAL, "field index outside [0, n_fields)");
    if (bits & PRHF_STATUS_PATHLEN) return fail(PRHF_EINVAL, "a ray has more path nodes than path_stride");
    if (bits & PRHF_STATUS_STALL)
        return fail(PRHF_EHIP, "streaming launch gave up: a wave waited seconds for a slot of its own workgroup (the outputs of "
                    "this call are incomplete; option stream_blocks = 0 takes the general kernel)");
    return PRHF_OK;
}

// What the operator and its derivatives (Jacobian, VJP, JVP) are called on.  n_points, mode: of a call on the whole
// batch (a work list names its own per slice)
struct OperatorInputs {
    const double* freq;
    int64_t n_freq;
    const double *den, *bmag, *bpsi, *alt;
    int64_t n_prof, n_alt, prof_stride, alt_stride;
    const double* mult;
    int32_t n_points, mode;
    uint32_t flags;
    bool dev() const { return (flags & PRHF_FLAG_DEVICE_PTRS) != 0; }
    bool shared_field() const { return (flags & PRHF_FLAG_SHARED_FIELD) != 0; }
    OperatorShape shape(size_t mult_elems) const {       // of a host-buffer call's inputs in the arena (prhf_layouts.h)
        const size_t P = (size_t)n_prof;
        return {(size_t)n_freq, P, (size_t)n_alt, shared_field() ? 1 : P, alt_stride ? P : 1, mult_elems};
    }
};
// ... and what an operator call does with them: its slices of the multiplier array, the result rows, the residual stage
struct OperatorWork {
    int64_t mult_len;
    const prhf_segment* segs;
    int32_t n_segs;
    double* out;
    const Residual* post;
};
// an input of a device-pointer call in a block's slot (prhf_layouts.h); the kernels read it only
double* mut(const double* p) { return const_cast<double*>(p); }
int kmode(int32_t mode) { return mode == PRHF_MODE_O ? PRHF_KMODE_O : PRHF_KMODE_X; }
// The one slice of a call on the whole batch
prhf_segment whole_batch(int64_t n_prof, int32_t mode, int32_t n_points) {
    prhf_segment seg;
    seg.prof_begin = 0;
    seg.prof_end = n_prof;
    seg.mode = mode;
    seg.n_points = n_points;
    seg.mult_offset = 0;
    seg.out_offset = 0;
    return seg;
}

// One operator call on its way through run(): the caller's arguments, and what one step leaves for the next
struct Call : OperatorInputs, OperatorWork {
    prhf_ctx* c;
    // stage_inputs:
    prhf_ctx::HostGrid* grid;   // host buffers with PRHF_FLAG_GRID_STABLE: the cached device copy of the grid
    double* d_out;              // host buffers: the result rows in the arena
    size_t in_elems, out_elems; // ... the doubles in front of them, and theirs
    bool out_direct;            // the kernels write the result into pinned host memory themselves
    double* vh_dev;             // the modeled trace on the device
    ManyBlock stage;            // ... and the residual stage's arrays there (one trace: obs, residual, cost)
    // update_tables:
    unsigned* order_made;       // the short-grid O launch's blocks by cost (short_order_kernel), or null: index order
};

// PRHF_FLAG_GRID_STABLE with host buffers: the cached copy of this grid, or null
prhf_ctx::HostGrid* find_host_grid(prhf_ctx* c, const double* mult, int64_t mult_len) {
    for (int g = 0; g < c->n_host_grids; ++g)
        if (c->host_grid[g].host == mult && c->host_grid[g].len == mult_len) return &c->host_grid[g];
    return nullptr;
}

// The argument checks of the operator and its derivatives, in parts: an entry point calls them in its own order, which
// is part of its contract (tests/test_gpu_operator_abi_rejections.py, tests/test_gpu_tracer_abi_rejections.py).
// others_given: the arrays of the entry point's own are there
int check_arrays(prhf_ctx* c, const OperatorInputs& in, bool others_given) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (!in.freq || !in.den || !in.bmag || !in.bpsi || !in.alt || !in.mult || !others_given)
        return fail(PRHF_EINVAL, "null array pointer");
    return PRHF_OK;
}
// whole_batch: n_points is the call's own
int check_shape(const OperatorInputs& in, bool whole_batch) {
    if (in.n_freq < 1 || in.n_prof < 0 || in.n_alt < 1 || (whole_batch && in.n_points < 1)) return fail(PRHF_EINVAL, "bad shape");
    if (in.n_alt > kMaxAltTall)
        return fail(PRHF_EINVAL, "n_alt %lld exceeds the limit of %lld levels", (long long)in.n_alt, kMaxAltTall);
    if (in.n_freq > (1 << 20)) return fail(PRHF_EINVAL, "n_freq too large");
    if (in.prof_stride < in.n_alt || (in.alt_stride != 0 && in.alt_stride < in.n_alt))
        return fail(PRHF_EINVAL, "row stride shorter than a row");
    return PRHF_OK;
}
int check_flags(const OperatorInputs& in) {
    if (in.flags & ~(PRHF_FLAG_DEVICE_PTRS | PRHF_FLAG_ASYNC | PRHF_FLAG_GRID_STABLE | PRHF_FLAG_SHARED_FIELD))
        return fail(PRHF_EINVAL, "unknown flag bits");
    if ((in.flags & PRHF_FLAG_ASYNC) && !in.dev()) return fail(PRHF_EINVAL, "PRHF_FLAG_ASYNC needs device pointers");
    return PRHF_OK;
}
// The stretched grid of a host-buffer call must not decrease (smooth_nonuniform_grid never does): the top-segment search
// of the main loop relies on it.  Device-resident grids are the caller's.
int check_grid(const double* mult, int64_t mult_len, const prhf_segment* segs, int32_t n_segs) {
    const long long bad = first_decreasing_grid_entry(mult, mult_len, segs, n_segs);
    if (bad >= 0) return fail(PRHF_EINVAL, "multiplier[%lld] decreases: the stretched grid must be non-decreasing", bad);
    return PRHF_OK;
}

int check_arguments(const Call& k) {
    PRHF_TRY(check_arrays(k.c, k, k.segs && (k.out || k.post)));
    if (k.post && (!k.post->vh_obs || (!k.post->residual && !k.post->cost)))
        return fail(PRHF_EINVAL, "null array pointer");
    PRHF_TRY(check_shape(k, false));
    if (k.n_segs < 1 || k.n_segs > PRHF_MAX_SEGMENTS)
        return fail(PRHF_EINVAL, "1..%d segments per launch", PRHF_MAX_SEGMENTS);
    PRHF_TRY(check_flags(k));
    // (A sounder frequency that is not a positive finite number gives a NaN column, host and device buffers alike:
    //  freq_table_kernel / pair_freq.  The reference returns NaN for 0 and NaN, and something meaningless for f < 0.)
    // (a stable host grid that is cached already was checked when it was uploaded)
    const bool grid_known = !k.dev() && (k.flags & PRHF_FLAG_GRID_STABLE) && find_host_grid(k.c, k.mult, k.mult_len);
    if (!k.dev() && !grid_known) PRHF_TRY(check_grid(k.mult, k.mult_len, k.segs, k.n_segs));
    return PRHF_OK;
}

// The highest density peak of the launch (np.argmax's rule, the first NaN ranking highest - stage_profile's): a host
// scan, or the peak pre-pass and one synchronisation.  The caller has entered the device.
int highest_peak(prhf_ctx* c, const double* den, int64_t n_prof, int64_t n_alt, int64_t prof_stride, bool dev, long long* out) {
    long long max_peak = 0;
    if (dev) {
        HIP_TRY(hipMemsetAsync(c->d_status + kWordPeak, 0, sizeof(unsigned), c->stream));
        HIP_TRY(prhf::launch_peak_levels(den, n_prof, n_alt, prof_stride, c->d_status + kWordPeak, c->stream));
        unsigned peak = 0;
        HIP_TRY(hipMemcpyAsync(&peak, c->d_status + kWordPeak, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        ++c->host_waits;
        HIP_TRY(hipStreamSynchronize(c->stream));
        max_peak = peak;
    } else {
        for (int64_t p = 0; p < n_prof; ++p) {
            const double* d = den + (size_t)p * prof_stride;
            double bv = -HUGE_VAL;
            long long bi = 0;
            for (int64_t i = 0; i < n_alt; ++i) {
                const double key = (d[i] != d[i]) ? HUGE_VAL : d[i];
                if (key > bv) { bv = key; bi = i; }
            }
            max_peak = std::max(max_peak, bi);
        }
    }
    *out = max_peak;
    return PRHF_OK;
}

// Profiles of more levels than LDS holds are staged in global memory and take the generic loop (vfo_tall_kernel):
// no main loop, no candidate list, no short-grid kernels - the same values as any profile that leaves those paths.
// Decided once the highest density peak of the launch is known: only the bottomside is staged, and a column of 2 500
// levels at 0.25 km has its peak near level 900 (highest_peak).  When every bottomside fits, the LDS kernels run with
// their staged arrays sized for that peak (KArgs::lds_levels).
int decide_tall(const Call& k, bool& tall, long long& lds_levels) {
    tall = k.n_alt > kMaxAlt;
    lds_levels = k.n_alt;
    if (!(tall && k.n_prof > 0 && k.c->knobs.trim_lds != 0)) return PRHF_OK;
    long long max_peak = 0;
    PRHF_TRY(highest_peak(k.c, k.den, k.n_prof, k.n_alt, k.prof_stride, k.dev(), &max_peak));
    if (max_peak + 1 <= kMaxAlt) {
        tall = false;
        lds_levels = max_peak + 1;
    }
    return PRHF_OK;
}

// The scratch of the chunked slices, the inputs of a host-buffer call on the device (three routes: the CPU's own
// stores through the BAR, one copy from the pinned pack buffer, or a copy per array), the residual stage's arrays;
// then the launch arguments' pointers and strides.
int stage_inputs(Call& k, const LaunchPlan& pl, prhf::KArgs& a) {
    prhf_ctx* c = k.c;
    const int64_t n_freq = k.n_freq, n_prof = k.n_prof, n_alt = k.n_alt, mult_len = k.mult_len;
    int rc;
    if ((rc = ensure(c, c->partial, (size_t)pl.partial_elems * 8)) != PRHF_OK) return rc;
    if ((rc = ensure(c, c->altmin, (size_t)pl.altmin_elems * 8)) != PRHF_OK) return rc;
    a.partial = static_cast<double*>(c->partial.p);
    a.altmin = static_cast<double*>(c->altmin.p);
    a.status = c->h_status_dev;

    const size_t out_elems = k.out_elems = (size_t)pl.out_rows * (size_t)n_freq;
    ResidualBlock one = {};                    // host buffers: the residual stage's arrays behind the result rows
    ManyBlock many = {};
    if (k.dev()) {
        a.freq = k.freq; a.den = k.den; a.bmag = k.bmag; a.bpsi = k.bpsi; a.alt = k.alt; a.mult = k.mult;
        a.out = k.out;
        a.prof_stride = k.prof_stride;
        a.field_stride = k.shared_field() ? 0 : k.prof_stride;
        a.alt_stride = k.alt_stride;
    } else {
        // a stable host grid lives in a device buffer of its own, uploaded on first sight
        if (k.flags & PRHF_FLAG_GRID_STABLE) {
            k.grid = find_host_grid(c, k.mult, mult_len);
            if (!k.grid && c->n_host_grids < prhf_ctx::kHostGrids) {
                prhf_ctx::HostGrid& g = c->host_grid[c->n_host_grids];
                if ((rc = ensure(c, g.mult, (size_t)mult_len * 8)) != PRHF_OK) return rc;
                HIP_TRY(hipMemcpyAsync(g.mult.p, k.mult, (size_t)mult_len * 8, hipMemcpyHostToDevice, c->stream));
                g.host = k.mult;
                g.len = mult_len;
                g.pairs_ready = false;
                k.grid = &g;
                ++c->n_host_grids;
            }
        }
        // The arena: the inputs, packed (operator_block), the result rows, the residual stage's block
        const OperatorShape shape = k.shape(k.grid ? 0 : (size_t)mult_len);
        OperatorBlock b;
        auto inputs = [&](Stager& st) {
            b = operator_block(st, shape);
            st.put(b.freq, k.freq, shape.n_freq);
            st.put_rows(b.den, k.den, shape.n_alt, shape.n_prof, k.prof_stride);
            if (n_prof > 0) st.put_rows(b.bmag, k.bmag, shape.n_alt, shape.field_rows, k.prof_stride);
            if (n_prof > 0) st.put_rows(b.bpsi, k.bpsi, shape.n_alt, shape.field_rows, k.prof_stride);
            if (k.alt_stride) st.put_rows(b.alt, k.alt, shape.n_alt, shape.n_prof, k.alt_stride);
            else st.put(b.alt, k.alt, shape.n_alt);
            if (!k.grid) st.put(b.mult, k.mult, shape.mult_len);
            k.in_elems = st.used() / 8;
        };
        auto results = [&](Carver& st) {
            k.d_out = st.take<double>(out_elems);
            if (k.post && k.post->n_iono)
                many = many_block(st, (size_t)k.post->n_iono, (size_t)n_freq, (size_t)n_prof, k.post->residual ? out_elems : 0,
                                  k.post->ionogram_of_row != nullptr);
            else if (k.post) one = residual_block(st, (size_t)n_freq, out_elems, (size_t)n_prof);
        };
        Stager sizing(c, nullptr);
        inputs(sizing);
        results(sizing);
        PRHF_TRY(ensure(c, c->arena, sizing.used()));
        double* const base = static_cast<double*>(c->arena.p);
        const size_t in_elems = k.in_elems;
        void* pack = nullptr;                  // the per-array route: a copy per array, rows as rows
        bool direct = false;
        if (in_elems * 8 <= kPackBytes && c->h_pack) {
            // A small call (the reference's usual one: a single profile): six separate uploads from pageable
            // memory cost more than the kernel.  Pack the inputs in the arena's own order into a pinned
            // buffer and send them in one piece.  The buffer is reused by the next call, so the copy must
            // have left it first: the previous call has synchronised unless it was asynchronous, which host
            // buffers never are.
            // On a large-BAR device (every Instinct board) the staging buffer is not needed either: device memory is
            // mapped into this process, so the CPU writes the 22 KB of a single-profile call straight into the arena -
            // posted write-combined stores over PCIe, 0.4 - 0.8 us (tools/probes/bar_probe.cpp) - and the copy kernel
            // the runtime would have launched for the upload, with its dependency in front of ours (~10 us between
            // them), is gone.  Ordering: the stores are fenced before the launch's doorbell write, which travels the same
            // way behind them; the kernel's start-of-kernel acquire drops what its L2 still holds of the arena.  The arena
            // must be idle: host-buffer calls synchronise before they return, but an asynchronous device-pointer call -
            // or a launch on a stream the context borrowed before - may still be using it; then the staged copy, which is
            // ordered by the stream, is taken.
            direct = c->large_bar && c->knobs.direct_upload != 0 && in_elems * 8 <= kDirectBytes &&
                     hipStreamQuery(c->stream) == hipSuccess && (!c->timed || hipEventQuery(c->end_ev()) == hipSuccess);
            (void)hipGetLastError();               // (hipErrorNotReady from the two queries is not an error)
            pack = direct ? base : c->h_pack;
        }
        Stager st(c, base, pack);
        inputs(st);
        HIP_TRY(st.error());
        if (direct) _mm_sfence();
        else if (pack) HIP_TRY(upload(c, base, pack, in_elems * 8));
        results(st);
        a.freq = b.freq; a.den = b.den; a.bmag = b.bmag; a.bpsi = b.bpsi; a.alt = b.alt;
        a.mult = k.grid ? static_cast<const double*>(k.grid->mult.p) : b.mult;
        double* const d_out = a.out = k.d_out;
        // rows that no segment covers must come back as NaN, not as whatever the arena held (all-ones bytes = NaN)
        long long covered = 0;
        for (int i = 0; i < k.n_segs; ++i) covered += k.segs[i].prof_end - k.segs[i].prof_begin;
        // A small result (the reference's usual call: one profile) goes straight from the kernel into pinned host
        // memory - the upper half of the pack buffer, which the device sees - instead of into the arena and through
        // a copy of its own: one runtime call and one DMA round trip less per call.
        k.out_direct = k.out && out_elems && !k.post && c->h_pack && out_elems * 8 <= kPackBytes / 4 &&
                       in_elems * 8 <= kPackBytes / 2;
        if (k.out_direct) {
            a.out = c->h_pack_dev + kPackBytes / 16;           // doubles: byte offset kPackBytes / 2
            if (covered < pl.out_rows) std::memset(c->h_pack + kPackBytes / 16, 0xFF, out_elems * 8);
            covered = pl.out_rows;                             // (no device-side fill)
        }
        if (covered < pl.out_rows && out_elems) HIP_TRY(hipMemsetAsync(d_out, 0xFF, out_elems * 8, c->stream));
        a.prof_stride = n_alt;
        a.field_stride = k.shared_field() ? 0 : n_alt;
        a.alt_stride = k.alt_stride ? n_alt : 0;
    }

    k.vh_dev = a.out;
    if (k.dev() && k.post && !k.out) {           // caller does not want the modeled trace: keep it in scratch
        if ((rc = ensure(c, c->arena, out_elems * 8)) != PRHF_OK) return rc;
        k.vh_dev = a.out = static_cast<double*>(c->arena.p);
    }
    // the residual stage's arrays: the caller's own on the device, else the arena's block behind the result rows
    if (!k.post) return PRHF_OK;
    const Residual& r = *k.post;
    k.stage = {mut(r.vh_obs), r.residual, r.cost, r.best_cost, r.best, const_cast<int32_t*>(r.ionogram_of_row)};
    if (k.dev()) return PRHF_OK;
    const bool rows_named = r.n_iono && r.ionogram_of_row && n_prof > 0;
    if (r.n_iono) k.stage = many;
    else k.stage = {one.obs, one.residual, r.cost ? one.cost : nullptr, nullptr, nullptr, nullptr};
    if (!r.residual) k.stage.residual = nullptr;
    if (!rows_named) k.stage.ionogram_of_row = const_cast<int32_t*>(r.ionogram_of_row);
    HIP_TRY(upload(c, k.stage.obs, r.vh_obs, (size_t)(r.n_iono ? r.n_iono : 1) * (size_t)n_freq * 8));
    if (rows_named) HIP_TRY(upload(c, many.ionogram_of_row, r.ionogram_of_row, (size_t)n_prof * 4));
    return PRHF_OK;
}

// The pair table of the main loop with the strided table's pieces behind it (option strided_top), into
// `table`: the context's own, or the one cached with a stable host grid
int build_pair_table(prhf_ctx* c, DevBuf& table, const double* d_mult, int64_t mult_len, const LaunchPlan& pl) {
    int rc;
    if ((rc = ensure(c, table, (size_t)pl.table_entries * 16)) != PRHF_OK) return rc;
    HIP_TRY(prhf::launch_grid_pairs(d_mult, mult_len, static_cast<double*>(table.p), c->stream));
    HIP_TRY(prhf::launch_grid_strided(d_mult, static_cast<double*>(table.p), pl.pieces, c->stream));
    return PRHF_OK;
}

// The tables the plan asks for: the pair table - built with the strided pieces and cached with them; a cached table
// serves a launch whose pieces are the same - and the per-frequency table.
int update_tables(Call& k, const LaunchPlan& pl, prhf::KArgs& a) {
    prhf_ctx* c = k.c;
    if (!pl.want_pairs) return PRHF_OK;
    int rc;
    auto same_pieces = [&](const prhf::StridedPieces& o) { return std::memcmp(&o, &pl.pieces, sizeof pl.pieces) == 0; };
    if (k.grid) {
        if (!k.grid->pairs_ready || !same_pieces(k.grid->pieces)) {
            if ((rc = build_pair_table(c, k.grid->pairs, a.mult, k.mult_len, pl)) != PRHF_OK) return rc;
            k.grid->pairs_ready = true;
            k.grid->pieces = pl.pieces;
        }
        a.pairs = static_cast<const double*>(k.grid->pairs.p);
    } else {
        const bool stable = k.dev() && (k.flags & PRHF_FLAG_GRID_STABLE) != 0;
        if (!(stable && c->pairs.p && c->pairs_src == a.mult && c->pairs_len == k.mult_len && same_pieces(c->pairs_pieces))) {
            c->pairs_src = nullptr;
            if ((rc = build_pair_table(c, c->pairs, a.mult, k.mult_len, pl)) != PRHF_OK) return rc;
            if (stable) {
                c->pairs_src = a.mult;
                c->pairs_len = k.mult_len;
                c->pairs_pieces = pl.pieces;
            }
        }
        a.pairs = static_cast<const double*>(c->pairs.p);
    }
    if (!pl.freq_table) return PRHF_OK;
    if ((rc = ensure(c, c->ftab, ((size_t)k.n_freq + 1) * 64)) != PRHF_OK) return rc;
    // The table's kernel zeroes, on the way, every control word the launches behind it count in: the block
    // queues and the heads of the short-grid kernels' lists and the classes of the block order.  One memset each,
    // they were six operations on the stream in front of a short-grid launch (config 3: ~25 us of 530).
    prhf::ZeroWords zero;
    std::memset(&zero, 0, sizeof zero);
    auto zero_head = [&](DevBuf& b, size_t bytes) -> int {
        int rcz = ensure(c, b, bytes);
        if (rcz != PRHF_OK) return rcz;
        zero.p[zero.n] = static_cast<unsigned*>(b.p);
        zero.words[zero.n++] = 1;
        return PRHF_OK;
    };
    zero.p[zero.n] = c->d_status;
    zero.words[zero.n++] = kStatusWords;
    if (pl.o.blocks > 0) {
        if ((rc = zero_head(c->leftover, pl.o.list_bytes)) != PRHF_OK) return rc;
        if ((rc = zero_head(c->leftover_tall, pl.o.list_bytes)) != PRHF_OK) return rc;
    }
    if (pl.x.blocks > 0) {
        if ((rc = zero_head(c->leftover_x, pl.x.list_bytes)) != PRHF_OK) return rc;
        if ((rc = zero_head(c->leftover_tall_x, pl.x.list_bytes)) != PRHF_OK) return rc;
    }
    if (pl.short_order) {
        const size_t words = PRHF_ORDER_CLASSES * (size_t)(pl.o.blocks + 1);
        const void* before = c->order.p;
        if ((rc = ensure(c, c->order, words * sizeof(unsigned))) != PRHF_OK) return rc;
        unsigned* order = static_cast<unsigned*>(c->order.p);
        if (!c->order_clean || c->order.p != before)
            HIP_TRY(hipMemsetAsync(order, 0, PRHF_ORDER_CLASSES * sizeof(unsigned), c->stream));
        prhf::KArgs ap = a;
        ap.n_segs = pl.o.n_segs;
        ap.n_blocks = pl.o.blocks;
        std::copy(pl.o.seg, pl.o.seg + pl.o.n_segs, ap.seg);
        c->order_clean = false;                // (until the follow-up kernel of this launch has run)
        HIP_TRY(prhf::launch_short_order(ap, order, a.freq, static_cast<double*>(c->ftab.p), zero, c->stream));
        k.order_made = order;
    } else {
        HIP_TRY(prhf::launch_freq_table(a.freq, k.n_freq, static_cast<double*>(c->ftab.p), zero, c->stream));
    }
    a.ftab = static_cast<const double*>(c->ftab.p);
    return PRHF_OK;
}

// The launches' block queues (StatusWord), where the per-frequency table's kernel has not zeroed them already.  A launch
// without a queue - the single profile - enqueues nothing.
int zero_control_words(prhf_ctx* c, const LaunchPlan& pl) {
    if (!pl.zero_queues) return PRHF_OK;
    HIP_TRY(hipMemsetAsync(c->d_status, 0, kLaunchQueueWords * sizeof(unsigned), c->stream));
    if (pl.x.n_segs > 0) HIP_TRY(hipMemsetAsync(c->d_status + kWordShortXFull, 0, sizeof(unsigned), c->stream));
    return PRHF_OK;
}

int launch_general(prhf_ctx* c, const LaunchPlan& pl, prhf::KArgs& a) {
    if (pl.queue) a.queue = c->d_status + kWordGeneral;
    if (pl.stream) {
        a.n_blocks = pl.stream_blocks;         // (the form's own tail: LaunchPlan::stream_tail_bpp)
        a.seg[0].tail_bpp = pl.stream_tail_bpp;
        a.seg[0].tail_prof = pl.stream_tail_prof;
        HIP_TRY(prhf::launch_vfo_stream(a, pl.stream_grid, c->stream));
        ++c->stream_launches;
    } else if (pl.tall) HIP_TRY(prhf::launch_vfo_tall(a, pl.grid, c->stream));
    else HIP_TRY(prhf::launch_vfo(a, pl.grid, pl.launch_tier, pl.lds_bytes, c->stream));
    return PRHF_OK;
}

// What tells the two short-grid kinds apart when they are launched: their control words, their lists, the tier of the
// follow-up launch
struct ShortRoute {
    StatusWord first, full, follow;
    DevBuf *left, *left_tall;
    int follow_tier;
    unsigned* order;            // O mode: the blocks by cost class (or null)
    bool traced;                // -DPRHF_TRACE builds: this kind's waves are stamped
};

// One kind of short-grid slices (ShortKind): the short-grid kernel, where the plan says so a second launch of it with
// full-size arrays over the profiles the compact one left, and the general kernel over the profiles both left on their
// list.  launch(args, geometry) starts the kind's kernel.
template <class Launch>
int launch_short_kind(prhf_ctx* c, const LaunchPlan& pl, const ShortKind& sk, const ShortRoute& r, const prhf::KArgs& a,
                      hipStream_t stream, Launch launch) {
    if (sk.blocks == 0) return PRHF_OK;
    prhf::KArgs as = a;
    as.n_segs = sk.n_segs;
    std::copy(sk.seg, sk.seg + sk.n_segs, as.seg);
    as.n_blocks = sk.blocks;
    as.short_prio = (int)c->knobs.short_prio;
    as.partial = nullptr;
    as.altmin = nullptr;
    as.trace = nullptr;
    int rc;
#ifdef PRHF_TRACE
    static DevBuf trace_short;
    const size_t short_trace_words = (size_t)sk.blocks * kWavesPerBlock * 8;
    unsigned long long* trace = nullptr;
    if (std::getenv("PRHF_TRACE_FILE") && r.traced) {
        if ((rc = ensure(c, trace_short, short_trace_words * 8)) != PRHF_OK) return rc;
        HIP_TRY(hipMemsetAsync(trace_short.p, 0, short_trace_words * 8, stream));
        as.trace = trace = static_cast<unsigned long long*>(trace_short.p);
    }
#endif
    // the list heads: zeroed by the per-frequency table's kernel where there is one
    if ((rc = ensure(c, *r.left, sk.list_bytes)) != PRHF_OK) return rc;
    as.leftover = static_cast<unsigned*>(r.left->p);
    if (!pl.freq_table) HIP_TRY(hipMemsetAsync(as.leftover, 0, sizeof(unsigned), stream));
    if (sk.second) {
        // a profile that peaks above the compact arrays goes on a block list of its own
        if ((rc = ensure(c, *r.left_tall, sk.list_bytes)) != PRHF_OK) return rc;
        as.leftover_tall = static_cast<unsigned*>(r.left_tall->p);
        if (!pl.freq_table) HIP_TRY(hipMemsetAsync(as.leftover_tall, 0, sizeof(unsigned), stream));
    }
    as.lds_levels = sk.first.lds_levels;
    as.short_queue = sk.first.short_queue;
    as.queue = sk.first.queue ? c->d_status + r.first : nullptr;
    // from four resident rounds on, the blocks are drawn in descending order of a cost estimate
    as.order = r.order;                        // (sorted beside the per-frequency table, or null: index order)
    if ((rc = launch(as, sk.first)) != PRHF_OK) return rc;
    if (sk.second) {
        // the profiles the compact launch left for full-size arrays: persistent workgroups read their number from
        // the device (3 us when there is none); what these leave - another input shape - joins the general list
        as.trace = nullptr;
        as.lds_levels = sk.full.lds_levels;
        as.short_queue = sk.full.short_queue;
        as.block_list = as.leftover_tall;
        as.order = nullptr;
        as.leftover_tall = nullptr;
        as.queue = c->d_status + r.full;
        if ((rc = launch(as, sk.full)) != PRHF_OK) return rc;
    }
#ifdef PRHF_TRACE
    if (trace) {                                   // eight wall-clock marks per wave and block (tools/wave_trace_short.py)
        std::vector<unsigned long long> host(short_trace_words);
        HIP_TRY(hipMemcpyAsync(host.data(), trace, short_trace_words * 8, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (FILE* fp = std::fopen(std::getenv("PRHF_TRACE_FILE"), "wb")) {
            std::fwrite(host.data(), 8, short_trace_words, fp);
            std::fclose(fp);
        }
    }
#endif
    // the follow-up: the general kernel over the blocks on the list
    as.trace = nullptr;
    as.lds_levels = a.lds_levels;
    as.short_queue = sk.first.short_queue;
    as.leftover_tall = nullptr;
    as.order = nullptr;
    as.block_list = as.leftover;
    as.leftover = nullptr;
    as.queue = c->d_status + r.follow;
    as.zero_after = r.order;
    HIP_TRY(prhf::launch_vfo(as, sk.follow_grid, r.follow_tier, pl.lds_bytes, stream));
    if (as.zero_after) c->order_clean = true;
    return PRHF_OK;
}

// The many-ionogram residual stage on device arrays: masked residuals and costs, then every ionogram's winner
hipError_t launch_many(prhf_ctx* c, const double* vh_model, int64_t n_rows, const double* vh_obs, int64_t n_iono,
                       int64_t n_freq, const int32_t* ionogram_of_row, double* residual, double* cost, int64_t* best, double* best_cost) {
    prhf::ResidualManyArgs m;
    m.vh_model = vh_model;
    m.vh_obs = vh_obs;
    m.ionogram_of_row = ionogram_of_row;
    m.n_rows = n_rows;
    m.n_items = ionogram_of_row ? n_rows : n_iono * n_rows;
    m.n_iono = (int)n_iono;
    m.n_freq = (int)n_freq;
    m.items_per_wave = PRHF_MANY_ITEMS_PER_WAVE;
    m.residual = residual;
    m.cost = cost;
    const hipError_t e = prhf::launch_residual_many(m, c->stream);
    if (e != hipSuccess) return e;
    return prhf::launch_residual_best(cost, ionogram_of_row, n_rows, (int)n_iono, reinterpret_cast<long long*>(best), best_cost,
                                      c->stream);
}

// What the two many-ionogram entries ask of their arguments, before any device is touched.  freq_mhz: the fused entry's
// grid, or null.
int check_many(const double* freq_mhz, int64_t n_freq, int64_t n_rows, const double* vh_obs, int64_t n_iono,
               const int32_t* ionogram_of_row, const double* residual_out, const double* cost_out, const int64_t* best_out,
               const double* best_cost_out, uint32_t flags) {
    if (!vh_obs || !cost_out || !best_out || !best_cost_out) return fail(PRHF_EINVAL, "null array pointer");
    if (n_rows < 0 || n_iono < 1 || n_freq < 1) return fail(PRHF_EINVAL, "bad shape");
    if (n_freq > PRHF_MANY_MAX_FREQ)
        return fail(PRHF_EINVAL, "n_freq %lld exceeds the many-ionogram limit of %d grid frequencies", (long long)n_freq,
                    PRHF_MANY_MAX_FREQ);
    if (n_rows > 0x7fffffffLL || n_iono > 0x7fffffffLL) return fail(PRHF_EINVAL, "bad shape: more than 2^31 - 1 rows or ionograms");
    if (!ionogram_of_row && residual_out)
        return fail(PRHF_EINVAL, "shared candidates have no dense residual output");
    if (!ionogram_of_row && n_rows > 0 && n_iono > (int64_t)((1LL << 36) / n_rows))
        return fail(PRHF_EINVAL, "bad shape: more than 2^36 (ionogram, candidate) pairs");
    if (flags & PRHF_FLAG_DEVICE_PTRS) return PRHF_OK;
    if (freq_mhz)
        for (int64_t f = 0; f < n_freq; ++f)
            if (!std::isfinite(freq_mhz[f])) return fail(PRHF_EINVAL, "freq_mhz[%lld] is not finite: the common grid must be", (long long)f);
    if (ionogram_of_row)
        for (int64_t p = 0; p < n_rows; ++p) {
            if (ionogram_of_row[p] < 0 || ionogram_of_row[p] >= n_iono)
                return fail(PRHF_EINVAL, "ionogram_of_row[%lld] outside [0, n_iono)", (long long)p);
            if (p > 0 && ionogram_of_row[p] < ionogram_of_row[p - 1])
                return fail(PRHF_EINVAL, "ionogram_of_row[%lld] decreases: the rows of an ionogram must be contiguous", (long long)p);
        }
    return PRHF_OK;
}

// Every kernel of the operator, in the order and on the streams the plan sets
int launch_all(Call& k, const LaunchPlan& pl, prhf::KArgs& a) {
    prhf_ctx* c = k.c;
    int rc;
    hipStream_t short_stream = pl.forked ? c->aux_stream : c->stream;
    // Fork and join by events: the general launch goes first, on the caller's stream (LaunchPlan::forked)
    if (pl.forked) {
        HIP_TRY(hipEventRecord(c->fork_ev, c->stream));        // tables, queues and inputs are in place
        HIP_TRY(hipStreamWaitEvent(c->aux_stream, c->fork_ev, 0));
        if ((rc = launch_general(c, pl, a)) != PRHF_OK) return rc;
    }
    const ShortRoute route_x = {kWordShortX, kWordShortXFull, kWordShortXFollow, &c->leftover_x, &c->leftover_tall_x, 1, nullptr, false};
    const ShortRoute route_o = {kWordShortO, kWordShortOFull, kWordShortOFollow, &c->leftover, &c->leftover_tall, 0, k.order_made, true};
    rc = launch_short_kind(c, pl, pl.x, route_x, a, short_stream, [&](const prhf::KArgs& as, const ShortLaunch& l) -> int {   // (the longer blocks first)
        HIP_TRY(prhf::launch_vfo_shortx(as, l.grid, l.lds_bytes, l.threads, short_stream));
        return PRHF_OK;
    });
    if (rc != PRHF_OK) return rc;
    rc = launch_short_kind(c, pl, pl.o, route_o, a, short_stream, [&](const prhf::KArgs& as, const ShortLaunch& l) -> int {
        HIP_TRY(prhf::launch_vfo_short(as, l.grid, l.lds_bytes, l.threads, pl.o.lanes, short_stream));
        return PRHF_OK;
    });
    if (rc != PRHF_OK) return rc;
    if (pl.forked) {
        HIP_TRY(hipEventRecord(c->join_ev, c->aux_stream));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->join_ev, 0));
        return PRHF_OK;
    }
    return launch_general(c, pl, a);
}

// The results of a host-buffer call on their way back, and the synchronisation of every call that is not asynchronous
int download_and_sync(Call& k) {
    prhf_ctx* c = k.c;
    const size_t out_elems = k.out_elems;
    // small results come back through the pinned buffer too (its upper half; the inputs of a call this small
    // fit the lower one) and are handed over after the synchronisation below
    const bool out_via_pack = !k.out_direct && !k.dev() && k.out && out_elems && c->h_pack && out_elems * 8 <= kPackBytes / 4 &&
                              k.in_elems * 8 <= kPackBytes / 2;
    double* h_out = c->h_pack ? c->h_pack + kPackBytes / 16 : nullptr;       // doubles: byte offset kPackBytes / 2
    if (k.out_direct) {
        // (written by the kernel itself)
    } else if (out_via_pack)
        HIP_TRY(hipMemcpyAsync(h_out, k.d_out, out_elems * 8, hipMemcpyDeviceToHost, c->stream));
    else if (!k.dev() && out_elems && k.out)
        HIP_TRY(hipMemcpyAsync(k.out, k.d_out, out_elems * 8, hipMemcpyDeviceToHost, c->stream));
    if (!k.dev() && k.post) {
        if (k.post->residual)
            HIP_TRY(hipMemcpyAsync(k.post->residual, k.stage.residual, out_elems * 8, hipMemcpyDeviceToHost, c->stream));
        if (k.post->cost && !k.post->n_iono)
            HIP_TRY(hipMemcpyAsync(k.post->cost, k.stage.cost, (size_t)k.n_prof * 8, hipMemcpyDeviceToHost, c->stream));
        if (k.post->n_iono) {
            if (k.post->cost_elems(k.n_prof))
                HIP_TRY(hipMemcpyAsync(k.post->cost, k.stage.cost, k.post->cost_elems(k.n_prof) * 8, hipMemcpyDeviceToHost,
                                       c->stream));
            HIP_TRY(hipMemcpyAsync(k.post->best, k.stage.best, (size_t)k.post->n_iono * 8, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipMemcpyAsync(k.post->best_cost, k.stage.best_cost, (size_t)k.post->n_iono * 8, hipMemcpyDeviceToHost, c->stream));
        }
    }
    if (k.flags & PRHF_FLAG_ASYNC) return PRHF_OK;
    const int rc = prhf_sync(c);
    if (out_via_pack || k.out_direct) std::memcpy(k.out, h_out, out_elems * 8);
    return rc;
}

// Every prhf_vfo_* call: check, decide where the profiles are staged, plan (plan_launch, prhf_plan.h), then carry the
// plan out step by step.  The steps above enqueue on the context's stream in the order they are called here.
int run(prhf_ctx* c, const OperatorInputs& in, const OperatorWork& w) {
    Call k = {in, w, c};
    const int64_t n_freq = in.n_freq, n_prof = in.n_prof, n_alt = in.n_alt, mult_len = w.mult_len;
    const prhf_segment* const segs = w.segs;
    const int32_t n_segs = w.n_segs;
    const Residual* const post = w.post;
    int rc;
    if ((rc = check_arguments(k)) != PRHF_OK) return rc;
    ENTER_DEVICE(c->device);
    bool tall;
    long long lds_levels;
    if ((rc = decide_tall(k, tall, lds_levels)) != PRHF_OK) return rc;

    const LaunchShape shape = {n_prof, n_freq, n_alt, lds_levels, tall, mult_len, c->cu_count, c->math};
    LaunchPlan pl;
    char why[160];
    if (plan_launch(shape, segs, n_segs, c->knobs, pl, why, sizeof why) != PRHF_OK) return fail(PRHF_EINVAL, "%s", why);

    prhf::KArgs a;
    std::memset(&a, 0, sizeof a);
    a.n_freq = n_freq;
    a.n_alt = n_alt;
    a.lds_levels = lds_levels;
    a.n_segs = pl.n_segs;
    std::copy(pl.seg, pl.seg + pl.n_segs, a.seg);
    a.n_blocks = pl.blocks;
    a.no_candidates = pl.no_candidates;
    a.plan_counters = c->d_plan_counters;
    a.plan_cap = (int)c->knobs.pair_plan_cap;
    if ((rc = stage_inputs(k, pl, a)) != PRHF_OK) return rc;

    // (a synchronous host-buffer call may go untimed - option `timing`: nothing is left on the stream when it returns,
    //  so no later launch or stream switch needs its end event either)
    const bool timed_launch = k.dev() || c->knobs.timing != 0;
    if (timed_launch) HIP_TRY(hipEventRecord(c->begin_ev(), c->stream));
    if ((rc = update_tables(k, pl, a)) != PRHF_OK) return rc;
#ifdef PRHF_TRACE
    // diagnostics build (tools/wave_trace.py): per-wave wall-clock stamps of this launch, dumped to $PRHF_TRACE_FILE
    static DevBuf trace_buf;
    // start, end, staged, four staging marks, workgroup (the streaming form: PRHF_STREAM_THREADS / 64 waves per block)
    const size_t trace_words = (size_t)pl.blocks * (pl.stream ? PRHF_STREAM_THREADS / 64 : kWavesPerBlock) * 8;
    if (std::getenv("PRHF_TRACE_FILE") && pl.blocks > 0) {
        if ((rc = ensure(c, trace_buf, trace_words * 8)) != PRHF_OK) return rc;
        HIP_TRY(hipMemsetAsync(trace_buf.p, 0, trace_words * 8, c->stream));
        a.trace = static_cast<unsigned long long*>(trace_buf.p);
    }
#endif
    if (pl.tall_stride) {                      // a tall launch: one slab of staged levels per resident workgroup
        a.tall_stride = pl.tall_stride;
        if ((rc = ensure(c, c->tall, (size_t)pl.tall_slabs * a.tall_stride)) != PRHF_OK) return rc;
        a.tall = static_cast<unsigned char*>(c->tall.p);
    }
    if ((rc = zero_control_words(c, pl)) != PRHF_OK) return rc;
    if ((rc = launch_all(k, pl, a)) != PRHF_OK) return rc;
#ifdef PRHF_TRACE
    if (a.trace) {
        std::vector<unsigned long long> host(trace_words);
        HIP_TRY(hipMemcpyAsync(host.data(), a.trace, trace_words * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (FILE* fp = std::fopen(std::getenv("PRHF_TRACE_FILE"), "wb")) {
            std::fwrite(host.data(), 8, trace_words, fp);
            std::fclose(fp);
        }
    }
#endif
    if (post && post->n_iono) {
        HIP_TRY(launch_many(c, k.vh_dev, n_prof, k.stage.obs, post->n_iono, n_freq, k.stage.ionogram_of_row, k.stage.residual, k.stage.cost, k.stage.best, k.stage.best_cost));
    } else if (post) HIP_TRY(prhf::launch_residual(k.vh_dev, k.stage.obs, n_prof, (int)n_freq, k.stage.residual, k.stage.cost, c->stream));
    if (timed_launch) {
        HIP_TRY(hipEventRecord(c->pending_end_ev(), c->stream));
        c->mark_timed();
    }
    c->status_pending = true;
    return download_and_sync(k);
}

// A large batch from HOST buffers (a NumPy caller with an ensemble): uploaded whole in front of one launch, the
// transfers - pageable memory, 10 - 30 GB/s - stood in front of and behind the kernel: 56.9 ms per call for a 41.2 ms
// kernel on config 4's shard (BENCH_r03 `host_buffers`).  Here the profiles go in three slabs of 10 %, 30 % and 60 %:
// slab k + 1 is uploaded (stream `up_stream`) while slab k is evaluated (the context's stream, through run() on the
// staged rows as device-resident input), and slab k's result rows travel back (`down_stream`) while slab k + 1 runs.
// A growing slab size keeps the first kernel's wait short and every later upload behind a kernel that is about as long.
// Values do not depend on the cut: a launch's rows do not depend on their neighbours (tests/test_gpu_full_size.py).
int run_host_slabs(prhf_ctx* c, const OperatorInputs& in, double* out) {
    const int64_t n_freq = in.n_freq, n_prof = in.n_prof, n_alt = in.n_alt, prof_stride = in.prof_stride, alt_stride = in.alt_stride;
    const int32_t n_points = in.n_points;
    const bool shared_field = in.shared_field();
    ENTER_DEVICE(c->device);
    const size_t row_bytes = (size_t)n_alt * 8;
    int rc;
    OperatorBlock b;
    double* d_out = nullptr;
    PRHF_TRY(carve(c, c->arena, [&](Stager& k) {
        b = operator_block(k, in.shape((size_t)n_points));
        d_out = k.take<double>((size_t)n_prof * (size_t)n_freq);
    }));
    // the arena may still be read by an earlier asynchronous launch of this context: the uploads wait for it
    HIP_TRY(hipEventRecord(c->slab_free, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->up_stream, c->slab_free, 0));
    HIP_TRY(hipMemcpyAsync(b.freq, in.freq, (size_t)n_freq * 8, hipMemcpyHostToDevice, c->up_stream));
    HIP_TRY(hipMemcpyAsync(b.mult, in.mult, (size_t)n_points * 8, hipMemcpyHostToDevice, c->up_stream));
    if (!alt_stride) HIP_TRY(hipMemcpyAsync(b.alt, in.alt, row_bytes, hipMemcpyHostToDevice, c->up_stream));
    if (shared_field) {
        HIP_TRY(hipMemcpyAsync(b.bmag, in.bmag, row_bytes, hipMemcpyHostToDevice, c->up_stream));
        HIP_TRY(hipMemcpyAsync(b.bpsi, in.bpsi, row_bytes, hipMemcpyHostToDevice, c->up_stream));
    }
    const int n_slabs = 3;
    const int64_t cut[4] = {0, std::max<int64_t>(1, n_prof / 10), std::max<int64_t>(2, (n_prof * 4) / 10), n_prof};
    const uint32_t dev_flags = PRHF_FLAG_DEVICE_PTRS | PRHF_FLAG_ASYNC | (shared_field ? PRHF_FLAG_SHARED_FIELD : 0);
    int first_error = PRHF_OK;
    for (int k = 0; k < n_slabs && first_error == PRHF_OK; ++k) {
        const int64_t p0 = cut[k], rows = cut[k + 1] - cut[k];
        if (rows <= 0) continue;
        auto up2d = [&](double* dst, const double* src, int64_t stride) {
            return hipMemcpy2DAsync(dst + (size_t)p0 * n_alt, row_bytes, src + (size_t)p0 * stride, (size_t)stride * 8, row_bytes,
                                    (size_t)rows, hipMemcpyHostToDevice, c->up_stream);
        };
        HIP_TRY(up2d(b.den, in.den, prof_stride));
        if (!shared_field) {
            HIP_TRY(up2d(b.bmag, in.bmag, prof_stride));
            HIP_TRY(up2d(b.bpsi, in.bpsi, prof_stride));
        }
        if (alt_stride) HIP_TRY(up2d(b.alt, in.alt, alt_stride));
        HIP_TRY(hipEventRecord(c->slab_up[k], c->up_stream));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->slab_up[k], 0));
        const size_t at = (size_t)p0 * n_alt;
        const prhf_segment seg = whole_batch(rows, in.mode, n_points);
        const size_t field_at = shared_field ? 0 : at, alt_at = alt_stride ? at : 0;
        const OperatorInputs slab = {b.freq, n_freq, b.den + at, b.bmag + field_at, b.bpsi + field_at, b.alt + alt_at, rows, n_alt, n_alt,
                                     alt_stride ? n_alt : 0, b.mult, n_points, in.mode, dev_flags};
        rc = run(c, slab, OperatorWork{n_points, &seg, 1, d_out + (size_t)p0 * n_freq, nullptr});
        if (rc != PRHF_OK) { first_error = rc; break; }
        HIP_TRY(hipEventRecord(c->slab_done[k], c->stream));
        // the rows of the slab before this one go home while this one runs (issued here, behind this slab's upload:
        // a copy from or to pageable memory holds the calling thread, and the upload is what the next kernel waits for)
        if (k > 0) {
            HIP_TRY(hipStreamWaitEvent(c->down_stream, c->slab_done[k - 1], 0));
            HIP_TRY(hipMemcpyAsync(out + (size_t)cut[k - 1] * n_freq, d_out + (size_t)cut[k - 1] * n_freq,
                                   (size_t)(cut[k] - cut[k - 1]) * n_freq * 8, hipMemcpyDeviceToHost, c->down_stream));
        }
    }
    if (first_error == PRHF_OK) {
        HIP_TRY(hipStreamWaitEvent(c->down_stream, c->slab_done[n_slabs - 1], 0));
        HIP_TRY(hipMemcpyAsync(out + (size_t)cut[n_slabs - 1] * n_freq, d_out + (size_t)cut[n_slabs - 1] * n_freq,
                               (size_t)(cut[n_slabs] - cut[n_slabs - 1]) * n_freq * 8, hipMemcpyDeviceToHost, c->down_stream));
    }
    HIP_TRY(hipStreamSynchronize(c->up_stream));
    const int rc_sync = prhf_sync(c);                  // the context's stream + the launches' status words
    HIP_TRY(hipStreamSynchronize(c->down_stream));
    return first_error != PRHF_OK ? first_error : rc_sync;
}

}  // namespace

extern "C" {

int prhf_abi_version(void) { return PRHF_ABI_VERSION; }

const char* prhf_last_error(void) { return g_err.c_str(); }

int prhf_device_count(int* n) {
    if (!n) return fail(PRHF_EINVAL, "null pointer");
    *n = 0;
    HIP_TRY(hipGetDeviceCount(n));
    return PRHF_OK;
}

int prhf_ctx_create(int device, prhf_ctx** out) {
    if (!out) return fail(PRHF_EINVAL, "null pointer");
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(PRHF_EINVAL, "device %d not in [0, %d)", device, n);
    ENTER_DEVICE(device);
    prhf_ctx* c = new (std::nothrow) prhf_ctx;
    if (!c) return fail(PRHF_ENOMEM, "out of host memory");
    c->device = device;
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->join_ev, hipEventDisableTiming)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->down_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->slab_free, hipEventDisableTiming)) != hipSuccess ||
        (e = create_events_untimed(c->slab_up, 3)) != hipSuccess ||
        (e = create_events_untimed(c->slab_done, 3)) != hipSuccess ||
        (e = create_events(c->ring0, prhf_ctx::kTimingRing)) != hipSuccess ||
        (e = create_events(c->ring1, prhf_ctx::kTimingRing)) != hipSuccess ||
        (e = hipMalloc(reinterpret_cast<void**>(&c->d_status), kStatusWords * sizeof(unsigned))) != hipSuccess ||
        (e = hipHostMalloc(reinterpret_cast<void**>(&c->h_status), PRHF_STATUS_WORDS * sizeof(unsigned),
                           hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess ||
        (e = hipHostGetDevicePointer(reinterpret_cast<void**>(&c->h_status_dev), c->h_status, 0)) != hipSuccess ||
        (e = hipMemset(c->d_status, 0, kStatusWords * sizeof(unsigned))) != hipSuccess ||
        (e = hipHostMalloc(reinterpret_cast<void**>(&c->h_pack), kPackBytes, hipHostMallocMapped | hipHostMallocCoherent)) !=
            hipSuccess ||
        (e = hipHostGetDevicePointer(reinterpret_cast<void**>(&c->h_pack_dev), c->h_pack, 0)) != hipSuccess ||
        (e = hipMalloc(reinterpret_cast<void**>(&c->d_words), 2 * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipHostMalloc(reinterpret_cast<void**>(&c->h_words), 2 * sizeof(unsigned long long),
                           hipHostMallocDefault)) != hipSuccess ||
        (e = hipMalloc(reinterpret_cast<void**>(&c->d_plan_counters), prhf::kPlanCounterWords * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipMemset(c->d_plan_counters, 0, prhf::kPlanCounterWords * sizeof(unsigned long long))) != hipSuccess ||
        (e = prhf::configure_kernels(staged_lds_bytes(kMaxAlt), kStreamLdsMax)) != hipSuccess) {
        prhf_ctx_destroy(c);
        return fail(PRHF_EHIP, "context setup failed: %s", hipGetErrorString(e));
    }
    c->stream = c->own_stream;
    std::memset(c->h_status, 0, PRHF_STATUS_WORDS * sizeof(unsigned));
#ifdef PRHF_DIAG
    // diagnostics build only: PRHF_<OPTION NAME IN CAPITALS>=value presets the options of every new context
    for (const KnobName& k : kKnobNames) {
        std::string env = "PRHF_";
        for (const char* p = k.name; *p; ++p) env += (char)std::toupper((unsigned char)*p);
        if (const char* v = std::getenv(env.c_str())) c->knobs.*(k.field) = std::min(k.hi, std::max(k.lo, std::atof(v)));
    }
#endif
    (void)hipDeviceGetAttribute(&c->cu_count, hipDeviceAttributeMultiprocessorCount, device);
    if (hipDeviceGetAttribute(&c->large_bar, hipDeviceAttributeIsLargeBar, device) != hipSuccess) c->large_bar = 0;
    if (c->cu_count < 1) c->cu_count = 256;
    *out = c;
    return PRHF_OK;
}

int prhf_ctx_destroy(prhf_ctx* c) {
    if (!c) return PRHF_OK;
    DeviceScope device_scope_(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->arena.p) (void)hipFree(c->arena.p);
    if (c->partial.p) (void)hipFree(c->partial.p);
    if (c->altmin.p) (void)hipFree(c->altmin.p);
    if (c->pairs.p) (void)hipFree(c->pairs.p);
    if (c->ftab.p) (void)hipFree(c->ftab.p);
    if (c->levels.p) (void)hipFree(c->levels.p);
    if (c->ptab.p) (void)hipFree(c->ptab.p);
    if (c->leftover.p) (void)hipFree(c->leftover.p);
    if (c->leftover_x.p) (void)hipFree(c->leftover_x.p);
    if (c->leftover_tall.p) (void)hipFree(c->leftover_tall.p);
    if (c->leftover_tall_x.p) (void)hipFree(c->leftover_tall_x.p);
    if (c->order.p) (void)hipFree(c->order.p);
    if (c->tall.p) (void)hipFree(c->tall.p);
    if (c->vjp.p) (void)hipFree(c->vjp.p);
    if (c->fields.p) (void)hipFree(c->fields.p);
    for (int g = 0; g < c->n_host_grids; ++g) {
        if (c->host_grid[g].mult.p) (void)hipFree(c->host_grid[g].mult.p);
        if (c->host_grid[g].pairs.p) (void)hipFree(c->host_grid[g].pairs.p);
    }
    if (c->d_status) (void)hipFree(c->d_status);
    if (c->h_status) (void)hipHostFree(c->h_status);
    if (c->h_pack) (void)hipHostFree(c->h_pack);
    if (c->d_words) (void)hipFree(c->d_words);
    if (c->h_words) (void)hipHostFree(c->h_words);
    if (c->d_plan_counters) (void)hipFree(c->d_plan_counters);
    for (int i = 0; i < prhf_ctx::kTimingRing; ++i) {
        if (c->ring0[i]) (void)hipEventDestroy(c->ring0[i]);
        if (c->ring1[i]) (void)hipEventDestroy(c->ring1[i]);
    }
    if (c->aux_stream) { (void)hipStreamSynchronize(c->aux_stream); (void)hipStreamDestroy(c->aux_stream); }
    if (c->up_stream) { (void)hipStreamSynchronize(c->up_stream); (void)hipStreamDestroy(c->up_stream); }
    if (c->down_stream) { (void)hipStreamSynchronize(c->down_stream); (void)hipStreamDestroy(c->down_stream); }
    for (int i = 0; i < 3; ++i) {
        if (c->slab_up[i]) (void)hipEventDestroy(c->slab_up[i]);
        if (c->slab_done[i]) (void)hipEventDestroy(c->slab_done[i]);
    }
    if (c->slab_free) (void)hipEventDestroy(c->slab_free);
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    if (c->join_ev) (void)hipEventDestroy(c->join_ev);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return PRHF_OK;
}

int prhf_ctx_set_stream(prhf_ctx* c, void* hip_stream, int32_t borrow) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    // a borrowed NULL is the legacy default stream (what torch reports for its default stream)
    hipStream_t next = borrow ? static_cast<hipStream_t>(hip_stream) : c->own_stream;
    if (next == c->stream) return PRHF_OK;
    ENTER_DEVICE(c->device);
    // Scratch buffers are reused across launches: work on the new stream must come after the last launch on
    // the old one.  Ordered through the event recorded behind that launch, not by synchronising the old
    // stream - a borrowed stream may have been destroyed by its owner since.
    if (c->timed) HIP_TRY(hipStreamWaitEvent(next, c->end_ev(), 0));
    c->stream = next;
    return PRHF_OK;
}

int prhf_ctx_set_option(prhf_ctx* c, const char* name, double value) {
    if (!c || !name) return fail(PRHF_EINVAL, "null pointer");
    for (const KnobName& k : kKnobNames)
        if (std::strcmp(k.name, name) == 0) {
            if (!(value >= k.lo && value <= k.hi))
                return fail(PRHF_EINVAL, "option %s: %g outside [%g, %g]", name, value, k.lo, k.hi);
            c->knobs.*(k.field) = value;
            return PRHF_OK;
        }
    return fail(PRHF_EINVAL, "unknown option '%s'", name);
}

int prhf_ctx_set_math(prhf_ctx* c, int level) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (level != PRHF_MATH_FAITHFUL && level != PRHF_MATH_FAST && level != PRHF_MATH_AUTO)
        return fail(PRHF_EINVAL, "unknown math tier");
    c->math = level;
    return PRHF_OK;
}

int prhf_vfo_batch_f64(prhf_ctx* ctx, const double* freq_mhz, int64_t n_freq, const double* den,
                       const double* bmag, const double* bpsi, const double* alt, int64_t n_prof, int64_t n_alt,
                       int64_t prof_stride_elems, int64_t alt_stride_elems, const double* multiplier,
                       int32_t n_points, int32_t mode, double* vh_out, uint32_t flags) {
    const OperatorInputs in{freq_mhz, n_freq, den, bmag, bpsi, alt, n_prof, n_alt, prof_stride_elems, alt_stride_elems,
                            multiplier, n_points, mode, flags};
    const prhf_segment seg = whole_batch(n_prof, mode, n_points);
    // a large batch from host buffers: in slabs, transfers beside the kernels (run_host_slabs).  The checks of run()
    // that concern the whole call are made by its first slab; a call that a check part refuses is left to run(), which
    // refuses it in its own order.
    const bool large_host = ctx && !in.dev() && ctx->knobs.host_slabs >= 3 && n_prof >= 64 &&
                            (size_t)n_prof * (size_t)n_alt * 24 >= kSlabMinBytes;
    if (large_host && check_arrays(ctx, in, vh_out != nullptr) == PRHF_OK && check_shape(in, true) == PRHF_OK &&
        (mode == PRHF_MODE_O || mode == PRHF_MODE_X) && check_flags(in) == PRHF_OK) {
        PRHF_TRY(check_grid(multiplier, n_points, &seg, 1));
        return run_host_slabs(ctx, in, vh_out);
    }
    return run(ctx, in, OperatorWork{n_points, &seg, 1, vh_out, nullptr});
}

int prhf_vfo_worklist_f64(prhf_ctx* ctx, const double* freq_mhz, int64_t n_freq, const double* den,
                          const double* bmag, const double* bpsi, const double* alt, int64_t n_prof,
                          int64_t n_alt, int64_t prof_stride_elems, int64_t alt_stride_elems,
                          const double* multiplier, int64_t multiplier_len, const prhf_segment* segs,
                          int32_t n_segs, double* vh_out, uint32_t flags) {
    const OperatorInputs in{freq_mhz, n_freq, den, bmag, bpsi, alt, n_prof, n_alt, prof_stride_elems, alt_stride_elems,
                            multiplier, 0, 0, flags};
    return run(ctx, in, OperatorWork{multiplier_len, segs, n_segs, vh_out, nullptr});
}

}  // extern "C"
// The entry points below have C linkage from their declarations in prhf.h (the templates among the shared steps need
// C++ linkage).  A new entry point defined below must be declared there first: without the declaration it is exported
// under a mangled name, which pyrayhf_amd/_native.py reports when it loads the library.

namespace {

// ---- The tracer and derivative entry points ----

// Host-side range check of an index array
int check_index(const char* name, const int64_t* idx, int64_t n, const char* limit_name, int64_t limit) {
    for (int64_t i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= limit)
            return fail(PRHF_EINVAL, "%s[%lld] outside [0, %s)", name, (long long)i, limit_name);
    return PRHF_OK;
}

// A host scan grid: strictly increasing (a NaN fails the test); lone_finite: a grid of one elevation holds a finite one
int check_scan_grid(const double* scan_elevation_deg, int64_t n_scan, bool lone_finite) {
    for (int64_t i = 0; i + 1 < n_scan; ++i)
        if (!(scan_elevation_deg[i + 1] > scan_elevation_deg[i]))
            return fail(PRHF_EINVAL, "scan_elevation_deg must be strictly increasing");
    if (lone_finite && n_scan == 1 && !std::isfinite(scan_elevation_deg[0]))
        return fail(PRHF_EINVAL, "scan_elevation_deg must be finite");
    return PRHF_OK;
}

// What the derivative entry points check alike; others_given: the arrays of their own are there
int derivative_check(prhf_ctx* c, const OperatorInputs& in, bool others_given) {
    PRHF_TRY(check_arrays(c, in, others_given));
    PRHF_TRY(check_shape(in, true));
    if (in.mode != PRHF_MODE_O && in.mode != PRHF_MODE_X) return fail(PRHF_EINVAL, "mode must be 'O' or 'X'");
    PRHF_TRY(check_flags(in));
    const prhf_segment seg = whole_batch(in.n_prof, in.mode, in.n_points);
    return in.dev() ? PRHF_OK : check_grid(in.mult, in.n_points, &seg, 1);
}

// Levels to stage: the whole column where `plan` (plan_vjp or plan_jvp of prhf_plan.h on this call's shape) takes it;
// else up to the highest density peak of the launch; refused there too: the planner's text.
template <class Planner>
int levels_to_stage(prhf_ctx* c, const OperatorInputs& in, Planner plan, long long* levels) {
    char why[256];
    *levels = in.n_alt;
    if (plan(*levels, why, sizeof why) == PRHF_OK) return PRHF_OK;
    long long max_peak = 0;
    PRHF_TRY(highest_peak(c, in.den, in.n_prof, in.n_alt, in.prof_stride, in.dev(), &max_peak));
    *levels = max_peak + 1;
    if (plan(*levels, why, sizeof why) != PRHF_OK) return fail(PRHF_EINVAL, "%s", why);
    return PRHF_OK;
}

// vh_out of a derivative call: the operator's own launch on the same arguments
int operator_launch(prhf_ctx* c, const OperatorInputs& in, double* vh_out) {
    return prhf_vfo_batch_f64(c, in.freq, in.n_freq, in.den, in.bmag, in.bpsi, in.alt, in.n_prof, in.n_alt, in.prof_stride,
                              in.alt_stride, in.mult, in.n_points, in.mode, vh_out, in.flags);
}

// The fields VjpArgs and JvpArgs share.  Host buffers: the six inputs go to the head of c->vjp, packed, and `rest`
// carves what the caller keeps behind them (its own input, the result).
template <class Args, class Rest>
int stage_derivative(prhf_ctx* c, const OperatorInputs& in, long long levels, Args& a, Rest rest) {
    std::memset(&a, 0, sizeof a);
    a.n_prof = in.n_prof; a.n_freq = in.n_freq; a.n_alt = in.n_alt; a.lds_levels = levels; a.n_points = in.n_points;
    a.mode = in.mode == PRHF_MODE_O ? PRHF_KMODE_O : PRHF_KMODE_X;
    a.status = c->h_status_dev;
    if (in.dev()) {
        a.freq = in.freq; a.den = in.den; a.bmag = in.bmag; a.bpsi = in.bpsi; a.alt = in.alt; a.mult = in.mult;
        a.prof_stride = in.prof_stride;
        a.field_stride = in.shared_field() ? 0 : in.prof_stride;
        a.alt_stride = in.alt_stride;
        return PRHF_OK;
    }
    const OperatorShape s = in.shape((size_t)in.n_points);
    PRHF_TRY(carve(c, c->vjp, [&](Stager& k) {
        const OperatorBlock b = operator_block(k, s);
        k.put(b.freq, in.freq, s.n_freq);
        k.put_rows(b.den, in.den, s.n_alt, s.n_prof, in.prof_stride);
        k.put_rows(b.bmag, in.bmag, s.n_alt, s.field_rows, in.prof_stride);
        k.put_rows(b.bpsi, in.bpsi, s.n_alt, s.field_rows, in.prof_stride);
        k.put_rows(b.alt, in.alt, s.n_alt, s.alt_rows, in.alt_stride);
        k.put(b.mult, in.mult, s.mult_len);
        a.freq = b.freq; a.den = b.den; a.bmag = b.bmag; a.bpsi = b.bpsi; a.alt = b.alt; a.mult = b.mult;
        rest(k);
    }));
    a.prof_stride = in.n_alt;
    a.field_stride = in.shared_field() ? 0 : in.n_alt;
    a.alt_stride = in.alt_stride ? in.n_alt : 0;
    return PRHF_OK;
}

// prhf_vfo_jacobian_f64 / prhf_vfo_vjp_f64: check, find the levels to stage, plan (plan_vjp, prhf_plan.h), stage host
// buffers, launch.
int vjp_run(prhf_ctx* c, const OperatorInputs& in, const double* grad_vh, double* vh_out, double* out, bool jacobian) {
    PRHF_TRY(derivative_check(c, in, out && (jacobian || grad_vh)));
    ENTER_DEVICE(c->device);
    VjpPlan pl;
    long long levels = in.n_alt;
    auto plan = [&](long long lv, char* why, size_t n) { return plan_vjp(in.n_prof, in.n_freq, lv, jacobian, pl, why, n); };
    if (in.n_prof > 0) PRHF_TRY(levels_to_stage(c, in, plan, &levels));
    if (vh_out) PRHF_TRY(operator_launch(c, in, vh_out));
    if (in.n_prof == 0) return PRHF_OK;
    const size_t P = (size_t)in.n_prof, F = (size_t)in.n_freq, A = (size_t)in.n_alt;
    const size_t out_elems = jacobian ? P * F * A : P * A, pf = jacobian ? 0 : P * F;
    prhf::VjpArgs a;
    double* d_g = nullptr;
    double* d_out = out;
    PRHF_TRY(stage_derivative(c, in, levels, a, [&](Stager& k) {
        d_g = k.take<double>(pf);
        d_out = k.take<double>(out_elems);
    }));
    if (!in.dev() && pf) HIP_TRY(upload(c, d_g, grad_vh, pf * 8));
    a.grad_vh = in.dev() ? grad_vh : d_g;
    a.out = d_out;
    a.waves = pl.waves;
    PRHF_TRY(timed_launch(c, true, [&] { return prhf::launch_vfo_vjp(a, jacobian, pl.lds_bytes, c->stream); }));
    if (!in.dev()) HIP_TRY(download(c, out, d_out, out_elems * 8));
    if (in.flags & PRHF_FLAG_ASYNC) return PRHF_OK;
    return prhf_sync(c);
}

// prhf_vfo_jvp_f64: as vjp_run with plan_jvp, then one launch per chunk of tangents
int jvp_run(prhf_ctx* c, const OperatorInputs& in, const double* tangents, int64_t n_tan, int64_t tan_stride, double* vh_out,
            double* out) {
    PRHF_TRY(derivative_check(c, in, n_tan <= 0 || (tangents && out)));
    if (n_tan < 0 || n_tan > (1 << 20)) return fail(PRHF_EINVAL, "bad number of tangents");
    if (tan_stride != 0 && tan_stride < n_tan * in.n_alt)
        return fail(PRHF_EINVAL, "tangent stride shorter than a profile's tangents");
    ENTER_DEVICE(c->device);
    JvpPlan pl;
    long long levels = in.n_alt;
    auto plan = [&](long long lv, char* why, size_t n) { return plan_jvp(in.n_prof, in.n_freq, lv, n_tan, pl, why, n); };
    if (n_tan > 0 && in.n_prof > 0) PRHF_TRY(levels_to_stage(c, in, plan, &levels));
    if (vh_out) PRHF_TRY(operator_launch(c, in, vh_out));
    if (in.n_prof == 0 || n_tan == 0) return PRHF_OK;
    const size_t out_elems = (size_t)in.n_prof * (size_t)in.n_freq * (size_t)n_tan;
    const size_t tan_sets = tan_stride ? (size_t)in.n_prof : 1, set_elems = (size_t)n_tan * (size_t)in.n_alt;
    prhf::JvpArgs a;
    double* d_tan = nullptr;
    double* d_out = out;
    PRHF_TRY(stage_derivative(c, in, levels, a, [&](Stager& k) {
        d_tan = k.take<double>(tan_sets * set_elems);
        d_out = k.take<double>(out_elems);
    }));
    if (!in.dev()) HIP_TRY(upload_rows(c, d_tan, tangents, set_elems, tan_sets, tan_stride));
    const double* const tan0 = in.dev() ? tangents : d_tan;
    a.tan_prof_stride = in.dev() ? tan_stride : (tan_stride ? (long long)set_elems : 0);
    a.out_stride = n_tan;
    PRHF_TRY(timed_launch(c, true, [&] {
        for (long long i = 0; i < pl.n_chunks; ++i) {
            const JvpChunk ch = jvp_chunk(pl, n_tan, i);
            a.tan = tan0 + (size_t)ch.first * (size_t)in.n_alt;
            a.out = d_out + ch.first;
            a.n_tan = ch.count;
            const hipError_t e = prhf::launch_vfo_jvp(a, ch.nt, pl.threads, ch.lds_bytes, c->stream);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }));
    if (!in.dev()) HIP_TRY(download(c, out, d_out, out_elems * 8));
    if (in.flags & PRHF_FLAG_ASYNC) return PRHF_OK;
    return prhf_sync(c);
}

}  // namespace

int prhf_vfo_jacobian_f64(prhf_ctx* ctx, const double* freq_mhz, int64_t n_freq, const double* den, const double* bmag,
                          const double* bpsi, const double* alt, int64_t n_prof, int64_t n_alt, int64_t prof_stride_elems,
                          int64_t alt_stride_elems, const double* multiplier, int32_t n_points, int32_t mode, double* vh_out,
                          double* jac_out, uint32_t flags) {
    const OperatorInputs in{freq_mhz, n_freq, den, bmag, bpsi, alt, n_prof, n_alt, prof_stride_elems, alt_stride_elems,
                            multiplier, n_points, mode, flags};
    return vjp_run(ctx, in, nullptr, vh_out, jac_out, true);
}

int prhf_vfo_vjp_f64(prhf_ctx* ctx, const double* freq_mhz, int64_t n_freq, const double* den, const double* bmag,
                     const double* bpsi, const double* alt, int64_t n_prof, int64_t n_alt, int64_t prof_stride_elems,
                     int64_t alt_stride_elems, const double* multiplier, int32_t n_points, int32_t mode, const double* grad_vh,
                     double* vh_out, double* grad_den_out, uint32_t flags) {
    const OperatorInputs in{freq_mhz, n_freq, den, bmag, bpsi, alt, n_prof, n_alt, prof_stride_elems, alt_stride_elems,
                            multiplier, n_points, mode, flags};
    return vjp_run(ctx, in, grad_vh, vh_out, grad_den_out, false);
}

int prhf_vfo_jvp_f64(prhf_ctx* ctx, const double* freq_mhz, int64_t n_freq, const double* den, const double* bmag,
                     const double* bpsi, const double* alt, int64_t n_prof, int64_t n_alt, int64_t prof_stride_elems,
                     int64_t alt_stride_elems, const double* multiplier, int32_t n_points, int32_t mode, const double* tangents,
                     int64_t n_tan, int64_t tan_prof_stride_elems, double* vh_out, double* dvh_out, uint32_t flags) {
    const OperatorInputs in{freq_mhz, n_freq, den, bmag, bpsi, alt, n_prof, n_alt, prof_stride_elems, alt_stride_elems,
                            multiplier, n_points, mode, flags};
    return jvp_run(ctx, in, tangents, n_tan, tan_prof_stride_elems, vh_out, dvh_out);
}

namespace {

static_assert(PRHF_LM_RUNNING == prhf_lm::kRunning && PRHF_LM_CONVERGED_F == prhf_lm::kConvergedF &&
              PRHF_LM_CONVERGED_X == prhf_lm::kConvergedX && PRHF_LM_SINGULAR == prhf_lm::kSingular &&
              PRHF_LM_NO_DATA == prhf_lm::kNoData && PRHF_LM_NO_COST == prhf_lm::kNoCost &&
              PRHF_LM_MAX_TANGENTS == prhf_lm::kMaxT, "prhf.h and prhf_lm_step.h name the same statuses");

// What prhf_vfo_lm_fit_f64 fits with and where its results go
struct LmProblem {
    const double* basis;
    int64_t n_tan, basis_stride;
    const double *vh_obs, *c0, *prior;
    prhf_lm_options opt;
    double *c, *cost;
    int32_t *status, *n_eval, *n_accept;
    double *lambda, *den, *vh, *history, *state;
};

int check_lm_options(const prhf_lm_options& o) {
    if (o.max_iter < 1 || o.max_iter > (1 << 20))
        return fail(PRHF_EINVAL, "max_iter %d outside [1, %d]", (int)o.max_iter, 1 << 20);
    if (!(o.lambda0 > 0.0 && o.lambda0 < HUGE_VAL)) return fail(PRHF_EINVAL, "lambda0 must be positive and finite");
    if (!(o.lambda_up > 1.0 && o.lambda_up < HUGE_VAL)) return fail(PRHF_EINVAL, "lambda_up must be greater than 1 and finite");
    if (!(o.lambda_down >= 1.0 && o.lambda_down < HUGE_VAL)) return fail(PRHF_EINVAL, "lambda_down must be at least 1 and finite");
    if (!(o.step_max > 0.0)) return fail(PRHF_EINVAL, "step_max must be positive");
    if (!(o.ftol >= 0.0) || !(o.xtol >= 0.0)) return fail(PRHF_EINVAL, "ftol and xtol must not be negative");
    return PRHF_OK;
}

// prhf_vfo_lm_fit_f64: check; carve the arena (host buffers: inputs and results too) and upload once; per evaluation
// the trial columns, jvp_run on them - the operator's launch and the JVP's, asynchronous on device pointers - and the
// step; the column at the result; download once; one synchronisation.  `in`: the operator's arguments with den0 as den
// and den0's stride (0: one column) as prof_stride.
int lm_run(prhf_ctx* c, const OperatorInputs& in, const LmProblem& q) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (q.n_tan < 1 || q.n_tan > PRHF_LM_MAX_TANGENTS)
        return fail(PRHF_EINVAL, "n_tan %lld outside [1, %d]: the basis goes through the JVP kernel in one pass", (long long)q.n_tan,
                    PRHF_LM_MAX_TANGENTS);
    const bool outputs = q.c && q.cost && q.status && q.n_eval && q.n_accept && q.lambda && q.den && q.vh;
    PRHF_TRY(check_arrays(c, in, q.basis && q.vh_obs && outputs));
    if (in.n_freq < 1 || in.n_prof < 0 || in.n_alt < 1 || in.n_points < 1) return fail(PRHF_EINVAL, "bad shape");
    if (in.n_alt > kMaxAltTall)
        return fail(PRHF_EINVAL, "n_alt %lld exceeds the limit of %lld levels", (long long)in.n_alt, kMaxAltTall);
    if (in.n_freq > (1 << 20) || in.n_prof > 0x7fffffffLL) return fail(PRHF_EINVAL, "n_freq or n_iono too large");
    if ((in.prof_stride != 0 && in.prof_stride < in.n_alt) || (in.alt_stride != 0 && in.alt_stride < in.n_alt) ||
        (q.basis_stride != 0 && q.basis_stride < q.n_tan * in.n_alt))
        return fail(PRHF_EINVAL, "row stride shorter than a row");
    if (in.mode != PRHF_MODE_O && in.mode != PRHF_MODE_X) return fail(PRHF_EINVAL, "mode must be 'O' or 'X'");
    PRHF_TRY(check_flags(in));
    PRHF_TRY(check_lm_options(q.opt));
    const bool dev = in.dev();
    if (!dev) {
        const prhf_segment seg = whole_batch(in.n_prof, in.mode, in.n_points);
        PRHF_TRY(check_grid(in.mult, in.n_points, &seg, 1));
        if (q.prior)
            for (int64_t t = 0; t < q.n_tan; ++t)
                if (!(q.prior[t] >= 0.0 && q.prior[t] < HUGE_VAL))
                    return fail(PRHF_EINVAL, "prior_weight[%lld] is negative or not finite", (long long)t);
    }
    std::fill(c->lm_counters, c->lm_counters + PRHF_LM_FIT_COUNTERS, 0);
    if (in.n_prof == 0) return PRHF_OK;
    ENTER_DEVICE(c->device);
    const uint64_t waits0 = c->host_waits;
    const unsigned long long timed0 = c->n_timed;

    const size_t I = (size_t)in.n_prof, F = (size_t)in.n_freq, A = (size_t)in.n_alt, T = (size_t)q.n_tan, NA = T * (T + 1) / 2;
    const size_t n_iter = (size_t)q.opt.max_iter, state_elems = T * T + 2 * T;
    const size_t den0_rows = in.prof_stride ? I : 1, field_rows = in.shared_field() ? 1 : I, alt_rows = in.alt_stride ? I : 1;
    const size_t basis_sets = q.basis_stride ? I : 1;
    // the inputs and results on the device: the caller's own, or the arena's copies
    OperatorInputs d = in;
    LmProblem r = q;
    double *den = nullptr, *tan = nullptr, *vh_eval = nullptr, *dvh = nullptr, *c_eval = nullptr, *nA = nullptr, *g = nullptr,
           *delta = nullptr;
    PRHF_TRY(carve(c, c->arena, [&](Stager& k) {
        den = k.take<double>(I * A);
        tan = k.take<double>(I * T * A);
        vh_eval = k.take<double>(I * F);
        dvh = k.take<double>(I * F * T);
        c_eval = k.take<double>(I * T);
        nA = k.take<double>(I * NA);
        g = k.take<double>(I * T);
        delta = k.take<double>(I * T);
        if (dev) return;
        double* p;
        k.put(p = k.take<double>(F), in.freq, F); d.freq = p;
        k.put_rows(p = k.take<double>(den0_rows * A), in.den, A, den0_rows, in.prof_stride); d.den = p;
        k.put_rows(p = k.take<double>(field_rows * A), in.bmag, A, field_rows, (int64_t)A); d.bmag = p;
        k.put_rows(p = k.take<double>(field_rows * A), in.bpsi, A, field_rows, (int64_t)A); d.bpsi = p;
        k.put_rows(p = k.take<double>(alt_rows * A), in.alt, A, alt_rows, in.alt_stride); d.alt = p;
        k.put(p = k.take<double>((size_t)in.n_points), in.mult, (size_t)in.n_points); d.mult = p;
        k.put_rows(p = k.take<double>(basis_sets * T * A), q.basis, T * A, basis_sets, q.basis_stride); r.basis = p;
        k.put(p = k.take<double>(I * F), q.vh_obs, I * F); r.vh_obs = p;
        r.prior = k.put<double>(q.prior, q.prior ? T : 0);
        r.c = k.take<double>(I * T);
        r.cost = k.take<double>(I);
        r.lambda = k.take<double>(I);
        r.den = k.take<double>(I * A);
        r.vh = k.take<double>(I * F);
        r.history = k.take<double>(q.history ? I * n_iter : 0);
        r.state = k.take<double>(q.state ? I * state_elems : 0);
        r.status = k.take<int32_t>(I);
        r.n_eval = k.take<int32_t>(I);
        r.n_accept = k.take<int32_t>(I);
    }));
    if (!dev) {
        if (!q.history) r.history = nullptr;
        if (!q.state) r.state = nullptr;
        d.prof_stride = in.prof_stride ? (int64_t)A : 0;
        d.alt_stride = in.alt_stride ? (int64_t)A : 0;
        r.basis_stride = q.basis_stride ? (int64_t)(T * A) : 0;
    }
    // the start: c0, or zeros (all-zero bytes)
    if (q.c0) HIP_TRY(hipMemcpyAsync(c_eval, q.c0, I * T * 8, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    else HIP_TRY(hipMemsetAsync(c_eval, 0, I * T * 8, c->stream));
    if (r.state) HIP_TRY(hipMemsetAsync(r.state, 0, I * state_elems * 8, c->stream));

    // the operator and the JVP read the trial columns: packed rows of the arena, device pointers, nothing waits
    OperatorInputs trial = d;
    trial.den = den;
    trial.prof_stride = (int64_t)A;
    trial.flags = PRHF_FLAG_DEVICE_PTRS | PRHF_FLAG_ASYNC | (in.flags & PRHF_FLAG_SHARED_FIELD) |
                  (dev ? (in.flags & PRHF_FLAG_GRID_STABLE) : 0u);
    prhf::LmSynthArgs sy = {};
    sy.den0 = d.den; sy.basis = r.basis; sy.c = c_eval; sy.status = nullptr; sy.den = den; sy.tan = tan;
    sy.n_iono = in.n_prof; sy.n_alt = in.n_alt; sy.den0_stride = d.prof_stride; sy.basis_stride = r.basis_stride;
    sy.n_tan = (int)T;
    prhf::LmStepArgs st = {};
    st.vh_obs = r.vh_obs; st.vh_eval = vh_eval; st.dvh = dvh; st.prior = r.prior;
    st.c = r.c; st.c_eval = c_eval; st.A = nA; st.g = g; st.delta = delta; st.cost = r.cost; st.lambda = r.lambda;
    st.status = r.status; st.n_eval = r.n_eval; st.n_accept = r.n_accept;
    st.vh_fit = r.vh; st.history = r.history; st.state_out = r.state;
    st.n_iono = in.n_prof; st.n_freq = (int)F; st.n_tan = (int)T; st.max_iter = q.opt.max_iter;
    st.lambda0 = q.opt.lambda0; st.lambda_up = q.opt.lambda_up; st.lambda_down = q.opt.lambda_down;
    st.step_max = q.opt.step_max; st.ftol = q.opt.ftol; st.xtol = q.opt.xtol;
    for (int k = 0; k < q.opt.max_iter; ++k) {
        sy.frozen = k > 0 ? r.status : nullptr;              // (a frozen ionogram's column and tangents stand from before)
        PRHF_TRY(timed_launch(c, false, [&] { return prhf::launch_lm_synth(sy, c->stream); }));
        PRHF_TRY(jvp_run(c, trial, tan, (int64_t)T, (int64_t)(T * A), vh_eval, dvh));
        st.k = k;
        PRHF_TRY(timed_launch(c, false, [&] { return prhf::launch_lm_step(st, c->stream); }));
        ++c->lm_counters[0];
    }
    sy.c = r.c; sy.status = r.status; sy.frozen = nullptr; sy.den = r.den; sy.tan = nullptr;
    PRHF_TRY(timed_launch(c, false, [&] { return prhf::launch_lm_synth(sy, c->stream); }));
    if (!dev) {
        HIP_TRY(download(c, q.c, r.c, I * T * 8));
        HIP_TRY(download(c, q.cost, r.cost, I * 8));
        HIP_TRY(download(c, q.lambda, r.lambda, I * 8));
        HIP_TRY(download(c, q.den, r.den, I * A * 8));
        HIP_TRY(download(c, q.vh, r.vh, I * F * 8));
        if (q.history) HIP_TRY(download(c, q.history, r.history, I * n_iter * 8));
        if (q.state) HIP_TRY(download(c, q.state, r.state, I * state_elems * 8));
        HIP_TRY(download(c, q.status, r.status, I * 4));
        HIP_TRY(download(c, q.n_eval, r.n_eval, I * 4));
        HIP_TRY(download(c, q.n_accept, r.n_accept, I * 4));
    }
    const int rc = (in.flags & PRHF_FLAG_ASYNC) ? PRHF_OK : prhf_sync(c);
    c->lm_counters[1] = c->n_timed - timed0;
    c->lm_counters[2] = c->host_waits - waits0;
    return rc;
}

}  // namespace

int prhf_vfo_lm_fit_f64(prhf_ctx* ctx, const double* freq_mhz, int64_t n_freq, const double* den0, const double* bmag,
                        const double* bpsi, const double* alt, int64_t n_iono, int64_t n_alt, int64_t den0_stride_elems,
                        int64_t alt_stride_elems, const double* multiplier, int32_t n_points, int32_t mode, const double* basis,
                        int64_t n_tan, int64_t basis_prof_stride_elems, const double* vh_obs, const double* c0,
                        const double* prior_weight, const prhf_lm_options* options, double* c_out, double* cost_out,
                        int32_t* status_out, int32_t* n_eval_out, int32_t* n_accept_out, double* lambda_out, double* den_out,
                        double* vh_out, double* cost_history_out, double* state_out, uint32_t flags) {
    const OperatorInputs in{freq_mhz, n_freq, den0, bmag, bpsi, alt, n_iono, n_alt, den0_stride_elems, alt_stride_elems,
                            multiplier, n_points, mode, flags};
    const prhf_lm_options defaults = {20, 0, 1e-3, 10.0, 10.0, 1.0, 1e-10, 1e-10};
    const LmProblem q = {basis, n_tan, basis_prof_stride_elems, vh_obs, c0, prior_weight, options ? *options : defaults,
                         c_out, cost_out, status_out, n_eval_out, n_accept_out, lambda_out, den_out, vh_out,
                         cost_history_out, state_out};
    return lm_run(ctx, in, q);
}

int prhf_lm_fit_counters(prhf_ctx* c, uint64_t* counters) {
    if (!c || !counters) return fail(PRHF_EINVAL, "null pointer");
    std::copy(c->lm_counters, c->lm_counters + PRHF_LM_FIT_COUNTERS, counters);
    return PRHF_OK;
}

int prhf_vfo_residual_f64(prhf_ctx* ctx, const double* freq_mhz, int64_t n_freq, const double* den,
                          const double* bmag, const double* bpsi, const double* alt, int64_t n_prof,
                          int64_t n_alt, int64_t prof_stride_elems, int64_t alt_stride_elems,
                          const double* multiplier, int32_t n_points, int32_t mode, const double* vh_obs,
                          double* vh_out, double* residual_out, double* cost_out, uint32_t flags) {
    const prhf_segment seg = whole_batch(n_prof, mode, n_points);
    Residual post{vh_obs, residual_out, cost_out};
    const OperatorInputs in{freq_mhz, n_freq, den, bmag, bpsi, alt, n_prof, n_alt, prof_stride_elems, alt_stride_elems,
                            multiplier, n_points, mode, flags};
    return run(ctx, in, OperatorWork{n_points, &seg, 1, vh_out, &post});
}

int prhf_vfo_residual_many_f64(prhf_ctx* ctx, const double* freq_mhz, int64_t n_freq, const double* den,
                               const double* bmag, const double* bpsi, const double* alt, int64_t n_prof,
                               int64_t n_alt, int64_t prof_stride_elems, int64_t alt_stride_elems,
                               const double* multiplier, int32_t n_points, int32_t mode, const double* vh_obs,
                               int64_t n_iono, const int32_t* ionogram_of_row, double* vh_out, double* residual_out,
                               double* cost_out, int64_t* best_out, double* best_cost_out, uint32_t flags) {
    if (!freq_mhz) return fail(PRHF_EINVAL, "null array pointer");
    PRHF_TRY(check_many(freq_mhz, n_freq, n_prof, vh_obs, n_iono, ionogram_of_row, residual_out, cost_out, best_out, best_cost_out,
                        flags));
    const prhf_segment seg = whole_batch(n_prof, mode, n_points);
    Residual post{vh_obs, residual_out, cost_out};
    post.n_iono = n_iono;
    post.ionogram_of_row = ionogram_of_row;
    post.best = best_out;
    post.best_cost = best_cost_out;
    const OperatorInputs in{freq_mhz, n_freq, den, bmag, bpsi, alt, n_prof, n_alt, prof_stride_elems, alt_stride_elems,
                            multiplier, n_points, mode, flags};
    return run(ctx, in, OperatorWork{n_points, &seg, 1, vh_out, &post});
}

// ---- The un-fused stage ops: checks, carve (put the inputs, take the outputs), timed_launch, downloads, tail ----

int prhf_mu_mup_f64(prhf_ctx* c, const double* X, const double* Y, const double* psi_deg, int64_t n,
                    int32_t mode, double* mu_out, double* mup_out, uint32_t flags) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (!X || !Y || !psi_deg || !mu_out || !mup_out) return fail(PRHF_EINVAL, "null array pointer");
    if (n < 0) return fail(PRHF_EINVAL, "bad shape");
    if (mode != PRHF_MODE_O && mode != PRHF_MODE_X) return fail(PRHF_EINVAL, "Mode must be O or X");
    if (flags & ~PRHF_FLAG_DEVICE_PTRS) return fail(PRHF_EINVAL, "unknown flag bits");
    if (n == 0) return PRHF_OK;
    ENTER_DEVICE(c->device);
    const bool dev = (flags & PRHF_FLAG_DEVICE_PTRS) != 0;
    const double* const src[3] = {X, Y, psi_deg};
    double* const dst[2] = {mu_out, mup_out};
    MuMupBlock b = {{mut(X), mut(Y), mut(psi_deg)}, {mu_out, mup_out}};
    if (!dev) PRHF_TRY(carve(c, c->arena, [&](Stager& k) {
        b = mu_mup_block(k, (size_t)n);
        for (int i = 0; i < 3; ++i) k.put(b.in[i], src[i], (size_t)n);
    }));
    PRHF_TRY(timed_launch(c, false, [&] {
        return prhf::launch_mu_mup(b.in[0], b.in[1], b.in[2], n, kmode(mode), c->math == PRHF_MATH_FAST ? 1 : 0, c->d_words,
                                   c->h_words, b.out[0], b.out[1], c->stream);
    }));
    for (int i = 0; i < 2 && !dev; ++i) HIP_TRY(download(c, dst[i], b.out[i], (size_t)n * 8));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PRHF_OK;
}

int prhf_find_vh_f64(prhf_ctx* c, const double* X, const double* Y, const double* psi_deg, const double* dh,
                     int64_t n_rows, int64_t n_cols, double alt_min, int32_t mode, double* vh_out,
                     uint32_t flags) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (!X || !Y || !psi_deg || !dh || !vh_out) return fail(PRHF_EINVAL, "null array pointer");
    if (n_rows < 0 || n_cols < 0) return fail(PRHF_EINVAL, "bad shape");
    if (mode != PRHF_MODE_O && mode != PRHF_MODE_X) return fail(PRHF_EINVAL, "Mode must be O or X");
    if (flags & ~PRHF_FLAG_DEVICE_PTRS) return fail(PRHF_EINVAL, "unknown flag bits");
    if (n_rows == 0) return PRHF_OK;
    ENTER_DEVICE(c->device);
    const bool dev = (flags & PRHF_FLAG_DEVICE_PTRS) != 0;
    const double* const src[4] = {X, Y, psi_deg, dh};
    FindVhBlock b = {{mut(X), mut(Y), mut(psi_deg), mut(dh)}, vh_out};
    if (!dev) PRHF_TRY(carve(c, c->arena, [&](Stager& k) {
        b = find_vh_block(k, (size_t)n_rows, (size_t)n_cols);
        for (int i = 0; i < 4 && n_cols > 0; ++i) k.put(b.in[i], src[i], (size_t)(n_rows * n_cols));
    }));
    PRHF_TRY(timed_launch(c, false, [&] {
        return prhf::launch_find_vh(b.in[0], b.in[1], b.in[2], b.in[3], n_rows, n_cols, alt_min, kmode(mode),
                                    c->math == PRHF_MATH_FAST ? 1 : 0, c->d_words, c->h_words, b.vh, c->stream);
    }));
    if (!dev) HIP_TRY(download(c, vh_out, b.vh, (size_t)n_rows * 8));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PRHF_OK;
}

int prhf_regrid_f64(prhf_ctx* c, const double* freq_hz, int64_t n_freq, const double* den, const double* bmag,
                    const double* bpsi, const double* alt, int64_t n_alt, const double* multiplier,
                    int32_t n_points, int32_t mode, double* out_freq, double* out_den, double* out_bmag,
                    double* out_bpsi, double* out_dist, double* out_alt, double* out_crit, int64_t* out_ind,
                    uint32_t flags) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (!freq_hz || !den || !bmag || !bpsi || !alt || !multiplier || !out_freq || !out_den || !out_bmag ||
        !out_bpsi || !out_dist || !out_alt || !out_crit || !out_ind)
        return fail(PRHF_EINVAL, "null array pointer");
    if (n_freq < 1 || n_alt < 1 || n_alt > kMaxAltTall || n_points < 1) return fail(PRHF_EINVAL, "bad shape");
    if (mode != PRHF_MODE_O && mode != PRHF_MODE_X) return fail(PRHF_EINVAL, "mode must be 'O' or 'X'");
    if (flags & ~PRHF_FLAG_DEVICE_PTRS) return fail(PRHF_EINVAL, "unknown flag bits");
    ENTER_DEVICE(c->device);
    const bool dev = (flags & PRHF_FLAG_DEVICE_PTRS) != 0;
    const size_t fn = (size_t)n_freq * (size_t)n_points;
    // The reference regrids the levels below the density peak only (library.py:371-375).  A column of more levels than
    // LDS holds stages just those, up to its peak (highest_peak: one synchronisation for device memory).  Shorter
    // columns take neither.
    long long levels = n_alt;
    if (n_alt > kMaxAlt) {
        long long peak = 0;
        PRHF_TRY(highest_peak(c, den, 1, n_alt, n_alt, dev, &peak));
        if (peak + 1 > kMaxAlt)
            return fail(PRHF_EINVAL, "regrid stages at most %lld levels up to the density peak (the 1400-level "
                        "bottomside limit); this column's peak is at level %lld", kMaxAlt, peak);
        levels = peak + 1;
    }
    const double* const col[4] = {den, bmag, bpsi, alt};
    double* const host[7] = {out_freq, out_den, out_bmag, out_bpsi, out_dist, out_alt, out_crit};
    RegridBlock b = {mut(freq_hz), {mut(den), mut(bmag), mut(bpsi), mut(alt)}, mut(multiplier),
                     {out_freq, out_den, out_bmag, out_bpsi, out_dist, out_alt, out_crit}, reinterpret_cast<long long*>(out_ind)};
    if (!dev) PRHF_TRY(carve(c, c->arena, [&](Stager& k) {
        b = regrid_block(k, (size_t)n_freq, (size_t)n_alt, (size_t)n_points);
        k.put(b.freq, freq_hz, (size_t)n_freq);
        for (int i = 0; i < 4; ++i) k.put(b.col[i], col[i], (size_t)n_alt);
        k.put(b.mult, multiplier, (size_t)n_points);
    }));
    prhf::RegridArgs a;
    std::memset(&a, 0, sizeof a);
    a.n_freq = n_freq; a.n_alt = n_alt; a.lds_levels = levels; a.n_points = n_points;
    a.mode = kmode(mode);
    a.status = c->h_status_dev;
    a.freq_hz = b.freq; a.den = b.col[0]; a.bmag = b.col[1]; a.bpsi = b.col[2]; a.alt = b.col[3]; a.mult = b.mult;
    a.out_freq = b.out[0]; a.out_den = b.out[1]; a.out_bmag = b.out[2]; a.out_bpsi = b.out[3];
    a.out_dist = b.out[4]; a.out_alt = b.out[5]; a.out_crit = b.out[6];
    a.out_ind = b.ind;
    PRHF_TRY(timed_launch(c, true, [&] { return prhf::launch_regrid(a, staged_lds_bytes(levels), c->stream); }));
    for (int i = 0; i < 7 && !dev; ++i) HIP_TRY(download(c, host[i], b.out[i], fn * 8));
    if (!dev) HIP_TRY(download(c, out_ind, b.ind, fn * 8));
    return prhf_sync(c);
}

int prhf_residual_f64(prhf_ctx* c, const double* vh_model, const double* vh_obs, int64_t n_prof, int64_t n_freq,
                      double* residual_out, double* cost_out, uint32_t flags) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (!vh_model || !vh_obs || (!residual_out && !cost_out)) return fail(PRHF_EINVAL, "null array pointer");
    if (n_prof < 0 || n_freq < 1 || n_freq > (1 << 20)) return fail(PRHF_EINVAL, "bad shape");
    if (flags & ~(PRHF_FLAG_DEVICE_PTRS | PRHF_FLAG_ASYNC | PRHF_FLAG_GRID_STABLE))
        return fail(PRHF_EINVAL, "unknown flag bits");
    const bool dev = (flags & PRHF_FLAG_DEVICE_PTRS) != 0;
    if ((flags & (PRHF_FLAG_ASYNC | PRHF_FLAG_GRID_STABLE)) && !dev)
        return fail(PRHF_EINVAL, "PRHF_FLAG_ASYNC and PRHF_FLAG_GRID_STABLE need device pointers");
    if (n_prof == 0) return PRHF_OK;
    ENTER_DEVICE(c->device);
    const size_t pf = (size_t)n_prof * (size_t)n_freq;
    const double* model = vh_model;
    ResidualBlock b = {mut(vh_obs), residual_out, cost_out};
    if (!dev) PRHF_TRY(carve(c, c->arena, [&](Stager& k) {
        model = k.put<double>(vh_model, pf);
        b = residual_block(k, (size_t)n_freq, pf, (size_t)n_prof);
        k.put(b.obs, vh_obs, (size_t)n_freq);
        if (!residual_out) b.residual = nullptr;
        if (!cost_out) b.cost = nullptr;
    }));
    PRHF_TRY(timed_launch(c, false, [&] {
        return prhf::launch_residual(model, b.obs, n_prof, (int)n_freq, b.residual, b.cost, c->stream);
    }));
    if (!dev && residual_out) HIP_TRY(download(c, residual_out, b.residual, pf * 8));
    if (!dev && cost_out) HIP_TRY(download(c, cost_out, b.cost, (size_t)n_prof * 8));
    if (flags & PRHF_FLAG_ASYNC) return PRHF_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PRHF_OK;
}

int prhf_residual_many_f64(prhf_ctx* c, const double* vh_model, int64_t n_rows, const double* vh_obs, int64_t n_iono,
                           int64_t n_freq, const int32_t* ionogram_of_row, double* residual_out, double* cost_out,
                           int64_t* best_out, double* best_cost_out, uint32_t flags) {
    if (!vh_model) return fail(PRHF_EINVAL, "null array pointer");
    PRHF_TRY(check_many(nullptr, n_freq, n_rows, vh_obs, n_iono, ionogram_of_row, residual_out, cost_out, best_out, best_cost_out,
                        flags));
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (flags & ~(PRHF_FLAG_DEVICE_PTRS | PRHF_FLAG_ASYNC)) return fail(PRHF_EINVAL, "unknown flag bits");
    const bool dev = (flags & PRHF_FLAG_DEVICE_PTRS) != 0;
    if ((flags & PRHF_FLAG_ASYNC) && !dev) return fail(PRHF_EINVAL, "PRHF_FLAG_ASYNC needs device pointers");
    ENTER_DEVICE(c->device);
    const size_t pf = (size_t)n_rows * (size_t)n_freq;
    const size_t cost_elems = many_cost_elems((size_t)n_rows, (size_t)n_iono, ionogram_of_row != nullptr);
    const double* model = vh_model;
    ManyBlock b = {mut(vh_obs), residual_out, cost_out, best_cost_out, best_out, const_cast<int32_t*>(ionogram_of_row)};
    if (!dev) PRHF_TRY(carve(c, c->arena, [&](Stager& k) {
        double* const m = k.take<double>(pf);
        if (pf) k.put(m, vh_model, pf);
        model = m;
        b = many_block(k, (size_t)n_iono, (size_t)n_freq, (size_t)n_rows, residual_out ? pf : 0, ionogram_of_row != nullptr);
        k.put(b.obs, vh_obs, (size_t)n_iono * (size_t)n_freq);
        if (ionogram_of_row && n_rows > 0) k.put(b.ionogram_of_row, ionogram_of_row, (size_t)n_rows);
        else b.ionogram_of_row = const_cast<int32_t*>(ionogram_of_row);
        if (!residual_out) b.residual = nullptr;
    }));
    PRHF_TRY(timed_launch(c, false, [&] {
        return launch_many(c, model, n_rows, b.obs, n_iono, n_freq, b.ionogram_of_row, b.residual, b.cost, b.best, b.best_cost);
    }));
    if (!dev) {
        if (residual_out && pf) HIP_TRY(download(c, residual_out, b.residual, pf * 8));
        if (cost_elems) HIP_TRY(download(c, cost_out, b.cost, cost_elems * 8));
        HIP_TRY(download(c, best_out, b.best, (size_t)n_iono * 8));
        HIP_TRY(download(c, best_cost_out, b.best_cost, (size_t)n_iono * 8));
    }
    if (flags & PRHF_FLAG_ASYNC) return PRHF_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PRHF_OK;
}

namespace {
// ---- The Snell family: prhf_snell_cartesian_f64 .. prhf_snell_muf_f64 ----

struct SnellGeometry {
    int geometry;
    double earth_radius_km, dz_target_km, apex_boost;
    int max_substeps;
};
int check_snell_geometry(int32_t geometry) {
    if (geometry != 0 && geometry != 1) return fail(PRHF_EINVAL, "geometry is 0 (flat Earth) or 1 (spherical Earth)");
    return PRHF_OK;
}
// The four spherical controls, checked where the geometry reads them; a flat Earth takes its defaults
int snell_controls(int32_t geometry, double earth_radius_km, double dz_target_km, double apex_boost, int32_t max_substeps,
                   SnellGeometry* geo) {
    *geo = SnellGeometry{0, 6371.0, 1.0, 200.0, 400};
    if (geometry == 0) return PRHF_OK;
    if (!(earth_radius_km > 0.0) || !(earth_radius_km < 1e300) || !(dz_target_km > 0.0) || !(apex_boost >= 0.0) || max_substeps < 1)
        return fail(PRHF_EINVAL, "bad spherical tracer controls");
    *geo = SnellGeometry{1, earth_radius_km, dz_target_km, apex_boost, max_substeps};
    return PRHF_OK;
}

// The profile columns a Snell call is made on, and the path arrays a tracer call may ask for
struct SnellColumns {
    const double *den, *bmag, *bpsi, *alt;
    int64_t n_prof, n_alt, alt_stride;
    int32_t mode;
};
struct SnellPaths {
    double *x, *z;
    int64_t stride;
};

// What the three drivers put into SnellArgs alike: the columns' shape, mode, geometry, status words
void snell_args(prhf_ctx* c, prhf::SnellArgs& a, const SnellGeometry& geo, int64_t n_rays, const SnellColumns& p) {
    a.n_rays = n_rays; a.n_prof = p.n_prof; a.n_alt = p.n_alt; a.prof_stride = p.n_alt; a.alt_stride = p.alt_stride;
    a.mode = p.mode == PRHF_MODE_O ? PRHF_KMODE_O : PRHF_KMODE_X;
    a.geometry = geo.geometry;
    a.earth_radius_km = geo.earth_radius_km;
    a.dz_target_km = geo.dz_target_km;
    a.apex_boost = geo.apex_boost;
    a.max_substeps = geo.max_substeps;
    a.status = c->h_status_dev;
    a.resident_cus = c->cu_count;
}

// The level tables of a grouped launch, c->levels.  Per group and level: mu' (8 B), the compacted entry (32 B), its grid
// level (4 B); per group: four scalars.
struct LevelTables {
    double *levels, *entries;
    int *info, *kidx;
};
LevelTables carve_level_tables(Carver& k, int64_t n_groups, int64_t n_alt) {
    const size_t cells = (size_t)n_groups * (size_t)(n_alt + 1);
    LevelTables t;
    t.levels = k.take<double>((cells + 1) & ~(size_t)1);          // (the entries behind them are read 16 bytes at a time)
    t.entries = k.take<double>(4 * cells);
    t.info = k.take<int>(4 * (size_t)n_groups);
    t.kidx = k.take<int>(cells);
    return t;
}
// limits: what the message names as counted in 32 bits ("groups", or "groups / rays" where the launch has rays of its
// own: n_rays, else 0); verb: what to do in batches
int check_level_tables(int64_t n_groups, int64_t n_alt, int64_t n_rays, const char* limits, const char* verb) {
    Carver sizing(nullptr);
    carve_level_tables(sizing, n_groups, n_alt);
    if (sizing.used() > ((size_t)64 << 30) || n_groups > 0x7fffffffLL || n_rays > 0x7fffffffLL)
        return fail(PRHF_EINVAL, "level tables of %lld groups exceed 64 GiB (or 2^31 - 1 %s): %s in batches",
                    (long long)n_groups, limits, verb);
    return PRHF_OK;
}
int level_tables(prhf_ctx* c, prhf::SnellArgs& a, int64_t n_groups, int64_t n_alt) {
    return carve(c, c->levels, [&](Stager& k) {
        const LevelTables t = carve_level_tables(k, n_groups, n_alt);
        a.levels = t.levels; a.group_entries = t.entries; a.group_info = t.info; a.group_kidx = t.kidx;
    });
}

// The per-profile scalars at the head of c->partial (the operator's chunk scratch is free here), 128-byte rounded
void carve_prof_info(Carver& k, prhf::SnellArgs& a, int64_t n_prof) {
    a.prof_info = k.take<double>(4 * (size_t)n_prof);
    k.align(128);
}
// The per-profile table of a launch with n_keys (profile, frequency) keys: option "snell_table", at most 1 GiB
int profile_table(prhf_ctx* c, prhf::SnellArgs& a, int64_t n_keys, int64_t n_prof, int64_t n_alt) {
    const size_t prof_elems = (size_t)n_prof * (size_t)n_alt;
    a.ptab = nullptr;
    if (c->knobs.snell_table > 0 && (double)n_keys >= c->knobs.snell_table * (double)n_prof && prof_elems * 32 <= ((size_t)1 << 30)) {
        PRHF_TRY(ensure(c, c->ptab, prof_elems * 32));
        a.ptab = static_cast<double*>(c->ptab.p);
    }
    return PRHF_OK;
}

// The four columns of a host-buffer call at the head of the arena: den, bmag, bpsi (n_prof, n_alt) and alt
void put_columns(Stager& k, prhf::SnellArgs& a, const SnellColumns& p) {
    const size_t prof_elems = (size_t)p.n_prof * (size_t)p.n_alt;
    a.den = k.put<double>(p.den, prof_elems);
    a.bmag = k.put<double>(p.bmag, prof_elems);
    a.bpsi = k.put<double>(p.bpsi, prof_elems);
    a.alt = k.put<double>(p.alt, p.alt_stride ? prof_elems : (size_t)p.n_alt);
}

// Grouped launch: freq_hz / profile_index describe n_groups (profile, frequency) groups and ray_group[r] names the
// group of ray r; ungrouped: ray_group == nullptr, n_groups == 0 and freq_hz / profile_index are per ray.
int snell_run(prhf_ctx* c, const SnellGeometry& geo, const SnellColumns& p, const double* freq_hz, const double* elevation_deg,
              const int64_t* profile_index, int64_t n_rays, double* out, const SnellPaths& paths, uint32_t flags,
              const int64_t* ray_group = nullptr, int64_t n_groups = 0) {
    const double *den = p.den, *bmag = p.bmag, *bpsi = p.bpsi, *alt = p.alt;
    const int64_t n_prof = p.n_prof, n_alt = p.n_alt, alt_stride_elems = p.alt_stride, path_stride = paths.stride;
    const int32_t mode = p.mode;
    double *const path_x = paths.x, *const path_z = paths.z;
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (!freq_hz || !elevation_deg || !den || !bmag || !bpsi || !alt || !out)
        return fail(PRHF_EINVAL, "null array pointer");
    const bool grouped = ray_group != nullptr;
    if (grouped && n_groups < 1) return fail(PRHF_EINVAL, "a grouped launch needs at least one group");
    const int64_t n_keys = grouped ? n_groups : n_rays;          // entries of freq_hz / profile_index
    if (grouped) PRHF_TRY(check_level_tables(n_groups, n_alt, n_rays, "groups / rays", "trace"));
    if (n_rays < 0 || n_prof < 1 || n_alt < 2 || n_alt > 3000) return fail(PRHF_EINVAL, "bad shape");
    if (grouped && n_prof > 0x7fffffffLL) return fail(PRHF_EINVAL, "a grouped launch takes at most 2^31 - 1 profiles");
    if ((path_x == nullptr) != (path_z == nullptr)) return fail(PRHF_EINVAL, "path_x and path_z go together");
    if (path_x && path_stride < 2 * (n_alt + 1) - 1)
        return fail(PRHF_EINVAL, "path_stride must hold 2 (n_alt + 1) - 1 nodes");
    if (mode != PRHF_MODE_O && mode != PRHF_MODE_X) return fail(PRHF_EINVAL, "Mode must be O or X");
    if (alt_stride_elems != 0 && alt_stride_elems != n_alt) return fail(PRHF_EINVAL, "alt stride is 0 or n_alt");
    if (flags & ~PRHF_FLAG_DEVICE_PTRS) return fail(PRHF_EINVAL, "unknown flag bits");
    if (n_rays == 0) return PRHF_OK;
    const bool dev = (flags & PRHF_FLAG_DEVICE_PTRS) != 0;
    if (!dev && profile_index) PRHF_TRY(check_index("profile_index", profile_index, n_keys, "n_prof", n_prof));
    if (!dev && grouped) PRHF_TRY(check_index("ray_group", ray_group, n_rays, "n_groups", n_groups));
    ENTER_DEVICE(c->device);
    prhf::SnellArgs a;
    std::memset(&a, 0, sizeof a);
    snell_args(c, a, geo, n_rays, p);
    a.path_stride = path_x ? path_stride : 0;
    a.reduced = (c->math == PRHF_MATH_FAITHFUL) ? 0 : 1;        // (grouped launches read faithful level tables either way)
    const size_t R = (size_t)n_rays, path_elems = path_x ? R * (size_t)path_stride : 0;
    const double* d_keyf = freq_hz;
    const long long* d_keyp = reinterpret_cast<const long long*>(profile_index);
    const long long* d_group = reinterpret_cast<const long long*>(ray_group);
    bool small_out = false;                    // a small host-buffer call: the kernel writes its results into pinned host memory
    if (dev) {
        a.den = den; a.bmag = bmag; a.bpsi = bpsi; a.alt = alt; a.elev_deg = elevation_deg;
        a.out = out; a.path_x = path_x; a.path_z = path_z;
    } else {
        auto inputs = [&](Stager& k) {
            put_columns(k, a, p);
            d_keyf = k.put<double>(freq_hz, (size_t)n_keys);
            d_keyp = k.put<long long>(profile_index, (size_t)n_keys);
            a.elev_deg = k.put<double>(elevation_deg, R);
            d_group = k.put<long long>(ray_group, R);
        };
        auto outputs = [&](Stager& k) {
            a.out = k.take<double>(PRHF_SNELL_OUTPUTS * R);
            a.path_x = k.take<double>(path_elems);
            a.path_z = k.take<double>(path_elems);
        };
        Stager sizing(c, nullptr);
        inputs(sizing);
        const size_t in_bytes = sizing.used();
        outputs(sizing);
        PRHF_TRY(ensure(c, c->arena, sizing.used()));
        // A small call (the reference's own: ONE ray, its path arrays back): six to eight uploads from pageable memory
        // and three copies back cost several times the kernels.  As in run(): the inputs are packed in the arena's own
        // order and sent in one piece - or, on a large-BAR device with the arena idle, written straight into it by the
        // CPU - and the kernel writes the results into pinned host memory that the device sees (the upper half of the
        // pack buffer).
        const size_t out_elems = PRHF_SNELL_OUTPUTS * R + 2 * path_elems;
        small_out = c->h_pack && in_bytes <= kPackBytes / 2 && out_elems * 8 <= kPackBytes / 4;
        const bool direct = small_out && c->large_bar && c->knobs.direct_upload != 0 && in_bytes <= kDirectBytes &&
                            hipStreamQuery(c->stream) == hipSuccess && (!c->timed || hipEventQuery(c->end_ev()) == hipSuccess);
        if (small_out) (void)hipGetLastError();        // (hipErrorNotReady from the two queries is not an error)
        void* const pack = !small_out ? nullptr : direct ? c->arena.p : c->h_pack;
        Stager k(c, c->arena.p, pack);
        inputs(k);
        HIP_TRY(k.error());
        if (direct) _mm_sfence();
        else if (small_out) HIP_TRY(upload(c, c->arena.p, pack, in_bytes));
        outputs(k);
        if (small_out) {
            a.out = c->h_pack_dev + kPackBytes / 16;               // doubles: byte offset kPackBytes / 2
            a.path_x = a.out + PRHF_SNELL_OUTPUTS * R;
            a.path_z = a.path_x + path_elems;
        }
        if (!path_x) a.path_x = a.path_z = nullptr;
    }
    if (grouped) {
        a.ray_group = d_group; a.group_freq = d_keyf; a.group_prof = d_keyp; a.n_groups = n_groups;
        PRHF_TRY(level_tables(c, a, n_groups, n_alt));
    } else {
        a.freq_hz = d_keyf; a.prof_idx = d_keyp;
    }
    // per-profile scalars; behind them the queue counters of the per-ray launch (persistent wavefronts drawing rays from a queue)
    PRHF_TRY(carve(c, c->partial, [&](Stager& k) {
        carve_prof_info(k, a, n_prof);
        unsigned* queue = k.take<unsigned>(prhf::snell_queue_bytes() / sizeof(unsigned));
        a.ray_queue = grouped ? nullptr : queue;
    }));
    PRHF_TRY(profile_table(c, a, n_keys, n_prof, n_alt));
    PRHF_TRY(timed_launch(c, true, [&] { return prhf::launch_snell(a, c->stream); }));
    if (small_out) {                                               // (written by the kernel itself into pinned memory)
        const int rc = prhf_sync(c);
        const double* h_out = c->h_pack + kPackBytes / 16;
        std::memcpy(out, h_out, PRHF_SNELL_OUTPUTS * R * 8);
        if (path_x) {
            std::memcpy(path_x, h_out + PRHF_SNELL_OUTPUTS * R, path_elems * 8);
            std::memcpy(path_z, h_out + PRHF_SNELL_OUTPUTS * R + path_elems, path_elems * 8);
        }
        return rc;
    }
    if (!dev) {
        HIP_TRY(download(c, out, a.out, PRHF_SNELL_OUTPUTS * R * 8));
        if (path_x) {
            HIP_TRY(download(c, path_x, a.path_x, path_elems * 8));
            HIP_TRY(download(c, path_z, a.path_z, path_elems * 8));
        }
    }
    return prhf_sync(c);
}
}  // namespace

int prhf_snell_cartesian_f64(prhf_ctx* c, const double* freq_hz, const double* elevation_deg,
                             const int64_t* profile_index, int64_t n_rays, const double* den, const double* bmag,
                             const double* bpsi, const double* alt, int64_t n_prof, int64_t n_alt,
                             int64_t alt_stride_elems, int32_t mode, double* out, double* path_x, double* path_z,
                             int64_t path_stride, uint32_t flags) {
    SnellGeometry geo;
    PRHF_TRY(snell_controls(0, 0.0, 0.0, 0.0, 0, &geo));
    return snell_run(c, geo, SnellColumns{den, bmag, bpsi, alt, n_prof, n_alt, alt_stride_elems, mode}, freq_hz, elevation_deg,
                     profile_index, n_rays, out, SnellPaths{path_x, path_z, path_stride}, flags);
}

int prhf_snell_spherical_f64(prhf_ctx* c, const double* freq_hz, const double* elevation_deg,
                             const int64_t* profile_index, int64_t n_rays, const double* den, const double* bmag,
                             const double* bpsi, const double* alt, int64_t n_prof, int64_t n_alt,
                             int64_t alt_stride_elems, int32_t mode, double earth_radius_km, double dz_target_km,
                             double apex_boost, int32_t max_substeps, double* out, double* path_x, double* path_z,
                             int64_t path_stride, uint32_t flags) {
    SnellGeometry geo;
    PRHF_TRY(snell_controls(1, earth_radius_km, dz_target_km, apex_boost, max_substeps, &geo));
    return snell_run(c, geo, SnellColumns{den, bmag, bpsi, alt, n_prof, n_alt, alt_stride_elems, mode}, freq_hz, elevation_deg,
                     profile_index, n_rays, out, SnellPaths{path_x, path_z, path_stride}, flags);
}

int prhf_snell_fan_f64(prhf_ctx* c, int32_t geometry, const double* group_freq_hz, const int64_t* group_profile_index,
                       int64_t n_groups, const int64_t* ray_group, const double* elevation_deg, int64_t n_rays,
                       const double* den, const double* bmag, const double* bpsi, const double* alt, int64_t n_prof,
                       int64_t n_alt, int64_t alt_stride_elems, int32_t mode, double earth_radius_km,
                       double dz_target_km, double apex_boost, int32_t max_substeps, double* out, double* path_x,
                       double* path_z, int64_t path_stride, uint32_t flags) {
    PRHF_TRY(check_snell_geometry(geometry));
    if (!ray_group) return fail(PRHF_EINVAL, "null array pointer");
    SnellGeometry geo;
    PRHF_TRY(snell_controls(geometry, earth_radius_km, dz_target_km, apex_boost, max_substeps, &geo));
    return snell_run(c, geo, SnellColumns{den, bmag, bpsi, alt, n_prof, n_alt, alt_stride_elems, mode}, group_freq_hz,
                     elevation_deg, group_profile_index, n_rays, out, SnellPaths{path_x, path_z, path_stride}, flags, ray_group,
                     n_groups);
}

int prhf_snell_home_f64(prhf_ctx* c, int32_t geometry, const double* group_freq_hz, const int64_t* group_profile_index,
                        int64_t n_groups, const int64_t* link_group, const double* link_range_km, int64_t n_links,
                        const double* scan_elevation_deg, int64_t n_scan, const double* den, const double* bmag,
                        const double* bpsi, const double* alt, int64_t n_prof, int64_t n_alt, int64_t alt_stride_elems,
                        int32_t mode, double earth_radius_km, double dz_target_km, double apex_boost, int32_t max_substeps,
                        double range_tol_km, int32_t max_iter, int32_t max_roots, double* out, int64_t* n_brackets,
                        uint32_t flags) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (!group_freq_hz || !link_group || !link_range_km || !scan_elevation_deg || !den || !bmag || !bpsi || !alt || !out ||
        !n_brackets)
        return fail(PRHF_EINVAL, "null array pointer");
    SnellGeometry geo;
    PRHF_TRY(check_snell_geometry(geometry));
    PRHF_TRY(snell_controls(geometry, earth_radius_km, dz_target_km, apex_boost, max_substeps, &geo));
    if (n_scan < 2) return fail(PRHF_EINVAL, "the scan grid needs at least 2 elevations");
    if (max_iter < 1 || max_iter > 128) return fail(PRHF_EINVAL, "max_iter is 1 .. 128");
    if (max_roots < 1 || max_roots > 64) return fail(PRHF_EINVAL, "max_roots is 1 .. 64");
    if (!(range_tol_km >= 0.0) || !std::isfinite(range_tol_km))
        return fail(PRHF_EINVAL, "range_tol_km must be finite and not negative");
    if (n_groups < 1) return fail(PRHF_EINVAL, "homing needs at least one group");
    PRHF_TRY(check_level_tables(n_groups, n_alt, 0, "groups", "home"));
    if (n_links < 0 || n_prof < 1 || n_prof > 0x7fffffffLL || n_alt < 2 || n_alt > 3000) return fail(PRHF_EINVAL, "bad shape");
    if (n_groups * n_scan > 0x7fffffffLL || n_links * (int64_t)max_roots > 0x7fffffffLL)
        return fail(PRHF_EINVAL, "more than 2^31 - 1 scan rays or result rows: home in batches");
    if (mode != PRHF_MODE_O && mode != PRHF_MODE_X) return fail(PRHF_EINVAL, "Mode must be O or X");
    if (alt_stride_elems != 0 && alt_stride_elems != n_alt) return fail(PRHF_EINVAL, "alt stride is 0 or n_alt");
    if (flags & ~PRHF_FLAG_DEVICE_PTRS) return fail(PRHF_EINVAL, "unknown flag bits");
    const bool dev = (flags & PRHF_FLAG_DEVICE_PTRS) != 0;
    if (!dev) {
        PRHF_TRY(check_scan_grid(scan_elevation_deg, n_scan, false));
        if (group_profile_index) PRHF_TRY(check_index("profile_index", group_profile_index, n_groups, "n_prof", n_prof));
        PRHF_TRY(check_index("link_group", link_group, n_links, "n_groups", n_groups));
    }
    if (n_links == 0) return PRHF_OK;
    ENTER_DEVICE(c->device);
    const SnellColumns p{den, bmag, bpsi, alt, n_prof, n_alt, alt_stride_elems, mode};
    prhf::HomeArgs h;
    std::memset(&h, 0, sizeof h);
    prhf::SnellArgs& a = h.s;
    snell_args(c, a, geo, 1, p);
    a.n_groups = n_groups;
    h.n_links = n_links; h.n_scan = (int)n_scan; h.range_tol = range_tol_km; h.max_iter = max_iter; h.max_roots = max_roots;
    const size_t G = (size_t)n_groups, L = (size_t)n_links, E = (size_t)n_scan;
    const size_t out_elems = L * (size_t)max_roots * PRHF_HOME_OUTPUTS;
    if (dev) {
        a.den = den; a.bmag = bmag; a.bpsi = bpsi; a.alt = alt;
        a.group_freq = group_freq_hz;
        a.group_prof = reinterpret_cast<const long long*>(group_profile_index);
        h.link_group = reinterpret_cast<const long long*>(link_group);
        h.link_range = link_range_km; h.scan_elev = scan_elevation_deg;
        h.out = out; h.n_brackets = reinterpret_cast<long long*>(n_brackets);
    } else {
        PRHF_TRY(carve(c, c->arena, [&](Stager& k) {
            put_columns(k, a, p);
            a.group_freq = k.put<double>(group_freq_hz, G);
            a.group_prof = k.put<long long>(group_profile_index, G);
            h.link_group = k.put<long long>(link_group, L);
            h.link_range = k.put<double>(link_range_km, L);
            h.scan_elev = k.put<double>(scan_elevation_deg, E);
            h.n_brackets = k.take<long long>(L);
            h.out = k.take<double>(out_elems);
        }));
    }
    PRHF_TRY(level_tables(c, a, n_groups, n_alt));
    // per-profile scalars; behind them the refine launch's counters, the work list and the scan's ground ranges
    PRHF_TRY(carve(c, c->partial, [&](Stager& k) {
        carve_prof_info(k, a, n_prof);
        h.queue = k.take<unsigned>(prhf::home_queue_bytes() / sizeof(unsigned));
        k.align(128);
        h.work = k.take<int>(L * (size_t)max_roots * 4);
        h.scan_d = k.take<double>(G * E);
    }));
    PRHF_TRY(profile_table(c, a, n_groups, n_prof, n_alt));
    PRHF_TRY(timed_launch(c, true, [&] { return prhf::launch_snell_home(h, c->stream); }));
    if (!dev) {
        HIP_TRY(download(c, out, h.out, out_elems * 8));
        HIP_TRY(download(c, n_brackets, h.n_brackets, L * 8));
    }
    return prhf_sync(c);
}

namespace {
// prhf_snell_skip_f64 (link_range_km null: group_freq_hz and group_profile_index describe n_groups groups) and
// prhf_snell_muf_f64 (a link is a group: group_profile_index is the links' profile index, n_groups their number, and the
// group frequencies are the device's own).
struct SkipControls {
    int32_t geometry;
    double earth_radius_km, dz_target_km, apex_boost;
    int32_t max_substeps;
    double elev_tol_deg;
    int32_t max_iter;
    double f_lo_hz, f_hi_hz;     // MUF only
    int32_t n_bisect;
};
int skip_run(prhf_ctx* c, const SkipControls& s, const SnellColumns& p, const double* group_freq_hz,
             const int64_t* group_profile_index, int64_t n_groups, const double* link_range_km, const double* scan_elevation_deg,
             int64_t n_scan, double* out, uint32_t flags) {
    const double *den = p.den, *bmag = p.bmag, *bpsi = p.bpsi, *alt = p.alt;
    const int64_t n_prof = p.n_prof, n_alt = p.n_alt, alt_stride_elems = p.alt_stride;
    const int32_t mode = p.mode;
    const bool muf = link_range_km != nullptr;
    if (!c) return fail(PRHF_EINVAL, "null context");
    if ((!muf && !group_freq_hz) || !scan_elevation_deg || !den || !bmag || !bpsi || !alt || !out)
        return fail(PRHF_EINVAL, "null array pointer");
    SnellGeometry geo;
    PRHF_TRY(check_snell_geometry(s.geometry));
    PRHF_TRY(snell_controls(s.geometry, s.earth_radius_km, s.dz_target_km, s.apex_boost, s.max_substeps, &geo));
    if (n_scan < 1) return fail(PRHF_EINVAL, "the scan grid needs at least 1 elevation");
    if (s.max_iter < 1 || s.max_iter > 128) return fail(PRHF_EINVAL, "max_iter is 1 .. 128");
    if (!(s.elev_tol_deg >= 0.0) || !std::isfinite(s.elev_tol_deg))
        return fail(PRHF_EINVAL, "elev_tol_deg must be finite and not negative");
    if (muf) {
        if (s.n_bisect < 1 || s.n_bisect > 64) return fail(PRHF_EINVAL, "n_bisect is 1 .. 64");
        if (!(s.f_lo_hz > 0.0) || !(s.f_hi_hz > s.f_lo_hz) || !std::isfinite(s.f_hi_hz))
            return fail(PRHF_EINVAL, "the frequency bracket needs 0 < f_lo_hz < f_hi_hz, both finite");
    }
    if (n_groups < 0 || n_prof < 1 || n_prof > 0x7fffffffLL || n_alt < 2 || n_alt > 3000) return fail(PRHF_EINVAL, "bad shape");
    PRHF_TRY(check_level_tables(n_groups, n_alt, 0, "groups", "search"));
    if (n_groups * n_scan > 0x7fffffffLL) return fail(PRHF_EINVAL, "more than 2^31 - 1 scan rays: search in batches");
    if (mode != PRHF_MODE_O && mode != PRHF_MODE_X) return fail(PRHF_EINVAL, "Mode must be O or X");
    if (alt_stride_elems != 0 && alt_stride_elems != n_alt) return fail(PRHF_EINVAL, "alt stride is 0 or n_alt");
    if (flags & ~PRHF_FLAG_DEVICE_PTRS) return fail(PRHF_EINVAL, "unknown flag bits");
    const bool dev = (flags & PRHF_FLAG_DEVICE_PTRS) != 0;
    if (!dev) {
        PRHF_TRY(check_scan_grid(scan_elevation_deg, n_scan, true));
        if (group_profile_index) PRHF_TRY(check_index("profile_index", group_profile_index, n_groups, "n_prof", n_prof));
    }
    if (n_groups == 0) return PRHF_OK;
    ENTER_DEVICE(c->device);
    prhf::MufArgs m;
    std::memset(&m, 0, sizeof m);
    prhf::SkipArgs& h = m.k;
    prhf::SnellArgs& a = h.s;
    snell_args(c, a, geo, 1, p);
    a.n_groups = n_groups;
    h.n_scan = (int)n_scan; h.elev_tol = s.elev_tol_deg; h.max_iter = s.max_iter;
    m.n_links = n_groups; m.f_lo = s.f_lo_hz; m.f_hi = s.f_hi_hz; m.n_bisect = s.n_bisect;
    const size_t G = (size_t)n_groups, E = (size_t)n_scan;
    const size_t out_elems = G * (muf ? PRHF_MUF_OUTPUTS : PRHF_SKIP_OUTPUTS);
    double* d_result = out;
    if (dev) {
        a.den = den; a.bmag = bmag; a.bpsi = bpsi; a.alt = alt;
        a.group_freq = group_freq_hz;
        a.group_prof = reinterpret_cast<const long long*>(group_profile_index);
        m.link_range = link_range_km; h.scan_elev = scan_elevation_deg;
    } else {
        PRHF_TRY(carve(c, c->arena, [&](Stager& k) {
            put_columns(k, a, p);
            a.group_freq = k.put<double>(group_freq_hz, G);              // (null for the MUF: the device's own, below)
            a.group_prof = k.put<long long>(group_profile_index, G);
            m.link_range = k.put<double>(link_range_km, G);
            h.scan_elev = k.put<double>(scan_elevation_deg, E);
            d_result = k.take<double>(out_elems);
        }));
    }
    PRHF_TRY(level_tables(c, a, n_groups, n_alt));
    // per-profile scalars; behind them the scan's ground ranges and - MUF - the links' frequencies, brackets, skip rows
    // of the trip and of the bracket's lower end, and "still searching" words
    PRHF_TRY(carve(c, c->partial, [&](Stager& k) {
        carve_prof_info(k, a, n_prof);
        h.scan_d = k.take<double>(G * E);
        h.out = d_result;
        if (!muf) return;
        m.group_freq = k.take<double>(G);
        m.state = k.take<double>(4 * G);
        m.best = k.take<double>(G * PRHF_SKIP_OUTPUTS);
        h.out = k.take<double>(G * PRHF_SKIP_OUTPUTS);
        m.active = k.take<int>(G);
        a.group_freq = m.group_freq;
        h.active = m.active;
        m.out = d_result;
    }));
    PRHF_TRY(profile_table(c, a, n_groups, n_prof, n_alt));
    PRHF_TRY(timed_launch(c, true, [&] {
        return muf ? prhf::launch_snell_muf(m, c->stream) : prhf::launch_snell_skip(h, c->stream);
    }));
    if (!dev) HIP_TRY(download(c, out, d_result, out_elems * 8));
    return prhf_sync(c);
}
}  // namespace

int prhf_snell_skip_f64(prhf_ctx* c, int32_t geometry, const double* group_freq_hz, const int64_t* group_profile_index,
                        int64_t n_groups, const double* scan_elevation_deg, int64_t n_scan, const double* den,
                        const double* bmag, const double* bpsi, const double* alt, int64_t n_prof, int64_t n_alt,
                        int64_t alt_stride_elems, int32_t mode, double earth_radius_km, double dz_target_km,
                        double apex_boost, int32_t max_substeps, double elev_tol_deg, int32_t max_iter, double* out,
                        uint32_t flags) {
    if (c && n_groups < 1) return fail(PRHF_EINVAL, "the search needs at least one group");
    const SkipControls s{geometry, earth_radius_km, dz_target_km, apex_boost, max_substeps, elev_tol_deg, max_iter, 0.0, 0.0, 0};
    return skip_run(c, s, SnellColumns{den, bmag, bpsi, alt, n_prof, n_alt, alt_stride_elems, mode}, group_freq_hz,
                    group_profile_index, n_groups, nullptr, scan_elevation_deg, n_scan, out, flags);
}

int prhf_snell_muf_f64(prhf_ctx* c, int32_t geometry, const int64_t* link_profile_index, const double* link_range_km,
                       int64_t n_links, double f_lo_hz, double f_hi_hz, int32_t n_bisect, const double* scan_elevation_deg,
                       int64_t n_scan, const double* den, const double* bmag, const double* bpsi, const double* alt,
                       int64_t n_prof, int64_t n_alt, int64_t alt_stride_elems, int32_t mode, double earth_radius_km,
                       double dz_target_km, double apex_boost, int32_t max_substeps, double elev_tol_deg, int32_t max_iter,
                       double* out, uint32_t flags) {
    if (c && !link_range_km) return fail(PRHF_EINVAL, "null array pointer");
    if (c && n_links < 1) return fail(PRHF_EINVAL, "the search needs at least one link");
    const SkipControls s{geometry, earth_radius_km, dz_target_km, apex_boost, max_substeps, elev_tol_deg, max_iter, f_lo_hz, f_hi_hz,
                         n_bisect};
    return skip_run(c, s, SnellColumns{den, bmag, bpsi, alt, n_prof, n_alt, alt_stride_elems, mode}, nullptr, link_profile_index,
                    n_links, link_range_km, scan_elevation_deg, n_scan, out, flags);
}

namespace {
// The two axes of a field: host memory, strictly increasing (a NaN fails the test), at least `least` values each and
// together no more than the kernels stage in LDS.  *uniform: all np.diff(axis) are equal (np.gradient's scalar branch).
int check_axis(const char* name, const double* g, int64_t n, int64_t least, int* uniform) {
    if (n < least) return fail(PRHF_EINVAL, "%s needs at least %lld values", name, (long long)least);
    *uniform = 1;
    const double d0 = g[1] - g[0];
    for (int64_t i = 0; i + 1 < n; ++i) {
        const double d = g[i + 1] - g[i];
        if (!(d > 0)) return fail(PRHF_EINVAL, "%s must be strictly increasing", name);
        if (!(d == d0)) *uniform = 0;
    }
    return PRHF_OK;
}
int check_field_shape(const double* axis0, const double* axis1, int64_t n_fields, int64_t n0, int64_t n1, int64_t least,
                      int* u0, int* u1) {
    if (!axis0 || !axis1) return fail(PRHF_EINVAL, "null array pointer");
    if (n_fields < 1 || n0 < 1 || n1 < 1 || n0 + n1 > PRHF_FIELD_MAX_AXES || n_fields > (int64_t)1 << 24)
        return fail(PRHF_EINVAL, "bad shape (the two axes hold at most %d values together)", PRHF_FIELD_MAX_AXES);
    int rc = check_axis("axis 0", axis0, n0, least, u0);
    if (rc != PRHF_OK) return rc;
    return check_axis("axis 1", axis1, n1, least, u1);
}
}  // namespace

int prhf_field_pack_f64(prhf_ctx* c, const double* mu, const double* mup, int64_t n_fields, int64_t n0, int64_t n1,
                        const double* axis0, const double* axis1, int32_t edge_order, double* records, uint32_t flags) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (!mu || !mup || !records) return fail(PRHF_EINVAL, "null array pointer");
    if (edge_order != 1 && edge_order != 2) return fail(PRHF_EINVAL, "edge_order is 1 or 2");
    if (flags & ~PRHF_FLAG_DEVICE_PTRS) return fail(PRHF_EINVAL, "unknown flag bits");
    int u0 = 0, u1 = 0;
    int rc = check_field_shape(axis0, axis1, n_fields, n0, n1, edge_order + 1, &u0, &u1);
    if (rc != PRHF_OK) return rc;
    ENTER_DEVICE(c->device);
    const bool dev = (flags & PRHF_FLAG_DEVICE_PTRS) != 0;
    const size_t cells = (size_t)n_fields * (size_t)n0 * (size_t)n1;
    FieldPackBlock b;
    PRHF_TRY(carve(c, c->arena, [&](Stager& k) {
        b = field_pack_block(k, (size_t)n0, (size_t)n1, dev ? 0 : cells);
        k.put(b.a0, axis0, (size_t)n0);
        k.put(b.a1, axis1, (size_t)n1);
        if (dev) return;
        k.put(b.mu, mu, cells);
        k.put(b.mup, mup, cells);
    }));
    prhf::FieldPackArgs a;
    std::memset(&a, 0, sizeof a);
    a.a0 = b.a0; a.a1 = b.a1; a.mu = dev ? mu : b.mu; a.mup = dev ? mup : b.mup;
    a.rec = records; a.n_fields = n_fields; a.n0 = (int)n0; a.n1 = (int)n1; a.uniform0 = u0; a.uniform1 = u1;
    a.edge_order = edge_order;
    PRHF_TRY(timed_launch(c, false, [&] { return prhf::launch_field_pack(a, c->stream); }));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PRHF_OK;
}

int prhf_field_sample_f64(prhf_ctx* c, const double* records, int64_t n_fields, int64_t n0, int64_t n1,
                          const double* axis0, const double* axis1, const double* p0, const double* p1,
                          const int64_t* field_index, int64_t n, double fill_n, double fill_grad, double fill_mup,
                          double* out_n, double* out_d1, double* out_d0, double* out_mup, uint32_t flags) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (!records || !p0 || !p1) return fail(PRHF_EINVAL, "null array pointer");
    if (!out_n && !out_d1 && !out_d0 && !out_mup) return fail(PRHF_EINVAL, "no output asked for");
    if (n < 0) return fail(PRHF_EINVAL, "bad shape");
    if (flags & ~PRHF_FLAG_DEVICE_PTRS) return fail(PRHF_EINVAL, "unknown flag bits");
    int u0 = 0, u1 = 0;
    int rc = check_field_shape(axis0, axis1, n_fields, n0, n1, 2, &u0, &u1);
    if (rc != PRHF_OK) return rc;
    const bool dev = (flags & PRHF_FLAG_DEVICE_PTRS) != 0;
    if (!dev && field_index)
        for (int64_t i = 0; i < n; ++i)
            if (field_index[i] < 0 || field_index[i] >= n_fields)
                return fail(PRHF_EINVAL, "field_index[%lld] outside [0, n_fields)", (long long)i);
    if (n == 0) return PRHF_OK;
    ENTER_DEVICE(c->device);
    double* const outs[4] = {out_n, out_d1, out_d0, out_mup};
    FieldSampleBlock b;
    PRHF_TRY(carve(c, c->arena, [&](Stager& k) {
        b = field_sample_block(k, (size_t)n0, (size_t)n1, dev ? 0 : (size_t)n);
        k.put(b.a0, axis0, (size_t)n0);
        k.put(b.a1, axis1, (size_t)n1);
        if (dev) return;
        k.put(b.p0, p0, (size_t)n);
        k.put(b.p1, p1, (size_t)n);
        k.put(b.field, field_index, (size_t)n);
    }));
    for (int i = 0; i < 4; ++i)
        if (dev || !outs[i]) b.out[i] = outs[i];
    prhf::FieldSampleArgs a;
    std::memset(&a, 0, sizeof a);
    a.rec = records; a.a0 = b.a0; a.a1 = b.a1; a.n = n; a.n_fields = n_fields; a.n0 = (int)n0; a.n1 = (int)n1;
    a.fill_n = fill_n; a.fill_grad = fill_grad; a.fill_mup = fill_mup; a.status = c->h_status_dev;
    a.p0 = dev ? p0 : b.p0; a.p1 = dev ? p1 : b.p1;
    a.field = dev || !field_index ? reinterpret_cast<const long long*>(field_index) : b.field;
    a.out_n = b.out[0]; a.out_d1 = b.out[1]; a.out_d0 = b.out[2]; a.out_mup = b.out[3];
    PRHF_TRY(timed_launch(c, true, [&] { return prhf::launch_field_sample(a, c->stream); }));
    for (int i = 0; i < 4 && !dev; ++i)
        if (outs[i]) HIP_TRY(download(c, outs[i], b.out[i], (size_t)n * 8));
    return prhf_sync(c);
}

namespace {
// ---- The gradient family: prhf_trace_gradient_f64 .. prhf_gradient_hop_muf_f64, and prhf_field_build_f64 ----

// The field grid of a call: records (n_fields, n0, n1, 4) on the device, the axes in host memory
struct FieldGrid {
    const double* records;
    int64_t n_fields, n0, n1;
    const double *axis0, *axis1;
};
// The tracer's controls as the exported calls take them (z_ground_km above the ground in both geometries; top, left,
// right: z_max_km, x_min_km, x_max_km, or r_max_km, phi_min, phi_max)
struct GradControls {
    int32_t geometry;
    double earth_radius_km, s_max_km, rtol, atol, max_step_km, z_ground_km, top, left, right;
    int32_t renormalize_every;
    double fill_n, fill_grad, fill_mup;
    bool spherical() const { return geometry == PRHF_GEO_SPHERICAL; }
};

// The checks of the tracer's controls, in three parts: prhf_trace_gradient*_f64 make other checks between them
int check_grad_geometry(const GradControls& t) {
    if (t.geometry != PRHF_GEO_CARTESIAN && t.geometry != PRHF_GEO_SPHERICAL)
        return fail(PRHF_EINVAL, "geometry is 0 (Cartesian) or 1 (spherical)");
    if (t.spherical() && (!(t.earth_radius_km > 0) || !std::isfinite(t.earth_radius_km)))
        return fail(PRHF_EINVAL, "earth_radius_km must be positive and finite");
    return PRHF_OK;
}
int check_grad_flags(uint32_t flags) {
    if (flags & ~PRHF_FLAG_DEVICE_PTRS) return fail(PRHF_EINVAL, "unknown flag bits");
    return PRHF_OK;
}
int check_grad_steps(const GradControls& t) {
    if (!(t.s_max_km > 0) || !std::isfinite(t.s_max_km)) return fail(PRHF_EINVAL, "s_max_km must be positive and finite");
    if (!(t.max_step_km > 0)) return fail(PRHF_EINVAL, "`max_step` must be positive.");
    if (!(t.rtol >= 0) || !(t.atol >= 0)) return fail(PRHF_EINVAL, "`atol` must be positive.");
    if (t.renormalize_every < 0) return fail(PRHF_EINVAL, "renormalize_every must not be negative");
    return PRHF_OK;
}
int check_grad_controls(const GradControls& t, uint32_t flags) {
    PRHF_TRY(check_grad_geometry(t));
    PRHF_TRY(check_grad_flags(flags));
    return check_grad_steps(t);
}
// ... and of a skip or MUF search on top of them
int check_grad_search(int64_t n_scan, double elev_tol_deg, int32_t max_iter) {
    if (n_scan < 1 || n_scan > 0x7fffffffLL) return fail(PRHF_EINVAL, "the scan grid needs at least 1 elevation");
    if (max_iter < 1 || max_iter > 128) return fail(PRHF_EINVAL, "max_iter is 1 .. 128");
    if (!(elev_tol_deg >= 0.0) || !std::isfinite(elev_tol_deg))
        return fail(PRHF_EINVAL, "elev_tol_deg must be finite and not negative");
    return PRHF_OK;
}

// Both axes of a field (host memory in every flag combination) at the head of the arena
template <class Args>
void put_axes(Stager& k, Args& a, const double* axis0, const double* axis1, int64_t n0, int64_t n1) {
    a.a0 = k.put<double>(axis0, (size_t)n0);
    a.a1 = k.put<double>(axis1, (size_t)n1);
}

// The tracer's arguments from the call's grid and controls; the axes, n_hops, hop_z0 and the per-ray arrays are the caller's
void grad_trace_args(prhf_ctx* c, prhf::GradTraceArgs& a, const FieldGrid& f, const GradControls& t) {
    a.rec = f.records; a.n0 = (int)f.n0; a.n1 = (int)f.n1; a.n_fields = f.n_fields;
    a.s_max = t.s_max_km;
    a.rtol = t.rtol < 100 * 2.220446049250313e-16 ? 100 * 2.220446049250313e-16 : t.rtol;     // (solve_ivp raises a too small rtol so)
    a.atol = t.atol; a.max_step = t.max_step_km;
    // (the reference's spherical tracer binds R_E + z_ground_km to the ground event before it subtracts, :2240)
    a.z_ground = t.spherical() ? t.earth_radius_km + t.z_ground_km : t.z_ground_km;
    a.z_max = t.top; a.x_min = t.left; a.x_max = t.right; a.renormalize_every = t.renormalize_every;
    a.fill_n = t.fill_n; a.fill_grad = t.fill_grad; a.fill_mup = t.fill_mup; a.status = c->h_status_dev;
    a.geometry = t.geometry; a.earth_radius = t.spherical() ? t.earth_radius_km : 0.0;
}

// Both gradient tracers.  Spherical: the axes are r and phi, top .. right carry r_max_km, phi_min, phi_max and the paths
// are t, r, phi, v_r, v_phi.  n_hops > 0: the multi-hop call (prhf_trace_gradient_hops_f64) - out is (n_rays, n_hops, 15)
// and the paths hold n_rays n_hops rows.
int grad_trace_run(prhf_ctx* c, int n_hops, const GradControls& t, const FieldGrid& f, const double* x0_km, const double* z0_km,
                   const double* elevation_deg, const int64_t* ray_field, int64_t n_rays, double* out, double* const paths[5],
                   int64_t path_stride, uint32_t flags) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (!f.records || !x0_km || !z0_km || !elevation_deg || !out) return fail(PRHF_EINVAL, "null array pointer");
    if (n_rays < 0) return fail(PRHF_EINVAL, "bad shape");
    PRHF_TRY(check_grad_flags(flags));
    int n_paths = 0;
    for (int k = 0; k < 5; ++k) n_paths += paths[k] != nullptr;
    if (n_paths != 0 && n_paths != 5) return fail(PRHF_EINVAL, "the five path arrays go together");
    if (n_paths && path_stride < 1) return fail(PRHF_EINVAL, "path_stride must hold at least the launch point");
    PRHF_TRY(check_grad_steps(t));
    int u0 = 0, u1 = 0;
    PRHF_TRY(check_field_shape(f.axis0, f.axis1, f.n_fields, f.n0, f.n1, 2, &u0, &u1));
    const bool dev = (flags & PRHF_FLAG_DEVICE_PTRS) != 0;
    if (!dev && ray_field) PRHF_TRY(check_index("ray_field", ray_field, n_rays, "n_fields", f.n_fields));
    if (n_rays == 0) return PRHF_OK;
    ENTER_DEVICE(c->device);
    const size_t R = (size_t)n_rays, path_elems = n_paths ? R * (size_t)(n_hops ? n_hops : 1) * (size_t)path_stride : 0;
    const size_t out_elems = R * (n_hops ? (size_t)n_hops * PRHF_GRAD_HOP_OUTPUTS : (size_t)PRHF_GRAD_OUTPUTS);
    prhf::GradTraceArgs a;
    std::memset(&a, 0, sizeof a);
    grad_trace_args(c, a, f, t);
    a.n_rays = n_rays; a.path_stride = n_paths ? path_stride : 0;
    a.n_hops = n_hops; a.hop_z0 = n_hops ? t.z_ground_km : 0.0;
    a.x0 = x0_km; a.z0 = z0_km; a.elev = elevation_deg; a.ray_field = reinterpret_cast<const long long*>(ray_field);
    a.out = out;
    double* d_paths[5] = {paths[0], paths[1], paths[2], paths[3], paths[4]};
    PRHF_TRY(carve(c, c->arena, [&](Stager& k) {
        put_axes(k, a, f.axis0, f.axis1, f.n0, f.n1);
        if (dev) return;
        a.x0 = k.put<double>(x0_km, R);
        a.z0 = k.put<double>(z0_km, R);
        a.elev = k.put<double>(elevation_deg, R);
        a.ray_field = k.put<long long>(ray_field, R);
        a.out = k.take<double>(out_elems);
        for (int i = 0; i < 5; ++i) d_paths[i] = n_paths ? k.take<double>(path_elems) : nullptr;
    }));
    // nodes a ray does not reach stay NaN (all bits set)
    for (int i = 0; i < 5 && n_paths; ++i) HIP_TRY(hipMemsetAsync(d_paths[i], 0xff, path_elems * 8, c->stream));
    a.path_t = d_paths[0]; a.path_x = d_paths[1]; a.path_z = d_paths[2]; a.path_vx = d_paths[3]; a.path_vz = d_paths[4];
    PRHF_TRY(timed_launch(c, true, [&] {
        return n_hops ? prhf::launch_grad_hop_trace(a, c->stream) : prhf::launch_grad_trace(a, c->stream);
    }));
    if (!dev) {
        HIP_TRY(download(c, out, a.out, out_elems * 8));
        for (int i = 0; i < 5 && n_paths; ++i) HIP_TRY(download(c, paths[i], d_paths[i], path_elems * 8));
    }
    return prhf_sync(c);
}
}  // namespace

int prhf_trace_gradient_f64(prhf_ctx* c, const double* records, int64_t n_fields, int64_t nz, int64_t nx,
                            const double* z_axis, const double* x_axis, const double* x0_km, const double* z0_km,
                            const double* elevation_deg, const int64_t* ray_field, int64_t n_rays, double s_max_km,
                            double rtol, double atol, double max_step_km, double z_ground_km, double z_max_km,
                            double x_min_km, double x_max_km, int32_t renormalize_every, double fill_n, double fill_grad,
                            double fill_mup, double* out, double* path_t, double* path_x, double* path_z, double* path_vx,
                            double* path_vz, int64_t path_stride, uint32_t flags) {
    const GradControls t{PRHF_GEO_CARTESIAN, 0.0, s_max_km, rtol, atol, max_step_km, z_ground_km, z_max_km, x_min_km, x_max_km,
                         renormalize_every, fill_n, fill_grad, fill_mup};
    const FieldGrid f{records, n_fields, nz, nx, z_axis, x_axis};
    double* const paths[5] = {path_t, path_x, path_z, path_vx, path_vz};
    return grad_trace_run(c, 0, t, f, x0_km, z0_km, elevation_deg, ray_field, n_rays, out, paths, path_stride, flags);
}

int prhf_trace_gradient_spherical_f64(prhf_ctx* c, const double* records, int64_t n_fields, int64_t nr, int64_t nphi,
                                      const double* r_axis, const double* phi_axis, const double* x0_km,
                                      const double* z0_km, const double* elevation_deg, const int64_t* ray_field,
                                      int64_t n_rays, double earth_radius_km, double s_max_km, double rtol, double atol,
                                      double max_step_km, double z_ground_km, double r_max_km, double phi_min,
                                      double phi_max, int32_t renormalize_every, double fill_n, double fill_grad,
                                      double fill_mup, double* out, double* path_t, double* path_r, double* path_phi,
                                      double* path_v_r, double* path_v_phi, int64_t path_stride, uint32_t flags) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    const GradControls t{PRHF_GEO_SPHERICAL, earth_radius_km, s_max_km, rtol, atol, max_step_km, z_ground_km, r_max_km, phi_min,
                         phi_max, renormalize_every, fill_n, fill_grad, fill_mup};
    PRHF_TRY(check_grad_geometry(t));
    const FieldGrid f{records, n_fields, nr, nphi, r_axis, phi_axis};
    double* const paths[5] = {path_t, path_r, path_phi, path_v_r, path_v_phi};
    return grad_trace_run(c, 0, t, f, x0_km, z0_km, elevation_deg, ray_field, n_rays, out, paths, path_stride, flags);
}

int prhf_trace_gradient_hops_f64(prhf_ctx* c, int32_t geometry, const double* records, int64_t n_fields, int64_t n0,
                                 int64_t n1, const double* axis0, const double* axis1, const double* x0_km,
                                 const double* z0_km, const double* elevation_deg, const int64_t* ray_field, int64_t n_rays,
                                 double earth_radius_km, double s_max_km, double rtol, double atol, double max_step_km,
                                 double z_ground_km, double top, double left, double right, int32_t renormalize_every,
                                 double fill_n, double fill_grad, double fill_mup, int32_t n_hops, double* out,
                                 double* path_t, double* path_a, double* path_b, double* path_va, double* path_vb,
                                 int64_t path_stride, uint32_t flags) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (n_hops < 1 || n_hops > PRHF_GRAD_MAX_HOPS) return fail(PRHF_EINVAL, "n_hops is 1 .. 16");
    const GradControls t{geometry, earth_radius_km, s_max_km, rtol, atol, max_step_km, z_ground_km, top, left, right,
                         renormalize_every, fill_n, fill_grad, fill_mup};
    PRHF_TRY(check_grad_geometry(t));
    if (n_rays > 0x7fffffffLL / PRHF_GRAD_MAX_HOPS) return fail(PRHF_EINVAL, "more than 2^27 - 1 rays: trace in batches");
    const FieldGrid f{records, n_fields, n0, n1, axis0, axis1};
    double* const paths[5] = {path_t, path_a, path_b, path_va, path_vb};
    return grad_trace_run(c, n_hops, t, f, x0_km, z0_km, elevation_deg, ray_field, n_rays, out, paths, path_stride, flags);
}

namespace {
// The groups of a homing or skip call: the field and the launch point of each
struct GradGroups {
    const int64_t* field;
    const double *x0_km, *z0_km;
    int64_t n;
};
// ... behind the axes in the arena, for GradHomeArgs and GradSkipArgs alike
template <class Args>
void put_groups(Stager& k, Args& h, const GradGroups& g) {
    h.group_field = k.put<long long>(g.field, (size_t)g.n);
    h.group_x0 = k.put<double>(g.x0_km, (size_t)g.n);
    h.group_z0 = k.put<double>(g.z0_km, (size_t)g.n);
}

// Both homing calls.  n_hops 0: prhf_gradient_home_f64 (rows of 15); else prhf_gradient_hop_home_f64.
int grad_home_run(prhf_ctx* c, int32_t n_hops, const GradControls& t, const FieldGrid& f, const GradGroups& g,
                  const int64_t* link_group, const double* link_target_km, int64_t n_links, const double* scan_elevation_deg,
                  int64_t n_scan, double range_tol_km, int32_t max_iter, int32_t max_roots, double* out, int64_t* n_brackets,
                  uint32_t flags) {
    const int row_width = n_hops ? 3 + PRHF_GRAD_HOP_OUTPUTS * n_hops : PRHF_GRAD_HOME_OUTPUTS;
    const int64_t n_groups = g.n;
    if (!f.records || !g.field || !g.x0_km || !g.z0_km || !link_group || !link_target_km || !scan_elevation_deg || !out ||
        !n_brackets)
        return fail(PRHF_EINVAL, "null array pointer");
    PRHF_TRY(check_grad_controls(t, flags));
    if (n_scan < 2) return fail(PRHF_EINVAL, "the scan grid needs at least 2 elevations");
    if (max_iter < 1 || max_iter > 128) return fail(PRHF_EINVAL, "max_iter is 1 .. 128");
    if (max_roots < 1 || max_roots > 64) return fail(PRHF_EINVAL, "max_roots is 1 .. 64");
    if (!(range_tol_km >= 0.0) || !std::isfinite(range_tol_km))
        return fail(PRHF_EINVAL, "range_tol_km must be finite and not negative");
    if (n_groups < 1) return fail(PRHF_EINVAL, "homing needs at least one group");
    if (n_links < 0) return fail(PRHF_EINVAL, "bad shape");
    if (n_scan > 0x7fffffffLL || n_groups * ((n_scan + 63) / 64) > 0x7fffffffLL || n_links * (int64_t)max_roots > 0x7fffffffLL)
        return fail(PRHF_EINVAL, "more than 2^31 - 1 scan rays or result rows: home in batches");
    int u0 = 0, u1 = 0;
    PRHF_TRY(check_field_shape(f.axis0, f.axis1, f.n_fields, f.n0, f.n1, 2, &u0, &u1));
    const bool dev = (flags & PRHF_FLAG_DEVICE_PTRS) != 0;
    if (!dev) {
        PRHF_TRY(check_scan_grid(scan_elevation_deg, n_scan, false));
        PRHF_TRY(check_index("group_field", g.field, n_groups, "n_fields", f.n_fields));
        PRHF_TRY(check_index("link_group", link_group, n_links, "n_groups", n_groups));
    }
    for (uint64_t& w : c->grad_home_counters) w = 0;
    if (n_links == 0) return PRHF_OK;
    ENTER_DEVICE(c->device);
    const size_t G = (size_t)n_groups, L = (size_t)n_links, E = (size_t)n_scan;
    const size_t out_elems = L * (size_t)max_roots * (size_t)row_width;
    prhf::GradHomeArgs h;
    std::memset(&h, 0, sizeof h);
    grad_trace_args(c, h.g, f, t);
    h.n_groups = n_groups; h.n_links = n_links; h.n_scan = (int)n_scan; h.range_tol = range_tol_km; h.max_iter = max_iter;
    h.max_roots = max_roots; h.row_width = row_width; h.g.n_hops = n_hops ? n_hops : 1; h.g.hop_z0 = t.z_ground_km;
    h.group_field = reinterpret_cast<const long long*>(g.field); h.group_x0 = g.x0_km; h.group_z0 = g.z0_km;
    h.link_group = reinterpret_cast<const long long*>(link_group); h.link_target = link_target_km;
    h.scan_elev = scan_elevation_deg; h.out = out; h.n_brackets = reinterpret_cast<long long*>(n_brackets);
    PRHF_TRY(carve(c, c->arena, [&](Stager& k) {
        put_axes(k, h.g, f.axis0, f.axis1, f.n0, f.n1);
        if (dev) return;
        put_groups(k, h, g);
        h.link_group = k.put<long long>(link_group, L);
        h.link_target = k.put<double>(link_target_km, L);
        h.n_brackets = k.take<long long>(L);
        h.scan_elev = k.put<double>(scan_elevation_deg, E);
        h.out = k.take<double>(out_elems);
    }));
    // the counters, the work list and the scan's ground ranges
    PRHF_TRY(carve(c, c->partial, [&](Stager& k) {
        h.queue = k.take<unsigned>(128 / sizeof(unsigned));
        h.work = k.take<int>(L * (size_t)max_roots * 4);
        h.scan_d = k.take<double>(G * E);
    }));
    PRHF_TRY(timed_launch(c, true, [&] { return prhf::launch_grad_home(h, c->stream); }));
    unsigned counters[PRHF_GRAD_HOME_COUNTERS] = {};
    HIP_TRY(download(c, counters, h.queue, sizeof counters));
    if (!dev) {
        HIP_TRY(download(c, out, h.out, out_elems * 8));
        HIP_TRY(download(c, n_brackets, h.n_brackets, L * 8));
    }
    const int rc = prhf_sync(c);
    for (int k = 0; k < PRHF_GRAD_HOME_COUNTERS; ++k) c->grad_home_counters[k] = counters[k];
    return rc;
}
}  // namespace

int prhf_gradient_home_f64(prhf_ctx* c, int32_t geometry, const double* records, int64_t n_fields, int64_t n0, int64_t n1,
                           const double* axis0, const double* axis1, const int64_t* group_field, const double* group_x0_km,
                           const double* group_z0_km, int64_t n_groups, const int64_t* link_group,
                           const double* link_target_km, int64_t n_links, const double* scan_elevation_deg, int64_t n_scan,
                           double earth_radius_km, double s_max_km, double rtol, double atol, double max_step_km,
                           double z_ground_km, double top, double left, double right, int32_t renormalize_every,
                           double fill_n, double fill_grad, double fill_mup, double range_tol_km, int32_t max_iter,
                           int32_t max_roots, double* out, int64_t* n_brackets, uint32_t flags) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    const GradControls t{geometry, earth_radius_km, s_max_km, rtol, atol, max_step_km, z_ground_km, top, left, right,
                         renormalize_every, fill_n, fill_grad, fill_mup};
    return grad_home_run(c, 0, t, FieldGrid{records, n_fields, n0, n1, axis0, axis1},
                         GradGroups{group_field, group_x0_km, group_z0_km, n_groups}, link_group, link_target_km, n_links,
                         scan_elevation_deg, n_scan, range_tol_km, max_iter, max_roots, out, n_brackets, flags);
}

int prhf_gradient_hop_home_f64(prhf_ctx* c, int32_t geometry, const double* records, int64_t n_fields, int64_t n0, int64_t n1,
                               const double* axis0, const double* axis1, const int64_t* group_field,
                               const double* group_x0_km, const double* group_z0_km, int64_t n_groups,
                               const int64_t* link_group, const double* link_target_km, int64_t n_links,
                               const double* scan_elevation_deg, int64_t n_scan, double earth_radius_km, double s_max_km,
                               double rtol, double atol, double max_step_km, double z_ground_km, double top, double left,
                               double right, int32_t renormalize_every, double fill_n, double fill_grad, double fill_mup,
                               double range_tol_km, int32_t max_iter, int32_t max_roots, int32_t n_hops, double* out,
                               int64_t* n_brackets, uint32_t flags) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (n_hops < 1 || n_hops > PRHF_GRAD_MAX_HOPS) return fail(PRHF_EINVAL, "n_hops is 1 .. 16");
    const GradControls t{geometry, earth_radius_km, s_max_km, rtol, atol, max_step_km, z_ground_km, top, left, right,
                         renormalize_every, fill_n, fill_grad, fill_mup};
    return grad_home_run(c, n_hops, t, FieldGrid{records, n_fields, n0, n1, axis0, axis1},
                         GradGroups{group_field, group_x0_km, group_z0_km, n_groups}, link_group, link_target_km, n_links,
                         scan_elevation_deg, n_scan, range_tol_km, max_iter, max_roots, out, n_brackets, flags);
}

int prhf_gradient_home_counters(prhf_ctx* c, uint64_t* counters) {
    if (!c || !counters) return fail(PRHF_EINVAL, "null pointer");
    for (int k = 0; k < PRHF_GRAD_HOME_COUNTERS; ++k) counters[k] = c->grad_home_counters[k];
    return PRHF_OK;
}

namespace {
// The end of a skip or MUF call of the gradient tracers: the counters come back with the results, one synchronisation
int grad_skip_finish(prhf_ctx* c, const unsigned* queue) {
    unsigned w[PRHF_GRAD_SKIP_QUEUE_WORDS] = {};
    HIP_TRY(download(c, w, queue, sizeof w));
    const int rc = prhf_sync(c);
    c->grad_skip_counters[0] = w[4];
    for (int k = 1; k < PRHF_GRAD_SKIP_COUNTERS; ++k) c->grad_skip_counters[k] = w[k];
    c->grad_skip_counters[PRHF_GRAD_SKIP_COUNTERS] = w[5];
    return rc;
}
// What the skip and MUF calls put into GradSkipArgs alike
void grad_skip_args(prhf::GradSkipArgs& h, int64_t n_groups, int64_t n_scan, double elev_tol_deg, int32_t max_iter, int row_width,
                    int32_t n_hops, const GradControls& t) {
    h.n_groups = n_groups; h.n_scan = (int)n_scan; h.elev_tol = elev_tol_deg; h.max_iter = max_iter;
    h.row_width = row_width; h.g.n_hops = n_hops ? n_hops : 1; h.g.hop_z0 = t.z_ground_km;
}
// ... and the head of their c->partial: the counters, the work list and the scan's ground ranges
void carve_grad_skip_scratch(Carver& k, prhf::GradSkipArgs& h, size_t G, size_t E) {
    h.queue = k.take<unsigned>(128 / sizeof(unsigned));
    h.work = k.take<int>(2 * G);
    h.scan_d = k.take<double>(G * E);
}
}  // namespace

int prhf_field_build_f64(prhf_ctx* c, const double* den, const double* bmag, const double* bpsi, int64_t n0, int64_t n1,
                         const double* axis0, const double* axis1, const double* freq_hz, int64_t n_freq, int32_t mode,
                         int32_t edge_order, double* records, double* mu_out, double* mup_out, uint32_t flags) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (!den || !bmag || !bpsi || !freq_hz || !records) return fail(PRHF_EINVAL, "null array pointer");
    if ((mu_out == nullptr) != (mup_out == nullptr)) return fail(PRHF_EINVAL, "mu_out and mup_out go together");
    if (mode != PRHF_MODE_O && mode != PRHF_MODE_X) return fail(PRHF_EINVAL, "Mode must be O or X");
    if (edge_order != 1 && edge_order != 2) return fail(PRHF_EINVAL, "edge_order is 1 or 2");
    if (flags & ~PRHF_FLAG_DEVICE_PTRS) return fail(PRHF_EINVAL, "unknown flag bits");
    int u0 = 0, u1 = 0;
    PRHF_TRY(check_field_shape(axis0, axis1, n_freq, n0, n1, edge_order + 1, &u0, &u1));
    const bool dev = (flags & PRHF_FLAG_DEVICE_PTRS) != 0;
    const size_t plane = (size_t)n0 * (size_t)n1, F = (size_t)n_freq, cells = F * plane;
    if (!dev)
        for (size_t i = 0; i < plane; ++i)
            if (den[i] < 0) return fail(PRHF_ENEGDEN, "Density must be non-negative");
    ENTER_DEVICE(c->device);
    const bool own_mu = !dev || !mu_out;
    prhf::FieldBuildArgs b;
    std::memset(&b, 0, sizeof b);
    prhf::FieldPackArgs a;
    std::memset(&a, 0, sizeof a);
    b.den = den; b.bmag = bmag; b.bpsi = bpsi; b.freq = freq_hz; b.mu = mu_out; b.mup = mup_out;
    PRHF_TRY(carve(c, c->arena, [&](Stager& k) {
        put_axes(k, a, axis0, axis1, n0, n1);
        if (!dev) {
            b.den = k.put<double>(den, plane);
            b.bmag = k.put<double>(bmag, plane);
            b.bpsi = k.put<double>(bpsi, plane);
            b.freq = k.put<double>(freq_hz, F);
        }
        if (own_mu) {
            b.mu = k.take<double>(cells);
            b.mup = k.take<double>(cells);
        }
    }));
    b.bmax = c->d_words; b.n_freq = n_freq; b.plane = (long long)plane;
    b.mode = mode == PRHF_MODE_O ? PRHF_KMODE_O : PRHF_KMODE_X;
    a.mu = b.mu; a.mup = b.mup; a.rec = records; a.n_fields = n_freq; a.n0 = (int)n0; a.n1 = (int)n1;
    a.uniform0 = u0; a.uniform1 = u1; a.edge_order = edge_order;
    PRHF_TRY(timed_launch(c, false, [&] {
        hipError_t e = prhf::launch_field_bmax(b.bmag, b.plane, c->d_words, c->stream);
        if (e == hipSuccess) e = prhf::launch_field_build(b, c->stream);
        if (e == hipSuccess) e = prhf::launch_field_pack(a, c->stream);
        return e;
    }));
    if (!dev && mu_out) {
        HIP_TRY(download(c, mu_out, b.mu, cells * 8));
        HIP_TRY(download(c, mup_out, b.mup, cells * 8));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PRHF_OK;
}

namespace {
// Both skip calls.  n_hops 0: prhf_gradient_skip_f64 (rows of 18); else prhf_gradient_hop_skip_f64 (6 + 15 n_hops).
int grad_skip_run(prhf_ctx* c, int32_t n_hops, const GradControls& t, const FieldGrid& f, const GradGroups& g,
                  const double* scan_elevation_deg, int64_t n_scan, double elev_tol_deg, int32_t max_iter, double* out,
                  uint32_t flags) {
    const int row_width = n_hops ? PRHF_GRAD_HOP_SKIP_OUTPUTS(n_hops) : PRHF_GRAD_SKIP_OUTPUTS;
    const int64_t n_groups = g.n;
    if (!f.records || !g.field || !g.x0_km || !g.z0_km || !scan_elevation_deg || !out)
        return fail(PRHF_EINVAL, "null array pointer");
    PRHF_TRY(check_grad_controls(t, flags));
    PRHF_TRY(check_grad_search(n_scan, elev_tol_deg, max_iter));
    if (n_groups < 1) return fail(PRHF_EINVAL, "the search needs at least one group");
    if (n_groups > 0x7fffffffLL || n_groups * ((n_scan + 63) / 64) > 0x7fffffffLL)
        return fail(PRHF_EINVAL, "more than 2^31 - 1 groups or scan wavefronts: search in batches");
    int u0 = 0, u1 = 0;
    PRHF_TRY(check_field_shape(f.axis0, f.axis1, f.n_fields, f.n0, f.n1, 2, &u0, &u1));
    const bool dev = (flags & PRHF_FLAG_DEVICE_PTRS) != 0;
    if (!dev) {
        PRHF_TRY(check_scan_grid(scan_elevation_deg, n_scan, true));
        PRHF_TRY(check_index("group_field", g.field, n_groups, "n_fields", f.n_fields));
    }
    for (uint64_t& w : c->grad_skip_counters) w = 0;
    ENTER_DEVICE(c->device);
    const size_t G = (size_t)n_groups, E = (size_t)n_scan, out_elems = G * (size_t)row_width;
    prhf::GradSkipArgs h;
    std::memset(&h, 0, sizeof h);
    grad_trace_args(c, h.g, f, t);
    grad_skip_args(h, n_groups, n_scan, elev_tol_deg, max_iter, row_width, n_hops, t);
    h.group_field = reinterpret_cast<const long long*>(g.field); h.group_x0 = g.x0_km; h.group_z0 = g.z0_km;
    h.scan_elev = scan_elevation_deg; h.out = out;
    PRHF_TRY(carve(c, c->arena, [&](Stager& k) {
        put_axes(k, h.g, f.axis0, f.axis1, f.n0, f.n1);
        if (dev) return;
        put_groups(k, h, g);
        h.scan_elev = k.put<double>(scan_elevation_deg, E);
        h.out = k.take<double>(out_elems);
    }));
    PRHF_TRY(carve(c, c->partial, [&](Stager& k) { carve_grad_skip_scratch(k, h, G, E); }));
    PRHF_TRY(timed_launch(c, true, [&] { return prhf::launch_grad_skip(h, n_hops != 0, c->stream); }));
    if (!dev) HIP_TRY(download(c, out, h.out, out_elems * 8));
    return grad_skip_finish(c, h.queue);
}
}  // namespace

int prhf_gradient_skip_f64(prhf_ctx* c, int32_t geometry, const double* records, int64_t n_fields, int64_t n0, int64_t n1,
                           const double* axis0, const double* axis1, const int64_t* group_field, const double* group_x0_km,
                           const double* group_z0_km, int64_t n_groups, const double* scan_elevation_deg, int64_t n_scan,
                           double earth_radius_km, double s_max_km, double rtol, double atol, double max_step_km,
                           double z_ground_km, double top, double left, double right, int32_t renormalize_every,
                           double fill_n, double fill_grad, double fill_mup, double elev_tol_deg, int32_t max_iter,
                           double* out, uint32_t flags) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    const GradControls t{geometry, earth_radius_km, s_max_km, rtol, atol, max_step_km, z_ground_km, top, left, right,
                         renormalize_every, fill_n, fill_grad, fill_mup};
    return grad_skip_run(c, 0, t, FieldGrid{records, n_fields, n0, n1, axis0, axis1},
                         GradGroups{group_field, group_x0_km, group_z0_km, n_groups}, scan_elevation_deg, n_scan, elev_tol_deg,
                         max_iter, out, flags);
}

int prhf_gradient_hop_skip_f64(prhf_ctx* c, int32_t geometry, const double* records, int64_t n_fields, int64_t n0, int64_t n1,
                               const double* axis0, const double* axis1, const int64_t* group_field,
                               const double* group_x0_km, const double* group_z0_km, int64_t n_groups,
                               const double* scan_elevation_deg, int64_t n_scan, double earth_radius_km, double s_max_km,
                               double rtol, double atol, double max_step_km, double z_ground_km, double top, double left,
                               double right, int32_t renormalize_every, double fill_n, double fill_grad, double fill_mup,
                               double elev_tol_deg, int32_t max_iter, int32_t n_hops, double* out, uint32_t flags) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (n_hops < 1 || n_hops > PRHF_GRAD_MAX_HOPS) return fail(PRHF_EINVAL, "n_hops is 1 .. 16");
    const GradControls t{geometry, earth_radius_km, s_max_km, rtol, atol, max_step_km, z_ground_km, top, left, right,
                         renormalize_every, fill_n, fill_grad, fill_mup};
    return grad_skip_run(c, n_hops, t, FieldGrid{records, n_fields, n0, n1, axis0, axis1},
                         GradGroups{group_field, group_x0_km, group_z0_km, n_groups}, scan_elevation_deg, n_scan, elev_tol_deg,
                         max_iter, out, flags);
}

namespace {
// The one ionosphere of a MUF call (prhf_field_build_f64's inputs) and its links
struct MufIonosphere {
    const double *den, *bmag, *bpsi;
    int64_t n0, n1;
    const double *axis0, *axis1;
    int32_t mode, edge_order;
};
struct MufLinks {
    const double *x0_km, *z0_km, *target_km;
    int64_t n;
    double f_lo_hz, f_hi_hz;
    int32_t n_bisect;
};
// Both MUF calls.  n_hops 0: prhf_gradient_muf_f64 (rows of 21); else prhf_gradient_hop_muf_f64 (3 + 6 + 15 n_hops).
int grad_muf_run(prhf_ctx* c, int32_t n_hops, const GradControls& t, const MufIonosphere& io, const MufLinks& lk,
                 const double* scan_elevation_deg, int64_t n_scan, double elev_tol_deg, int32_t max_iter, double* out,
                 uint32_t flags) {
    const int row_width = n_hops ? PRHF_GRAD_HOP_SKIP_OUTPUTS(n_hops) : PRHF_GRAD_SKIP_OUTPUTS;
    const int64_t n_links = lk.n, n0 = io.n0, n1 = io.n1;
    if (!io.den || !io.bmag || !io.bpsi || !lk.x0_km || !lk.z0_km || !lk.target_km || !scan_elevation_deg || !out)
        return fail(PRHF_EINVAL, "null array pointer");
    PRHF_TRY(check_grad_controls(t, flags));
    PRHF_TRY(check_grad_search(n_scan, elev_tol_deg, max_iter));
    if (io.mode != PRHF_MODE_O && io.mode != PRHF_MODE_X) return fail(PRHF_EINVAL, "Mode must be O or X");
    if (io.edge_order != 1 && io.edge_order != 2) return fail(PRHF_EINVAL, "edge_order is 1 or 2");
    if (lk.n_bisect < 1 || lk.n_bisect > 64) return fail(PRHF_EINVAL, "n_bisect is 1 .. 64");
    if (!(lk.f_lo_hz > 0.0) || !(lk.f_hi_hz > lk.f_lo_hz) || !std::isfinite(lk.f_hi_hz))
        return fail(PRHF_EINVAL, "the frequency bracket needs 0 < f_lo_hz < f_hi_hz, both finite");
    if (n_links < 1) return fail(PRHF_EINVAL, "the search needs at least one link");
    if (n_links * ((n_scan + 63) / 64) > 0x7fffffffLL)
        return fail(PRHF_EINVAL, "more than 2^31 - 1 scan wavefronts: search in batches");
    int u0 = 0, u1 = 0;
    PRHF_TRY(check_field_shape(io.axis0, io.axis1, n_links, n0, n1, io.edge_order + 1 > 2 ? io.edge_order + 1 : 2, &u0, &u1));
    const bool dev = (flags & PRHF_FLAG_DEVICE_PTRS) != 0;
    const size_t plane = (size_t)n0 * (size_t)n1, L = (size_t)n_links, E = (size_t)n_scan;
    if (!dev) {
        PRHF_TRY(check_scan_grid(scan_elevation_deg, n_scan, true));
        for (size_t i = 0; i < plane; ++i)
            if (io.den[i] < 0) return fail(PRHF_ENEGDEN, "Density must be non-negative");
    }
    for (uint64_t& w : c->grad_skip_counters) w = 0;
    ENTER_DEVICE(c->device);
    const size_t out_elems = L * (size_t)(3 + row_width);
    prhf::GradMufArgs m;
    std::memset(&m, 0, sizeof m);
    prhf::GradSkipArgs& h = m.k;
    // one field per link: mu, mu' and the records, 48 bytes per node (made room for before the first upload goes out)
    double* rec = nullptr;
    PRHF_TRY(carve(c, c->fields, [&](Stager& k) {
        m.b.mu = k.take<double>(L * plane);
        m.b.mup = k.take<double>(L * plane);
        rec = k.take<double>(4 * L * plane);
    }));
    m.b.den = io.den; m.b.bmag = io.bmag; m.b.bpsi = io.bpsi;
    h.group_x0 = lk.x0_km; h.group_z0 = lk.z0_km; m.link_target = lk.target_km; h.scan_elev = scan_elevation_deg; m.out = out;
    PRHF_TRY(carve(c, c->arena, [&](Stager& k) {
        put_axes(k, m.p, io.axis0, io.axis1, n0, n1);
        if (dev) return;
        m.b.den = k.put<double>(io.den, plane);
        m.b.bmag = k.put<double>(io.bmag, plane);
        m.b.bpsi = k.put<double>(io.bpsi, plane);
        h.group_x0 = k.put<double>(lk.x0_km, L);
        h.group_z0 = k.put<double>(lk.z0_km, L);
        m.link_target = k.put<double>(lk.target_km, L);
        h.scan_elev = k.put<double>(scan_elevation_deg, E);
        m.out = k.take<double>(out_elems);
    }));
    grad_trace_args(c, h.g, FieldGrid{rec, n_links, n0, n1, io.axis0, io.axis1}, t);
    h.g.a0 = m.p.a0; h.g.a1 = m.p.a1;
    grad_skip_args(h, n_links, n_scan, elev_tol_deg, max_iter, row_width, n_hops, t);
    m.n_links = n_links; m.f_lo = lk.f_lo_hz; m.f_hi = lk.f_hi_hz; m.n_bisect = lk.n_bisect;
    // behind the skip call's scratch, per link: its frequency, field index, bracket, the head of the row at the bracket's
    // lower end, the skip row of the trip and the "is searching" word
    PRHF_TRY(carve(c, c->partial, [&](Stager& k) {
        carve_grad_skip_scratch(k, h, L, E);
        m.group_freq = k.take<double>(L);
        m.group_field = k.take<long long>(L);
        m.state = k.take<double>(4 * L);
        m.best = k.take<double>(L * (PRHF_GRAD_SKIP_OUTPUTS - PRHF_GRAD_OUTPUTS));
        h.out = k.take<double>(L * (size_t)row_width);
        m.active = k.take<int>(L);
    }));
    h.group_field = m.group_field; h.active = m.active;
    m.b.freq = m.group_freq; m.b.active = m.active; m.b.bmax = c->d_words; m.b.n_freq = n_links; m.b.plane = (long long)plane;
    m.b.mode = io.mode == PRHF_MODE_O ? PRHF_KMODE_O : PRHF_KMODE_X;
    m.p.mu = m.b.mu; m.p.mup = m.b.mup; m.p.rec = rec; m.p.n_fields = n_links;
    m.p.n0 = (int)n0; m.p.n1 = (int)n1; m.p.uniform0 = u0; m.p.uniform1 = u1; m.p.edge_order = io.edge_order;
    PRHF_TRY(timed_launch(c, true, [&] { return prhf::launch_grad_muf(m, n_hops != 0, c->stream); }));
    if (!dev) HIP_TRY(download(c, out, m.out, out_elems * 8));
    return grad_skip_finish(c, h.queue);
}
}  // namespace

int prhf_gradient_muf_f64(prhf_ctx* c, int32_t geometry, const double* den, const double* bmag, const double* bpsi, int64_t n0,
                          int64_t n1, const double* axis0, const double* axis1, int32_t mode, int32_t edge_order,
                          const double* link_x0_km, const double* link_z0_km, const double* link_target_km, int64_t n_links,
                          double f_lo_hz, double f_hi_hz, int32_t n_bisect, const double* scan_elevation_deg, int64_t n_scan,
                          double earth_radius_km, double s_max_km, double rtol, double atol, double max_step_km,
                          double z_ground_km, double top, double left, double right, int32_t renormalize_every, double fill_n,
                          double fill_grad, double fill_mup, double elev_tol_deg, int32_t max_iter, double* out, uint32_t flags) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    const GradControls t{geometry, earth_radius_km, s_max_km, rtol, atol, max_step_km, z_ground_km, top, left, right,
                         renormalize_every, fill_n, fill_grad, fill_mup};
    return grad_muf_run(c, 0, t, MufIonosphere{den, bmag, bpsi, n0, n1, axis0, axis1, mode, edge_order},
                        MufLinks{link_x0_km, link_z0_km, link_target_km, n_links, f_lo_hz, f_hi_hz, n_bisect}, scan_elevation_deg,
                        n_scan, elev_tol_deg, max_iter, out, flags);
}

int prhf_gradient_hop_muf_f64(prhf_ctx* c, int32_t geometry, const double* den, const double* bmag, const double* bpsi,
                              int64_t n0, int64_t n1, const double* axis0, const double* axis1, int32_t mode,
                              int32_t edge_order, const double* link_x0_km, const double* link_z0_km,
                              const double* link_target_km, int64_t n_links, double f_lo_hz, double f_hi_hz, int32_t n_bisect,
                              const double* scan_elevation_deg, int64_t n_scan, double earth_radius_km, double s_max_km,
                              double rtol, double atol, double max_step_km, double z_ground_km, double top, double left,
                              double right, int32_t renormalize_every, double fill_n, double fill_grad, double fill_mup,
                              double elev_tol_deg, int32_t max_iter, int32_t n_hops, double* out, uint32_t flags) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    if (n_hops < 1 || n_hops > PRHF_GRAD_MAX_HOPS) return fail(PRHF_EINVAL, "n_hops is 1 .. 16");
    const GradControls t{geometry, earth_radius_km, s_max_km, rtol, atol, max_step_km, z_ground_km, top, left, right,
                         renormalize_every, fill_n, fill_grad, fill_mup};
    return grad_muf_run(c, n_hops, t, MufIonosphere{den, bmag, bpsi, n0, n1, axis0, axis1, mode, edge_order},
                        MufLinks{link_x0_km, link_z0_km, link_target_km, n_links, f_lo_hz, f_hi_hz, n_bisect}, scan_elevation_deg,
                        n_scan, elev_tol_deg, max_iter, out, flags);
}

int prhf_gradient_skip_counters(prhf_ctx* c, uint64_t* counters) {
    if (!c || !counters) return fail(PRHF_EINVAL, "null pointer");
    for (int k = 0; k < PRHF_GRAD_SKIP_COUNTERS; ++k) counters[k] = c->grad_skip_counters[k];
    return PRHF_OK;
}

int prhf_gradient_hop_skip_counters(prhf_ctx* c, uint64_t* counters) {
    if (!c || !counters) return fail(PRHF_EINVAL, "null pointer");
    for (int k = 0; k <= PRHF_GRAD_SKIP_COUNTERS; ++k) counters[k] = c->grad_skip_counters[k];
    return PRHF_OK;
}

namespace {
// n_words of the launches' counters from first_word on (prhf::kPlanCounterWords, since the context was made), once the
// stream has drained
int read_plan_counters(prhf_ctx* c, int first_word, int n_words, uint64_t* dst) {
    if (!c || !dst) return fail(PRHF_EINVAL, "null pointer");
    DeviceScope device_scope_(c->device);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(dst, c->d_plan_counters + first_word, (size_t)n_words * sizeof *dst, hipMemcpyDeviceToHost));
    return PRHF_OK;
}
}  // namespace

int prhf_pair_plan_counters(prhf_ctx* c, uint64_t* counters) { return read_plan_counters(c, 0, 2, counters); }

int prhf_panel_counters(prhf_ctx* c, uint64_t* counters) { return read_plan_counters(c, 2, 2, counters); }

int prhf_panel_upper_counters(prhf_ctx* c, uint64_t* counters) {
    PRHF_TRY(read_plan_counters(c, 4, 2, counters));
    // (the device counts the pairs that took the panel sum with the option on - each of them reports one or the other - and
    //  among them those that kept the lower region)
    counters[0] -= counters[1];
    return PRHF_OK;
}

int prhf_panel_plan_counters(prhf_ctx* c, uint64_t* counters) { return read_plan_counters(c, 6, 1, counters); }

int prhf_panel_quick_counters(prhf_ctx* c, uint64_t* counters) {
    if (!counters) return fail(PRHF_EINVAL, "null pointer");
    uint64_t w[prhf::kQuickSlots * prhf::kQuickSlotWords];
    PRHF_TRY(read_plan_counters(c, prhf::kQuickSlotBase, prhf::kQuickSlots * prhf::kQuickSlotWords, w));
    // (the waves add into one of kQuickSlots slots each: run_items)
    counters[0] = counters[1] = 0;
    for (int s = 0; s < prhf::kQuickSlots; ++s) {
        counters[0] += w[s * prhf::kQuickSlotWords];
        counters[1] += w[s * prhf::kQuickSlotWords + 1];
    }
    return PRHF_OK;
}

int prhf_stream_launches(prhf_ctx* c, uint64_t* count) {
    if (!c || !count) return fail(PRHF_EINVAL, "null pointer");
    *count = c->stream_launches;
    return PRHF_OK;
}

int prhf_occupancy(prhf_ctx* c, int64_t n_alt, int32_t math, int32_t* workgroups_per_cu) {
    if (!c || !workgroups_per_cu) return fail(PRHF_EINVAL, "null pointer");
    if (n_alt < 1 || n_alt > kMaxAlt) return fail(PRHF_EINVAL, "n_alt out of range");
    ENTER_DEVICE(c->device);
    int n = 0;
    HIP_TRY(prhf::query_occupancy(math, staged_lds_bytes(n_alt), &n));
    *workgroups_per_cu = n;
    return PRHF_OK;
}

int prhf_sync(prhf_ctx* c) {
    if (!c) return fail(PRHF_EINVAL, "null context");
    ENTER_DEVICE(c->device);
    ++c->host_waits;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->status_pending) {
        c->status_pending = false;
        unsigned bits = 0;
        for (int b = 0; b < PRHF_STATUS_WORDS; ++b) {
            if (reinterpret_cast<volatile unsigned*>(c->h_status)[b]) bits |= 1u << b;
            c->h_status[b] = 0;
        }
        return status_to_code(bits);
    }
    return PRHF_OK;
}

int prhf_last_kernel_ms(prhf_ctx* c, double* ms) {
    if (!c || !ms) return fail(PRHF_EINVAL, "null pointer");
    if (!c->timed) return fail(PRHF_EINVAL, "no launch has been timed on this context");
    ENTER_DEVICE(c->device);
    HIP_TRY(hipEventSynchronize(c->end_ev()));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, c->ring0[c->slot], c->end_ev()));
    *ms = t;
    return PRHF_OK;
}

int prhf_recent_kernel_ms(prhf_ctx* c, double* ms, int32_t capacity, int32_t* n_out) {
    if (!c || !ms || !n_out || capacity < 0) return fail(PRHF_EINVAL, "null pointer or negative capacity");
    ENTER_DEVICE(c->device);
    long long n = (long long)std::min<unsigned long long>(c->n_timed, (unsigned long long)prhf_ctx::kTimingRing);
    if (n > capacity) n = capacity;
    *n_out = (int32_t)n;
    if (n == 0) return PRHF_OK;
    HIP_TRY(hipEventSynchronize(c->end_ev()));             // the newest; the older ones completed before it
    for (long long i = 0; i < n; ++i) {                      // oldest first
        const int s = (int)((c->n_timed - (unsigned long long)n + (unsigned long long)i) % prhf_ctx::kTimingRing);
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, c->ring0[s], c->ring1[s]));
        ms[i] = t;
    }
    return PRHF_OK;
}
