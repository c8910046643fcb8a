// ---------------------------------------------------------------------------------------
// Many ionograms in one launch (DESIGN.md 4.5 "many ionograms"): residual_kernel's rule per (ionogram, candidate row),
// restricted to the frequencies of the common grid at which that ionogram has an observation, and the winning
// candidate of every ionogram.  Included by prhf_kernels.hip behind residual_kernel, whose additions these repeat.
//
// K_i = { f : vh_obs[i, f] is finite }.  The j-th member of K_i (rank by ballot and popcount prefix over the grid in
// chunks of 64) sits in slot j of the wave's LDS lists (its grid index and its observation; the ballot of every chunk
// is kept beside them for the NaNs of the dense residual rows), and lane l reads the
// slots l, l + 64, l + 128, ...: the lane and the trip residual_kernel gives element j of the compacted row
// vh_model[p, K_i] - so the three lane sums, their wave reductions, fill, residuals and cost are that kernel's bit for
// bit.  A wave walks items_per_wave consecutive items and rebuilds its lists only when the ionogram changes: rows of one
// ionogram are contiguous (own candidates), and with shared candidates item q = i C + c.  Nothing depends on how the
// items are cut over waves; no atomics.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ bool many_finite(double v) { return fabs(v) < __builtin_inf(); }

__global__ void __launch_bounds__(256) residual_many_kernel(ResidualManyArgs a) {
    extern __shared__ __attribute__((aligned(16))) double many_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int F = a.n_freq, Fp = (F + 1) & ~1;
    double* kobs = many_lds + (size_t)wave * Fp;                                          // observation of slot j
    int* kidx = reinterpret_cast<int*>(many_lds + (size_t)waves * Fp) + (size_t)wave * Fp;   // grid index of slot j
    const int chunks = (F + 63) >> 6;
    unsigned long long* kmask = reinterpret_cast<unsigned long long*>(reinterpret_cast<int*>(many_lds + (size_t)waves * Fp) +
                                                                      (size_t)waves * Fp) + (size_t)wave * chunks;   // kept bits of chunk c
    const long long q0 = ((long long)blockIdx.x * waves + wave) * a.items_per_wave;
    const long long q1 = (q0 + a.items_per_wave < a.n_items) ? q0 + a.items_per_wave : a.n_items;
    int cur = -1, K = 0;
    for (long long q = q0; q < q1; ++q) {
        long long row = q;
        int i;
        if (a.ionogram_of_row) {
            i = a.ionogram_of_row[q];
        } else {
            i = (int)(q / a.n_rows);
            row = q - (long long)i * a.n_rows;
        }
        i = uniform(i);
        double* res = a.residual ? a.residual + row * F : nullptr;
        if ((unsigned)i >= (unsigned)a.n_iono) {
            // an index that names no ionogram (device buffers: the host never saw it): nothing of vh_obs is read
            if (res)
                for (int f = lane; f < F; f += 64) res[f] = qnan();
            if (lane == 0) a.cost[q] = qnan();
            continue;
        }
        const double* obs = a.vh_obs + (long long)i * F;
        if (i != cur) {
            __builtin_amdgcn_wave_barrier();           // the lists' readers of the previous ionogram are done
            K = 0;
            for (int base = 0; base < F; base += 64) {
                const int f = base + lane;
                const double o = (f < F) ? obs[f] : qnan();
                const bool kept = many_finite(o);
                const unsigned long long mask = __ballot(kept);
                const int rank = K + __popcll(mask & ((1ull << lane) - 1ull));
                if (kept) {                            // rank < |K_i| <= F
                    kidx[rank] = f;
                    kobs[rank] = o;
                }
                if (lane == 0) kmask[base >> 6] = mask;
                K += __popcll(mask);
            }
            __builtin_amdgcn_wave_barrier();           // (one wave: its LDS operations complete in order)
            cur = i;
        }
        if (res)
            for (int f = lane; f < F; f += 64)
                if (!((kmask[f >> 6] >> lane) & 1ull)) res[f] = qnan();
        const double* v = a.vh_model + row * F;
        double sum = 0.0, cnt = 0.0;
        for (int j = lane; j < K; j += 64) {
            const double m = fabs(v[kidx[j]]);
            if (m == m) { sum += m; cnt += 1.0; }
        }
        sum = wave_sum(sum);
        cnt = wave_sum(cnt);
        const double mean = (cnt > 0.0) ? sum / cnt : qnan();
        const double fill = (mean == mean) ? fmax(mean, 100.0) : qnan();
        double c = 0.0;
        for (int j = lane; j < K; j += 64) {
            const int f = kidx[j];
            double m = v[f];
            if (!(m == m)) m = fill;
            const double r = kobs[j] - m;
            if (res) res[f] = r;
            c += r * r;
        }
        c = wave_sum(c);
        if (lane == 0) a.cost[q] = (K > 0) ? c : qnan();
    }
}

// One wavefront per ionogram: the lexicographic minimum of (cost, row) over the finite costs of its rows.
// Own candidates: the rows are found by bisection of the non-decreasing ionogram_of_row and taken only where the entry
// is the ionogram's (an unsorted device array is read within its bounds and misses rows, nothing else).
__global__ void __launch_bounds__(256) residual_best_kernel(const double* __restrict__ cost, const int* __restrict__ ionogram_of_row,
                                                            long long n_rows, int n_iono, long long* __restrict__ best,
                                                            double* __restrict__ best_cost) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n_iono) return;
    long long lo = 0, hi = n_rows;
    const double* c = cost;
    if (ionogram_of_row) {
        auto first_not_below = [&](long long key) {
            long long l = 0, h = n_rows;
            while (l < h) {
                const long long mid = l + ((h - l) >> 1);
                if (ionogram_of_row[mid] < key) l = mid + 1; else h = mid;
            }
            return l;
        };
        lo = first_not_below(i);
        hi = first_not_below(i + 1);
    } else {
        c = cost + i * n_rows;
    }
    constexpr int kNone = 0x7fffffff;
    double bc = __builtin_inf();
    int br = kNone;
    for (long long r = lo + lane; r < hi; r += 64) {
        if (ionogram_of_row && ionogram_of_row[r] != (int)i) continue;
        const double v = c[r];
        if (many_finite(v) && v < bc) { bc = v; br = (int)r; }       // rows ascend on a lane: the first of equals stays
    }
    auto take = [&](double oc, int orow) {
        if (oc < bc || (oc == bc && orow < br)) { bc = oc; br = orow; }
    };
    {
        double pc, qc;
        int pr, qr;
        halves(bc, &pc, &qc);
        halves(br, &pr, &qr);
        bc = pc; br = pr;
        take(qc, qr);
    }
    { const double oc = lane_xor<16>(bc); const int orow = lane_xor<16>(br); take(oc, orow); }
    { const double oc = lane_xor<8>(bc); const int orow = lane_xor<8>(br); take(oc, orow); }
    { const double oc = lane_xor<4>(bc); const int orow = lane_xor<4>(br); take(oc, orow); }
    { const double oc = lane_xor<2>(bc); const int orow = lane_xor<2>(br); take(oc, orow); }
    { const double oc = lane_xor<1>(bc); const int orow = lane_xor<1>(br); take(oc, orow); }
    if (lane == 0) {
        best[i] = (br == kNone) ? -1 : (long long)br;
        best_cost[i] = (br == kNone) ? qnan() : bc;
    }
}

// the lists of a wave: 12 bytes per grid frequency and 8 per chunk of 64; four waves per workgroup up to 1024
// frequencies, one above
static int residual_many_waves(int n_freq) { return n_freq <= 1024 ? 4 : 1; }

hipError_t launch_residual_many(const ResidualManyArgs& a, hipStream_t stream) {
    if (a.n_freq < 1 || a.n_freq > PRHF_MANY_MAX_FREQ || a.items_per_wave < 1 || a.n_iono < 0 || !a.cost) return hipErrorInvalidValue;
    if (a.n_items <= 0) return hipSuccess;
    const int waves = residual_many_waves(a.n_freq);
    const long long n_waves = (a.n_items + a.items_per_wave - 1) / a.items_per_wave;
    const long long blocks = (n_waves + waves - 1) / waves;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const size_t lds = (size_t)waves * ((size_t)((a.n_freq + 1) & ~1) * 12 + (size_t)((a.n_freq + 63) >> 6) * 8);
    hipLaunchKernelGGL(residual_many_kernel, dim3((unsigned)blocks), dim3((unsigned)waves * 64), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_residual_best(const double* cost, const int* ionogram_of_row, long long n_rows, int n_iono, long long* best,
                                double* best_cost, hipStream_t stream) {
    if (n_iono <= 0) return hipSuccess;
    const long long blocks = ((long long)n_iono + 3) / 4;
    hipLaunchKernelGGL(residual_best_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, cost, ionogram_of_row,
                       n_rows, n_iono, best, best_cost);
    return hipGetLastError();
}
