// prhf_layouts.h - what the operator and the stage ops keep in the context's arena on a host-buffer call, each block
// stated once as a function of a Carver (prhf_arena.h): the pass over a null base sizes the arena, the pass over the
// arena gives the pointers.  Standard library only: compiled into prhf_api.cpp and into tests/devtools/arena_host.cpp.

#ifndef PRHF_LAYOUTS_H
#define PRHF_LAYOUTS_H

#include <cstdint>

#include "prhf_arena.h"

namespace {

// The operator's inputs.  field_rows: 1 with a shared field, else n_prof; alt_rows: n_prof with an altitude row per
// profile, else 1; mult_len: 0 where a cached stable grid supplies the multiplier.  The result rows and the optional
// residual block lie behind them (stage_inputs, run_host_slabs, stage_derivative).
struct OperatorShape {
    size_t n_freq, n_prof, n_alt, field_rows, alt_rows, mult_len;
};
struct OperatorBlock {
    double *freq, *den, *bmag, *bpsi, *alt, *mult;
};
OperatorBlock operator_block(Carver& k, const OperatorShape& s) {
    OperatorBlock b;
    b.freq = k.take<double>(s.n_freq);
    b.den = k.take<double>(s.n_prof * s.n_alt);
    b.bmag = k.take<double>(s.field_rows * s.n_alt);
    b.bpsi = k.take<double>(s.field_rows * s.n_alt);
    b.alt = k.take<double>(s.alt_rows * s.n_alt);
    b.mult = k.take<double>(s.mult_len);
    return b;
}

// The residual stage against one trace: observations, residual rows, costs (the rows keep their room where the caller
// asks for costs only)
struct ResidualBlock {
    double *obs, *residual, *cost;
};
ResidualBlock residual_block(Carver& k, size_t n_freq, size_t row_elems, size_t n_prof) {
    ResidualBlock b;
    b.obs = k.take<double>(n_freq);
    b.residual = k.take<double>(row_elems);
    b.cost = k.take<double>(n_prof);
    return b;
}

// ... against many ionograms.  by_row: ionogram_of_row names each row's ionogram and there is a cost per row; else
// every ionogram weighs every row (shared candidates).  residual_elems: 0 where no residual rows are asked for.
size_t many_cost_elems(size_t n_rows, size_t n_iono, bool by_row) { return n_rows * (by_row ? 1 : n_iono); }
struct ManyBlock {
    double *obs, *residual, *cost, *best_cost;
    int64_t* best;
    int32_t* ionogram_of_row;
};
ManyBlock many_block(Carver& k, size_t n_iono, size_t n_freq, size_t n_rows, size_t residual_elems, bool by_row) {
    ManyBlock b;
    b.obs = k.take<double>(n_iono * n_freq);
    b.residual = k.take<double>(residual_elems);
    b.cost = k.take<double>(many_cost_elems(n_rows, n_iono, by_row));
    b.best_cost = k.take<double>(n_iono);
    b.best = k.take<int64_t>(n_iono);
    b.ionogram_of_row = k.take<int32_t>(n_rows);
    return b;
}

// The stage ops: n values of each input, then of each output
struct MuMupBlock {
    double *in[3], *out[2];                   // X, Y, psi; mu, mu'
};
MuMupBlock mu_mup_block(Carver& k, size_t n) {
    MuMupBlock b;
    for (double*& p : b.in) p = k.take<double>(n);
    for (double*& p : b.out) p = k.take<double>(n);
    return b;
}

struct FindVhBlock {
    double *in[4], *vh;                       // X, Y, psi, dh (n_rows, n_cols); vh (n_rows)
};
FindVhBlock find_vh_block(Carver& k, size_t n_rows, size_t n_cols) {
    FindVhBlock b;
    for (double*& p : b.in) p = k.take<double>(n_rows * n_cols);
    b.vh = k.take<double>(n_rows);
    return b;
}

struct RegridBlock {
    double *freq, *col[4], *mult, *out[7];    // den, bmag, bpsi, alt; freq, den, bmag, bpsi, dist, alt, crit (n_freq, n_points)
    long long* ind;
};
RegridBlock regrid_block(Carver& k, size_t n_freq, size_t n_alt, size_t n_points) {
    RegridBlock b;
    b.freq = k.take<double>(n_freq);
    for (double*& p : b.col) p = k.take<double>(n_alt);
    b.mult = k.take<double>(n_points);
    for (double*& p : b.out) p = k.take<double>(n_freq * n_points);
    b.ind = k.take<long long>(n_freq * n_points);
    return b;
}

// The two axes of a field (host memory in every call), in front of what a host-buffer call adds: mu, mu' of `cells`
// nodes (prhf_field_pack_f64); p0, p1, field_index and four outputs of n points (prhf_field_sample_f64).  A
// device-pointer call keeps the axes only: cells = 0, n = 0.
struct FieldPackBlock {
    double *a0, *a1, *mu, *mup;
};
FieldPackBlock field_pack_block(Carver& k, size_t n0, size_t n1, size_t cells) {
    FieldPackBlock b;
    b.a0 = k.take<double>(n0);
    b.a1 = k.take<double>(n1);
    b.mu = k.take<double>(cells);
    b.mup = k.take<double>(cells);
    return b;
}
struct FieldSampleBlock {
    double *a0, *a1, *p0, *p1;
    long long* field;
    double* out[4];
};
FieldSampleBlock field_sample_block(Carver& k, size_t n0, size_t n1, size_t n) {
    FieldSampleBlock b;
    b.a0 = k.take<double>(n0);
    b.a1 = k.take<double>(n1);
    b.p0 = k.take<double>(n);
    b.p1 = k.take<double>(n);
    b.field = k.take<long long>(n);
    for (double*& p : b.out) p = k.take<double>(n);
    return b;
}

}  // namespace

#endif  // PRHF_LAYOUTS_H
