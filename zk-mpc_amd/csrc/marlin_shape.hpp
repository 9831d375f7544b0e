// marlin_shape.hpp -- the integer half of Marlin::index: from ConstraintMatrices as to_matrices() gives them to the padded, square,
// balanced matrices the arithmetisation reads, and their transposes over H.  Host C++ only (no HIP in this header: it compiles with
// plain g++, tests/marlin_shape_main.cpp drives it alone).
//
// Replaces (reference):
//   pad_input_for_indexer_and_prover, make_matrices_square_for_indexer   arkworks/marlin/src/ahp/constraint_systems.rs:74-113
//   balance_matrices                                                     constraint_systems.rs:23-40
//   the per-row sort by column of arithmetize_matrix                     constraint_systems.rs:188-190
//   EvaluationDomain::reindex_by_subdomain                               poly/src/domain/mod.rs:195-217
//   the index sizes and AHPForR1CS::max_degree                           ahp/indexer.rs:121-208, ahp/mod.rs:75-97
#pragma once
#include "../../include/zkmpc_hip.h"
#include <algorithm>
#include <cstdint>
#include <vector>

namespace zk_marlin {

struct Csr {
    std::vector<uint32_t> row_ptr, col;
    std::vector<zk_fr> coeff;
    size_t rows() const { return row_ptr.size() - 1; }
    size_t nnz() const { return col.size(); }
};

struct Shape {
    zk_marlin_ix_info info;
    Csr m[3];                       // A, B (balanced), C: padded, square, every row in ascending column order (stable)
    Csr t[3];                       // their transposes with rows re-indexed into H: |H| rows, the columns are source rows in source order
    std::vector<uint8_t> swapped;   // balance_matrices: row k of A and B changed places
};

inline size_t next_pow2(size_t n) {
    size_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

// the position in the domain of size `self` of element `index` of a listing that puts the sub-domain of size `other` first
inline size_t reindex_by_subdomain(size_t self, size_t other, size_t index) {
    const size_t period = self / other;
    if (index < other) return index * period;
    const size_t i = index - other, x = period - 1;      // (index >= other needs self > other: x >= 1)
    return i + i / x + 1;
}

// What is wrong with the caller's matrices, or NULL.  Every row_ptr starts at 0 and never decreases, every column is a variable.
inline const char* check(const zk_r1cs_host* h) {
    if (!h) return "null system";
    if (h->num_instance == 0) return "num_instance = 0 (the instance holds at least the constant 1)";
    const size_t nv = h->num_instance + h->num_witness;
    if (nv < h->num_instance || nv >= ((size_t)1 << 31) || h->num_constraints >= ((size_t)1 << 31)) return "system too large";
    const uint32_t* rps[3] = {h->a_row_ptr, h->b_row_ptr, h->c_row_ptr};
    const uint32_t* cols[3] = {h->a_col, h->b_col, h->c_col};
    const zk_fr* cos[3] = {h->a_coeff, h->b_coeff, h->c_coeff};
    for (int k = 0; k < 3; k++) {
        const uint32_t* rp = rps[k];
        if (!rp) return "null row_ptr";
        if (rp[0] != 0) return "a row_ptr that does not start at 0";
        for (size_t r = 0; r < h->num_constraints; r++)
            if (rp[r + 1] < rp[r]) return "a row_ptr that decreases";
        const size_t nnz = rp[h->num_constraints];
        if (nnz && (!cols[k] || !cos[k])) return "null col / coeff";
        for (size_t e = 0; e < nnz; e++)
            if (cols[k][e] >= nv) return "a column that is not below num_instance + num_witness";
    }
    return nullptr;
}

namespace detail {

// rows of `src` (or, where take_other[k], of `other`) as the padded matrix: columns of witnesses moved up by `extra`, `rows` rows in
// all (the ones past the source are empty), every row stably sorted by column
inline void build(const uint32_t* rp_a, const uint32_t* col_a, const zk_fr* co_a, const uint32_t* rp_b, const uint32_t* col_b, const zk_fr* co_b,
                  const std::vector<uint8_t>* take_b, size_t nc_in, size_t rows, size_t ni_in, size_t extra, Csr* out) {
    out->row_ptr.assign(rows + 1, 0);
    size_t total = 0;
    for (size_t r = 0; r < nc_in; r++) {
        const uint32_t* rp = take_b && (*take_b)[r] ? rp_b : rp_a;
        total += rp[r + 1] - rp[r];
        out->row_ptr[r + 1] = (uint32_t)total;
    }
    for (size_t r = nc_in; r < rows; r++) out->row_ptr[r + 1] = (uint32_t)total;
    out->col.resize(total);
    out->coeff.resize(total);
    std::vector<uint32_t> order;
    for (size_t r = 0; r < nc_in; r++) {
        const bool b = take_b && (*take_b)[r];
        const uint32_t* rp = b ? rp_b : rp_a;
        const uint32_t* col = b ? col_b : col_a;
        const zk_fr* co = b ? co_b : co_a;
        const uint32_t lo = rp[r], n = rp[r + 1] - lo, dst = out->row_ptr[r];
        bool sorted = true;
        for (uint32_t j = 1; j < n; j++) sorted = sorted && col[lo + j - 1] <= col[lo + j];
        order.resize(n);
        for (uint32_t j = 0; j < n; j++) order[j] = lo + j;
        // (the shift keeps the order of columns: instance columns stay below every witness column)
        if (!sorted) std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return col[x] < col[y]; });
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t c = col[order[j]];
            out->col[dst + j] = c < ni_in ? c : (uint32_t)(c + extra);
            out->coeff[dst + j] = co[order[j]];
        }
    }
}

// counting sort by the re-indexed column: the entries of a transposed row keep the source's row-major order
inline void transpose(const Csr& m, size_t h_size, size_t x_size, Csr* out) {
    out->row_ptr.assign(h_size + 1, 0);
    out->col.resize(m.nnz());
    out->coeff.resize(m.nnz());
    for (size_t e = 0; e < m.nnz(); e++) out->row_ptr[reindex_by_subdomain(h_size, x_size, m.col[e]) + 1]++;
    for (size_t r = 0; r < h_size; r++) out->row_ptr[r + 1] += out->row_ptr[r];
    std::vector<uint32_t> next(out->row_ptr.begin(), out->row_ptr.end() - 1);
    for (size_t r = 0; r < m.rows(); r++)
        for (uint32_t e = m.row_ptr[r]; e < m.row_ptr[r + 1]; e++) {
            const uint32_t at = next[reindex_by_subdomain(h_size, x_size, m.col[e])]++;
            out->col[at] = (uint32_t)r;
            out->coeff[at] = m.coeff[e];
        }
}

}  // namespace detail

// The sizes alone (what a refusal for a short SRS needs before anything is built).  `h` has passed check().
inline zk_marlin_ix_info sizes(const zk_r1cs_host* h) {
    zk_marlin_ix_info s{};
    s.num_instance_in = h->num_instance; s.num_witness_in = h->num_witness; s.num_constraints_in = h->num_constraints;
    s.num_instance = next_pow2(h->num_instance);
    const size_t nv = s.num_instance + h->num_witness;
    // more variables than constraints: empty rows (0 * 0 = 0); otherwise unconstrained witnesses of value one
    s.num_constraints = std::max(nv, h->num_constraints);
    s.num_witness = s.num_constraints - s.num_instance;
    s.num_non_zero = std::max<size_t>({h->a_row_ptr[h->num_constraints], h->b_row_ptr[h->num_constraints], h->c_row_ptr[h->num_constraints]});
    s.h_size = next_pow2(s.num_constraints);
    s.k_size = next_pow2(s.num_non_zero);
    s.b_size = next_pow2(3 * s.k_size - 3);
    s.x_size = s.num_instance;
    // AHPForR1CS::max_degree with zk_bound = 1
    s.max_degree_needed = std::max({2 * s.h_size - 1, 3 * s.h_size - 1, s.h_size, 3 * s.k_size - 3});
    return s;
}

// The greedy walk of balance_matrices over the row lengths: the denser matrix hands its row to the other one.
inline std::vector<uint8_t> balance_swaps(const uint32_t* rp_a, const uint32_t* rp_b, size_t rows) {
    uint64_t da = rp_a[rows], db = rp_b[rows];
    std::vector<uint8_t> swap(rows, 0);
    bool a_is_denser = da >= db;
    for (size_t k = 0; k < rows; k++) {
        if (!a_is_denser) continue;
        const uint64_t la = rp_a[k + 1] - rp_a[k], lb = rp_b[k + 1] - rp_b[k];
        swap[k] = 1;
        da = da - la + lb;
        db = db - lb + la;
        a_is_denser = da >= db;
    }
    return swap;
}

inline void shape(const zk_r1cs_host* h, Shape* out) {
    out->info = sizes(h);
    const zk_marlin_ix_info& s = out->info;
    const size_t extra = s.num_instance - s.num_instance_in, nc_in = s.num_constraints_in;
    // (rows added by squaring are empty in both matrices: the walk over them changes no density, and swapping them changes nothing)
    out->swapped = balance_swaps(h->a_row_ptr, h->b_row_ptr, nc_in);
    std::vector<uint8_t> not_swapped(nc_in);
    for (size_t k = 0; k < nc_in; k++) not_swapped[k] = !out->swapped[k];
    // new A: B's row where swapped; new B: A's row where swapped
    detail::build(h->a_row_ptr, h->a_col, h->a_coeff, h->b_row_ptr, h->b_col, h->b_coeff, &out->swapped, nc_in, s.num_constraints, s.num_instance_in, extra, &out->m[0]);
    detail::build(h->a_row_ptr, h->a_col, h->a_coeff, h->b_row_ptr, h->b_col, h->b_coeff, &not_swapped, nc_in, s.num_constraints, s.num_instance_in, extra, &out->m[1]);
    detail::build(h->c_row_ptr, h->c_col, h->c_coeff, nullptr, nullptr, nullptr, nullptr, nc_in, s.num_constraints, s.num_instance_in, extra, &out->m[2]);
    for (int k = 0; k < 3; k++) detail::transpose(out->m[k], s.h_size, s.x_size, &out->t[k]);
}

}  // namespace zk_marlin
