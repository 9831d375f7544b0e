// The integer half of Marlin::index (zk-mpc_amd/csrc/marlin_shape.hpp) on generated systems: a self-checking driver for
// tests/test_marlin_shape_host.py.  Prints "ok" and returns 0, or names the first expectation that failed.  The entry-for-entry
// comparison with the oracle is the Python test's; here are the invariants, on many more shapes, in a build a sanitizer can watch.
#include "marlin_shape.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <map>
#include <tuple>
#include <vector>

using namespace zk_marlin;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); }  \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {                                     // xorshift64*: any stream will do
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

struct Sys {
    size_t ni, nw, nc;
    std::vector<uint32_t> rp[3], col[3];
    std::vector<zk_fr> co[3];
    zk_r1cs_host host() const {
        zk_r1cs_host h{};
        h.num_constraints = nc; h.num_instance = ni; h.num_witness = nw;
        h.a_row_ptr = rp[0].data(); h.a_col = col[0].data(); h.a_coeff = co[0].data();
        h.b_row_ptr = rp[1].data(); h.b_col = col[1].data(); h.b_coeff = co[1].data();
        h.c_row_ptr = rp[2].data(); h.c_col = col[2].data(); h.c_coeff = co[2].data();
        return h;
    }
};

// max_len[k]: the longest row of matrix k (0: the matrix is empty).  Every coefficient is unique: it names its entry.
static Sys make(size_t ni, size_t nw, size_t nc, const size_t max_len[3]) {
    Sys s{ni, nw, nc, {}, {}, {}};
    uint64_t tag = 1;
    for (int k = 0; k < 3; k++) {
        s.rp[k].push_back(0);
        for (size_t r = 0; r < nc; r++) {
            const size_t n = max_len[k] ? rnd() % (max_len[k] + 1) : 0;
            for (size_t j = 0; j < n; j++) {
                s.col[k].push_back((uint32_t)(rnd() % (ni + nw)));      // unsorted, repeats allowed
                s.co[k].push_back(zk_fr{{tag++, (uint64_t)k, r, j}});
            }
            s.rp[k].push_back((uint32_t)s.col[k].size());
        }
        s.col[k].push_back(0); s.co[k].push_back(zk_fr{});              // (data() of an empty vector may be null)
    }
    return s;
}

static void check_system(const Sys& s) {
    const zk_r1cs_host h = s.host();
    CHECK(check(&h) == nullptr);
    Shape sh;
    shape(&h, &sh);
    const zk_marlin_ix_info& f = sh.info;
    // square, the instance a power of two, nothing shrinks
    CHECK((f.num_instance & (f.num_instance - 1)) == 0 && f.num_instance >= s.ni && f.num_instance < 2 * s.ni);
    CHECK(f.num_instance + f.num_witness == f.num_constraints);
    CHECK(f.num_constraints == std::max(s.nc, f.num_instance + s.nw) && f.num_witness >= s.nw);
    CHECK(f.h_size >= f.num_constraints && f.h_size < 2 * f.num_constraints && f.k_size >= f.num_non_zero && f.x_size == f.num_instance);
    CHECK(f.b_size >= 3 * f.k_size - 3 && f.max_degree_needed >= 3 * f.h_size - 1 && f.max_degree_needed >= 3 * f.k_size - 3);
    size_t nnz_in[3];
    for (int k = 0; k < 3; k++) nnz_in[k] = s.rp[k][s.nc];
    CHECK(f.num_non_zero == std::max({nnz_in[0], nnz_in[1], nnz_in[2]}));
    const size_t extra = f.num_instance - s.ni;
    // the greedy rule replayed on the row lengths
    std::vector<uint8_t> want(s.nc, 0);
    {
        long long da = (long long)nnz_in[0], db = (long long)nnz_in[1];
        for (size_t r = 0; r < s.nc; r++) {
            if (da < db) continue;
            const long long la = s.rp[0][r + 1] - s.rp[0][r], lb = s.rp[1][r + 1] - s.rp[1][r];
            want[r] = 1;
            da += lb - la; db += la - lb;
        }
    }
    CHECK(sh.swapped == want);
    for (int k = 0; k < 3; k++) {
        const Csr& m = sh.m[k];
        CHECK(m.rows() == f.num_constraints && m.row_ptr[0] == 0 && m.nnz() == m.row_ptr.back() && m.coeff.size() == m.nnz());
        for (size_t r = 0; r < m.rows(); r++) {
            // where row r came from: its own matrix, or for A and B the other one
            const int src = k < 2 && r < s.nc && want[r] ? 1 - k : k;
            const size_t lo = r < s.nc ? s.rp[src][r] : 0, n = r < s.nc ? s.rp[src][r + 1] - lo : 0;
            CHECK(m.row_ptr[r + 1] - m.row_ptr[r] == n);
            std::vector<std::pair<uint32_t, uint64_t>> exp;                  // (shifted column, tag), stably sorted by column
            for (size_t j = 0; j < n; j++) {
                const uint32_t c = s.col[src][lo + j];
                exp.push_back({c < s.ni ? c : (uint32_t)(c + extra), s.co[src][lo + j].l[0]});
            }
            std::stable_sort(exp.begin(), exp.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
            for (size_t j = 0; j < n; j++) {
                const size_t e = m.row_ptr[r] + j;
                CHECK(m.col[e] == exp[j].first && m.coeff[e].l[0] == exp[j].second);         // entries conserved, in order
                CHECK(m.col[e] < f.num_constraints);
                CHECK(j == 0 || m.col[e - 1] <= m.col[e]);                                   // rows sorted
            }
        }
        // the transpose agrees with its matrix: the same entries, row r of H holding those of the column that re-indexes to r,
        // in the matrix's row-major order
        const Csr& t = sh.t[k];
        CHECK(t.rows() == f.h_size && t.nnz() == m.nnz() && t.row_ptr[0] == 0 && t.row_ptr.back() == m.nnz());
        std::vector<std::vector<std::pair<uint32_t, uint64_t>>> by_row(f.h_size);
        for (size_t r = 0; r < m.rows(); r++)
            for (uint32_t e = m.row_ptr[r]; e < m.row_ptr[r + 1]; e++) {
                const size_t at = reindex_by_subdomain(f.h_size, f.x_size, m.col[e]);
                CHECK(at < f.h_size);
                by_row[at].push_back({(uint32_t)r, m.coeff[e].l[0]});
            }
        for (size_t r = 0; r < f.h_size; r++) {
            CHECK(t.row_ptr[r + 1] - t.row_ptr[r] == by_row[r].size());
            for (size_t j = 0; j < by_row[r].size(); j++) {
                const size_t e = t.row_ptr[r] + j;
                CHECK(t.col[e] == by_row[r][j].first && t.coeff[e].l[0] == by_row[r][j].second);
            }
        }
    }
    // re-indexing is a bijection of the variables into H that sends instance i to i |H| / |X|
    std::vector<uint8_t> seen(f.h_size, 0);
    for (size_t c = 0; c < f.num_constraints; c++) {
        const size_t at = reindex_by_subdomain(f.h_size, f.x_size, c);
        CHECK(at < f.h_size && !seen[at]);
        seen[at] = 1;
        if (c < f.x_size) CHECK(at == c * (f.h_size / f.x_size));
    }
}

int main() {
    const size_t dense[3] = {5, 2, 4}, chain[3] = {1, 1, 1}, b_heavy[3] = {1, 6, 2}, no_c[3] = {3, 3, 0}, none[3] = {0, 0, 0};
    const std::tuple<size_t, size_t, size_t> shapes[] = {{1, 0, 1}, {1, 1, 1}, {2, 3, 10}, {2, 9, 4}, {3, 3, 3}, {4, 4, 8}, {5, 2, 7},
                                                         {7, 30, 40}, {8, 120, 64}, {2, 33, 31}, {16, 16, 32}, {3, 61, 64}, {2, 1000, 998}};
    size_t runs = 0;
    for (const auto& [ni, nw, nc] : shapes)
        for (const size_t* lens : {dense, chain, b_heavy, no_c, none})
            for (int rep = 0; rep < 3; rep++, runs++) check_system(make(ni, nw, nc, lens));

    // what check() refuses
    const Sys good = make(2, 4, 4, dense);
    {
        zk_r1cs_host h = good.host();
        CHECK(check(&h) == nullptr && check(nullptr) != nullptr);
        h.num_instance = 0; CHECK(check(&h) != nullptr);
        h = good.host(); h.b_row_ptr = nullptr; CHECK(check(&h) != nullptr);
        Sys bad = good; bad.rp[0][0] = 1; h = bad.host(); CHECK(check(&h) != nullptr);
        bad = good; bad.rp[2][2] = bad.rp[2][1] + 7; bad.rp[2][3] = bad.rp[2][2] - 1; h = bad.host(); CHECK(check(&h) != nullptr);
        bad = good; if (bad.rp[1][4]) { bad.col[1][0] = 6; h = bad.host(); CHECK(check(&h) != nullptr); }
    }
    printf("%zu systems\nok\n", runs);
    return 0;
}
