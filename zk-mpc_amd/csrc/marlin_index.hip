// marlin_index.hip -- Marlin::index as ONE entry point: from ConstraintMatrices and the SRS to the device-resident index the provers
// read (zk_marlin_index) and the IndexVerifierKey's bytes.
//
// Replaces (reference):
//   Marlin::index                                   arkworks/marlin/src/lib.rs:101-146
//   AHPForR1CS::index                               arkworks/marlin/src/ahp/indexer.rs:121-208
//   arithmetize_matrix, balance_matrices, padding   arkworks/marlin/src/ahp/constraint_systems.rs:23-264
// The integer shaping is host work (marlin_shape.hpp: one sequential walk and sorts of short rows); the field work is one kernel
// over the 3 |K| entries, batched transforms and one MSM job list.  zk-mpc_amd/marlin.py::Index / IndexKeys build the same index
// call by call from Python: the two are tested against each other word for word.
#include "../../include/zkmpc_hip.h"
#include "devutil.cuh"
#include "groth16_int.hpp"
#include "internal.hpp"
#include "marlin_bytes.hpp"
#include "marlin_shape.hpp"
#include <chrono>

using namespace zk;

struct zk_marlin_ix {
    zk_marlin_ix_info info{};
    zk_marlin_index view{};
    zk_r1cs *r1cs = nullptr, *r1cs_t = nullptr;
    char* polys = nullptr;          // 12 |K| coefficients: a_row a_col a_val a_row_col b_... c_...
    char* on_k = nullptr;           // 9 |K|: row, col, val of A*, B*, C* on K
    char* on_b = nullptr;           // 12 |B|: the twelve polynomials on B
    uint32_t* idx = nullptr;        // w_idx | x_idx, |H| words each
    std::vector<uint8_t> ivk;       // IndexVerifierKey::write
};

namespace {

uint32_t log2_of(size_t pow2) {
    uint32_t lg = 0;
    while (((size_t)1 << lg) < pow2) lg++;
    return lg;
}

// One matrix as the kernel reads it: entry i < nnz sits in row row[i], column col[i] (the zk_r1cs's own arrays: rows sorted by
// column) with coefficient coeff[i] in internal form, or 1 where coeff is NULL.
struct ArithMat { const uint32_t* row; const uint32_t* col; const uint32_t* coeff; uint32_t nnz; };
struct ArithArgs { ArithMat m[3]; };

// arithmetize_matrix (constraint_systems.rs:152-264) for A, B, C at once, one entry per thread over 3 |K|: the matrix is transposed
// (row <- the column's element of H, col <- the row's), val = coeff / u_H(row, row) with u_H(x, x) = |H| x^-1 (mod.rs:362-369),
// i.e. coeff * row / |H|.  Entries past a matrix's last: row = col = 1 (elems[0]), val = 0.  elems: w^i, internal form; every
// result leaves in the reference's form, fully reduced (the exact domain of fp29.cuh).  The evaluations on K go out twice: to on_k,
// which the prover's third round reads, and to polys, which the inverse transforms turn into coefficients in place.
__global__ void __launch_bounds__(256)
k_marlin_arith(ArithArgs a, const uint32_t* elems, FrK n_inv_ext, uint32_t log_k, uint32_t log_period, uint32_t x_size, void* on_k, void* polys) {
    const size_t K = (size_t)1 << log_k, total = 3 * K;
    const Fr to_ext = fp_const<FrParams>(FrParams::INT_TO_EXT);
    const Fr one_ext = fr_mul(fp_one<FrParams>(), to_ext);
    const Fr n_inv = frk(n_inv_ext);
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const uint32_t m = (uint32_t)(t >> log_k);
        const size_t i = t & (K - 1);
        const ArithMat mat = m == 0 ? a.m[0] : m == 1 ? a.m[1] : a.m[2];
        Fr row = one_ext, col = one_ext, val = fp_zero<FrParams>(), row_col = one_ext;
        if (i < mat.nnz) {
            // EvaluationDomain::reindex_by_subdomain: the sub-domain X first, then the rest of H in order
            const uint32_t c = mat.col[i];
            uint32_t at = c << log_period;
            if (c >= x_size) {
                const uint32_t j = c - x_size;
                at = j + j / ((1u << log_period) - 1) + 1;
            }
            const Fr w_col = tab_load(elems, at), w_row = tab_load(elems, mat.row[i]);
            row = fr_mul(w_col, to_ext);
            col = fr_mul(w_row, to_ext);
            val = fr_mul(w_col, n_inv);                                      // int * ext = ext
            if (mat.coeff) val = fr_mul(fr_load(mat.coeff, i), val);         // (the stored words are the internal form)
            row_col = fr_mul(row, w_row);
        }
        fr_store(on_k, (3 * m + 0) * K + i, row);
        fr_store(on_k, (3 * m + 1) * K + i, col);
        fr_store(on_k, (3 * m + 2) * K + i, val);
        fr_store(polys, (4 * m + 0) * K + i, row);
        fr_store(polys, (4 * m + 1) * K + i, col);
        fr_store(polys, (4 * m + 2) * K + i, val);
        fr_store(polys, (4 * m + 3) * K + i, row_col);
    }
}

// out: count vectors of 2^log_b elements = the count vectors of 2^log_k coefficients of `in`, each followed by zeros
__global__ void __launch_bounds__(256) k_marlin_spread(const void* in, uint32_t log_k, uint32_t log_b, size_t count, void* out) {
    const uint4* src = reinterpret_cast<const uint4*>(in);
    uint4* dst = reinterpret_cast<uint4*>(out);
    const size_t total = count << (log_b + 1), mask = ((size_t)2 << log_b) - 1;        // in 16-byte halves of an element
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t v = t >> (log_b + 1), h = t & mask;
        dst[t] = h < ((size_t)2 << log_k) ? src[(v << (log_k + 1)) + h] : make_uint4(0, 0, 0, 0);
    }
}

// instance | zeros up to the power of two | witness | ones up to square (pad_input_for_indexer_and_prover and
// make_matrices_square_for_prover, constraint_systems.rs:74-88,115-124)
__global__ void __launch_bounds__(256) k_marlin_pad_z(const void* z, size_t ni_in, size_t nw_in, size_t ni, size_t n, void* out) {
    const Fr one_ext = fr_mul(fp_one<FrParams>(), fp_const<FrParams>(FrParams::INT_TO_EXT));
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        Fr v = fp_zero<FrParams>();
        if (i < ni_in) v = fr_load(z, i);
        else if (i >= ni) v = i - ni < nw_in ? fr_load(z, ni_in + (i - ni)) : one_ext;
        fr_store(out, i, v);
    }
}

void release(zk_ctx* ctx, zk_marlin_ix* ix) {
    if (!ix) return;
    if (ix->r1cs) (void)zk_r1cs_free(ctx, ix->r1cs);
    if (ix->r1cs_t) (void)zk_r1cs_free(ctx, ix->r1cs_t);
    (void)hipStreamSynchronize(ctx->stream);
    for (void* p : {(void*)ix->polys, (void*)ix->on_k, (void*)ix->on_b, (void*)ix->idx})
        if (p) (void)hipFree(p);
    delete ix;
}

struct DevTmp {                     // a device buffer that lives for one call
    void* p = nullptr;
    ~DevTmp() { if (p) (void)hipFree(p); }
};

int upload_r1cs(zk_ctx* ctx, const zk_marlin::Csr* m, size_t rows, size_t ni, size_t nw, zk_r1cs** out) {
    zk_r1cs_host h{};
    h.num_constraints = rows; h.num_instance = ni; h.num_witness = nw;
    h.a_row_ptr = m[0].row_ptr.data(); h.a_col = m[0].col.data(); h.a_coeff = m[0].coeff.data();
    h.b_row_ptr = m[1].row_ptr.data(); h.b_col = m[1].col.data(); h.b_coeff = m[1].coeff.data();
    h.c_row_ptr = m[2].row_ptr.data(); h.c_col = m[2].col.data(); h.c_coeff = m[2].coeff.data();
    return zk_r1cs_upload(ctx, &h, out);
}

// count transforms of 2^log_n elements, back to back at base: all at once where a transform is one pass, four at a time through tmp
// (room for four) where it takes several
int transforms(zk_ctx* ctx, char* base, size_t count, uint32_t log_n, int inverse, void* tmp) {
    const size_t n = (size_t)1 << log_n, per = tmp ? 4 : count;
    for (size_t k = 0; k < count; k += per)
        ZK_TRY(zk_ntt_launch_strided(ctx, base + k * n * 32, std::min(per, count - k), n, log_n, inverse, 0, tmp));
    return ZK_OK;
}

int build(zk_ctx* ctx, const zk_r1cs_host* m, const zk_bases* powers_g, zk_marlin_ix* ix) {
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {      // with zk_set_profiling: host wall-clock of a phase, the device's work included
        if (!ctx->profiling) return;
        (void)hipStreamSynchronize(ctx->stream);
        const auto now = std::chrono::steady_clock::now();
        auto& tm = ctx->timers[std::string("marlin_index.") + what];
        tm.ms += (float)std::chrono::duration<double, std::milli>(now - t0).count();
        tm.count += 1;
        t0 = now;
    };
    zk_marlin::Shape sh;
    zk_marlin::shape(m, &sh);
    const zk_marlin_ix_info& s = ix->info = sh.info;
    const size_t H = s.h_size, K = s.k_size, B = s.b_size;
    const uint32_t log_h = log2_of(H), log_k = log2_of(K), log_b = log2_of(B);
    for (int k = 0; k < 3; k++)
        if (sh.m[k].nnz() > K) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_marlin_index_build: a balanced matrix has more than |K| entries");
    lap("shape");

    // the matrices for z_A, z_B (prover.rs:258-278) and their transposes for calculate_t (:406-423); the kernel below reads the
    // first's columns and coefficients where they are
    ZK_TRY(upload_r1cs(ctx, sh.m, s.num_constraints, s.num_instance, s.num_witness, &ix->r1cs));
    ZK_TRY(upload_r1cs(ctx, sh.t, H, 1, H - 1, &ix->r1cs_t));
    size_t entries = 0;
    for (int k = 0; k < 3; k++) entries += sh.m[k].nnz();
    std::vector<uint32_t> row_of(std::max<size_t>(entries, 1));
    std::vector<uint32_t> wx(2 * H);                                        // Index.w_evals_index: prover.rs:343-353
    {
        size_t at = 0;
        for (int k = 0; k < 3; k++)
            for (size_t r = 0; r < sh.m[k].rows(); r++)
                for (uint32_t e = sh.m[k].row_ptr[r]; e < sh.m[k].row_ptr[r + 1]; e++) row_of[at++] = (uint32_t)r;
        const size_t ratio = H / s.x_size;
        for (size_t k = 0; k < H; k++) {
            const bool on_x = k % ratio == 0;
            const size_t wi = k - k / ratio - 1;                            // (unused where on_x)
            wx[k] = on_x || wi >= s.num_witness ? 0xFFFFFFFFu : (uint32_t)(wi + s.num_instance);
            wx[H + k] = on_x ? 0xFFFFFFFFu : (uint32_t)k;
        }
    }
    DevTmp rows, tmp;
    ZK_HIP(ctx, hipMalloc(&rows.p, row_of.size() * 4));
    ZK_HIP(ctx, hipMalloc((void**)&ix->idx, 2 * H * 4));
    ZK_HIP(ctx, hipMalloc((void**)&ix->polys, 12 * K * 32));
    ZK_HIP(ctx, hipMalloc((void**)&ix->on_k, 9 * K * 32));
    ZK_HIP(ctx, hipMalloc((void**)&ix->on_b, 12 * B * 32));
    if (log_b > 10) ZK_HIP(ctx, hipMalloc(&tmp.p, 4 * B * 32));             // (a transform of more than 2^10 elements takes several passes)
    ZK_HIP(ctx, hipMemcpy(rows.p, row_of.data(), row_of.size() * 4, hipMemcpyHostToDevice));
    ZK_HIP(ctx, hipMemcpy(ix->idx, wx.data(), wx.size() * 4, hipMemcpyHostToDevice));
    lap("upload");

    const uint32_t* elems;
    Fr n_inv;
    ZK_TRY(zk_ntt_domain_elements(ctx, log_h, &elems, &n_inv));
    ArithArgs args{};
    {
        const uint32_t* r = (const uint32_t*)rows.p;
        for (int k = 0; k < 3; k++) {
            const auto& dm = ix->r1cs->m[k];
            args.m[k] = ArithMat{r, dm.col, dm.all_one ? nullptr : dm.coeff, (uint32_t)dm.nnz};
            r += dm.nnz;
        }
    }
    hipLaunchKernelGGL(k_marlin_arith, zk_grid(3 * K, 256), 256, 0, ctx->stream, args, elems, to_frk(fp_int_to_ext<FrParams>(n_inv)), log_k,
                       log_h - log2_of(s.x_size), (uint32_t)s.x_size, (void*)ix->on_k, (void*)ix->polys);
    ZK_HIP(ctx, hipGetLastError());
    lap("arith");

    ZK_TRY(transforms(ctx, ix->polys, 12, log_k, 1, log_k > 10 ? tmp.p : nullptr));
    hipLaunchKernelGGL(k_marlin_spread, zk_grid(24 * B, 256), 256, 0, ctx->stream, (const void*)ix->polys, log_k, log_b, (size_t)12, (void*)ix->on_b);
    ZK_HIP(ctx, hipGetLastError());
    ZK_TRY(transforms(ctx, ix->on_b, 12, log_b, 0, tmp.p));
    lap("transforms");

    // PC::commit without hiding or degree bounds (lib.rs:124-131): twelve MSMs over powers_g as one job list
    const zk_bases* tables[12];
    const void* scalars[12];
    size_t lens[12];
    zk_g1_projective sums[12];
    void* outs[12];
    for (int j = 0; j < 12; j++) { tables[j] = powers_g; scalars[j] = ix->polys + (size_t)j * K * 32; lens[j] = K; outs[j] = &sums[j]; }
    ZK_TRY(zk_msm_batch_dev(ctx, 12, tables, nullptr, scalars, lens, outs));
    const std::vector<Affine<G1Field>> aff = batch_to_aff(std::vector<zk_g1_projective>(sums, sums + 12));
    // IndexVerifierKey::write: index_info (num_variables, num_constraints, num_non_zero: indexer.rs:44-50) | index_comms
    for (const size_t v : {s.num_constraints, s.num_constraints, s.num_non_zero})
        for (int b = 0; b < 8; b++) ix->ivk.push_back((uint8_t)((uint64_t)v >> (8 * b)));
    for (int j = 0; j < 12; j++) comm_tobytes(Comm{aff[j], aff_inf<G1Field>(), false}, ix->ivk);
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));      // (rows and tmp go with this frame)
    lap("commit");

    zk_marlin_index& v = ix->view;
    v.num_constraints = v.num_variables = s.num_constraints;
    v.num_non_zero = s.num_non_zero;
    v.num_instance = s.num_instance;
    v.r1cs = ix->r1cs;
    v.r1cs_t = ix->r1cs_t;
    for (int j = 0; j < 12; j++) v.index_polys[j] = zk_poly_ref{ix->polys + (size_t)j * K * 32, K};
    for (int k = 0; k < 3; k++) {
        const char *ek = ix->on_k + (size_t)3 * k * K * 32, *eb = ix->on_b + (size_t)4 * k * B * 32;
        v.on_k[k] = zk_marlin_matrix_evals{ek, ek + K * 32, ek + 2 * K * 32, nullptr};
        v.on_b[k] = zk_marlin_matrix_evals{eb, eb + B * 32, eb + 2 * B * 32, eb + 3 * B * 32};
    }
    v.w_idx = ix->idx;
    v.x_idx = ix->idx + H;
    v.ivk_bytes = ix->ivk.data();
    v.ivk_len = ix->ivk.size();
    return ZK_OK;
}

}  // namespace

extern "C" int zk_marlin_index_build(zk_ctx* ctx, const zk_r1cs_host* m, const zk_bases* powers_g, zk_marlin_ix** out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !m || !powers_g || !out) return ZK_ERR_ARG;
    if (const char* bad = zk_marlin::check(m)) ZK_FAIL(ctx, ZK_ERR_ARG, std::string("zk_marlin_index_build: ") + bad);
    const zk_marlin_ix_info s = zk_marlin::sizes(m);
    if (powers_g->group != 1 || powers_g->n < s.max_degree_needed + 1)
        ZK_FAIL(ctx, ZK_ERR_ARG, "zk_marlin_index_build: IndexTooLarge: powers_g is not a G1 table of max_degree_needed + 1 = " +
                                     std::to_string(s.max_degree_needed + 1) + " points or more");
    if (s.b_size > ((size_t)1 << 28)) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_marlin_index_build: the domain of size 3 |K| - 3 is beyond the transforms (2^28)");
    zk_marlin_ix* ix = new zk_marlin_ix();
    int rc;
    try {
        rc = build(ctx, m, powers_g, ix);
    } catch (...) {
        release(ctx, ix);
        throw;
    }
    if (rc != ZK_OK) {
        const std::string why = ctx->last_error;         // (the release's own calls must not replace the reason)
        release(ctx, ix);
        ctx->last_error = why;
        return rc;
    }
    *out = ix;
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_marlin_ix_free(zk_ctx* ctx, zk_marlin_ix* ix) {
    ZK_API_BEGIN(ctx)
    if (!ctx) return ZK_ERR_ARG;
    release(ctx, ix);
    return ZK_OK;
    ZK_API_END
}

extern "C" const zk_marlin_index* zk_marlin_ix_view(const zk_marlin_ix* ix) { return ix ? &ix->view : nullptr; }

extern "C" int zk_marlin_ix_info_get(const zk_marlin_ix* ix, zk_marlin_ix_info* out) {
    ZK_API_BEGIN_NOCTX
    if (!ix || !out) return ZK_ERR_ARG;
    *out = ix->info;
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_marlin_pad_assignment_dev(zk_ctx* ctx, const zk_marlin_ix* ix, const void* z_dev, void* z_padded_dev) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !ix || !z_dev || !z_padded_dev) return ZK_ERR_ARG;
    const zk_marlin_ix_info& s = ix->info;
    const size_t n = s.num_instance + s.num_witness;
    hipLaunchKernelGGL(k_marlin_pad_z, zk_grid(n, 256), 256, 0, ctx->stream, z_dev, s.num_instance_in, s.num_witness_in, s.num_instance, n, z_padded_dev);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_marlin_vk_from_index(zk_ctx* ctx, const zk_marlin_ix* ix, const zk_bases* powers_g, const zk_bases* powers_gamma_g,
                                       const zk_g2_affine* h, const zk_g2_affine* beta_h, zk_marlin_vk_host* out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !ix || !powers_g || !powers_gamma_g || !h || !beta_h || !out) return ZK_ERR_ARG;
    const zk_marlin_ix_info& s = ix->info;
    if (powers_g->group != 1 || powers_gamma_g->group != 1 || powers_gamma_g->n == 0 || powers_g->n < s.max_degree_needed + 1)
        ZK_FAIL(ctx, ZK_ERR_ARG, "zk_marlin_vk_from_index: the SRS tables do not cover this index");
    // degree_bounds_and_shift_powers (marlin_pc/mod.rs:112-141): bound d has the shift power powers_of_g[max_degree - d]
    const size_t max_degree = powers_g->n - 1;
    ZK_TRY(zk_bases_download_g1(ctx, powers_g, 0, 1, &out->g));
    ZK_TRY(zk_bases_download_g1(ctx, powers_gamma_g, 0, 1, &out->gamma_g));
    ZK_TRY(zk_bases_download_g1(ctx, powers_g, max_degree - (s.h_size - 2), 1, &out->shift_h));
    ZK_TRY(zk_bases_download_g1(ctx, powers_g, max_degree - (s.k_size - 2), 1, &out->shift_k));
    out->h = *h;
    out->beta_h = *beta_h;
    out->ivk_bytes = ix->ivk.data();
    out->ivk_len = ix->ivk.size();
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_diag_marlin_shape_host(const zk_r1cs_host* m, int which, uint32_t* row_ptr, uint32_t* col, zk_fr* coeff, size_t cap,
                                         zk_marlin_ix_info* info) {
    ZK_API_BEGIN_NOCTX
    if (!m || which < 0 || which > 5 || zk_marlin::check(m)) return ZK_ERR_ARG;
    if (info) *info = zk_marlin::sizes(m);
    if (!row_ptr) return ZK_OK;
    zk_marlin::Shape sh;
    zk_marlin::shape(m, &sh);
    const zk_marlin::Csr& c = which < 3 ? sh.m[which] : sh.t[which - 3];
    if (c.nnz() > cap || (c.nnz() && (!col || !coeff))) return ZK_ERR_ARG;
    std::copy(c.row_ptr.begin(), c.row_ptr.end(), row_ptr);
    std::copy(c.col.begin(), c.col.end(), col);
    std::copy(c.coeff.begin(), c.coeff.end(), coeff);
    return ZK_OK;
    ZK_API_END
}
