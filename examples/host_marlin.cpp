// host_marlin.cpp -- a compiled-language host above the C ABI that goes from ConstraintMatrices and toxic waste to a Marlin proof and
// its verdict with no Python: the flow of the reference's Marlin test (arkworks/marlin/src/test.rs: universal_setup, index, prove,
// verify) written against include/zkmpc_hip.h only.  The circuit is the mul-chain w_i w_{i+1} = w_{i+2} with the last product
// public, given as to_matrices() would give it -- neither padded nor square.  Toxic waste and the prover's seed are fixed, so
// tests/test_gpu_host_marlin.py can name the bytes this program must print.
//
// Build and run (the test does exactly this):
//   g++ -std=c++17 -I include examples/host_marlin.cpp -L zk-mpc_amd/lib -lzkmpc_hip -Wl,-rpath,$PWD/zk-mpc_amd/lib
//       -Wl,--allow-shlib-undefined -o /tmp/host_marlin && /tmp/host_marlin [num_constraints]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "zkmpc_hip.h"

static zk_ctx* CTX = nullptr;
#define CK(expr)                                                                                        \
    do {                                                                                                \
        int rc_ = (expr);                                                                               \
        if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #expr, rc_, CTX ? zk_last_error(CTX) : "(no context: no GPU?)");  \
                        return 1; }                                                                     \
    } while (0)

static zk_fr fr(uint64_t v) {          // Fr::from(v): canonical integer -> Montgomery words (from_repr)
    uint64_t c[4] = {v, 0, 0, 0};
    zk_fr o;
    zk_fr_from_canonical(c, &o);
    return o;
}

int main(int argc, char** argv) {
    const size_t n = argc > 1 ? (size_t)atoll(argv[1]) : 100;
    if (n == 0) { fprintf(stderr, "num_constraints must be positive\n"); return 1; }
    CK(zk_ctx_create(0, 0, 1, &CTX));
    // variables: [1, pub] ++ [w_0 .. w_n]; constraint i: w_i * w_{i+1} = w_{i+2}, w_{n+1} being the public input
    auto var = [n](size_t j) -> uint32_t { return j <= n ? (uint32_t)(2 + j) : 1u; };
    std::vector<uint32_t> row_ptr(n + 1), col_a(n), col_b(n), col_c(n);
    std::vector<zk_fr> ones(n, fr(1));
    for (size_t i = 0; i <= n; i++) row_ptr[i] = (uint32_t)i;
    for (size_t i = 0; i < n; i++) { col_a[i] = var(i); col_b[i] = var(i + 1); col_c[i] = var(i + 2); }
    const zk_r1cs_host host{n, 2, n + 1, row_ptr.data(), col_a.data(), ones.data(), row_ptr.data(), col_b.data(), ones.data(),
                            row_ptr.data(), col_c.data(), ones.data()};
    zk_marlin_ix_info info;
    CK(zk_diag_marlin_shape_host(&host, 0, nullptr, nullptr, nullptr, 0, &info));      // the sizes: how long an SRS the index needs

    // KZG10::setup with explicit toxic waste (poly-commit/src/kzg10/mod.rs:44-135): powers_of_g[i] = beta^i g for i <= max_degree,
    // powers_of_gamma_g[i] = beta^i gamma_g for the three indices a hiding bound of 1 uses, h and beta h in G2
    const size_t max_degree = info.max_degree_needed + 3;
    const zk_fr beta = fr(0x5eed1234), g_k = fr(1), gamma_g_k = fr(7), h_k = fr(11), one = fr(1);
    void* pw = nullptr;
    CK(zk_dev_alloc(CTX, (max_degree + 1) * sizeof(zk_fr), &pw));
    CK(zk_fr_powers_dev(CTX, &beta, &one, max_degree + 1, pw));
    zk_bases *powers_g = nullptr, *powers_gamma_g = nullptr, *h_tab = nullptr;
    CK(zk_fixed_base_g1_dev(CTX, &g_k, pw, max_degree + 1, &powers_g));
    CK(zk_bases_precompute(CTX, powers_g));
    CK(zk_fixed_base_g1_dev(CTX, &gamma_g_k, pw, 3, &powers_gamma_g));
    CK(zk_fixed_base_g2_dev(CTX, &h_k, pw, 2, &h_tab));
    zk_g2_affine h2[2];                                                                // h, beta h
    CK(zk_bases_download_g2(CTX, h_tab, 0, 2, h2));

    // Marlin::index
    zk_marlin_ix* ix = nullptr;
    CK(zk_marlin_index_build(CTX, &host, powers_g, &ix));

    // the circuit's assignment (seeds 3, 5), then in the index's layout
    const zk_fr w0 = fr(3), w1 = fr(5);
    void *z = nullptr, *z_padded = nullptr;
    CK(zk_dev_alloc(CTX, (n + 3) * sizeof(zk_fr), &z));
    CK(zk_dev_alloc(CTX, (info.num_instance + info.num_witness) * sizeof(zk_fr), &z_padded));
    CK(zk_mul_chain_assignment_dev(CTX, n, &w0, &w1, z));
    CK(zk_marlin_pad_assignment_dev(CTX, ix, z, z_padded));

    // Marlin::prove
    uint8_t seed[32];
    for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(3 * i + 1);
    zk_rng* rng = nullptr;
    CK(zk_rng_from_seed(seed, 20, &rng));
    std::vector<uint8_t> proof(zk_marlin_proof_max_size());
    size_t proof_len = 0;
    CK(zk_marlin_prove(CTX, zk_marlin_ix_view(ix), powers_g, powers_gamma_g, z_padded, rng, 0, proof.data(), proof.size(), &proof_len));

    // Marlin::verify on the public input (the padded instance without its leading 1)
    zk_marlin_vk_host vk;
    CK(zk_marlin_vk_from_index(CTX, ix, powers_g, powers_gamma_g, &h2[0], &h2[1], &vk));
    std::vector<zk_fr> inputs(info.num_instance - 1);
    CK(zk_memcpy_d2h(CTX, inputs.data(), (const char*)z_padded + sizeof(zk_fr), inputs.size() * sizeof(zk_fr)));
    int ok = 0, ok_wrong = 1;
    CK(zk_marlin_verify_host(&vk, inputs.data(), inputs.size(), proof.data(), proof_len, &ok));
    std::vector<zk_fr> wrong = inputs;
    CK(zk_fr_add(&inputs[0], &one, &wrong[0]));
    CK(zk_marlin_verify_host(&vk, wrong.data(), wrong.size(), proof.data(), proof_len, &ok_wrong));

    printf("proof ");
    for (size_t i = 0; i < proof_len; i++) printf("%02x", proof[i]);
    printf("\nverdict %d\nverdict_wrong_input %d\n", ok, ok_wrong);

    CK(zk_rng_free(rng));
    CK(zk_marlin_ix_free(CTX, ix));
    CK(zk_bases_free(CTX, h_tab));
    CK(zk_bases_free(CTX, powers_gamma_g));
    CK(zk_bases_free(CTX, powers_g));
    CK(zk_dev_free(CTX, z_padded));
    CK(zk_dev_free(CTX, z));
    CK(zk_dev_free(CTX, pw));
    CK(zk_ctx_destroy(CTX));
    return ok == 1 && ok_wrong == 0 ? 0 : 1;
}
