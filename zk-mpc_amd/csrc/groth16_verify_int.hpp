// groth16_verify_int.hpp -- the steps of Groth16 verification that groth16_verify.hip defines and groth16_verify_keys.hip (several
// keys in one call) runs as well: one copy of the checks, the staging, prepare_inputs and the single-key forms themselves, which the
// several-key forms ARE when a batch uses one key.  groth16_verify.hip documents each where it is defined.
#pragma once
#include "groth16_int.hpp"

namespace zkvfy {

bool inputs_below_r(const zk_fr* inputs, size_t n);
// s[0] = sum r_i, s[j + 1] = sum r_i x_{i,j} over the proofs [lo, hi) of one key (inputs: count x ninp)
void coeff_sums(const uint64_t* coeffs, const zk_fr* inputs, size_t ninp, size_t lo, size_t hi, zk::HF* s);
void coeff_words(const uint64_t* c, uint32_t k[8]);
bool host_proof_points(const uint8_t proof[192], bool check_subgroup, zk::Affine<zk::G1Field>* a, zk::Affine<zk::G2Field>* b, zk::Affine<zk::G1Field>* c);
int stage_proofs(zk_ctx* ctx, size_t count, const uint8_t* proofs_host, bool check_subgroup, uint32_t* bad_any, uint32_t* bad_ac, uint32_t* bad_b,
                 uint32_t** ac, uint32_t** b, std::vector<uint8_t>* staging, ZkPhaseTimer* tm = nullptr, ZkHostLap* lap = nullptr);
int prepare_inputs_dev(zk_ctx* ctx, const zk_vkey* vk, size_t count, const zk_fr* inputs_host, uint32_t* prep, uint32_t* inf);
int verify_batch(zk_ctx* ctx, const zk_vkey* vk, size_t count, const zk_fr* inputs_host, size_t ninp, const zk_g1_affine* prepared,
                 const uint8_t* proofs_host, int* ok, bool check_subgroup, const char* entry);
int aggregate_host(const zk_vk_host* vk, size_t count, const zk_fr* inputs, size_t ninp, const uint8_t* proofs, const uint64_t* coeffs, int* ok_all,
                   zk_gt* folded);
int aggregate_dev(zk_ctx* ctx, const zk_vkey* pk, size_t count, const zk_fr* inputs_host, size_t ninp, const uint8_t* proofs_host, const uint64_t* coeffs,
                  int* ok_all, zk_gt* folded, const char* entry);

}  // namespace zkvfy
