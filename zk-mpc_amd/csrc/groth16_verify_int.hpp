// groth16_verify_int.hpp -- the steps of Groth16 verification that groth16_verify.hip defines and the batch forms of
// groth16_verify_keys.hip run for any number of keys: the checks of one key's inputs, the staging of the proofs and prepare_inputs.
// groth16_verify.hip documents each where it is defined.
#pragma once
#include "groth16_int.hpp"

namespace zkvfy {

bool inputs_below_r(const zk_fr* inputs, size_t n);
int inputs_ok(zk_ctx* ctx, const zk_vkey* vk, size_t count, const zk_fr* inputs_host, size_t ninp, const char* entry);
void coeff_words(const uint64_t* c, uint32_t k[8]);
bool host_proof_points(const uint8_t proof[192], bool check_subgroup, zk::Affine<zk::G1Field>* a, zk::Affine<zk::G2Field>* b, zk::Affine<zk::G1Field>* c);
int stage_proofs(zk_ctx* ctx, size_t count, const uint8_t* proofs_host, bool check_subgroup, uint32_t* bad_any, uint32_t* bad_ac, uint32_t* bad_b,
                 uint32_t** ac, uint32_t** b, std::vector<uint8_t>* staging, ZkPhaseTimer* tm = nullptr, ZkHostLap* lap = nullptr);
int prepare_inputs_dev(zk_ctx* ctx, const zk_vkey* vk, size_t count, const zk_fr* inputs_host, uint32_t* prep, uint32_t* inf);

}  // namespace zkvfy
