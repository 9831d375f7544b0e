// host_verify.cpp -- a compiled-language VERIFIER above the C ABI, written against include/zkmpc_hip.h only: it has no proving key and
// no constraint system, only what a verifier receives.  It loads two verifying keys from the bytes VerifyingKey::serialize writes
// (arkworks/groth16/src/data_structures.rs:43-58), reads a batch whose proofs belong to either key, and asks for ONE verdict over
// both keys (zk_groth16_vkeys_verify_aggregate, seeded) and for the verdict of every proof.
//
//   host_verify KEY0 KEY1 BATCH [SEED_HEX]
// KEY0, KEY1: files of VerifyingKey::serialize bytes (compressed).  BATCH: u64 count, then per proof u32 key (0 or 1), u32 n, n public
// inputs as Fr::serialize writes them (32 bytes, little-endian, canonical) and the 192 bytes of Proof::serialize; all little-endian.
// SEED_HEX: 64 hex digits drawn AFTER the proofs arrived (default: 00 01 .. 1f, for a reproducible run).
// Prints "ok_all <0|1>" and "ok_each <0|1> ..." in the batch's order (tests/test_gpu_host_verify.py holds them to the Python API).
//
// Build (examples/Makefile does exactly this):
//   g++ -std=c++17 -I include examples/host_verify.cpp -L zk-mpc_amd/lib -lzkmpc_hip -Wl,-rpath,$PWD/zk-mpc_amd/lib
//       -Wl,--allow-shlib-undefined -o /tmp/host_verify
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "zkmpc_hip.h"

static zk_ctx* CTX = nullptr;
#define CK(expr)                                                                                        \
    do {                                                                                                \
        int rc_ = (expr);                                                                               \
        if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #expr, rc_, CTX ? zk_last_error(CTX) : "(no context: no GPU?)");  \
                        return 1; }                                                                     \
    } while (0)

static bool read_file(const char* path, std::vector<uint8_t>* out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out->insert(out->end(), buf, buf + n);
    fclose(f);
    return true;
}

template <class T>
static bool take(const std::vector<uint8_t>& b, size_t* at, T* v) {      // a little-endian integer
    if (b.size() - *at < sizeof(T)) return false;
    *v = 0;
    for (size_t i = 0; i < sizeof(T); i++) *v |= (T)b[*at + i] << (8 * i);
    *at += sizeof(T);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: host_verify KEY0 KEY1 BATCH [SEED_HEX]\n"); return 2; }
    uint8_t seed[32];
    for (int i = 0; i < 32; i++) seed[i] = (uint8_t)i;
    if (argc > 4) {
        if (strlen(argv[4]) != 64) { fprintf(stderr, "SEED_HEX is 64 hex digits\n"); return 2; }
        for (int i = 0; i < 32; i++) {
            unsigned v;
            if (sscanf(argv[4] + 2 * i, "%2x", &v) != 1) { fprintf(stderr, "SEED_HEX is 64 hex digits\n"); return 2; }
            seed[i] = (uint8_t)v;
        }
    }
    std::vector<uint8_t> key_bytes[2], batch;
    if (!read_file(argv[1], &key_bytes[0]) || !read_file(argv[2], &key_bytes[1]) || !read_file(argv[3], &batch)) {
        fprintf(stderr, "cannot read the input files\n");
        return 2;
    }
    // the batch: key indices, the inputs concatenated in proof order, the proofs
    size_t at = 0;
    uint64_t count = 0;
    if (!take(batch, &at, &count) || count == 0 || count > (1u << 20)) { fprintf(stderr, "BATCH: bad count\n"); return 2; }
    std::vector<uint32_t> key_of(count);
    std::vector<zk_fr> inputs;
    std::vector<uint8_t> proofs(count * 192);
    for (uint64_t i = 0; i < count; i++) {
        uint32_t n = 0;
        if (!take(batch, &at, &key_of[i]) || !take(batch, &at, &n) || n > (1u << 20)) { fprintf(stderr, "BATCH: truncated\n"); return 2; }
        for (uint32_t j = 0; j < n; j++) {
            uint64_t c[4];
            for (int w = 0; w < 4; w++)
                if (!take(batch, &at, &c[w])) { fprintf(stderr, "BATCH: truncated\n"); return 2; }
            zk_fr x;
            if (zk_fr_from_canonical(c, &x) != 0) { fprintf(stderr, "BATCH: proof %llu input %u is not below r\n", (unsigned long long)i, j); return 2; }
            inputs.push_back(x);
        }
        if (batch.size() - at < 192) { fprintf(stderr, "BATCH: truncated\n"); return 2; }
        memcpy(&proofs[i * 192], &batch[at], 192);
        at += 192;
    }
    if (at != batch.size()) { fprintf(stderr, "BATCH: trailing bytes\n"); return 2; }

    CK(zk_ctx_create(0, 0, 1, &CTX));
    // VerifyingKey::deserialize with its subgroup test: a verifier does not trust the bytes
    zk_vkey* vkeys[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; k++) CK(zk_vkey_deserialize(CTX, key_bytes[k].data(), key_bytes[k].size(), 1, 1, &vkeys[k]));
    printf("keys %zu %zu inputs\n", zk_vkey_num_inputs(vkeys[0]), zk_vkey_num_inputs(vkeys[1]));
    int ok_all = 0;
    std::vector<int> ok_each(count, 0);
    CK(zk_groth16_vkeys_verify_aggregate(CTX, vkeys, 2, count, key_of.data(), inputs.empty() ? nullptr : inputs.data(), inputs.size(), proofs.data(), seed,
                                         &ok_all, ok_each.data()));
    printf("ok_all %d\nok_each", ok_all);
    for (uint64_t i = 0; i < count; i++) printf(" %d", ok_each[i]);
    printf("\n");
    for (int k = 0; k < 2; k++) CK(zk_vkey_free(CTX, vkeys[k]));
    CK(zk_ctx_destroy(CTX));
    return 0;
}
