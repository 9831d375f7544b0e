// marlin_bytes.hpp -- a marlin_pc commitment as the reference writes it: what the transcript absorbs (marlin_transcript.hpp, for the
// provers and the verifier) and what the indexer writes into the IndexVerifierKey's bytes (marlin_index.hip).
//   GroupAffine::write            ec/src/models/short_weierstrass_jacobian.rs:315-322
//   marlin_pc::Commitment::write  poly-commit/src/marlin/marlin_pc/data_structures.rs:252-263
#pragma once
#include "../../include/zkmpc_hip.h"
#include "hostfield64.hpp"
#include "hostgroup.hpp"
#include <vector>

namespace zk {

struct Comm { Affine<G1Field> c, s; bool has_shift = false; };

inline void g1_tobytes(const Affine<G1Field>& a, std::vector<uint8_t>& out) {     // GroupAffine::write: x | y | infinity; zero() = (0, 1, true)
    uint8_t b[48];
    if (aff_is_inf<G1Field>(a)) {
        out.insert(out.end(), 48, 0);
        out.push_back(1); out.insert(out.end(), 47, 0);
        out.push_back(1);
        return;
    }
    fq_canonical_bytes(a.x, b); out.insert(out.end(), b, b + 48);
    fq_canonical_bytes(a.y, b); out.insert(out.end(), b, b + 48);
    out.push_back(0);
}
inline void comm_tobytes(const Comm& c, std::vector<uint8_t>& out) {              // marlin_pc::Commitment::write
    g1_tobytes(c.c, out);
    out.push_back(c.has_shift ? 1 : 0);
    g1_tobytes(c.has_shift ? c.s : aff_inf<G1Field>(), out);
}
// projective -> affine for several points with ONE field inversion (the commitments of a round: 2 - 6 points) in the 64-bit host field
inline std::vector<Affine<G1Field>> batch_to_aff(const std::vector<zk_g1_projective>& pts) {
    using H = Fq64Field;
    std::vector<XYZZ<H>> x(pts.size());
    for (size_t i = 0; i < pts.size(); i++) x[i] = host64_proj_from_abi<H>((const uint64_t*)&pts[i]);
    std::vector<Affine<G1Field>> out;
    for (const Affine<H>& a : host64_batch_to_affine<H>(x)) out.push_back(aff_from_host64<G1Field>(a));
    return out;
}

}  // namespace zk
