// Marlin's Fiat-Shamir transcript (zk-mpc_amd/csrc/marlin_transcript.hpp) on cases that tests/test_marlin_transcript_host.py wrote: a
// stand-alone driver that includes the header alone, in a build a sanitizer can watch.  Reads the case file named on the command
// line, one case per line, tokens separated by blanks, every number in hex (a field element as its plain integer below the modulus):
//   |H|  ivk bytes  n  the n public inputs (without the leading 1)
//   nine commitments in the rounds' order (4, 3, 2), each as  POINT SHIFTED  with POINT = x:y or "inf" and SHIFTED = POINT or "-"
//   (no shifted commitment)  the seven evaluations
// and prints per case what the header derives: alpha eta_a eta_b eta_c beta gamma xi.
#include "marlin_transcript.hpp"
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

using namespace zk;

static int line_no = 0;
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) { printf("case %d: %s\n", line_no, #cond); exit(1); }                       \
    } while (0)

static std::vector<uint8_t> bytes_of(const std::string& hex) {                // two digits per byte, in order
    CHECK(hex.size() % 2 == 0);
    std::vector<uint8_t> out;
    for (size_t i = 0; i < hex.size(); i += 2) out.push_back((uint8_t)std::stoul(hex.substr(i, 2), nullptr, 16));
    return out;
}
template <int WORDS>
static void number(const std::string& hex, uint32_t w[WORDS]) {              // most significant digit first
    CHECK(!hex.empty() && hex.size() <= 8 * WORDS);
    for (int i = 0; i < WORDS; i++) w[i] = 0;
    for (size_t i = 0; i < hex.size(); i++) {
        const char c = hex[hex.size() - 1 - i];
        const uint32_t d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : 99;
        CHECK(d < 16);
        w[i / 8] |= d << (4 * (i % 8));
    }
}
static HF fr(const std::string& hex) { uint32_t w[8]; number<8>(hex, w); return HF::from_canon_words(w); }
static Fq fq(const std::string& hex) { uint32_t w[12]; number<12>(hex, w); return fp_canon_to_int<FqParams>(fp_unpack<FqParams>(w)); }
static Affine<G1Field> point(const std::string& t) {
    if (t == "inf") return aff_inf<G1Field>();
    const size_t colon = t.find(':');
    CHECK(colon != std::string::npos);
    return Affine<G1Field>{fq(t.substr(0, colon)), fq(t.substr(colon + 1))};
}
static void print(const HF& a, const char* end) {
    uint32_t w[8];
    a.canon_words(w);
    char buf[65];
    for (int i = 0; i < 8; i++) snprintf(buf + 8 * i, 9, "%08x", w[7 - i]);
    const char* p = buf;
    while (*p == '0' && p[1]) p++;
    printf("%s%s", p, end);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    if (!f) return 2;
    std::string line;
    while (std::getline(f, line)) {
        line_no++;
        std::istringstream in(line);
        std::string t;
        size_t h = 0, n = 0;
        CHECK(in >> std::hex >> h >> t >> n);
        const std::vector<uint8_t> ivk = bytes_of(t);
        std::vector<HF> pub(1, HF::one());
        for (size_t i = 0; i < n; i++) { CHECK(in >> t); pub.push_back(fr(t)); }
        Comm comms[9];
        for (Comm& c : comms) {
            std::string s;
            CHECK(in >> t >> s);
            c.c = point(t);
            c.has_shift = s != "-";
            c.s = c.has_shift ? point(s) : aff_inf<G1Field>();
        }
        std::vector<HF> ev;
        for (int i = 0; i < 7; i++) { CHECK(in >> t); ev.push_back(fr(t)); }
        CHECK(!(in >> t));
        const Dom H(h);
        marlin::Transcript fs(ivk.data(), ivk.size(), pub);
        const marlin::Transcript::Round1 r1 = fs.round1(&comms[0], 4, H);
        print(r1.alpha, " ");
        for (const HF& e : r1.eta) print(e, " ");
        print(fs.round2(&comms[4], 3, H), " ");
        print(fs.round3(&comms[7], 2), " ");
        print(fs.evaluations(ev), "\n");
    }
    return line_no ? 0 : 2;
}
