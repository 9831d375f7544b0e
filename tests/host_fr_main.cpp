// Fr on the host (zk-mpc_amd/csrc/hostfr.hpp) against cases that tests/test_host_fr.py computed with the oracle: a stand-alone driver
// that includes the header alone, in a build a sanitizer can watch.  Reads the case file named on the command line, one case per
// line, every number in hex and every field element as its plain integer below r; prints "ok <cases>" and returns 0, or names the
// first case that failed.
//   u64 X W            from_u64(X) is W
//   pow B E W          B.pow(E) is W
//   root LOG G         w = domain_root(LOG): w^(2^LOG) = 1, w^(2^(LOG-1)) = r - 1 for LOG >= 1, w is G unless G is "-"
//   binv N x.. y..     batch_inverse over the N values x leaves the N values y
//   limbs X l0 .. l8   X in internal form is those nine limbs, and back
//   abi X M            from_abi of the 256-bit word string M is X, and back
#include "hostfr.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace zk;

static int line_no = 0;
static char op[16];
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) { printf("case %d (%s): %s\n", line_no, op, #cond); exit(1); }                  \
    } while (0)

struct Words { uint64_t w[4]; };
static bool operator==(const Words& a, const Words& b) { return memcmp(a.w, b.w, sizeof a.w) == 0; }

static bool token(FILE* f, char* buf, size_t cap) {
    char fmt[16];
    snprintf(fmt, sizeof fmt, "%%%zus", cap - 1);
    return fscanf(f, fmt, buf) == 1;
}
static Words parse(const char* buf) {                               // up to 64 hex digits, most significant first
    const size_t n = strlen(buf);
    CHECK(n >= 1 && n <= 64);
    Words r{};
    for (size_t i = 0; i < n; i++) {
        const char c = buf[n - 1 - i];
        const uint64_t d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : 99;
        CHECK(d < 16);
        r.w[i / 16] |= d << (4 * (i % 16));
    }
    return r;
}
static Words words(FILE* f) {
    char buf[80];
    CHECK(token(f, buf, sizeof buf));
    return parse(buf);
}
static uint64_t u64(FILE* f) {
    const Words r = words(f);
    CHECK(!r.w[1] && !r.w[2] && !r.w[3]);
    return r.w[0];
}
static HF of_plain(const Words& c) { return HF{fp_canon_to_int<FrParams>(host_load_ext<FrParams>(c.w))}; }
static Words plain(const HF& a) {
    uint32_t w[8];
    a.canon_words(w);
    Words r;
    for (int i = 0; i < 4; i++) r.w[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
    return r;
}

int main(int argc, char** argv) {
    if (argc != 2) { printf("usage: host_fr <case file>\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    while (token(f, op, sizeof op)) {
        line_no++;
        if (!strcmp(op, "u64")) {
            const uint64_t x = u64(f);
            CHECK(plain(HF::from_u64(x)) == words(f));
        } else if (!strcmp(op, "pow")) {
            const HF b = of_plain(words(f));
            const uint64_t e = u64(f);
            CHECK(plain(b.pow(e)) == words(f));
        } else if (!strcmp(op, "root")) {
            const uint32_t log = (uint32_t)u64(f);
            char g[80];
            CHECK(token(f, g, sizeof g));
            const HF w = HF::domain_root(log);
            CHECK(w.pow((uint64_t)1 << log) == HF::one());
            if (log >= 1) CHECK(w.pow((uint64_t)1 << (log - 1)) == HF::one().neg());
            if (strcmp(g, "-")) CHECK(plain(w) == parse(g));
        } else if (!strcmp(op, "binv")) {
            const size_t n = (size_t)u64(f);
            std::vector<HF> v(n);
            for (auto& x : v) x = of_plain(words(f));
            HF::batch_inverse(v.data(), n);
            for (auto& x : v) CHECK(plain(x) == words(f));
        } else if (!strcmp(op, "limbs")) {
            const HF x = of_plain(words(f));
            uint32_t got[9], want[9];
            x.limbs(got);
            for (auto& l : want) l = (uint32_t)u64(f);
            CHECK(memcmp(got, want, sizeof got) == 0);
            CHECK(HF::from_limbs(want) == x);
        } else if (!strcmp(op, "abi")) {
            const Words x = words(f), m = words(f);
            zk_fr a;
            memcpy(a.l, m.w, sizeof a.l);
            CHECK(plain(HF::from_abi(a)) == x);
            const zk_fr back = of_plain(x).abi();
            CHECK(memcmp(back.l, m.w, sizeof back.l) == 0);
        } else {
            CHECK(!"a known case kind");
        }
    }
    fclose(f);
    printf("ok %d\n", line_no);
    return 0;
}
