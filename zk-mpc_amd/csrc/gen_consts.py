#!/usr/bin/env python3
"""Generate consts.cuh: radix-2^29 limb constants for the BLS12-377 fields used by the HIP kernels.

Primary inputs are the two moduli and the generator coordinates exactly as published in the
reference (arkworks/curves/bls12_377/src/fields/{fr,fq}.rs, curves/{g1,g2}.rs); everything
else is derived here with Python integers.

Representation (see fp29.cuh): an element is L limbs of 29 bits; the Montgomery radix of the
device arithmetic is RI = 2^(29*L) ("internal" form x*RI).  The reference keeps elements as
W 32-bit words in Montgomery form with RE = 2^(32*W) ("external" form x*RE).  RAW constants
below are plain integers k (no Montgomery factor), to be used as the second operand of
mmul(a, k) = a*k/RI.

Run: python3 gen_consts.py > consts.cuh
"""

R_MOD = 8444461749428370424248824938781546531375899335154063827935233455917409239041
Q_MOD = 258664426012969094010652733694893533536393512754914660539884262666720468348340822774968888139573360124440321458177
G1X = 81937999373150964239938255573465948239988671502647976594219695644855304257327692006745978603320413799295628339695
G1Y = 241266749859715473739788878240585681733927191168601896383759122102112907357779751001206799952863815012735208165030
G2X0 = 233578398248691099356572568220835526895379068987715365179118596935057653620464273615301663571204657964920925606294
G2X1 = 140913150380207355837477652521042157274541796891053068589147167627541651775299824604154852141315666357241556069118
G2Y0 = 63160294768292073209381361943935198908131692476676907196754037919244929611450776219210369229519898517858833747423
G2Y1 = 149157405641012693445398062341192467754805999074082136895788947234480009303640899064710353187729182149407503257491
# MNT4-753 base field (the SHE ciphertext modulus, src/she.rs:17-18): arkworks/curves/mnt4_753/src/fields/fq.rs:51 (MODULUS),
# :105 (GENERATOR = 17), :14 (TWO_ADICITY = 15); TWO_ADIC_ROOT_OF_UNITY (:16) = 17^T is derived below.
Q753_MOD = 41898490967918953402344214791240637128170709919953949071783502921025352812571106773058893763790338921418070971888253786114353726529584385201591605722013126468931404347949840543007986327743462853720628051692141265303114721689601
Q753_GENERATOR = 17
Q753_TWO_ADICITY = 15
FQ_TWO_ADICITY = 46          # fields/fq.rs:28
FQ_QNR = 15                  # a quadratic non-residue of Fq (checked below); any one gives a valid 2^46-th root of unity
assert pow(FQ_QNR, (Q_MOD - 1) // 2, Q_MOD) == Q_MOD - 1 and (Q_MOD - 1) % (1 << FQ_TWO_ADICITY) == 0 and ((Q_MOD - 1) >> FQ_TWO_ADICITY) % 2 == 1
FR_GENERATOR = 22
FR_TWO_ADICITY = 47
BLS_X = 0x8508C00000000001   # the curve's seed x (curves/mod.rs:16-19); r = x^4 - x^2 + 1, q = (x - 1)^2 r / 3 + x
assert R_MOD == BLS_X ** 4 - BLS_X ** 2 + 1 and 3 * Q_MOD == (BLS_X - 1) ** 2 * R_MOD + 3 * BLS_X
# the hard part of the final exponentiation (pairing.cuh) runs the chain of Hayashida, Hayasaka, Teruya, "Efficient final
# exponentiation via cyclotomic structure for pairings over families of elliptic curves" (eprint 2020/875), which yields the CUBE
assert 3 * ((Q_MOD ** 4 - Q_MOD ** 2 + 1) // R_MOD) == (BLS_X - 1) ** 2 * (BLS_X + Q_MOD) * (BLS_X ** 2 + Q_MOD ** 2 - 1) + 3
B = 29


def limbs(v, n):
    assert v < (1 << (B * n))
    return [(v >> (B * i)) & ((1 << B) - 1) for i in range(n)]


def arr(name, v, n, comment=""):
    return "    static constexpr uint32_t %s[%d] = {%s};%s" % (
        name, n, ", ".join("0x%08xu" % l for l in limbs(v, n)), ("  // " + comment) if comment else "")


def limbs_top(v, n):
    """n limbs, the last one holding everything above bit 29 (n - 1) (it may exceed 29 bits)."""
    assert v < (1 << (B * (n - 1) + 32))
    return [(v >> (B * i)) & ((1 << B) - 1) for i in range(n - 1)] + [v >> (B * (n - 1))]


def field(struct, p, L, W, internal=(), raw=(), LR=None):
    LR = LR or L
    RI = 1 << (B * LR)
    RE = 1 << (32 * W)
    assert RI > p
    kp = ["        {%s}," % ", ".join("0x%08xu" % l for l in limbs_top(k * p, L)) for k in range(9)]
    out = ["struct %s {" % struct,
           "    static constexpr int L = %d;      // 29-bit limbs" % L,
           "    static constexpr int LR = %d;     // Montgomery digits: the device's radix is RI = 2^(29 LR); LR = L + 1 leaves the" % LR,
           "                                      // product below p + 2^(29 (2L - LR) + 6) without a final subtraction (lazy domain)",
           "    static constexpr uint32_t KP[9][%d] = {   // k * p, k = 0..8; the top limb holds the excess over 29 bits" % L,
           ] + kp + ["    };",
           "    static constexpr int W = %d;      // 32-bit words of the external (arkworks) layout" % W,
           "    static constexpr int BITS = %d;" % p.bit_length(),
           arr("P", p, L),
           "    static constexpr uint32_t INV = 0x%08xu;  // -p^-1 mod 2^29" % ((-pow(p, -1, 1 << B)) % (1 << B)),
           arr("ONE", RI % p, L, "1 in internal form"),
           arr("RI2", (RI * RI) % p, L, "RAW: canonical -> internal"),
           arr("RAW_ONE", 1, L, "RAW: internal -> canonical"),
           arr("EXT_TO_CANON", (RI * pow(RE, -1, p)) % p, L, "RAW"),
           arr("CANON_TO_EXT", (RE * RI) % p, L, "RAW"),
           arr("EXT_TO_INT", (RI * RI * pow(RE, -1, p)) % p, L, "RAW (also fixes ext*ext products)"),
           arr("INT_TO_EXT", RE % p, L, "RAW"),
           arr("P_MINUS_2", p - 2, L, "Fermat inversion exponent (plain bits)"),
           ]
    for name, v in internal:
        out.append(arr(name, (v * RI) % p, L, "internal form"))
    for name, v in raw:
        out.append(arr(name, v % p, L, "RAW"))
    out.append("};")
    return "\n".join(out)


def sub_offset(p, L, K, j, top_bits=29):
    """K p written with limbs 0..L-2 in [j 2^29, (j + 1) 2^29) and whatever is left in the top limb: a + offset - b needs no
    borrow for any b whose limbs 0..L-2 are below j 2^29 (and whose top limb is below the offset's).  top_bits: the width the
    caller's arithmetic allows the top limb (29 for the Fr butterflies; 31 only where the caller has shown its sums keep inside
    32 bits: OFF3 of the 753-bit field)."""
    t = K * p - sum((j << B) << (B * i) for i in range(L - 1))
    assert t >= 0
    lo = [((t >> (B * i)) & ((1 << B) - 1)) + (j << B) for i in range(L - 1)]
    c = lo + [t >> (B * (L - 1))]
    assert sum(v << (B * i) for i, v in enumerate(c)) == K * p and c[-1] < (1 << top_bits), (K, hex(c[-1]))
    return c


def fr_lazy():
    """Constants of the lazy Fr domain of the NTT butterflies (frlazy.cuh): 2^261 / r = 438.8 leaves 8.8 bits of head room."""
    L = 9
    out = ["struct FrLazy {"]
    out.append(arr("RC", (1 << (B * L)) - R_MOD, L, "2^261 - r: a + q RC = (a - q r) + q 2^261"))
    out.append("    static constexpr uint32_t MQ = %du;      // floor(2^264 / r): q = (top limb * MQ) >> 32 <= floor(a / r)" % ((1 << 264) // R_MOD))
    for name, K, j in (("OFF2", 2, 1), ("OFF3", 3, 1), ("OFF5", 5, 2)):
        c = sub_offset(R_MOD, L, K, j)
        out.append("    static constexpr uint32_t %s[%d] = {%s};  // %d r, limbs 0..7 in [%d * 2^29, %d * 2^29)" % (
            name, L, ", ".join("0x%08xu" % v for v in c), K, j, j + 1))
    out.append("};")
    return "\n".join(out)


def fq753_lazy():
    """Constants of the lazy domain of the SHE butterflies (she.hip): 26 limbs hold 754 bits, q = 0.4427 * 2^754, so values below
    2.2 q keep every limb below 2^29 and a Montgomery product (RI = 2^754) of x < 2.2 q by y < q lands below 0.4427 x + q < 2 q."""
    L, q = 26, Q753_MOD
    out = ["struct Fq753Lazy {"]
    out.append(arr("RC", (1 << (B * L)) - q, L, "2^754 - q: a + k RC = (a - k q) + k 2^754"))
    d = (q >> (B * (L - 1))) + 1
    out.append("    static constexpr uint32_t MQ = %du;      // floor(2^56 / ((q >> 725) + 1)): k = (top limb * MQ) >> 56 <= floor(a / q)" % ((1 << 56) // d))
    for name, K in (("OFF2", 2), ("OFF3", 3)):
        c = sub_offset(q, L, K, 1, top_bits=31)
        out.append("    static constexpr uint32_t %s[%d] = {%s};  // %d q, limbs 0..24 in [2^29, 2^30)" % (
            name, L, ", ".join("0x%08xu" % v for v in c), K))
    out.append("};")
    return "\n".join(out)


def fq12_frobenius():
    """Fq12 = Fq2[w]/(w^6 - u), u^2 = -5 (pairing.cuh): the q^j-power map sends a_k w^k to conj^j(a_k) u^(k (q^j - 1) / 6) w^k, and
    u^(k (q^j - 1) / 6) = (-5)^(k (q^j - 1) / 12) lies in Fq because 12 divides q - 1.  FQ12_FROB[j - 1][k], internal form."""
    assert (Q_MOD - 1) % 12 == 0
    RI = 1 << (B * 14)
    out = ["static constexpr uint32_t FQ12_FROB[3][6][13] = {   // (-5)^(k (q^j - 1) / 12), j = 1..3, k = 0..5; internal form"]
    for j in (1, 2, 3):
        rows = []
        for k in range(6):
            g = pow(Q_MOD - 5, k * (Q_MOD ** j - 1) // 12, Q_MOD)
            rows.append("        {%s}," % ", ".join("0x%08xu" % l for l in limbs((g * RI) % Q_MOD, 13)))
        out += ["    {"] + rows + ["    },"]
    out.append("};")
    out.append("static constexpr uint64_t BLS12_X = 0x%016xull;   // the curve's seed (curves/mod.rs:16-19)" % BLS_X)
    return "\n".join(out)


# ---- subgroup membership through the endomorphisms (subgroup.cuh) --------------------------------------------------------------------
# A wrong constant below fails HERE (the build), not in a test: the identities are asserted on the generators with a textbook
# chord-and-tangent law over Fq and Fq2 = Fq[u]/(u^2 + 5).
def _f2mul(a, b):
    return ((a[0] * b[0] - 5 * a[1] * b[1]) % Q_MOD, (a[0] * b[1] + a[1] * b[0]) % Q_MOD)


def _f2inv(a):
    ni = pow((a[0] * a[0] + 5 * a[1] * a[1]) % Q_MOD, -1, Q_MOD)
    return (a[0] * ni % Q_MOD, -a[1] * ni % Q_MOD)


class _Fq:
    mul = staticmethod(lambda a, b: a * b % Q_MOD)
    sub = staticmethod(lambda a, b: (a - b) % Q_MOD)
    inv = staticmethod(lambda a: pow(a, -1, Q_MOD))
    k = staticmethod(lambda a, k: a * k % Q_MOD)
    zero = 0


class _Fq2:
    mul = staticmethod(_f2mul)
    sub = staticmethod(lambda a, b: ((a[0] - b[0]) % Q_MOD, (a[1] - b[1]) % Q_MOD))
    inv = staticmethod(_f2inv)
    k = staticmethod(lambda a, k: (a[0] * k % Q_MOD, a[1] * k % Q_MOD))
    zero = (0, 0)


def _ec_add(P, Q, F):
    if P is None or Q is None:
        return Q if P is None else P
    (x1, y1), (x2, y2) = P, Q
    if x1 == x2:
        if y1 != y2 or y1 == F.zero:
            return None
        lam = F.mul(F.k(F.mul(x1, x1), 3), F.inv(F.k(y1, 2)))
    else:
        lam = F.mul(F.sub(y2, y1), F.inv(F.sub(x2, x1)))
    x3 = F.sub(F.sub(F.mul(lam, lam), x1), x2)
    return (x3, F.sub(F.mul(lam, F.sub(x1, x3)), y1))


def _ec_mul(P, k, F):
    acc = None
    for bit in bin(k)[2:]:
        acc = _ec_add(acc, acc, F)
        if bit == "1":
            acc = _ec_add(acc, P, F)
    return acc


def subgroup_consts():
    """BETA2: phi(x, y) = (beta x, y) is lambda = x^2 - 1 on G1 (lambda^2 + lambda + 1 = r), so [x]([x] P) = P + phi(P) = -phi^2(P) =
    (beta^2 x, -y) exactly on the subgroup.  PSI_CX, PSI_CY: psi(x, y) = (conj(x) u^((q-1)/3), conj(y) u^((q-1)/2)) is the twist's
    untwist-Frobenius-twist map, [x] on G2; both coefficients lie in Fq (u^2 = -5 and 12 divides q - 1)."""
    import math
    lam = BLS_X * BLS_X - 1
    assert lam * lam + lam + 1 == R_MOD
    g1 = (G1X, G1Y)
    w = next(pow(g, (Q_MOD - 1) // 3, Q_MOD) for g in range(2, 50) if pow(g, (Q_MOD - 1) // 3, Q_MOD) != 1)
    lam_g1 = _ec_mul(g1, lam, _Fq)
    beta = next(b for b in (w, w * w % Q_MOD) if (b * G1X % Q_MOD, G1Y) == lam_g1)      # the beta of hostfield64.hpp::GLV_BETA
    beta2 = beta * beta % Q_MOD
    assert (beta2 * beta) % Q_MOD == 1 and beta2 != 1
    assert _ec_mul(_ec_mul(g1, BLS_X, _Fq), BLS_X, _Fq) == (beta2 * G1X % Q_MOD, Q_MOD - G1Y)
    assert (Q_MOD - 1) % 12 == 0
    cx, cy = pow(Q_MOD - 5, (Q_MOD - 1) // 6, Q_MOD), pow(Q_MOD - 5, (Q_MOD - 1) // 4, Q_MOD)
    g2 = ((G2X0, G2X1), (G2Y0, G2Y1))
    psi_g2 = ((G2X0 * cx % Q_MOD, -G2X1 * cx % Q_MOD), (G2Y0 * cy % Q_MOD, -G2Y1 * cy % Q_MOD))
    assert _ec_mul(g2, BLS_X, _Fq2) == psi_g2
    # psi^2 - t psi + q = 0 (t = x + 1): psi(Q) = x Q gives (q - x) Q = h1 r Q = O with h1 = (x - 1)^2 / 3, and the order of Q divides
    # #E'(Fq2) = h2 r; gcd(h1, h2) = 1 leaves r Q = O.  #E'(Fq2): the sextic twist of E(Fq2) whose order r divides.
    h1 = (BLS_X - 1) ** 2 // 3
    assert Q_MOD - BLS_X == h1 * R_MOD
    t2 = (BLS_X + 1) ** 2 - 2 * Q_MOD
    f2 = math.isqrt((4 * Q_MOD * Q_MOD - t2 * t2) // 3)
    assert 3 * f2 * f2 == 4 * Q_MOD * Q_MOD - t2 * t2
    orders = [n for n in (Q_MOD * Q_MOD + 1 - (t2 + 3 * f2) // 2, Q_MOD * Q_MOD + 1 - (t2 - 3 * f2) // 2) if n % R_MOD == 0]
    assert len(orders) == 1 and _ec_mul(g2, orders[0], _Fq2) is None
    assert math.gcd(h1, orders[0] // R_MOD) == 1
    # BETA itself: phi applied to a table entry (g1_lincomb.cuh: lincomb_term_glv)
    return [("BETA", beta), ("BETA2", beta2), ("PSI_CX", cx), ("PSI_CY", cy)]


def main():
    two_adic_root = pow(FR_GENERATOR, (R_MOD - 1) >> FR_TWO_ADICITY, R_MOD)
    print("// GENERATED by gen_consts.py -- do not edit.  29-bit little-endian limbs.")
    print("#pragma once")
    print("#include <stdint.h>")
    print("namespace zk {")
    print(field("FrParams", R_MOD, 9, 8, internal=[
        ("GENERATOR", FR_GENERATOR),                       # fr.rs:75-86 (22)
        ("GENERATOR_INV", pow(FR_GENERATOR, -1, R_MOD)),
        ("TWO_ADIC_ROOT", two_adic_root),                  # fr.rs:34-41
    ], raw=[
        # mmul(hi, WIDE_HI) = hi * 2^256 * RI: the upper half of a 512-bit sample folded into Fr (rng.hip)
        ("WIDE_HI", (1 << 256) * (1 << (B * 9)) * (1 << (B * 9))),
    ]))
    print("static constexpr int FR_TWO_ADICITY = %d;" % FR_TWO_ADICITY)
    print(fr_lazy())
    # Fq: ONE extra Montgomery digit (RI = 2^406, not 2^377).  q = 0.84 * 2^377 leaves no room between q and 2^(29 * 13):
    # with 13 digits every product needs a conditional subtraction and every sum a full reduction (43 % of the instructions
    # of a bucket addition).  With 14 digits a product of operands up to 7 q lands in [0, q + 2^354) by itself.
    print(field("FqParams", Q_MOD, 13, 12, LR=14, internal=[
        ("G1_GEN_X", G1X), ("G1_GEN_Y", G1Y),             # curves/g1.rs:43-51
        ("G2_GEN_X0", G2X0), ("G2_GEN_X1", G2X1),         # curves/g2.rs:63-86
        ("G2_GEN_Y0", G2Y0), ("G2_GEN_Y1", G2Y1),
        ("G2_B_C1", (-pow(5, -1, Q_MOD)) % Q_MOD),        # curves/g2.rs:28-35 (b' = 1/u)
        ("TS_ROOT", pow(FQ_QNR, (Q_MOD - 1) >> FQ_TWO_ADICITY, Q_MOD)),   # a primitive 2^46-th root of unity (QNR^T)
        ("INV2", (Q_MOD + 1) // 2),
    ] + subgroup_consts(), raw=[
        ("HALF", (Q_MOD - 1) // 2),                       # y > -y  <=>  canonical(y) > (q - 1) / 2
        ("TS_T_MINUS1_DIV2", (((Q_MOD - 1) >> FQ_TWO_ADICITY) - 1) // 2),   # Tonelli-Shanks exponent (plain bits)
    ]))
    print("static constexpr int FQ_TWO_ADICITY = %d;" % FQ_TWO_ADICITY)
    print(fq12_frobenius())
    root753 = pow(Q753_GENERATOR, (Q753_MOD - 1) >> Q753_TWO_ADICITY, Q753_MOD)
    assert pow(root753, 1 << (Q753_TWO_ADICITY - 1), Q753_MOD) == Q753_MOD - 1
    print(field("Fq753Params", Q753_MOD, 26, 24, internal=[
        ("TWO_ADIC_ROOT", root753),
        ("TWO_ADIC_ROOT_INV", pow(root753, -1, Q753_MOD)),
        ("INV2", (Q753_MOD + 1) // 2),
    ], raw=[
        ("HALF", (Q753_MOD - 1) // 2),                     # Encodedtext::decode threshold q/2 (src/she/encodedtext.rs:34-38)
        ("MOD_FR", Q753_MOD % R_MOD),                      # q mod p, subtracted from the upper half (ibid.)
    ]))
    print("static constexpr int FQ753_TWO_ADICITY = %d;" % Q753_TWO_ADICITY)
    print(fq753_lazy())
    # Fr constants that fold a 26-limb canonical integer into Fr: K[i] = 2^(29 i) * RE * RI mod r (RAW operands),
    # so that sum_i mmul(limb_i, K[i]) is the value mod r in external form.
    RI, RE = 1 << (B * 9), 1 << 256
    print("static constexpr uint32_t FR_FOLD29[26][9] = {")
    for i in range(26):
        print("    {%s}," % ", ".join("0x%08xu" % l for l in limbs((pow(2, B * i, R_MOD) * RE * RI) % R_MOD, 9)))
    print("};")
    print("}  // namespace zk")


if __name__ == "__main__":
    main()
