"""Would the exact NTT tests (test_gpu_ntt_exact.py) notice a wrong kernel?  No broken library is built or run: the device
schedule is restated on python integers (ntt_cases.model_ntt: the passes, columns, stages, twiddle exponents and the scatter of
k_ntt_pass), three single-line defects are planted in that model, and the tests' own comparator (ntt_cases.mismatch against the C
oracle) has to reject the result.  Runs without a GPU."""
import pytest

import ntt_cases as NC
import zkref_c as OC

# the kinds a defect can change at all: the eb negation exists on the inverse only, the post table on the coset inverse only
AFFECTED = {"twiddle": NC.KINDS, "eb": ((1, 0), (1, 1)), "post": ((1, 1),)}


@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 5, 6, 10, 11, 12])
def test_model_is_the_transform(log_n):
    """Without a defect the model equals the C oracle for every family and kind: one-pass sizes with odd and even logM, and
    the two-pass sizes 11 (6 + 5 levels) and 12 (6 + 6) with the inter-pass twiddles and the scatter."""
    for name in NC.FAMILIES:
        v = NC.family(name, log_n)
        for inverse, coset in NC.KINDS:
            got = NC.model_residues(v, log_n, inverse, coset)
            assert NC.mismatch(got, OC.fft(v, log_n, inverse, coset)) is None, (name, NC.KIND_NAME[inverse, coset])


def caught_by(defect, log_n):
    out = set()
    for name in NC.FAMILIES:
        v = NC.family(name, log_n)
        for kind in AFFECTED[defect]:
            got = NC.model_residues(v, log_n, kind[0], kind[1], defect)
            if NC.mismatch(got, OC.fft(v, log_n, kind[0], kind[1])) is not None:
                out.add((name, NC.KIND_NAME[kind]))
    return out


# what each structured family cannot see, by construction (the sparse spectra that make them exact closed forms also hide values)
MISSED = {
    "twiddle": {(n, k) for n in ("all_r-1", "alt_r-1_1", "geometric") for k in ("fft", "ifft", "coset_ifft")},
    "eb": {(n, k) for n in ("all_r-1", "alt_r-1_1") for k in ("ifft", "coset_ifft")},
    "post": {("all_r-1", "coset_ifft")},
}


@pytest.mark.parametrize("log_n", [11, 12])
@pytest.mark.parametrize("defect", NC.DEFECTS)
def test_comparator_rejects_planted_defects(defect, log_n):
    """At the two-pass sizes 11 and 12, for every family and every kind the defect can change.  What was found, and is asserted:
      twiddle (ONE (l, q) pair of the first pass, l = S - 1, q = M - 1, exponent + 1): caught in all four kinds by random,
        mask_0_r-1 and delta (its index has every low bit set, so its one non-zero column is l = S - 1), and in the coset
        forward kind by every family (the g^i pre-scale spreads any input over all frequencies).  Missed elsewhere by all_r-1,
        alt_r-1_1 and geometric: their first-pass sub-transforms are zero at (l, q), and a wrong factor of zero shows nothing.
      eb (not negated on the inverse): caught in both inverse kinds by random, mask_0_r-1, delta and geometric; missed by
        all_r-1 and alt_r-1_1, where x1 - x3 = 0 wherever the wrong twiddle multiplies.
      post (coset inverse's table read at idx, not dst): caught by every family except all_r-1, whose only non-zero output is
        element 0, its own bit reversal.
    So random input, the 0 / r-1 mask and the delta catch every defect in every kind it can change; the constant, alternating
    and geometric vectors are in the suite for the lazy range and the closed form, not for index mistakes."""
    every = {(n, NC.KIND_NAME[k]) for n in NC.FAMILIES for k in AFFECTED[defect]}
    got = caught_by(defect, log_n)
    assert every - got == MISSED[defect]
    for name in ("random", "mask_0_r-1", "delta"):
        assert all((name, NC.KIND_NAME[k]) in got for k in AFFECTED[defect])
