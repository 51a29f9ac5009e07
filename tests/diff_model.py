"""The exact model of the two-sample report: the two-sided Fisher exact test in integers and fractions, the delta filter in integers, the
tolerance that a double-precision result must keep, the case set of the tests, and the three files' rows by Python %-formatting.

p = sum{w(x) : w(x) <= w(mA) (1 + 1e-7)} / sum w(x) over the support, w(x) = C(dA, x) C(dB, mA + mB - x), with 1 + 1e-7 as the rational 10000001 / 10000000.
The weights are integers: the first one from math.comb, the others by the ratio w(x + 1) / w(x) = (dA - x)(c - x) / ((x + 1)(dB - c + x + 1)), which divides
exactly."""
import math
import random
from fractions import Fraction

TIE_NUM, TIE_DEN = 10000001, 10000000
A_DEPTHS = (1, 2, 3, 5, 8, 13, 30, 64, 200, 1000, 4000)
B_DEPTHS = (1, 2, 4, 7, 30, 65, 300, 2500)
DIRECTED = [(0, 1, 0, 1), (1, 1, 0, 1), (5, 10, 5, 10), (3, 6, 30, 60), (0, 4000, 2500, 2500), (4000, 4000, 0, 2500), (3, 3, 0, 3)]   # (mA, dA, mB, dB)
MORE_DIRECTED = [(2, 10, 8, 10), (0, 1, 1, 1), (1, 2, 3, 4), (2000, 4000, 1250, 2500), (0, 4000, 0, 2500), (4000, 4000, 2500, 2500), (1, 4000, 2499, 2500)]
CONTEXTS = ("CG", "CHG", "CHH", "CN")
POS_HEADER = "chr\tpos\tstrand\tcontext\tC_a\tCT_a\tratio_a\tC_b\tCT_b\tratio_b\tdelta\tp\n"
REGION_HEADER = "chr\tstart\tend\tname\tn_C\tC_a\tCT_a\tratio_a\tC_b\tCT_b\tratio_b\tdelta\tp\n"
BIN_HEADER = "chr\tstart\tend\tn_C\tC_a\tCT_a\tratio_a\tC_b\tCT_b\tratio_b\tdelta\tp\n"


def support(mA, dA, mB, dB):
    c = mA + mB
    return max(0, c - dB), min(dA, c)


def weights(mA, dA, mB, dB):
    """[w(lo), .., w(hi)] as integers"""
    c = mA + mB
    lo, hi = support(mA, dA, mB, dB)
    w = [math.comb(dA, lo) * math.comb(dB, c - lo)]
    for x in range(lo, hi):
        q, r = divmod(w[-1] * (dA - x) * (c - x), (x + 1) * (dB - c + x + 1))
        assert r == 0
        w.append(q)
    return w


def fisher(mA, dA, mB, dB):
    """the exact p as a Fraction"""
    w = weights(mA, dA, mB, dB)
    obs = w[mA - support(mA, dA, mB, dB)[0]]
    return Fraction(sum(x for x in w if x * TIE_DEN <= obs * TIE_NUM), sum(w))


def near_boundary(mA, dA, mB, dB):
    """some w(x) / w(mA) lies within 1e-8 of 1 + 1e-7 without being equal to it: a correctly rounded double may select differently there"""
    w = weights(mA, dA, mB, dB)
    obs = w[mA - support(mA, dA, mB, dB)[0]]
    return any(x * TIE_DEN != obs * TIE_NUM and abs(x * 10 ** 8 - obs * (10 ** 8 + 10)) <= obs for x in w)


def rtol(mA, dA, mB, dB):
    """64 (s + 16) 2^-53 for a support of s tables: a serial recurrence rounds at most 4 times per step and each sum once per term, so a weight and a sum of
    positive weights are within 5 s 2^-53 to first order; the bound is about 12 times that"""
    lo, hi = support(mA, dA, mB, dB)
    return Fraction(64 * (hi - lo + 1 + 16), 2 ** 53)


def p_error(got, quad):
    """None where `got` (a float) keeps the bound for the counts `quad`, else a description.  Below an exact p of 1e-290 relative weights reach the
    denormals: there the result must lie in [0, 1e-289]"""
    want = fisher(*quad)
    if not (got == got) or got < 0.0 or got > 1.0:
        return "%r: p = %r is no probability" % (quad, got)
    if want < Fraction(1, 10 ** 290):
        return None if got <= 1e-289 else "%r: p = %r, exact %.6e is below 1e-290" % (quad, got, want)
    err = abs(Fraction(got) - want) / want
    return None if err <= rtol(*quad) else "%r: p = %r, exact %r, relative error %.3e above %.3e" % (quad, got, float(want), float(err), float(rtol(*quad)))


def cases():
    """the 3,006 quadruples of the tests: 34 seeded draws of (mA, mB) per pair of depths, then the directed ones"""
    rng = random.Random(7)
    out = [(rng.randint(0, dA), dA, rng.randint(0, dB), dB) for dA in A_DEPTHS for dB in B_DEPTHS for _ in range(34)]
    return out + DIRECTED + MORE_DIRECTED


def delta_keeps(mA, dA, mB, dB, permille):
    return abs(mA * dB - mB * dA) * 1000 >= permille * dA * dB


def numbers_text(mA, dA, mB, dB, p):
    ra, rb = mA / dA, mB / dB
    return "\t%d\t%d\t%.3f\t%d\t%d\t%.3f\t%+.3f\t%.4e\n" % (mA, dA, ra, mB, dB, rb, rb - ra, p)


def pos_row_text(name, pos0, letter, cls, counts, p):
    """letter: the reference letter at the position (C: '+'); cls: 0..3"""
    return "%s\t%d\t%s\t%s" % (name, pos0 + 1, "+" if letter == "C" else "-", CONTEXTS[cls]) + numbers_text(*counts, p)


def interval_row_text(name, start, end, label, sums, p):
    """label None: a row of the bin file"""
    head = "%s\t%d\t%d" % (name, start, end) + ("" if label is None else "\t" + label)
    if not sums[0]:
        return head + "\t0\t0\t0\tNA\t0\t0\tNA\tNA\tNA\n"
    return head + "\t%d" % sums[0] + numbers_text(*sums[1:], p)


def context_class(ref, i):
    """the class of the cytosine at i of the sequence `ref` (C looks right, G looks left; a neighbour outside the sequence is no letter): 0 CG, 1 CHG, 2 CHH, 3 CN"""
    plus = ref[i] == "C"
    n1, n2 = (ref[i + 1:i + 2], ref[i + 2:i + 3]) if plus else (ref[i - 1:i] if i >= 1 else "", ref[i - 2:i - 1] if i >= 2 else "")
    g, h = ("G", "ATC") if plus else ("C", "ATG")
    if n1 == g:
        return 0
    if not n1 or n1 not in h:
        return 3
    if n2 == g:
        return 1
    return 2 if n2 and n2 in h else 3
