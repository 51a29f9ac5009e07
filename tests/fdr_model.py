"""The model of the q-values and the de novo DMRs of the two-sample report.

bh(p) is Benjamini-Hochberg in numpy, operation for operation what include/bsx.h defines: the family's p sorted ascending, r_k = (p_(k) * n) / k as two
double operations, q_(k) = min(1, min over j >= k of r_j), every row the q of its p; a NaN is outside the family and stays NaN.  The device's q must equal
it bit for bit.  candidate_runs / dmrs work on rows in plain Python integers: a row is (sequence, pos0, mA, dA, mB, dB), listed in the store's order."""
import numpy as np

import diff_model as D

POS_FDR_HEADER = D.POS_HEADER[:-1] + "\tq\n"
REGION_FDR_HEADER = D.REGION_HEADER[:-1] + "\tq\n"
DMR_HEADER = "chr\tstart\tend\tn_sig\tn_C\tC_a\tCT_a\tratio_a\tC_b\tCT_b\tratio_b\tdelta\tp\n"


def bh(p):
    p = np.asarray(p, np.float64)
    q = np.full(p.shape, np.nan)
    family = np.flatnonzero(~np.isnan(p))
    n = family.size
    if n == 0:
        return q
    order = family[np.argsort(p[family], kind="stable")]
    r = p[order] * float(n) / np.arange(1, n + 1)
    q_sorted = np.minimum.accumulate(r[::-1])[::-1]
    q[order] = np.minimum(q_sorted, 1.0)
    return q


def sign(mA, dA, mB, dB):
    x = mB * dA - mA * dB
    return (x > 0) - (x < 0)


def is_candidate(row, q, max_q, permille):
    return q <= max_q and D.delta_keeps(*row[2:], permille) and sign(*row[2:]) != 0


def candidate_runs(rows, q, max_q, permille, max_gap):
    """the maximal runs, each a list of indices into rows: candidates that follow one another among the candidates on one sequence with one sign, each at
    most max_gap behind the one before"""
    runs, last = [], None
    for i, (row, qi) in enumerate(zip(rows, q)):
        if not is_candidate(row, float(qi), max_q, permille):
            continue
        s = sign(*row[2:])
        if last is not None and last[0] == row[0] and last[2] == s and row[1] - last[1] <= max_gap:
            runs[-1].append(i)
        else:
            runs.append([i])
        last = (row[0], row[1], s)
    return runs


def dmrs(rows, q, max_q, permille, max_gap, min_sites):
    """[(sequence, start, end, n_sig)] of the runs with at least min_sites candidates"""
    return [(rows[r[0]][0], rows[r[0]][1], rows[r[-1]][1] + 1, len(r)) for r in candidate_runs(rows, q, max_q, permille, max_gap) if len(r) >= min_sites]


def q_text(q):
    return "NA" if q != q else "%.4e" % q


def with_q(row_text, q):
    """a row of diff_model with the q column behind it"""
    return row_text[:-1] + "\t" + q_text(q) + "\n"


def dmr_row_text(name, start, end, n_sig, sums, p):
    return "%s\t%d\t%d\t%d\t%d" % (name, start, end, n_sig, sums[0]) + D.numbers_text(*sums[1:], p)
