"""fp64 references and the tolerance shared by tests/test_silhouette_cpu.py and
tests/test_gpu_silhouette.py (no test in this file).

Tolerance of one `sums[q][c]` entry against fp64 arithmetic on the same inputs,
u the unit round-off of the arithmetic under test (2^-24 for the fp32 kernel,
2^-53 for the fp64 host path):

  * a difference a_d - b_d is rounded once: relative error <= u, so its square
    carries <= 2u, the product's own rounding one more;
  * the squares are non-negative, so summing D of them in any order adds a
    relative error of at most (D - 1) u to first order: the squared distance
    is within (D + 2) u;
  * the square root halves that and rounds once: a distance is within
    (D / 2 + 2) u <= (D + 3) u;
  * the distances are non-negative, so summing up to N of them in any order
    (lane partials, shuffles) adds at most (N - 1) u <= N u.

First order: (D + N + 3) u for any summation order; rtol = 2 (D + N + 3) u, the
factor 2 covering the higher-order terms.  A silhouette value is
(b - a) / max(a, b) with a and b such sums over exact counts: the difference
b - a has absolute error <= rtol (a + b) <= 2 rtol max(a, b), and the
denominator's relative error adds rtol |s| <= rtol: atol = 4 rtol bounds it
with room.  Nothing here is tuned to what the code gives.
"""
import numpy as np


def sums_rtol(N, D, u=2.0 ** -24):
    return 2.0 * (D + N + 3) * u


def silhouette_atol(N, D, u=2.0 ** -24):
    return 4.0 * sums_rtol(N, D, u)


def label_ids(labels):
    uniq = sorted(set(labels))
    return np.array([uniq.index(v) for v in labels], dtype=np.int64), len(uniq)


def cluster_sums_fp64(X, ids, C, Xq=None):
    """[Q, C] float64 sums of direct-difference Euclidean distances."""
    X = np.asarray(X, dtype=np.float64)
    Xq = X if Xq is None else np.asarray(Xq, dtype=np.float64)
    out = np.zeros((Xq.shape[0], C))
    for q in range(Xq.shape[0]):
        d = np.sqrt(((Xq[q][None, :] - X) ** 2).sum(1))
        out[q] = np.bincount(ids, weights=d, minlength=C)
    return out


def silhouette_samples_fp64(X, labels):
    """sklearn's definition, written out: singleton clusters and 0 / 0 score 0."""
    ids, C = label_ids(list(labels))
    S = cluster_sums_fp64(X, ids, C)
    n = np.bincount(ids, minlength=C).astype(np.float64)
    out = np.zeros(len(ids))
    for i, c in enumerate(ids):
        if n[c] == 1:
            continue
        a = S[i, c] / (n[c] - 1)
        b = min(S[i, k] / n[k] for k in range(C) if k != c)
        out[i] = 0.0 if max(a, b) == 0 else (b - a) / max(a, b)
    return out
