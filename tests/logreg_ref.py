"""Data, numpy fp64 references and the recorded sklearn results shared by
tests/test_logreg_cpu.py, tests/test_gpu_logreg.py and tests/golden/make_logreg_golden.py
(no test in this file).

The objective is sklearn's binary LogisticRegression(penalty="l2", fit_intercept=True),
scaled as sklearn >= 1.4 scales it, over wb = (w, b):

    f(wb) = (1/N) sum_i [softplus(z_i) - y_i z_i] + |w|^2 / (2 C N),   z_i = x_i . w + b

Everything here is numpy fp64 on the fp32 features; nothing of the code under test runs.
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "logreg_sklearn.json")
U = 2.0 ** -53                      # unit roundoff of fp64
CASES = [(301, 37, 1.5), (1030, 67, 1.5), (515, 384, 2.0)]   # (N, D, sep); the third is separable
BIG = (2051, 512, 2.0)              # the reference-sized probe (GPU end to end only)
N_VAL = 259


def features(N, D, seed, sep):
    """(x fp32 [N, D], y float64 [N] in {0, 1}): a unit class direction mu fixed by D alone (its
    own seed, so train and validation draws of one case share it), y ~ Bernoulli(0.3),
    x = relu(N(0, 1) + 0.5 + (2 y - 1) sep mu): non-negative like pooled features."""
    mu = np.random.default_rng(1000 + D).standard_normal(D)
    mu /= np.linalg.norm(mu)
    rng = np.random.default_rng(seed)
    y = (rng.random(N) < 0.3).astype(np.float64)
    if y.min() == y.max():          # tiny N: keep both classes
        y[0] = 1.0 - y[0]
    x = rng.standard_normal((N, D)) + 0.5 + (2.0 * y - 1.0)[:, None] * sep * mu
    return np.maximum(x, 0.0).astype(np.float32), y


def case(N, D, sep):
    """(train x, y, validation x, y) of one case: seeds N and N + 1, 259 validation rows."""
    x, y = features(N, D, N, sep)
    xv, yv = features(N_VAL, D, N + 1, sep)
    return x, y, xv, yv


def scores(X, wb):
    return np.asarray(X, dtype=np.float64) @ wb[:-1] + wb[-1]


def row_terms(z, y):
    """(l_i, p_i, s_i) per row in overflow-safe fp64: l = softplus((1 - 2 y) z)."""
    l = np.logaddexp(0.0, np.where(y > 0.5, -z, z))
    e = np.exp(-np.abs(z))
    p = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return l, p, e / (1.0 + e) ** 2


def loss_grad(X, y, wb, C=1.0):
    """(f, gradient [D + 1])."""
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    lam = 1.0 / (C * N)
    l, p, _ = row_terms(scores(X, wb), y)
    c = p - y
    g = np.append(X.T @ c, c.sum()) / N
    g[:-1] += lam * wb[:-1]
    return l.sum() / N + 0.5 * lam * (wb[:-1] ** 2).sum(), g


def hvp(X, y, wb, q, C=1.0):
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    _, _, s = row_terms(scores(X, wb), y)
    c = s * scores(X, q)
    h = np.append(X.T @ c, c.sum()) / N
    h[:-1] += q[:-1] / (C * N)
    return h


def hessian(X, y, wb, C=1.0):
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    _, _, s = row_terms(scores(X, wb), y)
    Xt = np.hstack([X, np.ones((N, 1))])
    H = (Xt * s[:, None]).T @ Xt / N
    H[np.arange(D), np.arange(D)] += 1.0 / (C * N)
    return H


def optimum(X, y, C=1.0, gtol=1e-13, max_iter=200):
    """The minimiser by a plain damped Newton method with np.linalg.solve, run until the
    largest gradient entry is at most gtol."""
    wb = np.zeros(np.asarray(X).shape[1] + 1)
    f, g = loss_grad(X, y, wb, C)
    for _ in range(max_iter):
        if np.abs(g).max() <= gtol:
            return wb
        d = np.linalg.solve(hessian(X, y, wb, C), -g)
        t = 1.0
        while True:
            ft, gt = loss_grad(X, y, wb + t * d, C)
            if ft <= f + 1e-4 * t * (g @ d) + 1e-15 * abs(f) or t < 1e-10:
                break
            t *= 0.5
        wb, f, g = wb + t * d, ft, gt
    raise RuntimeError(f"optimum: gradient {np.abs(g).max():.3e} after {max_iter} Newton steps")


def distance_bound(X, y, wb, wb_star, C=1.0):
    """(|wb - wb*|_2, 2 |g(wb)|_2 / lambda_min(H(wb*))): the strong-convexity bound on the
    distance to the optimum; the factor 2 covers the Hessian's change between the two points."""
    g = loss_grad(X, y, wb, C)[1]
    lam_min = np.linalg.eigvalsh(hessian(X, y, wb_star, C))[0]
    return float(np.linalg.norm(wb - wb_star)), float(2.0 * np.linalg.norm(g) / lam_min)


def balanced_accuracy(y, pred):
    y, pred = np.asarray(y), np.asarray(pred)
    return 0.5 * (((pred == 1) & (y == 1)).sum() / (y == 1).sum() + ((pred == 0) & (y == 0)).sum() / (y == 0).sum())


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def golden_case(golden, N, D):
    return golden["cases"][f"{N}x{D}"]
