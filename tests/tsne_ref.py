"""Data, references and gates shared by tests/test_tsne_cpu.py, tests/test_gpu_tsne.py
and tests/golden/make_tsne_golden.py (no test in this file).

The yardstick is scikit-learn's exact t-SNE: sklearn.manifold._t_sne._joint_probabilities
and _kl_divergence (degrees_of_freedom = 1) are called directly; what takes seconds
(TSNE.fit_transform over five seeds) is recorded in tests/golden/tsne_sklearn.json.
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsne_sklearn.json")
N_E2E, D_E2E, PERPLEXITY_E2E = 300, 32, 30.0
EPS = np.finfo(np.double).eps


def blobs(N=N_E2E, D=D_E2E, seed=0, dup=0):
    """Three Gaussian blobs (unit variance, centres of scale 4) from a seeded generator,
    fp32 [N, D] and the blob index; the last `dup` rows repeat the first `dup`."""
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.standard_normal((3, D))
    lab = np.arange(N) % 3
    x = (centres[lab] + rng.standard_normal((N, D))).astype(np.float32)
    if dup:
        x[N - dup:] = x[:dup]
    return x, lab


def sqdist_f32(x):
    """fp32 [N, N] squared distances from fp64 direct differences (exact zero diagonal)."""
    xd = np.asarray(x, dtype=np.float64)
    return ((xd[:, None, :] - xd[None, :, :]) ** 2).sum(-1).astype(np.float32)


def sk_joint(d2, perplexity):
    """sklearn's joint P as a dense fp64 [N, N]."""
    from scipy.spatial.distance import squareform
    from sklearn.manifold._t_sne import _joint_probabilities
    return squareform(_joint_probabilities(np.asarray(d2, dtype=np.float32), perplexity, 0))


def sk_conditional(d2, perplexity):
    from sklearn.manifold import _utils
    return _utils._binary_search_perplexity(np.ascontiguousarray(d2, dtype=np.float32), perplexity, 0)


def sk_kl_grad(y, P_dense, exag=1.0):
    """(KL of the unscaled P, gradient with the attractive term scaled by exag), both from
    sklearn's _kl_divergence in fp64: the KL from a call on P, the gradient from a call on
    exag P, which is what TSNE hands it during the early exaggeration."""
    from scipy.spatial.distance import squareform
    from sklearn.manifold._t_sne import _kl_divergence
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    P = squareform(np.asarray(P_dense, dtype=np.float64), checks=False)
    kl, _ = _kl_divergence(y.ravel().copy(), P, 1, n, 2)
    _, grad = _kl_divergence(y.ravel().copy(), exag * P, 1, n, 2)
    return float(kl), grad.reshape(n, 2)


def np_conditional(d2, perplexity):
    """An independent fp64 numpy restatement of the perplexity search (row by row, the
    entropy from the unnormalised sums), for the total-variation gate's yardstick."""
    d = np.asarray(d2, dtype=np.float32).astype(np.float64)
    n = d.shape[0]
    out = np.zeros((n, n))
    target = np.log(perplexity)
    for i in range(n):
        di = np.delete(d[i], i)
        beta, lo, hi = 1.0, -np.inf, np.inf
        for _ in range(100):
            e = np.exp(-di * beta)
            s = e.sum()
            if s == 0.0:
                s = 1e-8
            p = e / s
            diff = np.log(s) + beta * (di * e).sum() / s - target
            if abs(diff) <= 1e-5:
                break
            if diff > 0:
                lo = beta
                beta = beta * 2 if hi == np.inf else (beta + hi) / 2
            else:
                hi = beta
                beta = beta / 2 if lo == -np.inf else (beta + lo) / 2
        out[i] = np.insert(p, i, 0.0)
    return out


def np_joint(cond):
    P = cond + cond.T
    P = np.maximum(P / max(P.sum(), EPS), EPS)
    np.fill_diagonal(P, 0.0)
    return P


def total_variation(a, b):
    return 0.5 * np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).sum()


def row_entropy(cond):
    """fp64 Shannon entropy (nats) of every row, rows renormalised (a stored row need not sum to 1)."""
    c = np.asarray(cond, dtype=np.float64)
    c = c / c.sum(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(c > 0, c * np.log(c), 0.0)
    return -t.sum(1)


def np_update(grad, update, gains, momentum, lr):
    """_gradient_descent's step on fp32 arrays, as numpy rounds it: (gained grad, update, gains, step)."""
    grad, update, gains = (np.array(a, dtype=np.float32) for a in (grad, update, gains))
    inc = update * grad < 0.0
    dec = np.invert(inc)
    gains[inc] += 0.2
    gains[dec] *= 0.8
    np.clip(gains, 0.01, np.inf, out=gains)
    grad *= gains
    update = momentum * update - lr * grad
    assert update.dtype == np.float32
    return grad, update, gains


def fixed_y(N, scale, seed=1):
    """A fixed fp32 embedding [N, 2]: three separated groups at the given spread."""
    rng = np.random.default_rng(seed)
    lab = np.arange(N) % 3
    c = np.array([[1.0, 0.0], [-0.5, 0.9], [-0.5, -0.9]])
    return (scale * (c[lab] + 0.3 * rng.standard_normal((N, 2)))).astype(np.float32)


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def e2e_gates(golden, max_iter):
    """(KL ceiling, trustworthiness floor) from sklearn's five seeds at max_iter: the worst of
    the five, moved by their spread (max - min), the noise of the optimiser itself."""
    g = golden[f"max_iter_{max_iter}"]
    kl, tr = g["kl"], g["trustworthiness"]
    return max(kl) + (max(kl) - min(kl)), min(tr) - (max(tr) - min(tr))
