"""Clustering metrics and the t-SNE embedding over cached feature rows.

silhouette_samples / silhouette_score restate sklearn.metrics' Euclidean
silhouette (the reference calls it on the best checkpoint's features,
plot_tsne_and_calculate_silhouette.py:56-60).  With S[i, c] the sum of the
distances from row i to the rows of cluster c and n_c the cluster sizes:

    a_i = S[i, c_i] / (n_{c_i} - 1)
    b_i = min over c != c_i of S[i, c] / n_c
    s_i = (b_i - a_i) / max(a_i, b_i)

with s_i = 0 for the only member of a cluster and where the quotient is 0 / 0;
the score is the mean of s_i in fp64.  On a device tensor S comes from
ops.cluster_dist_sums (HIP, fp32 direct differences, no N x N matrix); on a CPU
tensor from torch.cdist in fp64 (the off-GPU path).

tsne restates sklearn.manifold.TSNE(method="exact", init="pca") (the reference
calls it on the same features, plot_tsne_and_calculate_silhouette.py:62-66); see
its docstring.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple, Union

import torch

MAX_CLUSTERS = 8   # kMaxClusters of csrc/retrieval_ops.hip


def label_ids(labels: Sequence) -> Tuple[List[int], list]:
    """Labels (ints, 0-d tensors, strings, or a 1-D tensor) -> (ids, sorted unique values)."""
    if torch.is_tensor(labels):
        labels = labels.reshape(-1).tolist()
    vals = [v.item() if torch.is_tensor(v) else v for v in labels]
    uniq = sorted(set(vals))
    index = {v: i for i, v in enumerate(uniq)}
    return [index[v] for v in vals], uniq


def _cluster_sums(x: torch.Tensor, ids: torch.Tensor, C: int) -> torch.Tensor:
    """[N, C] fp64 per-cluster distance sums."""
    if x.is_cuda:
        from . import ops
        return ops.cluster_dist_sums(x, ids.to(torch.int32), C).double()
    xd = x.double()
    onehot = torch.nn.functional.one_hot(ids, C).double()
    return torch.cdist(xd, xd, compute_mode="donot_use_mm_for_euclid_dist") @ onehot


def silhouette_samples(x: torch.Tensor, labels: Sequence) -> torch.Tensor:
    """fp64 [N] silhouette coefficient of every row of x [N, D] (on x's device)."""
    if x.dim() != 2:
        raise ValueError(f"silhouette_samples: x must be [N, D], got {tuple(x.shape)}")
    ids_l, uniq = label_ids(labels)
    N, C = x.shape[0], len(uniq)
    if len(ids_l) != N:
        raise ValueError(f"silhouette_samples: {N} rows but {len(ids_l)} labels")
    if not 1 < C < N:   # sklearn.metrics.cluster._unsupervised.check_number_of_labels
        raise ValueError("Number of labels is %d. Valid values are 2 to n_samples - 1 (inclusive)" % C)
    if C > MAX_CLUSTERS:
        raise ValueError(f"silhouette_samples: {C} distinct labels, at most {MAX_CLUSTERS} are supported")
    ids = torch.tensor(ids_l, dtype=torch.long, device=x.device)
    S = _cluster_sums(x, ids, C)
    n = torch.bincount(ids, minlength=C).double()
    own = torch.nn.functional.one_hot(ids, C).bool()
    n_own = n[ids]
    a = S.gather(1, ids[:, None]).squeeze(1) / (n_own - 1)       # 0 / 0 = nan for a singleton
    b = (S / n).masked_fill(own, float("inf")).min(dim=1).values
    s = (b - a) / torch.maximum(a, b)
    return torch.where(n_own == 1, torch.zeros_like(s), torch.nan_to_num(s, nan=0.0))


def silhouette_score(x: torch.Tensor, labels: Sequence) -> float:
    return float(silhouette_samples(x, labels).mean())


# ---------------- t-SNE ----------------
TSNE_MAX_N = 32768            # P [N, N] fp32 stays within 4 GB (kTsneMaxN of csrc/tsne_ops.hip)
_EPS = 2.220446049250313e-16  # sklearn's MACHINE_EPSILON (np.finfo(np.double).eps)
_EXPLORATION_ITERS = 250      # TSNE._EXPLORATION_MAX_ITER: the early-exaggeration stage
_N_ITER_CHECK = 50            # TSNE._N_ITER_CHECK


def tsne_pca_init(x: torch.Tensor) -> torch.Tensor:
    """[N, 2] fp32 on x's device: the first two principal components of x, the sign
    of each chosen so that the component's largest-magnitude entry is positive
    (sklearn's svd_flip), scaled so that the first has standard deviation 1e-4.  The
    D x D covariance and its eigh are host fp64: one copy of the features, before
    the descent starts, and the same bits whichever device x is on."""
    xd = x.detach().double().cpu()
    xc = xd - xd.mean(0, keepdim=True)
    w, v = torch.linalg.eigh(xc.T @ xc)
    comps = v[:, [-1, -2]] if v.shape[1] > 1 else torch.cat([v, torch.zeros_like(v)], 1)
    big = comps.abs().argmax(0)
    comps = comps * torch.sign(comps[big, torch.arange(2)]).masked_fill(comps[big, torch.arange(2)] == 0, 1.0)
    y = (xc @ comps).float()
    y = y / y[:, 0].std(unbiased=False) * 1e-4
    return y.to(x.device).contiguous()


def tsne_sqdist_cpu(x: torch.Tensor) -> torch.Tensor:
    """[N, N] fp32 squared distances from direct fp32 differences, in row chunks."""
    x = x.float()
    N, D = x.shape
    rows = max(1, (64 << 20) // max(1, 4 * N * D))
    return torch.cat([((x[r:r + rows, None, :] - x[None, :, :]) ** 2).sum(-1) for r in range(0, N, rows)])


def tsne_conditional_cpu(d2: torch.Tensor, perplexity: float) -> torch.Tensor:
    """fp64 [N, N]: sklearn's _binary_search_perplexity on fp32 squared distances,
    every row's search advanced together (a row that has stopped is left alone)."""
    d = d2.float().double()
    N = d.shape[0]
    off = ~torch.eye(N, dtype=torch.bool)
    target = math.log(perplexity)
    beta = torch.ones(N, dtype=torch.float64)
    lo = torch.full((N,), -math.inf, dtype=torch.float64)
    hi = torch.full((N,), math.inf, dtype=torch.float64)
    cond = torch.zeros(N, N, dtype=torch.float64)
    live = torch.arange(N)
    for _ in range(100):
        if live.numel() == 0:
            break
        b = beta[live]
        e = torch.exp(-d[live] * b[:, None]) * off[live]
        s = e.sum(1)
        s = torch.where(s == 0, torch.full_like(s, 1e-8), s)
        p = e / s[:, None]
        cond[live] = p
        diff = torch.log(s) + b * (d[live] * p).sum(1) - target
        go = diff.abs() > 1e-5
        up = go & (diff > 0)
        dn = go & ~(diff > 0)
        l, h = lo[live], hi[live]
        l = torch.where(up, b, l)
        h = torch.where(dn, b, h)
        nb = torch.where(up, torch.where(torch.isinf(h), b * 2, (b + h) / 2), b)
        nb = torch.where(dn, torch.where(torch.isinf(l), b / 2, (b + l) / 2), nb)
        beta[live], lo[live], hi[live] = nb, l, h
        live = live[go]
    return cond


def tsne_joint_cpu(cond: torch.Tensor) -> torch.Tensor:
    """fp32 [N, N] joint probabilities of an fp64 conditional matrix (_joint_probabilities)."""
    P = cond + cond.T
    P = torch.clamp_min(P / max(float(P.sum()), _EPS), _EPS)
    P.fill_diagonal_(0.0)
    return P.float()


def tsne_grad_cpu(y: torch.Tensor, P: torch.Tensor, exag: float = 1.0, dtype=torch.float32):
    """(KL of the unscaled P, gradient [N, 2]) of sklearn's _kl_divergence at degrees_of_freedom 1
    with P scaled by exag in the attractive term, in `dtype` throughout."""
    y, P = y.to(dtype), P.to(dtype)
    diff = y[:, None, :] - y[None, :, :]
    q = 1.0 / (1.0 + (diff ** 2).sum(-1))
    q.fill_diagonal_(0.0)
    Z = q.sum().clamp_min(_EPS)
    Q = (q / Z).clamp_min(_EPS)
    nz = P > 0
    kl = torch.where(nz, P * torch.log(P.clamp_min(_EPS) / Q), torch.zeros_like(P)).sum()
    grad = 4.0 * torch.einsum("ij,ijc->ic", (exag * P - q / Z) * q, diff)
    return float(kl), grad


def tsne_step_cpu(grad, y, update, gains, momentum, lr):
    """_gradient_descent's step, in place on y, update, gains (fp32, each operation rounded
    on its own); returns the gained gradient."""
    inc = update * grad < 0
    gains.copy_(torch.where(inc, gains + 0.2, gains * 0.8).clamp_min(0.01))
    grad = grad * gains
    update.copy_(momentum * update - lr * grad)
    y += update
    return grad


class _CpuDescent:
    def __init__(self, x, perplexity):
        self.P = tsne_joint_cpu(tsne_conditional_cpu(tsne_sqdist_cpu(x), perplexity))

    def start(self, y):
        self.y, self.update, self.gains = y, torch.zeros_like(y), torch.ones_like(y)
        self.stats = (float("nan"), float("nan"))

    def reset(self):
        self.update.zero_()
        self.gains.fill_(1.0)

    def step(self, exag, momentum, lr, check):
        kl, grad = tsne_grad_cpu(self.y, self.P, exag)
        grad = tsne_step_cpu(grad, self.y, self.update, self.gains, momentum, lr)
        if check:
            self.stats = (kl, float(grad.double().norm()))

    def read(self):
        return self.stats


class _HipDescent:
    def __init__(self, x, perplexity):
        from . import ops
        self.ops = ops
        self.P = ops.tsne_affinities(ops.tsne_sqdist(x), perplexity)

    def start(self, y):
        N = y.shape[0]
        self.y, self.update, self.gains = y, torch.zeros_like(y), torch.ones_like(y)
        self.parts = torch.zeros(N, self.ops.TSNE_PARTS, dtype=torch.float64, device=y.device)
        self.stats = torch.zeros(2, dtype=torch.float64, device=y.device)

    def reset(self):
        self.update.zero_()
        self.gains.fill_(1.0)

    def step(self, exag, momentum, lr, check):
        self.ops.tsne_pairs(self.y, self.P, self.parts, check)
        self.ops.tsne_update(self.parts, self.y, self.update, self.gains, exag, momentum, lr, check, self.stats)

    def read(self):   # the descent's only device-to-host copy: 16 bytes per check
        kl, gnorm = self.stats.tolist()
        return kl, gnorm


def tsne(x: torch.Tensor, perplexity: float = 30.0, max_iter: int = 1000, early_exaggeration: float = 12.0,
         learning_rate: Union[float, str] = "auto", n_iter_without_progress: int = 300,
         min_grad_norm: float = 1e-7) -> Tuple[torch.Tensor, float]:
    """(Y [N, 2] fp32 on x's device, KL divergence): sklearn's exact t-SNE of the rows of x [N, D].

    The schedule is TSNE(method="exact", init="pca")'s: the PCA init of tsne_pca_init,
    learning_rate "auto" = max(N / early_exaggeration / 4, 50), 250 iterations at the
    early exaggeration with momentum 0.5, the rest at exaggeration 1 with momentum 0.8
    (gains and update restart between the two, as _gradient_descent is called twice),
    and every 50 iterations its two stopping rules on (KL, norm of the gained gradient).
    The exaggeration scales the attractive term; P is never rescaled, and the KL is always
    that of the unscaled P.  The returned KL is the one of the last iteration run, taken
    before that iteration's step, as sklearn's kl_divergence_ is.

    On a device tensor the distances, the perplexity search (fp64), the all-pairs pass and
    the step are HIP kernels (csrc/tsne_ops.hip), bitwise reproducible, with one 16-byte
    read-back per 50 iterations.  On a CPU tensor the same algorithm runs in plain torch
    (fp64 search, fp32 descent)."""
    if x.dim() != 2:
        raise ValueError(f"tsne: x must be [N, D], got {tuple(x.shape)}")
    N = x.shape[0]
    if N > TSNE_MAX_N:
        raise ValueError(f"tsne: N={N} rows; the exact method keeps P [N, N] in fp32, which would exceed 4 GB "
                         f"above N={TSNE_MAX_N}")
    if not 0 < perplexity < N:   # sklearn: perplexity must be less than n_samples
        raise ValueError(f"tsne: perplexity ({perplexity}) must be positive and less than the number of rows ({N})")
    if max_iter < _EXPLORATION_ITERS:
        raise ValueError(f"tsne: max_iter must be at least {_EXPLORATION_ITERS}")
    x = x.detach().float()
    lr = max(N / early_exaggeration / 4.0, 50.0) if learning_rate == "auto" else float(learning_rate)
    run = (_HipDescent if x.is_cuda else _CpuDescent)(x, float(perplexity))
    run.start(tsne_pca_init(x))

    def descend(it, end, exag, momentum, patience):
        """_gradient_descent(it=it, max_iter=end): (KL of the last iteration, its index)."""
        run.reset()
        kl, best, best_it, i = float("nan"), math.inf, it, it
        for i in range(it, end):
            converge = (i + 1) % _N_ITER_CHECK == 0
            check = converge or i == end - 1
            run.step(exag, momentum, lr, check)
            if check:
                kl, gnorm = run.read()
            if converge:
                if kl < best:
                    best, best_it = kl, i
                elif i - best_it > patience:
                    break
                if gnorm <= min_grad_norm:
                    break
        return kl, i

    kl, it = descend(0, _EXPLORATION_ITERS, float(early_exaggeration), 0.5, _EXPLORATION_ITERS)
    if it + 1 < max_iter:
        kl, it = descend(it + 1, max_iter, 1.0, 0.8, n_iter_without_progress)
    return run.y, kl
