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

logistic_regression, balanced_accuracy and binary_auroc are the pretraining
linear probe (reference LinearProbeCallback.py:72-85: sklearn's
LogisticRegression, balanced_accuracy_score and roc_auc_score) on the features'
device; see their docstrings.

BinaryMetrics / binary_metrics are the baselines' epoch accumulator for accuracy,
precision, recall, F1 and AUROC on the host; BinaryMetricsDevice keeps its state on
the device (csrc/binmetric_ops.hip: integer counts, one 48-byte read per compute()).
Both finish with the host arithmetic of binary_metrics_from_counts.

grouped_binary_counts and subgroup_metrics_from_counts are the test-set evaluation
(reference scripts/test_eval_downstream.py: six sklearn metrics overall and per
dataset, entity, anatomy site, sex and age group): the same six integers for every
group of every level from one pass over the pairs (csrc/groupmetric_ops.hip), and
the script's own one-class rules on the host.
"""
from __future__ import annotations

import functools
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


# ---------------- the linear probe: logistic regression, balanced accuracy, AUROC ----------------
LOGREG_MAX_D = 2048    # kLrMaxD of csrc/logreg_ops.hip
_LOGREG_ROWS = 32      # kLrRows: rows per partial of the device passes
_CG_BUDGET = 32        # HVP + cg_step pairs enqueued per outer iteration
_ARMIJO_C1 = 1e-4
_MIN_STEP = 2.0 ** -30


def logreg_passes_cpu(x: torch.Tensor, y: torch.Tensor, u: torch.Tensor):
    """The GRAD pass in torch fp64 at u [D + 1]: (sum of the losses, sum_i c_i (x_i, 1) [D + 1],
    s [N]) with the overflow-safe forms of csrc/logreg_ops.hip (e = exp(-|t|))."""
    t = x @ u[:-1] + u[-1]
    e = torch.exp(-t.abs())
    inv = 1.0 / (1.0 + e)
    p = torch.where(t >= 0, inv, e * inv)
    c = p - y
    loss = (torch.where(y > 0.5, -t, t).clamp_min(0.0) + torch.log1p(e)).sum()
    return loss, torch.cat([x.T @ c, c.sum()[None]]), e * inv * inv


class _CpuNewton:
    """One outer iteration of the truncated Newton method in torch fp64: the same
    quantities in the same roles as the kernels of csrc/logreg_ops.hip."""

    def __init__(self, x, y, C, tol):
        self.x, self.y = x.double(), y.double()
        self.N, self.D = x.shape
        self.lam, self.tol = 1.0 / (C * self.N), tol
        self.w = torch.zeros(self.D + 1, dtype=torch.float64)
        self.nparts = 1

    def _f(self, u):
        loss, _, _ = logreg_passes_cpu(self.x, self.y, u)
        return float(loss / self.N + 0.5 * self.lam * (u[:-1] ** 2).sum())

    def _pen(self, v):   # lambda (v, 0)
        return torch.cat([self.lam * v[:-1], torch.zeros(1, dtype=torch.float64)])

    def iterate(self, budget):
        loss, gs, s = logreg_passes_cpu(self.x, self.y, self.w)
        g = gs / self.N + self._pen(self.w)
        f = float(loss / self.N + 0.5 * self.lam * (self.w[:-1] ** 2).sum())
        ginf, gn = float(g.abs().max()), float(g.norm())
        d, r, q = torch.zeros_like(g), -g, -g.clone()
        rs, cgtol, steps = float(g @ g), min(0.5, math.sqrt(gn)) * gn, 0
        done = ginf <= self.tol or rs == 0.0
        for _ in range(budget):
            if done:
                break
            c = s * (self.x @ q[:-1] + q[-1])
            hq = torch.cat([self.x.T @ c, c.sum()[None]]) / self.N + self._pen(q)
            curv = float(q @ hq)
            if not curv > 0.0:
                break
            alpha = rs / curv
            d, r = d + alpha * q, r - alpha * hq
            rs_new = float(r @ r)
            q, rs, steps = r + (rs_new / rs) * q, rs_new, steps + 1
            done = math.sqrt(rs) <= cgtol
        self.d, self.status = d, [f, ginf, float(g @ d), float("nan"), float(steps)]
        self.trial(1.0)

    def trial(self, t):
        self.wt = self.w + t * self.d
        self.status[3] = self._f(self.wt)

    def read(self):
        return tuple(self.status)

    def accept(self):
        self.w = self.wt


class _HipNewton:
    def __init__(self, x, y, C, tol):
        from . import ops
        self.ops, self.x, self.y, self.C, self.tol = ops, x, y.double().contiguous(), C, tol
        self.N, self.D = x.shape
        self.nparts = ops.logreg_nparts(self.N)
        z = functools.partial(torch.zeros, dtype=torch.float64, device=x.device)
        self.w, self.wt, self.s = z(self.D + 1), z(self.D + 1), z(self.N)
        self.parts, self.vec, self.state = z(self.nparts, self.D + 2), z(4, self.D + 1), z(ops.LOGREG_STATE)

    def iterate(self, budget):
        o, N, D = self.ops, self.N, self.D
        o.logreg_pass(o.LOGREG_GRAD, self.x, self.y, self.w, s=self.s, parts=self.parts)
        o.logreg_newton_begin(N, D, self.C, self.parts, self.w, self.tol, self.vec, self.state)
        q = self.vec[3]
        for _ in range(budget):   # the pairs past the done flag return at entry
            o.logreg_pass(o.LOGREG_HVP, self.x, None, q, s=self.s, parts=self.parts, state=self.state)
            o.logreg_cg_step(N, D, self.C, self.parts, self.vec, self.state)
        self.trial(1.0)

    def trial(self, t):
        o = self.ops
        o.logreg_trial(self.N, self.D, self.C, self.w, t, self.vec, self.wt, self.state)
        o.logreg_pass(o.LOGREG_LOSS, self.x, self.y, self.wt, parts=self.parts)
        o.logreg_trial_loss(self.N, self.D, self.parts, self.state)

    def read(self):   # the fit's only device-to-host copy: 40 bytes per outer iteration
        return tuple(self.state[:self.ops.LOGREG_STATUS].tolist())

    def accept(self):
        self.w, self.wt = self.wt, self.w


class LogisticRegressionFit:
    """What logistic_regression returns: coef_ [D] fp64 and intercept_ (0-d fp64) on the
    features' device, n_iter_ (outer iterations taken), converged_ (the gradient's
    largest entry was at most tol at coef_, intercept_)."""

    def __init__(self, wb: torch.Tensor, n_iter: int, converged: bool, loss: float):
        self._wb = wb
        self.coef_, self.intercept_ = wb[:-1], wb[-1]
        self.n_iter_, self.converged_, self.loss_ = n_iter, converged, loss

    def decision_function(self, x: torch.Tensor) -> torch.Tensor:
        """fp64 [M]: x_i . coef_ + intercept_ for the rows of x [M, D], on x's device."""
        if x.dim() != 2 or x.shape[1] != self.coef_.shape[0]:
            raise ValueError(f"decision_function: x must be [M, {self.coef_.shape[0]}], got {tuple(x.shape)}")
        if not x.is_cuda:
            return x.double() @ self.coef_.to(x.device) + self.intercept_.to(x.device)
        from . import ops
        x = _logreg_features(x)
        z = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
        if x.shape[0]:
            ops.logreg_pass(ops.LOGREG_SCORES, x, None, self._wb.to(x.device), z=z)
        return z

    def predict(self, x: torch.Tensor) -> torch.Tensor:
        """int64 [M]: class 1 where the score is > 0 (sklearn's rule), else 0."""
        return (self.decision_function(x) > 0).long()


def _logreg_features(x: torch.Tensor) -> torch.Tensor:
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    return x if x.stride(1) == 1 and x.stride(0) >= x.shape[1] else x.contiguous()


def logistic_regression(x: torch.Tensor, y: torch.Tensor, C: float = 1.0, max_iter: int = 100,
                        tol: float = 1e-8) -> LogisticRegressionFit:
    """sklearn's binary LogisticRegression(penalty="l2", C=C, fit_intercept=True) on x [N, D]
    (taken as fp32, the encoders' output) and y [N] in {0, 1}: the minimiser of

        f(w, b) = (1/N) sum_i [softplus(z_i) - y_i z_i] + |w|^2 / (2 C N),   z_i = x_i . w + b

    (sklearn >= 1.4's scaling; the intercept is not penalised), by a truncated Newton method
    in fp64 from w = 0: each outer iteration takes the direction d of at most _CG_BUDGET
    conjugate-gradient steps on H d = -g (stopped at |r| <= min(0.5, sqrt|g|) |g|), tries
    w + d, and halves the step while the Armijo test f(w + t d) <= f(w) + 1e-4 t g.d fails
    (beyond the rounding of the two sums).  It stops when the largest entry of the gradient is
    at most tol (converged_) or after max_iter outer iterations.  Unlike sklearn's L-BFGS,
    whose tol=1e-4 ends the descent far from the optimum on separable features, the result does
    not depend on the solver's path.

    On a device tensor every pass over x and every vector update is a HIP kernel
    (csrc/logreg_ops.hip), bitwise reproducible; the host reads 40 bytes per outer iteration,
    after one 16-byte read of the two class counts before the first launch.  On a CPU tensor
    the same driver runs on a torch-fp64 restatement of the passes.  ValueError, before any
    launch: y with one class only (as sklearn) or with values outside {0, 1}."""
    if x.dim() != 2 or y.dim() != 1 or y.shape[0] != x.shape[0]:
        raise ValueError(f"logistic_regression: x [N, D] and y [N], got {tuple(x.shape)} and {tuple(y.shape)}")
    N, D = x.shape
    if N < 1 or not 1 <= D <= LOGREG_MAX_D:
        raise ValueError(f"logistic_regression: N={N}, D={D}; at least one row and 1 to {LOGREG_MAX_D} columns")
    if not C > 0 or not tol > 0 or max_iter < 1:
        raise ValueError(f"logistic_regression: C={C}, tol={tol} must be positive and max_iter={max_iter} >= 1")
    y = y.detach().to(x.device)
    n1, n0 = torch.stack([(y == 1).sum(), (y == 0).sum()]).tolist()
    if n0 + n1 != N:
        raise ValueError("logistic_regression: the labels must be 0 or 1")
    if n0 == 0 or n1 == 0:
        raise ValueError("logistic_regression: the labels hold one class only, the fit needs both (as sklearn's)")
    x = _logreg_features(x)
    run = (_HipNewton if x.is_cuda else _CpuNewton)(x, y, float(C), float(tol))
    # the two loss sums of the Armijo test each carry at most (rows per partial + partials + 8)
    # roundings of relative size 2^-53: a difference below that is not a failed test
    noise = 2.0 * (_LOGREG_ROWS + run.nparts + 8) * 2.0 ** -53
    n_iter, converged, f = 0, False, float("nan")
    for _ in range(max_iter):
        run.iterate(_CG_BUDGET)
        f, ginf, gd, ft, _ = run.read()
        if ginf <= tol:
            converged = True
            break
        t = 1.0
        while not ft <= f + _ARMIJO_C1 * t * gd + noise * abs(f) and t > _MIN_STEP:
            t *= 0.5
            run.trial(t)
            ft = run.read()[3]
        run.accept()
        n_iter, f = n_iter + 1, ft
    return LogisticRegressionFit(run.w, n_iter, converged, f)


def balanced_accuracy(y: torch.Tensor, pred: torch.Tensor) -> float:
    """sklearn.metrics.balanced_accuracy_score for labels in {0, 1}: the mean of the two
    recalls, counted on the tensors' device (one 8-byte read).  The recall of a class that y
    lacks is 0, BinaryMetrics' zero-division rule, so a one-class y gives half the recall of
    the class present (sklearn warns and averages over the classes present instead)."""
    y, pred = y.reshape(-1), pred.reshape(-1).to(y.device)
    pos, neg = y == 1, y == 0
    n1, n0 = pos.sum().double(), neg.sum().double()
    r1 = ((pred == 1) & pos).sum().double() / n1.clamp_min(1.0)
    r0 = ((pred == 0) & neg).sum().double() / n0.clamp_min(1.0)
    return float(0.5 * (r1 + r0))


def binary_auroc(y: torch.Tensor, score: torch.Tensor) -> float:
    """sklearn.metrics.roc_auc_score for labels in {0, 1}: the Mann-Whitney statistic with
    tie-averaged ranks, (sum of the positives' ranks - n1 (n1 + 1) / 2) / (n1 n0), in fp64 on
    the tensors' device (torch.sort is the only plumbing; one 8-byte read).  0.0 for a one-class
    y, as BinaryMetrics (sklearn raises)."""
    y, score = y.reshape(-1), score.reshape(-1).double().to(y.device)
    pos = y == 1
    n1, n0 = pos.sum().double(), (y == 0).sum().double()
    vals, order = torch.sort(score)
    _, inverse, counts = torch.unique_consecutive(vals, return_inverse=True, return_counts=True)
    first = torch.cumsum(counts, 0) - counts                      # 0-based start of each tie group
    ranks = (first.double() + 0.5 * (counts.double() + 1.0))[inverse]   # 1-based average rank
    u = (ranks * pos[order].double()).sum() - n1 * (n1 + 1.0) / 2.0
    auc = torch.where((n1 > 0) & (n0 > 0), u / (n1 * n0).clamp_min(1.0), torch.zeros_like(u))
    return float(auc)


# ---------------- the baselines' binary classification metrics ----------------
BINMETRIC_MAX_N = 1 << 18   # kBmMaxN of csrc/binmetric_ops.hip: the ceiling of the O(n^2) pair count


def binary_metrics_from_counts(tp, fp, fn, tn, u2):
    """The five values of torchmetrics' Binary{Accuracy, Precision, Recall, F1Score, AUROC} from the
    confusion counts and u2 = 2 #{s_i > s_j} + #{s_i == s_j} over the pairs (positive i, negative
    j), twice the Mann-Whitney statistic with tie-averaged ranks: AUROC = u2 / (2 n1 n0).
    Precision, recall and F1 are 0.0 on a zero denominator (torchmetrics' zero_division default),
    the AUROC is 0.0 when a class is absent.  Every quotient is one fp64 division of exact
    integers (u2 may come as a float that holds an integer), so two callers that counted the same
    samples return the same bits."""
    n = tp + fp + fn + tn
    acc = (tp + tn) / n if n else 0.0
    prec = tp / (tp + fp) if tp + fp else 0.0
    rec = tp / (tp + fn) if tp + fn else 0.0
    f1 = 2 * prec * rec / (prec + rec) if prec + rec else 0.0
    npos, nneg = tp + fn, fp + tn
    auroc = float(u2 / (2 * npos * nneg)) if npos and nneg else 0.0
    return {"accuracy": acc, "precision": prec, "recall": rec, "f1": f1, "auroc": auroc}


class BinaryMetrics:
    """Epoch accumulator for torchmetrics' Binary{Accuracy, Precision, Recall,
    F1Score, AUROC} (threshold 0.5; precision / recall / F1 are 0 when their
    denominator is 0, as torchmetrics' zero_division default)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self._p, self._y = [], []

    def update(self, probs, labels):
        self._p.append(probs.detach().float().reshape(-1).cpu())
        self._y.append(labels.detach().reshape(-1).cpu().long())

    def compute(self):
        if not self._p:
            return {}
        p, y = torch.cat(self._p), torch.cat(self._y)
        return binary_metrics(p, y)


def binary_metrics(p: torch.Tensor, y: torch.Tensor):
    pred = (p >= 0.5).long()
    tp = int(((pred == 1) & (y == 1)).sum())
    fp = int(((pred == 1) & (y == 0)).sum())
    fn = int(((pred == 0) & (y == 1)).sum())
    tn = int(((pred == 0) & (y == 0)).sum())
    npos, nneg = tp + fn, fp + tn
    u2 = 0
    if npos and nneg:
        # Mann-Whitney U with average ranks for ties = the area under the ROC curve
        order = torch.argsort(p.double())
        ps = p.double()[order]
        ranks = torch.empty_like(ps)
        i, n = 0, ps.numel()
        while i < n:
            j = i
            while j + 1 < n and ps[j + 1] == ps[i]:
                j += 1
            ranks[i:j + 1] = 0.5 * (i + j) + 1.0
            i = j + 1
        r = torch.empty_like(ranks)
        r[order] = ranks
        u2 = 2.0 * float(r[y == 1].sum() - npos * (npos + 1) / 2)   # ranks are half-integers: exact
    return binary_metrics_from_counts(tp, fp, fn, tn, u2)


def binary_pair_counts_cpu(scores: torch.Tensor, labels: torch.Tensor) -> Tuple[int, int]:
    """(wins, ties) of csrc/binmetric_ops.hip's pair count in plain torch: over i with
    labels[i] == 1 and j with labels[j] == 0, #{scores[i] > scores[j]} and
    #{scores[i] == scores[j]}, in row chunks of the positives."""
    pos, neg = scores[labels == 1], scores[labels == 0]
    wins = ties = 0
    rows = max(1, (1 << 22) // max(1, neg.numel()))
    for r in range(0, pos.numel(), rows):
        p = pos[r:r + rows, None]
        wins += int((p > neg[None, :]).sum())
        ties += int((p == neg[None, :]).sum())
    return wins, ties


class BinaryMetricsDevice:
    """BinaryMetrics (above) with its state on the scores'
    device: reset(), update(probs, labels), compute() -> the same five keys, {} when empty.

    The scores (fp32) and labels (uint8) of an epoch sit in two buffers that double through torch
    when full; the host knows the fill count from the batch sizes.  update() is one launch
    (vlp_binmetric_append) that also adds the batch's tp, fp, fn, tn at probs >= 0.5 into an
    int64[4]; nothing is read back.  compute() counts the AUROC's pairs without a sort
    (vlp_binmetric_pairs, O(n^2) comparisons, meant for n <= 2^18 = BINMETRIC_MAX_N; beyond it the
    AUROC comes from binary_auroc on the device), folds, and reads 48 bytes -- tp, fp, fn, tn,
    wins, ties -- the accumulator's only device-to-host copy; binary_metrics_from_counts finishes
    on the host, as it does for binary_metrics, so the two paths return the same bits.  The device
    does no floating-point arithmetic.  reset() zeroes the counters and the fill count and
    allocates nothing.

    Labels are 0 or 1 (int64, int32, uint8 or bool; any other value is counted in no cell and no
    pair).  Scores are probabilities (sigmoid outputs), hence finite: a NaN is out of contract.
    On CPU tensors the same integer counts come from plain torch (binary_pair_counts_cpu)."""

    def __init__(self, capacity: int = 4096):
        self._capacity = max(1, int(capacity))
        self._scores = self._labels = self._counts = None
        self._n = 0

    def __len__(self):
        return self._n

    def reset(self):
        self._n = 0
        if self._counts is not None:
            self._counts.zero_()

    def _reserve(self, need: int, device: torch.device):
        if self._scores is not None and self._scores.device != device:
            if self._n:
                raise ValueError(f"BinaryMetricsDevice: update on {device} after rows on {self._scores.device}")
            self._scores = None
        if self._scores is None:
            cap = max(self._capacity, need)
            self._scores = torch.empty(cap, dtype=torch.float32, device=device)
            self._labels = torch.empty(cap, dtype=torch.uint8, device=device)
            self._counts = torch.zeros(4, dtype=torch.int64, device=device)
        elif need > self._scores.numel():
            cap = max(2 * self._scores.numel(), need)
            for name in ("_scores", "_labels"):
                old = getattr(self, name)
                new = torch.empty(cap, dtype=old.dtype, device=device)
                new[:self._n].copy_(old[:self._n])
                setattr(self, name, new)

    def update(self, probs: torch.Tensor, labels: torch.Tensor):
        p = probs.detach().reshape(-1)
        if p.dtype != torch.float32:
            p = p.float()
        y = labels.detach().reshape(-1).to(p.device, non_blocking=True)
        if y.dtype not in (torch.int64, torch.int32, torch.uint8, torch.bool):
            y = y.long()
        n = p.numel()
        if y.numel() != n:
            raise ValueError(f"BinaryMetricsDevice: {n} probabilities but {y.numel()} labels")
        if n == 0:
            return
        self._reserve(self._n + n, p.device)
        if p.is_cuda:
            from . import ops
            ops.binmetric_append(p.contiguous(), y.contiguous(), self._scores, self._labels, self._n, self._counts)
        else:
            y8 = torch.where(y == 1, 1, torch.where(y == 0, 0, 2)).to(torch.uint8)
            self._scores[self._n:self._n + n] = p
            self._labels[self._n:self._n + n] = y8
            pred = p >= 0.5
            self._counts += torch.stack([(pred & (y8 == 1)).sum(), (pred & (y8 == 0)).sum(),
                                         (~pred & (y8 == 1)).sum(), (~pred & (y8 == 0)).sum()])
        self._n += n

    def counts(self) -> List[int]:
        """[tp, fp, fn, tn, wins, ties] over the rows held (one 48-byte read on the device)."""
        n = self._n
        if n == 0:
            return [0] * 6
        s, y = self._scores[:n], self._labels[:n]
        if not s.is_cuda:
            return self._counts.tolist() + list(binary_pair_counts_cpu(s, y))
        from . import ops
        return ops.binmetric_counts(n, self._scores, self._labels, self._counts).tolist()

    def compute(self) -> dict:
        n = self._n
        if n == 0:
            return {}
        if self._scores.is_cuda and n > BINMETRIC_MAX_N:   # past the pair count's ceiling: the sort-based AUROC
            out = binary_metrics_from_counts(*self._counts.tolist(), 0)
            out["auroc"] = binary_auroc(self._labels[:n], self._scores[:n])
            return out
        tp, fp, fn, tn, wins, ties = self.counts()
        return binary_metrics_from_counts(tp, fp, fn, tn, 2 * wins + ties)


# ---------------- the test-set evaluation's per-subgroup metrics ----------------
NO_GROUP = 255   # kGmMaxGroups of csrc/groupmetric_ops.hip: the code of a row in no group of a level
SUBGROUP_METRICS = ("accuracy", "balanced_accuracy", "roc_auc", "precision", "recall", "f1_score")


def _labels_u8(labels: torch.Tensor) -> torch.Tensor:
    """vlp_binmetric_append's encoding: 1 where the label is 1, 0 where it is 0, else 2."""
    if labels.dtype == torch.uint8:
        return labels
    one, two = torch.ones_like(labels), torch.full_like(labels, 2)
    return torch.where(labels == 1, one, torch.where(labels == 0, torch.zeros_like(labels), two)).to(torch.uint8)


def grouped_binary_counts(scores: torch.Tensor, labels: torch.Tensor, codes: torch.Tensor,
                          n_groups: Sequence[int]) -> torch.Tensor:
    """int64 [cells, 6] on the scores' device: tp, fp, fn, tn, wins, ties -- BinaryMetricsDevice's
    six integers -- of every group of every level.  scores [n] (taken as fp32), labels [n] (0 or 1;
    any other value, and 2 in a uint8 tensor, is counted nowhere), codes [L, n] uint8 with row i's
    group in level l (0 .. n_groups[l] - 1, or NO_GROUP = 255 for none), 1 <= L <= 8 levels of at
    most 255 groups.  Level l's group g is row sum(n_groups[:l]) + g of the result; a declared
    group that no row carries is a row of zeros.

    On device tensors one pass over the pairs counts all levels (csrc/groupmetric_ops.hip: two
    launches, integers only, bitwise reproducible) and nothing is read back -- the caller's
    .tolist() is the one read of cells x 48 bytes.  On CPU tensors every level and group takes its
    boolean mask, the four threshold counts and binary_pair_counts_cpu, in plain torch: the
    reference the device is held to, bit for bit.  ValueError before any launch for L outside
    1 .. 8, a group count outside 1 .. 255 or lengths that do not match."""
    from . import ops
    n, L, cell_base = ops.groupmetric_check(scores, labels, codes, n_groups)
    if codes.dtype != torch.uint8:
        raise TypeError(f"grouped_binary_counts: codes must be uint8, got {codes.dtype}")
    s = scores.detach()
    if s.dtype != torch.float32:
        s = s.float()
    y = _labels_u8(labels.detach().to(s.device))
    codes = codes.to(s.device)
    if s.is_cuda:
        return ops.groupmetric_counts(s.contiguous(), y.contiguous(), codes.contiguous(), n_groups)
    out = torch.zeros(cell_base[-1], 6, dtype=torch.int64)
    pred, pos, neg = s >= 0.5, y == 1, y == 0
    for l in range(L):
        for g in range(cell_base[l + 1] - cell_base[l]):
            m = codes[l] == g
            wins, ties = binary_pair_counts_cpu(s[m], y[m])
            out[cell_base[l] + g] = torch.tensor([int((m & pred & pos).sum()), int((m & pred & neg).sum()),
                                                  int((m & ~pred & pos).sum()), int((m & ~pred & neg).sum()),
                                                  wins, ties])
    return out


def subgroup_metrics_from_counts(tp, fp, fn, tn, u2) -> dict:
    """The six values of the reference's calculate_metrics (scripts/test_eval_downstream.py:244-278:
    sklearn's accuracy_score, balanced_accuracy_score, roc_auc_score, precision_score, recall_score,
    f1_score at a 0.5 threshold) from the confusion counts and u2 = 2 wins + ties, in the script's
    key order.  These are the script's rules, not binary_metrics_from_counts':
      accuracy           (tp + tn) / n
      balanced_accuracy  the mean of the recalls of the classes present in the labels (sklearn drops
                         an absent class), so a one-class group gives that class's recall
      with fewer than two classes present roc_auc, precision, recall and f1_score are NaN
      roc_auc            u2 / (2 n1 n0)
      precision          tp / (tp + fp), 0.0 when nothing is predicted positive (sklearn's zero_division)
      recall             tp / (tp + fn)
      f1_score           2 tp / (2 tp + fp + fn), 0.0 on a zero denominator
    Every quotient is one fp64 division of exact integers.  An empty group is NaN throughout."""
    nan = float("nan")
    n1, n0 = tp + fn, fp + tn
    n = n1 + n0
    if n == 0:
        return dict.fromkeys(SUBGROUP_METRICS, nan)
    out = {"accuracy": (tp + tn) / n}
    if n1 and n0:
        out["balanced_accuracy"] = (tp / n1 + tn / n0) / 2
        out["roc_auc"] = float(u2 / (2 * n1 * n0))
        out["precision"] = tp / (tp + fp) if tp + fp else 0.0
        out["recall"] = tp / n1
        out["f1_score"] = 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0
    else:
        out["balanced_accuracy"] = tp / n1 if n1 else tn / n0
        out.update(roc_auc=nan, precision=nan, recall=nan, f1_score=nan)
    return out
