"""Clustering metrics over cached feature rows.

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
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

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
