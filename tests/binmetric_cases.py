"""Inputs and host-side integer references shared by tests/test_binmetrics_cpu.py and
tests/test_gpu_binmetrics.py (vlp_amd.metrics.BinaryMetricsDevice).

Scores are quantised to 1/16 so that ties are frequent.  Every expected value is a ratio of
integers counted here with python ints, never a value the code under test produced."""
import torch

SIZES = [1, 2, 3, 64, 255, 256, 257, 1000]
KEYS = ("accuracy", "precision", "recall", "f1", "auroc")
BATCHES = (7, 1, 250, 513, 0)


def random_case(n, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + n)
    p = torch.randint(0, 17, (n,), generator=g).float() / 16
    y = torch.randint(0, 2, (n,), generator=g)
    return p, y


def fixed_cases():
    """name -> (probs, labels, the values the issue states for the case)."""
    n = 40
    half = torch.arange(n) % 2
    lo, hi = torch.full((n // 2,), 0.25), torch.full((n // 2,), 0.75)
    return {
        "all_scores_equal": (torch.full((n,), 0.375), half, {"auroc": 0.5}),
        "all_labels_one": (torch.arange(n).float() / n, torch.ones(n, dtype=torch.long),
                           {"auroc": 0.0, "precision": 1.0, "recall": 0.5, "accuracy": 0.5}),
        "all_labels_zero": (torch.arange(n).float() / n, torch.zeros(n, dtype=torch.long),
                            {"auroc": 0.0, "precision": 0.0, "recall": 0.0, "f1": 0.0, "accuracy": 0.5}),
        "all_zero_predicted_zero": (torch.full((n,), 0.25), torch.zeros(n, dtype=torch.long),
                                    {"auroc": 0.0, "precision": 0.0, "recall": 0.0, "f1": 0.0, "accuracy": 1.0}),
        "half_is_positive": (torch.full((n,), 0.5), torch.ones(n, dtype=torch.long),
                             {"accuracy": 1.0, "precision": 1.0, "recall": 1.0, "f1": 1.0, "auroc": 0.0}),
        "perfect": (torch.cat([lo, hi]), torch.cat([torch.zeros(n // 2), torch.ones(n // 2)]).long(),
                    {"auroc": 1.0, "accuracy": 1.0, "f1": 1.0}),
        "inverted": (torch.cat([hi, lo]), torch.cat([torch.zeros(n // 2), torch.ones(n // 2)]).long(),
                     {"auroc": 0.0, "accuracy": 0.0, "precision": 0.0, "recall": 0.0, "f1": 0.0}),
    }


def host_counts(p, y):
    """[tp, fp, fn, tn, wins, ties] as python ints: the threshold cells at p >= 0.5 in fp32 and the
    pair counts over (positive i, negative j), by sorting the negatives (no n x n matrix)."""
    p, y = p.float().cpu(), y.cpu().long()
    pred = p >= 0.5
    cells = [int((pred & (y == 1)).sum()), int((pred & (y == 0)).sum()),
             int((~pred & (y == 1)).sum()), int((~pred & (y == 0)).sum())]
    neg = torch.sort(p[y == 0].double()).values
    pos = p[y == 1].double()
    below = torch.searchsorted(neg, pos, right=False)     # negatives strictly below each positive
    upto = torch.searchsorted(neg, pos, right=True)       # negatives below or equal
    return cells + [int(below.sum()), int((upto - below).sum())]


def brute_u2(p, y):
    """2 #{s_i > s_j} + #{s_i == s_j} over positives i and negatives j: a python double loop."""
    s, t = p.tolist(), y.tolist()
    u2 = 0
    for i in range(len(s)):
        if t[i] != 1:
            continue
        for j in range(len(s)):
            if t[j] == 0:
                u2 += 2 * (s[i] > s[j]) + (s[i] == s[j])
    return u2


def expected(p, y):
    """The five values from host_counts with python's integer division: what both
    binary_metrics and BinaryMetricsDevice must return, bit for bit."""
    tp, fp, fn, tn, wins, ties = host_counts(p, y)
    n = tp + fp + fn + tn
    prec = tp / (tp + fp) if tp + fp else 0.0
    rec = tp / (tp + fn) if tp + fn else 0.0
    return {"accuracy": (tp + tn) / n if n else 0.0, "precision": prec, "recall": rec,
            "f1": 2 * prec * rec / (prec + rec) if prec + rec else 0.0,
            "auroc": (2 * wins + ties) / (2 * (tp + fn) * (fp + tn)) if (tp + fn) and (fp + tn) else 0.0}
