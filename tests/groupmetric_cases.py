"""Inputs and an independent brute force shared by tests/test_groupmetrics_cpu.py and
tests/test_gpu_groupmetrics.py (vlp_amd.metrics.grouped_binary_counts).

brute_counts restates the contract with explicit Python loops over rows and pairs -- no masks,
no torch arithmetic -- so it shares nothing with the CPU path it checks."""
import torch

NO_GROUP = 255
QUANT = (0.125, 0.5, 0.625, 0.875)   # four fp32-exact scores, 0.5 (the threshold) among them: ties are frequent


def adversarial_case():
    """n = 40, three levels:
      level 0, 3 groups declared: group 2 is carried by no row (an empty declared group);
      level 1, 4 groups: group 3 holds a single row, group 1 holds positives only (one class);
      level 2, 2 groups: every fourth row carries 255 (in no group);
    rows 5, 17 and 29 have label 2 (counted nowhere), and rows with 255 appear in levels 0 and 1 too.
    Scores take four values."""
    n = 40
    g = torch.Generator().manual_seed(40)
    scores = torch.tensor(QUANT)[torch.randint(0, 4, (n,), generator=g)]
    labels = torch.randint(0, 2, (n,), generator=g).to(torch.uint8)
    l0 = torch.randint(0, 2, (n,), generator=g)
    l1 = torch.randint(0, 3, (n,), generator=g)
    l1[labels == 0] = torch.where(l1[labels == 0] == 1, 0, l1[labels == 0])   # group 1: positives only
    l1[7] = 3                                                                  # group 3: one row
    l2 = torch.randint(0, 2, (n,), generator=g)
    l2[::4] = NO_GROUP
    l0[3], l1[11] = NO_GROUP, NO_GROUP
    labels[[5, 17, 29]] = 2
    labels[2], l1[2] = 1, 1          # group 1 is not empty
    codes = torch.stack([l0, l1, l2]).to(torch.uint8)
    return scores, labels, codes, [3, 4, 2]


def random_case(n, n_groups, seed=0, quantised=True, no_group_rate=0.1, skip_rate=0.05):
    """scores [n] fp32, labels [n] uint8 (a few 2s), codes [L, n] uint8 (a few 255s)."""
    g = torch.Generator().manual_seed(1000 * seed + n + 7 * len(n_groups))
    if quantised:
        scores = torch.randint(0, 17, (n,), generator=g).float() / 16.0
    else:
        scores = torch.rand(n, generator=g)
    labels = torch.randint(0, 2, (n,), generator=g).to(torch.uint8)
    labels[torch.rand(n, generator=g) < skip_rate] = 2
    rows = []
    for G in n_groups:
        c = torch.randint(0, G, (n,), generator=g)
        c[torch.rand(n, generator=g) < no_group_rate] = NO_GROUP
        rows.append(c)
    return scores, labels, torch.stack(rows).to(torch.uint8), list(n_groups)


def brute_counts(scores, labels, codes, n_groups):
    """[[tp, fp, fn, tn, wins, ties] per cell] with Python loops over the rows and the pairs."""
    s, y, c = scores.tolist(), labels.tolist(), codes.tolist()
    n, out = len(s), []
    for l, G in enumerate(n_groups):
        for grp in range(G):
            cell = [0] * 6
            rows = [i for i in range(n) if c[l][i] == grp]
            for i in rows:
                if y[i] == 1:
                    cell[0 if s[i] >= 0.5 else 2] += 1
                elif y[i] == 0:
                    cell[1 if s[i] >= 0.5 else 3] += 1
            for i in rows:
                if y[i] != 1:
                    continue
                for j in rows:
                    if y[j] == 0:
                        cell[4] += s[i] > s[j]
                        cell[5] += s[i] == s[j]
            out.append(cell)
    return out
