"""References for the epoch-end retrieval path (vlp_row_topk, ops.sim_topk and
the module's precision@k / recall@k), with no GPU dependency.

The kernel's contract is "descending, ties to the lower index"; `topk_stable`
states it with one stable sort.  The metric references are written from the
reference's counting (VisionLanguageModule.py:364-439) and that rule, not from
oracle/clip.py, which selects with torch.topk and so has no defined tie order.

`half_unit_rows` gives embeddings whose every similarity is exact in fp32 on any
GEMM route, so top-k lists over them can be compared with `torch.equal`.
"""
import torch
import torch.nn.functional as F

NEG_INF = float("-inf")


def topk_stable(x, K):
    """x [R, N] (CPU) -> (vals [R, K], idx [R, K] int64): the first min(K, N)
    entries of a stable descending sort of each row, padded with -inf / -1."""
    assert x.dim() == 2 and not x.is_cuda
    R, N = x.shape
    s = torch.sort(x, dim=1, descending=True, stable=True)
    k = min(K, N)
    vals = torch.full((R, K), NEG_INF, dtype=x.dtype)
    idx = torch.full((R, K), -1, dtype=torch.int64)
    vals[:, :k] = s.values[:, :k]
    idx[:, :k] = s.indices[:, :k]
    return vals, idx


def sim_fp64(a, b):
    """fp64 similarity (on the CPU) of rows that are already normalised."""
    return a.detach().double().cpu() @ b.detach().double().cpu().T


def _normalised64(x):
    return F.normalize(x.detach().float()).double().cpu()


def precision_at_k_ref(e, labels, ks):
    """:364-400 with the kernel's tie rule.  The rows are normalised in fp32 as the
    module does, the similarity is fp64, the selection is `topk_stable`, entry 0
    is dropped whatever it is (with duplicate rows it is the lowest-index copy,
    not always the query) and the kept entries are counted as in the reference.
    The last step, (correct.float() / k).mean(), is an fp32 sum whose bits depend
    on the reduction order; it runs on the device `labels` lives on, over a
    vector whose every entry was fixed on the CPU, so a comparison with the
    module on that device is an equality."""
    assert all(k + 1 <= e.shape[0] for k in ks)
    n = _normalised64(e)
    _, top = topk_stable(n @ n.T, max(ks) + 1)
    lab = labels.detach().cpu()
    out = {}
    for k in ks:
        correct = (lab.unsqueeze(1) == lab[top[:, 1:k + 1]]).sum(dim=1)
        out[k] = (correct.to(labels.device).float() / k).mean().item()
    return out


def recall_at_k_ref(i, t, ks):
    """:402-439 with the kernel's tie rule: image r counts for recall@k when text r
    is among the first k entries of the stable descending order of row r."""
    _, top = topk_stable(_normalised64(i) @ _normalised64(t).T, max(ks))
    tgt = torch.arange(i.shape[0]).unsqueeze(1)
    return {k: (top[:, :k] == tgt).any(dim=1).sum().item() / i.shape[0] for k in ks}


def half_unit_rows(n, E, seed, dup=0):
    """[n, E] fp32 rows with exactly four non-zero entries in {-1, +1}: the norm
    is exactly 2, a normalised entry exactly +-0.5 or 0 and every dot product of
    two normalised rows a multiple of 0.25 in [-1, 1], exact in fp32 in any
    summation order.  `dup` times a row is copied over a later one, so the set
    holds exact duplicates (possibly chained)."""
    assert E >= 4 and n >= 2
    g = torch.Generator().manual_seed(seed)
    cols = torch.rand(n, E, generator=g).argsort(dim=1)[:, :4]
    sign = torch.randint(0, 2, (n, 4), generator=g).float() * 2 - 1
    x = torch.zeros(n, E).scatter_(1, cols, sign)
    for _ in range(dup):
        src = int(torch.randint(0, n - 1, (1,), generator=g))
        dst = int(torch.randint(src + 1, n, (1,), generator=g))
        x[dst] = x[src]
    h2 = 2 * F.normalize(x)
    assert torch.equal(h2, torch.round(h2)) and torch.equal(h2.abs().sum(dim=1), torch.full((n,), 4.0))
    return x


def random_unit_rows(n, E, seed):
    """[n, E] fp32 rows of a seeded normal draw, normalised in fp32."""
    return F.normalize(torch.randn(n, E, generator=torch.Generator().manual_seed(seed)))


# (N, E) of the sim_topk cases, with Q = 257 queries: E = 30 takes the pad-to-4
# branch; N = 37 and 1001 make the tile's row stride differ from N
SIM_Q = 257
SIM_CASES = [(37, 128), (1001, 128), (3000, 128), (37, 30), (1001, 30), (3000, 30)]


def exact_pair(N, E):
    """Normalised half-unit queries [257, E] and keys [N, E] with duplicates in both."""
    return (F.normalize(half_unit_rows(SIM_Q, E, 100 + N + E, dup=SIM_Q // 8)),
            F.normalize(half_unit_rows(N, E, 200 + N + E, dup=N // 4)))


def random_pair(N, E):
    return random_unit_rows(SIM_Q, E, 40 + N), random_unit_rows(N, E, 41 + E)


def metric_case(n=300, E=32, seed=5):
    """Half-unit image and text embeddings and labels for the module metrics:
    duplicate images (under equal and under different labels), captions that are
    their image's copy for about half the rows (so recall lies inside (0, 1)) and
    duplicate captions."""
    g = torch.Generator().manual_seed(seed)
    img = half_unit_rows(n, E, seed, dup=n // 8)
    lab = torch.randint(0, 3, (n,), generator=g)
    txt = img.clone()
    other = half_unit_rows(n, E, seed + 1)
    swap = torch.rand(n, generator=g) < 0.5
    txt[swap] = other[swap]
    for _ in range(n // 8):
        src = int(torch.randint(0, n - 1, (1,), generator=g))
        dst = int(torch.randint(src + 1, n, (1,), generator=g))
        txt[dst] = txt[src]
    return img, txt, lab


def sim_bound(q, k, c):
    """Per-element bound of an fp32 dot product of depth E against fp64:
    c * E * 2^-23 * sum_d |q_d k_d| (c = 1 is twice the worst case gamma_E)."""
    return c * q.shape[1] * 2.0 ** -23 * (q.double().abs() @ k.double().abs().T)


def tied_boundary_share(S, K):
    """Share of rows of S whose K-th and (K+1)-th entries in descending order are
    equal: the rows whose top-K list is decided by the tie rule."""
    v = torch.sort(S, dim=1, descending=True, stable=True).values
    return (v[:, K - 1] == v[:, K]).double().mean().item()


def topk_bound_check(vals, idx, S, b):
    """The gate of the random sim_topk case.  vals / idx [Q, K] are a top-K of an
    fp32 similarity whose fp64 value is S [Q, N], b [Q, N] the per-element bound
    of that fp32 dot product.  Asserts, for every row and with no element left
    out: K distinct in-range indices; values non-increasing; each value within
    the bound of its own S entry; every key not returned at most the K-th value
    plus its own bound plus the K-th entry's.  Returns the worst |err| / b."""
    vals, idx = vals.detach().double().cpu(), idx.detach().cpu()
    Q, K = idx.shape
    N = S.shape[1]
    assert K <= N and vals.shape == idx.shape and S.shape == b.shape == (Q, N)
    assert bool(((idx >= 0) & (idx < N)).all()), "index out of range"
    assert bool((idx.sort(dim=1).values.diff(dim=1) > 0).all()), "an index is returned twice"
    assert bool((vals.diff(dim=1) <= 0).all()), "values not non-increasing"
    err = (vals - S.gather(1, idx)).abs()
    bsel = b.gather(1, idx)
    worst = (err / bsel).max().item()
    assert bool((err <= bsel).all()), f"a returned value is off by {worst:.3f} of its bound"
    rest = torch.ones(Q, N, dtype=torch.bool).scatter_(1, idx, False)
    limit = vals[:, K - 1:K] + bsel[:, K - 1:K] + b
    over = rest & ~(S <= limit)
    assert not bool(over.any()), f"{int(over.sum())} keys left out that rank above the K-th entry"
    return worst
