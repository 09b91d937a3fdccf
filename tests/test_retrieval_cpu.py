"""CPU: the retrieval references of tests/retrieval_ref.py against brute force and
hand-counted answers, and the module's fallback branch (off the GPU, or
max(ks) + 1 > 16) against them on inputs full of exact ties.

Tied inputs.  `metric_case()` holds 300 rows of `half_unit_rows` with E = 32:
every similarity is a multiple of 0.25, so 100 % of the rows of the image-image
similarity have their 16th and 17th best entries equal, and 99.7 % of the rows
of the image-text similarity (printed by `test_exact_inputs_are_tied`, with the
shares of the sim_topk inputs).  Almost every top-k list over them is decided
by the tie rule.

While the fallback selected with torch.topk, `test_module_fallback_by_hand` and
`test_fallback_matches_refs_on_ties` failed on the CPU: the hand case gave
precision@1 = 0.4 for the counted 0.6, and on `metric_case()` precision@1 was
0.45 against 0.48, precision@15 0.3422 against 0.3376 and recall@10 0.4233
against 0.4333.  The fallback now selects with a stable descending sort.
"""
import pytest
import torch

from tests.retrieval_ref import (SIM_CASES, exact_pair, half_unit_rows, metric_case, precision_at_k_ref, random_pair,
                                 recall_at_k_ref, sim_bound, sim_fp64, tied_boundary_share, topk_bound_check,
                                 topk_stable)
from tests.test_gpu_linear_routes import C_F32

INF = float("inf")


def _module():
    from src.models.pretrain.VisionLanguageModule import VisionLanguageModule
    return VisionLanguageModule, VisionLanguageModule.__new__(VisionLanguageModule)


def _brute(x, K):
    vals, idx = [], []
    for row in x.tolist():
        order = sorted((-v, i) for i, v in enumerate(row))[:K]
        vals.append([row[i] for _, i in order] + [-INF] * (K - len(order)))
        idx.append([i for _, i in order] + [-1] * (K - len(order)))
    return torch.tensor(vals, dtype=x.dtype).reshape(len(vals), K), torch.tensor(idx).reshape(len(idx), K)


@pytest.mark.parametrize("N,K", [(1, 1), (1, 16), (5, 16), (16, 16), (17, 16), (40, 3), (200, 16)])
def test_topk_stable_vs_brute_force(N, K):
    g = torch.Generator().manual_seed(N * 31 + K)
    levels = torch.tensor([-INF, -1.5, -0.0, 0.0, 0.25, 0.25, 1.0, INF])
    x = levels[torch.randint(0, 8, (6, N), generator=g)]
    x[1] = 0.25                  # one value: indices 0..K-1
    x[2] = -INF
    vals, idx = topk_stable(x, K)
    bv, bi = _brute(x, K)
    assert torch.equal(idx, bi)
    assert torch.equal(vals.view(torch.int32), bv.view(torch.int32))   # bitwise: -0.0 and 0.0 tie, each keeps its sign
    k = min(K, N)
    assert torch.equal(idx[1, :k], torch.arange(k)) and torch.equal(idx[2, :k], torch.arange(k))
    assert bool((idx[:, k:] == -1).all()) and bool((vals[:, k:] == -INF).all())


def _f32(v):
    return torch.tensor(v, dtype=torch.float32).item()


def test_metric_refs_by_hand():
    # the reference notebook's example (cell 27): every nearest neighbour shares the label
    e = torch.tensor([[1, 1], [1, 1.1], [2, 1], [3, 1]], dtype=torch.float32)
    assert precision_at_k_ref(e, torch.tensor([0, 0, 1, 1]), [1]) == {1: 1.0}
    assert recall_at_k_ref(e, e, [1, 2]) == {1: 1.0, 2: 1.0}

    # row 2 repeats row 0 under another label: its stable order is 0, 2, 3, 1, 4, so
    # "drop entry 0" drops row 0 and keeps the query itself.  Orders after the drop:
    #   row 0: 2 3 | row 1: 3 0 (0 ties with 2 and 4) | row 2: 2 3 | row 3: 0 1 (0, 1, 2 tie) | row 4: 1 3
    # labels 0 1 1 0 1 -> correct@1 = 0 0 1 1 1, correct@2 = 1 0 1 1 1
    e = torch.tensor([[1, 0], [0, 1], [1, 0], [1, 1], [-1, 0]], dtype=torch.float32)
    lab = torch.tensor([0, 1, 1, 0, 1])
    assert precision_at_k_ref(e, lab, [1, 2]) == {1: _f32(3 / 5), 2: _f32(4 / 2 / 5)}

    # captions 0, 1 and captions 2, 3 are duplicates: the lower index of a pair comes
    # first, so images 1 and 3 find their own caption second
    t = torch.tensor([[1, 0], [1, 0], [0, 1], [0, 1]], dtype=torch.float32)
    i = torch.tensor([[1, 0], [1, 0.1], [0, 1], [0.1, 1]], dtype=torch.float32)
    assert recall_at_k_ref(i, t, [1, 2, 3]) == {1: 0.5, 2: 1.0, 3: 1.0}


def test_module_fallback_by_hand():
    """The hand-counted cases through the module's fallback branch."""
    V, m = _module()
    e = torch.tensor([[1, 0], [0, 1], [1, 0], [1, 1], [-1, 0]], dtype=torch.float32)
    lab = torch.tensor([0, 1, 1, 0, 1])
    assert V.precision_at_k_on_image_embeddings(m, e, lab, [1, 2]) == {1: _f32(3 / 5), 2: _f32(4 / 2 / 5)}
    t = torch.tensor([[1, 0], [1, 0], [0, 1], [0, 1]], dtype=torch.float32)
    i = torch.tensor([[1, 0], [1, 0.1], [0, 1], [0.1, 1]], dtype=torch.float32)
    assert V.recall_at_k_on_image_text_retreival(m, i, t, [1, 2, 3]) == {1: 0.5, 2: 1.0, 3: 1.0}


def test_half_unit_rows_premise():
    x = half_unit_rows(200, 32, 3, dup=30)
    assert x.shape == (200, 32) and x.dtype == torch.float32
    assert bool(((x != 0).sum(dim=1) == 4).all()) and bool((x.abs() <= 1).all())
    n = torch.nn.functional.normalize(x)
    s32, s64 = n @ n.T, sim_fp64(n, n)
    assert torch.equal(s32.double(), s64) and torch.equal(s64 * 4, torch.round(s64 * 4))
    dup = (s64 == 1).sum().item() - 200
    assert dup >= 2 * 20                          # at least 20 of the 30 copies survive as exact duplicate pairs
    assert torch.equal(x, half_unit_rows(200, 32, 3, dup=30))


def test_exact_inputs_are_tied():
    """The premise of the exact tests: top-16 boundaries fall inside tie groups."""
    img, txt, lab = metric_case()
    ni, nt = torch.nn.functional.normalize(img), torch.nn.functional.normalize(txt)
    s_ii, s_it = tied_boundary_share(sim_fp64(ni, ni), 16), tied_boundary_share(sim_fp64(ni, nt), 16)
    print(f"metric_case: tied top-16 boundary in {s_ii:.3f} of image-image rows, {s_it:.3f} of image-text rows")
    assert s_ii > 0.9 and s_it > 0.9
    for N, E in SIM_CASES:
        q, k = exact_pair(N, E)
        s = tied_boundary_share(sim_fp64(q, k), 16)
        print(f"sim_topk exact inputs N={N} E={E}: tied top-16 boundary in {s:.3f} of rows")
        assert s > 0.9
    # duplicate images under equal and under different labels, duplicate captions, a recall strictly inside (0, 1)
    same = (sim_fp64(ni, ni) == 1).triu(1)
    a, b = same.nonzero(as_tuple=True)
    assert bool((lab[a] == lab[b]).any()) and bool((lab[a] != lab[b]).any())
    assert bool((sim_fp64(nt, nt) == 1).triu(1).any())
    r = recall_at_k_ref(img, txt, [1, 16])
    assert 0.05 < r[1] < r[16] < 0.95


def test_fallback_matches_refs_on_ties():
    V, m = _module()
    img, txt, lab = metric_case()
    ks = [1, 3, 5, 10, 15]
    assert V.precision_at_k_on_image_embeddings(m, img, lab, ks) == precision_at_k_ref(img, lab, ks)
    assert V.recall_at_k_on_image_text_retreival(m, img, txt, ks) == recall_at_k_ref(img, txt, ks)
    # a longer k list does not move the shorter ks
    p20 = V.precision_at_k_on_image_embeddings(m, img, lab, ks + [20])
    r20 = V.recall_at_k_on_image_text_retreival(m, img, txt, ks + [20])
    assert {k: p20[k] for k in ks} == precision_at_k_ref(img, lab, ks)
    assert {k: r20[k] for k in ks} == recall_at_k_ref(img, txt, ks)


@pytest.mark.parametrize("N,E", SIM_CASES)
def test_bound_holds_for_fp32_replay(N, E):
    """The random sim_topk gate on a CPU fp32 replay (fp32 matmul, stable top-16):
    correct fp32 arithmetic meets the bound; the worst |err| / bound is printed."""
    q, k = random_pair(N, E)
    vals, idx = topk_stable(q @ k.T, 16)
    worst = topk_bound_check(vals, idx, sim_fp64(q, k), sim_bound(q, k, C_F32))
    print(f"CPU fp32 replay N={N} E={E}: worst |err|/bound {worst:.4f}")
