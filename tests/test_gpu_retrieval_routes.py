"""Every route of the epoch-end retrieval path against a stable fp64 reference:
row_topk_kernel / vlp_row_topk (csrc/retrieval_ops.hip), ops.sim_topk and the
module's precision@k / recall@k on the device.

The contract is "descending, ties to the lower index" (tests/retrieval_ref.py:
`topk_stable`).  Everything here is an equality, with one exception: the random
half of the sim_topk tests, whose bound is the linear suite's fp32 one.

Routes of row_topk_kernel and the case that reaches each (`SHAPES` x `PATTERNS`,
test_row_topk_direct; the tile has `ldx` columns with +inf behind column N, 8
rows of +inf behind row R, and the outputs 8 sentinel rows):

  route                                              case
  -------------------------------------------------  -----------------------------------
  one wave, three idle waves in the workgroup         R = 1
  a full workgroup / a partial last workgroup         R = 4 / R = 5, 7
  N < K: tail of idx = -1, vals = -inf                N = 1, 5 (K = 16, 15)
  N = K                                               N = 16, K = 16
  lanes without an element                            N = 1, 5, 16, 63
  one element per lane / lane 0 takes a second        N = 64 / 65
  per-lane list one short of full, full, overflowing  N = 1023, 1024, 1025 (1024 = 64 x 16)
  many evictions per lane (47 elements)               N = 3000
  K = 1, 2 (few pops) / 15, 16 (list drained)         K axis
  row stride = N / != N                               ldx = N / N + 3 (padding +inf)
  insert walks the whole chain / never inserts        `ascending` / `descending`
  tie-break in the insertion chain                    `equal`, `quant8` with N >= 65
  tie-break in the wave-wide pop                      `equal`, `quant8` (any N >= 2)
  all K results from one lane, list fully consumed    `one_lane0`, `one_lane63`, N >= 1024, K = 16
  17 large values in one lane (evict the 17th)        `one_lane0` N = 1025, 3000; `one_lane63` N = 3000
  -inf data ranks above the empty slots               `neg_inf`
  NaN is never selected (out of contract)             test_row_topk_nan
  argument checks before the launch                   test_row_topk_argument_checks

Routes of ops.sim_topk (Q = 257, K = 16):

  E % 4 != 0: zero-padded operands                    E = 30
  Np = ceil4(N) != N: tile padding left unwritten     N = 37, 1001
  N <= 64 (narrow GEMM) / wider                       N = 37 / 1001, 3000
  r0 > 0, sliced outputs, partial last chunk          test_sim_topk_chunked: rows = 1, 3, 100 ->
                                                      257, 86, 3 chunks (counted)

Module (test_module_metrics_device): kernel branch with ks = [1, 3, 5, 10, 15]
and [1, 5, 16]; the fallback branch on the device with 20 added to ks.

Exact inputs.  `half_unit_rows` similarities are multiples of 0.25, exact in fp32
on every GEMM route.  Share of query rows whose 16th and 17th best similarities
are equal, measured on the CPU (tests/test_retrieval_cpu.py::test_exact_inputs_are_tied):
E = 128: 100 % at N = 37, 1001 and 3000; E = 30: 98.8 % (N = 37), 91.8 % (1001),
100 % (3000); the module case (300 rows, E = 32): 100 % image-image, 99.7 %
image-text.  So almost every list is decided by the tie rule.

Random inputs.  b[r, j] = C_F32 * E * 2^-23 * sum_d |q_d k_d| with C_F32 = 1 imported
from tests/test_gpu_linear_routes.py (twice the worst-case bound of an fp32 dot
product of depth E).  Worst |err| / b over the returned entries:

  N, E          CPU fp32 replay   MI355X
  37, 128       0.0105            0.0140
  1001, 128     0.0212            0.0184
  3000, 128     0.0197            0.0186
  37, 30        0.0443            0.0596
  1001, 30      0.0576            0.0694
  3000, 30      0.0683            0.0724

Mutations tried on a scratch copy of csrc/retrieval_ops.hip and ops.py, each
inside the buffers, and the cases that caught them:

  1. tk_before's `ia < ib` reversed (all three sites at once): 64 cases -- every
     `quant8` and `equal` shape with N >= 2, every `neg_inf` shape, test_row_topk_nan
     on its quant8 shapes, all of test_sim_topk_exact and test_sim_topk_chunked,
     test_module_metrics_device.  The `distinct`, `ascending`, `descending`, one_lane
     and random cases pass, as do the five older retrieval cases of test_gpu_ops.py.
  2. the tie rule reversed in the per-lane insertion only (gate and chain): 45
     cases -- `equal` from N = 65 on, `quant8` from N = 1023 on, every `neg_inf`
     shape, test_sim_topk_exact at N = 1001 and 3000, the 12 chunked cases there,
     test_module_metrics_device.  The older cases pass.
  3. the tie rule reversed in the wave-wide pop only: the 64 cases of mutation 1.
     The older cases pass.
  4. the owner test `ix[0] == bi` replaced by `v[0] == bv` (every lane whose head
     ties pops): 56 cases -- `quant8` and `equal` at every shape with N >= 2 and K >= 2,
     `neg_inf` at the shapes with R > 1 and K >= 2, test_row_topk_nan on its quant8 shapes,
     all of test_sim_topk_exact and test_sim_topk_chunked,
     test_module_metrics_device.  The older cases pass.
  5. the pop shifting one slot too few (`j < kTopK - 2`): 6 cases, `one_lane0` and
     `one_lane63` at (7, 1024, 16), (4, 1025, 16) and (7, 3000, 16); nothing else,
     old or new, notices.
  6. the per-lane list one entry shorter (15 slots, K <= 16 still admitted): the
     same 6 one_lane cases and nothing else.
  7. `xr` strided by N instead of ldx: every pattern at every shape with ldx = N + 3
     and R > 1 (40 cases), test_row_topk_nan there, and every sim_topk test with
     N = 37 or 1001 (Np != N); N = 3000 passes.  The older
     test_row_topk_vs_torch[37-16] and [5-16] catch it as well.
  8. sim_topk writing every chunk to vals[0:] / idx[0:]: all 18 cases of
     test_sim_topk_chunked and nothing else, old or new.

Run time of this file on an MI355X: 137 cases in 3.4 s, the slowest 0.6 s.
"""
import math
import zlib

import pytest
import torch

from tests.retrieval_ref import (SIM_CASES, SIM_Q, exact_pair, metric_case, precision_at_k_ref, random_pair,
                                 recall_at_k_ref, sim_bound, sim_fp64, topk_bound_check, topk_stable)
from tests.test_gpu_linear_routes import C_F32

pytestmark = pytest.mark.gpu

INF = float("inf")
NAN = float("nan")
INVAL = 1            # hipErrorInvalidValue
GUARD = 8            # rows behind R in the tile and in both outputs
IDX_SENT = -7


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vlp_amd import ops as o
    return o


# ---------------------------------------------------------------- (a) vlp_row_topk called directly
# (R, N, K, ldx - N); every value of each axis appears, and every pattern runs every shape
SHAPES = [
    (1, 1, 16, 0),       # one wave, one element, N < K
    (4, 5, 15, 3),       # full workgroup, N < K
    (5, 16, 16, 0),      # N = K, a second workgroup with one wave
    (7, 63, 2, 3),       # lane 63 empty
    (1, 64, 1, 3),       # one element per lane, one pop
    (4, 65, 16, 0),      # lane 0 holds two
    (5, 1023, 15, 3),    # lane 63 one short of a full list
    (7, 1024, 16, 0),    # every list exactly full
    (4, 1025, 16, 3),    # lane 0 sees a 17th element
    (1, 1025, 2, 0),
    (7, 3000, 16, 3),    # 47 elements per lane
    (5, 3000, 1, 0),
]


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def _distinct(R, N, K, g):
    return torch.stack([(torch.randperm(N, generator=g).float() - N // 2) * 0.375 for _ in range(R)])


def _quant8(R, N, K, g):
    levels = torch.tensor([-3.0, -1.5, -0.0, 0.0, 0.25, 1.0, 2.0, 7.0])   # -0.0 and 0.0 tie
    return levels[torch.randint(0, 8, (R, N), generator=g)]


def _equal(R, N, K, g):
    return ((torch.arange(R).float() - 2) * 1.5).unsqueeze(1).expand(R, N).contiguous()


def _ascending(R, N, K, g):
    return torch.arange(N).float().unsqueeze(0) * 0.5 + torch.arange(R).float().unsqueeze(1)


def _descending(R, N, K, g):
    return -_ascending(R, N, K, g)


def _one_lane(lane):
    def make(R, N, K, g):
        x = torch.rand(R, N, generator=g)                      # background in [0, 1)
        slots = torch.arange(min(lane, N - 1), N, 64)          # the indices one lane reads
        m = min(len(slots), 17)
        for r in range(R):
            at = slots[torch.randperm(len(slots), generator=g)[:m]]
            x[r, at] = 100.0 + torch.randperm(m, generator=g).float()
        return x
    return make


def _neg_inf(R, N, K, g):
    """Rows cycle through: all -inf; fewer than K finite entries; -inf except the last entry."""
    x = torch.full((R, N), -INF)
    for r in range(R):
        v = (r + N) % 3
        if v == 1:
            m = min(K - 1, N) // 2
            x[r, torch.randperm(N, generator=g)[:m]] = torch.randn(m, generator=g)
        elif v == 2:
            x[r, N - 1] = -1.0
    return x


PATTERNS = {"distinct": _distinct, "quant8": _quant8, "equal": _equal, "ascending": _ascending,
            "descending": _descending, "one_lane0": _one_lane(0), "one_lane63": _one_lane(63), "neg_inf": _neg_inf}


def _row_topk(data, K, pad):
    """vlp_row_topk on a guarded tile holding `data` [R, N] (CPU); returns the whole
    guarded outputs on the CPU."""
    from vlp_amd._lib import lib, ptr
    R, N = data.shape
    ldx = N + pad
    x = torch.full((R + GUARD, ldx), INF)
    x[:R, :N] = data
    xd = x.cuda()
    vals = torch.full((R + GUARD, K), NAN, device="cuda")
    idx = torch.full((R + GUARD, K), IDX_SENT, dtype=torch.int32, device="cuda")
    lib().vlp_row_topk(R, N, ptr(xd), ldx, K, ptr(vals), ptr(idx), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return vals.cpu(), idx.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_exact(vals, idx, ref_vals, ref_idx):
    R = ref_idx.shape[0]
    assert torch.equal(idx[:R].long(), ref_idx)
    assert torch.equal(_bits(vals[:R]), _bits(ref_vals))          # the values are copies of x: bitwise
    assert bool(vals[R:].isnan().all()) and bool((idx[R:] == IDX_SENT).all()), "rows behind R written"


@pytest.mark.parametrize("R,N,K,pad", SHAPES)
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_row_topk_direct(ops, pattern, R, N, K, pad):
    data = PATTERNS[pattern](R, N, K, _gen(pattern, R, N, K))
    assert data.shape == (R, N) and data.dtype == torch.float32
    vals, idx = _row_topk(data, K, pad)
    ref_vals, ref_idx = topk_stable(data, K)
    _assert_exact(vals, idx, ref_vals, ref_idx)
    k = min(K, N)
    if pattern == "equal":
        assert torch.equal(idx[:R, :k].long(), torch.arange(k).expand(R, k))
    if pattern == "neg_inf":
        allinf = (data == -INF).all(dim=1)
        assert torch.equal(idx[:R, :k][allinf].long(), torch.arange(k).expand(int(allinf.sum()), k))
    assert bool((idx[:R, k:] == -1).all()) and bool((vals[:R, k:] == -INF).all())


@pytest.mark.parametrize("R,N,K,pad", [s for s in SHAPES if s[1] > s[2]])
def test_row_topk_nan(ops, R, N, K, pad):
    """NaN is out of contract, but never selected: with at least K other entries the
    result is exactly their stable top-K."""
    g = _gen("nan", R, N, K)
    data = _quant8(R, N, K, g) if N % 2 else _distinct(R, N, K, g)
    nn = min(3, N - K)
    clean = data.clone()
    for r in range(R):
        at = torch.randperm(N, generator=g)[:nn]
        if r == 0:
            at[0] = 0                                            # lane 0's first element
        data[r, at] = NAN
        clean[r, at] = -INF                                      # below every other entry: never among the K best
    assert bool(((clean > -INF).sum(dim=1) >= K).all())
    vals, idx = _row_topk(data, K, pad)
    ref_vals, ref_idx = topk_stable(clean, K)
    _assert_exact(vals, idx, ref_vals, ref_idx)
    assert not bool(vals[:R].isnan().any())


# ---------------------------------------------------------------- (b) argument checks
def test_row_topk_argument_checks(ops):
    from vlp_amd._lib import lib, ptr
    raw = lib()._fns["vlp_row_topk"]              # the return code only, no exception
    R, N, K = 5, 40, 16
    x = torch.randn(R + GUARD, N, device="cuda")
    vals = torch.full((R + GUARD, 17), NAN, device="cuda")
    idx = torch.full((R + GUARD, 17), IDX_SENT, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert raw(R, N, ptr(x), N, 0, ptr(vals), ptr(idx), s) == INVAL
    assert raw(R, N, ptr(x), N, 17, ptr(vals), ptr(idx), s) == INVAL
    assert raw(R, N, ptr(x), N - 1, K, ptr(vals), ptr(idx), s) == INVAL
    assert raw(-1, N, ptr(x), N, K, ptr(vals), ptr(idx), s) == INVAL
    assert raw(R, -1, ptr(x), N, K, ptr(vals), ptr(idx), s) == INVAL
    assert raw(0, N, ptr(x), N, K, ptr(vals), ptr(idx), s) == 0
    torch.cuda.synchronize()
    assert bool(vals.isnan().all()) and bool((idx == IDX_SENT).all())   # nothing was launched


# ---------------------------------------------------------------- (c) ops.sim_topk
K16 = 16


@pytest.fixture(scope="module")
def single_chunk(ops):
    """(vals, idx) of the default single-chunk sim_topk per (kind, N, E), computed once."""
    cache = {}

    def get(kind, N, E):
        if (kind, N, E) not in cache:
            q, k = exact_pair(N, E) if kind == "exact" else random_pair(N, E)
            assert ops.SIM_CHUNK_BYTES // (4 * ((N + 3) // 4 * 4)) >= SIM_Q
            vals, idx = ops.sim_topk(q.cuda(), k.cuda(), K16)
            cache[kind, N, E] = (q, k, vals.cpu(), idx.cpu())
        return cache[kind, N, E]
    return get


def _assert_exact_sim(vals, idx, q, k):
    ref_vals, ref_idx = topk_stable(sim_fp64(q, k), K16)
    assert idx.dtype == torch.int64 and torch.equal(idx, ref_idx)
    assert torch.equal(vals.double(), ref_vals)
    tie = vals.diff(dim=1) == 0
    assert bool(tie.any()) and bool((idx.diff(dim=1)[tie] > 0).all())   # equal keys in index order


@pytest.mark.parametrize("N,E", SIM_CASES)
def test_sim_topk_exact(ops, single_chunk, N, E):
    q, k, vals, idx = single_chunk("exact", N, E)
    _assert_exact_sim(vals, idx, q, k)


@pytest.mark.parametrize("N,E", SIM_CASES)
def test_sim_topk_random(ops, single_chunk, N, E):
    q, k, vals, idx = single_chunk("random", N, E)
    worst = topk_bound_check(vals, idx, sim_fp64(q, k), sim_bound(q, k, C_F32))
    print(f"sim_topk random N={N} E={E}: worst |err|/bound {worst:.4f}")


@pytest.mark.parametrize("N,E", SIM_CASES)
@pytest.mark.parametrize("rows", [1, 3, 100])
def test_sim_topk_chunked(ops, single_chunk, monkeypatch, rows, N, E):
    """257, 86 and 3 chunks (the last of 1, 2 and 57 rows): bitwise the single-chunk result."""
    single = {kind: single_chunk(kind, N, E) for kind in ("exact", "random")}
    nch = math.ceil(SIM_Q / rows)
    chunks = [rows] * (nch - 1) + [SIM_Q - rows * (nch - 1)]
    assert nch == {1: 257, 3: 86, 100: 3}[rows] and (rows == 1 or chunks[-1] < rows)
    monkeypatch.setattr(ops, "SIM_CHUNK_BYTES", rows * 4 * ((N + 3) // 4 * 4))
    calls = []
    fwd = ops.linear_fwd
    monkeypatch.setattr(ops, "linear_fwd", lambda *a, **kw: (calls.append(a[4]), fwd(*a, **kw))[1])
    for kind, (q, k, vals1, idx1) in single.items():
        del calls[:]
        vals, idx = ops.sim_topk(q.cuda(), k.cuda(), K16)
        assert calls == chunks                                   # the patched constant is the one the loop reads
        assert torch.equal(idx.cpu(), idx1), kind
        assert torch.equal(_bits(vals.cpu()), _bits(vals1)), kind
        if kind == "exact":
            _assert_exact_sim(vals.cpu(), idx.cpu(), q, k)


# ---------------------------------------------------------------- (d) module metrics on the device
def test_module_metrics_device(ops):
    from src.models.pretrain.VisionLanguageModule import VisionLanguageModule as V
    m = V.__new__(V)
    img, txt, lab = (t.cuda() for t in metric_case())
    kp, kr = [1, 3, 5, 10, 15], [1, 5, 16]
    p = V.precision_at_k_on_image_embeddings(m, img, lab, kp)
    r = V.recall_at_k_on_image_text_retreival(m, img, txt, kr)
    assert p == precision_at_k_ref(img, lab, kp)
    assert r == recall_at_k_ref(img, txt, kr)
    # 20 among the ks: the fallback branch, on the device, with the same tie rule
    p20 = V.precision_at_k_on_image_embeddings(m, img, lab, kp + [20])
    r20 = V.recall_at_k_on_image_text_retreival(m, img, txt, kr + [20])
    assert {k: p20[k] for k in kp} == p and {k: r20[k] for k in kr} == r
    assert p20 == precision_at_k_ref(img, lab, kp + [20])
    assert r20 == recall_at_k_ref(img, txt, kr + [20])
