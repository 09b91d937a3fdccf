"""GPU: csrc/binmetric_ops.hip (vlp_binmetric_append / _pairs / _fold) through
vlp_amd.metrics.BinaryMetricsDevice, against the class's CPU path, OnlyImagingModule's
binary_metrics and the integers counted on the host (tests/binmetric_cases.py).

Agreement is `==` everywhere: the device compares fp32 scores and adds integers, so its six
integers have one right value, and the host finishes both paths with the same fp64 divisions of
exact integers (see tests/test_binmetrics_cpu.py).  The sizes are those of the CPU test plus
n = 5000, which crosses the 256-row i tile and splits the j range over gridDim.y, and n = 257 with
one negative in the last row (a second i block and a second j tile that hold one row).  The pair
kernel's multi-tile loop (a j range longer than one 256-value LDS tile) only runs through the class
above n = 8192, so it is driven directly with 1, 2 and 3 splits at n = 1000 and n = 5000."""
import pytest
import torch

from tests.binmetric_cases import (BATCHES, KEYS, SIZES, expected, fixed_cases, host_counts, random_case)

pytestmark = pytest.mark.gpu

GPU_SIZES = SIZES + [5000]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vlp_amd import ops as o
    return o


@pytest.fixture(scope="module")
def M():
    from vlp_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def host_metrics():
    from src.models.baseline.OnlyImagingModule import binary_metrics
    return binary_metrics


def bf16_case(n, seed=0):
    """Probabilities as the bf16 modules produce them: torch.sigmoid of bf16 logits, cast to fp32
    (on the device), and random labels.  Ties are frequent, 0.5 included."""
    g = torch.Generator().manual_seed(77 * seed + n)
    logits = (2.0 * torch.randn(n, generator=g)).bfloat16().cuda()
    return torch.sigmoid(logits).float(), torch.randint(0, 2, (n,), generator=g).cuda()


def check(M, host_metrics, p, y, label_dtype=None):
    """p, y on the device.  Device == CPU path == binary_metrics == python-int expectation."""
    pc, yc = p.cpu(), y.cpu().long()
    d = M.BinaryMetricsDevice()
    d.update(p, y if label_dtype is None else y.to(label_dtype))
    c = M.BinaryMetricsDevice()
    c.update(pc, yc)
    raw = d.counts()
    print(f"n={p.numel()} device int64[6] {raw} host {host_counts(pc, yc)}")
    assert raw == host_counts(pc, yc) == c.counts()
    got, cpu, host, want = d.compute(), c.compute(), host_metrics(pc, yc), expected(pc, yc)
    assert tuple(got) == KEYS
    for k in KEYS:
        assert got[k] == cpu[k] == host[k] == want[k], (k, got[k], cpu[k], host[k], want[k])
    return d


@pytest.mark.parametrize("n", GPU_SIZES)
def test_quantised_scores_vs_host(M, host_metrics, n):
    p, y = random_case(n, 1)
    check(M, host_metrics, p.cuda(), y.cuda())


@pytest.mark.parametrize("n", GPU_SIZES)
def test_bf16_sigmoid_scores_vs_host_and_repeatable(ops, M, host_metrics, n):
    p, y = bf16_case(n, 2)
    d = check(M, host_metrics, p, y)
    a = ops.binmetric_counts(n, d._scores, d._labels, d._counts)
    b = ops.binmetric_counts(n, d._scores, d._labels, d._counts)
    assert a.dtype == torch.int64 and a.shape == (6,) and torch.equal(a, b)
    e = M.BinaryMetricsDevice()                    # a second accumulator, fed again
    e.update(p, y)
    assert torch.equal(ops.binmetric_counts(n, e._scores, e._labels, e._counts), a)


def test_one_negative_in_the_last_row(M, host_metrics):
    n = 257
    p, _ = bf16_case(n, 3)
    y = torch.ones(n, dtype=torch.long, device="cuda")
    y[-1] = 0
    d = check(M, host_metrics, p, y)
    tp, fp, fn, tn, wins, ties = d.counts()
    assert tp + fn == 256 and fp + tn == 1 and wins + ties <= 256


@pytest.mark.parametrize("name", sorted(fixed_cases()))
def test_fixed_cases(M, host_metrics, name):
    p, y, stated = fixed_cases()[name]
    got = check(M, host_metrics, p.cuda(), y.cuda()).compute()
    for k, v in stated.items():
        assert got[k] == v, (name, k, got[k], v)


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.uint8, torch.bool])
def test_label_dtypes(M, host_metrics, dtype):
    p, y = bf16_case(1000, 4)
    check(M, host_metrics, p, y, dtype)
    d = M.BinaryMetricsDevice()                    # labels still on the host, as a dataloader hands them over
    d.update(p, y.cpu().to(dtype))
    assert d.counts() == host_counts(p.cpu(), y.cpu())


def test_uneven_batches_doubling_and_reset(M, host_metrics):
    p, y = bf16_case(sum(BATCHES), 5)
    d = M.BinaryMetricsDevice(capacity=256)
    off = 0
    for b in BATCHES:
        d.update(p[off:off + b], y[off:off + b])
        off += b
    assert len(d) == sum(BATCHES) and d._scores.numel() >= sum(BATCHES) > 256 and d._scores.is_cuda
    want = host_counts(p.cpu(), y.cpu())
    assert d.counts() == want
    first = d.compute()
    assert first == host_metrics(p.cpu(), y.cpu().long())
    buffers = (d._scores.data_ptr(), d._labels.data_ptr(), d._counts.data_ptr())
    d.reset()
    assert d.compute() == {} and d.counts() == [0] * 6
    q, z = bf16_case(255, 6)
    d.update(q, z)
    assert d.counts() == host_counts(q.cpu(), z.cpu())
    d.reset()
    d.update(p, y)
    assert d.compute() == first and d.counts() == want
    assert (d._scores.data_ptr(), d._labels.data_ptr(), d._counts.data_ptr()) == buffers


@pytest.mark.parametrize("n", [1000, 5000])
def test_pair_kernel_splits_agree(ops, n):
    """vlp_binmetric_pairs with 1, 2, 3 and the most splits of the j range: the same two sums."""
    from vlp_amd._lib import lib, ptr, stream_of
    p, y = bf16_case(n, 7)
    y8 = y.to(torch.uint8)
    y8[::97] = 2                                   # rows the pair count must skip on either side
    keep = (y8 != 2).cpu()
    want = host_counts(p.cpu()[keep], y.cpu()[keep])[4:]
    bx = (n + ops.BINMETRIC_TILE - 1) // ops.BINMETRIC_TILE
    for splits in (1, 2, 3, bx):
        parts = torch.full((bx * splits, 2), -1, dtype=torch.int64, device="cuda")
        lib().vlp_binmetric_pairs(n, ptr(p), ptr(y8), splits, ptr(parts), stream_of())
        assert parts.sum(0).tolist() == want, (splits, parts.sum(0).tolist(), want)
        assert int(parts.min()) >= 0               # every partial was written


def test_argument_errors(ops, M):
    from vlp_amd._lib import HipError, lib, ptr, stream_of
    p, y = bf16_case(64, 8)
    scores = torch.empty(64, device="cuda")
    labels = torch.empty(64, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        ops.binmetric_append(p, y, scores, labels, 1, counts)          # 1 + 64 rows into 64 slots
    with pytest.raises(TypeError):
        ops.binmetric_append(p, y.float(), scores, labels, 0, counts)
    with pytest.raises(HipError):                                      # the C entry checks the same bound
        lib().vlp_binmetric_append(64, ptr(p), ptr(y), 0, ptr(scores), ptr(labels), 1, 64, ptr(counts), stream_of())
    with pytest.raises(HipError):
        lib().vlp_binmetric_append(64, ptr(p), ptr(y), 3, ptr(scores), ptr(labels), 0, 64, ptr(counts), stream_of())
    parts = torch.empty(4, 2, dtype=torch.int64, device="cuda")
    for n, splits in ((0, 1), (64, 0), (64, 2), (ops.BINMETRIC_MAX_N + 1, 1)):
        with pytest.raises(HipError):
            lib().vlp_binmetric_pairs(n, ptr(scores), ptr(labels), splits, ptr(parts), stream_of())
    with pytest.raises(ValueError):
        ops.binmetric_counts(65, scores, labels, counts)
    assert counts.tolist() == [0, 0, 0, 0]                             # nothing was launched
    ops.binmetric_append(p[:0], y[:0], scores, labels, 64, counts)     # an empty batch at the end: no launch
    assert ops.binmetric_counts(0, scores, labels, counts).tolist() == [0] * 6
