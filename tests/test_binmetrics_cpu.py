"""CPU: vlp_amd.metrics.BinaryMetricsDevice on CPU tensors (the plain-torch restatement of the
device's integer counts) against OnlyImagingModule's binary_metrics, and the two experiments that
use it through src.utils.config.compose.

Agreement is `==` on all five values, not a tolerance: the numerators and denominators on both
sides are exact integers or half-integers below 2^53 (binary_metrics' rank sum is a sum of
half-integers in fp64, the accumulator's 2 wins + ties a python int), each side does one fp64
division of the same exact quotient (u / (n1 n0) and 2u / (2 n1 n0) round alike), and accuracy,
precision, recall and F1 go through the shared binary_metrics_from_counts.  For n <= 64 the pair
count is also held to a python double loop, and every case to tests/binmetric_cases.expected,
which counts with python ints."""
import functools

import pytest
import torch

from src.models.baseline.OnlyImagingModule import BinaryMetrics, binary_metrics
from src.utils.config import compose, instantiate
from tests.binmetric_cases import (BATCHES, KEYS, SIZES, brute_u2, expected, fixed_cases, host_counts,
                                   random_case)
from vlp_amd.metrics import BinaryMetricsDevice, binary_metrics_from_counts


def _run(p, y, **kw):
    m = BinaryMetricsDevice(**kw)
    m.update(p, y)
    return m


@pytest.mark.parametrize("n", SIZES)
def test_random_ties_equal_binary_metrics(n):
    for seed in range(3):
        p, y = random_case(n, seed)
        m = _run(p, y)
        got, want = m.compute(), binary_metrics(p, y)
        assert tuple(got) == KEYS
        for k in KEYS:
            assert got[k] == want[k] == expected(p, y)[k], (n, seed, k, got[k], want[k])
        assert m.counts() == host_counts(p, y)
        if n <= 64:
            tp, fp, fn, tn, wins, ties = m.counts()
            assert 2 * wins + ties == brute_u2(p, y)
            assert got["auroc"] == (brute_u2(p, y) / (2 * (tp + fn) * (fp + tn)) if (tp + fn) and (fp + tn) else 0.0)


@pytest.mark.parametrize("name", sorted(fixed_cases()))
def test_fixed_cases(name):
    p, y, stated = fixed_cases()[name]
    got, want = _run(p, y).compute(), binary_metrics(p, y)
    for k in KEYS:
        assert got[k] == want[k], (name, k, got[k], want[k])
    for k, v in stated.items():
        assert got[k] == v, (name, k, got[k], v)


def test_label_dtypes_and_shapes():
    p, y = random_case(257, 7)
    want = binary_metrics(p, y)
    for dt in (torch.int64, torch.int32, torch.uint8, torch.bool):
        assert _run(p, y.to(dt)).compute() == want, dt
    assert _run(p.reshape(1, -1), y.reshape(-1, 1)).compute() == want         # flattened, as BinaryMetrics
    assert _run(p.double(), y).compute() == want                              # taken as fp32
    with pytest.raises(ValueError):
        _run(p, y[:-1])


def test_uneven_batches_across_a_buffer_doubling():
    p, y = random_case(sum(BATCHES), 11)
    m = BinaryMetricsDevice(capacity=256)          # 7 + 1 + 250 + 513 rows: grows 256 -> 771
    off = 0
    for b in BATCHES:
        m.update(p[off:off + b], y[off:off + b])
        off += b
    assert len(m) == sum(BATCHES) and m._scores.numel() >= sum(BATCHES) > 256
    one = _run(p, y)
    assert m.counts() == one.counts() == host_counts(p, y)
    assert m.compute() == one.compute() == binary_metrics(p, y)
    # the host accumulator fed the same batches agrees as well
    h = BinaryMetrics()
    off = 0
    for b in BATCHES:
        h.update(p[off:off + b], y[off:off + b])
        off += b
    assert h.compute() == m.compute()


def test_reset_and_reuse_allocates_nothing():
    m = BinaryMetricsDevice(capacity=64)
    assert m.compute() == {} and len(m) == 0
    m.reset()                                      # before the first update: nothing to zero
    p, y = random_case(1000, 5)
    m.update(p, y)
    first = m.compute()
    assert m.compute() == first                    # compute() leaves the state alone
    buffers = (m._scores.data_ptr(), m._labels.data_ptr(), m._counts.data_ptr())
    m.reset()
    assert m.compute() == {} and len(m) == 0
    assert (m._scores.data_ptr(), m._labels.data_ptr(), m._counts.data_ptr()) == buffers
    q, z = random_case(255, 6)
    m.update(q, z)
    assert m.compute() == binary_metrics(q, z)
    m.reset()
    m.update(p, y)
    assert m.compute() == first
    assert (m._scores.data_ptr(), m._labels.data_ptr(), m._counts.data_ptr()) == buffers


def test_shared_helper_rules():
    z = binary_metrics_from_counts(0, 0, 0, 0, 0)
    assert z == dict.fromkeys(KEYS, 0.0)
    assert binary_metrics_from_counts(0, 0, 3, 4, 0)["precision"] == 0.0      # nothing predicted positive
    assert binary_metrics_from_counts(0, 5, 0, 4, 0)["recall"] == 0.0         # no positives
    assert binary_metrics_from_counts(3, 0, 0, 0, 0)["auroc"] == 0.0          # one class only
    v = binary_metrics_from_counts(2, 1, 1, 3, 17)
    assert v["auroc"] == 17 / 24 and v["accuracy"] == 5 / 7 and v["f1"] == 2 * (2 / 3) * (2 / 3) / (4 / 3)
    assert binary_metrics_from_counts(2, 1, 1, 3, 17.0) == v                  # binary_metrics passes a float


# ---------------- the two experiments ----------------
DEFAULT_CALLBACKS = {"lr_monitor", "checkpoint_internal", "checkpoint_btxrd", "early_stopping_internal",
                     "early_stopping_btxrd", "snapshot_btxrd", "snapshot_internal", "snapshot_combined"}


def test_fusion_metrics_experiment_composes():
    c = compose("train", ["experiment=baseline_imaging_and_clinical/baseline_imaging_and_clinical_resnet_34_mi355x_metrics"])
    assert set(c["callbacks"]) == DEFAULT_CALLBACKS            # the reference's callbacks: default, nothing private
    assert c["callbacks"]["checkpoint_btxrd"]["monitor"] == "val/btxrd/accuracy"
    assert c["callbacks"]["checkpoint_internal"]["monitor"] == "val/internal/accuracy"
    assert c["callbacks"]["snapshot_combined"]["monitor"] == "val/combined/accuracy"
    assert c["post_fit_evaluation"] is True
    ref = compose("train", ["experiment=baseline_imaging_and_clinical/baseline_imaging_and_clinical_resnet_34"])
    for k in ("model", "data", "trainer", "optimizer", "scheduler"):
        assert c[k] == ref[k], k
    assert c["model"]["_target_"] == "src.models.baseline.FusionModule.FusionModule"
    m = instantiate(c["model"], device="cpu")
    assert isinstance(m.hparams.optimizer, functools.partial)
    assert isinstance(m.train_metrics, BinaryMetricsDevice)
    assert set(m.val_metrics) == {"internal", "btxrd", "combined"}
    assert all(isinstance(v, BinaryMetricsDevice) for v in m.val_metrics.values())
    assert m.all_val_probs == [] and m.all_val_image_features == []


def test_only_imaging_metrics_experiment_composes():
    c = compose("train", ["experiment=baseline_only_imaging/baseline_only_imaging_resnet_34_mi355x_metrics"])
    assert set(c["callbacks"]) == DEFAULT_CALLBACKS
    assert c["model"]["metrics_on_device"] is True and c["model"]["model"] == "resnet34"
    m = instantiate(c["model"], device="cpu")
    assert m.hparams.metrics_on_device is True
    assert isinstance(m.train_metrics, BinaryMetricsDevice)
    assert all(isinstance(v, BinaryMetricsDevice) for v in m.val_metrics.values())
    from src.models.baseline.OnlyImagingModule import OnlyImagingModule
    d = OnlyImagingModule("resnet34", None, device="cpu")                     # the default is the host accumulator
    assert d.hparams.metrics_on_device is False and isinstance(d.train_metrics, BinaryMetrics)
    assert all(isinstance(v, BinaryMetrics) for v in d.val_metrics.values())
