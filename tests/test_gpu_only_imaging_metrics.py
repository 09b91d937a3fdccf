"""GPU: OnlyImagingModule(metrics_on_device=True) logs what the default host accumulators log, bit
for bit: two modules with the same weights run the same train epoch and validation epoch, one with
BinaryMetricsDevice and one with BinaryMetrics, and every logged value is compared with `==`.  Both
take their probabilities from the same kernels on the same weights and inputs (the towers' forward
and the optimizer step are bitwise reproducible), so the two metric paths see identical inputs."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("accuracy", "precision", "recall", "f1", "auroc")
B, H = 8, 64


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    x_u8 = torch.randint(0, 256, (B, 1, H, H), generator=g, dtype=torch.uint8)
    return {"x-ray": ((x_u8.float() - 127.5) / 73.9).repeat(1, 3, 1, 1),
            "tumor": torch.randint(0, 2, (B,), generator=g),
            "dataset": ["INTERNAL" if (i + seed) % 3 else "BTXRD" for i in range(B)]}


def _epoch(m):
    opt = m.configure_optimizers()["optimizer"]
    m.train()
    for i, s in enumerate((1, 2)):
        opt.zero_grad(set_to_none=False)
        m.training_step(_batch(s), i).backward()
        opt.step()
    m.on_train_epoch_end()
    m.eval()
    for idx, seeds in enumerate(((3, 4), (5, 6))):
        for j, s in enumerate(seeds):
            m.validation_step(_batch(s), j, idx)
    m.on_validation_epoch_end()
    return {k: (float(v.detach()) if torch.is_tensor(v) else v) for k, v in m.logged.items()}


def test_device_and_host_accumulators_log_the_same_values():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from src.models.baseline.OnlyImagingModule import BinaryMetrics, OnlyImagingModule
    from vlp_amd.metrics import BinaryMetricsDevice
    make = functools.partial(OnlyImagingModule, "resnet34", functools.partial(torch.optim.AdamW, lr=1e-3),
                             label_weights=(0.7, 2.0), coral_lambda=0.5, compute_dtype="fp32")
    torch.manual_seed(21)
    host = make()
    dev = make(metrics_on_device=True)
    dev.load_state_dict(host.state_dict())
    assert isinstance(host.train_metrics, BinaryMetrics) and isinstance(dev.train_metrics, BinaryMetricsDevice)
    assert all(isinstance(v, BinaryMetricsDevice) for v in dev.val_metrics.values())
    a, b = _epoch(host), _epoch(dev)
    assert set(a) == set(b)
    for prefix in ("train", "val/internal", "val/btxrd", "val/combined"):
        for k in KEYS:
            assert f"{prefix}/{k}" in b, (prefix, k)
    for k in sorted(a):
        print(f"{k}: host {a[k]} device {b[k]}")
        assert a[k] == b[k], (k, a[k], b[k])
    assert dev.all_val_probs == [] and all(len(v) == 0 for v in dev.val_metrics.values())
    assert len(dev.train_metrics) == 0


def test_metrics_experiment_instantiates_with_the_flag():
    from src.utils.config import compose, instantiate
    from vlp_amd.metrics import BinaryMetricsDevice
    c = compose("train", ["experiment=baseline_only_imaging/baseline_only_imaging_resnet_34_mi355x_metrics"])
    assert c["model"]["metrics_on_device"] is True
    m = instantiate(c["model"])
    assert m.hparams.metrics_on_device is True and m.device.type == "cuda"
    assert isinstance(m.train_metrics, BinaryMetricsDevice)
    b = _batch(7)
    m.eval()
    m.validation_step(b, 0, 0)
    m.on_validation_epoch_end()
    assert all(f"val/combined/{k}" in m.logged for k in KEYS)
