"""CPU: the host side of gradient clipping (Lightning's gradient_clip_val /
gradient_clip_algorithm): the Trainer's arguments, its torch path for optimizers
without a fused clip (clip_grad_norm_ / clip_grad_value_ between backward and
step), FusedAdamW.set_gradient_clipping's argument checks and the experiment
config.  The device path is tests/test_gpu_grad_clip.py."""
import pytest
import torch

from src.utils.config import compose
from src.utils.trainer import Trainer


class _TwoLayer(torch.nn.Module):
    """Two nn.Linear layers with the hooks the Trainer drives; SGD with lr 0 so the
    parameters (and with them the next step's gradients) never move."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.a = torch.nn.Linear(5, 7)
        self.b = torch.nn.Linear(7, 2)

    @property
    def device(self):
        return self.a.weight.device

    def configure_optimizers(self):
        return torch.optim.SGD(self.parameters(), lr=0.0)

    def training_step(self, batch, i):
        return (self.b(torch.tanh(self.a(batch["x"]))) - batch["y"]).pow(2).sum()


def _data():
    g = torch.Generator().manual_seed(11)
    return [{"x": torch.randn(6, 5, generator=g) * 3, "y": torch.randn(6, 2, generator=g)}]


def _raw_grads():
    m = _TwoLayer()
    m.training_step(_data()[0], 0).backward()
    return [p.grad.clone() for p in m.parameters()]


def _fit(tmp_path, **kw):
    m = _TwoLayer()
    t = Trainer(max_epochs=1, enable_checkpointing=False, default_root_dir=str(tmp_path), **kw)
    t.fit(m, train_dataloaders=_data())
    return t, [p.grad.clone() for p in m.parameters()]


def _norm(gs):
    return torch.cat([g.double().flatten() for g in gs]).norm().item()


def test_trainer_rejects_unknown_clip_algorithm():
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        Trainer(gradient_clip_algorithm="foo")
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        Trainer(gradient_clip_val=1.0, gradient_clip_algorithm="foo")
    assert Trainer(gradient_clip_val=0.5).gradient_clip_algorithm == "norm"       # None means norm
    assert Trainer(gradient_clip_val=0.5, gradient_clip_algorithm="value").gradient_clip_algorithm == "value"


@pytest.mark.parametrize("val", [None, 0, 0.0])
def test_no_clip_value_leaves_gradients_untouched(tmp_path, val):
    raw = _raw_grads()
    for algo in (None, "norm", "value"):
        t, got = _fit(tmp_path, gradient_clip_val=val, gradient_clip_algorithm=algo)
        assert t.gradient_clip_val is None
        for a, b in zip(got, raw):
            assert torch.equal(a, b)
        assert "grad_norm" not in t.logged_metrics


def test_torch_path_clips_to_the_requested_norm(tmp_path):
    raw = _raw_grads()
    n0 = _norm(raw)
    v = 0.5 * n0
    t, got = _fit(tmp_path, gradient_clip_val=v)
    assert abs(_norm(got) - v) <= 1e-5 * v
    for a, b in zip(got, raw):            # one common factor: the direction is kept
        torch.testing.assert_close(a, b * (v / n0), rtol=1e-5, atol=0)
    # the logged norm is the norm before clipping
    assert abs(t.logged_metrics["grad_norm"] - n0) <= 1e-5 * n0
    # a threshold above the norm changes nothing but still logs the norm
    t, got = _fit(tmp_path, gradient_clip_val=4 * n0, gradient_clip_algorithm="norm")
    for a, b in zip(got, raw):
        assert torch.equal(a, b)
    assert abs(t.logged_metrics["grad_norm"] - n0) <= 1e-5 * n0


def test_torch_path_clips_to_the_requested_value(tmp_path):
    raw = _raw_grads()
    v = 0.25 * max(g.abs().max().item() for g in raw)
    t, got = _fit(tmp_path, gradient_clip_val=v, gradient_clip_algorithm="value")
    assert any((g.abs() > v).any() for g in raw)
    for a, b in zip(got, raw):
        assert torch.equal(a, b.clamp(-v, v))
    assert "grad_norm" not in t.logged_metrics      # clip_grad_value_ computes no norm


def _tiny_fused():
    from vlp_amd.arena import ArenaModule
    from vlp_amd.optim import FusedAdamW

    class Tiny(ArenaModule):
        def __init__(self):
            super().__init__()
            self._init_arena([("w", (5,)), ("b", (3, 7))], device="cpu")
            self._register(self, "w", "w")
            self._register(self, "b", "b")

    m = Tiny()
    return FusedAdamW(m.parameters(), lr=1e-3, arenas=[m])


def test_fused_adamw_set_gradient_clipping_arguments():
    opt = _tiny_fused()
    assert opt._clip is None and opt.last_grad_norm is None            # off by default
    opt.set_gradient_clipping(1.5)
    assert opt._clip == ("norm", 1.5)
    opt.set_gradient_clipping(2, algorithm="value")
    assert opt._clip == ("value", 2.0)
    for off in (None, 0, 0.0, -1.0):
        opt.set_gradient_clipping(1.0)
        opt.set_gradient_clipping(off)
        assert opt._clip is None
    for bad in ("foo", "Norm", None, ""):
        with pytest.raises(ValueError, match="norm.*value"):
            opt.set_gradient_clipping(1.0, algorithm=bad)
    with pytest.raises(ValueError):
        opt.set_gradient_clipping(None, algorithm="foo")               # checked even when turning off
    assert opt._clip is None


def test_trainer_hands_the_clip_to_a_fused_optimizer(tmp_path):
    """An optimizer with set_gradient_clipping gets the Trainer's setting once in fit
    and torch's clip_grad_* is not run on top of it."""
    seen = []

    class Opt(torch.optim.SGD):
        last_grad_norm = None

        def set_gradient_clipping(self, val, algorithm="norm"):
            seen.append((val, algorithm))

    class M(_TwoLayer):
        def configure_optimizers(self):
            return Opt(self.parameters(), lr=0.0)

    raw = _raw_grads()
    m = M()
    t = Trainer(max_epochs=2, enable_checkpointing=False, default_root_dir=str(tmp_path),
                gradient_clip_val=1e-3, gradient_clip_algorithm="value")
    t.fit(m, train_dataloaders=_data())
    assert seen == [(1e-3, "value")]
    for p, b in zip(m.parameters(), raw):
        assert torch.equal(p.grad, b)


def test_clip_experiment_composes():
    c = compose("train", ["experiment=pretrain/pretrain_vit_base_16_tinybert_mi355x_clip"])
    assert c["trainer"]["gradient_clip_val"] == 1.0
    base = compose("train", ["experiment=pretrain/pretrain_vit_base_16_tinybert_mi355x"])
    assert "gradient_clip_val" not in base["trainer"]
    # the clipped experiment is the plain one plus that key (and its own tags / run name)
    for k in ("model", "data", "optimizer"):
        assert c[k] == base[k], k
    assert {k: v for k, v in c["trainer"].items() if k != "gradient_clip_val"} == dict(base["trainer"])
