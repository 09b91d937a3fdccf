"""CPU: the host side of gradient accumulation (Lightning's accumulate_grad_batches): the
Trainer's argument, how often the optimizer, a scheduler and global_step advance, the loss
scale, where zero_grad / clipping / the data-parallel reduction run, what the Trainer asks of
an optimizer that accumulates on its own (FusedAdamW's protocol, played by a stub), and the
experiment config.  The device path is tests/test_gpu_grad_accum.py.

Step counts: an epoch of n batches takes ceil(n / k) optimizer steps, the last one over the
n % k batches left of a group: 10 batches give 10, 4 and 3 steps for k = 1, 3, 4."""
import math

import pytest
import torch

from src.utils.config import compose
from src.utils.trainer import Trainer

N_BATCHES = 10


class _Counting(torch.optim.SGD):
    """SGD that records the order of its calls."""

    def __init__(self, params, lr, events):
        super().__init__(params, lr=lr)
        self.events = events

    def zero_grad(self, set_to_none=True):
        self.events.append("zero")
        return super().zero_grad(set_to_none=set_to_none)

    def step(self, closure=None):
        self.events.append("step")
        return super().step(closure)


class _Linear(torch.nn.Module):
    """One weight vector, loss = w . x_i: the gradient of batch i is x_i exactly."""

    def __init__(self, interval="step", lr=0.0):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(4))
        self.events, self.interval, self.lr = [], interval, lr
        self.epoch_ends = 0

    @property
    def device(self):
        return self.w.device

    def configure_optimizers(self):
        opt = _Counting(self.parameters(), self.lr, self.events)
        self.sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0)
        return {"optimizer": opt, "lr_scheduler": {"scheduler": self.sched, "interval": self.interval, "frequency": 1}}

    def training_step(self, batch, i):
        self.events.append("batch")
        return (self.w * batch["x"]).sum()

    def on_train_epoch_end(self):
        self.epoch_ends += 1


def _data(n=N_BATCHES):
    g = torch.Generator().manual_seed(5)
    return [{"x": torch.randn(4, generator=g)} for _ in range(n)]


def _fit(model, tmp_path, data=None, **kw):
    kw.setdefault("max_epochs", 1)
    t = Trainer(enable_checkpointing=False, default_root_dir=str(tmp_path), **kw)
    t.fit(model, train_dataloaders=_data() if data is None else data)
    return t


@pytest.mark.parametrize("bad", [0, -1, 2.0, 1.5, "2", None, True])
def test_trainer_rejects_bad_accumulate_grad_batches(bad):
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        Trainer(accumulate_grad_batches=bad)


def test_trainer_accumulate_grad_batches_default_is_one():
    assert Trainer().accumulate_grad_batches == 1
    assert Trainer(accumulate_grad_batches=4).accumulate_grad_batches == 4


@pytest.mark.parametrize("k,steps", [(1, 10), (3, 4), (4, 3)])
def test_steps_scheduler_and_global_step_per_epoch(tmp_path, k, steps):
    assert steps == math.ceil(N_BATCHES / k)
    m = _Linear(interval="step")
    t = _fit(m, tmp_path, accumulate_grad_batches=k, log_every_n_steps=1)
    assert m.events.count("batch") == N_BATCHES
    assert m.events.count("step") == steps
    assert t.global_step == steps
    assert m.sched.last_epoch == steps                      # a step-interval scheduler: once per optimizer step
    assert m.events.count("zero") == steps                  # zero_grad only at the start of a group
    # the order inside one epoch: zero, k batches, step, ...; the remainder group steps too
    want = []
    for s in range(steps):
        want += ["zero"] + ["batch"] * min(k, N_BATCHES - s * k) + ["step"]
    assert m.events == want
    assert [s for s, _ in t.history] == list(range(1, steps + 1))      # logged at optimizer steps only
    assert len(t.step_times) == N_BATCHES


@pytest.mark.parametrize("k", [1, 4])
def test_epoch_interval_scheduler_still_steps_once_per_epoch(tmp_path, k):
    m = _Linear(interval="epoch")
    t = _fit(m, tmp_path, accumulate_grad_batches=k, max_epochs=2)
    assert m.sched.last_epoch == 2 and m.epoch_ends == 2
    assert t.global_step == 2 * math.ceil(N_BATCHES / k)


def test_groups_do_not_span_epochs(tmp_path):
    """7 batches, k = 4, two epochs: groups of 4 + 3 in each epoch, never 4 + 4 + 4 + 2."""
    m = _Linear()
    t = _fit(m, tmp_path, data=_data(7), accumulate_grad_batches=4, max_epochs=2)
    assert t.global_step == 4
    one = ["zero"] + ["batch"] * 4 + ["step"] + ["zero"] + ["batch"] * 3 + ["step"]
    assert m.events == one * 2


def test_max_steps_counts_optimizer_steps(tmp_path):
    m = _Linear()
    t = _fit(m, tmp_path, accumulate_grad_batches=3, max_steps=2, max_epochs=5)
    assert t.global_step == 2 and m.events.count("batch") == 6 and m.events.count("step") == 2


def test_limit_train_batches_leaves_a_remainder_that_steps(tmp_path):
    m = _Linear()
    t = _fit(m, tmp_path, accumulate_grad_batches=4, limit_train_batches=6)
    assert m.events.count("batch") == 6 and t.global_step == 2


@pytest.mark.parametrize("k", [2, 4])
def test_accumulated_gradient_is_the_mean_of_the_group(tmp_path, k):
    """lr 1 from w = 0: after the epoch w = -sum over groups of (sum of the group's x) / k,
    the remainder group included (Lightning scales every micro-batch by 1 / k, also there)."""
    data = _data()
    m = _Linear(lr=1.0)
    _fit(m, tmp_path, data=data, accumulate_grad_batches=k)
    want = -torch.stack([b["x"] for b in data]).sum(0) / k
    torch.testing.assert_close(m.w.detach(), want, rtol=1e-6, atol=1e-6)


def test_logged_loss_is_the_unscaled_loss_of_the_last_micro_batch(tmp_path):
    data = _data(4)
    m = _Linear(lr=0.0)
    with torch.no_grad():
        m.w.fill_(0.5)
    t = _fit(m, tmp_path, data=data, accumulate_grad_batches=4)
    assert t.history == [(1, pytest.approx((0.5 * data[3]["x"]).sum().item(), rel=1e-6))]


def test_clipping_sees_the_accumulated_gradient(tmp_path):
    """torch path: clip_grad_norm_ runs once per optimizer step, on the accumulated gradient."""
    data = _data(4)
    acc = torch.stack([b["x"] for b in data]).sum(0) / 4
    n0 = acc.norm().item()
    m = _Linear(lr=0.0)
    t = _fit(m, tmp_path, data=data, accumulate_grad_batches=4, gradient_clip_val=0.5 * n0)
    assert abs(t.logged_metrics["grad_norm"] - n0) <= 1e-5 * n0
    torch.testing.assert_close(m.w.grad, acc * 0.5, rtol=1e-5, atol=1e-7)


def test_data_parallel_reduction_runs_once_per_optimizer_step(tmp_path, monkeypatch):
    """A module without its own collectives: the gradient mean across ranks is taken of the
    accumulated gradient, right before each optimizer step."""
    m = _Linear()
    calls = []
    monkeypatch.setattr(Trainer, "_dp_world", staticmethod(lambda: 2))
    monkeypatch.setattr(Trainer, "average_gradients",
                        staticmethod(lambda model, world: (calls.append(world), model.events.append("reduce"))))
    t = _fit(m, tmp_path, accumulate_grad_batches=4)
    assert calls == [2] * t.global_step == [2, 2, 2]
    assert all(m.events[i + 1] == "step" for i, e in enumerate(m.events) if e == "reduce")


class _AccumulatingOpt(torch.optim.SGD):
    """FusedAdamW's accumulation protocol: the gradient buffer is overwritten by every backward
    (here: the Trainer's backward adds to p.grad, so accumulate() moves it away and clears it)."""
    last_grad_norm = None

    def __init__(self, params, events):
        super().__init__(params, lr=1.0)
        self.events, self.acc, self.clip = events, None, None

    def set_gradient_clipping(self, val, algorithm="norm"):
        self.clip = (val, algorithm)

    def accumulate(self, w=1.0, first=None):
        p = self.param_groups[0]["params"][0]
        self.events.append(("accumulate", w, first))
        self.acc = w * p.grad.clone() if first else self.acc + w * p.grad
        p.grad = None

    def reduce_accumulated(self):
        self.events.append("reduce")

    def zero_grad(self, set_to_none=True):
        self.events.append("zero")
        self.acc = None
        for p in self.param_groups[0]["params"]:
            p.grad = None

    def step(self, closure=None):
        p = self.param_groups[0]["params"][0]
        self.events.append("step" if p.grad is not None else "step-folded")
        g = self.acc if p.grad is None else p.grad if self.acc is None else self.acc + p.grad
        self.acc = None
        with torch.no_grad():
            p -= g


class _Fused(_Linear):
    handles_dp_collectives = True

    def configure_optimizers(self):
        self.opt = _AccumulatingOpt(self.parameters(), self.events)
        return self.opt


def test_accumulating_optimizer_protocol(tmp_path):
    """k - 1 micro-batches go through accumulate(1.0, first), the k-th stays in the gradient
    buffer for step(); the remainder group is folded entirely and step() runs without a fresh
    gradient.  The result is the mean-of-group update."""
    data = _data()
    m = _Fused()
    t = _fit(m, tmp_path, data=data, accumulate_grad_batches=4, gradient_clip_val=1e9)
    ev = [e for e in m.events if e != "batch"]
    group = ["zero", ("accumulate", 1.0, True), ("accumulate", 1.0, False), ("accumulate", 1.0, False), "step"]
    assert ev == group * 2 + ["zero", ("accumulate", 1.0, True), ("accumulate", 1.0, False), "step-folded"]
    assert t.global_step == 3 and m.opt.clip == (1e9, "norm")
    assert m.defer_grad_reduce is False
    torch.testing.assert_close(m.w.detach(), -torch.stack([b["x"] for b in data]).sum(0) / 4, rtol=1e-6, atol=1e-6)


def test_accumulating_optimizer_k1_is_the_plain_loop(tmp_path):
    m = _Fused()
    _fit(m, tmp_path, data=_data(3), accumulate_grad_batches=1)
    assert [e for e in m.events if e != "batch"] == ["zero", "step"] * 3
    assert not hasattr(m, "defer_grad_reduce")


def test_accumulating_optimizer_under_data_parallelism(tmp_path, monkeypatch):
    """World 2 and a module that reduces inside its backward: it is told to defer, every
    micro-batch is folded, and the accumulators are all-reduced once per optimizer step."""
    import src.utils.trainer as T
    monkeypatch.setattr(T, "_dist_on", lambda: True)
    monkeypatch.setattr(T, "_any_rank", lambda flag: flag)
    monkeypatch.setattr(Trainer, "_dp_world", staticmethod(lambda: 2))
    m = _Fused()
    t = _fit(m, tmp_path, data=_data(5), accumulate_grad_batches=3)
    assert m.defer_grad_reduce is True and t.global_step == 2
    ev = [e for e in m.events if e != "batch"]
    assert ev == ["zero", ("accumulate", 1.0, True), ("accumulate", 1.0, False), ("accumulate", 1.0, False), "reduce",
                  "step-folded",
                  "zero", ("accumulate", 1.0, True), ("accumulate", 1.0, False), "reduce", "step-folded"]


def test_accum_experiment_composes():
    c = compose("train", ["experiment=pretrain/pretrain_vit_base_16_tinybert_mi355x_accum"])
    assert c["trainer"]["accumulate_grad_batches"] == 4
    assert c["trainer"]["gradient_clip_val"] == 1.0
    assert c["data"]["batch_size"] == 64
    assert c["model"]["fused_optimizer"] is True
    clip = compose("train", ["experiment=pretrain/pretrain_vit_base_16_tinybert_mi355x_clip"])
    assert "accumulate_grad_batches" not in clip["trainer"]
    # the clipped experiment with a quarter of the batch and the accumulation key
    assert c["model"] == clip["model"] and c["optimizer"] == clip["optimizer"]
    assert {k: v for k, v in c["data"].items() if k != "batch_size"} == \
        {k: v for k, v in clip["data"].items() if k != "batch_size"}
    assert {k: v for k, v in c["trainer"].items() if k != "accumulate_grad_batches"} == dict(clip["trainer"])
    t = Trainer(**{k: v for k, v in c["trainer"].items() if k != "_target_"})
    assert t.accumulate_grad_batches == 4 and t.gradient_clip_val == 1.0
