"""CPU: the host side of the fused torch.optim.Adam step: which kernel FusedAdam launches in
every case (the ops stubbed), that FusedAdamW's launches are untouched, the module's choice of
optimizer, the experiment config, and the arithmetic behind the bounds of
tests/test_gpu_adam.py, on that file's own inputs:

  envelope        the kernel's formula evaluated with fp32 torch ops stays within the 1e-6
                  (rel-L2) of fp64 torch.optim.Adam that the GPU test asserts: the bound is met
                  by the arithmetic itself, not by a lucky kernel
  discrimination  fp64 torch.optim.AdamW (decoupled decay, the same wd = 0.2) is at least 100
                  times that bound away from fp64 Adam in p, exp_avg and exp_avg_sq: an
                  implementation that decays the parameter instead cannot pass the GPU test
"""
import functools

import pytest
import torch

from src.utils.config import compose, instantiate
from src.utils.trainer import Trainer
from tests.test_gpu_adam import BOUND, MODES, OFFS, SIZES, WD, adam64, case, clipped64, formula32
from tests.test_gpu_grad_clip import rel

ADAMW_OPS = ("adamw", "adamw_clip", "adamw_clip_accum")


# ---------------------------------------------------------------- FusedAdam's launches
def _tiny(cls, **kw):
    from vlp_amd.arena import ArenaModule

    class Tiny(ArenaModule):
        def __init__(self):
            super().__init__()
            self._init_arena([("w", (5,)), ("b", (3, 7))], device="cpu")
            self._register(self, "w", "w")
            self._register(self, "b", "b")

    m = Tiny()
    return m, cls(m.parameters(), lr=1e-3, arenas=[m], **kw)


class _Recorder:
    """vlp_amd.ops as FusedAdamW uses it: every call is recorded, nothing is computed."""

    def __init__(self):
        self.calls = []

    def grad_sumsq_nparts(self, n):
        return 1

    def __getattr__(self, name):
        def op(*a, **k):
            self.calls.append((name, a, k))
            return 1 if name.endswith("sumsq") else None
        return op

    def names(self):
        return [c[0] for c in self.calls]


def _backward(m):
    for k, p in m.named_parameters():
        p.grad = m.arena.gview(k)


def _run(cls, monkeypatch, clip, how):
    """One step(): how = plain | pending (two folded, the third fresh) | folded (all three)."""
    import vlp_amd.optim as O
    rec = _Recorder()
    monkeypatch.setattr(O, "ops", rec)
    m, opt = _tiny(cls)
    if clip is not None:
        opt.set_gradient_clipping(0.5, clip)
    if how != "plain":
        for i in range(3 if how == "folded" else 2):
            _backward(m)
            opt.accumulate(1.0, first=i == 0)
    if how != "folded":
        _backward(m)
    rec.calls.clear()
    opt.step(w=0.5)
    return m, opt, rec


@pytest.mark.parametrize("how", ["plain", "pending", "folded"])
@pytest.mark.parametrize("clip", [None, "norm", "value"])
def test_fused_adam_launches_one_adam_step_per_span(monkeypatch, clip, how):
    from vlp_amd.optim import FusedAdam
    m, opt, rec = _run(FusedAdam, monkeypatch, clip, how)
    assert not set(rec.names()) & set(ADAMW_OPS)                      # never an AdamW kernel
    steps = [c for c in rec.calls if c[0] == "adam_step"]
    assert len(steps) == 1                                            # w and b: one span of one arena
    _, a, k = steps[0]
    p, g = a[0], a[1]
    acc = opt._acc.get(id(m.arena))
    assert p.data_ptr() == m.arena.data.data_ptr()
    assert a[4:10] == (1e-3, 0.9, 0.999, 1e-8, 0, 1)                  # torch.optim.Adam's defaults, step 1
    # the gradient operand: the accumulator when every micro-batch was folded, else the arena
    assert g.data_ptr() == (acc.data_ptr() if how == "folded" else m.arena.grad.data_ptr())
    if how == "pending":
        assert k["acc"].data_ptr() == acc.data_ptr() and k["w"] == 0.5
    else:
        assert "acc" not in k and "w" not in k
    assert ("coef" in k, "clip_value" in k) == (clip == "norm", clip == "value")
    if clip == "value":
        assert k["clip_value"] == 0.5
    # the norm pass is FusedAdamW's
    norm = [n for n in rec.names() if n != "adam_step"]
    if clip == "norm":
        assert norm == ["grad_accum_sumsq" if how == "pending" else "grad_sumsq", "clip_coef"]
        assert k["coef"].data_ptr() == opt._clip_bufs[1][1:].data_ptr()
    else:
        assert norm == []
    assert set(opt.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}


@pytest.mark.parametrize("how", ["plain", "pending", "folded"])
@pytest.mark.parametrize("clip", [None, "norm", "value"])
def test_fused_adamw_launches_are_untouched(monkeypatch, clip, how):
    from vlp_amd.optim import FusedAdamW
    _, _, rec = _run(FusedAdamW, monkeypatch, clip, how)
    assert "adam_step" not in rec.names()
    want = "adamw_clip_accum" if how == "pending" else "adamw" if clip is None else "adamw_clip"
    assert [n for n in rec.names() if n in ADAMW_OPS] == [want]


def test_fused_adam_defaults_and_rejected_options():
    from vlp_amd.optim import FusedAdam, FusedAdamW
    _, opt = _tiny(FusedAdam)
    assert isinstance(opt, FusedAdamW)
    t = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))])
    for k in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize"):
        assert opt.defaults[k] == t.defaults[k], k
    assert opt.defaults["weight_decay"] == 0
    assert set(t.param_groups[0]) <= set(opt.param_groups[0]) | {"decoupled_weight_decay"}
    for kw in (dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(ValueError, match="amsgrad / maximize"):
            _tiny(FusedAdam, **kw)
    _tiny(FusedAdam, amsgrad=False, maximize=False, weight_decay=0.2)
    # what the Trainer dispatches on, and everything around the launch, is inherited (torch wraps
    # step() on every class, so it is not in this list: the launch tests above cover it)
    for name in ("set_gradient_clipping", "accumulate", "reduce_accumulated", "zero_grad", "_spans", "_launch_norm"):
        assert hasattr(FusedAdam, name) and name not in vars(FusedAdam), name
    assert "_launch" in vars(FusedAdam)


def test_fused_adam_state_dict_loads_into_torch_adam_and_back():
    from vlp_amd.optim import FusedAdam
    m, opt = _tiny(FusedAdam, weight_decay=0.2)
    for p in m.parameters():          # what a step leaves, without a kernel
        st = opt._bind(p)
        st["exp_avg"].fill_(0.5)
        st["exp_avg_sq"].fill_(0.25)
        opt._steps[id(p)] = 4
    sd = opt.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][0]["step"]) == 4.0
    clones = [torch.nn.Parameter(p.detach().clone()) for p in m.parameters()]
    t = torch.optim.Adam(clones, lr=1.0)
    t.load_state_dict(sd)
    assert t.param_groups[0]["weight_decay"] == 0.2 and t.param_groups[0]["lr"] == 1e-3
    for q in clones:
        q.grad = torch.ones_like(q)
    t.step()                          # torch accepts the groups and the state as its own
    assert float(t.state[clones[0]]["step"]) == 5.0
    m2, o2 = _tiny(FusedAdam)
    o2.load_state_dict(t.state_dict())
    w2 = m2._parameters["w"]
    assert o2._steps[id(w2)] == 5 and o2.param_groups[0]["weight_decay"] == 0.2
    assert torch.equal(o2.state[w2]["exp_avg"], t.state[clones[0]]["exp_avg"])
    assert o2.state[w2]["exp_avg"].data_ptr() == o2._moments(m2.arena)[0].data_ptr()   # back in the flat buffer
    bad = t.state_dict()
    bad["param_groups"][0]["amsgrad"] = True
    with pytest.raises(ValueError, match="amsgrad"):
        _tiny(FusedAdam)[1].load_state_dict(bad)


# ---------------------------------------------------------------- the module's choice
@pytest.fixture(scope="module")
def module():
    from src.models.pretrain.VisionLanguageModule import VisionLanguageModule
    return VisionLanguageModule("resnet34", "tinybert", functools.partial(torch.optim.Adam, lr=1e-3), False, False,
                                512, 312, 128, device="cpu")


def _optimizer(module, factory, fused=True):
    module.hparams["optimizer"], module.hparams["fused_optimizer"] = factory, fused
    return module.configure_optimizers()["optimizer"]


def test_module_builds_fused_adam_for_torch_adam(module):
    from vlp_amd.optim import FusedAdam, FusedAdamW
    opt = _optimizer(module, functools.partial(torch.optim.Adam, lr=2e-3, weight_decay=0.2, betas=(0.8, 0.9)))
    assert type(opt) is FusedAdam
    assert [g["name"] for g in opt.param_groups] == ["remaining_params", "projection_and_logitscale", "image_encoder",
                                                     "text_encoder"]
    for g in opt.param_groups:
        assert (g["lr"], g["weight_decay"], g["betas"]) == (2e-3, 0.2, (0.8, 0.9))
    arenas = {id(a) for a, _, _ in opt._loc.values()}
    assert arenas == {id(module._head.arena), id(module.image_encoder.model.arena), id(module.text_encoder.model.arena)}
    assert type(_optimizer(module, torch.optim.Adam)) is FusedAdam                       # a bare class, not a partial
    # options without a kernel, and the switch, keep torch's optimizer
    for kw in (dict(amsgrad=True), dict(maximize=True)):
        assert type(_optimizer(module, functools.partial(torch.optim.Adam, lr=1e-3, **kw))) is torch.optim.Adam
    assert type(_optimizer(module, functools.partial(torch.optim.Adam, lr=1e-3, amsgrad=False))) is FusedAdam
    assert type(_optimizer(module, functools.partial(torch.optim.Adam, lr=1e-3), fused=False)) is torch.optim.Adam
    # AdamW as before
    assert type(_optimizer(module, functools.partial(torch.optim.AdamW, lr=1e-3))) is FusedAdamW
    assert type(_optimizer(module, functools.partial(torch.optim.AdamW, lr=1e-3), fused=False)) is torch.optim.AdamW
    assert type(_optimizer(module, functools.partial(torch.optim.SGD, lr=1e-3))) is torch.optim.SGD


def test_adam_experiment_composes():
    c = compose("train", ["experiment=pretrain/pretrain_resnet34_distilbert_mi355x_adam"])
    factory = instantiate(c["optimizer"])
    assert factory.func is torch.optim.Adam
    assert factory.keywords == {"lr": 5e-5, "weight_decay": 0.2}
    assert c["trainer"]["accumulate_grad_batches"] == 2 and c["trainer"]["gradient_clip_val"] == 1.0
    assert c["model"]["fused_optimizer"] is True and c["model"]["text_encoder_model"] == "distilbert"
    base = compose("train", ["experiment=pretrain/pretrain_resnet34_distilbert_mi355x"])
    assert base["optimizer"]["_target_"] == "torch.optim.AdamW"
    assert c["model"]["optimizer"] == c["optimizer"]                     # the model is handed that factory
    assert {k: v for k, v in c["model"].items() if k != "optimizer"} == \
        {k: v for k, v in base["model"].items() if k != "optimizer"}
    # two micro-batches make the base experiment's batch
    assert c["data"]["batch_size"] * c["trainer"]["accumulate_grad_batches"] == base["data"]["batch_size"]
    assert {k: v for k, v in c["data"].items() if k != "batch_size"} == \
        {k: v for k, v in base["data"].items() if k != "batch_size"}
    t = Trainer(**{k: v for k, v in c["trainer"].items() if k != "_target_"})
    assert t.accumulate_grad_batches == 2 and t.gradient_clip_val == 1.0


# ---------------------------------------------------------------- the GPU test's bounds
CASES = [(n, offs, mode, acc) for n in SIZES for offs in OFFS for mode in MODES for acc in (False, True)]


@pytest.fixture(scope="module")
def figures():
    """Per case of tests/test_gpu_adam.py: rel-L2 of the fp32 formula against fp64 Adam, and of
    fp64 AdamW against fp64 Adam, in p, m, v (computed once)."""
    out = {}
    for n, offs, mode, acc in CASES:
        host, s64, cv = case(n, offs, mode, acc)
        c64 = clipped64(s64, mode, cv)
        ref = adam64(host, c64)
        f32, w64 = formula32(host, mode, cv, acc), adam64(host, c64, decoupled=True)
        out[n, offs, mode, acc] = ({k: rel(f32[k], ref[k]) for k in "pmv"}, {k: rel(w64[k], ref[k]) for k in "pmv"})
    return out


def test_fp32_formula_is_inside_the_gpu_bound(figures):
    worst = {k: max(f[0][k] for f in figures.values()) for k in "pmv"}
    print("fp32 formula vs fp64 Adam, worst rel-L2 over the GPU test's cases:", worst)
    for key, (env, _) in figures.items():
        for k in "pmv":
            assert env[k] <= BOUND, (key, k, env[k])


def test_decoupled_decay_is_far_outside_the_gpu_bound(figures):
    assert WD == 0.2
    least = {k: min(f[1][k] for f in figures.values()) for k in "pmv"}
    print("fp64 AdamW vs fp64 Adam, least rel-L2 over the GPU test's cases:", least)
    for key, (_, apart) in figures.items():
        for k in "pmv":
            assert apart[k] >= 100 * BOUND, (key, k, apart[k])
