"""torch.optim.Adam on the device (configs/optimizer/adam.yaml), with clipping and accumulation
fused into the step:

  vlp_adam_step   s = acc ? fma(w, g, acc) : g;  c = s * coef | clamp(s) | s;  gd = fma(wd, p, c);
                  the AdamW kernels' moment and parameter update on gd, no decay of p
  FusedAdam       FusedAdamW with that launch in place of vlp_adamw / _clip / _clip_accum

Inputs of the kernel tests: tests/test_gpu_grad_accum.py's adam_host (p ~ N(0, 1), gradients
and accumulator of 1e-7 and 1 interleaved, moments of 1e-2 / 1e-3), weight decay 0.2.

Bounds.
  against fp64: p, exp_avg, exp_avg_sq within 1e-6 (rel-L2) of torch.optim.Adam's arithmetic in
    fp64, the envelope of the AdamW twin (tests/test_gpu_grad_accum.py).  tests/test_adam_cpu.py
    evaluates the kernel's formula with fp32 torch ops on these very inputs and finds it inside
    that bound, and finds fp64 AdamW (decoupled decay, same wd) at least 1e-4 away in p,
    exp_avg and exp_avg_sq: a decoupled implementation cannot pass.  That margin is why these
    cases run at lr = 1e-2: the two parameter updates differ by terms proportional to lr, and at
    1e-3 the closest case (n = 3) is 7e-5 apart in p.
  stores: with an accumulator g and acc keep their bits; without, modes norm / value leave the
    clipped gradient in g, which is exact (a power-of-two coefficient, a clamp): equal bits;
    mode none leaves g alone.  The guards around every operand stay NaN.
  wd = 0: equal bits with vlp_adamw, vlp_adamw_clip or vlp_adamw_clip_accum (one shared update
    function; the L2 term fma(0, p, c) is c).
  optimizer, module, Trainer: parameter deltas within 3e-3 (rel-L2) of torch.optim.Adam's, the
    tolerance of the fused-vs-torch AdamW tests (tests/test_gpu_model.py).
"""
import copy
import functools
import math

import pytest
import torch

from oracle import weights as W
from tests.golden.synth import synth_batch
from tests.test_gpu_grad_accum import adam_device, adam_host, bits
from tests.test_gpu_grad_clip import DYADIC, HYP, flat, grad_norm64, mixed, rel, tiny_arena_module, ulp_diff

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 1023, 1024 * 256 + 7]
OFFS = [(0, 0), (1, 1), (0, 1)]       # (p / m / v / acc, g) offsets in floats; mixed: the all-scalar path
MODES = ["none", "norm", "value"]
WD, STEP, W_FRESH, COEF = 0.2, 3, 1.0 / 3.0, 0.25
LR = 1e-2       # against fp64: at 1e-3 Adam and AdamW are as close as 7e-5 in p for some n = 3 inputs; see below
BOUND = 1e-6


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def ops():
    from vlp_amd import ops as o
    return o


# ---------------------------------------------------------------- the cases and their references (host only)
def f32(x):
    """The fp32 value the kernel receives for the Python float x."""
    return torch.tensor(x, dtype=torch.float32).double().item()


def case(n, offs, mode, acc):
    """Host inputs of one kernel case and its clip value (an fp32 number: 0.4 of the largest
    gradient magnitude, so some elements are clamped and some are not)."""
    host = adam_host(n, 7 * n + offs[0])
    if not acc:
        del host["a"]
    s64 = host["a"].double() + f32(W_FRESH) * host["g"].double() if acc else host["g"].double()
    cv = f32(0.4 * s64.abs().max().item())
    return host, s64, cv


def clipped64(s64, mode, cv):
    return s64 * COEF if mode == "norm" else s64.clamp(-cv, cv) if mode == "value" else s64


def adam64(host, c64, betas=DYADIC, lr=LR, eps=HYP["eps"], wd=WD, step=STEP, decoupled=False):
    """torch.optim.Adam's step in fp64 on the clipped gradient c64 (decoupled: torch.optim.AdamW's)."""
    b1, b2 = betas
    p = host["p"].double()
    gd = c64 if decoupled else c64 + wd * p
    m = b1 * host["m"].double() + (1 - b1) * gd
    v = b2 * host["v"].double() + (1 - b2) * gd * gd
    p = (p * (1 - lr * wd) if decoupled else p) - lr / (1 - b1 ** step) * m / (v.sqrt() / math.sqrt(1 - b2 ** step) + eps)
    return {"p": p, "m": m, "v": v}


def formula32(host, mode, cv, acc, betas=DYADIC, lr=LR, eps=HYP["eps"], wd=WD, step=STEP):
    """The formula of include/vlp_hip.h (vlp_adam_step) with torch fp32 ops, one rounding each."""
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    b1, b2 = f(betas[0]), f(betas[1])
    p, g, m, v = host["p"], host["g"], host["m"], host["v"]
    s = torch.addcmul(host["a"].double(), f(W_FRESH).double(), g.double()).float() if acc else g   # one fma
    c = s * f(COEF) if mode == "norm" else s.clamp(-cv, cv) if mode == "value" else s
    gd = torch.addcmul(c.double(), f(wd).double(), p.double()).float()                               # one fma
    m = m + (1 - b1) * (gd - m)
    v = v * b2 + (1 - b2) * gd * gd
    step_size, bc2_sqrt = f(lr / (1 - betas[0] ** step)), f(math.sqrt(1 - betas[1] ** step))
    p = p - step_size * (m / (v.sqrt() / bc2_sqrt + f(eps)))
    return {"p": p, "m": m, "v": v}


def clip_kw(mode, cv):
    return dict(coef=torch.tensor([COEF], device="cuda")) if mode == "norm" else dict(clip_value=cv) if mode == "value" else {}


# ---------------------------------------------------------------- vlp_adam_step
@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("offs", OFFS)
@pytest.mark.parametrize("n", SIZES)
def test_adam_step_against_fp64_adam(ops, n, offs, mode, acc):
    host, s64, cv = case(n, offs, mode, acc)
    c64 = clipped64(s64, mode, cv)
    ref = adam64(host, c64)
    runs = []
    for _ in range(2):
        d = adam_device(host, offs)
        kw = dict(acc=d["a"].v, w=W_FRESH) if acc else {}
        ops.adam_step(d["p"].v, d["g"].v, d["m"].v, d["v"].v, LR, DYADIC[0], DYADIC[1], HYP["eps"], WD, STEP,
                      **kw, **clip_kw(mode, cv))
        torch.cuda.synchronize()
        assert all(x.guards_untouched() for x in d.values())
        if acc:
            assert torch.equal(bits(d["g"].v), bits(host["g"])) and torch.equal(bits(d["a"].v), bits(host["a"]))
        else:       # the clipped gradient, never the one with the L2 term
            assert torch.equal(bits(d["g"].v), bits(c64.float())), "g is not the clipped gradient"
        runs.append({k: d[k].v.cpu() for k in "pmv"})
    r = {k: rel(runs[0][k], ref[k]) for k in "pmv"}
    print(f"n {n} offs {offs} {mode} acc {acc}: rel-L2 vs fp64 Adam {r}")
    assert all(torch.isfinite(runs[0][k]).all() for k in "pmv")
    for k in "pmv":
        assert r[k] <= BOUND, (k, r[k])
        assert torch.equal(bits(runs[0][k]), bits(runs[1][k])), k              # reproducible
    assert not torch.equal(runs[0]["p"], host["p"])


def adamw_twin(ops, d, args, mode, cv, acc):
    """The AdamW entry point FusedAdamW launches for this case."""
    t = (d["p"].v, d["g"].v, d["m"].v, d["v"].v)
    if acc:
        ops.adamw_clip_accum(*t, *args, acc=d["a"].v, w=W_FRESH, **clip_kw(mode, cv))
    elif mode == "none":
        ops.adamw(*t, *args)
    else:
        ops.adamw_clip(*t, *args, **clip_kw(mode, cv))


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("offs", OFFS)
@pytest.mark.parametrize("n", SIZES)
def test_adam_step_without_weight_decay_is_the_adamw_family(ops, n, offs, mode, acc):
    host, _, cv = case(n, offs, mode, acc)
    args = (HYP["lr"], 0.9, 0.999, HYP["eps"], 0.0, STEP)
    a, b = adam_device(host, offs), adam_device(host, offs)
    adamw_twin(ops, a, args, mode, cv, acc)
    kw = dict(acc=b["a"].v, w=W_FRESH) if acc else {}
    ops.adam_step(b["p"].v, b["g"].v, b["m"].v, b["v"].v, *args, **kw, **clip_kw(mode, cv))
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(bits(a[k].v), bits(b[k].v)), k
        assert b[k].guards_untouched(), k
    assert not torch.equal(b["p"].v.cpu(), host["p"])
    # and the weight decay is not a no-op: with it the moments move
    c = adam_device(host, offs)
    kw = dict(acc=c["a"].v, w=W_FRESH) if acc else {}
    ops.adam_step(c["p"].v, c["g"].v, c["m"].v, c["v"].v, *args[:4], WD, STEP, **kw, **clip_kw(mode, cv))
    torch.cuda.synchronize()
    assert ulp_diff(c["m"].v, b["m"].v).max().item() > 2 and torch.equal(bits(c["g"].v), bits(b["g"].v))


def test_adam_step_rejects_bad_arguments(ops):
    from vlp_amd._lib import lib, stream_of
    raw = lib()._fns["vlp_adam_step"]
    t = [torch.ones(4, device="cuda") for _ in range(5)]
    ptrs = [x.data_ptr() for x in t[:4]]
    acc = t[4].data_ptr()
    tail = (1e-3, 0.9, 0.999, 1e-8, 0.2, 1e-2, 0.03)
    st = stream_of()
    inval = 1                                             # hipErrorInvalidValue
    for a in (acc, None):
        assert raw(4, *ptrs, *tail, 3, None, 1.0, a, 1.0, st) == inval
        assert raw(4, *ptrs, *tail, -1, None, 1.0, a, 1.0, st) == inval
        assert raw(4, *ptrs, *tail, 1, None, 1.0, a, 1.0, st) == inval      # norm mode without a coefficient
        for i in range(4):
            q = list(ptrs)
            q[i] = None
            assert raw(4, *q, *tail, 0, None, 1.0, a, 1.0, st) == inval
            q[i] = ptrs[i] + 2                                                 # not a float address
            assert raw(4, *q, *tail, 2, None, 1.0, a, 1.0, st) == inval
        for n in (0, -5):
            assert raw(n, *ptrs, *tail, 0, None, 1.0, a, 1.0, st) == 0
            assert raw(n, None, None, None, None, *tail, 2, None, 1.0, a, 1.0, st) == 0
    assert raw(4, *ptrs, *tail, 0, None, 1.0, acc + 2, 1.0, st) == inval
    torch.cuda.synchronize()
    assert all((x == 1).all() for x in t)                 # nothing was launched
    ops.adam_step(t[0][:0], t[1][:0], t[2][:0], t[3][:0], 1e-3, 0.9, 0.999, 1e-8, 0.2, 1)
    with pytest.raises(ValueError):
        ops.adam_step(*t[:4], 1e-3, 0.9, 0.999, 1e-8, 0.2, 1, coef=t[0], clip_value=1.0)
    with pytest.raises(ValueError):
        ops.adam_step(*t[:4], 1e-3, 0.9, 0.999, 1e-8, 0.2, 1, acc=t[4][:2])
    with pytest.raises(TypeError):
        ops.adam_step(t[0].double(), *t[1:4], 1e-3, 0.9, 0.999, 1e-8, 0.2, 1)
    torch.cuda.synchronize()
    assert all((x == 1).all() for x in t)


# ---------------------------------------------------------------- optimizer
GROUPS = (("w", "b", "d"), ("c", "e"))      # "d" never has a gradient
LRS = (1e-3, 1e-2)


def _tiny_pair():
    """The tiny arena module under FusedAdam (two groups of different lr, weight decay 0.2) and
    torch.optim.Adam on clones; micro(i) gives micro-batch i's gradients."""
    from vlp_amd.optim import FusedAdam
    m = tiny_arena_module()
    ps = dict(m.named_parameters())
    opt = FusedAdam([{"params": [ps[k] for k in ks], "lr": lr} for ks, lr in zip(GROUPS, LRS)], weight_decay=WD,
                    arenas=[m])
    names = [k for k in ps if k != "d"]
    ref = {k: torch.nn.Parameter(ps[k].detach().clone()) for k in names}
    topt = torch.optim.Adam([{"params": [ref[k] for k in ks if k != "d"], "lr": lr} for ks, lr in zip(GROUPS, LRS)],
                            weight_decay=WD)

    def micro(i):
        return {k: mixed(ps[k].numel(), 100 * i + j).view(ps[k].shape).cuda() * 1e-3 for j, k in enumerate(names)}
    return m, ps, opt, ref, topt, names, micro


def _cat(d, names):
    return torch.cat([d[k].detach().double().flatten().cpu() for k in names])


def _backward_into_arena(m, ps, grads):
    """What the towers' backward leaves: the arena overwritten, p.grad a view of it."""
    for k, g in grads.items():
        m.arena.gview(k).copy_(g)
        ps[k].grad = m.arena.gview(k)


def _torch_clip(params, algo, val):
    if algo == "norm":
        torch.nn.utils.clip_grad_norm_(params, val)
    elif algo == "value":
        torch.nn.utils.clip_grad_value_(params, val)


@pytest.mark.parametrize("algo", [None, "norm", "value"])
def test_fused_adam_matches_torch_adam(algo):
    from vlp_amd.optim import FusedAdam
    m, ps, opt, ref, topt, names, micro = _tiny_pair()
    p0, d0 = _cat(ps, names), ps["d"].detach().clone()
    g0 = micro(0)
    n0 = math.sqrt(sum(g.double().pow(2).sum().item() for g in g0.values()))
    val = None if algo is None else 0.5 * n0 if algo == "norm" else 0.3 * max(g.abs().max().item() for g in g0.values())
    opt.set_gradient_clipping(val, algo or "norm")

    def torch_step(mbs):
        """torch: the micro-batches summed in p.grad as autograd sums them, clip, step."""
        for k in names:
            tot = mbs[0][k].clone()
            for g in mbs[1:]:
                tot = tot + g[k]
            ref[k].grad = tot
        _torch_clip(list(ref.values()), algo, val)
        topt.step()

    # three plain steps
    for i in range(3):
        _backward_into_arena(m, ps, micro(i))
        torch_step([micro(i)])
        opt.step()
    torch.cuda.synchronize()
    r3 = rel(_cat(ps, names) - p0, _cat(ref, names) - p0)
    # one step from three micro-batches, the last one fresh; then one with all three folded
    rs = []
    for fold in (False, True):
        p1 = _cat(ps, names)
        q1 = _cat(ref, names)
        mbs = [micro(10 + i + (5 if fold else 0)) for i in range(3)]
        torch_step(mbs)
        for i, mb in enumerate(mbs):
            _backward_into_arena(m, ps, mb)
            if i < 2 or fold:
                opt.accumulate(1.0, first=i == 0)
                for k in names:                          # the next backward owes nothing to this one
                    m.arena.gview(k).fill_(float("nan"))
        opt.step()
        torch.cuda.synchronize()
        assert opt._pending is None
        rs.append(rel(_cat(ps, names) - p1, _cat(ref, names) - q1))
    print(f"{algo}: parameter delta rel-L2 vs torch.optim.Adam: three steps {r3:.3e}, three micro-batches "
          f"(last fresh) {rs[0]:.3e}, (all folded) {rs[1]:.3e}")
    assert r3 < 3e-3 and rs[0] < 3e-3 and rs[1] < 3e-3
    assert torch.equal(ps["d"], d0) and ps["d"] not in opt.state          # no gradient: skipped
    if algo == "norm":
        assert opt.last_grad_norm is not None and opt.last_grad_norm.item() > val
    # the state dict goes through torch.optim.Adam and back, and the next step still agrees
    sd = opt.state_dict()
    st = sd["state"][0]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 5.0
    tparams = {k: torch.nn.Parameter(ps[k].detach().clone()) for k in ps}
    t2 = torch.optim.Adam([{"params": [tparams[k] for k in ks], "lr": lr} for ks, lr in zip(GROUPS, LRS)], weight_decay=WD)
    t2.load_state_dict(copy.deepcopy(sd))      # torch keeps the tensors it is given: not the fused optimizer's own
    assert type(t2) is torch.optim.Adam and t2.param_groups[0]["weight_decay"] == WD
    m2 = tiny_arena_module()
    ps2 = dict(m2.named_parameters())
    with torch.no_grad():
        for k in ps:
            ps2[k].copy_(ps[k])
    o2 = FusedAdam([{"params": [ps2[k] for k in ks], "lr": lr} for ks, lr in zip(GROUPS, LRS)], weight_decay=WD,
                   arenas=[m2])
    o2.load_state_dict(t2.state_dict())
    o2.set_gradient_clipping(val, algo or "norm")
    p5 = _cat(ps, names)
    g = micro(30)
    for k in names:
        tparams[k].grad = g[k].clone()
    _torch_clip([tparams[k] for k in names], algo, val)
    t2.step()
    _backward_into_arena(m2, ps2, g)
    o2.step()
    _backward_into_arena(m, ps, g)
    opt.step()
    torch.cuda.synchronize()
    r_t, r_f = rel(_cat(ps2, names) - p5, _cat(tparams, names) - p5), rel(_cat(ps2, names) - p5, _cat(ps, names) - p5)
    print(f"{algo}: step 6 after the round trip: vs torch.optim.Adam fed the fused state {r_t:.3e}, vs the optimizer "
          f"that never left {r_f:.3e}")
    assert r_t < 3e-3 and r_f == 0.0
    assert float(o2.state_dict()["state"][0]["step"]) == 6.0


def test_fused_adam_rejects_amsgrad_and_maximize():
    from vlp_amd.optim import FusedAdam
    m = tiny_arena_module()
    for kw in (dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(ValueError, match="amsgrad"):
            FusedAdam(m.parameters(), arenas=[m], **kw)
    assert FusedAdam(m.parameters(), arenas=[m]).defaults["weight_decay"] == 0


# ---------------------------------------------------------------- module and Trainer
B, H, T = 4, 64, 12


def recipe_module(fused, **adam_kw):
    from src.models.pretrain.VisionLanguageModule import VisionLanguageModule
    m = VisionLanguageModule("resnet34", "tinybert", functools.partial(torch.optim.Adam, lr=1e-3, weight_decay=WD, **adam_kw),
                             False, False, 512, 312, 128, compute_dtype="fp32", text_dropout=0.0,
                             fused_optimizer=fused)
    W.apply_recipe(m, 0)
    m.train()
    return m


def test_module_steps_with_fused_adam_like_torch_adam():
    from vlp_amd.optim import FusedAdam
    batch = synth_batch(B, H, T, 0)
    mf, mt = recipe_module(True), recipe_module(False)
    of, ot = mf.configure_optimizers()["optimizer"], mt.configure_optimizers()["optimizer"]
    assert type(of) is FusedAdam and type(ot) is torch.optim.Adam
    assert [g["weight_decay"] for g in of.param_groups] == [g["weight_decay"] for g in ot.param_groups]
    p0 = flat(mf)
    assert torch.equal(p0, flat(mt))
    for mod, o in ((mf, of), (mt, ot)):
        o.zero_grad()
        mod.training_step(batch).backward()
        o.step()
    torch.cuda.synchronize()
    r = rel(flat(mf) - p0, flat(mt) - p0)
    print("one Adam step (weight decay 0.2), parameter delta rel-L2 fused vs torch:", r)
    assert r < 3e-3, r


def test_trainer_accumulates_two_micro_batches_with_fused_adam_like_torch(tmp_path):
    """accumulate_grad_batches=2 with clipping through the Trainer and FusedAdam, against two
    backward passes at loss / 2 without zero_grad, clip_grad_norm_ and torch.optim.Adam."""
    from src.utils.trainer import Trainer
    from vlp_amd.optim import FusedAdam
    batches = [synth_batch(B, H, T, s) for s in (0, 1)]
    mt = recipe_module(False, betas=DYADIC)
    ot = mt.configure_optimizers()["optimizer"]
    assert type(ot) is torch.optim.Adam
    p0 = flat(mt)
    for b in batches:
        (mt.training_step(b) / 2).backward()
    n0 = grad_norm64(mt.parameters())
    v = 0.5 * n0
    torch.nn.utils.clip_grad_norm_([p for p in mt.parameters() if p.grad is not None], v)
    ot.step()
    mf = recipe_module(True, betas=DYADIC)
    assert torch.equal(flat(mf), p0)
    mf.k_for_precision_at_k = mf.k_for_image_text_retreival = [3]      # 8 cached samples at the epoch end
    conf = mf.configure_optimizers()
    of = conf["optimizer"]
    assert type(of) is FusedAdam
    calls, plain_step, plain_acc = [], of.step, of.accumulate
    of.step = lambda *a, **k: (calls.append("step"), plain_step(*a, **k))[1]
    of.accumulate = lambda *a, **k: (calls.append("accumulate"), plain_acc(*a, **k))[1]
    mf.configure_optimizers = lambda: conf
    t = Trainer(accumulate_grad_batches=2, gradient_clip_val=v, max_epochs=1, enable_checkpointing=False,
                default_root_dir=str(tmp_path))
    t.fit(mf, train_dataloaders=batches)
    torch.cuda.synchronize()
    assert calls == ["accumulate", "step"] and t.global_step == 1
    d_f, d_t = flat(mf) - p0, flat(mt) - p0
    norm = t.logged_metrics["grad_norm"]
    print(f"accumulated norm: fused {norm:.9g} torch {n0:.9g}; parameter delta rel-L2 vs torch {rel(d_f, d_t):.3e}")
    # the norm that was clipped is the accumulated gradient's (one micro-batch's is nowhere near)
    assert abs(norm - n0) <= 1e-3 * n0
    assert rel(d_f, d_t) < 3e-3, rel(d_f, d_t)
