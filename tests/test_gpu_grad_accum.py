"""Gradient accumulation on the device (Lightning's accumulate_grad_batches) for the flat
gradient arenas, which every backward overwrites:

  vlp_grad_accum        acc = (first ? 0 : acc) + w g, one fused multiply-add per element
  vlp_grad_accum_sumsq  vlp_grad_sumsq's fp64 partials of s = fma(w, g, acc), s never stored
  vlp_adamw_clip_accum  vlp_adamw_clip's update on s; acc == NULL: vlp_adamw_clip itself

Inputs.  acc and g hold, element by element, values of one magnitude (tests/test_gpu_grad_clip.py's
`mixed`: 1e-4 and 1e3 interleaved), and w is 1, 0.25 or fp32(1/3): w g has at most 48
significant bits and acc + w g at most a few more, so the fp64 expression acc + w g is exact and
its rounding to fp32 is the fma's single rounding.  That is the "s32" the checks below use where
they need the kernel's own fp32 gradient.

Bounds.
  accumulate: one fma, |err| <= 2 eps32 (|acc| + |w g|) with eps32 = 2^-23, against fp64.
  partials / norm: tests/test_gpu_grad_clip.py's: each partial within 4e-12 (relative) of the
    fp64 sum of s32^2 over its segment; the norm within 1 fp32 ulp (2^-23, relative) of the fp64
    norm of acc + w g (rounding s costs at most 2^-24 of it, the norm's own rounding 2^-24 more).
  update: that file's: first-step moments <= 2 ulp from torch.optim.AdamW fed the fp32 gradient
    fl(s32 * coef) (betas with exact 1 - beta, see that file's docstring); p, exp_avg, exp_avg_sq
    within 1e-6 (rel-L2) of fp64 AdamW on coef (acc + w g); acc == NULL: vlp_adamw_clip's bits.
  module: the parameter deltas of one accumulated, clipped step within 3e-3 (rel-L2) of
    torch's, the tolerance of tests/test_gpu_model.py's fused-vs-torch AdamW test.
"""
import ctypes
import math

import pytest
import torch

from oracle import weights as W
from tests.golden.synth import synth_batch
from tests.test_gpu_grad_clip import (DYADIC, HYP, SEG, ULP, flat, grad_norm64, mixed, rel,
                                      tiny_arena_module, torch_adamw_step, ulp_diff)

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 1023, 1024 * 256 + 7]
OFFS = [(0, 0), (1, 1), (0, 1)]      # (accumulator / state, gradient) offsets in floats; mixed: the scalar path
EPS32 = 2.0 ** -23
WS = [1.0, 1.0 / 3.0]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def ops():
    from vlp_amd import ops as o
    return o


def w64(w):
    return torch.tensor(w, dtype=torch.float32).double().item()


class Guarded:
    """A span at element offset `off` of a NaN-filled, 16-B aligned device buffer."""

    def __init__(self, n, off, vals=None):
        self.buf = torch.full((n + 8,), float("nan"), device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.n, self.off = n, off
        self.v = self.buf[off:off + n]
        if vals is not None:
            self.v.copy_(vals)

    def guards_untouched(self):
        b = self.buf.cpu()
        return bool(torch.isnan(b[:self.off]).all() and torch.isnan(b[self.off + self.n:]).all())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------- vlp_grad_accum
@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("offs", OFFS)
@pytest.mark.parametrize("n", SIZES)
def test_accumulate_against_fp64(ops, n, offs, w):
    g1, g2 = mixed(n, 11 * n + offs[1]), mixed(n, 13 * n + 1)
    runs = []
    for _ in range(2):
        acc = Guarded(n, offs[0])                       # NaN inside too: first must not read it
        d1, d2 = Guarded(n, offs[1], g1), Guarded(n, offs[1], g2)
        ops.grad_accum(acc.v, d1.v, w, first=True)
        torch.cuda.synchronize()
        a1 = acc.v.cpu()
        ops.grad_accum(acc.v, d2.v, 0.25, first=False)
        torch.cuda.synchronize()
        a2 = acc.v.cpu()
        assert acc.guards_untouched() and d1.guards_untouched() and d2.guards_untouched()
        assert torch.equal(bits(d1.v), bits(g1)) and torch.equal(bits(d2.v), bits(g2))
        runs.append((a1, a2))
    (a1, a2), (b1, b2) = runs
    assert torch.isfinite(a1).all() and torch.isfinite(a2).all()
    ref1 = w64(w) * g1.double()
    bound1 = 2 * EPS32 * ref1.abs()
    err1 = (a1.double() - ref1).abs()
    ref2 = a1.double() + 0.25 * g2.double()
    bound2 = 2 * EPS32 * (a1.double().abs() + (0.25 * g2.double()).abs())
    err2 = (a2.double() - ref2).abs()
    print(f"n {n} offs {offs} w {w:.3g}: first err/bound {(err1 / bound1).max().item():.3f}, "
          f"second err/bound {(err2 / bound2).max().item():.3f}")
    assert (err1 <= bound1).all()
    assert (err2 <= bound2).all()
    assert torch.equal(bits(a1), bits(b1)) and torch.equal(bits(a2), bits(b2))      # reproducible


def test_accumulate_rejects_null_and_ignores_empty(ops):
    from vlp_amd._lib import lib, stream_of
    raw = lib()._fns["vlp_grad_accum"]
    st = stream_of()
    a, g = torch.full((8,), 7.0, device="cuda"), torch.ones(8, device="cuda")
    inval = 1                                             # hipErrorInvalidValue
    assert raw(8, None, g.data_ptr(), 1.0, 1, st) == inval
    assert raw(8, a.data_ptr(), None, 1.0, 0, st) == inval
    assert raw(8, a.data_ptr() + 2, g.data_ptr(), 1.0, 0, st) == inval      # not a float address
    for n in (0, -5):
        assert raw(n, None, None, 1.0, 1, st) == 0
        assert raw(n, a.data_ptr(), g.data_ptr(), 1.0, 1, st) == 0
    torch.cuda.synchronize()
    assert (a == 7.0).all()                               # nothing was launched
    with pytest.raises(ValueError):
        ops.grad_accum(a, g[:4])
    with pytest.raises(TypeError):
        ops.grad_accum(a.double(), g)


# ---------------------------------------------------------------- vlp_grad_accum_sumsq
@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("offs", OFFS)
@pytest.mark.parametrize("n", SIZES)
def test_accumulated_norm_against_fp64(ops, n, offs, w):
    a, g = mixed(n, 17 * n + offs[0]), mixed(n, 19 * n + 2)
    acc, dg = Guarded(n, offs[0], a), Guarded(n, offs[1], g)
    s64 = a.double() + w64(w) * g.double()                # exact (module docstring)
    s32 = s64.float()
    ref = s64.pow(2).sum().sqrt().item()
    k = ops.grad_sumsq_nparts(n)
    runs = []
    for _ in range(2):
        partials = torch.full((k + 2,), float("nan"), dtype=torch.float64, device="cuda")
        out = torch.full((2,), float("nan"), device="cuda")
        assert ops.grad_accum_sumsq(acc.v, dg.v, w, partials) == k
        ops.clip_coef(k, partials, 0.5 * ref, out)       # consumed as vlp_grad_sumsq's partials are
        torch.cuda.synchronize()
        runs.append((partials.cpu(), out.cpu()))
    (p0, o0), (p1, o1) = runs
    assert torch.isnan(p0[k:]).all(), "wrote past its partials"
    assert torch.equal(bits(acc.v), bits(a)) and torch.equal(bits(dg.v), bits(g))   # inputs left alone
    assert acc.guards_untouched() and dg.guards_untouched()
    seg_ref = torch.stack([c.double().pow(2).sum() for c in s32.split(SEG)])
    err = ((p0[:k] - seg_ref).abs() / seg_ref).max().item()
    print(f"n {n} offs {offs} w {w:.3g}: partials rel err {err:.2e}, norm {o0[0].item():.9g} ref {ref:.9g} "
          f"rel {abs(o0[0].item() - ref) / ref:.2e}")
    assert err <= 4e-12
    assert abs(o0[0].double().item() - ref) <= ULP * ref
    assert 0.49 < o0[1].item() < 0.51
    assert torch.equal(p0[:k].view(torch.int64), p1[:k].view(torch.int64))
    assert torch.equal(bits(o0), bits(o1))


def test_accumulated_norm_with_zero_weight_is_grad_sumsq_of_acc(ops):
    """w = 0: s = acc exactly, and the segments and the order of the sums are vlp_grad_sumsq's."""
    n = 3 * SEG + 5
    a = Guarded(n, 1, mixed(n, 3))
    g = Guarded(n, 1, mixed(n, 4))
    k = ops.grad_sumsq_nparts(n)
    p0 = torch.zeros(k, dtype=torch.float64, device="cuda")
    p1 = torch.zeros(k, dtype=torch.float64, device="cuda")
    assert ops.grad_sumsq(a.v, p0) == k and ops.grad_accum_sumsq(a.v, g.v, 0.0, p1) == k
    torch.cuda.synchronize()
    assert torch.equal(p0.cpu().view(torch.int64), p1.cpu().view(torch.int64))


def test_accumulated_norm_rejects_null_and_small_buffers(ops):
    from vlp_amd._lib import lib, stream_of
    raw = lib()._fns["vlp_grad_accum_sumsq"]
    st = stream_of()
    k = ctypes.c_int(-1)
    partials = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    a, g = torch.ones(8, device="cuda"), torch.ones(8, device="cuda")
    assert raw(0, None, None, 1.0, None, ctypes.byref(k), st) == 0 and k.value == 0
    for args in ((None, g.data_ptr(), 1.0, partials.data_ptr(), ctypes.byref(k)),
                 (a.data_ptr(), None, 1.0, partials.data_ptr(), ctypes.byref(k)),
                 (a.data_ptr(), g.data_ptr(), 1.0, None, ctypes.byref(k)),
                 (a.data_ptr(), g.data_ptr(), 1.0, partials.data_ptr(), None)):
        assert raw(8, *args, st) == 1
    torch.cuda.synchronize()
    assert (partials == 7.0).all()
    with pytest.raises(ValueError):
        ops.grad_accum_sumsq(torch.ones(SEG + 1, device="cuda"), torch.ones(SEG + 1, device="cuda"), 1.0, partials, 3)


# ---------------------------------------------------------------- vlp_adamw_clip_accum
def adam_host(n, seed):
    g = torch.Generator().manual_seed(seed)
    return {"p": torch.randn(n, generator=g), "g": mixed(n, seed + 1) * 1e-3, "a": mixed(n, seed + 2) * 1e-3,
            "m": torch.randn(n, generator=g) * 1e-2, "v": torch.rand(n, generator=g) * 1e-3}


def adam_device(host, offs):
    return {k: Guarded(t.numel(), offs[1] if k == "g" else offs[0], t) for k, t in host.items()}


def clip64(s64, mode, c, cv):
    return s64 * c if mode == "norm" else s64.clamp(-cv, cv) if mode == "value" else s64


def clip_kw(mode, c, cv):
    return dict(coef=torch.tensor([c], device="cuda")) if mode == "norm" else dict(clip_value=cv) if mode == "value" else {}


@pytest.mark.parametrize("mode", ["norm", "value", "none"])
@pytest.mark.parametrize("offs", OFFS)
@pytest.mark.parametrize("n", SIZES)
def test_adamw_clip_accum_against_fp64_adamw(ops, n, offs, mode):
    w, c, step = 1.0 / 3.0, 0.25, 3
    host = adam_host(n, 7 * n + offs[0])
    s64 = host["a"].double() + w64(w) * host["g"].double()
    cv = 0.4 * s64.abs().max().item()
    gc = clip64(s64, mode, c, cv)
    b1, b2 = DYADIC
    lr, eps, wd = HYP["lr"], HYP["eps"], HYP["wd"]
    m64 = b1 * host["m"].double() + (1 - b1) * gc
    v64 = b2 * host["v"].double() + (1 - b2) * gc * gc
    p64 = host["p"].double() * (1 - lr * wd) - lr / (1 - b1 ** step) * m64 / (v64.sqrt() / math.sqrt(1 - b2 ** step) + eps)
    runs = []
    for _ in range(2):
        d = adam_device(host, offs)
        ops.adamw_clip_accum(d["p"].v, d["g"].v, d["m"].v, d["v"].v, lr, b1, b2, eps, wd, step, acc=d["a"].v, w=w,
                             **clip_kw(mode, c, cv))
        torch.cuda.synchronize()
        assert all(x.guards_untouched() for x in d.values())
        assert torch.equal(bits(d["g"].v), bits(host["g"])) and torch.equal(bits(d["a"].v), bits(host["a"]))
        runs.append({k: d[k].v.cpu() for k in "pmv"})
    r = {k: rel(runs[0][k], ref) for k, ref in (("p", p64), ("m", m64), ("v", v64))}
    dp = rel(runs[0]["p"].double() - host["p"].double(), p64 - host["p"].double())
    print(f"n {n} offs {offs} {mode}: rel-L2 vs fp64 {r}, parameter delta {dp:.2e}")
    assert all(torch.isfinite(runs[0][k]).all() for k in "pmv")
    for k in "pmv":
        assert r[k] <= 1e-6, (k, r[k])
        assert torch.equal(bits(runs[0][k]), bits(runs[1][k])), k              # reproducible
    assert not torch.equal(runs[0]["p"], host["p"])


@pytest.mark.parametrize("mode", ["norm", "value", "none"])
@pytest.mark.parametrize("offs", OFFS)
@pytest.mark.parametrize("n", SIZES)
def test_adamw_clip_accum_first_step_moments_vs_torch(ops, n, offs, mode):
    """From zero moments exp_avg = (1 - b1) gc and exp_avg_sq = (1 - b2) gc^2 with gc the fp32
    gradient torch would hold: fl(s32 * 0.25), clamp(s32) or s32."""
    w, c = 1.0 / 3.0, 0.25
    host = adam_host(n, 5 * n + offs[0])
    host["m"].zero_()
    host["v"].zero_()
    s32 = (host["a"].double() + w64(w) * host["g"].double()).float().cuda()
    cv = 0.4 * s32.abs().max().item()
    gc = s32 * c if mode == "norm" else s32.clamp(-cv, cv) if mode == "value" else s32
    assert mode != "value" or n < 3 or 0 < (s32.abs() > cv).sum().item() < n
    d = adam_device(host, offs)
    ops.adamw_clip_accum(d["p"].v, d["g"].v, d["m"].v, d["v"].v, HYP["lr"], DYADIC[0], DYADIC[1], HYP["eps"],
                         HYP["wd"], 1, acc=d["a"].v, w=w, **clip_kw(mode, c, cv))
    torch.cuda.synchronize()
    tp, tm, tv = torch_adamw_step(host["p"].cuda(), gc, DYADIC)
    dm, dv, dpp = (ulp_diff(d["m"].v, tm).max().item(), ulp_diff(d["v"].v, tv).max().item(),
                   ulp_diff(d["p"].v, tp).max().item())
    print(f"n {n} offs {offs} {mode}: exp_avg {dm} ulp, exp_avg_sq {dv} ulp, p {dpp} ulp")
    assert dm <= 2 and dv <= 2


@pytest.mark.parametrize("mode", ["norm", "value"])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_adamw_clip_accum_without_accumulator_is_adamw_clip(ops, n, off, mode):
    host = adam_host(n, 3 * n + off)
    del host["a"]
    cv = 0.4 * host["g"].abs().max().item()
    a, b = adam_device(host, (off, off)), adam_device(host, (off, off))
    args = (HYP["lr"], 0.9, 0.999, HYP["eps"], HYP["wd"], 3)
    ops.adamw_clip(a["p"].v, a["g"].v, a["m"].v, a["v"].v, *args, **clip_kw(mode, 0.25, cv))
    ops.adamw_clip_accum(b["p"].v, b["g"].v, b["m"].v, b["v"].v, *args, acc=None, w=5.0, **clip_kw(mode, 0.25, cv))
    torch.cuda.synchronize()
    for k in "pgmv":
        assert torch.equal(bits(a[k].v), bits(b[k].v)), k
        assert b[k].guards_untouched()
    assert not torch.equal(b["g"].v.cpu(), host["g"]) or n < 3         # the clipped gradient was written back


def test_adamw_clip_accum_rejects_bad_arguments(ops):
    from vlp_amd._lib import lib, stream_of
    raw = lib()._fns["vlp_adamw_clip_accum"]
    t = [torch.ones(4, device="cuda") for _ in range(5)]
    ptrs = [x.data_ptr() for x in t[:4]]
    acc = t[4].data_ptr()
    tail = (1e-3, 0.9, 0.999, 1e-8, 0.01, 1e-2, 0.03)
    st = stream_of()
    assert raw(4, *ptrs, *tail, 3, None, 1.0, acc, 1.0, st) == 1
    assert raw(4, *ptrs, *tail, -1, None, 1.0, acc, 1.0, st) == 1
    assert raw(4, *ptrs, *tail, 1, None, 1.0, acc, 1.0, st) == 1            # norm mode without a coefficient
    assert raw(4, *ptrs, *tail, 0, None, 1.0, None, 1.0, st) == 1           # no accumulator: vlp_adamw_clip's modes
    assert raw(4, ptrs[0], None, ptrs[2], ptrs[3], *tail, 2, None, 1.0, acc, 1.0, st) == 1
    assert raw(4, *ptrs, *tail, 0, None, 1.0, acc + 2, 1.0, st) == 1
    assert raw(0, *ptrs, *tail, 0, None, 1.0, acc, 1.0, st) == 0
    torch.cuda.synchronize()
    assert all((x == 1).all() for x in t)
    with pytest.raises(ValueError):
        ops.adamw_clip_accum(*t[:4], 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, acc=None)
    with pytest.raises(ValueError):
        ops.adamw_clip_accum(*t[:4], 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, acc=t[4], coef=t[0], clip_value=1.0)


# ---------------------------------------------------------------- optimizer
def _tiny_pair():
    """The tiny arena module with FusedAdamW (two groups, "d" never has a gradient) and torch
    AdamW on clones; micro(i) gives micro-batch i's gradients."""
    from vlp_amd.optim import FusedAdamW
    m = tiny_arena_module()
    ps = dict(m.named_parameters())
    opt = FusedAdamW([{"params": [ps["w"], ps["b"], ps["d"]], "lr": 1e-3}, {"params": [ps["c"], ps["e"]], "lr": 1e-2}],
                     betas=DYADIC, arenas=[m])
    names = [k for k in ps if k != "d"]
    ref = {k: torch.nn.Parameter(ps[k].detach().clone()) for k in names}
    topt = torch.optim.AdamW([{"params": [ref["w"], ref["b"]], "lr": 1e-3}, {"params": [ref["c"], ref["e"]], "lr": 1e-2}],
                             betas=DYADIC)

    def micro(i):
        return {k: mixed(ps[k].numel(), 100 * i + j).view(ps[k].shape).cuda() * 1e-3 for j, k in enumerate(names)}
    return m, ps, opt, ref, topt, names, micro


def _poison(m, names):
    """NaN in every parameter's gradient (the alignment padding between them stays zero, as the
    arena keeps it): whatever is read before the next backward wrote it shows."""
    for k in names:
        m.arena.gview(k).fill_(float("nan"))


def _backward_into_arena(m, ps, grads):
    """What the towers' backward leaves: the arena overwritten, p.grad a view of it."""
    for k, g in grads.items():
        m.arena.gview(k).copy_(g)
        ps[k].grad = m.arena.gview(k)


@pytest.mark.parametrize("algo", ["norm", "value", None])
@pytest.mark.parametrize("folded", [False, True])
def test_fused_adamw_accumulates_three_micro_batches(algo, folded):
    """accumulate() twice and step() on the third (folded: accumulate() three times and a
    step() without fresh gradients) against torch: three backwards into p.grad, clip, AdamW."""
    m, ps, opt, ref, topt, names, micro = _tiny_pair()
    assert opt._acc == {}
    mbs = [micro(i) for i in range(3)]
    for k in names:
        ref[k].grad = mbs[0][k] + mbs[1][k]
        ref[k].grad = ref[k].grad + mbs[2][k]
    total = {k: ref[k].grad.clone() for k in names}
    n0 = math.sqrt(sum(g.double().pow(2).sum().item() for g in total.values()))
    val = None if algo is None else 0.5 * n0 if algo == "norm" else 0.3 * max(g.abs().max().item() for g in total.values())
    if algo == "norm":
        torch.nn.utils.clip_grad_norm_(list(ref.values()), val)
    elif algo == "value":
        torch.nn.utils.clip_grad_value_(list(ref.values()), val)
    topt.step()
    d0 = ps["d"].detach().clone()
    opt.set_gradient_clipping(val, algo or "norm")
    _poison(m, names)
    for i, mb in enumerate(mbs):
        _backward_into_arena(m, ps, mb)
        if i < 2 or folded:
            opt.accumulate(1.0, first=i == 0)
            assert all(p.grad is None for p in ps.values())
            _poison(m, names)                            # the next backward owes nothing to this one
    opt.step()
    torch.cuda.synchronize()
    assert opt._pending is None and len(opt._acc) == 1
    for k in names:
        assert rel(opt.state[ps[k]]["exp_avg"], topt.state[ref[k]]["exp_avg"]) <= 1e-6, k
        assert rel(opt.state[ps[k]]["exp_avg_sq"], topt.state[ref[k]]["exp_avg_sq"]) <= 1e-6, k
        assert rel(ps[k], ref[k]) <= 1e-6, k
    assert torch.equal(ps["d"], d0)
    if algo == "norm":
        assert abs(opt.last_grad_norm.double().item() - n0) <= ULP * n0
    # a plain step afterwards is the plain step: nothing pending, the fresh gradient alone
    _backward_into_arena(m, ps, mbs[0])
    for k in names:
        ref[k].grad = mbs[0][k].clone()
    if algo == "norm":
        torch.nn.utils.clip_grad_norm_(list(ref.values()), val)
    elif algo == "value":
        torch.nn.utils.clip_grad_value_(list(ref.values()), val)
    topt.step()
    opt.step()
    torch.cuda.synchronize()
    for k in names:
        assert rel(ps[k], ref[k]) <= 1e-6, k


def test_fused_adamw_accumulator_is_lazy_and_checked():
    m, ps, opt, ref, topt, names, micro = _tiny_pair()
    _backward_into_arena(m, ps, micro(0))
    opt.step()
    assert opt._acc == {}                                 # the default path allocates nothing
    with pytest.raises(RuntimeError, match="nothing accumulated"):
        opt.accumulate(1.0, first=False)
    with pytest.raises(RuntimeError, match="nothing accumulated"):
        opt.reduce_accumulated()
    opt.accumulate(1.0, first=True)
    assert opt._acc[id(m.arena)].numel() == m.arena.numel
    part = micro(1)
    del part["c"]
    _backward_into_arena(m, ps, part)
    with pytest.raises(RuntimeError, match="changed between micro-batches"):
        opt.accumulate(1.0, first=False)
    opt.zero_grad()
    assert opt._pending is None
    with pytest.raises(RuntimeError, match="no parameter has a gradient"):
        opt.accumulate(1.0)


# ---------------------------------------------------------------- module and Trainer
B, H, T = 4, 64, 12


def recipe_module(fused):
    import functools
    from src.models.pretrain.VisionLanguageModule import VisionLanguageModule
    m = VisionLanguageModule("resnet34", "tinybert", functools.partial(torch.optim.AdamW, lr=1e-3, betas=DYADIC),
                             False, False, 512, 312, 128, compute_dtype="fp32", text_dropout=0.0,
                             fused_optimizer=fused)
    W.apply_recipe(m, 0)
    m.train()
    return m


def test_trainer_accumulates_two_micro_batches_like_torch(tmp_path):
    """accumulate_grad_batches=2 with clipping through the Trainer and FusedAdamW, against two
    backward passes at loss / 2 without zero_grad, clip_grad_norm_ and torch.optim.AdamW; and
    not the step the last micro-batch alone would give."""
    from src.utils.trainer import Trainer
    from vlp_amd.optim import FusedAdamW
    batches = [synth_batch(B, H, T, s) for s in (0, 1)]
    # torch
    mt = recipe_module(False)
    ot = mt.configure_optimizers()["optimizer"]
    assert type(ot) is torch.optim.AdamW
    p0 = flat(mt)
    for b in batches:
        (mt.training_step(b) / 2).backward()
    n0 = grad_norm64(mt.parameters())
    v = 0.5 * n0
    torch.nn.utils.clip_grad_norm_([p for p in mt.parameters() if p.grad is not None], v)
    ot.step()
    # the last micro-batch alone
    ml = recipe_module(True)
    ol = ml.configure_optimizers()["optimizer"]
    ol.set_gradient_clipping(v)
    (ml.training_step(batches[1]) / 2).backward()
    ol.step()
    # the Trainer
    mf = recipe_module(True)
    assert torch.equal(flat(mf), p0)
    mf.k_for_precision_at_k = mf.k_for_image_text_retreival = [3]      # 8 cached samples at the epoch end
    conf = mf.configure_optimizers()
    of = conf["optimizer"]
    assert isinstance(of, FusedAdamW)
    calls, plain_step, plain_acc = [], of.step, of.accumulate
    of.step = lambda *a, **k: (calls.append("step"), plain_step(*a, **k))[1]
    of.accumulate = lambda *a, **k: (calls.append("accumulate"), plain_acc(*a, **k))[1]
    mf.configure_optimizers = lambda: conf
    t = Trainer(accumulate_grad_batches=2, gradient_clip_val=v, max_epochs=1, enable_checkpointing=False,
                default_root_dir=str(tmp_path))
    t.fit(mf, train_dataloaders=batches)
    torch.cuda.synchronize()
    assert calls == ["accumulate", "step"] and t.global_step == 1
    d_f, d_t, d_l = flat(mf) - p0, flat(mt) - p0, flat(ml) - p0
    norm = t.logged_metrics["grad_norm"]
    print(f"accumulated norm: fused {norm:.9g} torch {n0:.9g}; parameter delta rel-L2 vs torch {rel(d_f, d_t):.3e}, "
          f"last micro-batch alone vs torch {rel(d_l, d_t):.3e}, fused vs last alone {rel(d_f, d_l):.3e}")
    # the norm that was clipped is the accumulated gradient's (two backward runs differ by the
    # order of their atomic sums only, far below 1e-3; one micro-batch's norm is nowhere near)
    assert abs(norm - n0) <= 1e-3 * n0
    assert rel(d_f, d_t) < 3e-3, rel(d_f, d_t)
    # ten times the tolerance apart from the step on the last micro-batch alone
    assert rel(d_f, d_l) > 3e-2, rel(d_f, d_l)
