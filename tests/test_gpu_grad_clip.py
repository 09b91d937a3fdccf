"""Gradient clipping on the device (torch.nn.utils.clip_grad_norm_ / clip_grad_value_,
Lightning's gradient_clip_val), fused into FusedAdamW.step():

  vlp_grad_sumsq   fp64 partial sums of g^2, one per 16384-element segment of a span
  vlp_clip_coef    norm = sqrt(sum of partials), coef = min(1, max_norm / (norm + 1e-6))
  vlp_adamw_clip   vlp_adamw on g * coef (or clamp(g, +-value)), the clipped g written back

Bounds.
  norm: every square is exact in fp64 (24-bit x 24-bit significands) and every sum is fp64,
    so the sum of n <= 2^20 + 3 non-negative terms is within n * 2^-53 < 1.2e-10 of the
    exact one, the fp64 sqrt halves that, and the one rounding to fp32 adds half an fp32 ulp:
    well inside 1 fp32 ulp, checked as relative 1.2e-7 (2^-23) against
    g.double().pow(2).sum().sqrt().
  partials: each is an fp64 sum of at most 16384 non-negative terms, as is the reference's
    (in another order): both within 16384 * 2^-53 = 1.9e-12 of the exact sum, checked at 4e-12.
  coefficient: fp32 add and IEEE fp32 divide of the same operands as torch: equal bits.
  update: where torch and the kernel evaluate the same fp32 expression the results may differ
    by the order of one or two roundings: <= 2 ulp.

Hyper-parameters of the "vs torch" moment checks: the step kernel forms 1 - beta in fp32
(1.f - 0.999f = 0.99998712e-3) where torch rounds the double 1 - 0.999 to fp32 (1.0000000475e-3):
1.3e-5 apart with the default betas (the known envelope of tests/test_gpu_bn_routes.py
test_adamw), which would drown the <= 2 ulp / 1e-6 checks of what the clip adds.  Those checks
therefore use betas (0.875, 0.96875), for which 1 - beta is exact in both; the default betas
are checked against the kernel's own fp32 formula evaluated by torch.
"""
import ctypes
import functools
import math

import pytest
import torch

from tests.golden.synth import synth_batch

pytestmark = pytest.mark.gpu

SEG = 16384                    # elements per partial (include/vlp_hip.h, vlp_grad_sumsq)
SIZES = [1, 3, 255, 256, 257, 65541, 2 ** 20 + 3]
ULP = 2.0 ** -23               # 1 fp32 ulp, relative (1.2e-7)
DYADIC = (0.875, 0.96875)      # betas with 1 - beta exact in fp32 and in fp64


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def ops():
    from vlp_amd import ops as o
    return o


def mixed(n, seed):
    """1e-4 and 1e3 magnitudes interleaved, random signs and mantissas: an fp32 running
    sum of the squares (1e6 each) would drop every small square (1e-8)."""
    g = torch.Generator().manual_seed(seed)
    r = (torch.rand(n, generator=g) + 0.5) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    scale = torch.where(torch.arange(n) % 2 == 0, torch.tensor(1e-4), torch.tensor(1e3))
    return (r * scale).float()


def on_device(vals, off):
    """vals in a NaN-filled device buffer at element offset `off` (offset 1: the span starts
    4 B past a 16-B boundary); a read outside the span would poison the sum."""
    buf = torch.full((vals.numel() + 8,), float("nan"), device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + vals.numel()]
    v.copy_(vals)
    return v


def ulp_diff(a, b):
    """Distance in fp32 units in the last place (finite inputs)."""
    def key(x):
        i = x.detach().contiguous().view(torch.int32).to(torch.int64).cpu()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (key(a) - key(b)).abs()


def coef_torch(norm32, max_norm):
    """clamp(max_norm / (total_norm + 1e-6), max=1) from an fp32 total norm, every operation
    in fp32 on the host (both operands of the division as fp32 tensors: a Python scalar on the
    left would make torch multiply by the reciprocal instead)."""
    return torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (norm32.float().cpu() + 1e-6), max=1.0)


def clipped_norm(norm, max_norm):
    """The norm clip_grad_norm_ leaves behind (the 1e-6 in the coefficient keeps it a little
    below max_norm)."""
    return norm * min(1.0, max_norm / (norm + 1e-6))


# ---------------------------------------------------------------- norm
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_norm_single_span(ops, n, off):
    vals = mixed(n, n + off)
    g = on_device(vals, off)
    ref = vals.double().pow(2).sum().sqrt().item()
    k = ops.grad_sumsq_nparts(n)
    assert k == (n + SEG - 1) // SEG
    runs = []
    for _ in range(2):
        partials = torch.full((k + 2,), float("nan"), dtype=torch.float64, device="cuda")
        out = torch.full((2,), float("nan"), device="cuda")
        assert ops.grad_sumsq(g, partials) == k
        ops.clip_coef(k, partials, 0.5 * ref, out)
        torch.cuda.synchronize()
        runs.append((partials.cpu(), out.cpu()))
    (p0, o0), (p1, o1) = runs
    assert torch.isnan(p0[k:]).all(), "wrote past its partials"
    # per segment against fp64
    seg_ref = torch.stack([c.double().pow(2).sum() for c in vals.split(SEG)])
    err = ((p0[:k] - seg_ref).abs() / seg_ref).max().item()
    print(f"n {n} off {off}: partials rel err {err:.2e}, norm {o0[0].item():.9g} ref {ref:.9g} "
          f"rel {abs(o0[0].item() - ref) / ref:.2e}")
    assert err <= 4e-12
    assert abs(o0[0].double().item() - ref) <= ULP * ref
    assert torch.equal(o0[1:], coef_torch(o0[:1], 0.5 * ref))
    # bitwise reproducible
    assert torch.equal(p0[:k].view(torch.int64), p1[:k].view(torch.int64))
    assert torch.equal(o0.view(torch.int32), o1.view(torch.int32))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_norm_three_spans_in_one_partials_buffer(ops, n, off):
    """The span under test between two others (257 elements at the opposite alignment, 16385
    at offset 3), laid end to end in one partials buffer as FusedAdamW.step() does."""
    spans = [(mixed(257, 5), 1 - off), (mixed(n, 7 * n + off), off), (mixed(SEG + 1, 9), 3)]
    dev = [on_device(v, o) for v, o in spans]
    total = sum(ops.grad_sumsq_nparts(v.numel()) for v, _ in spans)
    assert total == 1 + (n + SEG - 1) // SEG + 2
    ref = math.sqrt(sum(v.double().pow(2).sum().item() for v, _ in spans))
    runs = []
    for _ in range(2):
        partials = torch.full((total + 1,), float("nan"), dtype=torch.float64, device="cuda")
        out = torch.zeros(2, device="cuda")
        o = 0
        for g in dev:
            o += ops.grad_sumsq(g, partials, o)
        assert o == total
        ops.clip_coef(total, partials, 1.0, out)
        torch.cuda.synchronize()
        runs.append((partials.cpu(), out.cpu()))
    (p0, o0), (p1, o1) = runs
    assert torch.isnan(p0[total:]).all() and torch.isfinite(p0[:total]).all()
    seg_ref = torch.stack([c.double().pow(2).sum() for v, _ in spans for c in v.split(SEG)])
    assert ((p0[:total] - seg_ref).abs() / seg_ref).max().item() <= 4e-12
    print(f"n {n} off {off}: norm {o0[0].item():.9g} ref {ref:.9g} rel {abs(o0[0].item() - ref) / ref:.2e}")
    assert abs(o0[0].double().item() - ref) <= ULP * ref
    assert torch.equal(p0[:total].view(torch.int64), p1[:total].view(torch.int64))
    assert torch.equal(o0.view(torch.int32), o1.view(torch.int32))


def test_sumsq_empty_span_and_null_pointers(ops):
    from vlp_amd._lib import lib, stream_of
    raw = lib()._fns["vlp_grad_sumsq"]
    st = stream_of()
    k = ctypes.c_int(-1)
    partials = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    g = torch.ones(8, device="cuda")
    for n in (0, -3):                                     # no-op, whatever the pointers
        assert raw(n, None, None, ctypes.byref(k), st) == 0 and k.value == 0
        assert raw(n, g.data_ptr(), partials.data_ptr(), ctypes.byref(k), st) == 0
    inval = 1                                             # hipErrorInvalidValue
    assert raw(8, None, partials.data_ptr(), ctypes.byref(k), st) == inval
    assert raw(8, g.data_ptr(), None, ctypes.byref(k), st) == inval
    assert raw(8, g.data_ptr(), partials.data_ptr(), None, st) == inval
    torch.cuda.synchronize()
    assert (partials == 7.0).all()                        # nothing was launched
    with pytest.raises(ValueError):                       # the wrapper checks the room first
        ops.grad_sumsq(torch.ones(SEG + 1, device="cuda"), partials, 3)
    assert ops.grad_sumsq(g[:0], partials) == 0


# ---------------------------------------------------------------- coefficient
@pytest.mark.parametrize("parts,max_norm", [
    ([9.0, 16.0], 10.0),          # norm 5 below max_norm: coefficient exactly 1
    ([9.0, 16.0], 5.0),           # max_norm == norm: 5 / (5 + 1e-6) < 1
    ([9.0, 16.0], 2.0),
    ([1e6, 3.0, 1e-8], 0.37),
    ([0.0, 0.0, 0.0], 1.0),       # norm exactly 0: 1 / 1e-6 clamps to 1
    ([0.0], 1e-7),                # norm exactly 0, max_norm below the epsilon: 0.1
    ([], 1.0),                    # no partials at all
    ([4.0, float("inf")], 1.0),   # non-finite values propagate as in torch: coefficient 0 ...
    ([4.0, float("nan")], 1.0),   # ... and NaN
])
def test_coefficient_matches_torch_formula(ops, parts, max_norm):
    p = torch.tensor(parts + [123.0], dtype=torch.float64, device="cuda")   # one entry past nparts
    out = torch.full((2,), -1.0, device="cuda")
    ops.clip_coef(len(parts), p, max_norm, out)
    torch.cuda.synchronize()
    out = out.cpu()
    norm = torch.tensor(parts, dtype=torch.float64).sum().sqrt().float()
    want = torch.stack([norm, coef_torch(norm, max_norm)])
    print(parts, max_norm, out.tolist(), want.tolist())
    assert torch.equal(out.view(torch.int32), want.view(torch.int32)) or \
        (torch.isnan(want).all() and torch.isnan(out).all())
    if parts == [9.0, 16.0] and max_norm == 10.0:
        assert out[1].item() == 1.0
    if parts == [0.0]:
        assert out[0].item() == 0.0 and 0.0 < out[1].item() < 1.0


# ---------------------------------------------------------------- update kernel
HYP = dict(lr=1e-3, eps=1e-8, wd=0.01)


def adam_inputs(n, off, seed):
    g = torch.Generator().manual_seed(seed)
    host = {"p": torch.randn(n, generator=g), "g": mixed(n, seed + 1) * 1e-3,
            "m": torch.randn(n, generator=g) * 1e-2, "v": torch.rand(n, generator=g) * 1e-3}
    return host, lambda: {k: on_device(t, off) for k, t in host.items()}


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_adamw_clip_with_unit_coefficient_is_adamw(ops, n, off):
    host, fresh = adam_inputs(n, off, 3 * n + off)
    one = torch.ones(1, device="cuda")
    a, b = fresh(), fresh()
    args = (HYP["lr"], 0.9, 0.999, HYP["eps"], HYP["wd"], 3)
    ops.adamw(a["p"], a["g"], a["m"], a["v"], *args)
    ops.adamw_clip(b["p"], b["g"], b["m"], b["v"], *args, coef=one)
    torch.cuda.synchronize()
    for k in "pgmv":
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert torch.equal(b["g"].cpu(), host["g"])
    assert not torch.equal(b["p"].cpu(), host["p"]) or n == 0


def torch_adamw_step(p, g, betas):
    """One torch.optim.AdamW step from zero moments on the device: (p, exp_avg, exp_avg_sq)."""
    q = torch.nn.Parameter(p.clone())
    q.grad = g.clone()
    opt = torch.optim.AdamW([q], lr=HYP["lr"], betas=betas, eps=HYP["eps"], weight_decay=HYP["wd"])
    opt.step()
    return q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]


@pytest.mark.parametrize("mode", ["norm", "value"])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_adamw_clip_first_step_moments_vs_torch(ops, n, off, mode):
    """One step from zero moments: exp_avg = (1 - b1) gc, exp_avg_sq = (1 - b2) gc^2 and
    g = gc, with gc = 0.25 g (norm mode) or clamp(g, +-c) (value mode), against torch fp32.
    (The parameters alone would not do: Adam's first update does not depend on the scale of g.)"""
    host, fresh = adam_inputs(n, off, 5 * n + off)
    host["m"].zero_()
    host["v"].zero_()
    d = fresh()
    g0 = d["g"].clone()
    cv = 0.4 * host["g"].abs().max().item()
    if mode == "norm":
        gc = g0 * 0.25
        kw = dict(coef=torch.tensor([0.25], device="cuda"))
    else:
        gc = g0.clamp(-cv, cv)
        kw = dict(clip_value=cv)
        assert n < 3 or (0 < (g0.abs() > cv).sum().item() < n)      # some clamped, some not
    for betas in (DYADIC, (0.9, 0.999)):
        d = fresh()
        ops.adamw_clip(d["p"], d["g"], d["m"], d["v"], HYP["lr"], betas[0], betas[1], HYP["eps"], HYP["wd"], 1, **kw)
        torch.cuda.synchronize()
        assert torch.equal(d["g"], gc), "clipped gradient not written back"
        if betas is DYADIC:
            _, tm, tv = torch_adamw_step(host["p"].cuda(), gc, betas)
        else:
            # the kernel's own fp32 constants (see the module docstring), evaluated by torch
            b1 = torch.tensor(betas[0], dtype=torch.float32, device="cuda")
            b2 = torch.tensor(betas[1], dtype=torch.float32, device="cuda")
            tm, tv = (1 - b1) * gc, (1 - b2) * gc * gc
        dm, dv = ulp_diff(d["m"], tm).max().item(), ulp_diff(d["v"], tv).max().item()
        print(f"n {n} off {off} {mode} betas {betas}: exp_avg {dm} ulp, exp_avg_sq {dv} ulp")
        assert dm <= 2 and dv <= 2


def test_adamw_clip_rejects_bad_modes(ops):
    from vlp_amd._lib import lib, stream_of
    raw = lib()._fns["vlp_adamw_clip"]
    t = [torch.ones(4, device="cuda") for _ in range(4)]
    ptrs = [x.data_ptr() for x in t]
    tail = (1e-3, 0.9, 0.999, 1e-8, 0.01, 1e-2, 0.03)
    st = stream_of()
    assert raw(4, *ptrs, *tail, 0, None, 1.0, st) == 1               # mode 0 is vlp_adamw's job
    assert raw(4, *ptrs, *tail, 3, None, 1.0, st) == 1
    assert raw(4, *ptrs, *tail, 1, None, 1.0, st) == 1               # norm mode without a coefficient
    assert raw(4, ptrs[0], None, ptrs[2], ptrs[3], *tail, 2, None, 1.0, st) == 1
    assert raw(0, *ptrs, *tail, 2, None, 1.0, st) == 0
    torch.cuda.synchronize()
    assert all((x == 1).all() for x in t)
    with pytest.raises(ValueError):
        ops.adamw_clip(*t, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1)
    with pytest.raises(ValueError):
        ops.adamw_clip(*t, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, coef=t[0], clip_value=1.0)


# ---------------------------------------------------------------- optimizer
def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def tiny_arena_module():
    from vlp_amd.arena import ArenaModule

    class Tiny(ArenaModule):
        def __init__(self):
            super().__init__()
            self._init_arena([("w", (5,)), ("b", (3, 7)), ("c", (SEG + 16,)), ("d", (9,)), ("e", (2, 2))],
                             device="cuda")
            for k in "wbcde":
                self._register(self, k, k)
            g = torch.Generator().manual_seed(1)
            with torch.no_grad():
                for p in self.parameters():
                    p.copy_(torch.randn(p.shape, generator=g))
    return Tiny()


@pytest.mark.parametrize("algo", ["norm", "value"])
def test_fused_adamw_clips_gradients_held_outside_the_arena(algo):
    """p.grad tensors that are not views of the arena (the copy branch of _spans): the
    arena copy is clipped by the kernel and p.grad ends up clipped too; a parameter without
    a gradient ("d") is outside the norm; two groups share one norm."""
    from vlp_amd.optim import FusedAdamW
    m = tiny_arena_module()
    ps = dict(m.named_parameters())
    groups = [{"params": [ps["w"], ps["b"], ps["d"]], "lr": 1e-3}, {"params": [ps["c"], ps["e"]], "lr": 1e-2}]
    opt = FusedAdamW(groups, betas=DYADIC, arenas=[m])
    raw = {k: mixed(p.numel(), 40 + i).view(p.shape).cuda() * 1e-3 for i, (k, p) in enumerate(ps.items()) if k != "d"}
    for k, g in raw.items():
        ps[k].grad = g.clone()
    n0 = math.sqrt(sum(g.double().pow(2).sum().item() for g in raw.values()))
    val = 0.5 * n0 if algo == "norm" else 0.3 * max(g.abs().max().item() for g in raw.values())
    # torch on clones
    ref = {k: torch.nn.Parameter(ps[k].detach().clone()) for k in raw}
    for k in raw:
        ref[k].grad = raw[k].clone()
    topt = torch.optim.AdamW([{"params": [ref["w"], ref["b"]], "lr": 1e-3}, {"params": [ref["c"], ref["e"]], "lr": 1e-2}],
                             betas=DYADIC)
    if algo == "norm":
        torch.nn.utils.clip_grad_norm_(list(ref.values()), val)
    else:
        torch.nn.utils.clip_grad_value_(list(ref.values()), val)
    topt.step()
    d0 = ps["d"].detach().clone()
    opt.set_gradient_clipping(val, algo)
    opt.step()
    torch.cuda.synchronize()
    for k in raw:
        assert ps[k].grad.data_ptr() != m.arena.gview(k).data_ptr()
        assert not torch.equal(ps[k].grad, raw[k]) or k in ("w", "e")      # big tensors really were clipped
        assert rel(ps[k].grad, ref[k].grad) <= 1e-6, k
        assert torch.equal(ps[k].grad, m.arena.gview(k)), k
        assert rel(opt.state[ps[k]]["exp_avg"], topt.state[ref[k]]["exp_avg"]) <= 1e-6, k
        assert rel(opt.state[ps[k]]["exp_avg_sq"], topt.state[ref[k]]["exp_avg_sq"]) <= 1e-6, k
        assert rel(ps[k], ref[k]) <= 1e-6, k
    assert torch.equal(ps["d"], d0) and ps["d"].grad is None
    if algo == "norm":
        assert abs(opt.last_grad_norm.double().item() - n0) <= ULP * n0
        clipped = math.sqrt(sum(ps[k].grad.double().pow(2).sum().item() for k in raw))
        assert abs(clipped - clipped_norm(n0, val)) <= 1e-6 * val
    else:
        assert opt.last_grad_norm is None
        for k in raw:
            assert torch.equal(ps[k].grad, raw[k].clamp(-val, val)), k
    # clipping off again: the plain step, gradients left alone
    opt.set_gradient_clipping(None)
    before = {k: ps[k].grad.clone() for k in raw}
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(ps[k].grad, before[k]) for k in raw)


B, H, T = 4, 64, 12


def small_module(fused=True, betas=None):
    """The module of the golden step (B = 4, 64 x 64, T = 12, fp32) at its own init, as
    tests/test_gpu_model.py's three-step optimizer test builds it."""
    from src.models.pretrain.VisionLanguageModule import VisionLanguageModule
    torch.manual_seed(0)
    kw = {} if betas is None else {"betas": betas}
    m = VisionLanguageModule("resnet34", "tinybert", functools.partial(torch.optim.AdamW, lr=1e-3, **kw),
                             False, False, 512, 312, 128, compute_dtype="fp32", text_dropout=0.0,
                             fused_optimizer=fused)
    m.train()
    return m


def flat(m):
    # attention key biases have an exactly-zero true gradient: AdamW turns their rounding
    # noise into +-lr steps (tests/test_gpu_model.py leaves them out for the same reason)
    return torch.cat([p.detach().double().flatten().cpu() for k, p in m.named_parameters()
                      if "attention.self.key.bias" not in k])


def grad_norm64(params):
    return math.sqrt(sum(p.grad.double().pow(2).sum().item() for p in params if p.grad is not None))


def test_fused_adamw_norm_clip_matches_torch_on_the_small_module():
    from vlp_amd.optim import FusedAdamW
    batch = synth_batch(B, H, T, 0)
    mf, mt = small_module(True, DYADIC), small_module(False, DYADIC)
    of, ot = mf.configure_optimizers()["optimizer"], mt.configure_optimizers()["optimizer"]
    assert isinstance(of, FusedAdamW) and type(ot) is torch.optim.AdamW
    p0 = flat(mf)
    assert torch.equal(p0, flat(mt))
    # step 1: one backward; torch gets clones of its gradients
    of.zero_grad()
    mf.training_step(batch).backward()
    n0 = grad_norm64(mf.parameters())
    max_norm = 0.5 * n0
    for (k, pf), pt in zip(mf.named_parameters(), mt.parameters()):
        pt.grad = None if pf.grad is None else pf.grad.detach().clone()
    torch.nn.utils.clip_grad_norm_([p for p in mt.parameters() if p.grad is not None], max_norm)
    ot.step()
    of.set_gradient_clipping(max_norm)
    of.step()
    torch.cuda.synchronize()
    assert abs(of.last_grad_norm.double().item() - n0) <= ULP * n0
    assert abs(grad_norm64(mf.parameters()) - clipped_norm(n0, max_norm)) <= 1e-6 * max_norm
    worst = {"grad": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}
    for (k, pf), pt in zip(mf.named_parameters(), mt.parameters()):
        assert (pf.grad is None) == (pt.grad is None), k
        if pf.grad is None:
            continue
        r = {"grad": rel(pf.grad, pt.grad), "exp_avg": rel(of.state[pf]["exp_avg"], ot.state[pt]["exp_avg"]),
             "exp_avg_sq": rel(of.state[pf]["exp_avg_sq"], ot.state[pt]["exp_avg_sq"])}
        for q, v in r.items():
            worst[q] = max(worst[q], v)
            assert v <= 1e-6, (k, q, v)
    print("worst per-parameter rel-L2 vs clip_grad_norm_ + torch AdamW:", worst)
    # steps 2 and 3: each model on its own gradients, both clipped to max_norm
    for _ in range(2):
        of.zero_grad()
        mf.training_step(batch).backward()
        of.step()
        ot.zero_grad()
        mt.training_step(batch).backward()
        torch.nn.utils.clip_grad_norm_([p for p in mt.parameters() if p.grad is not None], max_norm)
        ot.step()
    torch.cuda.synchronize()
    r3 = rel(flat(mf) - p0, flat(mt) - p0)
    print("three clipped steps, parameter delta rel-L2 vs torch:", r3)
    assert r3 < 3e-3, r3


def test_huge_max_norm_is_bitwise_the_unclipped_run():
    """max_norm = 1e30 (coefficient exactly 1) against clipping off, three steps.  The backward
    has order-dependent atomic sums (DESIGN, "bench.py --dump-outputs"), so the two optimizers
    are given the same gradients: one backward per step, copied to the second module."""
    batch = synth_batch(B, H, T, 0)
    ma, mb = small_module(), small_module()
    oa, ob = ma.configure_optimizers()["optimizer"], mb.configure_optimizers()["optimizer"]
    oa.set_gradient_clipping(1e30)
    for _ in range(3):
        oa.zero_grad()
        ob.zero_grad()
        ma.training_step(batch).backward()
        for pa, pb in zip(ma.parameters(), mb.parameters()):
            pb.grad = None if pa.grad is None else pa.grad.detach().clone()
        oa.step()
        ob.step()
    torch.cuda.synchronize()
    assert oa.last_grad_norm.item() > 0 and ob.last_grad_norm is None
    for (k, pa), pb in zip(ma.named_parameters(), mb.parameters()):
        assert torch.equal(pa.detach().view(torch.int32), pb.detach().view(torch.int32)), k
        if pa in oa.state:
            for q in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(oa.state[pa][q], ob.state[pb][q]), (k, q)


# ---------------------------------------------------------------- trainer
def test_trainer_clips_every_step_and_logs_the_norm(tmp_path):
    from src.utils.trainer import Trainer
    batches = [synth_batch(B, H, T, s) for s in (0, 1)]
    probe = small_module()
    probe.training_step(batches[0]).backward()
    v = 0.5 * grad_norm64(probe.parameters())           # below the first step's norm: the clip is active
    del probe

    m = small_module()
    m.k_for_precision_at_k = m.k_for_image_text_retreival = [3]      # 8 cached samples at the epoch end
    conf = m.configure_optimizers()
    opt = conf["optimizer"]
    after, plain_step = [], opt.step

    def step(*a, **k):
        r = plain_step(*a, **k)
        after.append((grad_norm64(m.parameters()), opt.last_grad_norm.item()))
        return r
    opt.step = step
    m.configure_optimizers = lambda: conf
    t = Trainer(gradient_clip_val=v, max_steps=2, max_epochs=1, enable_checkpointing=False,
                default_root_dir=str(tmp_path))
    t.fit(m, train_dataloaders=batches)
    assert t.global_step == 2 and len(after) == 2
    print("v", v, "(norm after the step, norm before clipping):", after)
    for clipped, before in after:
        assert clipped <= v * (1 + 1e-5)
        assert abs(clipped - clipped_norm(before, v)) <= 1e-5 * v      # clipped to v, not to less
    assert after[0][1] > v, "the first step's norm was meant to be above the threshold"
    assert "grad_norm" in t.logged_metrics
    assert t.logged_metrics["grad_norm"] == after[-1][1]
