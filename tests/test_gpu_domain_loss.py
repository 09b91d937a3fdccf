"""GPU: the on-device weighted BCE + CORAL loss (csrc/domain_loss_ops.hip, vlp_amd/domain_loss.py)
against the fp64 closed form on the CPU evaluated from the same fp32 inputs (tests/domain_loss_ref.py).

Bounds.  The op accumulates in fp64 and rounds once to fp32 on output, so a gradient element may
differ from the reference by one fp32 rounding, 2^-23 |ref|, plus 1e-9 max|ref| of its tensor for the
different fp64 summation order; the three fp64 losses agree to 1e-12 relative, and a loss or a
gradient that the rule makes 0 is exactly 0.  Shapes: D in {1, 3, 33, 384, 512, 1024} (below a tile,
no multiple of one, one statistics strip and a half, whole tiles, several) and N in {1, 4, 65, 300}
(below, at and across the 32-row steps and the 256-row chunk)."""
import functools
import types

import pytest
import torch

from tests.domain_loss_ref import codes_of, domain_loss_ref
from tests.test_domain_loss_cpu import GOLD, coral_case

pytestmark = pytest.mark.gpu

LAYOUTS = ("2v2", "interleaved", "all_source", "1vrest", "mixed")
KINDS = (torch.int64, torch.int32, torch.uint8, torch.bool)


def _codes(layout, N):
    if layout == "2v2":            # the minimum live case; the other rows take no part
        c = [0, 0, 1, 1] + [2] * N
    elif layout == "interleaved":
        c = [i % 2 for i in range(N)]
    elif layout == "all_source":
        c = [0] * N
    elif layout == "1vrest":       # one source row: CORAL exactly 0 (1 v 5 at N = 6)
        c = [0] + [1] * N
    else:                          # rows of neither domain mixed in
        c = [(0, 2, 1, 1, 0, 2, 0)[i % 7] for i in range(N)]
    return torch.tensor(c[:N], dtype=torch.uint8)


@functools.lru_cache(maxsize=None)
def _inputs(N, D, seed=0, shift=0.0):
    g = torch.Generator().manual_seed(1000 * N + D + seed)
    x = torch.randn(N, D, generator=g) + shift
    z = torch.randn(N, generator=g) * 3
    y = torch.randint(0, 2, (N,), generator=g)
    return x, z, y


def _bounds(dev, ref, name):
    """max over the elements of |dev - ref| / (2^-23 |ref| + 1e-9 max|ref|); <= 1 passes."""
    ref = ref.double()
    tol = 2.0 ** -23 * ref.abs() + 1e-9 * ref.abs().max()
    err = (dev.double().cpu() - ref).abs()
    if not ref.any():
        assert not dev.any(), f"{name}: the reference is exactly 0, the device is not"
        return 0.0
    return float((err / tol).max())


def _check(out, g_feat, g_logits, ref, tag):
    o = out.cpu()
    for k, name in enumerate(("total", "cls", "coral")):
        r = ref[name].item()
        assert abs(o[k].item() - r) <= 1e-12 * abs(r), (tag, name, o[k].item(), r)
    if g_feat is not None:
        e = _bounds(g_feat, ref["g_feat"], "g_feat")
        assert e <= 1.0, (tag, "g_feat", e)
        dead = ref["g_feat"].abs().sum(1) == 0
        assert not g_feat.cpu()[dead].any(), (tag, "rows outside CORAL carry a feature gradient")
    if g_logits is not None:
        e = _bounds(g_logits, ref["g_logits"], "g_logits")
        assert e <= 1.0, (tag, "g_logits", e)


@pytest.mark.parametrize("D", [1, 3, 33, 384, 512, 1024])
@pytest.mark.parametrize("N", [1, 4, 65, 300])
def test_op_vs_fp64_closed_form(N, D):
    from vlp_amd import ops
    x, z, y = _inputs(N, D)
    xd, zd = x.cuda(), z.cuda()
    k = 0
    for layout in LAYOUTS:
        codes = _codes(layout, N)
        for lam in (0.0, 0.5, 1000.0):
            w0, w1 = ((1.0, 1.0), (0.7, 2.0))[k % 2]
            kind = KINDS[k % len(KINDS)]
            k += 1
            ref = domain_loss_ref(x, z, y, codes, w0, w1, lam)
            out, gf, gl = ops.domain_loss(xd, zd, y.to(kind).cuda(), codes.cuda(), w0, w1, lam)
            tag = (N, D, layout, lam, (w0, w1), kind)
            _check(out, gf, gl, ref, tag)
            ns, nt = int((codes == 0).sum()), int((codes == 1).sum())
            if ns <= 1 or nt <= 1 or lam == 0.0:
                assert out[2].item() == 0.0 and not gf.any(), tag        # exactly 0, BCE still live
                assert out[1].item() > 0.0 and gl.abs().min().item() > 0.0, tag
            else:
                assert out[2].item() > 0.0, tag
            if (codes == 2).any():       # a row of neither domain still has its BCE gradient
                assert gl.cpu()[codes == 2].abs().min().item() > 0.0, tag


@pytest.mark.parametrize("N,D", [(65, 33), (300, 512)])
def test_row_stride_null_gradient_and_repeat(N, D):
    """ldf > D; a call without the gradient pass returns the same `out` bits; two calls agree bit
    for bit."""
    from vlp_amd import ops
    x, z, y = _inputs(N, D, seed=1)
    codes = _codes("mixed", N)
    wide = torch.full((N, D + 5), float("nan"), device="cuda")
    wide[:, :D] = x.cuda()
    xs = wide[:, :D]
    assert xs.stride(0) == D + 5
    args = (z.cuda(), y.cuda(), codes.cuda(), 0.7, 2.0, 1000.0)
    ref = domain_loss_ref(x, z, y, codes, 0.7, 2.0, 1000.0)
    a = ops.domain_loss(xs, *args)
    _check(*a, ref, ("strided", N, D))
    b = ops.domain_loss(xs, *args)
    c = ops.domain_loss(x.cuda(), *args)
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v) and torch.equal(u, w)
    o, gf, gl = ops.domain_loss(xs, *args, grad=False)
    assert gf is None and gl is None and torch.equal(o, a[0])


def test_large_magnitude_features():
    """x = 30 + randn: the second moments are ~900 and their difference is O(1), so the fp32 torch
    path loses digits to cancellation in a term multiplied by lambda = 1000; the op keeps its bound."""
    from src.models.baseline.FusionModule import FusionModule
    from vlp_amd import ops
    N, D, lam = 65, 33, 1000.0
    x, z, y = _inputs(N, D, seed=2, shift=30.0)
    codes = _codes("interleaved", N)
    ref = domain_loss_ref(x, z, y, codes, 1.0, 1.0, lam)
    out, gf, gl = ops.domain_loss(x.cuda(), z.cuda(), y.cuda(), codes.cuda(), 1.0, 1.0, lam)
    me = types.SimpleNamespace(label_weights=torch.ones(2), hparams=types.SimpleNamespace(coral_lambda=lam))
    xt = x.cuda().requires_grad_()
    tot, _, cor = FusionModule._compute_loss(me, xt, z.cuda(), y, ["INTERNAL" if c == 0 else "BTXRD" for c in codes])
    gt, = torch.autograd.grad(tot, xt)
    rc, rg = ref["coral"].item(), ref["g_feat"]
    e_dev = (abs(out[2].item() - rc) / rc, ((gf.double().cpu() - rg).norm() / rg.norm()).item())
    e_t32 = (abs(cor.item() - rc) / rc, ((gt.double().cpu() - rg).norm() / rg.norm()).item())
    msg = (f"coral {rc:.6e}: relative error of (loss, gradient) device op {e_dev[0]:.2e}, {e_dev[1]:.2e}; "
           f"fp32 torch path {e_t32[0]:.2e}, {e_t32[1]:.2e}")
    print(msg)
    _check(out, gf, gl, ref, msg)
    assert e_t32[0] > e_dev[0] and e_t32[1] > e_dev[1], msg


def test_invalid_arguments_are_refused_and_empty_batch_writes_zeros():
    from vlp_amd import _lib, ops
    L = _lib.lib()
    N, D = 8, 16
    f = torch.randn(N, D, device="cuda")
    z = torch.randn(N, device="cuda")
    y = torch.zeros(N, dtype=torch.int64, device="cuda")
    c = torch.zeros(N, dtype=torch.uint8, device="cuda")
    out = torch.full((3,), 7.0, dtype=torch.float64, device="cuda")
    nbytes = ops.domain_loss_ws_bytes(N, D)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    p = _lib.ptr
    good = dict(N=N, D=D, feat=p(f), ldf=D, logits=p(z), label=p(y), label_kind=0, domain=p(c), w0=1.0, w1=1.0,
                coral_lambda=1.0, out=p(out), g_feat=None, g_logits=None, ws=p(ws), ws_bytes=nbytes, stream=s)
    L.vlp_domain_loss(*good.values())
    torch.cuda.synchronize()
    assert out[1].item() > 0.0 and out[2].item() == 0.0
    bad = [dict(feat=None), dict(logits=None), dict(label=None), dict(domain=None), dict(out=None), dict(ws=None),
           dict(N=-1), dict(N=(1 << 18) + 1), dict(D=0), dict(D=2049), dict(ldf=D - 1), dict(label_kind=-1),
           dict(label_kind=3), dict(ws_bytes=nbytes - 8)]
    out.fill_(7.0)
    for change in bad:
        with pytest.raises(_lib.HipError):
            L.vlp_domain_loss(*{**good, **change}.values())
    torch.cuda.synchronize()
    assert (out == 7.0).all()                      # refused before any launch
    L.vlp_domain_loss(*{**good, "N": 0, "feat": None, "logits": None, "label": None, "domain": None,
                        "ws": None, "ws_bytes": 0}.values())
    torch.cuda.synchronize()
    assert not out.any()                           # N = 0: nothing launched, zeros written


def test_goldens_through_the_autograd_function():
    from vlp_amd.domain_loss import DomainLossFn, domain_loss
    for name in [k for k in GOLD if k.startswith("coral_")]:
        c = GOLD[name]
        feat, logits, labels, codes, ns = coral_case(c)
        x = feat.cuda().requires_grad_()
        tot, cls, cor = DomainLossFn.apply(x, logits.cuda(), labels.cuda(), codes.cuda(), 1.0, 1.0, 1.0)
        assert tot.dim() == cls.dim() == cor.dim() == 0 and tot.dtype == torch.float32 and tot.is_cuda
        assert not cls.requires_grad and not cor.requires_grad and tot.requires_grad
        assert torch.allclose(cor.cpu(), c["loss"], rtol=1e-5, atol=1e-7), (name, cor.item(), c["loss"].item())
        if "grad_source" in c:
            g, = torch.autograd.grad(tot, x)
            assert torch.allclose(g[:ns].cpu(), c["grad_source"], rtol=1e-4, atol=1e-8), name
            assert torch.allclose(g[ns:].cpu(), c["grad_target"], rtol=1e-4, atol=1e-8), name
    for case in GOLD["compute_loss"]:
        f = case["features"].cuda().requires_grad_()
        lg = case["logits"].cuda().requires_grad_()
        tot, cls, cor = domain_loss(f, lg, case["labels"], case["dataset"], case["label_weights"],
                                    float(case["coral_lambda"]))
        assert abs(tot.item() - case["loss"].item()) < 1e-6
        assert abs(cls.item() - case["classification_loss"].item()) < 1e-6
        assert abs(cor.item() - case["coral_loss"].item()) < 1e-6
        (3.0 * tot).backward()                     # the backward scales by the incoming gradient
        assert torch.allclose(lg.grad.cpu() / 3.0, case["grad_logits"], rtol=1e-5, atol=1e-8)
        assert torch.allclose(f.grad.cpu() / 3.0, case["grad_features"], rtol=1e-4, atol=1e-9)
    # under no_grad (validation) the gradient pass is skipped and the losses are the same bits
    with torch.no_grad():
        t2, c2, r2 = domain_loss(f.detach(), lg.detach(), case["labels"], case["dataset"], case["label_weights"],
                                 float(case["coral_lambda"]))
    assert torch.equal(t2, tot.detach()) and torch.equal(c2, cls) and torch.equal(r2, cor)


# ---------------- module level ----------------
B, H = 8, 64


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    x_u8 = torch.randint(0, 256, (B, 1, H, H), generator=g, dtype=torch.uint8)
    one_hot = torch.nn.functional.one_hot
    return {"x-ray": ((x_u8.float() - 127.5) / 73.9).repeat(1, 3, 1, 1),
            "tumor": torch.randint(0, 2, (B,), generator=g),
            "dataset": ["INTERNAL" if (i + seed) % 2 else "BTXRD" for i in range(B)],
            "anatomy_site_encoded": one_hot(torch.randint(0, 9, (B,), generator=g), 9).float(),
            "age_encoded": one_hot(torch.randint(0, 4, (B,), generator=g), 4).float(),
            "sex_encoded": one_hot(torch.randint(0, 2, (B,), generator=g), 2).float()}


def _modules(kind):
    opt = functools.partial(torch.optim.AdamW, lr=1e-3)
    if kind == "fusion":
        from src.models.baseline.FusionModule import FusionModule as M
    else:
        from src.models.baseline.OnlyImagingModule import OnlyImagingModule as M
    make = functools.partial(M, "resnet34", opt, label_weights=(0.7, 2.0), coral_lambda=0.5, compute_dtype="fp32")
    torch.manual_seed(33)
    off = make()
    on = make(loss_on_device=True)
    on.load_state_dict(off.state_dict())
    assert off.hparams.loss_on_device is False and on.hparams.loss_on_device is True
    return off, on


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.mark.parametrize("kind", ["fusion", "only_imaging"])
def test_training_step_and_combined_validation_match_the_torch_path(kind):
    """One training step + backward and one validation epoch, flag off against flag on, same seeded
    weights and batches: the logged losses to 1e-5 relative (the fp32 torch path's own error
    against fp64, the golden tolerance), every parameter gradient and the tower's flat gradient
    arena to rel-L2 1e-3 (the envelope of tests/test_fusion.py's 64 px step against its oracle)."""
    off, on = _modules(kind)
    logs = []
    for m in (off, on):
        m.train()
        m.training_step(_batch(1), 0).backward()
        m.eval()
        with torch.no_grad():
            m.validation_step(_batch(2), 0, 0)
            m.validation_step(_batch(3), 0, 1)
        m.on_validation_epoch_end()
        logs.append({k: float(v.detach()) if torch.is_tensor(v) else v for k, v in m.logged.items()})
    torch.cuda.synchronize()
    a, b = logs
    keys = ["train/loss", "train/classification_loss", "train/coral_loss", "val/combined/loss",
            "val/combined/classification_loss", "val/combined/coral_loss"]
    for k in keys:
        print(f"{kind} {k}: torch path {a[k]!r} device op {b[k]!r}")
        assert a[k] > 0.0 and abs(a[k] - b[k]) <= 1e-5 * abs(a[k]), (k, a[k], b[k])
    tower = "image_network" if kind == "fusion" else "network"
    e = _rel(getattr(on, tower).arena.grad, getattr(off, tower).arena.grad)
    print(f"{kind} flat gradient arena rel-L2 {e:.2e}")
    assert getattr(off, tower).arena.grad.norm().item() > 0.0 and e <= 1e-3, e
    pon = dict(on.named_parameters())
    checked = 0
    for name, p in off.named_parameters():
        if p.grad is None:
            assert pon[name].grad is None, name
            continue
        if p.grad.norm().item() < 1e-6:           # analytically 0 (a bias that feeds a BatchNorm)
            assert pon[name].grad.norm().item() < 1e-6, name
            continue
        e = _rel(pon[name].grad, p.grad)
        assert e <= 1e-3, (name, e)
        checked += 1
    assert checked >= 40      # stem, downsample convs, the BNs, the head (convs behind a zero-initialised BN are 0)


def test_device_path_makes_no_host_synchronisation():
    from src.models.baseline.OnlyImagingModule import OnlyImagingModule
    m = OnlyImagingModule("resnet34", None, label_weights=(0.7, 2.0), coral_lambda=1000.0, loss_on_device=True)
    g = torch.Generator().manual_seed(5)
    feats = torch.randn(B, 512, 1, 1, generator=g).cuda().requires_grad_()
    logits = torch.randn(B, generator=g).cuda().requires_grad_()
    labels = torch.randint(0, 2, (B,), generator=g)
    dataset = _batch(0)["dataset"]
    m._compute_loss(feats, logits, labels, dataset)[0].backward()      # warm up: library load, allocator
    feats.grad = logits.grad = None
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device="cuda").sum().item()
            live = False
        except RuntimeError:
            live = True
        if not live:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') is inert on this torch build: .item() did not raise")
        tot, cls, cor = m._compute_loss(feats, logits, labels, dataset)
        tot.backward()
        with torch.no_grad():
            m._compute_loss(feats.detach(), logits.detach(), labels, dataset)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert cor.item() > 0.0 and feats.grad.abs().sum().item() > 0.0 and logits.grad.abs().sum().item() > 0.0
