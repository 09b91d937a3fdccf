"""ViT tower (vlp_amd/vit.py) on the HIP kernels against tests/vit_ref.py in fp64:
forward features and every parameter gradient of a two-block vit_base_patch16_224
on name-keyed deterministic weights, at 32 px (N = 5 tokens, B = 3) and 224 px
(N = 197, B = 2), both pool modes, fp32 and bf16, both input forms; then one
VisionLanguageModule step (ViT + TinyBERT) against the fp64 restatement and one
fused AdamW step.

Tolerances: each checked tensor's HIP error (rel-L2 against fp64) is gated at 4 x the
error of the same model in plain torch on the CPU at the kernel's precision -- fp32
throughout, or (bf16) fp32 arithmetic with every GEMM weight operand and every stored
activation and activation gradient rounded to bf16 -- against the same fp64 values,
with a floor of 1e-6 (fp32) or 2e-3 (bf16).  Both errors are printed (pytest -s).
"""
import functools

import pytest
import torch

from tests.golden.synth import synth_batch
from tests.vit_ref import ViTRef, deterministic_weights

pytestmark = pytest.mark.gpu
DEPTH = 2


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


class _RoundBF16(torch.autograd.Function):
    """A tensor stored in bf16: the value on the way forward, its gradient on the way back."""

    @staticmethod
    def forward(ctx, t):
        return t.to(torch.bfloat16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def _wq_bf16(w):
    return w + (w.detach().to(torch.bfloat16).to(w.dtype) - w.detach())     # operand copy; fp32 master gradient


@functools.lru_cache(maxsize=None)
def _weights(size, pool):
    ref = ViTRef(768, DEPTH, 12, 3072, size, pool)
    return deterministic_weights([(k, tuple(p.shape)) for k, p in ref.named_timm_parameters()])


@functools.lru_cache(maxsize=None)
def _inputs(size, B, u8):
    g = torch.Generator().manual_seed(size + B)
    if u8:
        xu = torch.randint(0, 256, (B, 1, size, size), generator=g, dtype=torch.uint8)
        x = ((xu.float() - 127.5) * (torch.tensor(1.0) / torch.tensor(73.9))).expand(B, 3, size, size).contiguous()
    else:
        xu, x = None, torch.randn(B, 3, size, size, generator=g)
    dfeat = torch.randn(B, 768, generator=g)
    return xu, x, dfeat


def _run_ref(size, pool, x, dfeat, dtype, bf16=False):
    m = ViTRef(768, DEPTH, 12, 3072, size, pool).to(dtype)
    m.load_timm_state_dict(_weights(size, pool))
    kw = dict(act=_RoundBF16.apply, wq=_wq_bf16) if bf16 else {}
    f = m(x.to(dtype), **kw)
    f.backward(dfeat.to(dtype))
    return f.detach(), {k: p.grad for k, p in m.named_timm_parameters()}


@functools.lru_cache(maxsize=None)
def _reference(size, B, pool, u8):
    """fp64 values and the CPU errors at fp32 / bf16 precision, computed once per shape."""
    _, x, dfeat = _inputs(size, B, u8)
    f64, g64 = _run_ref(size, pool, x, dfeat, torch.float64)
    cpu = {}
    for name, bf in (("fp32", False), ("bf16", True)):
        f, g = _run_ref(size, pool, x, dfeat, torch.float32, bf16=bf)
        cpu[name] = (rel(f, f64), {k: rel(g[k], g64[k]) for k in g64})
    return f64, g64, cpu


@pytest.mark.parametrize("u8", [False, True], ids=["f32x3", "u8"])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("pool", ["token", "avg"])
@pytest.mark.parametrize("size,B", [(32, 3), (224, 2)])
def test_tower_vs_fp64(size, B, pool, mode, u8):
    from vlp_amd.vit import ViTTower
    xu, x, dfeat = _inputs(size, B, u8)
    f64, g64, cpu = _reference(size, B, pool, u8)
    t = ViTTower("vit_base_patch16_224", img_size=size, compute_dtype=mode, device="cuda", depth=DEPTH,
                 global_pool=pool)
    missing = t.load_state_dict({k: v.float() for k, v in _weights(size, pool).items()})
    assert not missing.missing_keys and not missing.unexpected_keys
    t.train()
    feat = t((xu if u8 else x).cuda())
    assert feat.shape == (B, 768) and feat.dtype == torch.float32
    feat.backward(dfeat.cuda())
    torch.cuda.synchronize()
    floor = 1e-6 if mode == "fp32" else 2e-3
    e_cpu_f, e_cpu_g = cpu[mode]
    e = rel(feat, f64)
    print(f"vit_tower {size}px {pool} {mode} {'u8' if u8 else 'f32'}: feat hip {e:.3e} cpu {e_cpu_f:.3e}")
    bad = []
    if e > max(4 * e_cpu_f, floor):
        bad.append(("feat", e, e_cpu_f))
    params = dict(t.named_parameters())
    assert set(params) == set(g64)
    worst = (0.0, None, 0.0)
    for k, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        if g64[k].norm() == 0:
            assert p.grad.abs().max().item() == 0, k
            continue
        eg = rel(p.grad, g64[k])
        ratio = eg / max(4 * e_cpu_g[k], floor)
        if ratio > worst[0]:
            worst = (ratio, k, eg)
        if ratio > 1:
            bad.append((k, eg, e_cpu_g[k]))
    print(f"vit_tower {size}px {pool} {mode}: worst gradient {worst[1]} hip {worst[2]:.3e} "
          f"cpu {e_cpu_g[worst[1]]:.3e} (ratio to gate {worst[0]:.2f})")
    assert not bad, bad


def test_tower_rejects_other_input_sizes():
    from vlp_amd.vit import ViTTower
    t = ViTTower(img_size=32, compute_dtype="fp32", device="cuda", depth=1)
    with pytest.raises(ValueError):
        t(torch.zeros(1, 3, 48, 48, device="cuda"))


def test_clip_step_vit_tinybert_vs_fp64():
    """One VisionLanguageModule step with image_model="vit_base_patch16_224" (two blocks,
    32 px, B = 4, fp32, dropout 0): loss and every gradient against the fp64 restatement
    (ViTRef + the oracle's TinyBERT and CLIP head), gated as above against the same
    restatement in fp32 on the CPU; then one fused AdamW step moves every parameter that
    has a gradient."""
    from oracle.clip import OracleVLP, clip_forward, compute_loss
    from src.models.pretrain.VisionLanguageModule import VisionLanguageModule
    from vlp_amd.optim import FusedAdamW
    torch.manual_seed(0)
    m = VisionLanguageModule("vit_base_patch16_224", "tinybert", functools.partial(torch.optim.AdamW, lr=1e-3), False,
                             False, 768, 312, 128, compute_dtype="fp32", text_dropout=0.0, image_size=32,
                             image_depth=DEPTH)
    w = _weights(32, "avg")
    m.image_encoder.model.load_state_dict({k: v.float() for k, v in w.items()})
    m.train()
    b = synth_batch(4, 32, 12, 11)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}

    def restatement(dtype):
        o = OracleVLP(128, text_dropout=0.0).to(dtype)
        o.load_state_dict({k: v.to(dtype) for k, v in sd.items() if not k.startswith("image_")}, strict=False)
        o.train()
        vit = ViTRef(768, DEPTH, 12, 3072, 32, "avg").to(dtype)
        vit.load_timm_state_dict({k[len("image_encoder.model."):]: v for k, v in sd.items()
                                  if k.startswith("image_encoder.model.")})
        proj = sd["image_projection"].to(dtype).requires_grad_()
        logits, _, _ = clip_forward(vit(b["x-ray"].to(dtype)), o.text_encoder(**b["caption_tokenized"]), proj,
                                    o.text_projection, o.logit_scale)
        loss, _, _ = compute_loss(logits)
        loss.backward()
        g = {"image_encoder.model." + k: p.grad for k, p in vit.named_timm_parameters()}
        g.update({k: p.grad for k, p in o.named_parameters() if not k.startswith("image_")})
        g["image_projection"] = proj.grad
        return loss.detach(), g

    l64, g64 = restatement(torch.float64)
    l32, g32 = restatement(torch.float32)
    loss, _, _, _, _ = m.training_step_outputs(b)
    loss.backward()
    torch.cuda.synchronize()
    e, ec = abs(loss.item() - l64.item()) / abs(l64.item()), abs(l32.item() - l64.item()) / abs(l64.item())
    print(f"vit_clip loss hip {e:.3e} cpu {ec:.3e}")
    assert e <= max(4 * ec, 1e-6), (loss.item(), l64.item())
    bad, worst = [], (0.0, None, 0.0)
    with_grad = []
    for k, p in m.named_parameters():
        if p.grad is None:
            continue
        with_grad.append((k, p))
        # attention.self.key.bias: a constant added to every key of a query leaves the softmax
        # unchanged, so the true gradient is 0 and both sides hold rounding noise
        if g64.get(k) is None or g64[k].norm() == 0 or k.endswith("attention.self.key.bias"):
            continue
        eg, ecg = rel(p.grad, g64[k]), rel(g32[k], g64[k])
        ratio = eg / max(4 * ecg, 1e-6)
        if ratio > worst[0]:
            worst = (ratio, k, eg, ecg)
        if ratio > 1:
            bad.append((k, eg, ecg))
    print(f"vit_clip worst gradient {worst[1]} hip {worst[2]:.3e} cpu {worst[3]:.3e} (ratio to gate {worst[0]:.2f})")
    assert any(k.startswith("image_encoder.model.blocks.1.attn.qkv") for k, _ in with_grad)
    assert not bad, bad
    opt = m.configure_optimizers()["optimizer"]
    assert isinstance(opt, FusedAdamW)
    before = {k: p.detach().clone() for k, p in with_grad}
    opt.step()
    torch.cuda.synchronize()
    # a parameter whose gradient is identically zero still decays (weight_decay) unless it is zero itself
    still = [k for k, p in with_grad if torch.equal(p.detach(), before[k]) and p.grad.abs().max() > 0]
    assert not still, still
