"""ViT kernels against plain torch references.

  attention  vlp_vit_attn_fwd / _bwd (the flash-attention kernels of csrc/nest_ops.hip
             at head dim 64) vs fp64 softmax(q k^T / 8) v and its autograd: out, lse and
             every column of dqkv; tile edges of 64 and 128 tokens and the real token
             count 197; rows past the last token poisoned with NaN; run-to-run bit equality
  patch      vlp_vit_patch_prep vs F.unfold (bit-exact), both input forms
  assemble   vlp_vit_assemble vs cat((cls, patch), 1) + pos (exact)

Tolerances (attention): for each checked tensor the HIP error is a rel-L2 against
fp64, gated at 4 x the error of the same computation in plain torch on the CPU at the
kernel's precision (fp32 throughout, or bf16-rounded operands / stored tensors with
fp32 accumulation) against the same fp64 values, with a floor of 1e-6 (fp32) or 2e-3
(bf16).  The factor 4 allows for a different summation order and the exp2-domain
softmax.  Both errors are printed (pytest -s).
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DT = [torch.float32, torch.bfloat16]
DH = 64
PAD = 64            # poisoned rows behind the last token


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlp_amd import ops as o
    return o


def heads(qkv, B, N, H):
    return qkv.view(B, N, 3, H, DH).permute(2, 0, 3, 1, 4)               # 3 x [B, H, N, 64]


def attn_fp64(qkv, do, B, N, H):
    x = qkv.double().requires_grad_()
    q, k, v = heads(x, B, N, H)
    o = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(B * N, H * DH)
    o.backward(do.double())
    with torch.no_grad():
        lse = torch.logsumexp(q @ k.transpose(-1, -2) / math.sqrt(DH), -1) / math.log(2)
    return o.detach(), lse.reshape(-1), x.grad


def attn_cpu_at_precision(qkv, do, B, N, H, dt):
    """The flash-attention arithmetic in plain fp32 torch; for bf16 every MFMA operand
    (P, dS) and every stored tensor (out, dqkv) is rounded to bf16, sums stay fp32."""
    r = (lambda t: t.to(torch.bfloat16).float()) if dt == torch.bfloat16 else (lambda t: t)
    sc = 1 / math.sqrt(DH)
    q, k, v = heads(qkv.float(), B, N, H)
    s = q @ k.transpose(-1, -2) * sc
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    out = r(r(p) @ v)                                                        # [B, H, N, 64]
    dh_ = do.float().view(B, N, H, DH).permute(0, 2, 1, 3)
    delta = (dh_ * out).sum(-1, keepdim=True)
    ds = p * (dh_ @ v.transpose(-1, -2) - delta)
    dv = r(p).transpose(-1, -2) @ dh_
    dq = r(ds) @ k * sc
    dk = r(ds).transpose(-1, -2) @ q * sc
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B * N, H * DH)
    dqkv = r(torch.cat([back(dq), back(dk), back(dv)], 1))
    return back(out), (lse / math.log(2)).reshape(-1), dqkv


@pytest.mark.parametrize("dt", DT, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,H", [(1, 1), (2, 3)])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 128, 129, 197])
def test_attention_fwd_bwd(ops, dt, B, H, N):
    g = torch.Generator().manual_seed(1000 * N + 10 * H + B)
    C = DH * H
    qkv = torch.randn(B * N, 3 * C, generator=g)
    qkv[:, :2 * C] *= 0.6                     # logits q.k/8 ~ N(0, 0.36^2): a few units across a row
    qkv = qkv.to(dt).float()
    do = torch.randn(B * N, C, generator=g).to(dt).float()
    o_ref, lse_ref, dqkv_ref = attn_fp64(qkv, do, B, N, H)
    o_cpu, lse_cpu, dqkv_cpu = attn_cpu_at_precision(qkv, do, B, N, H, dt)
    R = B * N

    def padded(t):                            # the tensor followed by PAD rows of NaN
        buf = torch.full((R + PAD, t.shape[1]), float("nan"), dtype=dt, device="cuda")
        buf[:R] = t.to(dt)
        return buf

    runs = []
    for _ in range(2):
        qd, dod = padded(qkv), padded(do)
        out = torch.full((R + PAD, C), float("nan"), dtype=dt, device="cuda")
        dqkv = torch.full((R + PAD, 3 * C), float("nan"), dtype=dt, device="cuda")
        lse = torch.full((B * H * N + PAD,), float("nan"), device="cuda")
        delta = torch.full((B * H * N + PAD,), float("nan"), device="cuda")
        ops.vit_attn_fwd(qd, out, lse, B, H, N, 1 / math.sqrt(DH))
        ops.vit_attn_bwd(qd, out, dod, lse, delta, dqkv, B, H, N, 1 / math.sqrt(DH))
        torch.cuda.synchronize()
        runs.append((out.cpu(), lse.cpu(), dqkv.cpu()))
    (out, lse, dqkv), (out2, lse2, dqkv2) = runs
    # nothing written behind the last row, nothing read from there: every result is finite
    assert torch.isnan(out[R:].float()).all() and torch.isnan(dqkv[R:].float()).all()
    assert torch.isnan(lse[B * H * N:]).all()
    assert torch.isfinite(out[:R].float()).all() and torch.isfinite(lse[:B * H * N]).all()
    assert torch.isfinite(dqkv[:R].float()).all(), "dqkv: a column was not written or the tail leaked in"
    # no atomics, fixed summation order: bitwise reproducible
    assert torch.equal(out[:R], out2[:R]) and torch.equal(lse[:B * H * N], lse2[:B * H * N])
    assert torch.equal(dqkv[:R], dqkv2[:R])
    floor = 1e-6 if dt == torch.float32 else 2e-3
    for name, got, cpu, ref in (("out", out[:R], o_cpu, o_ref), ("lse", lse[:B * H * N], lse_cpu, lse_ref),
                                ("dq", dqkv[:R, :C], dqkv_cpu[:, :C], dqkv_ref[:, :C]),
                                ("dk", dqkv[:R, C:2 * C], dqkv_cpu[:, C:2 * C], dqkv_ref[:, C:2 * C]),
                                ("dv", dqkv[:R, 2 * C:], dqkv_cpu[:, 2 * C:], dqkv_ref[:, 2 * C:])):
        if N == 1 and name in ("dq", "dk"):
            # one key: the softmax is constant and the true gradient is exactly 0.  What is left is
            # dO.V - delta, two 64-term fp32 dot products of the same terms in different orders
            # (each within 64 eps of sum |dO_d V_d|), times |q| or |k| / 8
            v = qkv[:, 2 * C:].view(R, H, DH)
            terms = (do.view(R, H, DH).abs() * v.abs()).sum(-1).max().item()
            bound = 2 * 64 * 2.0 ** -24 * terms * qkv[:, :2 * C].abs().max().item() / 8
            assert got.float().abs().max().item() <= bound, (name, got.float().abs().max().item(), bound)
            continue
        e_hip, e_cpu = rel(got.float(), ref), rel(cpu, ref)
        print(f"vit_attn {name:3s} {'bf16' if dt == torch.bfloat16 else 'fp32'} B{B} H{H} N{N}: "
              f"hip {e_hip:.3e} cpu {e_cpu:.3e}")
        assert e_hip <= max(4 * e_cpu, floor), (name, e_hip, e_cpu)


def test_attention_rejects_other_head_dims(ops):
    from vlp_amd._lib import lib
    t = torch.zeros(64 * 3 * 64, device="cuda")
    for fn, dh in ((lib().vlp_vit_attn_fwd, 32), (lib().vlp_nest_attn_fwd, 64)):
        with pytest.raises(RuntimeError):
            fn(0, 1, 1, 64, dh, t.data_ptr(), t.data_ptr(), t.data_ptr(), 0.1, None)


@pytest.mark.parametrize("dt", DT, ids=["fp32", "bf16"])
@pytest.mark.parametrize("u8", [False, True], ids=["f32x3", "u8"])
def test_patch_prep_is_unfold(ops, dt, u8):
    g = torch.Generator().manual_seed(5)
    B, Hi, Wi = 2, 32, 48
    if u8:
        xu = torch.randint(0, 256, (B, 1, Hi, Wi), generator=g, dtype=torch.uint8)
        inv = torch.tensor(1.0) / torch.tensor(73.9)
        x = ((xu.float() - 127.5) * inv).expand(B, 3, Hi, Wi).contiguous()
    else:
        x = torch.randn(B, 3, Hi, Wi, generator=g)
    P = (Hi // 16) * (Wi // 16)
    ref = F.unfold(x, 16, stride=16).transpose(1, 2).reshape(B * P, 768)      # columns (c, ky, kx)
    out = torch.full((B * P, 768), float("nan"), dtype=dt, device="cuda")
    if u8:
        ops.vit_patch_prep(out, B, Hi, Wi, x_u8=xu.cuda(), mean=127.5, std=73.9)
    else:
        ops.vit_patch_prep(out, B, Hi, Wi, x=x.cuda())
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref.to(dt))            # fp32 bit-exact; bf16 = the rounded fp32
    # the GEMM weight is patch_embed.proj.weight.view(D, 768) as stored
    w = torch.randn(8, 3, 16, 16, generator=g)
    conv = F.conv2d(x, w, stride=16).flatten(2).transpose(1, 2).reshape(B * P, 8)
    assert rel(ref @ w.view(8, 768).T, conv) < 1e-5
    with pytest.raises(RuntimeError):
        ops.vit_patch_prep(out, B, 40, 48, x=x.cuda())
    with pytest.raises(RuntimeError):
        ops.vit_patch_prep(out, B, Hi, Wi)


@pytest.mark.parametrize("dt", DT, ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,N,D", [(3, 5, 768), (2, 197, 1024)])
def test_assemble_is_exact(ops, dt, B, N, D):
    g = torch.Generator().manual_seed(N)
    patch = torch.randn(B * (N - 1), D, generator=g).to(dt)
    cls, pos = torch.randn(D, generator=g), torch.randn(N, D, generator=g)
    ref = (torch.cat([cls.expand(B, 1, D), patch.float().view(B, N - 1, D)], 1) + pos).to(dt)
    tok = torch.full((B * N, D), float("nan"), dtype=dt, device="cuda")
    ops.vit_assemble(patch.cuda(), cls.cuda(), pos.cuda(), tok, B, N, D)
    torch.cuda.synchronize()
    assert torch.equal(tok.cpu().view(B, N, D), ref)
