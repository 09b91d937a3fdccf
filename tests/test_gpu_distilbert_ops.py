"""DistilBERT-shaped text kernels vs the HF DistilBertModel sub-modules they
replace (the reference's default text encoder, VisionLanguageModule.py:43,
:57-60): attention heads of 64 (the DP = 64 instantiations of vlp_attn_fwd /
vlp_attn_bwd, dynamic LDS), LayerNorm rows of 768, embeddings without a
token-type table.

  attention  H = 12, dh = 64 at T = 12 / 40 (the T <= 48 tile) and T = 64 (the full
             tile), and H = 3, dh = 48 (channel masking inside the 64-wide padding),
             against the torch restatement of HF's eager attention in fp64; the
             restatement itself is held to a 1-layer DistilBertModel on the CPU
  dropout    p = 0.1 at dh = 64: with V = the first T identity columns the context
             IS P', so the mask is read off the output
  LayerNorm  D = 768 (M = 37: a row tail), D = 520 (first size past the old 512
             bound, partial last chunk group), D = 312 (regression)
  embeddings tt = None, temb = None vs HF DistilBERT Embeddings at dropout 0

Tolerances are tests/test_gpu_bert_ops.py's: fp32 storage rel-L2 <= 2e-5 (attention
backward and embedding gradients 5e-5); bf16 storage <= 2e-2 against fp64 math on the
same bf16-rounded inputs.
"""
import math

import pytest
import torch

DT = [torch.float32, torch.bfloat16]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def tol(dt, fp32=2e-5):
    return fp32 if dt == torch.float32 else 2e-2


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vlp_amd import ops as o
    return o


def masks(B, T, g):
    """attention_mask rows with 1 + L ~ U{8..T-2} + 1 valid tokens (CLS ... SEP)."""
    am = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        L = int(torch.randint(min(8, T - 2), T - 1, (1,), generator=g))
        am[b, :L + 2] = 1
    am[0, :] = 1   # one full-length caption
    return am


def ref_attention(qkv, am, T, H, dh, scale, drop=None):
    """HF eager attention (modeling_distilbert eager_attention_forward) on projected
    q|k|v rows [B*T, 3*H*dh]; drop = the dropout multiplier on P ([B, H, T, T])."""
    B = qkv.shape[0] // T
    q, k, v = qkv.view(B, T, 3, H, dh).permute(2, 0, 3, 1, 4)       # [B, H, T, dh] each
    s = q @ k.transpose(-1, -2) * scale
    s = s + (1.0 - am[:, None, None, :].to(s.dtype)) * torch.finfo(s.dtype).min
    p = torch.softmax(s, dim=-1)
    pd = p if drop is None else p * drop
    ctx = (pd @ v).permute(0, 2, 1, 3).reshape(B * T, H * dh)
    return ctx, p


def test_reference_attention_is_hf_distilbert_attention():
    """CPU: the restatement equals the attention context of a 1-layer HF
    DistilBertModel (hooks: the embeddings' output, out_lin's input)."""
    from transformers import DistilBertConfig, DistilBertModel
    torch.manual_seed(0)
    cfg = DistilBertConfig(n_layers=1, dropout=0.0, attention_dropout=0.0)
    m = DistilBertModel(cfg).eval()
    B, T, H, dh = 4, 40, cfg.n_heads, cfg.dim // cfg.n_heads
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(1000, 30000, (B, T), generator=g)
    am = masks(B, T, g)
    cap = {}
    m.embeddings.register_forward_hook(lambda mod, i, o: cap.__setitem__("h", o))
    at = m.transformer.layer[0].attention
    at.out_lin.register_forward_hook(lambda mod, i, o: cap.__setitem__("ctx", i[0]))
    with torch.no_grad():
        m(input_ids=ids, attention_mask=am)
    h = cap["h"].reshape(B * T, cfg.dim)
    qkv = torch.cat([h @ at.q_lin.weight.T + at.q_lin.bias, h @ at.k_lin.weight.T + at.k_lin.bias,
                     h @ at.v_lin.weight.T + at.v_lin.bias], 1)
    ctx, _ = ref_attention(qkv, am, T, H, dh, 1 / math.sqrt(dh))
    assert rel(ctx, cap["ctx"].reshape(B * T, cfg.dim)) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("H,dh,B,T", [(12, 64, 3, 12), (12, 64, 2, 40), (12, 64, 2, 64), (3, 48, 2, 40)])
def test_attention_fwd_bwd(ops, dt, H, dh, B, T):
    D = H * dh
    g = torch.Generator().manual_seed(T + dh)
    am = masks(B, T, g)
    qkv = torch.randn(B * T, 3 * D, generator=g).to(dt).float()
    dctx = torch.randn(B * T, D, generator=g).to(dt).float()
    scale = 1 / math.sqrt(dh)
    x = qkv.clone().double().requires_grad_()
    ctx_ref, p_ref = ref_attention(x, am, T, H, dh, scale)
    ctx_ref.backward(dctx.double())
    qd, amd = qkv.to(dt).cuda(), am.cuda()
    # NaN-filled outputs: every element the kernels own must be written
    ctx = torch.full((B * T, D), float("nan"), dtype=dt, device="cuda")
    P = torch.full((B, H, T, T), float("nan"), device="cuda")
    ops.attn_fwd(qd, amd, ctx, P, B, T, H, dh, scale)
    dq = torch.full_like(qd, float("nan"))
    ops.attn_bwd(qd, P, dctx.to(dt).cuda(), dq, B, T, H, dh, scale)
    torch.cuda.synchronize()
    r_p, r_c, r_d = rel(P, p_ref), rel(ctx.float(), ctx_ref), rel(dq.float(), x.grad)
    print(f"attn H={H} dh={dh} B={B} T={T} {dt}: P {r_p:.3e} ctx {r_c:.3e} dqkv {r_d:.3e}")
    assert r_p < tol(dt)
    assert r_c < tol(dt)
    # padded (masked) keys get exactly zero probability
    pm = P.cpu()[am[:, None, None, :].expand(B, H, T, T) == 0]
    assert pm.numel() and pm.abs().max().item() == 0.0
    assert r_d < tol(dt, 5e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DT)
def test_attention_dropout_dh64(ops, dt):
    """V = the first T columns of the identity per head: ctx[:, :T] is P' = mask * P."""
    H, dh, B, T, p, seed = 12, 64, 2, 40, 0.1, 1234
    D = H * dh
    g = torch.Generator().manual_seed(7)
    am = masks(B, T, g)
    qkv = torch.randn(B, T, 3, H, dh, generator=g)
    qkv[:, :, 2] = torch.eye(T, dh)[None, :, None, :]               # V[b, j, h, d] = (d == j)
    qkv = qkv.reshape(B * T, 3 * D).to(dt).float()
    v = qkv.view(B, T, 3, H, dh)[:, :, 2]
    assert torch.equal(v[0, :, 0, :T], torch.eye(T)) and torch.equal(v[1, :, 5, :T], torch.eye(T))
    scale = 1 / math.sqrt(dh)
    qd, amd = qkv.to(dt).cuda(), am.cuda()
    outs = []
    for _ in range(2):
        ctx = torch.empty(B * T, D, dtype=dt, device="cuda")
        P = torch.empty(B, H, T, T, device="cuda")
        ops.attn_fwd(qd, amd, ctx, P, B, T, H, dh, scale, p=p, seed=seed)
        outs.append((ctx, P))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])   # bit-identical
    ctx, P = outs[0][0].float().cpu(), outs[0][1].cpu()
    pd = ctx.view(B, T, H, dh)[..., :T].permute(0, 2, 1, 3)          # P' [B, H, i, j]
    big = P > 1e-3                                                    # entries with a well-defined ratio
    ratio = pd[big] / P[big]
    keep = ratio > 0.5
    # the mask holds only 0 and 1/(1-p) (bf16: P' was rounded to bf16 twice, 2^-8 each)
    rt = 1e-5 if dt == torch.float32 else 2 ** -7
    assert (ratio[~keep] == 0).all()
    assert ((ratio[keep] * (1 - p) - 1).abs() < rt).all()
    n = int(big.sum())
    share = keep.double().mean().item()
    sigma = math.sqrt(p * (1 - p) / n)
    print(f"dropout {dt}: n {n} kept share {share:.5f} (1-p {1 - p}, sigma {sigma:.2e})")
    assert n > 10000 and abs(share - (1 - p)) < 4 * sigma
    # backward with the same seed == fp64 autograd through the restatement with that mask
    drop = (pd != 0).double() / (1 - p)
    dctx = torch.randn(B * T, D, generator=g).to(dt).float()
    x = qkv.clone().double().requires_grad_()
    ctx_ref, _ = ref_attention(x, am, T, H, dh, scale, drop=drop)
    ctx_ref.backward(dctx.double())
    dq = torch.empty_like(qd)
    ops.attn_bwd(qd, outs[0][1], dctx.to(dt).cuda(), dq, B, T, H, dh, scale, p=p, seed=seed)
    torch.cuda.synchronize()
    assert rel(ctx, ctx_ref) < tol(dt)
    r = rel(dq.float(), x.grad)
    print(f"dropout {dt}: dqkv rel-L2 {r:.3e}")
    assert r < tol(dt, 5e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,D", [(37, 768), (37, 520), (37, 312)])
def test_layernorm_fwd_bwd(ops, dt, M, D):
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(M, D, generator=g) * 3 + 1).to(dt).float()
    dy = torch.randn(M, D, generator=g).to(dt).float()
    ln = torch.nn.LayerNorm(D, eps=1e-12).double()      # sa_layer_norm / output_layer_norm / embeddings.LayerNorm
    with torch.no_grad():
        ln.weight.copy_(torch.rand(D, generator=g) + 0.5)
        ln.bias.copy_(torch.randn(D, generator=g) * 0.1)
    xr = x.double().requires_grad_()
    y_ref = ln(xr)
    y_ref.backward(dy.double())
    xd = x.to(dt).cuda()
    y = torch.full_like(xd, float("nan"))
    mu, rs = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    w, b = ln.weight.detach().float().cuda(), ln.bias.detach().float().cuda()
    ops.layernorm_fwd(xd, w, b, 1e-12, y, mu, rs, M, D)
    dx = torch.full_like(xd, float("nan"))
    dgam, dbet = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    ops.layernorm_bwd(dy.to(dt).cuda(), xd, mu, rs, w, dx, None, dgam, dbet, M, D)
    torch.cuda.synchronize()
    r = [rel(y.float(), y_ref), rel(dx.float(), xr.grad), rel(dgam, ln.weight.grad), rel(dbet, ln.bias.grad)]
    print(f"layernorm M={M} D={D} {dt}: y {r[0]:.3e} dx {r[1]:.3e} dgamma {r[2]:.3e} dbeta {r[3]:.3e}")
    assert all(v < tol(dt) for v in r), r


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DT)
def test_embeddings_without_token_types(ops, dt):
    """word + position rows -> LayerNorm (HF DistilBERT Embeddings, dropout 0)."""
    from transformers import DistilBertConfig
    from transformers.models.distilbert.modeling_distilbert import Embeddings
    cfg = DistilBertConfig(dropout=0.0)
    D = cfg.dim
    torch.manual_seed(0)
    emb = Embeddings(cfg).double().eval()
    B, T = 4, 40
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, cfg.vocab_size, (B, T), generator=g)
    ids[:, 5] = ids[:, 9]                     # repeated tokens: scatter-add collisions
    ids[:, -3:] = 0                           # padding id: nn.Embedding(padding_idx=0) gets no gradient
    out_ref = emb(input_ids=ids)
    gout = torch.randn(B, T, D, generator=g).to(dt).float()
    out_ref.backward(gout.double())
    M = B * T
    W_, P_ = emb.word_embeddings.weight.detach().float().cuda(), emb.position_embeddings.weight.detach().float().cuda()
    lw, lb = emb.LayerNorm.weight.detach().float().cuda(), emb.LayerNorm.bias.detach().float().cuda()
    e = torch.empty(M, D, dtype=dt, device="cuda")
    idc = ids.cuda().reshape(-1).contiguous()
    ops.embed_fwd(idc, None, W_, P_, None, e, M, T, D)
    h = torch.empty_like(e)
    mu, rs = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    ops.layernorm_fwd(e, lw, lb, 1e-12, h, mu, rs, M, D)
    de = torch.empty_like(e)
    dlw, dlb = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    ops.layernorm_bwd(gout.reshape(M, D).to(dt).cuda(), e, mu, rs, lw, de, None, dlw, dlb, M, D)
    dW, dP = torch.zeros_like(W_), torch.zeros_like(P_)
    ops.embed_bwd(idc, None, de, dW, dP, None, M, T, D)
    torch.cuda.synchronize()
    assert rel(h.float(), out_ref.reshape(M, D)) < tol(dt)
    rows = torch.unique(ids)
    rows = rows[rows != 0]
    gW = emb.word_embeddings.weight.grad
    assert rel(dW.cpu()[rows], gW[rows]) < tol(dt, 5e-5)
    assert dW.cpu()[0].abs().max().item() == 0.0 and gW[0].abs().max().item() == 0.0     # the padding row
    assert dW.cpu().abs().sum().item() == pytest.approx(dW.cpu()[rows].abs().sum().item())   # untouched rows stay 0
    assert rel(dP.cpu()[:T], emb.position_embeddings.weight.grad[:T]) < tol(dt, 5e-5)
    assert dP.cpu()[T:].abs().max().item() == 0.0
    assert rel(dlw, emb.LayerNorm.weight.grad) < tol(dt) and rel(dlb, emb.LayerNorm.bias.grad) < tol(dt)


@pytest.mark.gpu
def test_rejections(ops):
    """Argument checks that return hipErrorInvalidValue before any launch."""
    H, T = 2, 8
    qkv = torch.zeros(T, 3 * H * 65, device="cuda")
    ctx, P = torch.zeros(T, H * 65, device="cuda"), torch.zeros(H * T * T, device="cuda")
    with pytest.raises(RuntimeError):
        ops.attn_fwd(qkv, None, ctx, P, 1, T, H, 65, 0.1)
    with pytest.raises(RuntimeError):
        ops.attn_bwd(qkv, P, ctx, torch.zeros_like(qkv), 1, T, H, 65, 0.1)
    x = torch.zeros(4, 1032, device="cuda")
    v, s = torch.zeros(1032, device="cuda"), torch.zeros(4, device="cuda")
    with pytest.raises(RuntimeError):
        ops.layernorm_fwd(x, v, v, 1e-12, torch.zeros_like(x), s, s, 4, 1032)
    with pytest.raises(RuntimeError):
        ops.layernorm_bwd(x, x, s, s, v, torch.zeros_like(x), None, torch.zeros_like(v), torch.zeros_like(v), 4, 1032)
    torch.cuda.synchronize()
