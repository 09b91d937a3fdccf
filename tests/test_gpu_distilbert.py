"""DistilBertTower and the distilbert VisionLanguageModule vs HF DistilBertModel in
fp64 (the reference's default text encoder, VisionLanguageModule.py:43, :57-60).

Tower: 2 layers at full width (hidden 768, 12 heads of 64, FFN 3072), HF init
from seed 0 with the 1-D parameters perturbed (HF starts every bias at 0 and every
LayerNorm at 1/0, which would hide a misplaced bias), weights copied through
load_hf_state_dict.  B = 4 at T = 12 and 40 with padding masks; the loss is a
fixed random linear form on the CLS rows.  last_hidden_state and the gradient of
every parameter are compared per tensor, on the full path and on cls_only.

Bound.  The fp32 envelope of a tensor is rel-L2(HF fp32, HF fp64) on the same
inputs, measured on the CPU inside the test; HIP fp32 must stay within 10 x that
envelope (the margin for a different but equally valid fp32 summation order
across 2 layers).  The envelope is floored at 2^-23: a value stored in fp32
cannot be expected closer to fp64 than fp32's own spacing.  bf16: <= 2e-2 on
the hidden state, <= 5e-2 on gradients, or 10 x the fp32 envelope where that is
larger.  k_lin.bias: softmax is invariant to a key bias, so its true gradient is 0
and every implementation returns rounding noise; a ratio to that noise says
nothing.  Its error is therefore measured against the norm of the same layer's
q_lin.bias gradient (both are column sums of the attention backward's output over
the same rows, so their rounding noise has the same scale), in the envelope and
in the comparison alike.

Measured envelopes (HF fp32 vs fp64 on the CPU, this file's seeds; they move a
little with the CPU's BLAS, which is why the test measures them itself and prints
them) and what the HIP tower gave on an MI355X:
  T = 12: last_hidden_state 2.3e-7 .. 2.9e-7, gradients 1.2e-7 (the floor) .. 8.8e-7
  T = 40: last_hidden_state 2.2e-7 .. 2.9e-7, gradients 1.2e-7 .. 8.3e-7
  HIP fp32: hidden 5.5e-7 .. 5.8e-7 (2.6 x its envelope), worst gradient 2.5 x its
  envelope (layer 1 sa_layer_norm); HIP bf16: hidden 5.4e-3, gradients <= 6e-3.
Module step (B = 4, 64 px, T = 12, fp32): envelopes image_emb 4.4e-6, text_emb
4.1e-7; HIP 7.5e-6 and 1.0e-6; loss 1.4e-6 relative (see the test for its floor).
"""
import functools
import math

import pytest
import torch

B, LAYERS = 4, 2
FLOOR = 2.0 ** -23


def rel(a, b, scale=None):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / ((b if scale is None else scale.double().cpu()).norm() + 1e-300)).item()


def grad_rel(name, got, ref):
    """rel-L2 of one parameter's gradient; k_lin.bias (true gradient 0) on q_lin.bias's scale."""
    scale = ref[name.replace("k_lin.bias", "q_lin.bias")] if name.endswith("k_lin.bias") else None
    return rel(got[name].float(), ref[name], scale)


def inputs(T):
    g = torch.Generator().manual_seed(100 + T)
    ids = torch.randint(1000, 30000, (B, T), generator=g)
    am = torch.zeros(B, T, dtype=torch.long)
    for b in range(B):
        L = int(torch.randint(min(8, T - 2), T - 1, (1,), generator=g))
        am[b, :L + 2] = 1
    am[0, :] = 1
    ids = ids * am                                   # padding id 0 on masked positions, as the collator emits
    ids[:, 0] = 101
    ids[1, 3] = ids[1, 2]                            # a repeated token
    gcls = torch.randn(B, 768, generator=g)
    return ids, am, gcls


@functools.lru_cache(maxsize=None)
def hf_models():
    from transformers import DistilBertConfig, DistilBertModel
    torch.manual_seed(0)
    m = DistilBertModel(DistilBertConfig(n_layers=LAYERS, dropout=0.0, attention_dropout=0.0)).eval()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in m.parameters():
            if p.ndim == 1:
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    import copy
    return m, copy.deepcopy(m).double()


def hf_run(m, T):
    ids, am, gcls = inputs(T)
    m.zero_grad(set_to_none=True)
    h = m(input_ids=ids, attention_mask=am).last_hidden_state
    (h[:, 0, :] * gcls.to(h.dtype)).sum().backward()
    return h.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


@functools.lru_cache(maxsize=None)
def reference(T):
    """(fp64 hidden, fp64 grads, envelope per tensor) -- computed once per T, never modified."""
    m32, m64 = hf_models()
    h64, g64 = hf_run(m64, T)
    h32, g32 = hf_run(m32, T)
    env = {"last_hidden_state": max(rel(h32, h64), FLOOR), "cls": max(rel(h32[:, 0], h64[:, 0]), FLOOR)}
    for n in g64:
        env[n] = max(grad_rel(n, g32, g64), FLOOR)
    gs = [v for k, v in env.items() if k not in ("last_hidden_state", "cls")]
    print(f"envelope T={T}: last_hidden_state {env['last_hidden_state']:.3e} cls {env['cls']:.3e} "
          f"gradients {min(gs):.3e} .. {max(gs):.3e}")
    return h64, g64, env


def make_tower(dtype):
    from vlp_amd.distilbert import DistilBertConfig, DistilBertTower
    t = DistilBertTower(DistilBertConfig(0.0, 0.0, layers=LAYERS), compute_dtype=dtype, device="cuda")
    res = t.load_hf_state_dict({"distilbert." + k: v for k, v in hf_models()[0].state_dict().items()})
    assert not res.missing_keys and not res.unexpected_keys
    return t.train()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("cls_only", [False, True])
@pytest.mark.parametrize("T", [12, 40])
def test_tower_matches_hf_fp64(T, cls_only, dtype):
    h64, g64, env = reference(T)
    ids, am, gcls = inputs(T)
    t = make_tower(dtype)
    tt = torch.zeros_like(ids)                       # the collator always sends it; DistilBERT ignores it
    if cls_only:
        h, sv = t.run_forward(ids.cuda(), am.cuda(), tt.cuda(), True, cls_only=True)
        t.run_backward(sv, gcls.cuda())
        torch.cuda.synchronize()
        r_h, e_h = rel(h.float(), h64[:, 0]), env["cls"]
        grads = {n: t.arena.gview(n) for n in g64}
    else:
        h = t(input_ids=ids.cuda(), attention_mask=am.cuda(), token_type_ids=tt.cuda())
        (h[:, 0, :] * gcls.cuda()).sum().backward()
        torch.cuda.synchronize()
        r_h, e_h = rel(h, h64), env["last_hidden_state"]
        grads = {n: p.grad for n, p in t.named_parameters()}
    assert set(grads) == set(g64)
    fp32 = dtype == "fp32"
    bound_h = 10 * e_h if fp32 else max(2e-2, 10 * e_h)
    print(f"T={T} cls_only={cls_only} {dtype}: hidden rel-L2 {r_h:.3e} (envelope {e_h:.3e}, bound {bound_h:.3e})")
    bad = []
    worst = (0.0, None)
    for n, gr in g64.items():
        r = grad_rel(n, grads, g64)
        bound = 10 * env[n] if fp32 else max(5e-2, 10 * env[n])
        if r / env[n] > worst[0]:
            worst = (r / env[n], n)
        if not r <= bound:
            bad.append((n, r, env[n]))
    print(f"  worst gradient / envelope: {worst[0]:.2f} x ({worst[1]})")
    assert r_h <= bound_h, (r_h, e_h)
    assert not bad, bad


@pytest.fixture(scope="module")
def module_and_reference():
    """The distilbert module with recipe weights (image tower, projections) and
    HF-initialised text weights, and the fp64 / fp32 composition of the same step."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import copy
    from oracle import clip as oc
    from oracle import weights as W
    from oracle.resnet34 import create_model
    from tests.golden.synth import synth_batch
    from transformers import DistilBertConfig, DistilBertModel
    from src.models.pretrain.VisionLanguageModule import VisionLanguageModule
    m = VisionLanguageModule("resnet34", "distilbert", functools.partial(torch.optim.AdamW, lr=5e-5), False, False,
                             text_embedding_dim=768, embedding_dim=128, compute_dtype="fp32", text_dropout=0.0)
    torch.manual_seed(0)
    hf = DistilBertModel(DistilBertConfig(dropout=0.0, attention_dropout=0.0)).eval()
    sd = {}
    for k, v in m.state_dict().items():
        if k.startswith("text_encoder.model."):
            sd[k] = hf.state_dict()[k[len("text_encoder.model."):]]
        else:
            sd[k] = W.value_for(k, v.shape, 0).to(v.dtype)
    m.load_state_dict(sd)
    batch = synth_batch(4, 64, 12, 0)
    img = create_model("resnet34")
    img.load_state_dict({k[len("image_encoder.model."):]: v for k, v in sd.items()
                         if k.startswith("image_encoder.model.")})

    def compose(dt):
        im, tx = copy.deepcopy(img).to(dt).train(), copy.deepcopy(hf).to(dt)
        ct = batch["caption_tokenized"]
        with torch.no_grad():
            f_img = im(batch["x-ray"].to(dt))
            f_txt = tx(input_ids=ct["input_ids"], attention_mask=ct["attention_mask"]).last_hidden_state[:, 0, :]
            logits, ie, te = oc.clip_forward(f_img, f_txt, sd["image_projection"].to(dt),
                                             sd["text_projection"].to(dt), sd["logit_scale"].to(dt))
            loss, _, _ = oc.compute_loss(logits)
        return loss, ie, te, logits

    return m, hf, batch, compose(torch.float64), compose(torch.float32)


@pytest.mark.gpu
def test_module_structure(module_and_reference):
    m, hf = module_and_reference[:2]
    tower = m.text_encoder.model
    assert sum(p.numel() for p in tower.parameters()) == 66362880 == sum(p.numel() for p in hf.parameters())
    keys = [k[len("text_encoder.model."):] for k in m.state_dict() if k.startswith("text_encoder.model.")]
    assert keys == list(hf.state_dict().keys())
    from src.models.pretrain.VisionLanguageModule import VisionLanguageModule
    with pytest.raises(ValueError):
        VisionLanguageModule("resnet34", "distilbert", functools.partial(torch.optim.AdamW, lr=5e-5), False, False,
                             text_embedding_dim=312, embedding_dim=128)
    with pytest.raises(ValueError):
        VisionLanguageModule("resnet34", "tinybert", functools.partial(torch.optim.AdamW, lr=5e-5), False, False,
                             text_embedding_dim=768, embedding_dim=128)
    with pytest.raises(ValueError):
        VisionLanguageModule("resnet34", "roberta", functools.partial(torch.optim.AdamW, lr=5e-5), False, False,
                             text_embedding_dim=768, embedding_dim=128)


@pytest.mark.gpu
def test_module_training_step_and_adamw(module_and_reference):
    """One fp32 training_step (B = 4, 64 px, T = 12, dropout 0) vs the fp64 composition of
    oracle/resnet34.py, HF DistilBertModel and the reference's projection / normalise /
    logits / symmetric-CE lines, under the envelope rule; then one FusedAdamW step.

    The loss is one scalar, so its measured envelope is a single draw that can land
    near 0 by chance.  Its floor is the spacing of the fp32 logits it is computed from
    (loss = mean(logsumexp(l) - l_ii): both terms carry the logits' rounding, and the
    logits reach a few units): 2^-23 * max|logits| / loss, about 2.6e-7 here."""
    m, hf, batch, (l64, ie64, te64, lg64), (l32, ie32, te32, _) = module_and_reference
    m.train()
    opt = m.configure_optimizers()["optimizer"]
    from vlp_amd.optim import FusedAdamW
    assert isinstance(opt, FusedAdamW)
    loss, _, _, ie, te = m.training_step_outputs(batch)
    env = {"loss": max(abs(l32.item() - l64.item()), FLOOR * lg64.abs().max().item()) / abs(l64.item()),
           "image_emb": max(rel(ie32, ie64), FLOOR), "text_emb": max(rel(te32, te64), FLOOR)}
    got = {"loss": abs(loss.item() - l64.item()) / abs(l64.item()), "image_emb": rel(ie, ie64),
           "text_emb": rel(te, te64)}
    print("module step: " + ", ".join(f"{k} {got[k]:.3e} (envelope {env[k]:.3e})" for k in env))
    for k in env:
        assert got[k] <= 10 * env[k], (k, got[k], env[k])
    tower = m.text_encoder.model
    before = tower.arena.data.clone()
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in m.parameters())
    for owner, attr, full in tower._param_slots:
        p = owner._parameters[attr]
        assert p.data_ptr() == tower.arena.view(full).data_ptr(), full      # still views of the arena
        o, n, shape = tower.arena.layout[full]
        if len(shape) == 2:                                                     # every weight matrix moved
            assert not torch.equal(before[o:o + n], tower.arena.data[o:o + n]), full
