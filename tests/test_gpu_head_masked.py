"""The duplicate-caption mask of the contrastive loss (`vlp_clip_loss_fused_masked`,
`vlp_ce_sym_masked`, VisionLanguageModule(duplicate_caption_mask=True)) on the GPU.

Semantics under test: with one caption id per gathered row, an entry (i, j),
i != j, with cid[i] == cid[j] is left out of both softmaxes as if its logit were
-inf; the diagonal always stays; the losses stay means over all N rows / columns.
The reference is that sentence in torch fp64 (`masked_ref`): masked_fill(-inf),
two cross_entropy calls, autograd.

Tolerances are those tests/test_gpu_head.py applies to the same quantities (fp32
kernels against fp64): losses |delta| <= 1e-5; embedding gradients rtol 1e-4,
atol 1e-6 * max|ref|; d logit_scale rel 1e-4 and exactly 0 when clamped.  Where the
semantics promise an exact zero (a row left with its diagonal alone) the test asks
for an exact zero.
"""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
F = torch.nn.functional
GOLD = os.path.join(os.path.dirname(__file__), "golden")
LS0 = math.log(1 / 0.07)          # the reference's initial logit_scale (:111)
IDS8 = [0, 1, 0, 2, 1, 3, 0, 4]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def embeddings(N, E, seed):
    g = torch.Generator().manual_seed(seed)
    ie = F.normalize(torch.randn(N, E, generator=g, dtype=torch.float64))
    te = F.normalize(torch.randn(N, E, generator=g, dtype=torch.float64))
    return ie.float(), te.float()


def excluded(cid):
    cid = torch.as_tensor(cid)
    return (cid[:, None] == cid[None, :]) & ~torch.eye(len(cid), dtype=torch.bool)


def masked_ref(ie, te, ls, cid, w=(1.0, 1.0), logits=None):
    """fp64: the masked symmetric cross-entropy and its gradients (of
    (w[0] image_loss + w[1] text_loss) / 2) from fp32 embeddings or explicit logits."""
    out = {}
    if logits is None:
        x, y = ie.double().requires_grad_(), te.double().requires_grad_()
        l = torch.tensor([ls], dtype=torch.float64, requires_grad=True)
        lg = torch.clamp(l.exp(), max=100.0) * x @ y.t()
    else:
        lg = logits.double().requires_grad_()
    out["logits"] = lg
    N = lg.shape[0]
    m = lg.masked_fill(excluded(cid), float("-inf"))
    lab = torch.arange(N)
    rows, cols = F.cross_entropy(m, lab, reduction="none"), F.cross_entropy(m.t(), lab, reduction="none")
    li, lt = rows.mean(), cols.mean()
    ((w[0] * li + w[1] * lt) / 2).backward()
    out.update(image_loss=li.item(), text_loss=lt.item(), loss=((li + lt) / 2).item(),
               rows=rows.detach(), cols=cols.detach())
    if logits is None:
        out.update(d_img=x.grad, d_txt=y.grad, d_ls=l.grad.item())
    else:
        out["d_logits"] = lg.grad
    return out


def run_fused(B, N, E, off, ie, te, ls, cid=None, role_w=None):
    """One rank's launch (rows / columns off .. off + B of the N x N matrix); every
    output is pre-filled with NaN, so an unwritten element cannot pass."""
    from vlp_amd import ops
    dev = torch.device("cuda")
    nan = float("nan")
    gi, gt = torch.full((N, E), nan, device=dev), torch.full((N, E), nan, device=dev)
    small = torch.full((4,), nan, device=dev)
    lse = torch.full((2, B), nan, device=dev)
    ied, ted = ie.to(dev).contiguous(), te.to(dev).contiguous()
    lsd = torch.tensor([ls], dtype=torch.float32, device=dev)
    rw = None if role_w is None else torch.tensor(role_w, dtype=torch.float32, device=dev)
    if cid is None:
        ops.clip_loss_fused(B, N, E, off, ied, ted, lsd, gi, gt, small[2:3], small[0:2], lse_out=lse, role_w=rw)
    else:
        c = torch.as_tensor(cid, dtype=torch.int32).to(dev)
        ops.clip_loss_fused_masked(B, N, E, off, ied, ted, lsd, c, gi, gt, small[2:3], small[0:2], lse_out=lse,
                                   role_w=rw)
    torch.cuda.synchronize()
    return {"d_img": gi.cpu(), "d_txt": gt.cpu(), "parts": small[0:2].cpu(), "d_ls": small[2].item(),
            "lse": lse.cpu()}


def run_ranks(Bs, N, E, ie, te, ls, cid, role_w=None):
    """Consecutive ranks of Bs rows each; sums as the step's collectives form them."""
    tot = {"d_img": torch.zeros(N, E, dtype=torch.float64), "d_txt": torch.zeros(N, E, dtype=torch.float64),
           "parts": torch.zeros(2, dtype=torch.float64), "d_ls": 0.0, "per_rank": []}
    off = 0
    for B in Bs:
        r = run_fused(B, N, E, off, ie, te, ls, cid, role_w)
        for k in ("d_img", "d_txt", "parts", "lse"):
            assert torch.isfinite(r[k]).all(), (k, off)
        tot["d_img"] += r["d_img"].double()
        tot["d_txt"] += r["d_txt"].double()
        tot["parts"] += r["parts"].double()
        tot["d_ls"] += r["d_ls"]
        tot["per_rank"].append((off, B, r))
        off += B
    assert off == N
    return tot


def close(got, want, what):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    atol = 1e-6 * max(want.abs().max().item(), 1e-30)
    torch.testing.assert_close(got, want, rtol=1e-4, atol=atol, msg=lambda m: f"{what}: {m}")


def check_against_ref(tot, ref, N, clamped=False):
    print(f"loss {(tot['parts'].sum() / (2 * N)).item():.7f} ref {ref['loss']:.7f}  d_ls {tot['d_ls']:.6e} "
          f"ref {ref['d_ls']:.6e}")
    assert abs(tot["parts"][0].item() / N - ref["image_loss"]) <= 1e-5
    assert abs(tot["parts"][1].item() / N - ref["text_loss"]) <= 1e-5
    assert abs(tot["parts"].sum().item() / (2 * N) - ref["loss"]) <= 1e-5
    for off, B, r in tot["per_rank"]:       # each rank's own partial sums and log-sum-exps
        assert abs(r["parts"][0].item() - ref["rows"][off:off + B].sum().item()) <= 1e-5 * B
        assert abs(r["parts"][1].item() - ref["cols"][off:off + B].sum().item()) <= 1e-5 * B
    close(tot["d_img"], ref["d_img"], "d img emb")
    close(tot["d_txt"], ref["d_txt"], "d txt emb")
    if clamped:
        assert ref["d_ls"] == 0.0 and tot["d_ls"] == 0.0, tot["d_ls"]
    else:
        assert abs(tot["d_ls"] - ref["d_ls"]) <= 1e-4 * abs(ref["d_ls"]), (tot["d_ls"], ref["d_ls"])


# ---- 1. all ids distinct: the masked entry point is the unmasked one, bit for bit
@pytest.mark.parametrize("B,N,off,E", [(8, 8, 0, 128), (8, 8, 0, 32), (4, 16, 4, 128), (4, 16, 4, 32),
                                       (256, 2048, 512, 128)])
def test_distinct_ids_bitwise_equal_unmasked(B, N, off, E):
    ie, te = embeddings(N, E, 11)
    a = run_fused(B, N, E, off, ie, te, LS0)
    b = run_fused(B, N, E, off, ie, te, LS0, cid=torch.arange(N))
    for k in ("d_img", "d_txt", "parts", "lse"):
        assert not torch.isnan(a[k]).any() and torch.equal(a[k], b[k]), k
    assert a["d_ls"] == b["d_ls"]


# ---- 2. masked parity against fp64
def straddle_ids():
    """N = 16 over 4 ranks of 4: id 0 on ranks 0, 1, 2 (rows 0, 4, 10), id 1 on ranks 0 and 1
    (rows 1, 7), id 3 on ranks 0 and 3 (rows 3, 13)."""
    return [0, 1, 2, 3, 0, 4, 5, 1, 6, 7, 0, 8, 9, 3, 10, 11]


def slab_ids(N, lo, hi):
    """Distinct ids, except that keys lo .. hi - 1 share row 0's id."""
    cid = torch.arange(N) + 100
    cid[0] = 7
    cid[lo:hi] = 7
    return cid


@pytest.mark.parametrize("E", [32, 128])
@pytest.mark.parametrize("case", ["B8", "B4_N16_ranks", "B40_N72_slab", "B48_N144_tile", "B8_clamped"])
def test_masked_vs_fp64(case, E):
    ls = LS0
    if case == "B8":
        Bs, cid = [8], IDS8
    elif case == "B4_N16_ranks":
        Bs, cid = [4, 4, 4, 4], straddle_ids()
    elif case == "B40_N72_slab":
        # row 0 against keys 32..63: one whole staged 32-key slab dropped; rows see full
        # slabs and the partial last one (keys 64..71); second rank: the remaining 32 rows
        Bs, cid = [40, 32], slab_ids(72, 32, 64)
    elif case == "B48_N144_tile":
        # row 0 against keys 64..127: one whole 64-key tile dropped, the split-key fold
        # meets the neutral partial (-inf, 0) between two live ones
        Bs, cid = [48, 48, 48], slab_ids(144, 64, 128)
    else:
        Bs, cid, ls = [8], IDS8, math.log(150.0)     # exp > 100: clamped, no d logit_scale
    N = sum(Bs)
    ie, te = embeddings(N, E, 3 + E)
    ref = masked_ref(ie, te, ls, cid)
    tot = run_ranks(Bs, N, E, ie, te, ls, cid)
    check_against_ref(tot, ref, N, clamped=case == "B8_clamped")


def test_excluded_pairs_get_exact_zeros():
    """E = 4, two rows that are each other's only off-diagonal partner, with one id:
    both softmaxes keep the diagonal alone, whose loss and gradient are exactly 0."""
    ie, te = embeddings(2, 4, 5)
    r = run_fused(2, 2, 4, 0, ie, te, LS0, cid=[3, 3])
    assert torch.equal(r["d_img"], torch.zeros(2, 4)) and torch.equal(r["d_txt"], torch.zeros(2, 4))
    assert torch.equal(r["parts"], torch.zeros(2)) and r["d_ls"] == 0.0
    # the same pair inside a larger batch (rows 1 and 2 of N = 4): ordinary rows again
    ie, te = embeddings(4, 4, 6)
    cid = [0, 1, 1, 2]
    a = run_fused(4, 4, 4, 0, ie, te, LS0, cid=cid)
    ref = masked_ref(ie, te, LS0, cid)
    close(a["d_img"], ref["d_img"], "d img emb")
    close(a["d_txt"], ref["d_txt"], "d txt emb")
    assert a["d_ls"] != 0.0


# ---- 3. every caption equal: nothing but diagonals
def test_all_captions_equal_is_exactly_zero():
    for E in (32, 128):
        ie, te = embeddings(8, E, 9)
        r = run_fused(8, 8, E, 0, ie, te, LS0, cid=[5] * 8)
        for k in ("d_img", "d_txt", "parts", "lse"):
            assert torch.isfinite(r[k]).all(), k
        assert torch.equal(r["d_img"], torch.zeros(8, E)) and torch.equal(r["d_txt"], torch.zeros(8, E))
        assert torch.equal(r["parts"], torch.zeros(2))        # image and text loss, hence the loss
        assert r["d_ls"] == 0.0


# ---- 4. per-direction gradients
@pytest.mark.parametrize("w", [(1.0, 0.0), (0.0, 1.0)])
def test_role_weights_under_mask(w):
    E = 128
    ie, te = embeddings(8, E, 13)
    ref = masked_ref(ie, te, LS0, IDS8, w=(2 * w[0], 2 * w[1]))     # (2 image_loss) / 2 = image_loss
    r = run_fused(8, 8, E, 0, ie, te, LS0, cid=IDS8, role_w=(2 * w[0], 2 * w[1]))
    close(r["d_img"], ref["d_img"], "d img emb")
    close(r["d_txt"], ref["d_txt"], "d txt emb")
    assert abs(r["d_ls"] - ref["d_ls"]) <= 1e-4 * abs(ref["d_ls"]), (r["d_ls"], ref["d_ls"])


# ---- 5. explicit logits
def test_ce_sym_masked_vs_fp64_and_fused():
    from vlp_amd import ops
    E = 128
    ie, te = embeddings(8, E, 17)
    s = min(math.exp(LS0), 100.0)
    logits = (s * ie.double() @ te.double().t()).float()
    ref = masked_ref(None, None, None, IDS8, logits=logits)
    dev = torch.device("cuda")
    out = torch.zeros(3, device=dev)
    dl = torch.zeros(8, 8, device=dev)
    ops.ce_sym_masked(logits.to(dev).contiguous(), torch.tensor(IDS8, dtype=torch.int32, device=dev), out, dl)
    torch.cuda.synchronize()
    for k, v in zip(("loss", "image_loss", "text_loss"), out.tolist()):
        assert abs(v - ref[k]) <= 1e-5, (k, v, ref[k])
    close(dl, ref["d_logits"], "d logits")
    assert torch.equal(dl.cpu()[excluded(IDS8)], torch.zeros(int(excluded(IDS8).sum())))
    fused = run_fused(8, 8, E, 0, ie, te, LS0, cid=IDS8)
    assert abs(fused["parts"].sum().item() / 16 - out[0].item()) <= 1e-5


# ---- 6. the module
def make_module(**kw):
    from oracle import weights as W
    from src.models.pretrain.VisionLanguageModule import VisionLanguageModule
    m = VisionLanguageModule("resnet34", "tinybert", functools.partial(torch.optim.AdamW, lr=5e-5),
                             False, False, 512, 312, 128, compute_dtype="fp32", text_dropout=0.0, **kw)
    W.apply_recipe(m, 0)
    m.train()
    return m


def test_module_step_masked_and_default():
    from tests.golden.synth import synth_batch
    gd = torch.load(os.path.join(GOLD, "step_B4_H64_T12.pt"), weights_only=True)
    batch = synth_batch(4, 64, 12, 0)
    batch["caption"] = ["a", "b", "a", "c"]
    # flag off: the golden's loss, at the gate of tests/test_gpu_model.py
    m = make_module()
    loss = m.training_step(batch)
    assert abs(loss.item() - gd["train_loss"].item()) < 1e-3, (loss.item(), gd["train_loss"].item())
    del m
    m = make_module(duplicate_caption_mask=True)
    assert m.hparams["duplicate_caption_mask"] is True
    step = m.training_step(batch).item()
    logits, _, _ = m(batch)
    api = m._compute_loss(logits, False, False, batch["caption"], m._caption_keys(batch))[0].item()
    ref = masked_ref(None, None, None, [0, 1, 0, 2], logits=logits.detach().cpu())["loss"]
    plain = masked_ref(None, None, None, [0, 1, 2, 3], logits=logits.detach().cpu())["loss"]
    print(f"masked step {step:.7f} api {api:.7f} fp64 {ref:.7f} (unmasked fp64 {plain:.7f})")
    assert abs(step - api) <= 1e-5 and abs(step - ref) <= 1e-5 and abs(api - ref) <= 1e-5
    assert abs(ref - plain) > 1e-4       # the mask moved this batch's loss: the comparison can tell
    # a datamodule's caption_id tensor takes the strings' place
    batch2 = dict(batch, caption=["p", "q", "r", "s"], caption_id=torch.tensor([40, 7, 40, 9]))
    assert abs(m.training_step(batch2).item() - ref) <= 1e-5


# ---- 7. world size 2 (gloo, both ranks on this GPU)
def test_world2_gloo_masked(tmp_path):
    B, E = 4, 32
    captions = ["k%d" % i for i in (0, 1, 2, 3, 4, 2, 5, 0)]      # "k2", "k0" cross the ranks
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1",
           "--nnodes=1", "--nproc-per-node", "2", os.path.join(ROOT, "tests", "_masked_dp_worker.py"),
           str(tmp_path), str(B), str(E), ",".join(captions)]
    r = subprocess.run(cmd, env=dict(os.environ, OMP_NUM_THREADS="4"), timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    from vlp_amd.clip_model import caption_hash64, compact_caption_ids
    ie, te = embeddings(2 * B, E, 21)
    want_ids = compact_caption_ids(caption_hash64(captions))
    assert torch.equal(excluded(want_ids), excluded([0, 1, 2, 3, 4, 2, 5, 0]))
    one = run_fused(2 * B, 2 * B, E, 0, ie, te, LS0, cid=want_ids)      # the single-process N = 8 run
    loss1 = one["parts"].sum().item() / (4 * B)
    for k in range(2):
        res = torch.load(tmp_path / f"r{k}.pt", weights_only=True)
        assert torch.equal(res["cid_all"], want_ids), res["cid_all"]      # rank order, same ids
        assert abs(res["loss"] - loss1) <= 1e-5, (res["loss"], loss1)
        close(res["g_img"], one["d_img"][k * B:(k + 1) * B], f"rank {k} d img emb")
        close(res["g_txt"], one["d_txt"][k * B:(k + 1) * B], f"rank {k} d txt emb")
