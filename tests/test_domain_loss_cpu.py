"""CPU: the closed form of the on-device weighted BCE + CORAL loss (tests/domain_loss_ref.py, what
csrc/domain_loss_ops.hip computes) against the reference-made goldens of tests/golden/fusion_loss.pt
at the tolerances tests/test_fusion.py holds the torch path to, and against autograd in fp64; the
host pieces of the feature (domain_codes, the C ABI's two entry points, the module flag, the two
experiments).  The GPU side is tests/test_gpu_domain_loss.py."""
import functools
import os
import subprocess

import pytest
import torch

from tests.conftest import PKG, ROOT
from tests.domain_loss_ref import codes_of, domain_loss_ref

GOLD = torch.load(os.path.join(os.path.dirname(__file__), "golden", "fusion_loss.pt"), weights_only=True)
LIB = os.path.join(PKG, "vlp_amd", "libvlp_hip.so")
HDR = os.path.join(ROOT, "include", "vlp_hip.h")
ENTRY_POINTS = ("vlp_domain_loss_ws_bytes", "vlp_domain_loss")


def coral_case(c):
    """A coral_* golden as the op's inputs: the source rows, then the target rows, lambda 1."""
    ns, nt = c["source"].shape[0], c["target"].shape[0]
    feat = torch.cat([c["source"], c["target"]])
    codes = torch.tensor([0] * ns + [1] * nt, dtype=torch.uint8)
    return feat, torch.zeros(ns + nt), torch.zeros(ns + nt, dtype=torch.int64), codes, ns


@pytest.mark.parametrize("name", [k for k in GOLD if k.startswith("coral_")])
def test_closed_form_vs_reference_coral_golden(name):
    c = GOLD[name]
    feat, logits, labels, codes, ns = coral_case(c)
    r = domain_loss_ref(feat, logits, labels, codes, 1.0, 1.0, 1.0)
    assert torch.allclose(r["coral"].float(), c["loss"], rtol=1e-5, atol=1e-7), (r["coral"].item(), c["loss"].item())
    assert torch.allclose(r["cls"], torch.log(torch.tensor(2.0, dtype=torch.float64)), rtol=1e-15)
    if "grad_source" in c:
        assert torch.allclose(r["g_feat"][:ns].float(), c["grad_source"], rtol=1e-4, atol=1e-8)
        assert torch.allclose(r["g_feat"][ns:].float(), c["grad_target"], rtol=1e-4, atol=1e-8)


def test_closed_form_vs_reference_compute_loss_golden():
    cases = GOLD["compute_loss"]
    assert len(cases) == 4
    dead = 0
    for case in cases:
        lw = case["label_weights"]
        r = domain_loss_ref(case["features"], case["logits"], case["labels"], codes_of(case["dataset"]),
                            float(lw[0]), float(lw[1]), float(case["coral_lambda"]))
        assert abs(r["total"].item() - case["loss"].item()) < 1e-6
        assert abs(r["cls"].item() - case["classification_loss"].item()) < 1e-6
        assert abs(r["coral"].item() - case["coral_loss"].item()) < 1e-6
        assert torch.allclose(r["g_logits"].float(), case["grad_logits"], rtol=1e-5, atol=1e-8)
        assert torch.allclose(r["g_feat"].float(), case["grad_features"], rtol=1e-4, atol=1e-9)
        if case["dataset"].count("INTERNAL") <= 1 and float(case["coral_lambda"]) != 0.0:
            dead += 1
            assert r["coral"].item() == 0.0 and not r["g_feat"].any()
    assert dead == 1      # the 1-vs-5 split: CORAL exactly 0 (FusionModule.py:375-376)


@pytest.mark.parametrize("ns,nt,D", [(2, 2, 8), (5, 3, 16), (7, 9, 33)])
def test_closed_form_gradients_vs_autograd_fp64(ns, nt, D):
    """The written-out gradients against autograd through the package's torch path in fp64, with
    rows of neither domain mixed in and both label weights live."""
    from src.utils.coral_loss.coral import coral
    g = torch.Generator().manual_seed(ns * 100 + nt)
    N = ns + nt + 2
    codes = torch.tensor([0] * ns + [2] + [1] * nt + [2], dtype=torch.uint8)[torch.randperm(N, generator=g)]
    x = torch.randn(N, D, generator=g, dtype=torch.float64).requires_grad_()
    z = torch.randn(N, generator=g, dtype=torch.float64).mul(3).requires_grad_()
    y = torch.randint(0, 2, (N,), generator=g)
    lam, w0, w1 = 0.5, 0.7, 2.0
    u = torch.where(y == 0, torch.tensor(w0, dtype=torch.float64), torch.tensor(w1, dtype=torch.float64))
    cls = torch.nn.functional.binary_cross_entropy_with_logits(z, y.double(), weight=u)
    cor = lam * coral(x[codes == 0], x[codes == 1])
    gx, gz = torch.autograd.grad(cls + cor, (x, z))
    r = domain_loss_ref(x, z, y, codes, w0, w1, lam)
    assert abs(r["cls"].item() - cls.item()) <= 1e-15 * abs(cls.item()) * 8
    assert abs(r["coral"].item() - cor.item()) <= 1e-13 * abs(cor.item())
    assert (r["g_feat"] - gx).abs().max().item() <= 1e-13 * gx.abs().max().item()
    assert (r["g_logits"] - gz).abs().max().item() <= 1e-15
    assert not r["g_feat"][codes == 2].any() and r["g_logits"][codes == 2].abs().min() > 0


def test_domain_codes():
    from vlp_amd.domain_loss import domain_codes
    c = domain_codes(["INTERNAL", "BTXRD", "internal", "", "BTXRD", "MURA", "INTERNAL"])
    assert c.dtype == torch.uint8 and c.device.type == "cpu"
    assert c.tolist() == [0, 1, 2, 2, 1, 2, 0]
    assert domain_codes([]).shape == (0,)
    assert torch.equal(domain_codes(["BTXRD", "x"]), codes_of(["BTXRD", "x"]))


def test_header_declares_and_library_exports_the_entry_points():
    from vlp_amd import _lib
    protos = _lib.parse_header(HDR)
    for name in ENTRY_POINTS:
        assert name in protos, name
    args = [a for _, a in protos["vlp_domain_loss"]["args"]]
    assert args == ["N", "D", "feat", "ldf", "logits", "label", "label_kind", "domain", "w0", "w1", "coral_lambda",
                    "out", "g_feat", "g_logits", "ws", "ws_bytes", "stream"]
    if not os.path.exists(LIB):
        pytest.skip("libvlp_hip.so not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in ENTRY_POINTS:
        assert name in exported, name
    L = _lib.lib()
    assert L._dll.vlp_abi_version() == 3          # additive: the ABI version stays
    # the workspace query is pure host code: sizes grow with N and D, bad sizes are refused
    from vlp_amd import ops
    small, big = ops.domain_loss_ws_bytes(64, 512), ops.domain_loss_ws_bytes(4096, 512)
    assert 512 * 512 * 8 <= small < big and ops.domain_loss_ws_bytes(0, 1) > 0
    for N, D in ((-1, 8), (8, 0), (8, 2049), ((1 << 18) + 1, 8)):
        with pytest.raises(_lib.HipError):
            ops.domain_loss_ws_bytes(N, D)


def test_module_flag_defaults_off_and_cpu_tensors_keep_the_torch_path():
    from src.models.baseline.FusionModule import FusionModule
    from src.models.baseline.OnlyImagingModule import OnlyImagingModule
    opt = functools.partial(torch.optim.AdamW, lr=1e-3)
    assert FusionModule("resnet34", opt, device="cpu").hparams.loss_on_device is False
    assert OnlyImagingModule("resnet34", opt, device="cpu").hparams.loss_on_device is False
    case = GOLD["compute_loss"][1]
    outs = []
    for flag in (False, True):      # CPU features: the flag changes nothing, bit for bit
        m = OnlyImagingModule("resnet34", opt, device="cpu", label_weights=tuple(case["label_weights"].tolist()),
                              coral_lambda=float(case["coral_lambda"]), loss_on_device=flag)
        assert m.hparams.loss_on_device is flag
        outs.append(m._compute_loss(case["features"], case["logits"], case["labels"], case["dataset"]))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert outs[0][2].item() > 0.0


@pytest.mark.parametrize("experiment,target", [
    ("baseline_only_imaging/baseline_only_imaging_resnet_34_mi355x_coral",
     "src.models.baseline.OnlyImagingModule.OnlyImagingModule"),
    ("baseline_imaging_and_clinical/baseline_imaging_and_clinical_resnet_34_mi355x_coral",
     "src.models.baseline.FusionModule.FusionModule")])
def test_coral_experiments_compose(experiment, target):
    from src.utils.config import compose, instantiate
    c = compose("train", [f"experiment={experiment}"])
    assert c["model"]["_target_"] == target and c["model"]["model"] == "resnet34"
    assert c["model"]["loss_on_device"] is True and c["model"]["metrics_on_device"] is True
    assert c["model"]["coral_lambda"] == 1000
    assert c["data"]["batch_size"] == 64 and c["optimizer"]["lr"] == 0.00012925748253710286
    assert "AdamW" in c["optimizer"]["_target_"]
    warm = compose("train", ["scheduler=cosine_with_warmup", "trainer.max_epochs=300"])["scheduler"]
    assert c["scheduler"] == warm and c["scheduler"]["num_training_steps"] == 300
    m = instantiate(c["model"], device="cpu")
    assert m.hparams.loss_on_device is True and m.hparams.coral_lambda == 1000
