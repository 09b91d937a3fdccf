"""GPU: the t-SNE kernels (vlp_tsne_sqdist / _affinities / _pairs / _update), the device path of
vlp_amd.metrics.tsne and the post-fit evaluation's embedding, against scikit-learn.

Gates as in tests/test_tsne_cpu.py (references in tests/tsne_ref.py; no limit comes from the
kernels' own results), with what the device adds:

  * row entropy: the kernel returns the conditional matrix in fp32, so a row's fp64 entropy may be
    off by what that storage adds.  The slack is measured in the test on sklearn's own fp64
    conditional rounded to fp32 (largest change of a row's entropy: 3.2e-11 at N = 20, 2.3e-8 at
    N = 257, 3.7e-8 at N = 300) and added to sklearn's 1e-5.
  * one iteration: the gradient's relative L2 error and the KL's absolute error against
    _kl_divergence in fp64 are at most twice the error of the fp32 CPU restatement
    (metrics.tsne_grad_cpu) on the same inputs, and never asked below the floor 32 * 2^-24 =
    1.9e-6 derived in tests/test_tsne_cpu.py (restatement, measured: gradient 2.3e-7 .. 5.4e-7,
    KL 5.5e-8 .. 1.5e-7; kernels, measured on an MI355X: gradient 1.8e-8 .. 6.9e-8, KL 1.2e-9 .. 1.7e-8).
  * the step: from row partials that make the gradient an exact fp32 array, Y, update and gains
    equal numpy's fp32 _gradient_descent arithmetic bit for bit.
  * end to end, the full 1000 iterations: KL at most the worst of sklearn's five seeds plus their
    spread, trustworthiness at least the worst minus the spread (tests/golden/tsne_sklearn.json),
    two runs torch.equal.
"""
import glob
import os

import numpy as np
import pytest
import torch

from tests import tsne_ref as R
from tests.test_tsne_cpu import AFFINITY_CASES, GRAD_FLOOR, KL_FLOOR, U, step_case

pytestmark = pytest.mark.gpu

SIZE = ["data.batch_size=4", "data.image_size=64", "data.n_samples=12", "data.n_val_samples=4",
        "data.num_workers=0", "trainer.max_epochs=2", "model.compute_dtype=fp32"]
EVAL = "baseline_only_imaging/baseline_only_imaging_resnet_34_mi355x_eval"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vlp_amd import ops as o
    return o


@pytest.fixture(scope="module")
def M():
    from vlp_amd import metrics
    return metrics


# (70, 37): one tile with a column tail; (257, 32): one row past four tiles; (130, 1027): D tail over many chunks
@pytest.mark.parametrize("N,D", [(70, 37), (257, 32), (130, 1027)])
def test_sqdist_vs_fp64(ops, N, D):
    x, _ = R.blobs(N, D, seed=5, dup=3)
    got = ops.tsne_sqdist(torch.from_numpy(x).cuda()).cpu().numpy()
    ref = R.sqdist_f32(x).astype(np.float64)
    err = np.abs(got - ref).max() / ref.max()
    print(f"N={N} D={D}: max err {err:.3e} of the largest distance (limit {2 * (D + 2) * U:.3e})")
    assert (got.diagonal() == 0).all() and np.array_equal(got, got.T) and (got[:3, N - 3:].diagonal() == 0).all()
    assert err <= 2 * (D + 2) * U


@pytest.mark.parametrize("N,perplexity,dup", AFFINITY_CASES)
def test_affinities_vs_sklearn(ops, N, perplexity, dup):
    x, _ = R.blobs(N, 32, seed=3, dup=dup)
    d2 = R.sqdist_f32(x)
    Pd, cond = ops.tsne_affinities(torch.from_numpy(d2).cuda(), perplexity, return_conditional=True)
    P, cond = Pd.cpu().numpy(), cond.cpu().numpy()
    csk = R.sk_conditional(d2, perplexity)
    slack = np.abs(R.row_entropy(csk.astype(np.float32)) - R.row_entropy(csk)).max()
    dev = np.abs(R.row_entropy(cond) - np.log(perplexity)).max()
    tv = R.total_variation(P, R.sk_joint(d2, perplexity))
    tv_np = R.total_variation(R.np_joint(R.np_conditional(d2, perplexity)), R.sk_joint(d2, perplexity))
    print(f"N={N}: entropy off by {dev:.4e} (fp32 storage slack {slack:.3e}); TV {tv:.3e} "
          f"(numpy restatement {tv_np:.3e})")
    assert cond.dtype == np.float32 and (cond.diagonal() == 0).all()
    assert dev <= 1e-5 + slack
    assert tv <= max(4 * tv_np, 1e-6)
    assert P.dtype == np.float32 and np.array_equal(P, P.T) and (P.diagonal() == 0).all()
    assert (P[~np.eye(N, dtype=bool)] > 0).all()
    again = ops.tsne_affinities(torch.from_numpy(d2).cuda(), perplexity)
    assert torch.equal(again, Pd)


def _device_iteration(ops, y, P32, exag):
    """(KL, gradient fp64 [N, 2]) of one device iteration from y: the gradient recovered from the
    step the update kernel takes from zero update and unit gains (gain 0.8, update = -lr 0.8 g)."""
    N = y.shape[0]
    yd = torch.from_numpy(y).cuda()
    parts = torch.full((N, ops.TSNE_PARTS), float("nan"), dtype=torch.float64, device="cuda")
    ops.tsne_pairs(yd, P32, parts, True)
    plain = torch.full_like(parts, float("nan"))
    ops.tsne_pairs(yd, P32, plain, False)
    assert torch.equal(plain[:, :5], parts[:, :5]) and (plain[:, 5:] == 0).all()
    p = parts.cpu().numpy()
    grad = 4.0 * (exag * p[:, 1:3] - p[:, 3:5] / p[:, 0].sum())
    upd, gains = torch.zeros_like(yd), torch.ones_like(yd)
    stats = torch.zeros(2, dtype=torch.float64, device="cuda")
    ops.tsne_update(parts, yd, upd, gains, exag, 0.5, 1.0, True, stats)
    kl, gnorm = stats.tolist()
    # Z is summed in the kernel's order there and in numpy's here: a last-bit fp64 difference may
    # move the fp32 cast of a gradient entry by one ulp
    want = -(grad.astype(np.float32) * np.float32(0.8))
    assert (np.abs(upd.cpu().numpy() - want) <= 2.0 ** -22 * np.abs(want)).all() and (gains == 0.8).all()
    assert abs(gnorm - np.linalg.norm(want.astype(np.float64))) <= 1e-6 * gnorm
    return kl, grad


@pytest.mark.parametrize("N", [300, 1030])
@pytest.mark.parametrize("scale", [1e-4, 10.0])
def test_one_iteration_vs_sklearn(ops, M, N, scale):
    x, _ = R.blobs(N, 32, seed=2)
    P = R.sk_joint(R.sqdist_f32(x), 30.0)
    P32 = torch.from_numpy(P).float()
    y = R.fixed_y(N, scale)
    for exag in (1.0, 12.0):
        kl64, g64 = R.sk_kl_grad(y, P, exag)
        kl_c, g_c = M.tsne_grad_cpu(torch.from_numpy(y), P32, exag)
        gerr_c = np.linalg.norm(g_c.numpy().astype(np.float64) - g64) / np.linalg.norm(g64)
        kl, g = _device_iteration(ops, y, P32.cuda(), exag)
        gerr = np.linalg.norm(g - g64) / np.linalg.norm(g64)
        print(f"N={N} scale={scale} exag={exag}: grad rel L2 {gerr:.3e} (fp32 restatement {gerr_c:.3e}), "
              f"KL err {abs(kl - kl64):.3e} (restatement {abs(kl_c - kl64):.3e})")
        assert gerr <= max(2 * gerr_c, GRAD_FLOOR)
        assert abs(kl - kl64) <= max(2 * abs(kl_c - kl64), KL_FLOOR)


@pytest.mark.parametrize("momentum,lr", [(0.5, 50.0), (0.8, 85.33333333333333)])
def test_step_equals_numpy(ops, momentum, lr):
    grad, update, gains = step_case(1100)   # more rows than the workgroup has threads
    N = grad.shape[0]
    y = R.fixed_y(N, 3.0)
    gg, u_ref, g_ref = R.np_update(grad, update, gains, momentum, lr)
    parts = np.zeros((N, 7))
    parts[:, 0] = 1.0                    # Z = N exactly
    parts[:, 1:3] = grad / 4.0           # exag 1, no repulsion: the gradient is `grad` exactly
    parts[:, 5], parts[:, 6] = 0.25, 1.0 / N
    dev = [torch.from_numpy(a.copy()).cuda() for a in (y, update, gains)]
    stats = torch.zeros(2, dtype=torch.float64, device="cuda")
    ops.tsne_update(torch.from_numpy(parts).cuda(), *dev, 1.0, momentum, lr, True, stats)
    yd, ud, gd = (t.cpu().numpy() for t in dev)
    assert np.array_equal(gd, g_ref) and np.array_equal(ud, u_ref) and np.array_equal(yd, y + u_ref)
    assert (gd[4:8] == np.float32(0.01)).all()
    kl, gnorm = stats.tolist()
    assert abs(kl - (0.25 * N + np.log(N))) <= 1e-12 * N
    assert abs(gnorm - np.linalg.norm(gg.astype(np.float64))) <= 1e-12 * gnorm
    # check = 0 leaves the statistics alone and takes the same step
    dev2 = [torch.from_numpy(a.copy()).cuda() for a in (y, update, gains)]
    stats2 = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
    ops.tsne_update(torch.from_numpy(parts).cuda(), *dev2, 1.0, momentum, lr, False, stats2)
    assert all(torch.equal(a, b) for a, b in zip(dev, dev2)) and (stats2 == -1).all()


def test_end_to_end_1000_iterations(M):
    from sklearn.manifold import trustworthiness
    x, _ = R.blobs()
    P = R.sk_joint(R.sqdist_f32(x), R.PERPLEXITY_E2E)
    golden = R.load_golden()
    assert golden["data_sum"] == float(x.astype(np.float64).sum())
    kl_max, trust_min = R.e2e_gates(golden, 1000)
    xd = torch.from_numpy(x).cuda()
    y, kl_own = M.tsne(xd, R.PERPLEXITY_E2E)
    y2, kl2 = M.tsne(xd, R.PERPLEXITY_E2E)
    assert y.is_cuda and y.shape == (300, 2) and y.dtype == torch.float32 and torch.isfinite(y).all()
    kl = R.sk_kl_grad(y.cpu().numpy(), P)[0]
    trust = trustworthiness(x, y.cpu().numpy(), n_neighbors=5)
    print(f"KL {kl:.4f} (own {kl_own:.4f}, gate <= {kl_max:.4f}); trustworthiness {trust:.4f} (gate >= {trust_min:.4f})")
    assert abs(kl_own - kl) <= 1e-2   # the returned KL is taken before the last step
    assert kl <= kl_max and trust >= trust_min
    assert torch.equal(y, y2) and kl_own == kl2


def test_errors_on_device(M, ops):
    from vlp_amd._lib import HipError
    x = torch.zeros(10, 4, device="cuda")
    with pytest.raises(ValueError, match="perplexity"):
        M.tsne(x, perplexity=10.0)
    with pytest.raises(ValueError, match="4 GB"):
        M.tsne(torch.zeros(32769, 1, device="cuda"), perplexity=30.0)
    with pytest.raises(HipError):   # refused by the C entry before any launch
        ops.tsne_affinities(torch.zeros(10, 10, device="cuda"), 10.0)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from src import train as T
    from src.utils.config import compose
    out = {}
    for name, experiment in (("tsne", EVAL + "_tsne"), ("plain", EVAL)):
        d = tmp_path_factory.mktemp(name)
        metrics, _ = T.train(compose("train", [f"experiment={experiment}", f"paths.output_dir={d}"] + SIZE))
        out[name] = (metrics, str(d))
    return out


def test_train_writes_the_embedding(runs):
    metrics, d = runs["tsne"]
    plain, _ = runs["plain"]
    extra = set(metrics) - set(plain)   # train() reports every fold metric with its `_std` over the folds
    assert extra == {k + s for k in ("tsne_kl_validation", "tsne_kl_train") for s in ("", "_std")}
    assert set(plain) <= set(metrics)
    for split, n in (("validation", 8), ("train", 12)):
        assert np.isfinite(metrics[f"tsne_kl_{split}"])
        files = glob.glob(os.path.join(d, "**", f"tsne_{split}.npz"), recursive=True)
        assert len(files) == 1
        z = np.load(files[0])
        assert z["y"].shape == (n, 2) and np.isfinite(z["y"]).all() and len(z["tumor"]) == len(z["dataset"]) == n
        assert set(z["dataset"].tolist()) == {"INTERNAL", "BTXRD"}
        pytest.importorskip("matplotlib")
        assert os.path.exists(files[0][:-4] + ".png")


def test_train_without_the_key_is_unchanged(runs):
    plain, d = runs["plain"]
    assert not any("tsne" in k for k in plain)
    assert glob.glob(os.path.join(d, "**", "tsne_*"), recursive=True) == []
