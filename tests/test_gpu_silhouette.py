"""GPU: vlp_cluster_dist_sums, the device silhouette and the baselines' post-fit
evaluation (reference src/train.py:179-183 and :261-327,
plot_tsne_and_calculate_silhouette.py:15-98, plot_confusion_matrix.py:14-60).

Tolerance (derived, not tuned; full derivation in tests/silhouette_ref.py).  The
kernel computes each distance as sqrtf(sum_d (a_d - b_d)^2) in fp32, u = 2^-24:
a difference is within u, its square within 2u plus the product's rounding; the
squares are non-negative, so their sum over D columns in any order is within
(D + 2) u to first order; the root halves that and rounds once, (D / 2 + 2) u <=
(D + 3) u; the distances are non-negative, so summing up to N of them in any order
adds at most N u.  One `sums` entry is therefore within (D + N + 3) u of fp64
arithmetic on the same fp32 inputs; rtol = 2 (D + N + 3) 2^-24, the factor 2
covering the higher-order terms.  A silhouette value (b - a) / max(a, b): the
cancellation in b - a gives atol = 4 rtol.
"""
import numpy as np
import pytest
import torch

from tests.silhouette_ref import cluster_sums_fp64, silhouette_atol, silhouette_samples_fp64, sums_rtol

pytestmark = pytest.mark.gpu

EVAL_KEYS = ([f"silhouette_score_based_on_{w}_{s}" for w in ("tumor", "dataset") for s in ("validation", "train")]
             + [f"confusion_matrix_{s}/{k}" for s in ("validation", "train") for k in ("tn", "fp", "fn", "tp")])


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from vlp_amd import ops as o
    return o


def _normal(N, D, seed):
    return torch.from_numpy(np.random.default_rng(seed).normal(size=(N, D)).astype(np.float32))


def _check_sums(got, ref, N, D, what):
    rtol = sums_rtol(N, D)
    rel = np.abs(got - ref) / ref
    print(f"{what}: max rel err {rel.max():.3e} (rtol {rtol:.3e})")
    assert got.shape == ref.shape and (ref > 0).all()
    assert (np.abs(got - ref) <= rtol * ref).all()


# (37, 10, 3): one partial tile everywhere; (300, 512, 2): several query blocks and key tiles, 16 full
# column chunks; (257, 384, 8): every cluster, one row past two key tiles; (64, 1027, 2): the column tail
@pytest.mark.parametrize("N,D,C", [(37, 10, 3), (300, 512, 2), (257, 384, 8), (64, 1027, 2)])
def test_cluster_dist_sums_vs_fp64(ops, N, D, C):
    x = _normal(N, D, N + D)
    ids = np.arange(N) % C
    got = ops.cluster_dist_sums(x.cuda(), torch.from_numpy(ids).int().cuda(), C)
    assert got.dtype == torch.float32 and got.shape == (N, C)
    _check_sums(got.double().cpu().numpy(), cluster_sums_fp64(x.numpy(), ids, C), N, D, f"N={N} D={D} C={C}")


def test_cluster_dist_sums_query_slice(ops):
    """Q != N: the queries are a 50-row slice of the keys (a view with the keys' row stride)."""
    N, D, C = 300, 96, 3
    x = _normal(N, D, 5)
    ids = np.arange(N) % C
    xd = x.cuda()
    got = ops.cluster_dist_sums(xd, torch.from_numpy(ids).int().cuda(), C, xq=xd[120:170])
    assert got.shape == (50, C)
    ref = cluster_sums_fp64(x.numpy(), ids, C, Xq=x.numpy()[120:170])
    _check_sums(got.double().cpu().numpy(), ref, N, D, "xq slice")
    full = ops.cluster_dist_sums(xd, torch.from_numpy(ids).int().cuda(), C)
    assert torch.equal(got, full[120:170])        # the order of a row's sum does not depend on where the row sits


def test_cluster_dist_sums_exact_zeros_and_repeatability(ops):
    N, D, C = 300, 70, 3
    x = _normal(N, D, 9)
    x[200] = x[3]
    ids = (torch.arange(N) % C).int().cuda()
    a = ops.cluster_dist_sums(x.cuda(), ids, C)
    b = ops.cluster_dist_sums(x.cuda(), ids, C)
    assert torch.equal(a, b)                      # no atomics, fixed reduction order
    assert torch.equal(a[3], a[200])              # equal rows: equal bits, their mutual distance exactly 0
    same = x[:1].repeat(N, 1).cuda()
    z = ops.cluster_dist_sums(same, ids, C)
    assert (z == 0).all() and z.shape == (N, C)


def test_cluster_dist_sums_argument_errors(ops):
    from vlp_amd._lib import lib, ptr
    x = _normal(16, 8, 1).cuda()
    ids = (torch.arange(16) % 2).int().cuda()
    with pytest.raises(ValueError, match="C=9"):
        ops.cluster_dist_sums(x, ids, 9)
    bad = ids.clone()
    bad[5] = 2
    with pytest.raises(ValueError, match=r"labels must lie in \[0, 2\)"):
        ops.cluster_dist_sums(x, bad, 2)
    neg = ids.clone()
    neg[0] = -1
    with pytest.raises(ValueError, match="labels must lie"):
        ops.cluster_dist_sums(x, neg, 2)
    # the C ABI refuses before any launch: only the return code is read
    raw = lib()._fns["vlp_cluster_dist_sums"]
    out = torch.full((16, 9), -1.0, device="cuda")
    inval = 1                                     # hipErrorInvalidValue
    s = torch.cuda.current_stream().cuda_stream
    assert raw(16, 16, 8, ptr(x), 8, ptr(x), 8, ptr(ids), 9, ptr(out), s) == inval
    assert raw(16, 16, 8, ptr(x), 8, ptr(x), 8, ptr(ids), 0, ptr(out), s) == inval
    assert raw(16, 16, 0, ptr(x), 8, ptr(x), 8, ptr(ids), 2, ptr(out), s) == inval
    assert raw(16, 16, 8, ptr(x), 7, ptr(x), 8, ptr(ids), 2, ptr(out), s) == inval
    assert raw(16, 16, 8, ptr(x), 8, ptr(x), 7, ptr(ids), 2, ptr(out), s) == inval
    assert raw(-1, 16, 8, ptr(x), 8, ptr(x), 8, ptr(ids), 2, ptr(out), s) == inval
    assert raw(16, -1, 8, ptr(x), 8, ptr(x), 8, ptr(ids), 2, ptr(out), s) == inval
    assert raw(0, 16, 8, ptr(x), 8, ptr(x), 8, ptr(ids), 2, ptr(out), s) == 0
    torch.cuda.synchronize()
    assert (out == -1).all()                      # nothing was launched
    assert lib().vlp_abi_version() == 3


def _sil_cases():
    g = np.random.default_rng(21)
    blobs = g.normal(size=(200, 16)).astype(np.float32)
    blobs[:100] += 50.0
    blobs[100:] -= 50.0
    mixed = g.normal(size=(301, 48)).astype(np.float32)
    single = (np.arange(130) % 2).tolist()
    single[77] = 2
    return {
        "blobs": (blobs, [0] * 100 + [1] * 100),
        "interleaved": (mixed, (np.arange(301) % 2).tolist()),
        "strings": (mixed, ["INTERNAL" if i % 3 else "BTXRD" for i in range(301)]),
        "singleton": (mixed[:130], single),
    }


@pytest.mark.parametrize("case", ["blobs", "interleaved", "strings", "singleton"])
def test_silhouette_device_vs_fp64(ops, case):
    from vlp_amd import metrics
    x, y = _sil_cases()[case]
    N, D = x.shape
    s = metrics.silhouette_samples(torch.from_numpy(x).cuda(), y)
    assert s.is_cuda and s.dtype == torch.float64
    ref = silhouette_samples_fp64(x, y)
    atol = silhouette_atol(N, D)
    err = np.abs(s.cpu().numpy() - ref).max()
    score = metrics.silhouette_score(torch.from_numpy(x).cuda(), y)
    print(f"{case}: score {score:.6f} fp64 {ref.mean():.6f}; max sample err {err:.3e} (atol {atol:.3e})")
    assert err <= atol and abs(score - ref.mean()) <= atol
    if case == "blobs":
        assert score > 0.9
    if case == "interleaved":
        assert abs(score) < 0.05
    if case == "singleton":
        assert s[77].item() == 0.0


@pytest.mark.parametrize("case", ["blobs", "interleaved", "strings", "singleton"])
def test_silhouette_device_vs_sklearn(ops, case):
    sk = pytest.importorskip("sklearn.metrics")
    from vlp_amd import metrics
    x, y = _sil_cases()[case]
    ref = sk.silhouette_score(x.astype(np.float64), y)
    got = metrics.silhouette_score(torch.from_numpy(x).cuda(), y)
    atol = silhouette_atol(*x.shape)
    print(f"{case}: score {got:.6f} sklearn {ref:.6f} diff {abs(got - ref):.3e} (atol {atol:.3e})")
    assert abs(got - ref) <= atol


# ---------------- end to end through train() ----------------
# 12 training rows is the smallest synthetic fold whose tumour labels are not the dataset names
# renamed (the first 8 alternate together); 4 + 4 validation rows hold both names and both labels
SIZE = ["data.batch_size=4", "data.image_size=64", "data.n_samples=12", "data.n_val_samples=4",
        "data.num_workers=0", "trainer.max_epochs=1", "model.compute_dtype=fp32"]


def _recompute(best, loaders):
    """Features, logits, labels and names of the loaders from `best`, on the host."""
    from src.utils.post_fit_evaluation import _features_and_logits
    feats, logits, y, names = [], [], [], []
    best.eval()
    with torch.no_grad():
        for loader in loaders:
            for batch in loader:
                f, lg = _features_and_logits(best, batch)
                feats.append((f.mean((2, 3)) if f.dim() == 4 else f).float().cpu())
                logits.append(lg.float().flatten().cpu())
                y.extend(batch["tumor"].tolist())
                names.extend(batch["dataset"])
    return torch.cat(feats).numpy(), torch.cat(logits).numpy(), np.array(y), names


@pytest.mark.parametrize("experiment,monitor", [
    ("baseline_only_imaging/baseline_only_imaging_resnet_34_mi355x_eval", "val/combined/accuracy"),
    ("baseline_imaging_and_clinical/baseline_imaging_and_clinical_resnet_34_mi355x_eval", "val/btxrd/loss")])
def test_train_reports_post_fit_evaluation(tmp_path, experiment, monitor):
    from src import train as T
    from src.utils.config import compose
    from src.utils.post_fit_evaluation import best_checkpoint_callback
    cfg = compose("train", [f"experiment={experiment}", f"paths.output_dir={tmp_path}"] + SIZE)
    metrics, objs = T.train(cfg)
    for k in EVAL_KEYS:
        assert k in metrics and np.isfinite(metrics[k]), k
        print(f"{k}: {metrics[k]}")
    for split, n in (("validation", 8), ("train", 12)):
        assert sum(metrics[f"confusion_matrix_{split}/{k}"] for k in ("tn", "fp", "fn", "tp")) == n

    cb = best_checkpoint_callback(objs["trainer"])
    assert cb.monitor == monitor and cb.best_model_path.startswith(str(tmp_path))
    model = objs["model"]
    best = type(model).load_from_checkpoint(cb.best_model_path, device=model.device)
    fold, _ = next(objs["datamodule"].get_cv_splits())
    feats, logits, y, names = _recompute(best, fold.val_dataloader())
    assert feats.shape == (8, 512) and set(names) == {"INTERNAL", "BTXRD"} and set(y.tolist()) == {0, 1}
    pred = (torch.sigmoid(torch.from_numpy(logits)) > 0.5).numpy()      # strict, in the logits' own fp32
    want = {"tn": (~pred & (y == 0)).sum(), "fp": (pred & (y == 0)).sum(),
            "fn": (~pred & (y == 1)).sum(), "tp": (pred & (y == 1)).sum()}
    for k, v in want.items():
        assert metrics[f"confusion_matrix_validation/{k}"] == int(v), k
    atol = silhouette_atol(*feats.shape)
    for what, labels in (("tumor", y.tolist()), ("dataset", names)):
        ref = silhouette_samples_fp64(feats, labels).mean()
        got = metrics[f"silhouette_score_based_on_{what}_validation"]
        print(f"{what}: {got:.6f} vs fp64 {ref:.6f} (atol {atol:.3e})")
        assert abs(got - ref) <= atol
    tr_feats, _, tr_y, tr_names = _recompute(best, [fold.train_dataloader()])
    assert set(tr_names) == {"INTERNAL", "BTXRD"} and set(tr_y.tolist()) == {0, 1} and len(tr_y) == 12
