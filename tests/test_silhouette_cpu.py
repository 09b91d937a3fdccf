"""CPU: silhouette scores and the baselines' post-fit evaluation (reference
src/train.py:179-183 and :261-327, plot_tsne_and_calculate_silhouette.py:15-98,
plot_confusion_matrix.py:14-60) without a device: vlp_amd.metrics on CPU tensors
(fp64 torch.cdist path) against sklearn and an fp64 numpy restatement, the
checkpoint-callback priority, evaluate_split / post_fit_evaluation with a
stand-in module, and the new experiment configs.

Tolerance (derived, not tuned; full derivation in tests/silhouette_ref.py): all
summed terms are non-negative, so one per-cluster distance sum is within
(D + N + 3) u of exact arithmetic to first order for any summation order
(differences u, squares and their sum (D + 2) u, halved by the root plus its
rounding, N u for the sum of distances); rtol = 2 (D + N + 3) u covers the
higher orders, and the b - a cancellation of a silhouette value gives
atol = 4 rtol.  Here the arithmetic is fp64: u = 2^-53.
"""
import types

import numpy as np
import pytest
import torch

from src.utils.config import compose
from tests.silhouette_ref import silhouette_atol, silhouette_samples_fp64

U64 = 2.0 ** -53
N, D = 37, 24


def _x(seed=0):
    return np.random.default_rng(seed).normal(size=(N, D)).astype(np.float32)


def _cases():
    x = _x()
    dup = x.copy()
    dup[20] = dup[7]
    single = (np.arange(N) % 2).tolist()
    single[5] = 2
    return {
        "three_labels": (x, (np.arange(N) % 3).tolist()),
        "string_labels": (x, ["INTERNAL" if i % 3 else "BTXRD" for i in range(N)]),
        "singleton": (x, single),
        "duplicate_rows": (dup, (np.arange(N) % 3).tolist()),
    }


@pytest.mark.parametrize("case", ["three_labels", "string_labels", "singleton", "duplicate_rows"])
def test_silhouette_cpu_vs_fp64(case):
    from vlp_amd import metrics
    x, y = _cases()[case]
    got = metrics.silhouette_samples(torch.from_numpy(x), y)
    assert got.dtype == torch.float64 and got.shape == (N,)
    ref = silhouette_samples_fp64(x, y)
    atol = silhouette_atol(N, D, U64)
    err = np.abs(got.numpy() - ref).max()
    print(f"{case}: max |s - fp64| {err:.3e} (atol {atol:.3e})")
    assert err <= atol
    assert abs(metrics.silhouette_score(torch.from_numpy(x), y) - ref.mean()) <= atol
    if case == "singleton":
        assert got[5].item() == 0.0
    # labels as 0-d tensors / a tensor, as the reference collects them
    if case == "three_labels":
        assert torch.equal(metrics.silhouette_samples(torch.from_numpy(x), [torch.tensor(v) for v in y]), got)
        assert torch.equal(metrics.silhouette_samples(torch.from_numpy(x), torch.tensor(y)), got)


@pytest.mark.parametrize("case", ["three_labels", "string_labels", "singleton", "duplicate_rows"])
def test_silhouette_cpu_vs_sklearn(case):
    sk = pytest.importorskip("sklearn.metrics")
    from vlp_amd import metrics
    x, y = _cases()[case]
    atol = silhouette_atol(N, D, U64)
    ref = sk.silhouette_score(x.astype(np.float64), y)
    got = metrics.silhouette_score(torch.from_numpy(x), y)
    print(f"{case}: score {got:.6f} sklearn {ref:.6f} diff {abs(got - ref):.3e} (atol {atol:.3e})")
    assert abs(got - ref) <= atol
    refs = sk.silhouette_samples(x.astype(np.float64), y)
    assert np.abs(metrics.silhouette_samples(torch.from_numpy(x), y).numpy() - refs).max() <= atol


def test_silhouette_label_count_errors():
    from vlp_amd import metrics
    x = torch.from_numpy(_x())
    for labels, n in (([0] * N, 1), (list(range(N)), N)):
        with pytest.raises(ValueError, match=rf"Number of labels is {n}\. Valid values are 2 to n_samples - 1 "
                                             r"\(inclusive\)"):
            metrics.silhouette_score(x, labels)
    with pytest.raises(ValueError, match="9 distinct labels, at most 8"):
        metrics.silhouette_score(x, [i % 9 for i in range(N)])
    from vlp_amd import ops
    with pytest.raises(ValueError, match="C=9"):           # checked before anything touches a device
        ops.cluster_dist_sums(x, torch.zeros(N, dtype=torch.int32), 9)


def _cb(monitor, path="x.ckpt"):
    return types.SimpleNamespace(monitor=monitor, best_model_path=path)


def test_best_checkpoint_callback_priority():
    from src.utils.post_fit_evaluation import best_checkpoint_callback as best
    internal, btxrd, btxrd2 = _cb("val/internal/accuracy"), _cb("val/btxrd/accuracy"), _cb("val/btxrd/loss")
    combined, last = _cb("val/combined/accuracy"), _cb(None)
    early = types.SimpleNamespace(monitor="val/combined/loss")          # EarlyStopping: no best_model_path
    tr = lambda *cbs: types.SimpleNamespace(callbacks=list(cbs))        # noqa: E731
    assert best(tr(internal, btxrd, combined)) is combined
    assert best(tr(early, combined, btxrd)) is combined
    assert best(tr(internal, btxrd, early)) is btxrd
    assert best(tr(btxrd, btxrd2)) is btxrd2                             # train.py:285-287 keeps the last one
    assert best(tr(internal, last)) is None and best(tr()) is None
    # Lightning's trainer.checkpoint_callbacks is used where it exists
    assert best(types.SimpleNamespace(checkpoint_callbacks=[btxrd], callbacks=[combined])) is btxrd
    # the project's own trainer and callbacks
    from src.utils.trainer import EarlyStopping, ModelCheckpoint, Trainer
    ck_c, ck_b = ModelCheckpoint(monitor="val/combined/accuracy", mode="max"), ModelCheckpoint(monitor="val/btxrd/loss")
    assert best(Trainer(callbacks=[ck_b, EarlyStopping("val/combined/loss"), ck_c])) is ck_c
    assert best(Trainer(callbacks=[ck_b])) is ck_b
    assert best(Trainer(callbacks=[])) is None                          # the default checkpoint has no monitor


class _StandIn(torch.nn.Module):
    """An OnlyImagingModule-shaped module on CPU: 64-d pixel features as a [B, 64, 1, 1] map,
    logit = scale * (first pixel - 128), so a first pixel of 128 is a probability of exactly 0.5."""

    device = torch.device("cpu")

    def __init__(self, scale=0.25, device=None):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.tensor(float(scale)))
        self.modes = []

    def _unpack(self, batch):
        return batch["x-ray-u8"], batch["tumor"], batch["dataset"]

    def forward_features(self, x):
        self.modes.append((self.training, torch.is_grad_enabled()))
        return (x.float().flatten(1) / 255.0)[:, :, None, None]

    def forward_head(self, f):
        return self.scale * (torch.round(f.mean((2, 3))[:, 0] * 255.0) - 128.0)

    def features_and_logits(self, batch):
        f = self.forward_features(self._unpack(batch)[0])
        return f, self.forward_head(f)

    @classmethod
    def load_from_checkpoint(cls, path, device=None):
        m = cls(device=device)
        m.load_state_dict(torch.load(path, weights_only=True)["state_dict"])
        return m


class _Loader:
    """A DataLoader stand-in: iterable over batches, not a list (a list is a list of loaders)."""

    def __init__(self, batches):
        self.batches = batches

    def __iter__(self):
        return iter(self.batches)


def _batches(n, bs, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, 1, 8, 8), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 2, (n,), generator=g)
    x[0, 0, 0, 0], y[0] = 128, 1            # probability exactly 0.5 on a positive: a false negative
    x[1, 0, 0, 0], y[1] = 129, 1            # just above: a true positive
    names = ["INTERNAL" if i % 3 else "BTXRD" for i in range(n)]
    return _Loader([{"x-ray-u8": x[i:i + bs], "tumor": y[i:i + bs], "dataset": names[i:i + bs]}
                    for i in range(0, n, bs)])


def _expect(loaders, scale):
    batches = [b for l in loaders for b in l]
    x = torch.cat([b["x-ray-u8"] for b in batches])
    y = torch.cat([b["tumor"] for b in batches]).numpy()
    names = [n for b in batches for n in b["dataset"]]
    feats = (x.float().flatten(1) / 255.0).numpy()
    prob = torch.sigmoid(scale * (x[:, 0, 0, 0].float() - 128.0)).numpy()
    return feats, y, names, prob


def test_evaluate_split_stand_in_module():
    from src.utils.post_fit_evaluation import evaluate_split
    a, b = _batches(21, 8, 0), _batches(14, 8, 1)
    m = _StandIn()
    m.train()
    res = evaluate_split(m, [a, b])
    assert m.training and m.modes and all(mode == (False, False) for mode in m.modes)   # eval + no_grad inside
    m.eval()
    evaluate_split(m, a)                                                 # a single loader, eval mode stays
    assert not m.training
    feats, y, names, prob = _expect([a, b], 0.25)
    assert (prob == 0.5).sum() == 2 and y[prob == 0.5].all()
    pred = prob > 0.5
    cm = [[int((~pred & (y == 0)).sum()), int((pred & (y == 0)).sum())],
          [int((~pred & (y == 1)).sum()), int((pred & (y == 1)).sum())]]
    assert res["confusion_matrix"] == cm and all(isinstance(v, int) for r in res["confusion_matrix"] for v in r)
    assert res["confusion_matrix"][1][0] >= 2                            # the two 0.5s are false negatives
    loose = prob >= 0.5                                                  # BinaryMetrics' rule would move them
    assert int((loose & (y == 1)).sum()) == cm[1][1] + 2
    atol = silhouette_atol(35, 64, U64)
    assert abs(res["silhouette_score_based_on_tumor"] - silhouette_samples_fp64(feats, y.tolist()).mean()) <= atol
    assert abs(res["silhouette_score_based_on_dataset"] - silhouette_samples_fp64(feats, names).mean()) <= atol
    sk = pytest.importorskip("sklearn.metrics")
    assert sk.confusion_matrix(y, pred.astype(np.int64)).tolist() == res["confusion_matrix"]
    assert abs(res["silhouette_score_based_on_dataset"] - sk.silhouette_score(feats.astype(np.float64), names)) <= atol


def test_evaluate_split_single_dataset_name_is_nan(caplog):
    from src.utils.post_fit_evaluation import evaluate_split
    a = _batches(12, 4, 2)
    for b in a.batches:
        b["dataset"] = ["BTXRD"] * len(b["dataset"])
    with caplog.at_level("WARNING", logger="project"):
        res = evaluate_split(_StandIn(), a)
    assert np.isnan(res["silhouette_score_based_on_dataset"]) and np.isfinite(res["silhouette_score_based_on_tumor"])
    assert any("one dataset name" in r.getMessage() for r in caplog.records)


def test_post_fit_evaluation_stand_in_module(tmp_path, caplog):
    from src.utils.post_fit_evaluation import evaluate_split, post_fit_evaluation
    val, train = [_batches(10, 4, 3), _batches(9, 4, 4)], _batches(17, 4, 5)
    dm = types.SimpleNamespace(val_dataloader=lambda: val, train_dataloader=lambda: train)
    best = _StandIn(scale=-0.5)                     # the checkpoint differs from the module in hand
    path = str(tmp_path / "best.ckpt")
    torch.save({"state_dict": best.state_dict()}, path)
    trainer = types.SimpleNamespace(callbacks=[_cb("val/btxrd/accuracy", "missing.ckpt"),
                                               _cb("val/combined/accuracy", path)])
    out = post_fit_evaluation(_StandIn(scale=0.25), dm, trainer)
    keys = {f"silhouette_score_based_on_{w}_{s}" for w in ("tumor", "dataset") for s in ("validation", "train")}
    keys |= {f"confusion_matrix_{s}/{k}" for s in ("validation", "train") for k in ("tn", "fp", "fn", "tp")}
    assert set(out) == keys
    for split, loaders, n in (("validation", val, 19), ("train", train, 17)):
        ref = evaluate_split(best, loaders)
        (tn, fp), (fn, tp) = ref["confusion_matrix"]
        assert [out[f"confusion_matrix_{split}/{k}"] for k in ("tn", "fp", "fn", "tp")] == [tn, fp, fn, tp]
        assert tn + fp + fn + tp == n
        assert out[f"silhouette_score_based_on_tumor_{split}"] == ref["silhouette_score_based_on_tumor"]
        assert out[f"silhouette_score_based_on_dataset_{split}"] == ref["silhouette_score_based_on_dataset"]
    other = evaluate_split(_StandIn(scale=0.25), val)["confusion_matrix"]
    assert other != evaluate_split(best, val)["confusion_matrix"]       # so the reload is what was measured
    # no combined / btxrd checkpoint callback: the message, and nothing else
    with caplog.at_level("INFO", logger="project"):
        assert post_fit_evaluation(_StandIn(), dm, types.SimpleNamespace(callbacks=[_cb("val/internal/loss", path)])) == {}
    assert any("no checkpoint callback monitoring" in r.getMessage() for r in caplog.records)
    # a callback that never saved a best model
    assert post_fit_evaluation(_StandIn(), dm, types.SimpleNamespace(callbacks=[_cb("val/btxrd/loss", "")])) == {}


def test_baseline_modules_load_from_checkpoint():
    from src.models.baseline.FusionModule import FusionModule
    from src.models.baseline.OnlyImagingModule import OnlyImagingModule
    for cls in (OnlyImagingModule, FusionModule):
        assert cls.load_from_checkpoint.__self__ is cls


def test_eval_experiments_compose_with_the_gate():
    c = compose("train", ["experiment=baseline_only_imaging/baseline_only_imaging_resnet_34_mi355x_eval"])
    assert c["post_fit_evaluation"] is True
    assert c["model"]["_target_"] == "src.models.baseline.OnlyImagingModule.OnlyImagingModule"
    assert c["model"]["model"] == "resnet34"
    monitors = [v.get("monitor") for v in c["callbacks"].values() if "ModelCheckpoint" in v.get("_target_", "")]
    assert "val/combined/accuracy" in monitors
    f = compose("train", ["experiment=baseline_imaging_and_clinical/baseline_imaging_and_clinical_resnet_34_mi355x_eval"])
    assert f["post_fit_evaluation"] is True and f["model"]["_target_"] == "src.models.baseline.FusionModule.FusionModule"
    monitors = [v.get("monitor") for v in f["callbacks"].values() if "ModelCheckpoint" in v.get("_target_", "")]
    assert "val/btxrd/loss" in monitors                                  # a metric FusionModule logs
    # existing experiments and the primary config carry no key: the evaluation stays off
    old = compose("train", ["experiment=baseline_imaging_and_clinical/baseline_imaging_and_clinical_resnet_34"])
    assert "post_fit_evaluation" not in old and "post_fit_evaluation" not in compose("train", [])
    for k in ("model", "callbacks", "trainer", "data", "optimizer", "scheduler"):
        want = dict(old[k])
        got = dict(f[k])
        if k == "callbacks":
            got.pop("checkpoint_btxrd_loss")
        assert got == want, k
