"""GPU: FusionModule's classification metrics (reference FusionModule.py:393-504): the train/,
val/internal/, val/btxrd/ and val/combined/ accuracy, precision, recall, F1 and AUROC from the
device-resident BinaryMetricsDevice, the combined validation losses over the cached epoch, and
the checkpoint the reference's callbacks take from val/btxrd/accuracy.

The expected values come from logits the test records at the module's own forward (the very
tensors training_step / validation_step turn into probabilities), through OnlyImagingModule's host
binary_metrics: identical inputs, so the comparison is `==`."""
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("accuracy", "precision", "recall", "f1", "auroc")
B, H = 8, 64


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    oh = torch.nn.functional.one_hot
    x_u8 = torch.randint(0, 256, (B, 1, H, H), generator=g, dtype=torch.uint8)
    return {"x-ray": ((x_u8.float() - 127.5) / 73.9).repeat(1, 3, 1, 1),
            "tumor": torch.randint(0, 2, (B,), generator=g),
            "dataset": ["INTERNAL" if (i + seed) % 3 else "BTXRD" for i in range(B)],        # mixed rows
            "anatomy_site_encoded": oh(torch.randint(0, 9, (B,), generator=g), 9).float(),
            "age_encoded": oh(torch.randint(0, 4, (B,), generator=g), 4).float(),
            "sex_encoded": oh(torch.randint(0, 2, (B,), generator=g), 2).float()}


@pytest.fixture(scope="module")
def epoch():
    """Two training steps + on_train_epoch_end, two validation steps per dataloader +
    on_validation_epoch_end; what the module logged and what the test saw at its forward."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from src.models.baseline.FusionModule import FusionModule
    from src.models.baseline.OnlyImagingModule import binary_metrics
    torch.manual_seed(11)
    m = FusionModule("resnet34", functools.partial(torch.optim.AdamW, lr=1e-3), label_weights=(0.7, 2.0),
                     coral_lambda=0.5, compute_dtype="fp32")
    seen = []
    forward = m.forward

    def recording_forward(*a, **kw):
        logits, features = forward(*a, **kw)
        seen.append((logits.detach().clone(), features.detach().clone()))
        return logits, features

    m.forward = recording_forward
    opt = m.configure_optimizers()["optimizer"]
    out = {"module": m, "binary_metrics": binary_metrics}

    def host(logit_list, label_list):
        p = torch.sigmoid(torch.cat(logit_list)).float().cpu()
        return binary_metrics(p, torch.cat(label_list).long())

    m.train()
    train = [_batch(s) for s in (1, 2)]
    for i, b in enumerate(train):
        opt.zero_grad(set_to_none=False)
        m.training_step(b, i).backward()
        opt.step()
    out["train_want"] = host([lg for lg, _ in seen], [b["tumor"] for b in train])
    assert "train/accuracy" not in m.logged
    m.on_train_epoch_end()
    out["train_len_after"] = len(m.train_metrics)

    m.eval()
    del seen[:]
    val = {0: [_batch(s) for s in (3, 4)], 1: [_batch(s) for s in (5, 6)]}
    last_loss = {}
    with torch.no_grad():
        for idx in (0, 1):
            for j, b in enumerate(val[idx]):
                last_loss[idx] = float(m.validation_step(b, j, idx))
    out["last_loss"] = last_loss
    order = val[0] + val[1]
    logits, feats = [lg for lg, _ in seen], [f for _, f in seen]
    labels = [b["tumor"] for b in order]
    out["val_want"] = {"internal": host(logits[:2], labels[:2]), "btxrd": host(logits[2:], labels[2:]),
                       "combined": host(logits, labels)}
    # the caches hold the epoch in order, and the combined loss is _compute_loss over them
    assert len(m.all_val_probs) == 4 and len(m.all_val_datset_labels) == 4 * B
    assert torch.equal(torch.cat(m.all_val_logits), torch.cat(logits))
    assert torch.equal(torch.cat(m.all_val_image_features), torch.cat(feats))
    assert torch.equal(torch.cat(m.all_val_labels).cpu(), torch.cat(labels))
    assert torch.equal(torch.cat(m.all_val_probs), torch.sigmoid(torch.cat(logits)))
    assert m.all_val_datset_labels == [d for b in order for d in b["dataset"]]
    with torch.no_grad():
        out["combined_losses"] = [float(v) for v in m._compute_loss(
            torch.cat(m.all_val_image_features), torch.cat(m.all_val_logits), torch.cat(m.all_val_labels),
            list(m.all_val_datset_labels))]
        m.on_validation_epoch_end()
    out["logged"] = dict(m.logged)
    return out


def test_keys_logged(epoch):
    logged = epoch["logged"]
    for k in KEYS:
        for prefix in ("train", "val/internal", "val/btxrd", "val/combined"):
            assert f"{prefix}/{k}" in logged, (prefix, k)
    for k in ("loss", "classification_loss", "coral_loss"):
        assert f"val/combined/{k}" in logged and f"train/{k}" in logged, k
    assert "val/internal/loss" in logged and "val/btxrd/loss" in logged       # as before


def test_values_equal_host_metrics(epoch):
    logged = epoch["logged"]
    for k in KEYS:
        print(f"train/{k} {logged[f'train/{k}']} host {epoch['train_want'][k]}")
        assert logged[f"train/{k}"] == epoch["train_want"][k], k
        for key, want in epoch["val_want"].items():
            print(f"val/{key}/{k} {logged[f'val/{key}/{k}']} host {want[k]}")
            assert logged[f"val/{key}/{k}"] == want[k], (key, k)
    assert all(isinstance(logged[f"val/combined/{k}"], float) for k in KEYS)


def test_combined_losses_and_earlier_keys(epoch):
    logged = epoch["logged"]
    loss, cls, cor = epoch["combined_losses"]
    assert float(logged["val/combined/loss"]) == loss
    assert float(logged["val/combined/classification_loss"]) == cls
    assert float(logged["val/combined/coral_loss"]) == cor
    assert cor > 0.0 and loss == pytest.approx(cls + cor, rel=1e-6)
    # what validation_step logged before this feature keeps its key and its value: the step's loss
    assert float(logged["val/internal/loss"]) == epoch["last_loss"][0]
    assert float(logged["val/btxrd/loss"]) == epoch["last_loss"][1]


def test_caches_and_accumulators_are_empty_afterwards(epoch):
    m = epoch["module"]
    assert m.all_val_probs == [] and m.all_val_labels == [] and m.all_val_logits == []
    assert m.all_val_image_features == [] and m.all_val_datset_labels == []
    assert epoch["train_len_after"] == 0
    assert all(len(v) == 0 and v.compute() == {} for v in m.val_metrics.values())


def test_trainer_keeps_the_best_btxrd_accuracy_checkpoint(tmp_path):
    """One epoch through the Trainer with the reference's checkpoint_btxrd monitor: the module
    logs val/btxrd/accuracy, so ModelCheckpoint finds a score and keeps a loadable file."""
    from src.data.DownstreamDataModule import DownstreamDataModule
    from src.models.baseline.FusionModule import FusionModule
    from src.utils.trainer import ModelCheckpoint, Trainer
    torch.manual_seed(12)
    m = FusionModule("resnet34", functools.partial(torch.optim.AdamW, lr=1e-3), compute_dtype="fp32")
    dm = DownstreamDataModule(batch_size=8, num_workers=0, image_size=32, n_samples=40, n_val_samples=16)
    fold, _ = next(dm.get_cv_splits())
    ck = ModelCheckpoint(monitor="val/btxrd/accuracy", mode="max", dirpath=str(tmp_path))
    t = Trainer(max_epochs=1, callbacks=[ck], default_root_dir=str(tmp_path))
    t.fit(m, fold)
    for key in ("internal", "btxrd", "combined"):
        for k in KEYS:
            assert 0.0 <= t.logged_metrics[f"val/{key}/{k}"] <= 1.0, (key, k)
    assert ck.best_model_path and os.path.isfile(ck.best_model_path)
    assert ck.best_model_score == t.logged_metrics["val/btxrd/accuracy"]
    best = FusionModule.load_from_checkpoint(ck.best_model_path, device=m.device)
    sd = m.state_dict()
    for k, v in best.state_dict().items():
        assert torch.equal(v, sd[k]), k
