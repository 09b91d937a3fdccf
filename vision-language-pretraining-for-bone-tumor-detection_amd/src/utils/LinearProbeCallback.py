"""Linear probe on the image encoder's features during pretraining (reference
src/utils/LinearProbeCallback.py:17-116).

Same constructor (train_dataloader, val_dataloaders, every_n_epochs=5), same gate
(every n-th epoch, skipped while sanity checking), same probe (eval-mode 512-d
features -> sklearn LogisticRegression(max_iter=1000, lbfgs) -> balanced accuracy
and AUROC on the concatenated validation sets), same two logged keys.

MI355X: the features come from the HIP ResNet34 tower (eval-mode BN from the
running statistics) on the uint8 upload when the loader provides it, with the
batches moved by the side-stream DevicePrefetcher.  As in the reference, the
encoder is left in eval mode (the trainer puts the module back in train mode
before the next step).

fit="sklearn" (the default) is the reference's probe: the [B, 512] features come
back to the host and sklearn fits and scores them.  fit="device" keeps features
and labels on the GPU: vlp_amd.metrics.logistic_regression minimises the same
objective there to a gradient of 1e-8 (csrc/logreg_ops.hip; deterministic, where
L-BFGS's tol=1e-4 leaves the coefficients dependent on the solver's path), and
balanced_accuracy / binary_auroc score it there; sklearn is not imported.

The two values are also written into trainer.logged_metrics (Lightning's
callback_metrics), where the probe-based checkpoint and early-stopping
callbacks (configs/callbacks/*_linear_probe_accuracy.yaml) monitor them.
"""
from __future__ import annotations

import logging

import numpy as np
import torch
from torch.utils.data import ConcatDataset, DataLoader

from src.data.PretrainDataModule import DevicePrefetcher

logger = logging.getLogger("project")


class LinearProbeCallback:
    def __init__(self, train_dataloader: DataLoader, val_dataloaders: list, every_n_epochs: int = 5,
                 fit: str = "sklearn"):
        if fit not in ("sklearn", "device"):
            raise ValueError(f"LinearProbeCallback: fit must be 'sklearn' or 'device', got {fit!r}")
        self.train_dataloader = train_dataloader
        val_dataset = ConcatDataset([dl.dataset for dl in val_dataloaders])
        self.val_dataloader = DataLoader(val_dataset, batch_size=train_dataloader.batch_size, shuffle=False,
                                         collate_fn=train_dataloader.collate_fn,
                                         pin_memory=torch.cuda.is_available())
        self.every_n_epochs = every_n_epochs
        self.fit = fit

    def on_validation_start(self, trainer, pl_module) -> None:
        if trainer.current_epoch % self.every_n_epochs != 0:
            return
        if getattr(trainer, "sanity_checking", False):
            return
        bacc, auroc = self._linear_probe_training(pl_module.image_encoder, pl_module.device)
        monitored = getattr(trainer, "logged_metrics", None)
        for key, value in (("downstream_validation/linear_probe_balanced_accuracy", bacc),
                           ("downstream_validation/linear_probe_auroc", auroc)):
            pl_module.log(key, value, on_step=False, on_epoch=True)
            if isinstance(monitored, dict):
                monitored[key] = float(value)

    def _linear_probe_training(self, image_encoder, device):
        image_encoder = image_encoder.eval()
        if self.fit == "device":
            return self._device_probe(image_encoder, device)
        from sklearn.linear_model import LogisticRegression
        from sklearn.metrics import balanced_accuracy_score, roc_auc_score
        X_train, y_train = self._extract_features(image_encoder, self.train_dataloader, device)
        X_val, y_val = self._extract_features(image_encoder, self.val_dataloader, device)
        clf = LogisticRegression(max_iter=1000, solver="lbfgs")
        clf.fit(X_train, y_train)
        y_pred = clf.predict(X_val)
        balanced_acc = balanced_accuracy_score(y_val, y_pred)
        auroc = roc_auc_score(y_val, clf.predict_proba(X_val)[:, 1])
        return balanced_acc, auroc

    def _device_probe(self, image_encoder, device):
        from vlp_amd import metrics
        X_train, y_train = self._extract_features_device(image_encoder, self.train_dataloader, device)
        X_val, y_val = self._extract_features_device(image_encoder, self.val_dataloader, device)
        clf = metrics.logistic_regression(X_train, y_train)
        if not clf.converged_:
            logger.warning("LinearProbeCallback: the device fit stopped at its iteration limit")
        scores = clf.decision_function(X_val)
        # the AUROC of predict_proba[:, 1], as the reference: scores that saturate to 1.0 tie there
        return (metrics.balanced_accuracy(y_val, (scores > 0).long()),
                metrics.binary_auroc(y_val, torch.sigmoid(scores)))

    def _extract_features(self, encoder, dataloader, device):
        feats, labels = [], []
        with torch.no_grad():
            for batch in DevicePrefetcher(dataloader, device):
                imgs = batch["x-ray"] if "x-ray" in batch else batch["x-ray-u8"]
                feats.append(encoder(imgs.to(device, non_blocking=True)).float().cpu().numpy())
                labels.append(batch["tumor"].cpu().numpy())
        return np.concatenate(feats, axis=0), np.concatenate(labels, axis=0)

    def _extract_features_device(self, encoder, dataloader, device):
        """(features [N, D] fp32, labels [N]) on `device`: nothing is copied to the host."""
        feats, labels = [], []
        with torch.no_grad():
            for batch in DevicePrefetcher(dataloader, device):
                imgs = batch["x-ray"] if "x-ray" in batch else batch["x-ray-u8"]
                feats.append(encoder(imgs.to(device, non_blocking=True)).float())
                labels.append(batch["tumor"].to(device, non_blocking=True))
        return torch.cat(feats, dim=0), torch.cat(labels, dim=0)
