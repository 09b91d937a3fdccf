"""What the downstream baselines (OnlyImagingModule, FusionModule) share: the weighted
BCE + CORAL loss, the data-parallel gradient hook, checkpoint loading, the optimizer /
scheduler dict, the metric accumulators, the validation cache and the training and
validation steps, which are the same in the reference's two modules but for names.

A subclass builds its networks and implements

    get_image_network()                                 # the HIP tower (arena, _param_slots)
    features_and_logits(batch) -> (features, logits)    # moves inputs to the device, one forward

and sets `_val_loss_on_step` / `_index_error_hint` where the two modules differ.
`ResNet34Classifier`, the image network of both, lives here as well.

Metrics: the reference's torchmetrics Binary{Accuracy, Precision, Recall, F1Score, AUROC}
under train/, val/internal/, val/btxrd/ and val/combined/ are vlp_amd.metrics accumulators.
BinaryMetrics keeps the epoch on the host; with BinaryMetricsDevice the probabilities and
labels stay on the device (one launch per step, no device-to-host copy) and each set of five
values costs one 48-byte read at the end of the epoch.  Both return the same bits.

Loss: with the hyper-parameter `loss_on_device=True` _compute_loss is one fp64 device op for
the weighted BCE, the CORAL term and both gradients (vlp_amd/domain_loss.py,
csrc/domain_loss_ops.hip): no boolean-mask index and no device-to-host read in the training
step or the epoch-end combined loss.  The default path is the reference's tensor ops.
"""
from __future__ import annotations

import logging
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

_PKG = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", ".."))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from src.models.pretrain.VisionLanguageModule import _Base, load_lightning_checkpoint  # noqa: E402
from src.utils.coral_loss.coral import coral  # noqa: E402
from vlp_amd.domain_loss import domain_loss  # noqa: E402
from vlp_amd.metrics import BinaryMetrics, BinaryMetricsDevice  # noqa: E402
from vlp_amd.resnet34 import ResNet34Tower  # noqa: E402

logger = logging.getLogger("project")

supported_models = ["vit_base_patch16_224", "vit_large_patch16_224", "resnet50", "resnet34", "nest_small",
                    "resnet50-res512-all"]


class ResNet34Classifier(ResNet34Tower):
    """timm resnet34(num_classes) on the HIP tower: forward_features / forward_head / forward."""

    def __init__(self, num_classes: int = 10, compute_dtype: str = "fp32", device=None):
        super().__init__(drop_rate=0.0, compute_dtype=compute_dtype, device=device)
        self.fc = nn.Linear(512, num_classes, device=device)

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        self.fc._apply(fn)
        return self

    def forward_features(self, x):
        return ResNet34Tower.forward(self, x)[:, :, None, None]

    def forward_head(self, x):
        return self.fc(x.mean((2, 3)) if x.dim() == 4 else x)

    def forward(self, x):
        return self.forward_head(self.forward_features(x))


class BaselineModule(_Base):
    _val_loss_on_step = True       # on_step of val/{key}/loss (the in-repo log ignores it, Lightning does not)
    _index_error_hint = ""         # appended to the unsupported-dataloader-index error

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location=None, strict=True, **kwargs):
        """Lightning-format checkpoint -> module (weights_only=True), as VisionLanguageModule's;
        the post-fit evaluation reloads the best checkpoint with it (train.py:305)."""
        return load_lightning_checkpoint(cls, checkpoint_path, map_location, strict, **kwargs)

    def _load_pretrained_vision_encoder(self, path):
        """A pretrained VisionLanguageModule checkpoint's image encoder into get_image_network()."""
        name = type(self).__name__
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        sd = {k.replace("image_encoder.model.", ""): v for k, v in ckpt["state_dict"].items()
              if k.startswith("image_encoder.model.")}
        missing, unexpected = self.get_image_network().load_state_dict(sd, strict=False)
        used = sum(v.numel() for k, v in sd.items() if k not in unexpected)
        if unexpected:
            logger.warning("%s: unexpected keys in the pretrained vision encoder: %s", name, unexpected)
        logger.info("%s: loaded %d pretrained vision-encoder parameters from %s (%d missing keys)",
                    name, used, path, len(missing))

    def _make_metrics(self, on_device: bool):
        metric = BinaryMetricsDevice if on_device else BinaryMetrics
        self.train_metrics = metric()
        self.val_metrics = {k: metric() for k in ("internal", "btxrd", "combined")}

    def _clear_val_cache(self):
        self.all_val_probs, self.all_val_labels, self.all_val_logits = [], [], []
        self.all_val_features, self.all_val_datset_labels = [], []

    def all_reduce_gradients(self, world: int) -> None:
        """Data-parallel gradient mean (DDP semantics, called by the trainer after
        backward): one SUM all-reduce over the tower's flat gradient arena and one
        over the remaining (head) gradients, both scaled by 1/world."""
        dist = torch.distributed
        tower = self.get_image_network()
        slots = [(owner._parameters[attr], full) for owner, attr, full in tower._param_slots]
        tower_ids = {id(p) for p, _ in slots}
        aliased = all(p.grad is not None and p.grad.data_ptr() == tower.arena.gview(full).data_ptr()
                      for p, full in slots)
        if aliased:          # tower gradients live in the arena: one call over the flat buffer
            dist.all_reduce(tower.arena.grad)
            tower.arena.grad.mul_(1.0 / world)
            rest = [p for p in self.parameters() if p.grad is not None and id(p) not in tower_ids]
        else:
            rest = [p for p in self.parameters() if p.grad is not None]
        if rest:
            flat = torch.cat([p.grad.reshape(-1) for p in rest])
            dist.all_reduce(flat)
            flat.mul_(1.0 / world)
            off = 0
            for p in rest:
                p.grad.copy_(flat[off:off + p.numel()].view_as(p.grad))
                off += p.numel()

    def _optimizer_dict(self, optimizer):
        if self.hparams.scheduler is not None:
            scheduler = self.hparams.scheduler(optimizer=optimizer)
            return {"optimizer": optimizer,
                    "lr_scheduler": {"scheduler": scheduler, "interval": "epoch", "frequency": 1}}
        return {"optimizer": optimizer}

    # ---------------- loss (FusionModule :341-390 == OnlyImagingModule :251-302) ----------------
    def _compute_loss(self, image_features, logits, labels, dataset):
        if getattr(self.hparams, "loss_on_device", False) and image_features.is_cuda:
            # one fp64 device op (csrc/domain_loss_ops.hip): no mask index, no read-back, and the
            # :375-376 rule below decided on the device from the rows' domain codes
            return domain_loss(image_features, logits, labels, dataset, self.label_weights,
                               self.hparams.coral_lambda)
        labels = labels.to(logits.device)
        lw = self.label_weights.to(logits.device)
        sample_weights = torch.where(labels == 0, lw[0], lw[1])
        classification_loss = F.binary_cross_entropy_with_logits(logits, labels.float(), weight=sample_weights)
        zero = torch.zeros((), device=logits.device)
        if self.hparams.coral_lambda == 0.0:
            return classification_loss, classification_loss, zero
        pooled = image_features.mean((2, 3)) if image_features.dim() == 4 else image_features
        internal = torch.tensor([d == "INTERNAL" for d in dataset], dtype=torch.bool)
        btxrd = torch.tensor([d == "BTXRD" for d in dataset], dtype=torch.bool)
        if internal.sum() <= 1 or btxrd.sum() <= 1:                                  # :375-376
            return classification_loss, classification_loss, zero
        dev = pooled.device
        coral_loss = self.hparams.coral_lambda * coral(pooled[internal.to(dev)], pooled[btxrd.to(dev)])
        return classification_loss + coral_loss, classification_loss, coral_loss

    # ---------------- steps (FusionModule :392-504, OnlyImagingModule :305-430) ----------------
    def training_step(self, batch, batch_idx=None):
        features, logits = self.features_and_logits(batch)
        labels, dataset = batch["tumor"], batch["dataset"]
        loss, cls, cor = self._compute_loss(features, logits, labels, dataset)
        self.train_metrics.update(torch.sigmoid(logits), labels)
        bs = labels.shape[0]
        self.log("train/classification_loss", cls, on_step=True, on_epoch=True, batch_size=bs)
        self.log("train/coral_loss", cor, on_step=True, on_epoch=True, batch_size=bs)
        self.log("train/loss", loss, on_step=True, on_epoch=True, batch_size=bs)
        return loss

    def on_train_epoch_end(self):
        for k, v in self.train_metrics.compute().items():
            self.log(f"train/{k}", v, on_step=False, on_epoch=True)
        self.train_metrics.reset()

    @torch.no_grad()
    def validation_step(self, batch, batch_idx, dataloader_idx=0):
        features, logits = self.features_and_logits(batch)
        labels, dataset = batch["tumor"], batch["dataset"]
        loss, _, _ = self._compute_loss(features, logits, labels, dataset)
        key = {0: "internal", 1: "btxrd"}.get(dataloader_idx)
        if key is None:
            raise ValueError(f"{type(self).__name__}: Validation dataloader index {dataloader_idx} is not "
                             f"supported.{self._index_error_hint}")
        probs = torch.sigmoid(logits)
        self.all_val_probs.append(probs)
        self.all_val_labels.append(labels.to(probs.device))
        self.all_val_logits.append(logits)
        self.all_val_features.append(features)
        self.all_val_datset_labels.extend(dataset)
        self.val_metrics[key].update(probs, labels)
        self.log(f"val/{key}/loss", loss, on_step=self._val_loss_on_step, on_epoch=True, add_dataloader_idx=False,
                 batch_size=labels.shape[0])
        return loss

    def _combined_metrics(self, probs, labels):
        combined = self.val_metrics["combined"]
        combined.update(probs, labels)
        values = combined.compute()
        combined.reset()
        return values

    @torch.no_grad()
    def on_validation_epoch_end(self):
        for key in ("internal", "btxrd"):
            for k, v in self.val_metrics[key].compute().items():
                self.log(f"val/{key}/{k}", v, on_step=False, on_epoch=True, add_dataloader_idx=False)
            self.val_metrics[key].reset()
        if not self.all_val_probs:
            return
        probs, labels = torch.cat(self.all_val_probs), torch.cat(self.all_val_labels)
        logits, features = torch.cat(self.all_val_logits), torch.cat(self.all_val_features)
        loss, cls, cor = self._compute_loss(features, logits, labels, self.all_val_datset_labels)
        bs = features.shape[0]
        self.log("val/combined/loss", loss, on_step=False, on_epoch=True, add_dataloader_idx=False, batch_size=bs)
        self.log("val/combined/classification_loss", cls, on_step=False, on_epoch=True,
                 add_dataloader_idx=False, batch_size=bs)
        self.log("val/combined/coral_loss", cor, on_step=False, on_epoch=True, add_dataloader_idx=False,
                 batch_size=bs)
        for k, v in self._combined_metrics(probs, labels).items():
            self.log(f"val/combined/{k}", v, on_step=False, on_epoch=True, add_dataloader_idx=False, batch_size=bs)
        self._clear_val_cache()
