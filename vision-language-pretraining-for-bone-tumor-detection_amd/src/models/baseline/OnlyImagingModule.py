"""Drop-in for the reference's src/models/baseline/OnlyImagingModule.py: the
imaging-only binary tumour classifier (the default model of configs/train.yaml),
built on the MI355X image towers of the pretraining path.

Same constructor (model, optimizer, scheduler, label_weights, coral_lambda,
pretrained_vlp_module, :36-106), same `network` sub-module with timm key names
(`network.<timm resnet34 incl. fc>` / `network.<timm nest_small incl. head>`),
forward(x) -> flattened logits (:236-237), forward_features / forward_head
(:245-249) and configure_optimizers (:108-120).  _compute_loss (:251-302: weighted
BCE + optional CORAL between the INTERNAL and BTXRD samples' pooled features),
training_step (:305-335), validation_step's dataloader-index rule (:337-384) and
on_validation_epoch_end's combined evaluation over the cached probabilities, logits
and features (:386-430) are BaselineModule's, shared with FusionModule.

The networks:
  * resnet34: `ResNet34Classifier` (timm resnet34(num_classes=1) on the HIP
    tower, vlp_amd/resnet34.py); its fused average pool emits the pooled
    features, so forward_features returns [B, 512, 1, 1] -- every consumer in
    the reference takes the spatial mean of that map (forward_head's global
    pool, _compute_loss :282-283), the identity on a 1x1 map;
  * nest_small: `NestClassifier` (timm nest_small(num_classes=1) on the HIP NesT
    tower, vlp_amd/nest.py; `image_size` sets timm's img_size, default 224 as
    timm's), features [B, 384, 1, 1] after the final LayerNorm and token mean.
Not built (NotImplementedError): resnet50 and the torchxrayvision
resnet50-res512-all backbone.  vit_base/large_patch16_224 raise NotImplementedError
here as well: the tower and a ready `ViTClassifier` exist (vlp_amd/vit.py, used by
the pretraining ImageEncoder) but are not wired into this module yet.  Checkpoints of a pretrained
VisionLanguageModule load with torch.load(weights_only=True) (the reference uses
weights_only=False, :76).

Metrics: torchmetrics is not used; vlp_amd.metrics.BinaryMetrics restates the
Binary{Accuracy,Precision,Recall,F1Score,AUROC} values at threshold 0.5 that the
reference logs on the host (the default here), BinaryMetricsDevice
(`metrics_on_device=True`) on the device; both return the same bits.  With
`loss_on_device=True` the loss is one fp64 device op (vlp_amd/domain_loss.py).
"""
from __future__ import annotations

import logging
import os
import sys
from typing import Tuple

import torch
import torch.nn as nn

_PKG = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", ".."))
if _PKG not in sys.path:
    sys.path.insert(0, _PKG)

from src.models.baseline.BaselineModule import BaselineModule, ResNet34Classifier, supported_models  # noqa: E402
from src.models.pretrain.VisionLanguageModule import _HAVE_LIGHTNING, _default_device  # noqa: E402
from vlp_amd.metrics import BinaryMetrics, binary_metrics  # noqa: E402,F401  (re-exported)
from vlp_amd.nest import NestTower  # noqa: E402

logger = logging.getLogger("project")


class NestClassifier(NestTower):
    """timm nest_small(num_classes) on the HIP tower: forward_features / forward_head / forward."""

    def __init__(self, num_classes: int = 1, img_size: int = 224, compute_dtype: str = "fp32", device=None,
                 drop_path_rate: float = 0.5):
        super().__init__("nest_small", img_size=img_size, drop_path_rate=drop_path_rate,
                         compute_dtype=compute_dtype, device=device)
        self.head = nn.Linear(self.dims[-1], num_classes, device=device)

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        self.head._apply(fn)
        return self

    def forward_features(self, x):
        return NestTower.forward(self, x)[:, :, None, None]

    def forward_head(self, x):
        return self.head(x.mean((2, 3)) if x.dim() == 4 else x)

    def forward(self, x):
        return self.forward_head(self.forward_features(x))


class OnlyImagingModule(BaselineModule):
    _index_error_hint = " Supported indices are: 0, 1."

    def __init__(
        self,
        model: str,
        optimizer,
        scheduler=None,
        label_weights: Tuple[float] = (1.0, 1.0),
        coral_lambda: float = 0.0,
        pretrained_vlp_module: str = None,
        compute_dtype: str = "fp32",
        image_size: int = 224,
        device=None,
        metrics_on_device: bool = False,
        loss_on_device: bool = False,
        **kwargs,
    ):
        super().__init__()
        hp = dict(model=model, optimizer=optimizer, scheduler=scheduler, label_weights=label_weights,
                  coral_lambda=coral_lambda, pretrained_vlp_module=pretrained_vlp_module,
                  compute_dtype=compute_dtype, image_size=image_size, metrics_on_device=metrics_on_device,
                  loss_on_device=loss_on_device, **kwargs)
        if _HAVE_LIGHTNING:  # pragma: no cover
            self.save_hyperparameters(logger=False)
        else:
            self.save_hyperparameters(hp, logger=False)
        if model not in supported_models:                                              # :49-52
            raise ValueError(f"OnlyImagingModule: Model {model} is not supported. Supported models are: "
                             f"{supported_models}")
        if model not in ("resnet34", "nest_small"):
            raise NotImplementedError(f"OnlyImagingModule: {model} is not built for MI355X "
                                      "(resnet34 and nest_small are)")
        dev = _default_device(device)
        if model == "resnet34":
            self.network = ResNet34Classifier(1, compute_dtype=compute_dtype, device=dev)
        else:
            self.network = NestClassifier(1, img_size=image_size, compute_dtype=compute_dtype, device=dev,
                                          drop_path_rate=kwargs.get("drop_path_rate", 0.5))   # timm's default
        if pretrained_vlp_module is not None:                                          # :75-98
            self._load_pretrained_vision_encoder(pretrained_vlp_module)
        self.label_weights = torch.Tensor(label_weights)                               # :101
        self._make_metrics(metrics_on_device)
        self._clear_val_cache()
        logger.info("OnlyImagingModule (MI355X): initialized %s, compute_dtype=%s", model, compute_dtype)

    @property
    def device(self):
        return self.network.arena.data.device

    def get_image_network(self):
        return self.network

    # ---------------- optimizer (:108-120) ----------------
    def configure_optimizers(self):
        return self._optimizer_dict(self.hparams.optimizer(params=self.parameters()))

    # ---------------- forward (:236-249) ----------------
    def forward(self, x):
        return self.network(x.to(self.device, non_blocking=True)).flatten()

    def forward_features(self, x):
        return self.network.forward_features(x.to(self.device, non_blocking=True))

    def forward_head(self, x):
        return self.network.forward_head(x).flatten()

    def _unpack(self, batch):
        x = batch["x-ray"] if "x-ray" in batch else batch["x-ray-u8"]
        if hasattr(self.network, "u8_norm"):
            self.network.u8_norm = tuple(batch.get("x-ray-u8-norm", (127.5, 73.9)))
        return x, batch["tumor"], batch["dataset"]

    def features_and_logits(self, batch):
        features = self.forward_features(self._unpack(batch)[0])
        return features, self.forward_head(features)

    def _combined_metrics(self, probs, labels):
        if self.hparams.metrics_on_device:
            return super()._combined_metrics(probs, labels)
        return binary_metrics(probs.float().cpu(), labels.cpu().long())    # not through the accumulator
