"""Drop-in for the reference's src/models/baseline/FusionModule.py (late fusion of
ResNet34 imaging logits with a clinical-data MLP; SURVEY §8(f) row 1, BASELINE
configs[4]) on MI355X.

Same constructor (model, optimizer, scheduler, label_weights, coral_lambda,
pretrained_vlp_module, vision_encoder_lr, :38-50), same sub-module names and
state-dict keys (tabular_network.*, image_network.<timm resnet34 incl. fc>,
combination_network.*), same forward(x, age, sex, anatomy_site) -> (logits,
image_features) (:318-326) and configure_optimizers (:127-201: image_backbone /
head_and_remaining groups).  _compute_loss (:341-390), training_step (:392-420),
validation_step's dataloader index rule (:423-468), on_validation_epoch_end's
combined evaluation over the cached probabilities, logits and image features
(:470-504) and the metrics (:251-286) are BaselineModule's, shared with
OnlyImagingModule; the accumulators here are always vlp_amd.metrics.BinaryMetricsDevice.

The image network is the HIP ResNet34 tower of the pretraining path
(vlp_amd/resnet34.py, every conv / BN / pool on the hand-written kernels, >99.9 %
of the step's FLOPs).  Its fused average-pool kernel produces the pooled features
directly, so forward_features returns them as [B, 512, 1, 1]: the reference's
consumers only take the spatial mean of that map (forward_head's global pool,
CORAL's mean over (2, 3), :366-369), which is the identity on a 1x1 map.  The
fc, the 15->32->20->10 tabular MLP with BatchNorm1d, the 20->1 combination and
the loss (a few kFLOP per sample) run as device tensor ops; with
`loss_on_device=True` the loss is one fp64 device op instead (vlp_amd/domain_loss.py).

Not built: the vit / resnet50 / nest_small / torchxrayvision backbones
(NotImplementedError).  The t-SNE of the image features is part
of the post-fit evaluation (src/utils/post_fit_evaluation.py, `post_fit_tsne`).
Pretrained VLP checkpoints load with torch.load(weights_only=True) (the
reference uses weights_only=False, :84).
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

from src.models.baseline.BaselineModule import BaselineModule, ResNet34Classifier, supported_models  # noqa: E402,F401
from src.models.pretrain.VisionLanguageModule import _HAVE_LIGHTNING, _default_device  # noqa: E402

logger = logging.getLogger("project")


class FusionModule(BaselineModule):
    _val_loss_on_step = False      # val/{key}/loss is logged per epoch only here

    def __init__(
        self,
        model: str,
        optimizer,
        scheduler=None,
        label_weights: Tuple[float] = (1.0, 1.0),
        coral_lambda: float = 0.0,
        pretrained_vlp_module: str = None,
        vision_encoder_lr: float = None,
        compute_dtype: str = "fp32",
        device=None,
        loss_on_device: bool = False,
        **kwargs,
    ):
        super().__init__()
        hp = dict(model=model, optimizer=optimizer, scheduler=scheduler, label_weights=label_weights,
                  coral_lambda=coral_lambda, pretrained_vlp_module=pretrained_vlp_module,
                  vision_encoder_lr=vision_encoder_lr, compute_dtype=compute_dtype,
                  loss_on_device=loss_on_device, **kwargs)
        if _HAVE_LIGHTNING:  # pragma: no cover
            self.save_hyperparameters(logger=False)
        else:
            self.save_hyperparameters(hp, logger=False)
        assert vision_encoder_lr is None or vision_encoder_lr >= 0.0, \
            "FusionModule: vision_encoder_lr must be None or >= 0.0"                  # :52
        if model not in supported_models:
            raise ValueError(f"FusionModule: Model {model} is not supported. Supported models are: "
                             f"{supported_models}")
        if model != "resnet34":
            raise NotImplementedError(f"FusionModule: {model} is not built for MI355X (resnet34 is)")
        dev = _default_device(device)
        self.tabular_network = nn.Sequential(                                          # :60-70
            nn.Linear(15, 32), nn.BatchNorm1d(32), nn.ReLU(),
            nn.Linear(32, 20), nn.BatchNorm1d(20), nn.ReLU(),
            nn.Linear(20, 10), nn.BatchNorm1d(10), nn.ReLU()).to(dev)
        self.image_network = ResNet34Classifier(10, compute_dtype=compute_dtype, device=dev)
        if pretrained_vlp_module is not None:                                          # :82-113
            self._load_pretrained_vision_encoder(pretrained_vlp_module)
        self.combination_network = nn.Linear(20, 1).to(dev)                            # :117
        self.label_weights = torch.Tensor(label_weights)                               # :119
        self._make_metrics(on_device=True)                                             # :251-286
        self._clear_val_cache()
        logger.info("FusionModule (MI355X): initialized %s, compute_dtype=%s", model, compute_dtype)

    @property
    def device(self):
        return self.combination_network.weight.device

    @property
    def all_val_image_features(self):          # the reference's name for the cached features
        return self.all_val_features

    def get_image_network(self):
        return self.image_network

    # ---------------- optimizer (:127-201) ----------------
    def configure_optimizers(self):
        lr_v = self.hparams.vision_encoder_lr
        if lr_v is not None and lr_v >= 0.0:
            backbone, head = [], []
            for name, p in self.image_network.named_parameters():
                (head if ("head" in name or "classifier" in name or "fc" in name) else backbone).append(p)
            img_ids = {id(p) for p in self.image_network.parameters()}
            remaining = [p for p in self.parameters() if id(p) not in img_ids]
            groups = [{"params": backbone, "lr": lr_v, "name": "image_backbone"},
                      {"params": head + remaining, "name": "head_and_remaining_parameters"}]
            return self._optimizer_dict(self.hparams.optimizer(params=groups))
        return self._optimizer_dict(self.hparams.optimizer(params=self.parameters()))

    # ---------------- forward (:318-326) ----------------
    def forward(self, x, age_encoded, sex_encoded, anatomy_site_encoded):
        dev = self.device
        image_features = self.forward_image_features(x.to(dev, non_blocking=True))
        image_logits = self.forward_image_head(image_features)
        clinical = torch.cat((anatomy_site_encoded, age_encoded, sex_encoded), dim=1).to(dev, non_blocking=True)
        clinical_logits = self.tabular_network(clinical.float())
        logits = self.combination_network(torch.cat((image_logits, clinical_logits), dim=1)).flatten()
        return logits, image_features

    def forward_image_features(self, x):
        return self.image_network.forward_features(x)

    def forward_image_head(self, x):
        return self.image_network.forward_head(x)

    def _unpack(self, batch):
        x = batch["x-ray"] if "x-ray" in batch else batch["x-ray-u8"]
        self.image_network.u8_norm = tuple(batch.get("x-ray-u8-norm", (127.5, 73.9)))
        return (x, batch["tumor"], batch["dataset"], batch["anatomy_site_encoded"], batch["age_encoded"],
                batch["sex_encoded"])

    def features_and_logits(self, batch):
        x, _, _, site, age, sex = self._unpack(batch)
        logits, image_features = self.forward(x, age, sex, site)
        return image_features, logits
