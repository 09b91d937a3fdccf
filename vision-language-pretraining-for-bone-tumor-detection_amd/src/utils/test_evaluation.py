"""Test-set evaluation with per-subgroup metrics (reference scripts/test_eval_downstream.py
and scripts/linear_probe_test_eval_downstream.py: collect_probs, evaluate_results,
calculate_metrics): a model's probabilities over DownstreamDataModule.test_dataloader(fold)
and one table of (level, group, fold, metric, value) -- six metrics overall and per dataset,
entity, anatomy site, sex, encoded age and age group.

The probabilities stay on the device in one growing buffer.  The tumour label and the seven
levels' group codes are built per batch on the host from the batch's metadata (groups numbered
in order of first appearance, pandas' unique() order in the reference) and uploaded as uint8.
Per fold, vlp_amd.metrics.grouped_binary_counts counts every group of every level in one pass
(csrc/groupmetric_ops.hip) and the host reads cells x 48 bytes; subgroup_metrics_from_counts
applies the script's rules per cell.  The reference takes about 40 boolean-mask subsets per fold
and six sklearn calls on each; pandas and sklearn are not imported here.

Not built: the W&B run-id lookup (the scripts take checkpoint paths) and --save-failures (the
PNG dumps of misclassified radiographs).
"""
from __future__ import annotations

import csv
import logging
import math
import os
from typing import Callable, List, Sequence, Tuple

import torch

from vlp_amd import metrics

log = logging.getLogger("project")

LEVELS = ("overall", "dataset", "entity", "anatomy_site", "sex", "age_encoded", "age_group")
MAX_GROUPS = 255      # codes 0 .. 254; metrics.NO_GROUP marks a row outside every group
PREDICTION_COLUMNS = ("dataset", "entity", "anatomy_site", "sex", "age", "age_encoded", "tumor", "prob", "age_group")


def age_group(age: int) -> str:
    """The scripts' three age groups (test_eval_downstream.py:71-76)."""
    return "0-18" if age < 19 else ("19-39" if age < 40 else "40+")


class _DeviceRows:
    """A 1-D or 2-D buffer on one device that doubles along its last dimension when full."""

    def __init__(self, rows: int, dtype, capacity: int = 1024):
        self.rows, self.dtype, self.capacity, self.n, self.buf = rows, dtype, capacity, 0, None

    def append(self, t: torch.Tensor):
        b = t.shape[-1]
        if self.buf is None or self.n + b > self.buf.shape[-1]:
            cap = max(self.capacity, self.n + b, 2 * (self.buf.shape[-1] if self.buf is not None else 0))
            new = torch.empty((self.rows, cap), dtype=self.dtype, device=t.device)
            if self.buf is not None:
                new[:, :self.n].copy_(self.buf[:, :self.n])
            self.buf = new
        self.buf[:, self.n:self.n + b].copy_(t.reshape(self.rows, b), non_blocking=True)
        self.n += b

    def view(self) -> torch.Tensor:
        return self.buf[:, :self.n].contiguous()


class Predictions:
    """One fold's test-set predictions: probs [n] fp32, tumor [n] uint8 and codes [7, n] uint8 on
    one device; groups[l] the names of level l's groups, index = code; columns the host-side
    metadata per row (the scripts' prediction table without the probabilities)."""

    def __init__(self, probs, tumor, codes, groups, columns):
        self.probs, self.tumor, self.codes, self.groups, self.columns = probs, tumor, codes, groups, columns

    def __len__(self):
        return self.probs.shape[0]

    def to(self, device) -> "Predictions":
        return Predictions(self.probs.to(device), self.tumor.to(device), self.codes.to(device), self.groups,
                           self.columns)

    def cpu(self) -> "Predictions":
        return self.to("cpu")


def batch_levels(batch: dict) -> List[list]:
    """The seven levels' group names of a batch's rows, LEVELS' order, from its metadata."""
    n = len(batch["dataset"])
    ages = [int(a) for a in batch["age"].tolist()]
    return [["overall"] * n, list(batch["dataset"]), list(batch["entity"]), list(batch["anatomy_site"]),
            list(batch["sex"]), [str(int(i)) for i in batch["age_encoded"].argmax(1).tolist()],
            [age_group(a) for a in ages]]


class _LevelCoder:
    """Group name -> uint8 code per level, numbered in order of first appearance."""

    def __init__(self):
        self.index = [dict() for _ in LEVELS]

    def encode(self, names: List[list]) -> torch.Tensor:
        """uint8 [7, B] (host) of a batch's group names, LEVELS' order."""
        rows = []
        for l, level in enumerate(names):
            index = self.index[l]
            for name in level:
                if name not in index:
                    if len(index) == MAX_GROUPS:
                        raise ValueError(f"test evaluation: level {LEVELS[l]!r} has more than {MAX_GROUPS} groups")
                    index[name] = len(index)
            rows.append([index[name] for name in level])
        return torch.tensor(rows, dtype=torch.uint8)

    def groups(self) -> List[list]:
        return [list(d) for d in self.index]


def _labels_u8(y: torch.Tensor) -> torch.Tensor:
    return torch.where(y == 1, 1, torch.where(y == 0, 0, 2)).to(torch.uint8)


def _collect(prob_fn: Callable[[dict], torch.Tensor], dataloader) -> Predictions:
    coder = _LevelCoder()
    probs, tumor = _DeviceRows(1, torch.float32), _DeviceRows(1, torch.uint8)
    codes = _DeviceRows(len(LEVELS), torch.uint8)
    columns = {k: [] for k in PREDICTION_COLUMNS if k != "prob"}
    for batch in dataloader:
        p = prob_fn(batch).detach().reshape(-1).float()
        names = batch_levels(batch)
        y = batch["tumor"].reshape(-1).cpu()
        if y.numel() != p.numel() or len(names[0]) != p.numel():
            raise ValueError(f"test evaluation: {p.numel()} probabilities for {y.numel()} labels")
        probs.append(p)
        tumor.append(_labels_u8(y).to(p.device, non_blocking=True))
        codes.append(coder.encode(names).to(p.device, non_blocking=True))
        for k, v in (("dataset", names[1]), ("entity", names[2]), ("anatomy_site", names[3]), ("sex", names[4]),
                     ("age", [int(a) for a in batch["age"].tolist()]), ("age_encoded", names[5]),
                     ("tumor", [int(t) for t in y.tolist()]), ("age_group", names[6])):
            columns[k].extend(v)
    if probs.n == 0:
        raise ValueError("test evaluation: the dataloader yielded no rows")
    return Predictions(probs.view()[0], tumor.view()[0], codes.view(), coder.groups(), columns)


def predictions_from_table(columns: dict, probs: torch.Tensor) -> Predictions:
    """Predictions from the scripts' prediction table: columns "dataset", "entity", "anatomy_site",
    "sex", "age", "age_encoded" (the one-hot's index) and "tumor" as lists of one length, probs [n] on
    the device the counts should run on."""
    n = probs.numel()
    ages = [int(a) for a in columns["age"]]
    names = [["overall"] * n, list(columns["dataset"]), list(columns["entity"]), list(columns["anatomy_site"]),
             list(columns["sex"]), [str(int(a)) for a in columns["age_encoded"]], [age_group(a) for a in ages]]
    if any(len(level) != n for level in names) or len(columns["tumor"]) != n:
        raise ValueError(f"test evaluation: the table's columns do not all hold {n} rows")
    coder = _LevelCoder()
    codes = coder.encode(names).to(probs.device)
    y = torch.tensor([int(t) for t in columns["tumor"]], dtype=torch.long)
    cols = {"dataset": names[1], "entity": names[2], "anatomy_site": names[3], "sex": names[4], "age": ages,
            "age_encoded": names[5], "tumor": y.tolist(), "age_group": names[6]}
    return Predictions(probs.detach().reshape(-1).float(), _labels_u8(y).to(probs.device), codes, coder.groups(),
                       cols)


def collect_probs(model, dataloader) -> Predictions:
    """sigmoid(logits) of `model` (a BaselineModule: its features_and_logits(batch)) over a test
    dataloader: eval mode, no_grad."""
    def prob_fn(batch):
        return torch.sigmoid(model.features_and_logits(batch)[1].float().flatten())

    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            return _collect(prob_fn, dataloader)
    finally:
        model.train(was_training)


def collect_probe_probs(image_encoder, classification_head, dataloader, device) -> Predictions:
    """sigmoid(decision_function) of a fitted vlp_amd.metrics.LogisticRegressionFit on the image
    encoder's eval-mode features (sklearn's predict_proba[:, 1] in the reference), on `device`."""
    def prob_fn(batch):
        imgs = batch["x-ray"] if "x-ray" in batch else batch["x-ray-u8"]
        feats = image_encoder(imgs.to(device, non_blocking=True)).float()
        return torch.sigmoid(classification_head.decision_function(feats)).float()

    image_encoder.eval()
    with torch.no_grad():
        return _collect(prob_fn, dataloader)


def fold_rows(fold: int, pred: Predictions) -> List[Tuple[str, str, int, str, float]]:
    """One fold's rows: levels in LEVELS' order, groups by first appearance, metrics in
    subgroup_metrics_from_counts' key order.  One grouped count, one read."""
    n_groups = [len(g) for g in pred.groups]
    counts = metrics.grouped_binary_counts(pred.probs, pred.tumor, pred.codes, n_groups).tolist()
    rows, cell = [], 0
    for level, groups in zip(LEVELS, pred.groups):
        for group in groups:
            tp, fp, fn, tn, wins, ties = counts[cell]
            cell += 1
            for metric, value in metrics.subgroup_metrics_from_counts(tp, fp, fn, tn, 2 * wins + ties).items():
                rows.append((level, group, fold, metric, value))
    return rows


def format_value(v: float) -> str:
    return "NaN" if math.isnan(v) else repr(float(v))


def evaluate_results(output_file: str, predictions_per_fold: Sequence[Predictions]):
    """Write the table `level,group,fold,metric,value` (NaN as `NaN`) for the folds' predictions
    and return its rows as tuples (reference evaluate_results, :120-242)."""
    rows = []
    for fold, pred in enumerate(predictions_per_fold):
        rows.extend(fold_rows(fold, pred))
    parent = os.path.dirname(output_file)
    if parent:
        os.makedirs(parent, exist_ok=True)
    with open(output_file, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(("level", "group", "fold", "metric", "value"))
        for level, group, fold, metric, value in rows:
            w.writerow((level, group, fold, metric, format_value(value)))
    log.info("Test Eval: Saved evaluation results to %s", output_file)
    return rows


def save_predictions(folder: str, predictions_per_fold: Sequence[Predictions]) -> None:
    """predictions_fold_{i}.csv with the reference's columns (one read of the probabilities per fold)."""
    os.makedirs(folder, exist_ok=True)
    for i, pred in enumerate(predictions_per_fold):
        cols = dict(pred.columns, prob=[repr(p) for p in pred.probs.double().tolist()])
        with open(os.path.join(folder, f"predictions_fold_{i}.csv"), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(PREDICTION_COLUMNS)
            w.writerows(zip(*(cols[k] for k in PREDICTION_COLUMNS)))
    log.info("Test Eval: Saved predictions to %s", folder)
