"""Post-fit evaluation of the baseline modules' best checkpoint (reference
src/train.py:179-183 and :261-327, plot_tsne_and_calculate_silhouette.py:15-98,
plot_confusion_matrix.py:14-60): two silhouette scores of the image network's
features (clusters = tumour label, clusters = source dataset) and the 2x2
confusion matrix at a 0.5 threshold, for the validation and the train loaders.

On request (`tsne=True`, the config key `post_fit_tsne`) the 2-D t-SNE of the same
features is computed as well (reference :62-66, sklearn's exact method restated in
vlp_amd.metrics.tsne) and written per split as `tsne_{split}.npz` and, where
matplotlib imports, as the reference's scatter `tsne_{split}.png`.  The W&B
upload of the figures and the confusion-matrix figure are not built.

Each batch goes through the module once (features and logits come from
the same forward); the features stay on the device and the silhouette's distance
sums and the t-SNE run there (vlp_amd/metrics.py -> vlp_cluster_dist_sums,
vlp_tsne_*), only the tumour labels and dataset names are host lists.  There are
no collectives: under data parallelism every rank evaluates the loaders it is given.
"""
from __future__ import annotations

import logging
import os
from typing import Any, Dict, Optional

import numpy as np

import torch

from vlp_amd import metrics

log = logging.getLogger("project")


def best_checkpoint_callback(trainer):
    """The checkpoint callback whose best model is evaluated (train.py:283-296): the
    first one monitoring a `combined` metric, else the last one monitoring a `btxrd`
    metric, else None."""
    callbacks = getattr(trainer, "checkpoint_callbacks", None)
    if callbacks is None:
        callbacks = [cb for cb in getattr(trainer, "callbacks", []) if hasattr(cb, "best_model_path")]
    btxrd = combined = None
    for cb in callbacks:
        monitor = getattr(cb, "monitor", None) or ""
        if "btxrd" in monitor:
            btxrd = cb
        if "combined" in monitor:
            combined = cb
            break
    return combined if combined is not None else btxrd


def _features_and_logits(model, batch):
    """One pass: (features [B, F] or [B, F, h, w], logits [B])."""
    return model.features_and_logits(batch)


def evaluate_split(model, dataloaders, tsne: bool = False) -> Dict[str, Any]:
    """Silhouette scores and confusion matrix of `model` over a loader or a list of loaders.
    With `tsne` also "tsne" ([N, 2] CPU tensor), "tsne_kl" and the "tumor" / "dataset" lists
    its rows follow (perplexity N - 1 below 30 samples, else 30: reference :62-65)."""
    if not isinstance(dataloaders, (list, tuple)):
        dataloaders = [dataloaders]
    was_training = model.training
    model.eval()
    feats, preds, tumor, dataset = [], [], [], []
    try:
        with torch.no_grad():
            for loader in dataloaders:
                for batch in loader:
                    f, logits = _features_and_logits(model, batch)
                    if f.dim() == 4:
                        f = f.mean((2, 3))
                    feats.append(f.float())
                    preds.append(torch.sigmoid(logits.float().flatten()) > 0.5)   # strict, plot_confusion_matrix.py:48
                    tumor.extend(int(t) for t in batch["tumor"].tolist())
                    dataset.extend(batch["dataset"])
    finally:
        model.train(was_training)
    x, pred = torch.cat(feats), torch.cat(preds)
    y = torch.tensor(tumor, dtype=torch.bool, device=pred.device)
    tn, fp = int((~pred & ~y).sum()), int((pred & ~y).sum())
    fn, tp = int((~pred & y).sum()), int((pred & y).sum())
    if len(set(dataset)) < 2:
        log.warning("post_fit_evaluation: the split holds one dataset name only (%s); its dataset silhouette "
                    "score is nan", sorted(set(dataset)))
        by_dataset = float("nan")
    else:
        by_dataset = metrics.silhouette_score(x, dataset)
    out = {"silhouette_score_based_on_tumor": metrics.silhouette_score(x, tumor),
           "silhouette_score_based_on_dataset": by_dataset,
           "confusion_matrix": [[tn, fp], [fn, tp]]}
    if tsne:
        emb, kl = metrics.tsne(x, perplexity=len(tumor) - 1 if len(tumor) < 30 else 30)
        out.update({"tsne": emb.cpu(), "tsne_kl": kl, "tumor": tumor, "dataset": dataset})
    return out


_MARKERS = "oXs^vD"


def save_tsne(res: Dict[str, Any], split: str, out_dir: str) -> None:
    """tsne_{split}.npz (y, tumor, dataset) and, if matplotlib imports, tsne_{split}.png: the
    embedding coloured by dataset, marker by tumour label, both silhouette scores in the corner."""
    os.makedirs(out_dir, exist_ok=True)
    y = res["tsne"].numpy()
    tumor, dataset = np.asarray(res["tumor"]), np.asarray(res["dataset"])
    np.savez(os.path.join(out_dir, f"tsne_{split}.npz"), y=y, tumor=tumor, dataset=dataset)
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        log.info("post_fit_evaluation: matplotlib is not installed; tsne_%s.png is not written", split)
        return
    fig, ax = plt.subplots(figsize=(10, 8))
    colours = plt.get_cmap("tab10")
    for di, name in enumerate(sorted(set(dataset.tolist()))):
        for ti, t in enumerate(sorted(set(tumor.tolist()))):
            sel = (dataset == name) & (tumor == t)
            if sel.any():
                ax.scatter(y[sel, 0], y[sel, 1], s=60, color=colours(di % 10), marker=_MARKERS[ti % len(_MARKERS)],
                           edgecolors="white", linewidths=0.5, label=f"{name}, tumor {t}")
    ax.set_xlabel("tsne-1")
    ax.set_ylabel("tsne-2")
    ax.set_title(f"{split}: t-SNE of features colored by Dataset (color) and Tumor (marker)")
    ax.text(0.99, 0.01,
            f"Silhouette Score Based on Tumor/No Tumor: {res['silhouette_score_based_on_tumor']:.4f}\n"
            f"Silhouette Score Based on Dataset: {res['silhouette_score_based_on_dataset']:.4f}",
            ha="right", va="bottom", transform=ax.transAxes, fontsize=12,
            bbox=dict(facecolor="white", alpha=0.6, edgecolor="gray"))
    ax.legend(bbox_to_anchor=(1.05, 1), loc="upper left")
    fig.tight_layout()
    fig.savefig(os.path.join(out_dir, f"tsne_{split}.png"), dpi=100)
    plt.close(fig)


def post_fit_evaluation(model, datamodule, trainer, tsne: bool = False,
                        out_dir: Optional[str] = None) -> Dict[str, Any]:
    """Reload the best checkpoint and evaluate the validation and train loaders; the
    reference's W&B keys, the confusion matrix as four counts per split.  With `tsne`
    also `tsne_kl_{split}`, and the embedding files of save_tsne in `out_dir` (default:
    the directory of the best checkpoint)."""
    cb = best_checkpoint_callback(trainer)
    if cb is None:
        log.info("Train: No silhouette scores or confusion matrix, since no checkpoint callback monitoring a "
                 "combined or btxrd metric was found.")
        return {}
    path = cb.best_model_path
    if not path or not os.path.exists(path):
        log.warning("Train: the checkpoint callback monitoring %s saved no best model; no post-fit evaluation.",
                    cb.monitor)
        return {}
    log.info("Train: Calculating silhouette scores and confusion matrix of validation and train data with the "
             "best %s model: %s", cb.monitor, path)
    best = type(model).load_from_checkpoint(path, device=model.device)
    out: Dict[str, Any] = {}
    for split, loaders in (("validation", datamodule.val_dataloader()), ("train", datamodule.train_dataloader())):
        res = evaluate_split(best, loaders, tsne=tsne)
        out[f"silhouette_score_based_on_tumor_{split}"] = res["silhouette_score_based_on_tumor"]
        out[f"silhouette_score_based_on_dataset_{split}"] = res["silhouette_score_based_on_dataset"]
        (tn, fp), (fn, tp) = res["confusion_matrix"]
        for k, v in (("tn", tn), ("fp", fp), ("fn", fn), ("tp", tp)):
            out[f"confusion_matrix_{split}/{k}"] = v
        if tsne:
            out[f"tsne_kl_{split}"] = res["tsne_kl"]
            save_tsne(res, split, out_dir or os.path.dirname(path))
    for k, v in out.items():
        log.info("Train: %s = %s", k, v)
    return out
