"""Evaluate a pretrained VisionLanguageModule with one linear probe per fold on the held-out
test set (reference scripts/linear_probe_test_eval_downstream.py):

    python scripts/linear_probe_test_eval_downstream.py OUTPUT_FILE VLP_CKPT [--folds K]
                                                        [--save-predictions DIR]

Per fold the image encoder's eval-mode features of the fold's train loader and of its two
validation loaders (concatenated) are extracted on the device, as LinearProbeCallback does;
vlp_amd.metrics.logistic_regression(C=1.0, max_iter=1000) is fitted there; the validation accuracy
and AUROC are logged with their mean +- std over the folds; the test probabilities are
sigmoid(decision_function) on the device, and the same table as test_eval_downstream.py's is
written.  sklearn is not imported.
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
from typing import List, Optional

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))

import torch  # noqa: E402

from scripts.test_eval_downstream import add_data_arguments, data_module  # noqa: E402
from src.utils import test_evaluation as te  # noqa: E402
from src.utils.LinearProbeCallback import LinearProbeCallback  # noqa: E402
from vlp_amd import metrics  # noqa: E402

logger = logging.getLogger("project")


def train_linear_probes_k_fold(image_encoder, dm, device):
    """([fit per fold], validation accuracies, validation AUROCs) over dm.get_cv_splits()."""
    heads, accs, aurocs = [], [], []
    for folds, _ in dm.get_cv_splits():
        probe = LinearProbeCallback(folds.train_dataloader(), folds.val_dataloader(), fit="device")
        x_train, y_train = probe._extract_features_device(image_encoder, probe.train_dataloader, device)
        x_val, y_val = probe._extract_features_device(image_encoder, probe.val_dataloader, device)
        clf = metrics.logistic_regression(x_train, y_train, C=1.0, max_iter=1000)
        if not clf.converged_:
            logger.warning("Linear Probe Test Eval: the fit of fold %d stopped at its iteration limit", len(heads))
        scores = clf.decision_function(x_val)
        heads.append(clf)
        accs.append(float(((scores > 0).long() == y_val.long()).double().mean()))
        aurocs.append(metrics.binary_auroc(y_val, torch.sigmoid(scores)))
    return heads, accs, aurocs


def _mean_std(v):
    t = torch.tensor(v, dtype=torch.float64)
    return float(t.mean()), float(t.std(unbiased=False))


def main(argv: Optional[List[str]] = None):
    parser = argparse.ArgumentParser(description="Fit one linear probe per fold on a pretrained image encoder and "
                                     "evaluate it on the test set, as (level, group, fold, metric, value).")
    parser.add_argument("output_file", type=str)
    parser.add_argument("checkpoint", type=str, help="A VisionLanguageModule checkpoint.")
    parser.add_argument("--folds", type=int, default=4)
    parser.add_argument("--n-samples", type=int, default=512, help="Rows of a synthetic training fold.")
    parser.add_argument("--n-val-samples", type=int, default=64, help="Rows per synthetic validation dataset.")
    add_data_arguments(parser)
    args = parser.parse_args(argv)
    from src.models.pretrain.VisionLanguageModule import VisionLanguageModule
    device = torch.device(args.device or ("cuda" if torch.cuda.is_available() else "cpu"))
    dm = data_module(args, n_folds=args.folds, n_samples=args.n_samples, n_val_samples=args.n_val_samples)
    module = VisionLanguageModule.load_from_checkpoint(args.checkpoint, device=device)
    module.eval()
    encoder = module.image_encoder
    heads, accs, aurocs = train_linear_probes_k_fold(encoder, dm, device)
    logger.info("Linear Probe Test Eval: validation accuracies %s and AUROCs %s", accs, aurocs)
    logger.info("Linear Probe Test Eval: Mean validation accuracy: %s +- %s", *_mean_std(accs))
    logger.info("Linear Probe Test Eval: Mean validation AUROC: %s +- %s", *_mean_std(aurocs))
    predictions = [te.collect_probe_probs(encoder, clf, dm.test_dataloader(fold), device)
                   for fold, clf in enumerate(heads)]
    if args.save_predictions:
        te.save_predictions(args.save_predictions, predictions)
    return te.evaluate_results(args.output_file, predictions)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
