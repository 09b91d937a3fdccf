"""Evaluate the baselines' best checkpoints on the held-out test set (reference
scripts/test_eval_downstream.py):

    python scripts/test_eval_downstream.py OUTPUT_FILE CKPT [CKPT ...] [--save-predictions DIR]

One checkpoint per fold, in fold order; each is loaded as an OnlyImagingModule, else as a
FusionModule, run over DownstreamDataModule.test_dataloader(fold), and the table of
(level, group, fold, metric, value) is written to OUTPUT_FILE (src/utils/test_evaluation.py).
The arguments are checkpoint paths: the reference's W&B run-id lookup is not built, nor is
--save-failures.
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
from typing import List, Optional

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))

import torch  # noqa: E402

from src.data.DownstreamDataModule import DownstreamDataModule  # noqa: E402
from src.utils import test_evaluation as te  # noqa: E402

logger = logging.getLogger("project")


def load_model(path: str, device):
    from src.models.baseline.FusionModule import FusionModule
    from src.models.baseline.OnlyImagingModule import OnlyImagingModule
    try:
        return OnlyImagingModule.load_from_checkpoint(path, device=device)
    except Exception as e:   # not an OnlyImagingModule checkpoint
        try:
            return FusionModule.load_from_checkpoint(path, device=device)
        except Exception as e2:
            raise RuntimeError(f"Failed to load model from checkpoint {path}: {e}, {e2}") from e2


def add_data_arguments(parser: argparse.ArgumentParser) -> None:
    parser.add_argument("--batch-size", type=int, default=128)
    parser.add_argument("--image-size", type=int, default=224)
    parser.add_argument("--num-workers", type=int, default=2)
    parser.add_argument("--n-test-samples", type=int, default=128, help="Rows per synthetic test dataset.")
    parser.add_argument("--try-with-only-n-samples", type=int, default=None)
    parser.add_argument("--device", type=str, default=None, help="Default: cuda if available.")
    parser.add_argument("--save-predictions", type=str, default=None,
                        help="Folder for predictions_fold_{i}.csv; not written when absent.")


def data_module(args, **kwargs) -> DownstreamDataModule:
    return DownstreamDataModule(using_crops=False, batch_size=args.batch_size, num_workers=args.num_workers,
                                image_size=args.image_size, n_test_samples=args.n_test_samples,
                                try_with_only_n_samples=args.try_with_only_n_samples, **kwargs)


def main(argv: Optional[List[str]] = None):
    parser = argparse.ArgumentParser(description="Evaluate one baseline checkpoint per fold on the test set: six "
                                     "metrics overall and per dataset, entity, anatomy_site, sex, age_encoded and "
                                     "age_group, as (level, group, fold, metric, value).")
    parser.add_argument("output_file", type=str)
    parser.add_argument("checkpoints", nargs="+", type=str, help="One checkpoint per fold, in fold order.")
    add_data_arguments(parser)
    args = parser.parse_args(argv)
    device = torch.device(args.device or ("cuda" if torch.cuda.is_available() else "cpu"))
    dm = data_module(args)
    predictions = []
    for fold, path in enumerate(args.checkpoints):
        logger.info("Test Eval: Evaluating model checkpoint: %d/%d - %s", fold + 1, len(args.checkpoints), path)
        model = load_model(path, device)
        predictions.append(te.collect_probs(model, dm.test_dataloader(fold)))
    if args.save_predictions:
        te.save_predictions(args.save_predictions, predictions)
    return te.evaluate_results(args.output_file, predictions)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main()
