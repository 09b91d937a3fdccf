"""Time the optimizer step alone on the ResNet34 + DistilBERT module's arenas, with HIP events:
FusedAdam, FusedAdamW and torch.optim.Adam, each plain and with norm clipping on a pending
accumulator, interleaved and repeated.  Writes every raw value as JSON.

  python tools/adam_step_bench.py --out profiles/fused_adam_ab.json [--only fused_adamw]

"clip+pending": the fused optimizers step on acc + w*g with the norm pass (accumulate() and
the re-binding of p.grad run before the first event and are not timed).  torch accumulates in
p.grad during backward, so its row is clip_grad_norm_ (one host read-back) + step().
The events bracket step() as the Trainer calls it: host launch overhead between the kernels
of one step is inside the interval."""
import argparse
import functools
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vision-language-pretraining-for-bone-tumor-detection_amd")]

from src.models.pretrain.VisionLanguageModule import VisionLanguageModule  # noqa: E402
from vlp_amd.optim import FusedAdamW  # noqa: E402

WARMUP, ITERS, REPEATS = 20, 100, 3
FACTORY = {"fused_adam": (torch.optim.Adam, True), "fused_adamw": (torch.optim.AdamW, True),
           "torch_adam": (torch.optim.Adam, False)}


def build(kind):
    cls, fused = FACTORY[kind]
    m = VisionLanguageModule("resnet34", "distilbert", functools.partial(cls, lr=5e-5, weight_decay=0.2), False, False,
                             512, 768, 128, compute_dtype="bf16", fused_optimizer=fused)
    opt = m.configure_optimizers()["optimizer"]
    arenas = [m._head.arena, m.image_encoder.model.arena, m.text_encoder.model.arena]
    g = torch.Generator(device="cuda").manual_seed(0)
    for a in arenas:
        a.grad.copy_(torch.randn(a.grad.shape, generator=g, device="cuda") * 1e-3)
    views = []
    for tower in (m._head, m.image_encoder.model, m.text_encoder.model):
        for owner, attr, full in tower._param_slots:
            views.append((owner._parameters[attr], tower.arena.gview(full)))
    return m, opt, views


def bind(views):
    for p, g in views:
        p.grad = g


def run(kind, opt, views, mode, iters):
    fused = isinstance(opt, FusedAdamW)
    params = [p for p, _ in views]
    if fused:
        opt.set_gradient_clipping(1.0 if mode == "clip+pending" else None)
    times = []
    for _ in range(iters):
        bind(views)
        if fused and mode == "clip+pending":
            opt.accumulate(0.5, first=True)
            bind(views)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if fused:
            opt.step(w=0.5)
        else:
            if mode == "clip+pending":
                torch.nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()
        b.record()
        times.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in times]      # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default=None, help="one of " + ", ".join(FACTORY))
    args = ap.parse_args()
    kinds = [args.only] if args.only else list(FACTORY)
    built = {k: build(k) for k in kinds}
    n_params = sum(p.numel() for p, _ in built[kinds[0]][2])
    rows = []
    for rep in range(REPEATS):
        for mode in ("plain", "clip+pending"):
            for kind in kinds:          # interleaved: every configuration once per repeat
                _, opt, views = built[kind]
                run(kind, opt, views, mode, WARMUP)
                us = run(kind, opt, views, mode, ITERS)
                rows.append({"optimizer": kind, "mode": mode, "repeat": rep, "median_us": statistics.median(us),
                             "mean_us": statistics.fmean(us), "min_us": min(us), "us": us})
                print(f"{kind:12s} {mode:13s} repeat {rep}: median {rows[-1]['median_us']:.1f} us, "
                      f"mean {rows[-1]['mean_us']:.1f}, min {rows[-1]['min_us']:.1f}", flush=True)
    out = {"what": "optimizer step alone, HIP events around step(), microseconds", "module": "resnet34 + distilbert, bf16",
           "parameters": n_params, "warmup": WARMUP, "iters": ITERS, "repeats": REPEATS,
           "device": torch.cuda.get_device_name(0), "library": os.environ.get("VLP_HIP_LIB", "in-tree"), "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main()
