"""Time vlp_clip_loss_fused_masked against vlp_clip_loss_fused in one process.

The 8-GPU operating point per rank: B = 256, N = 2048, E = 128, caption ids drawn
from 880 values (the reference's caption file).  Both calls are warm;
rounds alternate unmasked / masked blocks of `--block` back-to-back calls between
two events, and the per-call figure is the median over the rounds.

    python tools/time_masked_loss.py --out profiles/masked_loss_timing.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vision-language-pretraining-for-bone-tumor-detection_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--block", type=int, default=20)
    a = ap.parse_args()
    from vlp_amd import ops
    B, N, E, U = 256, 2048, 128, 880
    g = torch.Generator().manual_seed(5)
    ie = torch.nn.functional.normalize(torch.randn(N, E, generator=g)).cuda()
    te = torch.nn.functional.normalize(torch.randn(N, E, generator=g)).cuda()
    cid = torch.randint(0, U, (N,), generator=g).to(torch.int32).cuda()
    ls = torch.tensor([2.6592600], device="cuda")
    gi, gt = torch.empty(N, E, device="cuda"), torch.empty(N, E, device="cuda")
    small = torch.zeros(4, device="cuda")

    def plain():
        ops.clip_loss_fused(B, N, E, 3 * B, ie, te, ls, gi, gt, small[2:3], small[0:2])

    def masked():
        ops.clip_loss_fused_masked(B, N, E, 3 * B, ie, te, ls, cid, gi, gt, small[2:3], small[0:2])

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.block):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.block

    for _ in range(3):
        block(plain)
        block(masked)
    tp, tm = [], []
    for _ in range(a.rounds):
        tp.append(block(plain))
        tm.append(block(masked))
    same = (cid[:, None] == cid[None, :]).sum().item() - N
    res = {"shape": {"B": B, "N": N, "E": E, "unique_ids": U, "offset": 3 * B},
           "dropped_entries_per_row": same / N,
           "unmasked_us": statistics.median(tp), "masked_us": statistics.median(tm),
           "unmasked_us_min_max": [min(tp), max(tp)], "masked_us_min_max": [min(tm), max(tm)],
           "rounds": a.rounds, "calls_per_block": a.block,
           "method": "alternating blocks of back-to-back calls between two events, median of rounds",
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
