"""The test-set evaluation's counts for the seven levels (overall, dataset, entity, anatomy_site,
sex, age_encoded, age_group), one grouped device op against one accumulator per subgroup, on one GPU.

    python tools/groupmetric_bench.py [--calls 20] [--windows 5] [--out profiles/groupmetric_ab.json]

Per size -- n = 2048 and n = 16384 rows, 36 groups over the seven levels -- two paths produce the
same [cells, 6] integers from the same device tensors:
  grouped       one vlp_amd.metrics.grouped_binary_counts call (csrc/groupmetric_ops.hip: every
                group of every level in one pass over the pairs) and one .tolist()
  per_subgroup  what the code base offered before: per level and group a boolean mask, the masked
                rows into a fresh BinaryMetricsDevice, and its counts() (one pair count, one fold and
                one read-back each; each of the two mask indexes reads its row count back as well)
They run in alternating windows of back-to-back calls after a warm-up, each window timed by the
host clock around the calls (every call ends in a read-back, so the host clock is what an
evaluation waits for); the best of the windows is reported.  One further call of each path runs
under torch.profiler to count its device kernels and memory copies.  The two results are compared
with torch.equal before anything is timed.  Needs an MI355X; there is no CPU path.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vision-language-pretraining-for-bone-tumor-detection_amd")]

SIZES = (2048, 16384)
LEVELS = ("overall", "dataset", "entity", "anatomy_site", "sex", "age_encoded", "age_group")
N_GROUPS = (1, 2, 15, 9, 2, 4, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groupmetric_ab.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("groupmetric_bench needs a GPU")
    from vlp_amd import metrics
    rows = []
    for n in SIZES:
        g = torch.Generator().manual_seed(n)
        # sigmoid outputs of a classifier that is right more often than not; every row is in a group
        y = (torch.rand(n, generator=g) < 0.4).to(torch.uint8)
        s = torch.sigmoid(1.5 * (2.0 * y.float() - 1.0) * torch.rand(n, generator=g) + torch.randn(n, generator=g))
        codes = torch.stack([torch.randint(0, G, (n,), generator=g) for G in N_GROUPS]).to(torch.uint8)
        s, y, codes = s.cuda(), y.cuda(), codes.cuda()

        def grouped():
            return metrics.grouped_binary_counts(s, y, codes, N_GROUPS).tolist()

        def per_subgroup():
            out = []
            for l, G in enumerate(N_GROUPS):
                for grp in range(G):
                    m = codes[l] == grp
                    acc = metrics.BinaryMetricsDevice(capacity=n)
                    acc.update(s[m], y[m])
                    out.append(acc.counts())
            return out

        paths = {"grouped": grouped, "per_subgroup": per_subgroup}
        assert grouped() == per_subgroup(), "the two paths disagree"
        row = {"n": n, "cells": sum(N_GROUPS), "identical_counts": True}
        for name, fn in paths.items():
            for _ in range(3):
                fn()
            row[name] = {"ms_per_call_host_clock": []}
        for _ in range(a.windows):
            for name, fn in paths.items():
                torch.cuda.synchronize()
                h0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                torch.cuda.synchronize()
                row[name]["ms_per_call_host_clock"].append(round((time.perf_counter() - h0) * 1e3 / a.calls, 4))
        for name, fn in paths.items():
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    fn()
                    torch.cuda.synchronize()
                dev_events = [e for e in prof.events() if getattr(e, "device_type", None) is not None
                              and "cuda" in str(e.device_type).lower()]
                copies = [e for e in dev_events if "memcpy" in e.name.lower()]
                d2h = [e for e in copies if "dtoh" in e.name.lower().replace(" ", "").replace("->", "to")
                       or "devicetohost" in e.name.lower().replace(" ", "")]
                row[name]["device_kernels_per_call"] = len(dev_events) - len(copies)
                row[name]["device_memcpys_per_call"] = len(copies)
                row[name]["device_to_host_copies_per_call"] = len(d2h)
            except Exception as e:   # the profiler is optional plumbing: say so, keep the times
                row[name]["device_kernels_per_call"] = f"not measured ({type(e).__name__}: {e})"
        row["grouped"]["launches_by_construction"] = 2
        row["grouped"]["read_backs_by_construction"] = 1
        row["per_subgroup"]["read_backs_by_construction"] = (f"{3 * sum(N_GROUPS)} (per group: two mask indexes' row "
                                                             f"counts and the accumulator's 48 bytes)")
        row["best_ms_host_clock"] = {k: min(row[k]["ms_per_call_host_clock"]) for k in paths}
        rows.append(row)
        print(json.dumps(row))
    res = {"what": "counts of the test-set evaluation's seven levels: one grouped op vs one BinaryMetricsDevice per "
                   "subgroup, MI355X", "levels": dict(zip(LEVELS, N_GROUPS)), "calls_per_window": a.calls,
           "windows": a.windows,
           "order": "alternating windows grouped, per_subgroup, ... on the same tensors after 3 warm-up calls each",
           "sizes": rows,
           "not_touched": "the training steps and bench.py's headline do not run this code; not re-measured"}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
