"""The baselines' loss section (FusionModule._compute_loss: weighted BCE + lambda CORAL), torch
path against the on-device op (`loss_on_device`, csrc/domain_loss_ops.hip), on one GPU.

    python tools/domain_loss_bench.py [--calls 200] [--windows 5] [--coral-lambda 1000]
                                      [--fusion-off F --fusion-on F] [--out profiles/domain_loss_ab.json]

Per shape -- N = 64 and N = 512 at D = 512 with forward + backward, N = 4096 at D = 512 under
no_grad (the epoch-end combined validation loss) -- the two paths run in alternating windows of
back-to-back calls on the same device tensors after a warm-up.  Each window is timed twice: by
device events (the stream's time from the first launch to the last kernel's end) and by the host
clock around the window and a final synchronise (what a training loop waits for: the torch path
reads the two domain counts back in every call, the device op reads nothing).  One further call of
each path runs under torch.profiler to count its device kernels and memory copies.  The accuracy
of both paths against the fp64 closed form on the CPU is recorded beside the times.

--fusion-off / --fusion-on name the JSON lines of two tools/fusion_bench.py runs (flag off, flag
on) to store in the same file.  Needs an MI355X; there is no CPU path.
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vision-language-pretraining-for-bone-tumor-detection_amd")]

SHAPES = ((64, 512, True), (512, 512, True), (4096, 512, False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--coral-lambda", type=float, default=1000.0)
    ap.add_argument("--fusion-off", default="")
    ap.add_argument("--fusion-on", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "domain_loss_ab.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("domain_loss_bench needs a GPU")
    from src.models.baseline.FusionModule import FusionModule
    from tests.domain_loss_ref import codes_of, domain_loss_ref
    lam, lw = a.coral_lambda, torch.tensor([0.7, 2.0])
    selfs = {name: types.SimpleNamespace(label_weights=lw, hparams=types.SimpleNamespace(
        coral_lambda=lam, loss_on_device=flag)) for name, flag in (("torch", False), ("device", True))}
    rows = []
    for N, D, grad in SHAPES:
        g = torch.Generator().manual_seed(N)
        # pooled ResNet34 features are non-negative (ReLU, then the mean) and of order 1
        x = torch.randn(N, D, generator=g).abs()
        z, y = torch.randn(N, generator=g), torch.randint(0, 2, (N,), generator=g)
        dataset = ["INTERNAL" if i % 3 else "BTXRD" for i in range(N)]
        feats = x.cuda()[:, :, None, None].requires_grad_(grad)
        logits, labels = z.cuda().requires_grad_(grad), y.cuda()

        def call(name):
            feats.grad = logits.grad = None
            if grad:
                out = FusionModule._compute_loss(selfs[name], feats, logits, labels, dataset)
                out[0].backward()
            else:
                with torch.no_grad():
                    out = FusionModule._compute_loss(selfs[name], feats, logits, labels, dataset)
            return out

        ref = domain_loss_ref(x, z, y, codes_of(dataset), float(lw[0]), float(lw[1]), lam)
        row = {"N": N, "D": D, "backward": grad, "coral_fp64": ref["coral"].item()}
        for name in selfs:
            for _ in range(10):
                out = call(name)
            torch.cuda.synchronize()
            acc = {"coral_rel_err": abs(out[2].item() - ref["coral"].item()) / ref["coral"].item(),
                   "cls_rel_err": abs(out[1].item() - ref["cls"].item()) / ref["cls"].item()}
            if grad:
                gr = ref["g_feat"]
                acc["grad_feat_rel_l2"] = ((feats.grad.double().cpu()[:, :, 0, 0] - gr).norm() / gr.norm()).item()
            row[name] = {"accuracy_vs_fp64": {k: float(f"{v:.3e}") for k, v in acc.items()},
                         "ms_per_call_device_events": [], "ms_per_call_host_clock": []}
        for _ in range(a.windows):
            for name in selfs:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                h0 = time.perf_counter()
                t0.record()
                for _ in range(a.calls):
                    call(name)
                t1.record()
                torch.cuda.synchronize()
                h1 = time.perf_counter()
                row[name]["ms_per_call_device_events"].append(round(t0.elapsed_time(t1) / a.calls, 4))
                row[name]["ms_per_call_host_clock"].append(round((h1 - h0) * 1e3 / a.calls, 4))
        for name in selfs:
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    call(name)
                    torch.cuda.synchronize()
                dev_events = [e for e in prof.events() if getattr(e, "device_type", None) is not None
                              and "cuda" in str(e.device_type).lower()]
                copies = [e for e in dev_events if "memcpy" in e.name.lower() or "copy" in e.name.lower()
                          and "kernel" not in e.name.lower()]
                row[name]["device_kernels_per_call"] = len(dev_events) - len(copies)
                row[name]["device_memcpys_per_call"] = len(copies)
            except Exception as e:   # the profiler is optional plumbing: say so, keep the times
                row[name]["device_kernels_per_call"] = f"not measured ({type(e).__name__}: {e})"
        row["best_ms_host_clock"] = {n: min(row[n]["ms_per_call_host_clock"]) for n in selfs}
        row["best_ms_device_events"] = {n: min(row[n]["ms_per_call_device_events"]) for n in selfs}
        rows.append(row)
        print(json.dumps(row))
    res = {"what": "FusionModule._compute_loss (weighted BCE + CORAL), torch path vs loss_on_device, MI355X",
           "coral_lambda": lam, "label_weights": lw.tolist(), "calls_per_window": a.calls, "windows": a.windows,
           "order": "alternating windows torch, device, ... on the same tensors after 10 warm-up calls each",
           "shapes": rows,
           "not_touched": "the pretraining step and bench.py's headline do not run this code; not re-measured"}
    for key, path in (("fusion_bench_loss_on_device_off", a.fusion_off), ("fusion_bench_loss_on_device_on", a.fusion_on)):
        if path:
            with open(path) as f:
                res[key] = json.loads(f.read().strip().splitlines()[-1])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
