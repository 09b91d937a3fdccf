"""Digests of every output bit of the optimizer step and gradient-norm launches, recorded from
a library whose bits are to be kept (tests/test_gpu_optim_bits.py reruns every case).

Needs a GPU.  Run it with the library of the commit to pin, never with the code under test:

    VLP_HIP_LIB=/path/to/that/libvlp_hip.so python tests/golden/make_optim_bits.py --commit <its commit>

Writes tests/golden/optim_bits.json: sha256 digests only, and the commit they come from.

Step cases: the 12 launches of LAUNCHES at every n of SIZES, offsets of OFFS ((0, 1): operands of
mixed 16-B alignment, the all-scalar path), weight decay of WDS and betas of BETAS, at step 3,
w = 1/3 with an accumulator, coef = 0.25 and the clip value of tests/test_gpu_adam.py::case.  One
digest per case over the raw bytes of p, m, v, g and (where there is one) acc, in that order.
Norm cases: the partials buffer (two NaN entries behind the last partial included) of
vlp_grad_sumsq and vlp_grad_accum_sumsq at every n of NORM_SIZES, the same offsets and w of WS.
Inputs: adam_host / adam_device of tests/test_gpu_grad_accum.py and mixed / on_device of
tests/test_gpu_grad_clip.py; their digests are recorded too, so that a changed generator is
not mistaken for a changed kernel.
"""
import argparse
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (os.path.join(ROOT, "vision-language-pretraining-for-bone-tumor-detection_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tests.test_gpu_adam import COEF, STEP, W_FRESH, case, clip_kw  # noqa: E402
from tests.test_gpu_grad_accum import adam_device  # noqa: E402
from tests.test_gpu_grad_clip import HYP, mixed, on_device  # noqa: E402

FIXTURE = os.path.join(HERE, "optim_bits.json")

SIZES = [1, 3, 4, 5, 1023, 1024 * 256 + 7]
OFFS = [(0, 0), (1, 1), (0, 1)]        # (p / m / v / acc, g) offsets in floats
WDS = [0.01, 0.2]
BETAS = [(0.9, 0.999), (0.875, 0.96875)]
# name -> (entry point of vlp_amd.ops, clip mode, with an accumulator)
LAUNCHES = {
    "adamw": ("adamw", "none", False),
    "adamw_clip-norm": ("adamw_clip", "norm", False),
    "adamw_clip-value": ("adamw_clip", "value", False),
    "adamw_clip_accum-none": ("adamw_clip_accum", "none", True),
    "adamw_clip_accum-norm": ("adamw_clip_accum", "norm", True),
    "adamw_clip_accum-value": ("adamw_clip_accum", "value", True),
    "adam_step-none": ("adam_step", "none", False),
    "adam_step-norm": ("adam_step", "norm", False),
    "adam_step-value": ("adam_step", "value", False),
    "adam_step-acc-none": ("adam_step", "none", True),
    "adam_step-acc-norm": ("adam_step", "norm", True),
    "adam_step-acc-value": ("adam_step", "value", True),
}
NORM_SIZES = [1, 3, 255, 257, 16384, 16385, 65541]
WS = [1.0, 1.0 / 3.0]
NORM_LAUNCHES = ("grad_sumsq", "grad_accum_sumsq")


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def step_key(n, offs, wd, betas):
    return f"n{n} off{offs[0]}{offs[1]} wd{wd} b{betas[0]}"


def step_inputs(launch, n, offs):
    """(host tensors, clip value, the fixture's key of the two, their digest): a function of n,
    the first offset (the seed) and whether there is an accumulator"""
    _, mode, acc = LAUNCHES[launch]
    host, _, cv = case(n, offs, mode, acc)
    key = f"step{'+acc' if acc else ''} n{n} off{offs[0]}"
    return host, cv, key, digest(*host.values(), torch.tensor([cv], dtype=torch.float64))


def run_step(ops, launch, host, cv, offs, wd, betas):
    """One launch on fresh device copies of `host`: the digest of everything it may write."""
    fn, mode, acc = LAUNCHES[launch]
    d = adam_device(host, offs)
    t = (d["p"].v, d["g"].v, d["m"].v, d["v"].v)
    args = (HYP["lr"], betas[0], betas[1], HYP["eps"], wd, STEP)
    kw = clip_kw(mode, cv)
    if acc:
        kw.update(acc=d["a"].v, w=W_FRESH)
    getattr(ops, fn)(*t, *args, **kw)
    torch.cuda.synchronize()
    assert all(x.guards_untouched() for x in d.values()), "wrote outside its span"
    return digest(*(d[k].v for k in ("p", "m", "v", "g", "a") if k in d))


def norm_cases(launch):
    return [(n, offs, w) for n in NORM_SIZES for offs in OFFS for w in (WS if launch == "grad_accum_sumsq" else WS[:1])]


def norm_key(n, offs, w):
    return f"n{n} off{offs[0]}{offs[1]} w{w:.3g}"


def norm_inputs(launch, n, offs):
    if launch == "grad_sumsq":
        host = [mixed(n, n + offs[1])]
    else:
        host = [mixed(n, 17 * n + offs[0]), mixed(n, 19 * n + 2)]
    return host, f"{launch} n{n} off{offs[0]}{offs[1]}", digest(*host)


def run_norm(ops, launch, host, offs, w):
    n = host[0].numel()
    k = ops.grad_sumsq_nparts(n)
    partials = torch.full((k + 2,), float("nan"), dtype=torch.float64, device="cuda")
    if launch == "grad_sumsq":
        wrote = ops.grad_sumsq(on_device(host[0], offs[1]), partials)
    else:
        wrote = ops.grad_accum_sumsq(on_device(host[0], offs[0]), on_device(host[1], offs[1]), w, partials)
    torch.cuda.synchronize()
    assert wrote == k
    return digest(partials)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose library VLP_HIP_LIB names")
    args = ap.parse_args()
    from vlp_amd import ops
    out = {"commit": args.commit, "device": torch.cuda.get_device_name(0),
           "constants": dict(lr=HYP["lr"], eps=HYP["eps"], step=STEP, w=W_FRESH, coef=COEF),
           "inputs": {}, "step": {}, "norm": {}}
    for launch in LAUNCHES:
        rows = out["step"][launch] = {}
        for n, offs in ((n, offs) for n in SIZES for offs in OFFS):
            host, cv, kin, din = step_inputs(launch, n, offs)
            out["inputs"][kin] = din
            for wd, betas in ((wd, betas) for wd in WDS for betas in BETAS):
                rows[step_key(n, offs, wd, betas)] = run_step(ops, launch, host, cv, offs, wd, betas)
    for launch in NORM_LAUNCHES:
        rows = out["norm"][launch] = {}
        for n, offs, w in norm_cases(launch):
            host, kin, din = norm_inputs(launch, n, offs)
            out["inputs"][kin] = din
            rows[norm_key(n, offs, w)] = run_norm(ops, launch, host, offs, w)
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{FIXTURE}: {sum(len(v) for v in out['step'].values())} step cases, "
          f"{sum(len(v) for v in out['norm'].values())} norm cases, library of {out['commit']}")


if __name__ == "__main__":
    main()
