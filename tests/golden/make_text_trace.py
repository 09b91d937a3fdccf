"""The text towers' kernel-launch sequence per configuration, and their state-dict / arena layout,
recorded on the CPU from towers whose launches are to be kept (tests/test_text_trace_cpu.py reruns
every configuration).

Needs no GPU and no built library (the text towers call no host predicate, so nothing runs).  Run
it on the commit to pin, never on the code under test:

    python tests/golden/make_text_trace.py --commit <that commit>

Writes tests/golden/text_launch_trace.json:
  "traces": per configuration one line per `ops.<name>(...)` call the tower's drivers make, in
    order, in make_tower_trace.Recorder's format (tensors named by identity, optional parameters
    logged where they differ from the default).  The recorder stands in for the `ops` attribute
    of the module that defines the tower's run_forward (vlp_amd.tinybert when this was recorded).
    On top of Recorder, a tensor that is entirely zero at its first appearance is marked `=0`.
    During a trace torch.empty returns buffers filled with a non-zero sentinel, so the mark
    tells a torch.zeros buffer from a torch.empty one: the CLS-only backward is only correct
    because dctx and the scattered ds1 addend start as zeros.  (Zero biases and the zeroed
    gradient arena carry the mark too; the weights, LayerNorm gains and inputs do not.)
  "layouts": per tower list(state_dict().keys()) and [(name, offset, numel)] of arena.layout, at
    the default full-size TinyBERT and at the small DistilBERT the traces use.
"""
import argparse
import contextlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.golden.make_tower_trace import Recorder  # noqa: E402  (it puts the package on sys.path)

FIXTURE = os.path.join(HERE, "text_launch_trace.json")
B, TN = 2, 8
SENTINEL = 3.0


class ZeroMarkRecorder(Recorder):
    """Recorder that marks a tensor `=0` where it first appears if every element is zero."""

    def _tensor(self, t):
        s = super()._tensor(t)
        first = ":" in s
        return s + "=0" if first and t.numel() and not torch.count_nonzero(t) else s


@contextlib.contextmanager
def sentinel_empty():
    """torch.empty hands out SENTINEL-filled buffers, so `=0` can only mean torch.zeros."""
    real = torch.empty

    def empty(*a, **kw):
        return real(*a, **kw).fill_(SENTINEL)
    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


def _cfg(tower, dtype, cls_only, training=True, mask=True, tt=True, steps=1):
    return {"tower": tower, "dtype": dtype, "cls_only": cls_only, "training": training, "mask": mask, "tt": tt,
            "steps": steps}


def configs():
    """Per tower and per cls_only: both dtypes, training / eval, attention_mask and token_type_ids
    given / None, and the second of two steps on a kept tower."""
    c = {}
    for tower in ("tinybert", "distilbert"):
        for cls_only in (False, True):
            pre = f"{tower}-{'cls' if cls_only else 'full'}-"
            c[pre + "bf16-train-mask-tt"] = _cfg(tower, "bf16", cls_only)
            c[pre + "fp32-eval-nomask-nott"] = _cfg(tower, "fp32", cls_only, training=False, mask=False, tt=False)
            c[pre + "bf16-train-mask-nott-step2"] = _cfg(tower, "bf16", cls_only, tt=False, steps=2)
            c[pre + "fp32-train-nomask-tt"] = _cfg(tower, "fp32", cls_only, mask=False)
    return c


def small_tower(kind, dtype="fp32"):
    """The towers the traces run: 2 layers, so cls_only runs one full layer and one CLS layer."""
    if kind == "tinybert":
        from vlp_amd.tinybert import TinyBertConfig, TinyBertTower
        cfg = TinyBertConfig(0.1, 0.1)
        cfg.vocab_size, cfg.max_pos, cfg.type_vocab, cfg.layers = 50, 16, 2, 2   # hidden 312, 12 heads, ffn 1200
        return TinyBertTower(cfg, compute_dtype=dtype, device="cpu")
    from vlp_amd.distilbert import DistilBertConfig, DistilBertTower
    cfg = DistilBertConfig(0.1, 0.1, hidden=64, layers=2, heads=2, ffn=128, vocab_size=50, max_pos=16)
    return DistilBertTower(cfg, compute_dtype=dtype, device="cpu")


_TOWERS = {}


def _tower(kind, dtype):
    if (kind, dtype) not in _TOWERS:
        _TOWERS[kind, dtype] = small_tower(kind, dtype)
    return _TOWERS[kind, dtype]


def trace(cfg):
    """The launch lines of one configuration (of its last step), from a fresh workspace and seed."""
    from vlp_amd import ops
    tower = _tower(cfg["tower"], cfg["dtype"])
    mod = sys.modules[type(tower).run_forward.__module__]   # the module whose `ops` the drivers call
    tower._ws, tower._seed = {}, 0x5EED
    ids = (torch.arange(B * TN) % tower.cfg.vocab_size).view(B, TN)
    mask = tt = None
    if cfg["mask"]:
        mask = torch.ones(B, TN, dtype=torch.long)
        mask[:, TN - 2:] = 0
    if cfg["tt"]:
        tt = torch.zeros(B, TN, dtype=torch.long)
        tt[:, TN // 2:] = 1
    dcls = torch.full((B, tower.cfg.hidden), 0.01)
    try:
        with sentinel_empty():
            for _ in range(cfg["steps"]):
                rec = mod.ops = ZeroMarkRecorder(ops)
                h, sv = tower.run_forward(ids, mask, tt, cfg["training"], cls_only=cfg["cls_only"])
                tower.run_backward(sv, dcls)
    finally:
        mod.ops = ops
        tower._ws = {}
    return rec.lines


def layouts():
    from vlp_amd.tinybert import TinyBertTower
    out = {}
    for name, t in (("tinybert", TinyBertTower(device="cpu")), ("distilbert-small", small_tower("distilbert"))):
        out[name] = {"keys": list(t.state_dict().keys()),
                     "layout": [[k, v[0], v[1]] for k, v in t.arena.layout.items()]}
    return out


def write_fixture(res, path):
    """One line per call, per state-dict key and per arena entry."""
    def block(d):
        return ",\n".join(json.dumps(k) + ": [\n" + ",\n".join(json.dumps(l) for l in v) + "\n]" for k, v in d.items())
    lay = ",\n".join(json.dumps(k) + ": {\n" + block(v) + "\n}" for k, v in res["layouts"].items())
    with open(path, "w") as f:
        f.write('{"commit": ' + json.dumps(res["commit"]) + ', "traces": {\n' + block(res["traces"])
                + '\n}, "layouts": {\n' + lay + "\n}}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose text towers are recorded")
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    res = {"commit": args.commit, "traces": {name: trace(cfg) for name, cfg in configs().items()},
           "layouts": layouts()}
    write_fixture(res, args.out)
    print(f"{args.out}: " + ", ".join(f"{k} {len(v)}" for k, v in res["traces"].items()))


if __name__ == "__main__":
    main()
