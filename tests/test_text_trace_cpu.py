"""CPU: the text towers launch the same kernels, in the same order, on the same buffers, and keep
their state-dict keys and arena offsets.

The host side of TinyBertTower and DistilBertTower decides which linear / attention / LayerNorm /
embedding kernel runs and what each operand is.  Every launch goes through the driver module's
attribute `ops`, so with a recorder in that place (tests/golden/make_text_trace.py: every call
logged with its tensors named by identity, nothing run) a tower constructed on the CPU yields its
whole launch sequence without a device or the built library.  tests/golden/text_launch_trace.json
holds that sequence per configuration, recorded before the four copies of the encoder layer became
one forward and one backward driver; the fixture is never regenerated, so any difference is a
change of behaviour in the towers.

Configurations (B = 2, T = 8, 2 layers; TinyBERT 312 / 12 heads / 1200, DistilBERT 64 / 2 heads /
128): for each tower, with the full last layer and with the CLS-only one -- bf16 training (dropout
0.1 / 0.1) with attention mask and token types, the second of two such steps without token types
(seed advanced, cast target cached), fp32 eval with neither, and fp32 training with token types
only.  Every trace includes the backward.  A tensor that is all zero when first seen carries `=0`
while torch.empty hands out non-zero buffers, so a zero-filled buffer turned into an
uninitialised one (the CLS backward's dctx and ds1 addend) changes the trace.
"""
import json
import re

import pytest

from tests.golden import make_text_trace as G

CONFIGS = G.configs()


@pytest.fixture(scope="module")
def golden():
    with open(G.FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_configuration(golden):
    assert set(golden["traces"]) == set(CONFIGS)
    need = {"dtype": {"bf16", "fp32"}, "training": {True, False}, "mask": {True, False}, "tt": {True, False},
            "steps": {1, 2}}
    for tower in ("tinybert", "distilbert"):
        for cls_only in (False, True):
            sel = [c for c in CONFIGS.values() if c["tower"] == tower and c["cls_only"] == cls_only]
            for k, vals in need.items():
                assert {c[k] for c in sel} == vals, (tower, cls_only, k)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_launch_trace_is_unchanged(golden, name):
    got, want = G.trace(CONFIGS[name]), golden["traces"][name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: call {i} differs\n  now:      {g}\n  recorded: {w}"
    assert len(got) == len(want), f"{name}: {len(got)} calls, {len(want)} recorded"


def test_zero_filled_buffers_are_marked(golden):
    """The recorded CLS backward shows its two zero-filled buffers, and no activation buffer from
    torch.empty is ever marked."""
    lines = golden["traces"]["tinybert-cls-bf16-train-mask-tt"]
    dctx = [l for l in lines if l.startswith("linear_dgrad(") and "lddx=" in l]
    scat = [l for l in lines if l.startswith("scatter_rows(")]
    assert len(dctx) == 1 and "bf16[16,312]=0,2,312,312,lddx=2496" in dctx[0]
    assert len(scat) == 1 and "bf16[16,312]=0,2,312,312,2496" in scat[0]
    assert len(re.findall(r"bf16\[[\d,]+\]=0", "\n".join(lines))) == 2


def test_state_dict_keys_and_arena_layout_are_unchanged(golden):
    got = G.layouts()
    assert set(got) == set(golden["layouts"])
    for name, want in golden["layouts"].items():
        assert got[name]["keys"] == want["keys"], name
        assert got[name]["layout"] == want["layout"], name
