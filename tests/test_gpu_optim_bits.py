"""Every output bit of the optimizer step and gradient-norm launches against
tests/golden/optim_bits.json, the digests tests/golden/make_optim_bits.py recorded from the
library of the commit the fixture names (the four step kernels and two norm kernels that
step_kernel and sumsq_kernel of csrc/optim_ops.hip replaced).  The fixture is never regenerated
from the code under test: a kernel change that moves a bit fails here.

Each case's host inputs are digested first: a failure there says that the input generators (or
torch's random streams) changed, not the kernels.  The cases, their inputs and their keys are
the generator's own functions.
"""
import json

import pytest
import torch

from tests.golden import make_optim_bits as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def ops():
    from vlp_amd import ops as o
    return o


@pytest.fixture(scope="module")
def golden():
    with open(G.FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_every_case(golden):
    assert set(golden["step"]) == set(G.LAUNCHES) and set(golden["norm"]) == set(G.NORM_LAUNCHES)
    for launch in G.LAUNCHES:
        assert len(golden["step"][launch]) == len(G.SIZES) * len(G.OFFS) * len(G.WDS) * len(G.BETAS)
    for launch in G.NORM_LAUNCHES:
        assert len(golden["norm"][launch]) == len(G.norm_cases(launch))


@pytest.mark.parametrize("launch", list(G.LAUNCHES))
def test_step_bits(ops, golden, launch):
    want, moved = golden["step"][launch], []
    for n in G.SIZES:
        for offs in G.OFFS:
            host, cv, kin, din = G.step_inputs(launch, n, offs)
            assert din == golden["inputs"][kin], f"inputs changed ({kin}): the kernels were not compared"
            for wd in G.WDS:
                for betas in G.BETAS:
                    key = G.step_key(n, offs, wd, betas)
                    if G.run_step(ops, launch, host, cv, offs, wd, betas) != want[key]:
                        moved.append(key)
    assert not moved, f"kernel changed: {launch} gives other bits than {golden['commit']} in {len(moved)} cases: {moved}"


@pytest.mark.parametrize("launch", G.NORM_LAUNCHES)
def test_norm_partials_bits(ops, golden, launch):
    want, moved = golden["norm"][launch], []
    for n, offs, w in G.norm_cases(launch):
        host, kin, din = G.norm_inputs(launch, n, offs)
        assert din == golden["inputs"][kin], f"inputs changed ({kin}): the kernels were not compared"
        if G.run_norm(ops, launch, host, offs, w) != want[G.norm_key(n, offs, w)]:
            moved.append(G.norm_key(n, offs, w))
    assert not moved, f"kernel changed: {launch} gives other partials than {golden['commit']} in {len(moved)} cases: {moved}"
