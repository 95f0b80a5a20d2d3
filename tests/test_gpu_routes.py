"""-m gpu: the kernels the native plan selects, held against a recording (tests/golden/plan_census.json, made by tools/plan_census.py
before the plan's routing moved into one table).  Per configuration one small training step with the launch census on: the
{kernel variant: launches} dict and the launcher-call count of the step must EQUAL the recording - kernel selection is host logic, no
tolerance applies.  The shapes put dense blocks on both sides of every pixel threshold (B=3 228x304: 12 996 / 3 306 / 855 / 240 pixels;
B=2: dense_e2 at 8 664; B=4: dense_e4 at 1 140); the deterministic configuration also pins the SHA-256 of the flat gradient buffer and of
the logits (that mode promises bit-reproducible gradients)."""
import json
import os
import sys

import pytest
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_census  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLDEN, "plan_census.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def model():
    return plan_census.new_model(torch.device("cuda:0"))


def test_the_recording_covers_every_configuration(gold):
    assert sorted(gold) == sorted(plan_census.CONFIGS)
    assert "grad_sha256" in gold["b3_deterministic"] and "logits_sha256" in gold["b3_deterministic"]


@pytest.mark.parametrize("name", list(plan_census.CONFIGS))
def test_step_launches_the_recorded_kernels(model, gold, name):
    got, want = plan_census.record(model, name), gold[name]
    diff = {k: (got["census"].get(k, 0), want["census"].get(k, 0)) for k in set(got["census"]) | set(want["census"])
            if got["census"].get(k, 0) != want["census"].get(k, 0)}
    assert not diff, "kernel variant: (launched, recorded) %r" % diff
    assert got["launches"] == want["launches"]
    assert got == want                                   # the deterministic configuration: gradient and logits hashes too
