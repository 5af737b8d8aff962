"""GPU: the five evaluation passes of denoise.py return, bit for bit, what they returned while each of them spelled out its
own reconstruction step, noise draw and accumulator layout: tests/golden/eval_passes_parent.json holds the results of that
commit on seeded networks and inputs (tools/gen_golden_eval_passes.py, which also defines the cases and the calls).  Every
float, the key order, the digests of the returned images, the kernel launches, the host reads and the noise stream's state
after the call are compared with ==: the tests that compare a pass with a flag against the same pass without it would not
see both move together; this file does."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("gen_golden_eval_passes", os.path.join(ROOT, "tools", "gen_golden_eval_passes.py"))
GEN = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GEN)


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "eval_passes_parent.json")) as f:
        return json.load(f)


def test_the_fixture_holds_every_case_and_nothing_else(golden):
    assert set(golden) == set(GEN.CASES)
    assert all(set(rec) == {"keys", "values", "launches", "host_reads", "noise"} for rec in golden.values())


@pytest.mark.parametrize("name", list(GEN.CASES))
def test_the_pass_returns_the_parents_result(golden, name):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    want, got = golden[name], GEN.run_case(name)
    print(name, "launches", got["launches"], "host reads", got["host_reads"], "noise", got["noise"])
    assert got["keys"] == want["keys"], "the keys or their insertion order moved"
    moved = {k: (want["values"][k], got["values"][k]) for k in want["keys"] if got["values"][k] != want["values"][k]}
    assert not moved, f"{name}: (parent, now) {moved}"
    assert got["launches"] == want["launches"], "kernel launches per call"
    assert got["host_reads"] == want["host_reads"], "Tensor.tolist + Tensor.item calls per call"
    assert got["noise"] == want["noise"], "the default noise stream's [seed, iteration counter] after the call"
