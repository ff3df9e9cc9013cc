"""The table of tests/cli_refusal_cases.py through the real binary: the first stdout line and the exit status of every
refused command line are the recorded ones (tests/golden/cli_refusals.json).  No case touches a device."""
import json
import os

import pytest

import cli_refusal_cases as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binary_refuses_as_recorded():
    with open(os.path.join(ROOT, "tests", "golden", "cli_refusals.json")) as f:
        recorded = json.load(f)
    got = rc.record(os.path.join(ROOT, "miekki_amd", "miekki"))
    for name in recorded:
        assert got[name] == recorded[name], name
    assert sorted(got) == sorted(recorded)
