"""host/options.hpp without a GPU, through tests/helpers/options_check.cpp built with -fsanitize=address,undefined: every
command line of tests/cli_refusal_cases.py is refused with the words and the status that the binary gave before its rules
became a table (tests/golden/cli_refusals.json), and no rule refuses a command line of every mode."""
import json
import os
import subprocess

import pytest

import cli_refusal_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "cli_refusals.json")) as f:
    RECORDED = json.load(f)


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    d = tmp_path_factory.mktemp("options_check")
    exe = str(d / "options_check_san")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "host"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "helpers", "options_check.cpp"), "-lz"], check=True)
    rc.write_files(str(d))

    def run(c):
        return rc.first_line_and_status([exe, *map(str, rc.where(c)), "miekki", *c["args"]], c, str(d))
    return run


def test_the_record_holds_every_case():
    assert sorted(RECORDED) == sorted(c["name"] for c in rc.CASES)
    assert len(RECORDED) == len(rc.CASES) >= 50
    assert all(r["status"] == 1 for r in RECORDED.values())


@pytest.mark.parametrize("c", rc.CASES, ids=lambda c: c["name"])
def test_refusal_is_the_recorded_one(tool, c):
    assert tool(c) == RECORDED[c["name"]]


@pytest.mark.parametrize("c", rc.ACCEPTED, ids=lambda c: c["name"])
def test_accepted_command_line_is_not_refused(tool, c):
    assert tool(c) == {"line": "", "status": 0}
