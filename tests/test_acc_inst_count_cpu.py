"""The MSM accumulation's hot loop, counted statically (tools/acc_inst_count.py).

msm_acc_kernel's time is its instruction count (DESIGN, "The accumulation's issue cost"), so
the count is held like a bound: the kernel is cross-compiled for gfx950 with the library's
flags and its hot loop must keep four waves per SIMD without scratch, the 1487 wide
multiplies of 8M + 2S under ten reductions, and no more other vector instructions than
the "after" column of DESIGN's table records.
"""
import json
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "tools", "acc_inst_count.py")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def counts():
    if not os.path.exists(os.environ.get("HIPCC", HIPCC)):
        pytest.skip("hipcc not found")
    out = subprocess.run([sys.executable, TOOL, "--json"], check=True, capture_output=True, text=True).stdout
    return json.loads(out)


def _design_row(name):
    """(before, after) of the row `| name | before | after |` in DESIGN's count table"""
    with open(os.path.join(REPO, "DESIGN.md")) as f:
        m = re.search(r"^\|\s*%s\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|" % re.escape(name), f.read(), re.M)
    assert m, f"DESIGN.md has no count-table row {name!r}"
    return int(m.group(1)), int(m.group(2))


def test_hot_loop_keeps_its_occupancy_and_its_multiply_floor(counts):
    assert counts["ScratchSize"] == 0
    assert counts["NumVgprs"] <= 128
    assert counts["Occupancy"] >= 4
    assert counts["mad"] <= 1487


def test_other_valu_count_is_no_higher_than_design_records(counts):
    before, after = _design_row("other VALU")
    assert before == 1021
    assert after <= before - 180
    assert counts["other"] <= after, (counts["other"], counts["by_mnemonic"])
    assert counts["valu"] == counts["mad"] + counts["other"]

