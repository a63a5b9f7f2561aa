"""The NTT kernels, counted statically (tools/ntt_inst_count.py).

The passes are bound by instruction issue (DESIGN, "The F29 product as one asm block; the
NTT's in-register lane exchange"), so what they execute is held like a bound: ntt.hip is
cross-compiled for gfx950 with the library's flags; the persistent 6-bit pass must exchange
lanes without LDS, stay out of scratch and execute no more vector instructions than the
count fixed here (which DESIGN's table must state too); no kernel may run at fewer waves per
SIMD than before the block products; and no lane swap may read a register that an asm statement wrote fewer than two wait states earlier
(the compiler pads that hazard only for its own instructions).
"""
import json
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(REPO, "tools", "ntt_inst_count.py")
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, os.path.join(REPO, "tools"))

# static VALU count of ntt_pass29p_kernel<6>: before the block products, and the bound since
VALU_BEFORE, VALU_BOUND = 7748, 7320

# waves per SIMD of every NTT pass kernel before the block products (the C++ product forms
# and the ds_bpermute exchange)
OCCUPANCY_BEFORE = {
    "ntt_pass29_kernel<3,true>": 3, "ntt_pass29_kernel<4,true>": 4, "ntt_pass29_kernel<5,true>": 3,
    "ntt_pass29_kernel<6,true>": 4, "ntt_pass29_kernel<3,false>": 3, "ntt_pass29_kernel<4,false>": 4,
    "ntt_pass29_kernel<5,false>": 3, "ntt_pass29_kernel<6,false>": 4,
    "ntt_pass29p_kernel<3>": 2, "ntt_pass29p_kernel<4>": 2, "ntt_pass29p_kernel<5>": 2, "ntt_pass29p_kernel<6>": 2,
    "ntt_last29_kernel<true,true>": 2, "ntt_last29_kernel<true,false>": 2,
    "ntt_last29_kernel<false,true>": 3, "ntt_last29_kernel<false,false>": 3,
    "ntt_first_sparse29_kernel": 5,
}


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(os.environ.get("HIPCC", HIPCC)):
        pytest.skip("hipcc not found")
    out = subprocess.run([sys.executable, TOOL, "--json"], check=True, capture_output=True, text=True).stdout
    return json.loads(out)


def _design_row(name):
    """(before, after) of the row `| name | before | after |` in DESIGN's NTT count table"""
    with open(os.path.join(REPO, "DESIGN.md")) as f:
        m = re.search(r"^\|\s*%s\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|" % re.escape(name), f.read(), re.M)
    assert m, f"DESIGN.md has no count-table row {name!r}"
    return int(m.group(1)), int(m.group(2))


def test_persistent_pass_exchanges_in_registers_and_holds_its_count(report):
    k = report["kernels"]["ntt_pass29p_kernel<6>"]
    assert k["ds_bpermute"] == 0
    assert k["ScratchSize"] == 0
    assert k["valu"] <= VALU_BOUND, (k["valu"], k["by_mnemonic"])
    assert _design_row("VALU of `ntt_pass29p_kernel<6>`") == (VALU_BEFORE, VALU_BOUND)


def test_no_kernel_spills_or_loses_occupancy(report):
    ks = report["kernels"]
    assert set(OCCUPANCY_BEFORE) <= set(ks), set(OCCUPANCY_BEFORE) - set(ks)
    for name, occ in OCCUPANCY_BEFORE.items():
        assert ks[name]["Occupancy"] >= occ, (name, ks[name])
        assert ks[name]["ScratchSize"] == 0, (name, ks[name])
        assert ks[name]["ds_bpermute"] == 0, name


def test_no_lane_swap_reads_a_fresh_asm_write(report):
    assert report["swap_hazards"] == []


def test_the_hazard_scan_sees_a_violation():
    import ntt_inst_count as N
    block = "\t;;#ASMSTART\n\tv_and_b32 v7, s2, v2\n\tv_lshrrev_b64 v[2:3], 29, v[2:3]\n\tv_mov_b32 v9, v2\n\t;;#ASMEND\n"
    assert N.swap_hazards(block + "\tv_permlane32_swap_b32_e32 v9, v20\n")
    assert N.swap_hazards(block + "\ts_nop 0\n\tv_permlane16_swap_b32_e32 v1, v9\n")
    assert N.swap_hazards(block + "\tv_mov_b32_dpp v4, v9 row_ror:8 row_mask:0xf bank_mask:0xf\n")
    # two states behind the write, another register, or a compiler-made write: no finding
    assert not N.swap_hazards(block + "\ts_nop 1\n\tv_permlane32_swap_b32_e32 v9, v20\n")
    assert not N.swap_hazards(block + "\tv_permlane32_swap_b32_e32 v7, v20\n")
    assert not N.swap_hazards("\tv_mov_b32_e32 v9, v2\n\tv_permlane32_swap_b32_e32 v9, v20\n")
