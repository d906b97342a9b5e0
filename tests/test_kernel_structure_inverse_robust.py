"""The robust inverse-compositional kernel's gfx950 code object (gn_inverse_robust_kernel.hip; no GPU needed): the figures
DESIGN.md §22 records, read from the metadata the compiler writes beside the assembly.  Metadata only, no instruction
searches."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "photoconsistency-visual-odometry_amd", "csrc")
WORKGROUPS_PER_CU = 2          # 256-thread workgroups per CU = waves per SIMD
STATIC_LDS = 16 * 1024 + 32    # the histogram, delta, the four wave totals, padding to 16 bytes
DYNAMIC_LDS = 8 * (32 + 8 + 4 * 32) + 4 * 4      # lds_fixed_bytes(256), as every level kernel


@pytest.fixture(scope="module")
def isa():
    subprocess.run(["make", "-s", "-C", CSRC, "isa"], check=True, capture_output=True)
    return open(os.path.join(CSRC, "build", "gn_inverse_robust_kernel.s")).read().split("\n")


def _meta(isa, key):
    vals = [int(m.group(1)) for l in isa for m in [re.match(rf"\s*(?:-\s*)?\.{key}:\s*(\d+)", l)] if m]
    assert len(vals) == 1, (key, vals)
    return vals[0]


def test_the_kernel_exists_once(isa):
    names = [l for l in isa if re.match(r"\s*\.name:\s+_ZN9phovo_hip.*gn_level_kernel_inverse_robust", l)]
    assert len(names) == 1, names


def test_workgroup_registers_scratch_and_lds(isa):
    figures = {k: _meta(isa, k) for k in ("max_flat_workgroup_size", "vgpr_count", "agpr_count", "sgpr_count",
                                          "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    print(figures)
    assert figures["max_flat_workgroup_size"] == 256
    # the whole budget of two waves per SIMD, and five dwords of scratch that only the pair's set-up and the
    # solve touch (no spill inside the pixel loop)
    assert figures["vgpr_count"] == 256 and figures["agpr_count"] == 0
    assert figures["private_segment_fixed_size"] == 20 and figures["vgpr_spill_count"] == 4
    budget = (512 // WORKGROUPS_PER_CU) // 8 * 8
    assert figures["vgpr_count"] + figures["agpr_count"] <= budget
    assert figures["group_segment_fixed_size"] == STATIC_LDS             # + DYNAMIC_LDS at the launch
    # two workgroups per CU fit the 160 KiB of LDS many times over: registers set the occupancy, not the histogram
    assert WORKGROUPS_PER_CU * (STATIC_LDS + DYNAMIC_LDS) <= 160 * 1024
    assert STATIC_LDS + DYNAMIC_LDS == 17776                             # what phovo_engine_last_launches reports
