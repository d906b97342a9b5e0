"""The prior-carrying inverse-compositional kernels' gfx950 code objects (gn_inverse_prior_kernel.hip; no GPU needed): the
figures DESIGN.md §24 records, read from the metadata the compiler writes beside the assembly.  Metadata only, no
instruction searches."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "photoconsistency-visual-odometry_amd", "csrc")
WORKGROUPS_PER_CU = 2          # 256-thread workgroups per CU = waves per SIMD
PRIOR_LDS = 8 * 42             # the pair's block (34 doubles) and its record (7), padded to 16 bytes
ROBUST_LDS = 16 * 1024 + 32    # the histogram, delta, the four wave totals, padding (gn_inverse_robust_kernel.hip's)
DYNAMIC_LDS = 8 * (32 + 8 + 4 * 32) + 4 * 4      # lds_fixed_bytes(256), as every level kernel
KEYS = ("max_flat_workgroup_size", "vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count",
        "private_segment_fixed_size", "group_segment_fixed_size")


@pytest.fixture(scope="module")
def kernels():
    """{robust: {key: value}} of the file's two kernels, from the metadata block of each."""
    subprocess.run(["make", "-s", "-C", CSRC, "isa"], check=True, capture_output=True)
    text = open(os.path.join(CSRC, "build", "gn_inverse_prior_kernel.s")).read()
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for block in re.split(r"\n  - \.", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.match(r"_ZN9phovo_hip.*gn_level_kernel_inverse_priorILi256ELi2ELb([01])E", name)
        assert m, name
        figures = {}
        for key in KEYS:
            vals = re.findall(rf"(?:^|\n)\s*\.?{key}:\s*(\d+)", block)
            assert len(vals) == 1, (name, key, vals)
            figures[key] = int(vals[0])
        assert m.group(1) not in out
        out[m.group(1) == "1"] = figures
    return out


def test_the_two_kernels_exist_once(kernels):
    assert set(kernels) == {False, True}


@pytest.mark.parametrize("robust", [False, True], ids=["objective5", "objective6"])
def test_workgroup_registers_scratch_and_lds(kernels, robust):
    figures = kernels[robust]
    print(figures)
    assert figures["max_flat_workgroup_size"] == 256
    # the whole budget of two waves per SIMD, and the spills that come with the longer serial section.  (WHERE
    # the scratch instructions stand is not something metadata can show: §24 has the listing of the basic blocks.)
    assert figures["vgpr_count"] == 256 and figures["agpr_count"] == 0
    assert figures["vgpr_spill_count"] == (43 if robust else 25)
    assert figures["private_segment_fixed_size"] == (176 if robust else 104)
    budget = (512 // WORKGROUPS_PER_CU) // 8 * 8
    assert figures["vgpr_count"] + figures["agpr_count"] <= budget
    static = PRIOR_LDS + (ROBUST_LDS if robust else 0)
    assert figures["group_segment_fixed_size"] == static                 # + DYNAMIC_LDS at the launch
    assert WORKGROUPS_PER_CU * (static + DYNAMIC_LDS) <= 160 * 1024
    assert static + DYNAMIC_LDS == (18112 if robust else 1696)           # what phovo_engine_last_launches reports
