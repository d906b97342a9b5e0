"""The gfx950 code objects of gn_evaluate_robust_kernels.hip (no GPU needed): the figures DESIGN.md §23 records, read from
the metadata the compiler writes beside the assembly, and the figures of k_eval_inverse and gn_level_kernel_inverse_robust,
which this file restates and must not have moved.  Metadata, and one look at the atomics: the file's
only atomics are the integer adds of the histogram (LDS and global), no float atomic anywhere.  Vector and LDS mnemonics
only; no other instruction search."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "photoconsistency-visual-odometry_amd", "csrc")
WAVES_PER_SIMD = 3             # k_eval_robust's __launch_bounds__(256, 3): DESIGN.md §23
HIST_WAVES_PER_SIMD = 4        # k_eval_robust_hist's
KEYS = ("max_flat_workgroup_size", "vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
        "private_segment_fixed_size", "group_segment_fixed_size")


@pytest.fixture(scope="module")
def build():
    subprocess.run(["make", "-s", "-C", CSRC, "isa"], check=True, capture_output=True)
    return os.path.join(CSRC, "build")


def _kernels(path):
    """{kernel name: {key: value}} from the amdhsa.kernels metadata of one assembly file."""
    text = open(path).read()
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", "\n" + meta)[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {k: int(re.search(rf"\.{k}:\s*(\d+)", block).group(1)) for k in KEYS}
    return out


def _one(kernels, part):
    names = [n for n in kernels if part in n]
    assert len(names) == 1, (part, sorted(kernels))
    return kernels[names[0]]


def test_the_four_kernels_and_their_registers(build):
    kernels = _kernels(os.path.join(build, "gn_evaluate_robust_kernels.s"))
    assert len(kernels) == 4, sorted(kernels)
    hist, delta = _one(kernels, "18k_eval_robust_histE"), _one(kernels, "19k_eval_robust_deltaE")
    tile, finish = _one(kernels, "13k_eval_robustE"), _one(kernels, "20k_eval_robust_finishE")
    for name, k in (("k_eval_robust_hist", hist), ("k_eval_robust_delta", delta), ("k_eval_robust", tile),
                    ("k_eval_robust_finish", finish)):
        print(name, k)
        assert k["max_flat_workgroup_size"] == 256
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0
    # a SIMD has 512 registers per lane: the waves per SIMD the launch bounds name must fit, accumulation registers
    # included, in the allocation granule of 8
    assert tile["vgpr_count"] + tile["agpr_count"] <= (512 // WAVES_PER_SIMD) // 8 * 8 == 168
    assert hist["vgpr_count"] + hist["agpr_count"] <= (512 // HIST_WAVES_PER_SIMD) // 8 * 8 == 128
    assert delta["vgpr_count"] + delta["agpr_count"] <= 128 and finish["vgpr_count"] + finish["agpr_count"] <= 128
    # static LDS: 32 pose constants + the 16 KiB histogram; four wave totals; 32 pose constants + 4 waves x 32 sums;
    # 8 subsets x 32 sums
    assert hist["group_segment_fixed_size"] == 32 * 8 + 4096 * 4
    assert delta["group_segment_fixed_size"] == 4 * 4
    assert tile["group_segment_fixed_size"] == (32 + 4 * 32) * 8
    assert finish["group_segment_fixed_size"] == 8 * 32 * 8


def test_the_only_atomics_are_the_histograms_integer_adds(build):
    text = open(os.path.join(build, "gn_evaluate_robust_kernels.s")).read()
    code = [ln.split("//")[0].split(";")[0].strip() for ln in text.splitlines()]
    mnemonics = [ln.split()[0] for ln in code if ln and not ln.startswith(".") and not ln.endswith(":")]
    atomics = {m for m in mnemonics
               if "atomic" in m or re.match(r"ds_(add|sub|rsub|inc|dec|min|max|and|or|xor|mskor|cmpst|wrxchg|pk_add)", m)}
    print(sorted(atomics))
    assert atomics, "the histogram kernel has lost its atomics"
    for m in atomics:                                            # (the assembler spells the 32-bit global add with or without _u32)
        assert re.fullmatch(r"ds_add_u32|global_atomic_add(_u32)?", m), m
    assert "ds_add_u32" in atomics and any(m.startswith("global_atomic_add") for m in atomics)
    assert not any(re.search(r"_f(16|32|64)$|pk_add", m) for m in atomics)


def test_the_restated_kernels_figures_have_not_moved(build):
    inv = _one(_kernels(os.path.join(build, "gn_evaluate_inverse_kernels.s")), "14k_eval_inverseE")
    print("k_eval_inverse", inv)
    assert inv["vgpr_count"] == 137 and inv["private_segment_fixed_size"] == 0
    rob = _one(_kernels(os.path.join(build, "gn_inverse_robust_kernel.s")), "gn_level_kernel_inverse_robust")
    print("gn_level_kernel_inverse_robust", rob)
    assert rob["vgpr_count"] == 256 and rob["private_segment_fixed_size"] == 20
