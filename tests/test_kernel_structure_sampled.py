"""Structure of the sampled-system kernels' gfx950 assembly (gn_evaluate_sampled_kernels.hip; no GPU needed): the two
six-column row kinds for each plane storage, the eight-column kind for fp64 planes and the two finishing widths exist;
nothing goes to scratch, in the pixel loops or anywhere else; there is no atomic of any kind (the sums are fixed-order and the
kernel boundary is the only synchronisation); a workgroup is 256 threads."""
import os
import re
import subprocess

import pytest

import test_kernel_structure as ks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "photoconsistency-visual-odometry_amd", "csrc")


@pytest.fixture(scope="module")
def isa():
    subprocess.run(["make", "-s", "-C", CSRC, "isa"], check=True, capture_output=True)
    return open(os.path.join(CSRC, "build", "gn_evaluate_sampled_kernels.s")).read().split("\n")


@pytest.fixture(scope="module")
def kernels(isa):
    out = {}
    for a, l in enumerate(isa):
        m = re.match(r"^(_ZN9phovo_hip\w*k_eval_sampled\w*):", l)
        if m:
            b = next(i for i in range(a, len(isa)) if "s_endpgm" in isa[i])
            out[m.group(1)] = isa[a:b + 1]
    return out


def test_every_instantiation_exists(kernels):
    names = list(kernels)
    for storage in ("dd", "ff", "6__halff"):                       # F64, F32, F16 (depth fp32)
        for kind in (0, 1):                                        # the reference's Jacobian, the corrected one
            assert sum(f"k_eval_sampledI{storage}Li{kind}EE" in n for n in names) == 1, (storage, kind)
    assert sum("k_eval_sampledIddLi2EE" in n for n in names) == 1   # eight columns: fp64 planes
    assert sum("k_eval_sampled_finishILi1EE" in n for n in names) == 1
    assert sum("k_eval_sampled_finishILi2EE" in n for n in names) == 1
    assert len(names) == 9


def test_no_scratch(kernels):
    for name, body in kernels.items():
        assert not any("scratch_" in l for l in body), name
    ks.test_no_scratch_in_innermost_loops(kernels)


def test_no_atomics(kernels):
    for name, body in kernels.items():
        assert not [l for l in body if re.search(r"\b(global|buffer|flat|ds)_\w*atomic", l)], name


def test_workgroups_are_256_threads(isa, kernels):
    sizes = {}                              # (the metadata states a kernel's size right in front of its name)
    size = None
    for l in isa:
        m = re.match(r"\s*\.max_flat_workgroup_size:\s*(\d+)", l)
        if m:
            size = int(m.group(1))
        m = re.match(r"\s*\.name:\s*(\S+)", l)
        if m and m.group(1) in kernels:
            sizes[m.group(1)] = size
    assert set(sizes) == set(kernels)
    assert set(sizes.values()) == {256}, sizes
