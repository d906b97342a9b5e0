"""The randomised sweep of the sampled-system kernels (gn_evaluate_sampled_kernels.hip) on the device:
tests/tools/fuzz_objectives.py in mode `sampled`, as a subprocess, in the three forms of fuzz_objectives.SAMPLED_SWEEPS.
Reference: sampled_system_ref.system6 / system8 in fp64 on the planes the device holds, under
sampled_system_ref.check_against; a case that misses is set aside only where one ulp of fx moves the checker's own answer
by more than a quarter of the bar or changes its row count (the tool's docstring has the rule).
tests/test_sampled_sweep_cpu.py holds the same seeds and counts to full coverage, and the checker alone to the caps,
without a device."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "tools", "fuzz_objectives.py")
sys.path.insert(0, os.path.dirname(TOOL))
import fuzz_objectives as fo  # noqa: E402


@pytest.mark.parametrize("flags,cases,seed", fo.SAMPLED_SWEEPS, ids=[f[0] if f else "plain" for f, _, _ in fo.SAMPLED_SWEEPS])
def test_sampled_randomised_sweep_against_checker(flags, cases, seed):
    """0 failures, the case count, fewer than 5 % of the cases set aside, every coverage class and every tile class reached,
    and (but for the 40 cases of `big`) empty systems and systems of fewer rows than columns among those checked."""
    r = subprocess.run([sys.executable, TOOL, str(cases), str(seed), "sampled", *flags], capture_output=True, text=True,
                       timeout=300)
    out = r.stdout
    print(out[-4000:])
    assert r.returncode == 0, out[-3000:] + r.stderr[-2000:]
    m = re.search(r"^(\d+) cases, (\d+) failures, (\d+) skipped", out, re.M)
    assert m and int(m.group(1)) == cases and int(m.group(2)) == 0, out[-3000:]
    assert int(m.group(3)) < 0.05 * cases, out[-3000:]
    assert "checker raised" not in out
    m = re.search(r"(\d+) systems checked, (\d+) empty, (\d+) of fewer rows than columns", out)
    assert m and int(m.group(1)) >= 2 * cases, out[-3000:]
    if "big" not in flags:
        assert int(m.group(2)) > 0 and int(m.group(3)) > 0, out[-3000:]
    line = [l for l in out.splitlines() if l.startswith("coverage (sampled")][0]
    for k in fo.SAMPLED_CLASSES:
        assert re.search(rf"(^|\s){re.escape(k)}: [1-9]", line), (k, line)
    line = [l for l in out.splitlines() if l.startswith("geometries exercised")][0]
    for g in ("tiles1", "tiles2-16", "tiles17+"):
        assert re.search(rf"(^|\s){re.escape(g)}: [1-9]", line), (g, line)
