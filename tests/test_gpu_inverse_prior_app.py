"""The VisualOdometry app's --prior-weight <wt>,<wr> (GPU) on the small synthetic TUM-format sequence the other
app tests build: a constant-velocity Gaussian prior in the pair-by-pair loop of --method inverse | robust, through the C++
classes' SetPosePrior() / GetPriorReport().  With 0,0 the trajectory file is the one without the flag, byte for byte; a
positive weight changes it, equals the Python class driven the same way byte for byte, and stays within the numpy checker's
poses (tests/inverse_prior_ref.py on planes read back from the device); --batch and the other methods refuse the flag."""
import os
import subprocess

import numpy as np
import pytest

import phovo_amd  # noqa: F401
from phovo_amd import native, odometry, sequence

import inverse_prior_ref as pr
import inverse_ref as ir
from test_gpu_apps import K_VO, _write_tum

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "apps", "bin")
CFG5 = os.path.join(ROOT, "config_files", "config_5_level_optimization_analytic.yml")
N_FRAMES = 5
WT, WR = 2e4, 2e5              # of the order of H's translation and rotation diagonal at 160x120: data and prior both move the pose
LAMBDA = np.diag([WT] * 3 + [WR] * 3)


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "apps")])


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    path = tmp_path_factory.mktemp("prior_app")
    return path, _write_tum(path, N_FRAMES, K_VO)


def _run(path, name, extra):
    out = path / "out" / f"{name}.txt"
    return subprocess.run([os.path.join(BIN, "PhotoconsistencyVisualOdometry"), CFG5, str(path), str(out)] + extra,
                          capture_output=True, text=True, timeout=600), out


def _vo(path, name, extra):
    r, out = _run(path, name, extra)
    assert r.returncode == 0, r.stderr
    return open(out).read(), r.stdout


@pytest.mark.parametrize("method", ["inverse", "robust"])
def test_zero_weights_leave_the_trajectory_file_byte_for_byte(dataset, method):
    path, frames = dataset
    plain, _ = _vo(path, f"{method}_plain", ["--method", method])
    zero, stdout = _vo(path, f"{method}_zero", ["--method", method, "--prior-weight", "0,0"])
    assert zero == plain and len(plain.strip().split("\n")) == 2 + len(frames) - 1
    assert stdout.count("Prior: ") == len(frames) - 1            # the flag ran: every pair printed its record
    moved, _ = _vo(path, f"{method}_moved", ["--method", method, "--prior-weight", f"{WT},{WR}"])
    assert moved != plain and "nan" not in moved.lower()


@pytest.mark.parametrize("method", ["inverse", "robust"])
def test_positive_weights_are_the_python_class_driven_the_same_way(dataset, method):
    """The C++ class behind the app and the Python class are two clients of one C ABI: the same frames, the previous
    pair's result as the next pair's prior, zero for the first -- the same bytes; and the records the app prints are the
    class's."""
    path, frames = dataset
    text, stdout = _vo(path, f"{method}_cpp", ["--method", method, "--prior-weight", f"{WT},{WR}"])
    cls = odometry.CPhotoconsistencyOdometryInverse if method == "inverse" else odometry.CPhotoconsistencyOdometryRobust
    states, lines = [], []
    prior = np.zeros(6)
    with cls(0) as po:
        po.ReadConfigurationFile(CFG5)
        po.SetIntrinsicMatrix(K_VO)
        for t in range(1, len(frames)):
            po.SetSourceFrame(frames[t - 1][1], frames[t - 1][2].astype(np.float64) * (1.0 / 5000.0))
            po.SetTargetFrame(frames[t][1], frames[t][2].astype(np.float64) * (1.0 / 5000.0))
            po.SetInitialStateVector(np.zeros(6))
            po.SetPosePrior(prior, LAMBDA)
            po.Optimize()
            prior = po.GetOptimalStateVector()
            states.append(prior)
            lines.append("Prior: " + native.format_prior_report(frames[t][0], po.GetPriorReport()))
    assert text == sequence.chain_and_format(states, [f[0] for f in frames[1:]])
    assert [l for l in stdout.split("\n") if l.startswith("Prior: ")] == lines


def test_positive_weights_stay_within_the_checkers_poses(dataset):
    """--method inverse against the numpy checker run pair by pair on planes read back from the device, each pair under
    the CHECKER's previous result as its prior.  Every pair's state is within pose_bar of the checker's (the flat 1e-9 x
    max(1, |x|) here; asserted), so the chained pose after p pairs -- a product of p matrices with entries of at most 1, each
    within a few bars -- is held to 8 p bars, entry by entry, and the text carries 17 digits."""
    path, frames = dataset
    text, _ = _vo(path, "inverse_checked", ["--method", "inverse", "--prior-weight", f"{WT},{WR}"])
    ncfg = native.read_config_file(CFG5)
    nl = ncfg.num_levels
    mi = list(ncfg.max_num_iterations[:nl])
    cfg = dict(num_levels=nl, lam=list(ncfg.lambda_optimization_step[:nl]), max_iter=mi, min_grad=list(ncfg.min_gradient_norm[:nl]))
    states, prior = [], np.zeros(6)
    with odometry.AlignmentEngine() as eng:
        eng.read_configuration_file(CFG5)
        eng.set_objective(native.OBJECTIVE_INVERSE_COMPOSITIONAL)
        eng.set_intrinsic_matrix(K_VO)
        eng.reserve_frames(len(frames), 640, 480)
        for f, (_, gray, d16) in enumerate(frames):
            eng.upload_frame(f, gray, d16.astype(np.float64) * (1.0 / 5000.0))
        for t in range(1, len(frames)):
            pyr = []
            for l in range(nl):
                if mi[l] <= 0:
                    pyr.append(None)
                    continue
                i0, d0, gx0, gy0 = eng.get_level_planes(t - 1, l)
                pyr.append((i0, d0, gx0, gy0, eng.get_level_planes(t, l)[0]))
            ref = pr.optimize(pyr, K_VO, cfg, prior, LAMBDA)
            print(f"pair {t}: iterations {ref['iterations']} cond {ref['cond']:.2e} margin {ref['margin']:.2e}")
            assert ref["flags"] == 0 and ref["margin"] > 1e-6
            assert ir.pose_bar(ref["cond"], ref["state"]) <= 1e-9 * max(1.0, np.abs(ref["state"]).max())
            prior = ref["state"]
            states.append(prior)
    expected = sequence.chain_and_format(states, [f[0] for f in frames[1:]]).strip().split("\n")[2:]
    got = text.strip().split("\n")[2:]
    assert len(got) == len(expected) == len(frames) - 1
    for p, (a, b) in enumerate(zip(got, expected)):
        va, vb = np.array(a.split(" "), dtype=np.float64), np.array(b.split(" "), dtype=np.float64)
        err = np.abs(va[1:] - vb[1:]).max()
        print(f"pose {p + 1}: |app - checker| = {err:.2e}")
        assert va[0] == vb[0] and err <= 8 * (p + 1) * 1e-9


@pytest.mark.parametrize("extra,needle", [
    (["--batch", "--method", "inverse", "--prior-weight", "1,1"], "cannot be combined with --batch"),
    (["--batch", "--method", "robust", "--prior-weight", "0,0"], "cannot be combined with --batch"),
    (["--prior-weight", "1,1"], "--prior-weight needs --method inverse or --method robust"),
    (["--method", "affine", "--prior-weight", "1,1"], "--prior-weight needs --method inverse or --method robust"),
    (["--method", "inverse", "--prior-weight", "1"], "--prior-weight needs <wt>,<wr>"),
    (["--method", "inverse", "--prior-weight", "1,-2"], "--prior-weight needs <wt>,<wr>"),
    (["--method", "inverse", "--prior-weight", "nan,1"], "--prior-weight needs <wt>,<wr>"),
])
def test_the_flag_is_refused(dataset, extra, needle):
    path, _ = dataset
    r, out = _run(path, "refused", extra)
    assert r.returncode != 0 and needle in r.stderr
    usage = subprocess.run([os.path.join(BIN, "PhotoconsistencyVisualOdometry")], capture_output=True, text=True, timeout=60)
    assert usage.returncode != 0 and usage.stdout.rstrip().endswith("[--prior-weight <wt>,<wr>]")
    assert "affine|geometric]" in usage.stdout
