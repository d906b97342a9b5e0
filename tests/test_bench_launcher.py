"""`python bench.py --gpus N` must start its own ranks when no launcher wraps it (the driver's SCALE runs may call it
either way), and the parent must do so before anything touches the GPU.  These tests drive that logic on the CPU with
PHOVO_BENCH_BACKEND=gloo up to the device check, where the ranks stop ("no CPU fallback")."""
import ast
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, extra_env=None, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(extra_env or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout, env=env)


def test_parent_starts_the_ranks_itself_and_relays_their_status():
    """Two gloo ranks on the CPU: both join the group (world size 2), both stop at the device check, the parent exits
    non-zero with their message and prints no result line."""
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--pairs", "4", "--distinct", "2",
              "--no-cpu-baseline", "--no-reference-termination"], {"PHOVO_BENCH_BACKEND": "gloo"})
    assert "starting 2 ranks" in r.stderr
    assert "torch.distributed.run" in r.stderr and "--nproc-per-node=2" in r.stderr
    assert "rank 0/2 joined the gloo group" in r.stderr and "rank 1/2 joined the gloo group" in r.stderr
    import phovo_amd  # noqa: F401
    from phovo_amd import native
    if native.lib().phovo_device_count() < 1:
        assert r.returncode != 0
        assert "needs an MI355X" in r.stderr
        assert r.stdout.strip() == ""
    else:                                           # on a GPU box this is a real two-rank run on the shared card
        assert r.returncode == 0, r.stderr[-2000:]
        import json
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["n_gpus"] == 2


def test_under_a_launcher_the_parent_path_is_not_taken():
    """RANK set = already one of the ranks: no second launcher is started (the world-size check speaks instead)."""
    r = _run(["--gpus", "2", "--no-cpu-baseline"], {"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0",
                                                      "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29999",
                                                      "PHOVO_BENCH_BACKEND": "gloo"})
    assert "starting 2 ranks" not in r.stderr
    assert r.returncode != 0 and "needs WORLD_SIZE=2" in r.stderr


def test_parent_touches_nothing_gpu_side_before_launching():
    """Structure check: at module level bench.py imports neither torch nor the package (whose import loads
    libphovo_hip.so and with it the HIP runtime), and main() calls launch_ranks() before its first such import."""
    tree = ast.parse(open(BENCH).read())
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    names = {a.name.split(".")[0] for n in top if isinstance(n, ast.Import) for a in n.names}
    names |= {n.module.split(".")[0] for n in top if isinstance(n, ast.ImportFrom) and n.module}
    assert not names & {"torch", "phovo_amd", "oracle"}, names
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    first_import = min(n.lineno for n in ast.walk(main) if isinstance(n, (ast.Import, ast.ImportFrom)))
    launch = min(n.lineno for n in ast.walk(main)
                 if isinstance(n, ast.Call) and getattr(n.func, "id", "") == "launch_ranks")
    assert launch < first_import
    lr = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "launch_ranks")
    src = ast.get_source_segment(open(BENCH).read(), lr)
    assert "os.exec" not in src and "execv" not in src          # children, never a replaced process
    assert "Popen" in src


import pytest  # noqa: E402


@pytest.mark.gpu
def test_two_gloo_ranks_share_the_gpu_and_print_one_contract_line():
    """`python bench.py --gpus 2` with no launcher around it, on a one-GPU box (gloo instead of RCCL, which refuses two
    ranks on one device): the parent starts both ranks, each aligns its own shard on the shared card, one all_gather per
    step, rank 0 prints ONE JSON line with the driver's contract keys; value = pairs of both ranks / slowest rank's time."""
    import json
    r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--pairs", "256", "--distinct", "8", "--full",
              "--no-cpu-baseline"], {"PHOVO_BENCH_BACKEND": "gloo"})       # --full: the shipped-threshold leg across two ranks
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak" and d["dtype"] == "f64"
    assert d["config"]["pairs_per_gpu"] == 256 and d["config"]["global_pairs_per_step"] == 512
    assert d["value"] > 0 and d["nonfinite_pairs"] == 0 and d["cpu_baseline"] is None
    assert d["full"] is True and d["reference_termination"]["value"] > 0
    assert abs(d["value"] - 512 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]
    assert "rank 0/2 joined the gloo group" in r.stderr and "rank 1/2 joined the gloo group" in r.stderr


def test_dump_outputs_writes_float64_fields_and_a_fixed_sample_above_the_cap(tmp_path, monkeypatch):
    """--dump-outputs on made-up results: one float64 .npy per field with a row per pair; above the size cap the same
    seeded subset of pairs in every run and every field, named by pair_index.npy, and the files stay under the cap."""
    import numpy as np
    import bench
    import phovo_amd  # noqa: F401
    from phovo_amd import native
    n, nl = 300, 4
    rs = np.random.RandomState(5)
    states = rs.standard_normal((n, 6))
    reports = [native.PairReport() for _ in range(n)]
    for i, r in enumerate(reports):
        r.iterations[:nl] = [i % 7, 3, 20, 50]
        r.gradient_norm, r.flags = 0.25 * i, i % 3
        r.valid_pixels[:nl] = [i, 2 * i, 3 * i, 4 * i]
    bench.dump_outputs(str(tmp_path / "all"), states, reports, nl, 0, 1)
    names = ["flags", "gradient_norm", "iterations", "pair_index", "states", "valid_pixels"]
    assert sorted(f[:-4] for f in os.listdir(tmp_path / "all")) == names
    load = {k: np.load(tmp_path / "all" / f"{k}.npy") for k in names}
    assert all(a.dtype == np.float64 and a.shape[0] == n for a in load.values())
    np.testing.assert_array_equal(load["states"], states)
    np.testing.assert_array_equal(load["iterations"][:, 0], np.arange(n) % 7)
    np.testing.assert_array_equal(load["valid_pixels"][:, 3], 4 * np.arange(n))
    np.testing.assert_array_equal(load["pair_index"], np.arange(n))

    cap = 8 * (1 + 6 + nl + 1 + 1 + nl) * 50                      # room for 50 pairs
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", cap)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), states, reports, nl, 1, 2)
    for k in names:
        a, b = np.load(tmp_path / "s1" / f"{k}_rank1.npy"), np.load(tmp_path / "s2" / f"{k}_rank1.npy")
        assert a.shape[0] == 50 and np.array_equal(a, b), k
    idx = np.load(tmp_path / "s1" / "pair_index_rank1.npy").astype(int)
    assert len(set(idx)) == 50 and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(np.load(tmp_path / "s1" / "states_rank1.npy"), states[idx])
    np.testing.assert_array_equal(np.load(tmp_path / "s1" / "gradient_norm_rank1.npy"), 0.25 * idx)
    assert sum(a.nbytes for a in (np.load(tmp_path / "s1" / f"{k}_rank1.npy") for k in names)) <= cap


def test_steps_below_one_are_refused():
    r = _run(["--steps", "0"])
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr


@pytest.mark.gpu
def test_dump_outputs_hold_the_last_timed_step_and_repeat_exactly(tmp_path):
    """Two runs with the same arguments: `--steps` timed steps each, and the dumped results of the last one are bit for bit
    the same (seeded inputs, one arithmetic per pair), finite, one row per pair, with the iteration counts the line reports."""
    import json
    import numpy as np
    args = ["--steps", "3", "--warmup", "1", "--pairs", "256", "--distinct", "8", "--no-cpu-baseline",
            "--no-reference-termination"]
    lines = []
    for d in ("a", "b"):
        r = _run(args + ["--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    for d in lines:
        assert d["steps"] == 3 and d["roofline"]["step_wall_ms"]["steps"] == 3
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and "states.npy" in names
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and a.shape[0] == 256 and np.array_equal(a, b), f
    states = np.load(tmp_path / "a" / "states.npy")
    assert states.shape == (256, 6) and np.all(np.isfinite(states)) and np.any(states != 0)
    its = np.load(tmp_path / "a" / "iterations.npy")
    np.testing.assert_array_equal(its.mean(axis=0), lines[0]["iterations_per_pair"])


# what a plain run leaves null and `--full` fills: every leg that takes runs of its own after the timed steps
LEGS_BEHIND_FULL = ("reference_termination", "end_to_end_pcie_inclusive", "single_pair", "cpu_baseline",
                    "cpu_baseline_all_cores", "parity")


def test_full_is_an_option_off_by_default_and_a_plain_run_has_no_leg_to_leave_out(monkeypatch):
    """parse(): without --full every leg after the timed steps is off, whatever the --no-... options say (scripts that pass
    them keep working); with --full they run unless one of those options takes its group out."""
    import bench
    for argv, full, no_cpu, no_ref in (
            ([], False, True, True),
            (["--gpus", "1", "--steps", "5", "--warmup", "2"], False, True, True),
            (["--no-cpu-baseline"], False, True, True),
            (["--full"], True, False, False),
            (["--full", "--no-cpu-baseline"], True, True, False),
            (["--full", "--no-reference-termination"], True, False, True)):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        a = bench.parse()
        assert (a.full, a.no_cpu_baseline, a.no_reference_termination) == (full, no_cpu, no_ref), argv
    r = _run(["--help"])
    assert r.returncode == 0 and "--full" in r.stdout


def test_every_leg_behind_full_is_guarded_by_one_of_the_two_switches():
    """Structure check: main() imports the oracle, and calls its optimize(), the class surface's Optimize() or an
    enqueue_align() of its own (the timed steps enqueue inside run_steps()), only under an `if` whose test reads
    args.no_cpu_baseline or args.no_reference_termination (directly, or through `cpu`, which is set under such an `if`)."""
    src = open(BENCH).read()
    main = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "main")
    guards = ("no_cpu_baseline", "no_reference_termination", "cpu is not None")

    def guarded(node, under):
        if isinstance(node, ast.If):
            test = ast.get_source_segment(src, node.test)
            inner = under or any(g in test for g in guards)
            return [x for c in node.body for x in guarded(c, inner)] + [x for c in node.orelse for x in guarded(c, under)]
        found = []
        if not under:
            for n in ast.walk(node):
                if isinstance(n, ast.ImportFrom) and n.module == "oracle":
                    found.append(("import oracle", n.lineno))
                if isinstance(n, ast.Call) and getattr(n.func, "attr", "") in ("Optimize", "enqueue_align", "optimize"):
                    found.append((n.func.attr, n.lineno))
        if not isinstance(node, (ast.FunctionDef, ast.If)):
            return found
        return found + [x for c in ast.iter_child_nodes(node) for x in guarded(c, under)]

    loose = [x for stmt in main.body for x in guarded(stmt, False)]
    assert loose == [], loose


@pytest.mark.gpu
def test_a_plain_run_skips_every_leg_that_full_runs_and_times_the_same_steps():
    """The same small workload plain and with --full: the plain line carries null for every leg behind --full and says
    full = false; the --full line fills them all, its parity against the CPU oracle holds, and the contract fields both
    lines share (metric, unit, dtype, steps, iteration counts, launches of a timed step) are equal."""
    import json
    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--pairs", "256", "--distinct", "8"]
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full", "--cpu-seconds", "0.5", "--cpu-threads", "2"])):
        r = _run(args + extra)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(out) == 1, r.stdout[-2000:]
        lines[name] = json.loads(out[0])
    plain, full = lines["plain"], lines["full"]
    assert plain["full"] is False and full["full"] is True
    for key in LEGS_BEHIND_FULL:
        assert key in plain and plain[key] is None, key
        assert full[key] is not None, key
    assert full["parity"]["ok"] and full["parity"]["checked"] >= 1
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline_all_cores"]["cores"] == 2
    assert full["reference_termination"]["value"] > 0 and full["end_to_end_pcie_inclusive"]["value"] > 0
    for key in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "scaling", "config",
                "iterations_per_pair", "nonfinite_pairs", "launches", "pipelined"):
        assert plain[key] == full[key], key
    for d in (plain, full):
        assert d["value"] > 0 and abs(d["value"] - 256 * 2 / (d["ms_per_step"] * 2e-3)) < 1e-6 * d["value"]
        assert d["roofline"]["step_wall_ms"]["steps"] == 2
