"""bench.py's launch contract (round-2 verdict #1): `bench.py --gpus N` with no RANK in the environment starts N
fresh rank processes itself before touching torch / HIP; a world size that differs from --gpus is an error, never a silent
1-GPU number; a failing rank makes the launcher exit non-zero.  CPU tests of the launch step; the -m gpu test runs the
real thing (two ranks sharing the box's GPU, gloo carrying the collectives)."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(kw)
    return env


def test_dry_launch_starts_n_children_with_the_rank_environment():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "3", "--dry-launch"], env=_env(), capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr
    rep = json.loads(p.stdout.strip().splitlines()[-1])
    kids = rep["dry_launch"]
    assert rep["rc"] == [0, 0, 0]
    assert [k["rank"] for k in kids] == [0, 1, 2] and [k["local_rank"] for k in kids] == [0, 1, 2]
    assert all(k["world_size"] == 3 and k["master_addr"] == "127.0.0.1" for k in kids)
    assert len({k["master_port"] for k in kids}) == 1 and kids[0]["master_port"] > 0


def test_dry_launch_child_never_imports_torch():
    """The launcher parent and the dry children must finish without importing torch (= without any chance of touching HIP):
    poison the import."""
    poison = os.path.join(ROOT, "tests", "_poison")
    os.makedirs(os.path.join(poison, "torch"), exist_ok=True)
    with open(os.path.join(poison, "torch", "__init__.py"), "w") as f:
        f.write("raise ImportError('torch must not be imported by the launcher or by --dry-launch children')\n")
    try:
        p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-launch"], env=_env(PYTHONPATH=poison),
                           capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert len(json.loads(p.stdout.strip().splitlines()[-1])["dry_launch"]) == 2
    finally:
        import shutil
        shutil.rmtree(poison, ignore_errors=True)


def test_world_size_mismatch_is_an_error():
    """RANK set (we ARE a rank) but the world has 1 rank while --gpus says 2: exit 2, no JSON line."""
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=_env(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 2, (p.returncode, p.stderr[-2000:])
    assert "refusing to run" in p.stderr and not p.stdout.strip()


@pytest.mark.skipif(__import__("torch").cuda.is_available(), reason="on a GPU box the ranks would run the real bench")
def test_a_failing_rank_fails_the_launch():
    """Here (no GPU) every rank comes up under gloo, passes the world-size check and then fails on 'no HIP device': the
    launcher must report that as a non-zero exit code and must not print a JSON line."""
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0", "--gaussians", "100",
                        "--width", "64", "--height", "48"], env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode != 0
    assert "rank(s) failed" in p.stderr
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]  # (gloo itself prints a connection note to stdout)


@pytest.mark.gpu
def test_bench_gpus_2_self_launches_two_ranks(launch_ranks):
    """`python bench.py --gpus 2 ...` WITHOUT torchrun, started from the GPU-free launcher (the pytest process has touched
    HIP): two ranks share the one GPU of the box, gloo carries the collectives.  The JSON line must say n_gpus = 2 =
    ranks_seen and carry the exchange report with every form timed."""
    rc, out = launch_ranks([sys.executable, BENCH, "--gpus", "2", "--gaussians", "20000", "--width", "640", "--height", "480",
                            "--steps", "4", "--warmup", "1", "--no-cpu-baseline", "--steady-steps", "20", "--full"], 1,
                           env={"GSR_DIST_BACKEND": "gloo"}, timeout=900, raw=True)
    assert rc == [0], out[0]
    line = [ln for ln in out[0].splitlines() if ln.startswith("{")][-1]
    rep = json.loads(line)
    assert rep["n_gpus"] == 2 and rep["ranks_seen"] == 2
    assert rep["config"]["launch"].startswith("self-launched")
    ex = rep["exchange"]
    assert set(ex["forms"]) == {"factored+overlap", "factored", "plain"}  # each from its own fresh rank group
    assert all(f.get("ms_per_step", 0) > 0 for f in ex["forms"].values()), ex["forms"]
    assert ex["headline_form"] == ex["library_default_form"] == "factored+overlap"
    assert rep["steady_state"]["steps"] == 5 and rep["untimed_steps_total"] == 1 + 15 + 5 + 5  # W + settle + survey + re-settle
    assert ex["bytes_per_gpu"] == int(2 * 0.5 * 11 * 20000 * 4 + 1 * 3 * 20000 * 4)
    assert ex["forms"]["plain"]["bytes_per_gpu"] == int(2 * 0.5 * 59 * 20000 * 4)
    assert ex["ms"] > 0 and ex["backend"] == "gloo"
    # gloo with device tensors cannot keep two communicators in flight: the line must say which form really ran
    assert ex["overlap"] is False and "sequential" in ex["form"]


# ---- the supervisor (round-3 verdict "Next #1"): sections in fresh children, timeouts, merge -------------------------------
def _fake(argv, timeout=300, **env):
    p = subprocess.run([sys.executable, BENCH] + argv, env=_env(GSR_BENCH_FAKE=env.pop("GSR_BENCH_FAKE", "1"), **env),
                       capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p, (json.loads(lines[-1]) if lines else None), lines


def test_supervisor_n1_merges_sections_into_one_line():
    p, rep, lines = _fake(["--steps", "3", "--warmup", "1", "--full"])
    assert p.returncode == 0 and len(lines) == 1, p.stderr
    assert rep["ms_per_step"] == 1.5 and rep["cpu_baseline"]["kind"] == "port" and "config2" in rep["extra_configs"]


def test_a_failing_or_hanging_extra_section_never_costs_the_headline():
    p, rep, _ = _fake(["--steps", "3", "--warmup", "1", "--section-timeout", "3", "--full"], GSR_BENCH_FAIL_FORM="extras")
    assert p.returncode == 0 and rep["ms_per_step"] == 1.5 and "error" in rep["extras_error"]
    assert rep["cpu_baseline"]["kind"] == "port"
    p, rep, _ = _fake(["--steps", "3", "--warmup", "1", "--section-timeout", "2", "--full"], GSR_BENCH_HANG_FORM="cpu_baseline")
    assert p.returncode == 0 and rep["cpu_baseline"] == {"timeout": 2.0, "wall_s": rep["cpu_baseline"]["wall_s"]}
    assert "extra_configs" in rep
    p, rep, _ = _fake(["--steps", "3", "--warmup", "1", "--full"], GSR_BENCH_FAIL_FORM="headline")
    assert p.returncode != 0 and rep is None


@pytest.mark.parametrize("hang", ["factored", "factored+overlap"])
def test_a_hanging_exchange_form_is_recorded_and_the_line_survives(hang):
    p, rep, lines = _fake(["--gpus", "2", "--steps", "3", "--warmup", "1", "--section-timeout", "3", "--full"], GSR_BENCH_HANG_FORM=hang)
    assert p.returncode == 0 and len(lines) == 1, p.stderr
    forms = rep["exchange"]["forms"]
    assert forms[hang] == {"timeout": 3.0, "wall_s": forms[hang]["wall_s"]}
    assert forms["plain"]["ms_per_step"] == 3.0
    # headline: the library default when its group completed, else the best completed form
    assert rep["exchange"]["headline_form"] == ("factored+overlap" if hang == "factored" else "factored")
    assert rep["n_gpus"] == 2 and "timed out" in p.stderr


def test_a_failing_plain_form_is_recorded_and_all_forms_failing_fails():
    p, rep, _ = _fake(["--gpus", "2", "--steps", "3", "--warmup", "1", "--full"], GSR_BENCH_FAIL_FORM="plain")
    assert p.returncode == 0 and "error" in rep["exchange"]["forms"]["plain"] and rep["exchange"]["headline_form"] == "factored+overlap"
    p, rep, _ = _fake(["--gpus", "2", "--steps", "3", "--warmup", "1", "--section-timeout", "2", "--full"],
                      GSR_BENCH_FAKE="hang-all")
    assert p.returncode != 0 and rep is None and "rank(s) failed" in p.stderr


def test_rank0_stdout_larger_than_a_pipe_does_not_block_the_launch():
    """rank 0's pipe was only read after every rank had exited (64 KB of NCCL_DEBUG output = deadlock)."""
    p, rep, lines = _fake(["--gpus", "2", "--steps", "3", "--warmup", "1"], timeout=120, GSR_BENCH_FAKE_NOISE="300000")
    assert p.returncode == 0 and len(lines) == 1 and rep["n_gpus"] == 2


def test_supervisors_under_torchrun_rendezvous_each_form_on_a_fresh_port():
    """The driver's launch: `python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2`.  Every torchrun worker is a
    supervisor; each form's rank group does a REAL gloo rendezvous + all-reduce on the port rank 0 published (the agent's own
    store and its TORCHELASTIC_* variables must not leak into the children)."""
    from bench import _free_port
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", str(_free_port()), BENCH, "--gpus", "2", "--steps", "3", "--warmup", "1", "--full"],
                       env=_env(GSR_BENCH_FAKE="dist"), capture_output=True, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, p.stderr[-3000:]
    rep = json.loads(lines[0])
    assert rep["n_gpus"] == 2 and set(rep["exchange"]["forms"]) == {"plain", "factored", "factored+overlap"}
    assert all("ms_per_step" in f for f in rep["exchange"]["forms"].values())


def test_guarded_extras_record_errors_instead_of_raising(monkeypatch):
    import bench

    class FakeWl:
        def __init__(self, *a, **kw): self.kw = kw
        def measure(self, steps, warmup): return {"steps": steps}
        def summary(self, m): return {"ms_per_step": 1.0}
        def close(self): pass

    monkeypatch.setattr(bench, "Workload", FakeWl)
    monkeypatch.setenv("GSR_BENCH_FAIL_EXTRA", "config5")
    args = bench.parse_args([])
    out = bench.extra_configs(None, None, args)
    assert out["config2"]["ms_per_step"] == 1.0 and "error" in out["config5"] and out["rgbd"]["ms_per_step"] == 1.0
    assert set(out["trainer_step"]) == {"tail_step", "tail_in_backward"}
    assert bench.guarded(lambda: 1 / 0)["error"].startswith("ZeroDivisionError")


@pytest.mark.gpu
def test_bench_one_rank_rccl_runs_every_form_in_its_own_process(launch_ranks):
    """GSR_DIST_FORCE=1: the collectives run on a ONE-rank "nccl" (= RCCL) communicator — the only way to push the real RCCL code
    path of every exchange form (communicator creation with a timeout, the two extra communicators of the overlapped form, async
    work handles, stream joins) through the supervisor on a one-GPU box: three sections, three fresh processes, one line."""
    rc, out = launch_ranks([sys.executable, BENCH, "--gpus", "1", "--gaussians", "20000", "--width", "640", "--height", "480",
                            "--steps", "4", "--warmup", "1", "--steady-steps", "20", "--full"], 1,
                           env={"GSR_DIST_FORCE": "1"}, timeout=900, raw=True)
    assert rc == [0], out[0]
    rep = json.loads([ln for ln in out[0].splitlines() if ln.startswith("{")][-1])
    ex = rep["exchange"]
    assert ex["backend"] == "nccl" and set(ex["forms"]) == {"plain", "factored", "factored+overlap"}
    assert all(f.get("ms_per_step", 0) > 0 for f in ex["forms"].values()), ex["forms"]
    assert ex["headline_form"] == "factored+overlap" and ex["overlap"] is True
    assert rep["n_gpus"] == 1 and rep["ranks_seen"] == 1


# ---- round 5: the first 8-GPU line must be self-interpreting; PMC numbers must not go stale silently ------------------------
def test_headline_form_flag_and_the_form_named_in_the_line():
    """--headline-form plain makes the line's top-level numbers the ONE all-reduce north_star names (default: the library
    default form); either way config.parallelism / config.exchange_form say which form `value` is, every form is reported with
    its expected_ms (bytes / 7 x 153 GB/s), and a failed plain group falls back to the best completed form — and says so."""
    p, rep, lines = _fake(["--gpus", "2", "--steps", "3", "--warmup", "1", "--full"])
    assert p.returncode == 0 and len(lines) == 1, p.stderr
    ex = rep["exchange"]
    assert ex["headline_form"] == "factored+overlap" and ex["headline_form_requested"] == "default"
    assert rep["config"]["exchange_form"] == "factored+overlap" and "factored+overlap" in rep["config"]["parallelism"]
    assert rep["ms_per_step"] == 1.8 and all(f["expected_ms"] == 0.1 for f in ex["forms"].values())
    p, rep, lines = _fake(["--gpus", "2", "--steps", "3", "--warmup", "1", "--headline-form", "plain", "--full"])
    assert p.returncode == 0 and len(lines) == 1, p.stderr
    ex = rep["exchange"]
    assert ex["headline_form"] == "plain" and ex["headline_form_requested"] == "plain" and ex["library_default_form"] == "factored+overlap"
    assert rep["ms_per_step"] == 3.0 and rep["config"]["exchange_form"] == "plain"
    assert rep["config"]["parallelism"].startswith("[exchange form of this line: plain]")
    assert ex["forms"]["factored+overlap"]["ms_per_step"] == 1.8  # the others are still there
    p, rep, _ = _fake(["--gpus", "2", "--steps", "3", "--warmup", "1", "--headline-form", "plain", "--full"], GSR_BENCH_FAIL_FORM="plain")
    assert p.returncode == 0 and rep["exchange"]["headline_form"] == "factored+overlap" and rep["config"]["exchange_form"] == "factored+overlap"


def test_expected_exchange_time_is_bytes_over_the_xgmi_peak():
    import bench
    assert bench.XGMI_PEAK_GBS == 7 * 153.0
    # 236 MB arena at n = 8: 2 (n-1)/n S bytes per GPU -> 413 MB / 1071 GB/s = 0.386 ms
    b = int(2 * 7 / 8 * 59 * 1_000_000 * 4)
    assert abs(b / (bench.XGMI_PEAK_GBS * 1e9) * 1e3 - 0.3856) < 1e-3


def test_pmc_measurements_go_stale_with_the_kernel_sources(tmp_path):
    """profiles/pmc_traffic.json entries carry the git blob hashes of the kernel sources they were measured on; bench.py
    reports `traffic: null` + `pmc_stale: true` once one of them changed (round-4 verdict, weak #8)."""
    import bench
    now = bench.kernel_source_hashes()
    assert set(now) == set(bench.PMC_KERNEL_SOURCES) and all(len(h) == 40 for h in now.values())
    # the hash IS git's blob hash (so `git rev-parse <commit>:<path>` backfills old measurements)
    f = os.path.join(ROOT, "gaussiansplatting.jl_amd", "csrc", "binning.hip")
    if os.path.isdir(os.path.join(ROOT, ".git")):
        assert subprocess.run(["git", "hash-object", f], capture_output=True, text=True, cwd=ROOT).stdout.strip() == now["binning.hip"]
    assert bench.pmc_stale_files({"kernel_sources": dict(now)}) == []
    assert bench.pmc_stale_files({"kernel_sources": dict(now, **{"composite.hip": "0" * 40})}) == ["composite.hip"]
    assert bench.pmc_stale_files({}) == sorted(bench.PMC_KERNEL_SOURCES)  # a record without hashes is stale by definition
    # a copy of the tree with one kernel source touched
    import shutil
    d = tmp_path / "gaussiansplatting.jl_amd" / "csrc"
    d.mkdir(parents=True)
    for name in bench.PMC_KERNEL_SOURCES:
        shutil.copy(os.path.join(ROOT, "gaussiansplatting.jl_amd", "csrc", name), d / name)
    assert bench.pmc_stale_files({"kernel_sources": now}, root=str(tmp_path)) == []
    with open(d / "pergauss.hip", "a") as fh:
        fh.write("// touched\n")
    assert bench.pmc_stale_files({"kernel_sources": now}, root=str(tmp_path)) == ["pergauss.hip"]
    # every committed measurement names its sources (an entry measured before a file joined the list is stale for that file)
    doc = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    assert all(rec.get("kernel_sources") and set(rec["kernel_sources"]) <= set(bench.PMC_KERNEL_SOURCES) for rec in doc["configs"].values())
    import importlib.util
    spec = importlib.util.spec_from_file_location("pmc_parse", os.path.join(ROOT, "tools", "pmc_parse.py"))
    pp = importlib.util.module_from_spec(spec); spec.loader.exec_module(pp)
    assert tuple(pp.KERNEL_SOURCES) == tuple(bench.PMC_KERNEL_SOURCES) and pp.kernel_source_hashes() == now


def test_scenes_section_is_merged_and_priced():
    """extra_configs.scenes comes from its own child process; annotate_predictions prices every record against the headline's
    stage times (and never costs the line)."""
    import bench
    p, rep, lines = _fake(["--steps", "3", "--warmup", "1", "--full"])
    assert p.returncode == 0 and rep["extra_configs"]["scenes"]["hot_tile_32k"]["ms_per_step"] == 2.0
    p, rep, _ = _fake(["--steps", "3", "--warmup", "1", "--section-timeout", "3", "--full"], GSR_BENCH_HANG_FORM="scenes")
    assert p.returncode == 0 and "timeout" in rep["extra_configs"]["scenes"] and "config2" in rep["extra_configs"]
    p, rep, _ = _fake(["--steps", "3", "--warmup", "1", "--no-scenes", "--full"])
    assert p.returncode == 0 and "scenes" not in rep["extra_configs"]
    head = {"preprocess": 0.126, "tile_scan": 0.013, "sort_composite_fwd": 0.355, "loss_fwd": 0.067, "loss_bwd": 0.051,
            "composite_bwd": 0.656, "pergauss_bwd": 0.142}
    cfg = {"n_gaussians": 1_000_000, "visible": 858_462, "tile_instances": 3_888_089}
    same = {"resolution": [1920, 1080], "mode": "rgb", "n_gaussians": 1_000_000, "visible": 858_462, "tile_instances": 3_888_089,
            "stages_ms": dict(head), "ms_per_step": sum(head.values())}
    pr = bench.predict_from_headline(same, head, cfg)
    assert abs(pr["ratio"] - 1.0) < 1e-3 and pr["within_bar"] and pr["stages_over_bar"] == []
    slow = dict(same, stages_ms=dict(head, composite_bwd=1.5, tile_sort=0.2, composite_fwd=0.1), ms_per_step=sum(head.values()) + 1.144)
    pr = bench.predict_from_headline(slow, head, cfg)
    assert pr["stages_over_bar"] == ["composite_bwd", "sort_composite_fwd"] and not pr["within_bar"]
    # tier launches priced with the fused forward; the tier walk runs beside the fused launch: sorts + the longer of the two
    assert pr["stages"]["sort_composite_fwd"]["measured_ms"] == round(0.2 + max(0.355, 0.1), 4) and "beside" in pr["model"]
    comp = dict(same, stages_ms={k: v for k, v in dict(head, tile_sort=0.4, composite_fwd=0.45).items() if k != "sort_composite_fwd"})
    pr = bench.predict_from_headline(comp, head, cfg)   # compact mode: no fused launch, the stages follow each other
    assert pr["stages"]["sort_composite_fwd"]["measured_ms"] == round(0.4 + 0.45, 4) and "beside" not in pr["model"]
    # the loss head of a larger image does not run out of the Infinity Cache as config 3's does: priced against its stand-alone
    # per-pixel cost too, and named only when it breaks the bar against both (round 6; round-5 verdict "weak #9")
    px = 2560 * 1440 / (1920 * 1080)
    big = {"resolution": [2560, 1440], "mode": "rgbd", "n_gaussians": 3_000_000, "visible": 2_500_000, "tile_instances": 9_000_000,
           "stages_ms": {"loss_fwd": 0.1205, "loss_bwd": 0.1186}, "ms_per_step": 0.24}
    pr = bench.predict_from_headline(big, head, cfg)
    assert pr["stages"]["loss_bwd"]["ratio"] > 1.3 and "standalone_predicted_ms" in pr["stages"]["loss_bwd"]
    assert pr["stages_over_bar"] == [] and "Infinity Cache" in pr["stages"]["loss_bwd"]["note"]
    pr = bench.predict_from_headline(dict(big, stages_ms={"loss_fwd": 0.1205, "loss_bwd": 0.2}), head, cfg)
    assert pr["stages_over_bar"] == ["loss_bwd"]
    pr = bench.predict_from_headline(dict(same, stages_ms=dict(head, loss_bwd=0.09)), head, cfg)   # in-cache size: no exemption
    assert pr["stages_over_bar"] == ["loss_bwd"] and "note" not in pr["stages"]["loss_bwd"]
    line = {"roofline": {"stages_ms": head}, "config": cfg, "extra_configs": {"scenes": {"a": dict(same), "b": {"error": "x"}}}}
    bench.annotate_predictions(line)
    assert line["extra_configs"]["scenes"]["a"]["vs_config3_cost"]["within_bar"] and "vs_config3_cost" not in line["extra_configs"]["scenes"]["b"]


def test_total_budget_bounds_the_run_and_skipped_sections_are_recorded():
    """Round-5 verdict, next #3: the section limits used to add up to more than the driver's 1800 s.  Now the whole run has ONE
    budget: a section gets min(its own limit, budget left - 30 s), what no longer fits is {"skipped": "budget"}, the worst-case
    wall is below the budget by construction, and the merged-so-far line is written out after every section."""
    import bench
    # worst case by construction: every section hangs until its limit -> the sum of the limits handed out stays below the budget
    args = bench.parse_args(["--full"])
    assert args.total_budget == 900.0 and args.total_budget < 1800.0
    secs = bench.plan_sections(args, 1)
    assert secs == ["headline", "cpu_baseline", "extras", "scenes", "train_protocol"]
    left, total = args.total_budget, 0.0
    for i, _ in enumerate(secs):
        own = args.section_timeout * (1.5 if i == 0 else 1.0)
        if i > 0 and left - 30.0 < min(own, 20.0):
            continue
        total += min(own, max(left - 30.0, 20.0 if i == 0 else 0.0))
        left = args.total_budget - total
    assert total <= args.total_budget - 30.0 + 1e-6
    # five fake sections of ~7.5 s each under a 62 s budget (30 s of it the reserve): the first ones run, the rest is skipped — and
    # says so
    t0 = time.time()
    p, rep, lines = _fake(["--steps", "3", "--warmup", "1", "--total-budget", "62", "--full"], GSR_BENCH_FAKE_SLEEP="7", timeout=200)
    wall = time.time() - t0
    assert p.returncode == 0 and len(lines) == 1, p.stderr
    assert rep["ms_per_step"] == 1.5 and rep["cpu_baseline"]["kind"] == "port"
    budget = rep["bench_budget"]
    assert budget["total_budget_s"] == 62.0 and list(budget["sections"]) == secs
    skipped = [k for k, v in budget["sections"].items() if v == "skipped: budget"]
    assert skipped and skipped[-1] == "train_protocol" and "headline" not in skipped and "cpu_baseline" not in skipped
    for k in skipped:
        where = rep["extra_configs"][k] if k in ("scenes", "train_protocol") else rep.get("extras_error")
        assert where["skipped"] == "budget"
    assert wall < 62.0 and rep["bench_wall_s"] < 62.0
    # the partial line went out after every finished section (stderr; and gpurun_out/bench_partial.json when that directory exists)
    partial = [ln for ln in p.stderr.splitlines() if ln.startswith("bench.py partial line: ")]
    assert len(partial) == len(secs) - len(skipped)
    first = json.loads(partial[0].split(": ", 1)[1])
    assert first["ms_per_step"] == 1.5 and first["partial"]["sections_done"] == ["headline"] and "cpu_baseline" not in first
    # a hanging LATE section costs its own limit, never the line; and everything that fits is there
    p, rep, _ = _fake(["--steps", "3", "--warmup", "1", "--section-timeout", "3", "--full"], GSR_BENCH_HANG_FORM="train_protocol")
    assert p.returncode == 0 and "timeout" in rep["extra_configs"]["train_protocol"] and "hot_tile_32k" in rep["extra_configs"]["scenes"]
    p, rep, _ = _fake(["--steps", "3", "--warmup", "1", "--full"])
    assert rep["extra_configs"]["train_protocol"]["ms_per_step"]["mean"] == 1.2
    assert rep["extra_configs"]["scenes"]["trained_by_protocol"]["ms_per_step"] == 1.9   # (c): the trained scene joins the scenes
    p, rep, _ = _fake(["--steps", "3", "--warmup", "1", "--no-train-protocol", "--full"])
    assert "train_protocol" not in rep["extra_configs"] and "trained_by_protocol" not in rep["extra_configs"]["scenes"]


# ---- a plain run measures the headline alone (everything else: --full); --dump-outputs ------------------------------------
def test_a_plain_run_measures_the_headline_alone():
    """Without --full the supervisor runs one section — N = 1: the headline; N > 1: the rank group of the form the headline asks
    for — and nothing else: no CPU baseline, no extras, no other exchange form, no partial line."""
    import bench
    assert bench.plan_sections(bench.parse_args([]), 1) == ["headline"]
    assert bench.plan_sections(bench.parse_args(["--gpus", "2"]), 2) == ["factored+overlap"]
    assert bench.plan_sections(bench.parse_args(["--gpus", "2", "--headline-form", "plain"]), 2) == ["plain"]
    p, rep, lines = _fake(["--steps", "3", "--warmup", "1"])
    assert p.returncode == 0 and len(lines) == 1, p.stderr
    assert rep["ms_per_step"] == 1.5 and rep["steps"] == 3 and list(rep["bench_budget"]["sections"]) == ["headline"]
    assert not {"cpu_baseline", "other_tile_lists", "extra_configs", "extras_error"} & set(rep)
    assert "partial line" not in p.stderr
    p, rep, lines = _fake(["--gpus", "2", "--steps", "3", "--warmup", "1"])
    assert p.returncode == 0 and len(lines) == 1, p.stderr
    assert list(rep["exchange"]["forms"]) == ["factored+overlap"] and rep["ms_per_step"] == 1.8


def test_dump_outputs_writes_float32_and_the_same_sample_every_time(tmp_path):
    """dump_outputs: float32 .npy per output; the loss and an image up to 1920 x 1080 x 3 whole; a larger image and every
    per-Gaussian array beyond DUMP_ROWS rows as a fixed, sorted choice of pixels / rows — the same rows for every array and
    every run — and never more than 64 MB."""
    import numpy as np
    import torch

    import bench
    n = 100_000
    g = torch.Generator().manual_seed(0)
    idx = torch.arange(n, dtype=torch.float32)
    outs = {"image": torch.arange(1080 * 1920, dtype=torch.float32).repeat_interleave(5).view(1080, 1920, 5),
            "loss": torch.tensor(0.25, dtype=torch.float64),
            "grad_means": torch.stack([idx, -idx, idx], 1), "grad_shs": idx.view(n, 1, 1).expand(n, 16, 3).contiguous(),
            "grad_opacities": torch.randn(n, 1, generator=g)}
    total = bench.dump_outputs(str(tmp_path / "a"), outs)
    assert total <= bench.DUMP_MAX_BYTES
    bench.dump_outputs(str(tmp_path / "b"), outs)
    got = {}
    for name in outs:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b), name
        got[name] = a
    assert got["loss"] == np.float32(0.25)
    pix = got["image"][:, 0]
    assert got["image"].shape == (bench.DUMP_IMAGE_BYTES // 20, 5) and np.all(np.diff(pix) > 0)
    assert np.array_equal(got["image"], np.repeat(pix[:, None], 5, 1))
    rows = got["grad_means"][:, 0]
    assert rows.shape == (bench.DUMP_ROWS,) and np.all(np.diff(rows) > 0)
    assert np.array_equal(got["grad_shs"], np.broadcast_to(rows[:, None, None], (bench.DUMP_ROWS, 16, 3)))
    assert np.array_equal(got["grad_opacities"], outs["grad_opacities"].numpy()[rows.astype(np.int64)])
    # 1920 x 1080 :rgb is written whole, and so is a model of at most DUMP_ROWS Gaussians
    small = {"image": torch.rand(1080, 1920, 3, generator=g), "grad_means": torch.rand(bench.DUMP_ROWS, 3, generator=g)}
    bench.dump_outputs(str(tmp_path / "c"), small)
    assert np.array_equal(np.load(tmp_path / "c" / "image.npy"), small["image"].view(-1, 3).numpy())
    assert np.array_equal(np.load(tmp_path / "c" / "grad_means.npy"), small["grad_means"].numpy())


@pytest.mark.gpu
def test_a_plain_run_dumps_the_last_timed_step(launch_ranks, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` without --full: the headline alone, K timed steps, and the
    image / loss / five gradients of the last timed step as float32 .npy files."""
    import numpy as np
    out = tmp_path / "outputs"
    rc, o = launch_ranks([sys.executable, BENCH, "--gpus", "1", "--gaussians", "20000", "--width", "640", "--height", "480",
                          "--steps", "4", "--warmup", "1", "--dump-outputs", str(out)], 1, timeout=600, raw=True)
    assert rc == [0], o[0]
    rep = json.loads([ln for ln in o[0].splitlines() if ln.startswith("{")][-1])
    assert rep["steps"] == 4 and rep["ms_per_step"] > 0 and rep["value"] > 0 and rep["dtype"] == "f32"
    assert not {"cpu_baseline", "other_tile_lists", "extra_configs", "steady_state"} & set(rep)
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == {"image", "loss", "grad_means", "grad_shs", "grad_opacities", "grad_scales", "grad_rotations"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got["image"].shape == (640 * 480, 3) and got["grad_shs"].shape == (20000, 16, 3) and float(got["loss"]) > 0
    assert np.abs(got["grad_means"]).sum() > 0
