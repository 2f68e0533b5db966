"""bench.py's contract with the driver, on a real GPU: ONE JSON line with the agreed keys, for the single-process
form and for the N > 1 code path (ranks joined over the launcher's TCP store, callbacks all-reduced every 10 sweeps by the
engine's own RCCL communicator) forced onto one rank -- the 8-GPU runs are the driver's, so this is the only place that
path meets a device before round end."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 400_000


def run_bench(extra_env, *args):
    env = dict(os.environ, **extra_env)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "40", "--warmup", "10", "--spinup-s", "0.05",
           "--repeats", "3", "--min-gpu-seconds", "0", "--chains-per-gpu", str(M), *args]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def check_line(d, n_gpus, cb_every):
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["n_gpus"] == n_gpus and d["steps"] == 40 and d["warmup"] == 10
    assert d["unit"] == "chain-updates/s" and d["dtype"] == "f64" and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["config"]["chains_per_gpu"] == M and d["config"]["callbacks_allreduce_every"] == cb_every
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    assert rf["algorithmic_bytes_per_launch"] == 16 * M
    # ONE clock per line: frac comes from the interval value and ms_per_step come from, so frac x peak x ms_per_step is the
    # algorithmic bytes of one launch; the HIP-event figure of the same launches rides beside it under its own names
    nbytes = rf["algorithmic_bytes_per_launch"]
    assert abs(rf["frac"] * rf["peak"] * 1e9 * d["ms_per_step"] * 1e-3 - nbytes) < 1e-6 * nbytes
    assert abs(rf["frac_events"] * rf["peak"] * 1e9 * rf["avg_launch_us"] * 1e-6 - nbytes) < 1e-6 * nbytes
    assert rf["frac_events"] >= rf["frac"] * 0.95 and "perf_counter" in rf["clock"]
    assert rf["valu_busy"] is None                                     # from the committed PMC passes (profiles/) ...
    assert rf["traffic"] is None                                       # ... taken at 1e7 chains per launch: not quoted for this size
    assert isinstance(rf["traffic_provenance"]["kernel_sources_unchanged_since"], bool)
    assert "regime" in rf and ("infinity-cache" in rf["regime"] or "HBM" in rf["regime"])
    rp = d["repeat"]
    assert rp["blocks"] == 3 and rp["ms_per_step_min"] <= rp["ms_per_step_median"] and len(rp["ms_per_step_all"]) == 3
    # value = chains x steps / wall; the event-timed launches cannot take longer than the wall clock around them
    assert abs(d["value"] - M * 40 / (d["ms_per_step"] * 1e-3 * 40)) < 1e-6 * d["value"]
    assert rf["avg_launch_us"] <= d["ms_per_step"] * 1e3 * 1.05
    # the chains sample exp(-2 x^2) poorly after 50 sweeps from U(-2,2), but acceptance is already at its plateau
    assert 0.90 < d["check"]["acceptance"] < 0.97 and 0.2 < d["check"]["mean_energy"] < 1.5
    if n_gpus == 1 and cb_every == 0:
        fz = d["fused_sweepstep16"]           # the sweepstep = 16 form, next to the headline, never instead of it
        assert fz["mh_steps_per_launch"] == 16 and 0 < fz["us_per_sweep_min"] <= fz["us_per_sweep_median"]
        assert fz["us_per_sweep_min"] < rf["avg_launch_us"]                # no HBM round trip and no launch per sweep


def test_single_process_line():
    d = run_bench({}, "--full", "--no-cpu-baseline")
    check_line(d, 1, 0)
    assert "cpu_baseline" not in d
    c = d["config"]
    # no communicator in a single process; the HIP runtime libamc.so is bound to is named with its file
    assert c["rccl_ranks"] is None and c["librccl"] is None
    assert c["hip_runtime_version"] > 60000000 and "libamdhip64" in c["hip_runtime"]
    assert c["torch_imported"] is False and c["rccl_library_forced"] is False
    # BASELINE configs 3 and 5 end to end next to the headline, never instead of it
    oc = d["other_configs"]
    assert "error" not in oc and 0 < oc["config3_double_well_K2"]["us_per_time_step"] < oc["config5_pgmc"]["us_per_time_step"]
    for name in ("config3_double_well_K2", "config5_pgmc"):   # u16 counters for the first 65 535 steps: never slower than u32 by much
        assert 0 < oc[name]["us_per_time_step_first_65535_steps"] < 1.5 * oc[name]["us_per_time_step"]
    assert 0.1 < oc["config5_pgmc"]["sigma_2_after"] < 2.0 and oc["config5_pgmc"]["sigma_2_after"] != 0.1      # it learned
    # the widened paths as lines of their own: Float32 state (8 algorithmic bytes per update), a script-defined potential (16)
    for name, nbytes in (("f32_state", 8), ("custom_potential", 16)):
        w = oc[name]
        assert "error" not in w, w
        assert w["algorithmic_bytes_per_update"] == nbytes and 0 < w["us_per_launch_min"] <= w["us_per_launch_median"]
        assert abs(w["frac"] * 8000.0 * 1e9 * w["us_per_launch_median"] * 1e-6 - nbytes * M) < 1e-6 * nbytes * M


def test_distributed_path_on_one_rank():
    env = {"AMC_BENCH_FORCE_DIST": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29531", "RANK": "0",
           "LOCAL_RANK": "0", "WORLD_SIZE": "1", "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    d = run_bench(env, "--gpus", "1", "--full", "--no-cpu-baseline")
    check_line(d, 1, 10)
    c = d["config"]
    # the communicator itself says how many ranks it spans (ncclCommCount): a SCALE line shows "RCCL saw N ranks" by itself
    assert c["rccl_ranks"] == 1 and c["rccl_rank"] == 0 and c["rccl_ranks_by_rank"] == [1]
    assert "librccl" in c["librccl"] and c["rccl_version"] > 20000
    assert c["callbacks_allreduce_via"].startswith("rccl")
    assert c["hip_runtime_versions_by_rank"] == [c["hip_runtime_version"]]
    # the N > 1 route runs on the stack the single process runs on: no torch in the worker, the system's HIP runtime
    assert c["torch_imported"] is False and "/opt/rocm" in c["hip_runtime"]


def test_preflight_block_comes_before_the_first_collective():
    """N > 1 (here: the route forced onto one rank): every rank says on stderr what it is about to run on -- devices visible,
    the IPC mode, the librccl file, master and store ports -- BEFORE the store group and the communicator exist, and a rank whose
    device does not exist ends there with a sentence, not in a rendezvous."""
    env = {"AMC_BENCH_FORCE_DIST": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29537", "RANK": "0",
           "LOCAL_RANK": "0", "WORLD_SIZE": "1", "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--spinup-s", "0.05", "--repeats", "1",
           "--min-gpu-seconds", "0", "--chains-per-gpu", str(M), "--no-cpu-baseline", "--no-other-configs", "--no-ladder"]
    r = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    first = r.stderr.lstrip().splitlines()[0]
    assert first.startswith("[bench preflight rank 0/1]") and "hip_devices_visible=1" in first and "HSA_ENABLE_IPC_MODE_LEGACY=0" in first
    assert "librccl=/opt/rocm/lib/librccl.so" in first and "store_port=29538" in first
    # LOCAL_RANK names a device this process cannot see: an error of its own -- unless the launcher isolates one device per rank
    # (HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES set: every rank then sees a single device 0 and takes it)
    isolated = bool(os.environ.get("HIP_VISIBLE_DEVICES") or os.environ.get("ROCR_VISIBLE_DEVICES"))
    bad = subprocess.run(cmd, env=dict(os.environ, **dict(env, LOCAL_RANK="5", MASTER_PORT="29541")), capture_output=True, text=True, timeout=600)
    if isolated:
        assert bad.returncode == 0 and "local_rank=5 device=0" in bad.stderr
    else:
        assert bad.returncode != 0 and "device 5" in bad.stderr and "1 HIP device(s) visible" in bad.stderr
    legacy = subprocess.run(cmd, env=dict(os.environ, **dict(env, HSA_ENABLE_IPC_MODE_LEGACY="1", MASTER_PORT="29545")), capture_output=True, text=True, timeout=600)
    assert legacy.returncode != 0 and "dmabuf IPC" in legacy.stderr


def test_min_gpu_seconds_keeps_the_device_busy():
    """--min-gpu-seconds: the K-step block is repeated (outside `value`) until that much wall clock has gone by, so that a coarse
    sampler of GPU activity outside the process finds the device at work."""
    env = dict(os.environ)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "40", "--warmup", "10", "--spinup-s", "0.05", "--repeats", "2",
           "--min-gpu-seconds", "2.0", "--chains-per-gpu", str(M), "--full", "--no-cpu-baseline", "--no-other-configs", "--no-ladder"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][0])
    rp = d["repeat"]
    assert rp["blocks"] > 100 and rp["seconds"] > 1.0 and len(rp["ms_per_step_all"]) == 5
    assert rp["ms_per_step_min"] <= rp["ms_per_step_p10"] <= rp["ms_per_step_median"] <= rp["ms_per_step_p90"]


def test_gpus_flag_without_a_launcher_is_an_error():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       env={k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK")}, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "torch.distributed.run" in r.stderr


def test_default_size_line_carries_the_ladder():
    """At the default ensemble size the line also holds the M-ladder (4e7 and 1.6e8 chains: state far beyond the 256 MiB
    Infinity Cache) next to the headline figure and its regime."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "30", "--warmup", "5", "--spinup-s", "0.2", "--repeats", "2",
           "--min-gpu-seconds", "0", "--full", "--no-cpu-baseline"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][0])
    rf = d["roofline"]
    assert "infinity-cache" in rf["regime"]
    # the committed PMC figures belong to this size: quoted here, with where they come from (and only here: check_line's runs
    # at another size get null)
    pv = rf["traffic_provenance"]
    assert rf["traffic"] is not None and 0.99 < rf["traffic"] / rf["algorithmic_bytes_per_launch"] < 1.05
    assert pv["measured_in_this_run"] is False and pv["source"].startswith("profiles/") and pv["commit"]
    rows = rf["ladder"]
    assert [row["chains"] for row in rows] == [40_000_000, 160_000_000]
    for row in rows:
        assert row["regime"].startswith("HBM") and 0.2 < row["frac"] < 1.0
        assert abs(row["achieved_GBps"] - 16 * row["chains"] / row["us_per_launch_min"] / 1e3) < 1e-6 * row["achieved_GBps"]


def test_two_ranks_on_one_device_fall_back_to_the_store():
    """The driver's N > 1 launch line (`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`) with two
    ranks, both pointed at the one GPU this box has: RCCL refuses two ranks on one device, so the communicator cannot be
    built -- the run must not die there (a crashed bench leaves no scaling record at all) but say so and sum the callbacks
    over the launcher's store.  What this exercises on hardware: the store group under the real launcher, sharding by
    global chain id over two processes, the pipelined callbacks, max over ranks, ONE JSON line from rank 0."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, AMC_BENCH_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "40",
           "--warmup", "10", "--spinup-s", "0.05", "--repeats", "3", "--min-gpu-seconds", "0", "--chains-per-gpu", str(M), "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:] + r.stderr[-4000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["chains_total"] == 2 * M and d["config"]["callbacks_allreduce_every"] == 10
    assert "store" in d["config"]["callbacks_allreduce_via"] or "rccl" in d["config"]["callbacks_allreduce_via"]
    assert d["config"]["torch_imported"] is False            # the launcher only starts the workers
    assert 0.90 < d["check"]["acceptance"] < 0.97
    if "store" in d["config"]["callbacks_allreduce_via"]:       # all or none: no rank kept a communicator the other lacks
        assert d["config"]["rccl_ranks"] is None and d["config"]["rccl_ranks_by_rank"] == [None, None]
        # ... and a run RCCL did not carry is no measurement of the two-GPU path: no value, a reason, a non-zero exit
        assert d["value"] is None and "RCCL did not carry this run" in d["value_withheld"] and r.returncode != 0
    else:
        assert d["config"]["rccl_ranks"] == 2 and r.returncode == 0
        # whole-job value: both shards' updates over the slowest rank's wall time
        assert abs(d["value"] - 2 * M * 40 / (d["ms_per_step"] * 1e-3 * 40)) < 1e-6 * d["value"]


def test_plain_line_is_lean_and_its_outputs_repeat(tmp_path):
    """A plain run (no --full) times the K steps and prints the line without the extras; --dump-outputs writes what the timed
    steps computed, float64, with the same bits from run to run under the same arguments -- and under --full, whose extras come after."""
    import numpy as np
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    d = run_bench({}, "--dump-outputs", str(a))
    assert d["full"] is False and d["steps"] == 40 and d["warmup"] == 10 and d["ms_per_step"] > 0
    assert d["higher_is_better"] is True and d["dtype"] == "f64" and d["unit"] == "chain-updates/s"
    assert abs(d["value"] - M * 40 / (d["ms_per_step"] * 1e-3 * 40)) < 1e-6 * d["value"]
    for key in ("repeat", "fused_sweepstep16", "other_configs"):
        assert d[key] is None, key
    assert d["roofline"]["ladder"] is None and "cpu_baseline" not in d
    run_bench({}, "--dump-outputs", str(b))
    full = run_bench({}, "--full", "--no-cpu-baseline", "--no-other-configs", "--dump-outputs", str(c))
    assert full["full"] is True and full["repeat"]["blocks"] == 3
    names = sorted(os.listdir(a))
    assert names == ["accepted.npy", "callback_acceptance.npy", "callback_energy.npy", "chain_id.npy", "e.npy", "total.npy", "x.npy"]
    for name in names:
        want = np.load(a / name)
        assert want.dtype == np.float64 and want.size > 0 and np.all(np.isfinite(want)), name
        for other in (b, c):
            assert np.array_equal(np.load(other / name), want, equal_nan=True), (name, other)
    x, e = np.load(a / "x.npy"), np.load(a / "e.npy")
    assert x.shape == e.shape == (M,) and np.array_equal(np.load(a / "chain_id.npy"), np.arange(M))
    # the ensemble started over after the clock ramp: 12 blocks of the timed region's shape, the W warm-up steps, the K timed ones
    assert np.array_equal(np.load(a / "total.npy"), [M * (12 * 40 + 10 + 40)])
    energy, acceptance = np.load(a / "callback_energy.npy"), np.load(a / "callback_acceptance.npy")
    assert energy.shape == acceptance.shape == (1,) and energy[0] == pytest.approx(float(np.mean(e)), rel=1e-12)
    assert d["check"]["mean_energy"] == energy[0] and d["check"]["acceptance"] == acceptance[0]
