"""GPU: one HIP runtime per process whatever the import order (crowdstep first, torch second), checked in a fresh child."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import sys
sys.path[:0] = [%(root)r, %(root)r + "/tests", %(root)r + "/tests/golden"]
assert "torch" not in sys.modules
import numpy as np
from social_navigation_pyenvs_amd import _lib
from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym
from test_facade_cpu import make_config
W = 64
env = BatchedSocialNavGym(make_config("hsfm_farina", "hybrid_scenario", 5, False), W)
env.reset(phase="test", first_case=0, device=True)          # crowdstep objects FIRST: hipMalloc, kernels
assert "torch" not in sys.modules, "crowdstep must not need torch for this"
import torch                                                 # torch SECOND
a = torch.zeros((W, 2), dtype=torch.float32, device="cuda")
a[:, 1] = 0.5
for _ in range(3):
    obs, rew, term, trunc, info = env.step_device(a)
torch.cuda.synchronize()
assert obs.is_cuda and obs.shape == (W, 5, 5) and bool(torch.isfinite(obs).all())
hip = sorted({l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l})
assert len(hip) == 1, hip                                    # ONE HIP runtime mapped
print("OK", hip[0], _lib.hip_runtime_path)
'''


def test_crowdstep_first_then_torch_share_one_hip_runtime():
    env = dict(os.environ)
    env.pop("CROWDSTEP_HIP_RUNTIME", None)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1].startswith("OK")


def test_bench_launches_its_own_ranks_and_prints_one_parsable_line(tmp_path):
    """`python bench.py --gpus 2` with no launcher around it (the rehearsal form for a one-GPU box: both ranks on GPU 0, gloo for the
    barrier): the parent starts two fresh rank processes before touching HIP, relays rank 0's line -- ONE line on stdout, strict JSON
    under 4 KB, n_gpus = 2, one record per rank with its device and PCI address, value = the worlds of BOTH ranks over the slowest
    rank's time -- and `--gpus 2` on a box that shows one GPU (no --same-device) refuses instead of measuring one rank."""
    import json

    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--same-device", "--dist-backend", "gloo", "--steps", "4", "--warmup", "2",
           "--repeats", "3", "--worlds", "512", "--full", "--no-other-configs", "--no-cpu-baseline", "--full-json", str(tmp_path / "bench_full_test.json")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and len(lines[0].encode()) < 4096
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["dist"]["world_size"] == 2 and d["dist"]["backend"] == "gloo" and d["dist"]["launcher"] == "self"
    assert [x["rank"] for x in d["ranks"]] == [0, 1] and all(x["pci"] and x["worlds"] == 512 for x in d["ranks"])
    assert d["config"]["worlds_total"] == 1024 and d["scaling"] == "weak"
    assert abs(d["value"] - 1024 * 25 * 20 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
    assert d["roofline"]["bound"] == "hbm" and 0 < d["roofline"]["frac"] < 1.5
    from social_navigation_pyenvs_amd import _lib
    if _lib.device_count() < 2:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"], capture_output=True, text=True,
                           timeout=300, env=env)
        assert r.returncode == 3 and r.stdout.strip() == "" and "needs 2 visible" in r.stderr


WG_CHILD = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, %(root)r)
from social_navigation_pyenvs_amd import scenarios as sc
from social_navigation_pyenvs_amd.batched import CrowdWorlds
out = []
for model, W, n in (("hsfm_farina", 37, 25), ("sfm_helbing", 45, 10), ("hsfm_new_moussaid", 9, 17)):
    S, goals, P, rb = sc.hybrid_worlds(W, n, model)
    cw = CrowdWorlds(S, goals, P, None, None, type=model, all_params_equal=True, respawn_bounds=rb,
                     respawn_worlds=(np.arange(W) %% 2 == 1).astype(np.int32), layout="soa")
    for _ in range(6):
        cw.step(0.0125, 20)
    out.append(hashlib.sha256(np.ascontiguousarray(cw.get_states()).tobytes() + np.ascontiguousarray(cw.get_goals()).tobytes()).hexdigest())
print("WGHASH " + " ".join(out))
"""


def test_one_wavefront_blocks_step_the_same_bits_however_many_share_a_workgroup():
    """The one-wavefront step kernels (k_sfm_step MAXT = 64, the DPP-row kernel) go to the dispatcher four independent wavefronts to a
    workgroup (sfmstep_kernel.h; CROWDSTEP_WG_WAVES = 1 / 2 / 4 is read once per process): the stepped worlds are the same bits whatever the
    width -- grids that are not a multiple of it included (37 x 25: 19 blocks; 45 x 10: 12 DPP-row wavefronts; 9 x 17: 3 blocks)."""
    hashes = {}
    for wg in ("1", "2", "4"):
        env = dict(os.environ, CROWDSTEP_WG_WAVES=wg)
        r = subprocess.run([sys.executable, "-c", WG_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("WGHASH ")]
        assert line, r.stdout[-500:]
        hashes[wg] = line[-1]
    assert hashes["1"] == hashes["2"] == hashes["4"], hashes


EAGER_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
import bench
args = bench.parse(%(argv)r)
spec = bench.workload_spec(args)
cw, _, _ = bench.build_worlds(spec, 0, 1)
for _ in range(args.warmup + args.steps):
    cw.step(spec["dt"], spec["substeps"], cw.bench_action)
np.save(%(out)r + "/states.npy", cw.get_states())
np.save(%(out)r + "/goals.npy", cw.get_goals())
"""


def test_bench_plain_run_times_exactly_its_steps_and_dumps_what_they_computed(tmp_path):
    """A plain `bench.py --steps K --warmup W` times exactly K steps (K > GRAPH_STEPS: full graphs and a remainder graph), prints the headline
    without the --full blocks, and --dump-outputs writes the worlds as W + K eager steps of the same inputs leave them, bit for bit, on every run."""
    import json

    import numpy as np

    argv = ["--gpus", "1", "--steps", "1203", "--warmup", "3", "--worlds", "96"]
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv + ["--dump-outputs", str(tmp_path / run)],
                           capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["steps"] == 1203 and d["warmup"] == 3 and d["timing_repeats"] == 1 and d["n_gpus"] == 1
        assert d["ms_per_step"] > 0 and abs(d["value"] - 96 * 25 * 20 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
        assert {"metric", "unit", "higher_is_better", "dtype"} <= set(d) and d["dtype"] == "f32" and d["higher_is_better"] is True
        assert not {"roofline", "other_configs", "cpu_baseline", "gym_step", "finite_fraction"} & set(d)
        assert d["outputs"]["arrays"]["states"] == [96, 25, 13]
    r = subprocess.run([sys.executable, "-c", EAGER_CHILD % {"root": ROOT, "argv": argv, "out": str(tmp_path)}], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    for name in ("states", "goals"):
        want = np.load(tmp_path / f"{name}.npy")
        for run in ("a", "b"):
            got = np.load(tmp_path / run / f"{name}.npy")
            assert got.dtype == np.float32 and got.shape == want.shape
            assert np.array_equal(got, want, equal_nan=True), (name, run, float(np.nanmax(np.abs(got - want))))


def test_bare_python_values_step_the_same_bits_as_wrapped_arguments():
    """cs_step and cs_step_f64 through the signature table (_lib.ABI): the same uploaded worlds (2 x 3 humans, Helbing's SFM, shared
    parameters, no walls, no robot: each human has two partners) stepped for 2 substeps with every argument in its ctypes wrapper and with
    bare Python values -- dt a Python float, converted to float / double by the header's type -- leave the same bits."""
    import ctypes as C

    import numpy as np

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd import scenarios as sc
    from social_navigation_pyenvs_amd.batched import CrowdWorlds, CrowdWorlds64

    lib = _lib.load()
    pos, yaw, goals = sc.circular_crossing(2, 3, radius=1.5)
    S = sc.make_states(pos, yaw, goals)
    P = np.tile(sc.default_params("sfm_helbing"), (3, 1))
    dt = 0.0125
    for worlds, entry, real, wrap in ((CrowdWorlds, lib.cs_step, np.float32, C.c_float), (CrowdWorlds64, lib.cs_step_f64, np.float64, C.c_double)):
        cw = worlds(S, goals, P, type=0)
        d = cw.descriptor()
        rows = []
        for args in ((C.byref(d), wrap(dt), C.c_int(2), C.c_void_p(None), C.c_void_p(cw.stream)), (C.byref(d), dt, 2, None, cw.stream)):
            cw.set_states(S)
            cw.set_goals(goals)
            _lib.check(entry(*args))
            rows.append(cw.get_states())
        assert rows[0].dtype == real and rows[0].shape == (2, 3, 13) and np.isfinite(rows[0]).all()
        assert not np.array_equal(rows[0][..., :2], S[..., :2].astype(real)), "the worlds did not move"
        assert rows[0].tobytes() == rows[1].tobytes()
