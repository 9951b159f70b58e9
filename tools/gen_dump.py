#!/usr/bin/env python3
"""Every byte the device generators write, for the A/B of two builds of the library (a refactor of csrc/generate.hip must not move one):

    CROWDSTEP_LIB=<build A> python tools/gen_dump.py dump A.npz
    CROWDSTEP_LIB=<build B> python tools/gen_dump.py dump B.npz        (a process each: one library per process)
    python tools/gen_dump.py compare A.npz B.npz                       (exit status 1 when an array differs)

Dumped per case: the raw state buffer, goal lists, robot rows, respawn flags, status and scenario of four worlds that held a fill
pattern before the call (so the rows a failed world must leave alone count too).  The case table is the product of
  scenario (4) x n (2, 5, 8, 9, 63, 64, 65, 70: both kernels and their edges) x insert_robot x randomize_attributes x randomize_positions
  x AoS / SoA x robot row x SFM / ORCA x max_tries (1, 2, default), and one masked call per scenario x n x layout x robot row x model.
Worlds of up to 9 humans stand on the default circle / box, larger ones on a circle of 30 m and a box of 60 x 20 m; combinations that
cannot be generated stay in the table (their status and untouched rows are part of the result).  Then the live worlds of 96-world
device-resident loops under the three refill cadences of tests/test_gpu_generators.py::test_step_device_is_the_same_whatever_the_refill_cadence
(the pre-staged episodes: k_refill_staged, k_consume_staged and the in-place fallback)."""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENARIOS = ("circle_crossing", "parallel_traffic", "circular_crossing_with_static_obstacles", "hybrid_scenario")
NS = (2, 5, 8, 9, 63, 64, 65, 70)
W = 4


def _worlds(n, layout, robot_row, model):
    from social_navigation_pyenvs_amd.batched import CrowdWorlds

    rows = n + int(robot_row)
    return CrowdWorlds(np.zeros((W, rows, 13)), np.zeros((W, n, 2, 2)), np.zeros((n, 20)), None, None, type=model, all_params_equal=True,
                       robot_row=robot_row, robot=np.zeros((W, 13)), respawn_worlds=np.ones(W, np.int32), layout=layout)


def _fill(cw):
    cw.d_state.upload(np.full(cw.d_state.shape, 7, np.float32), cw.stream)
    cw.d_goals.upload(np.full(cw.d_goals.shape, 5, np.float32), cw.stream)
    cw.d_robot.upload(np.full(cw.d_robot.shape, 3, np.float32), cw.stream)
    cw.d_world_flags.upload(np.ones(W, np.int32), cw.stream)


def _take(out, name, cw, status, scn):
    for key, arr in (("states", cw.d_state.download(cw.stream)), ("goals", cw.get_goals()), ("robot", cw.get_robot()),
                     ("flags", cw.d_world_flags.download(cw.stream)), ("status", status), ("scenario", scn)):
        out[f"{name}/{key}"] = np.array(arr)


def dump_cases(out):
    from social_navigation_pyenvs_amd import generators as gen

    case = 0
    for n, layout, robot_row, model in itertools.product(NS, ("aos", "soa"), (False, True), ("sfm_helbing", "orca")):
        cw = _worlds(n, layout, robot_row, model)
        box = dict(circle_radius=30, traffic_length=60, traffic_height=20) if n > 9 else {}
        tag = f"n{n}/{layout}/row{int(robot_row)}/{model}"
        for scenario in SCENARIOS:
            for ir, ra, rp, mt in itertools.product((True, False), (False, True), (True, False), (1, 2, gen.MAX_PLACEMENT_TRIES)):
                case += 1
                _fill(cw)
                status, scn = gen.generate_worlds(cw, scenario, 1000 + 4 * case + np.arange(W), insert_robot=ir, randomize_attributes=ra,
                                                  randomize_positions=rp, max_tries=mt, raise_on_failure=False, **box)
                _take(out, f"{tag}/{scenario}/ir{int(ir)}ra{int(ra)}rp{int(rp)}/mt{mt}", cw, status, scn)
            case += 1                                       # a masked call over worlds of another seed
            _fill(cw)
            gen.generate_worlds(cw, scenario, 500 + 4 * case + np.arange(W), raise_on_failure=False, max_tries=3000, **box)
            status, scn = gen.generate_worlds(cw, scenario, 900000 + 4 * case + np.arange(W), mask=np.array([1, 0, 0, 1]), raise_on_failure=False,
                                              max_tries=3000, **box)
            _take(out, f"{tag}/{scenario}/masked", cw, status, scn)
    return case


def dump_cadences(out):
    import torch
    from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_generators import _config                 # the cadence test's own configuration, not a copy of it

    cfg = _config("circle_crossing", human_num=6)
    Wl = 96
    for name, every, depth, fold in (("default", None, None, True), ("never_again", 10 ** 9, 2, False), ("every_step", 1, 1, False)):
        env = BatchedSocialNavGym(cfg, Wl)
        if every is not None:
            env.REFILL_EVERY, env.STAGE_DEPTH, env.FOLD_RESET = every, depth, fold
        env.reset(phase="train", first_case=7, device=True)
        ended = 0
        for _ in range(90):                                  # the robots are driven into the nearest human: short episodes, many resets
            rb = env.cw.d_robot.torch().view(Wl, 13)
            d = env.observe_device()[:, :, 0:2] - rb[:, None, 0:2]
            near = d[torch.arange(Wl), d.norm(dim=2).argmin(dim=1)]
            a = (near / near.norm(dim=1, keepdim=True).clamp(min=1e-6)).contiguous()
            obs, rew, term, trunc, info = env.step_device(a)
            ended += int((term | trunc).sum())
        assert ended > 0 and env.failed_resets() == 0, (name, ended)
        print(f"cadence {name}: {ended} episodes ended and were regenerated")
        flags = env.cw.d_world_flags                        # (a pure circle-crossing batch has no respawn flags)
        for key, arr in (("states", env.cw.d_state.download(env.cw.stream)), ("goals", env.cw.get_goals()), ("robot", env.cw.get_robot()),
                         ("flags", np.zeros(0, np.int32) if flags is None else flags.download(env.cw.stream)), ("obs", obs.cpu().numpy()),
                         ("ended", np.array([ended]))):
            out[f"cadence/{name}/{key}"] = np.array(arr)


def compare(pa, pb):
    A, B = np.load(pa), np.load(pb)
    names = sorted(A.files)
    assert names == sorted(B.files), "the two dumps hold different cases"
    bad = [k for k in names if A[k].dtype != B[k].dtype or A[k].shape != B[k].shape or A[k].tobytes() != B[k].tobytes()]
    ok1 = sum(1 for k in names if k.endswith("/status") and np.any(A[k] == 0))
    failed = sum(1 for k in names if k.endswith("/status") and np.any(A[k] != 0))
    print(f"{len(names)} arrays compared byte for byte ({sum(A[k].nbytes for k in names)} bytes; {ok1} calls with a generated world, "
          f"{failed} with a refused one): {len(bad)} differ")
    for k in bad[:20]:
        print("  differs:", k)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    from social_navigation_pyenvs_amd import _lib

    out = {}
    cases = dump_cases(out)
    dump_cadences(out)
    np.savez(sys.argv[2], **out)
    print(f"{cases} generator calls and three refill cadences, {len(out)} arrays -> {sys.argv[2]} (library {_lib.LIB_PATH})")
