#!/usr/bin/env python3
"""Device time of one Gym step (20 fused substeps) of float64 worlds, cs_step_f64 (csrc/sfmstep_f64.hip), beside the two
other ways to step the same worlds, measured in the same run on the same machine:

    f64_ms       cs_step_f64 on CrowdWorlds64                      HIP events around the launch
    f32_ms       cs_step on CrowdWorlds (the float32 default)      HIP events around the launch
    oracle_ms    the float64 C oracle (oracle/sfm_step.inc, test infrastructure) on `--threads` host threads: wall clock

at 4096 worlds x 25 humans hsfm_farina and 4096 x 10 sfm_helbing (circular crossing from the host generators: `--distinct` worlds,
tiled to `--worlds`).  Every repeat starts from the same rows (re-uploaded outside the timed span); warm device; median with minimum
and maximum.  Prints one JSON line per case; `--out` also writes them to a file.

    python tools/step_f64_bench.py [--worlds 4096] [--repeats 20] [--threads 16] [--out profiles/step_f64_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
for _d in ("tests", os.path.join("tests", "golden")):
    sys.path.insert(0, os.path.join(ROOT, _d))

CASES = [("hsfm_farina", 25), ("sfm_helbing", 10)]


def crossing_worlds(model, humans, distinct, worlds):
    import numpy as np
    from test_facade_cpu import make_env

    rows = []
    for case in range(distinct):
        env = make_env(model, "circle_crossing", humans, False)
        env.reset(phase="test", test_case=case)
        mm = env.motion_model_manager
        rows.append((np.array(mm.states), np.array(mm.goals), np.array(mm.params), np.array(mm.safety_space)))
        type_, peq = int(mm.sfm_type), bool(mm.all_equal_humans)
    reps = (worlds + distinct - 1) // distinct
    S, G, P, saf = (np.concatenate([np.stack([r[i] for r in rows])] * reps)[:worlds] for i in range(4))
    return S, G, P, saf, type_, peq


def main():
    import numpy as np

    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from oracle import crowd_oracle as orc
    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.batched import CrowdWorlds, CrowdWorlds64

    _lib.require_gpu()
    dt = 0.0125
    stat = lambda xs: dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)))
    lines = []
    for model, humans in CASES:
        S, G, P, saf, type_, peq = crossing_worlds(model, humans, min(a.distinct, a.worlds), a.worlds)
        w64 = CrowdWorlds64(S, G, P, saf, None, type=type_, all_params_equal=peq)
        w32 = CrowdWorlds(S, G, P, saf, None, type=type_, all_params_equal=peq)

        def device(cw):
            cw.set_states(S); cw.set_goals(G); cw.sync()
            e0, e1 = _lib.Event(), _lib.Event()
            e0.record(cw.stream)
            cw.step(dt, a.substeps)
            e1.record(cw.stream)
            return e0.elapsed_ms(e1)

        def oracle():
            run = orc.StepBlockRunner(type_, S, G, None, P, saf, peq, dtype=np.float64, threads=a.threads)
            t0 = time.perf_counter()
            run.run(dt, a.substeps)
            return (time.perf_counter() - t0) * 1e3, run.S

        for _ in range(3):
            device(w64), device(w32)
        oracle()
        t = dict(f64_ms=[], f32_ms=[], oracle_ms=[])
        for _ in range(a.repeats):
            t["f64_ms"].append(device(w64))
            t["f32_ms"].append(device(w32))
            ms, ref = oracle()
            t["oracle_ms"].append(ms)
        device(w64)
        err = float(np.max(np.abs(w64.get_states()[..., 0:2] - ref[..., 0:2])))
        r = dict(model=model, worlds=a.worlds, humans=humans, substeps=a.substeps, repeats=a.repeats, oracle_threads=a.threads,
                 host_cores=orc.effective_cores(), device=_lib.device_name(0), f64_position_error_against_oracle_m=err,
                 **{k: stat(v) for k, v in t.items()})
        r["f64_over_f32"] = r["f64_ms"]["median"] / r["f32_ms"]["median"]
        r["oracle_over_f64"] = r["oracle_ms"]["median"] / r["f64_ms"]["median"]
        print(json.dumps(r), flush=True)
        lines.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
