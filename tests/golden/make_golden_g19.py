#!/usr/bin/env python3
"""Generate tests/golden/g19_transform.npz by RUNNING THE REFERENCE's ``MultiHumanRL.transform`` and value networks on the current state.

TEST INFRASTRUCTURE ONLY.  Run from the repo root:  python tests/golden/make_golden_g19.py

The reference is imported through make_golden.py's harness; only numbers (inputs and what the reference produced) and short names are
written.  24 seeded joint states -- n in {1, 5} humans, 13 and 15 columns (theta and omega visible), six of each, the goal at least 1 m
from the robot, every input a float32 value (what the reference's ``torch.Tensor([...])`` makes of it anyway) -- and per state:

  rows      the reference's ``MultiHumanRL.transform(state)`` (float32 [n][13 | 15]): what its trainer stores as ``last_state``
  rows64    a float64 restatement of ``rotate`` (crowd_nav/policy/cadrl.py:305-345) on the same inputs, written here in numpy
  cadrl     the reference CADRL ``model(rows[None])`` [n] (one output per human: the policy's value is their minimum)
  sarl      the reference SARL ``model(rows[None])`` (one output)

Case kinds: "weights" (one per network: cadrl / sarl x 13 / 15 columns, seeded at the scale G16 seeds them -- N(0, 0.25) matrices,
N(0, 0.1) biases; SARL's attention output layer scaled by 0.1, as the GPU suite calms it, so that the published softmax without maximum
subtraction overflows nowhere -- recorded as the seed, the key order and the SHA-256 of the float32 bytes: draw_weights) and "states"
(one per column count, the states stacked: state i owns the human rows offset[i] .. offset[i] + n[i]).
"""
import configparser
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (imports the reference through _refharness)
import _refharness  # noqa: E402
from golden_io import save_cases  # noqa: E402

ns = mg.ns
F32 = np.float32


def rotate64(robot, humans, headed):
    """rotate (cadrl.py:305-345) for a holonomic robot, float64: robot [9] FullState order, humans [n][5 | 7] -> [n][13 | 15]"""
    robot, humans = np.asarray(robot, np.float64), np.asarray(humans, np.float64)
    px, py, vx, vy, radius, gx, gy, v_pref = robot[:8]
    rot = np.arctan2(gy - py, gx - px)
    c, s = np.cos(rot), np.sin(rot)
    n = len(humans)
    one = np.ones(n)
    hx, hy = humans[:, 0] - px, humans[:, 1] - py
    cols = [np.hypot(gx - px, gy - py) * one, v_pref * one, 0.0 * one, radius * one, (vx * c + vy * s) * one, (vy * c - vx * s) * one,
            hx * c + hy * s, hy * c - hx * s, humans[:, 2] * c + humans[:, 3] * s, humans[:, 3] * c - humans[:, 2] * s, humans[:, 4],
            np.hypot(hx, hy), radius + humans[:, 4]]
    if headed:
        cols += [humans[:, 5] - 0.0, humans[:, 6]]
    return np.stack(cols, 1)


def draw_state(rng, n, headed):
    f = lambda x: float(F32(x))
    p = rng.uniform(-4, 4, 2)
    ang, dist = rng.uniform(0, 2 * np.pi), rng.uniform(1.0, 9.0)
    robot = [f(p[0]), f(p[1]), f(rng.uniform(-1, 1)), f(rng.uniform(-1, 1)), f(rng.uniform(0.2, 0.4)), f(p[0] + dist * np.cos(ang)),
             f(p[1] + dist * np.sin(ang)), f(rng.uniform(0.5, 1.5)), f(rng.uniform(-3, 3))]
    if np.hypot(robot[5] - robot[0], robot[6] - robot[1]) < 1.0:
        robot[5] = f(robot[5] + 1.0)
    humans = []
    for _ in range(n):
        a, d = rng.uniform(0, 2 * np.pi), rng.uniform(0.7, 6.0)
        h = [f(robot[0] + d * np.cos(a)), f(robot[1] + d * np.sin(a)), f(rng.uniform(-1, 1)), f(rng.uniform(-1, 1)), f(rng.uniform(0.2, 0.5))]
        if headed:
            h += [f(rng.uniform(-np.pi, np.pi)), f(rng.uniform(-1, 1))]
        humans.append(h)
    return robot, humans


def make_policy(name, headed):
    import torch
    from crowd_nav.policy.policy_factory import policy_factory

    pcfg = configparser.RawConfigParser()
    pcfg.read(os.path.join(_refharness.REFERENCE_ROOT, "crowd_nav", "configs", "policy.config"))
    pcfg.set("sarl", "with_theta_and_omega_visible", "true" if headed else "false")
    policy = policy_factory[name]()
    policy.configure(pcfg)
    seed = {"cadrl": 1901, "sarl": 1902}[name] + 10 * int(headed)
    digest = draw_weights(policy.model, seed, calm=name == "sarl")
    policy.set_device(torch.device("cpu"))
    policy.set_phase("test")
    return policy, seed, digest


def draw_weights(model, seed, calm):
    """Seeded weights at G16's scale -- N(0, 0.25) matrices, N(0, 0.1) biases -- drawn from numpy's frozen RandomState stream in the sorted
    order of the state_dict keys, so that a test rebuilds them from the seed alone (the fixture records the seed and the SHA-256 of the
    float32 bytes, not 1 MB of noise).  calm: SARL's attention output layer times 0.1 (float32).  Returns the digest."""
    import hashlib

    import torch

    rs = np.random.RandomState(seed)
    sd = model.state_dict()
    h = hashlib.sha256()
    last_attention = max((k for k in sd if k.startswith("attention.") and k.endswith(".weight")), key=lambda k: int(k.split(".")[1]), default=None)
    with torch.no_grad():
        for key in sorted(sd):
            w = (rs.standard_normal(tuple(sd[key].shape)) * (0.25 if sd[key].dim() > 1 else 0.1)).astype(F32)
            if calm and last_attention and key.rsplit(".", 1)[0] == last_attention.rsplit(".", 1)[0]:
                w = w * F32(0.1)
            sd[key].copy_(torch.from_numpy(w))
            h.update(key.encode() + b"\0" + np.ascontiguousarray(w).tobytes())
    return h.hexdigest()


def generate():
    import torch
    from crowd_nav.utils.state import JointState

    State, Obs, ObsHeaded = ns.state.FullState, ns.state.ObservableState, ns.state.ObservableStateHeaded
    rng = np.random.default_rng(1919)
    cases = []
    for headed in (False, True):
        made = {name: make_policy(name, headed) for name in ("cadrl", "sarl")}
        pols = {name: m[0] for name, m in made.items()}
        for name, (pol, seed, digest) in made.items():
            assert pol.kinematics == "holonomic" and bool(pol.with_theta_and_omega_visible) == headed
            sd = pol.model.state_dict()
            cases.append(dict(kind="weights", wkey=f"{name}_{15 if headed else 13}", policy=name, cols=15 if headed else 13, seed=seed, calm=name == "sarl",
                              sha256=digest, weights_keys=sorted(str(k) for k in sd.keys()),
                              weights_shapes=[list(sd[k].shape) for k in sorted(sd.keys())]))
        robots, counts, humans_all, rows, rows64, cadrl_out, sarl_out = [], [], [], [], [], [], []
        for n in (1, 5):
            for _ in range(6):
                robot, humans = draw_state(rng, n, headed)
                state = JointState(State(*robot), [(ObsHeaded if headed else Obs)(*h) for h in humans])
                with torch.no_grad():
                    x = pols["sarl"].transform(state)              # MultiHumanRL.transform
                    assert x.dtype == torch.float32 and tuple(x.shape) == (n, 15 if headed else 13)
                    v_c = pols["cadrl"].model(x.unsqueeze(0))      # [1, n, 1]
                    v_s = pols["sarl"].model(x.unsqueeze(0))       # [1, 1]
                robots.append(robot)
                counts.append(n)
                humans_all += humans
                rows.append(x.numpy().astype(F32))
                rows64.append(rotate64(robot, humans, headed))
                cadrl_out.append(v_c.numpy().astype(F32).reshape(n))
                sarl_out.append(float(v_s.item()))
        counts = np.array(counts, np.int32)
        cases.append(dict(kind="states", cols=15 if headed else 13, headed=headed, n=counts,
                          offset=np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32), robot=np.array(robots, np.float64),
                          humans=np.array(humans_all, np.float64), rows=np.concatenate(rows), rows64=np.concatenate(rows64),
                          cadrl=np.concatenate(cadrl_out), sarl=np.array(sarl_out, F32)))
    return cases


if __name__ == "__main__":
    cases = generate()
    for c in cases:
        if c["kind"] == "states":
            err = float(np.max(np.abs(c["rows"].astype(np.float64) - c["rows64"])))
            print(f"{c['cols']} columns: {len(c['n'])} states, reference float32 rows against the float64 restatement: max |diff| {err:.3e}; "
                  f"finite values: {bool(np.all(np.isfinite(c['cadrl'])) and np.all(np.isfinite(c['sarl'])))}; max |V| {float(np.max(np.abs(c['sarl']))):.3f}")
    print("g19_transform:", len(cases), "cases ->", save_cases("g19_transform", cases))
