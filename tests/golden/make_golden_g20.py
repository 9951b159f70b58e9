#!/usr/bin/env python3
"""Generate tests/golden/g20_occupancy.npz by RUNNING THE REFERENCE's OM-SARL (``sarl.with_om = true``): its occupancy maps, its
``transform`` and network, and its decisions in its own Gym.

TEST INFRASTRUCTURE ONLY.  Run from the repo root:  python tests/golden/make_golden_g20.py

The reference is imported through make_golden.py's harness; only numbers (inputs and what the reference produced) and short names are
written.  Weights are recorded as seed + key order + SHA-256 (tests/om_cases.py draw_weights, golden G19's).  Case kinds:

  "maps"      one per grid configuration of om_cases.CONFIGS: states of n in {2, 3, 5, 9} humans (float32 values; positions within 1.6 m of
              a common centre -- dense enough that most pairs fall inside a 4 m grid --, velocities within 1 m/s) stacked -- state i owns the human rows offset[i] .. offset[i] + n[i] -- among them, by
              construction, a standing centre human that is also a standing other, two humans 0.1 m apart (one cell, so a mean is a mean),
              a human 20 m away (outside every grid) and an exactly coincident pair.  Recorded: ``ref`` the reference's
              build_occupancy_maps (float32), ``maps64`` om_cases.maps64's float64 restatement, ``pre`` its pre-floor cell coordinates of
              every pair (state i owns n[i]^2 rows from pre_offset[i]).  A state with a pair within 1e-5 of an integer pre-floor coordinate
              is redrawn (the coincident pair at an even cell_num sits at exactly cell_num / 2 in float32 too and is exempt).
  "weights"   one per OM-SARL network (13 / 15 columns for the transform cases, 13 for the decisions)
  "transform" one per column count at the default [om]: the reference's transform(state) rows [n][61 | 63] and model(rows[None])
  "decision"  the reference OM-SARL deciding in its own Gym (hsfm_farina, circle crossing, 5 humans, robot_visible=False, as G16) through
              the SERIAL branch (policy.parallelize = False after reset): the robot's full state, the observation, the next human states
              handed to build_occupancy_maps, the maps it returned, the 81 network outputs, rewards and action values, the arg-max
  "exception" what the PARALLEL branch (policy.parallelize = True, as SocialNavGym.reset leaves it) raises for OM-SARL
"""
import configparser
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (imports the reference through _refharness)
import _refharness  # noqa: E402
import om_cases  # noqa: E402
from golden_io import save_cases  # noqa: E402

ns = mg.ns
F32 = np.float32


def make_policy(cfg=om_cases.CONFIGS[0], headed=False, seed=None):
    import torch
    from crowd_nav.policy.policy_factory import policy_factory

    pcfg = configparser.RawConfigParser()
    pcfg.read(os.path.join(_refharness.REFERENCE_ROOT, "crowd_nav", "configs", "policy.config"))
    pcfg.set("sarl", "with_om", "true")
    pcfg.set("sarl", "with_theta_and_omega_visible", "true" if headed else "false")
    for key, value in zip(("cell_num", "cell_size", "om_channel_size"), cfg):
        pcfg.set("om", key, str(value))
    policy = policy_factory["sarl"]()
    policy.configure(pcfg)
    assert policy.name == "OM-SARL" and policy.with_om
    digest = None if seed is None else om_cases.draw_weights(policy.model, seed, calm=True)
    policy.set_device(torch.device("cpu"))
    policy.set_phase("test")
    return policy, digest


def draw_humans(rng, n, variant):
    f = lambda x: float(F32(x))
    centre = rng.uniform(-4, 4, 2)
    h = [[f(centre[0] + rng.uniform(-1.6, 1.6)), f(centre[1] + rng.uniform(-1.6, 1.6)), f(rng.uniform(-1, 1)), f(rng.uniform(-1, 1))] for _ in range(n)]
    if variant == 0:                    # a standing human: a centre whose frame is the world's, and a standing other for the rest
        h[0][2] = h[0][3] = 0.0
    elif variant == 1 and n >= 3:       # two humans 0.1 m apart: one cell for most centres
        h[2][0], h[2][1] = f(h[1][0] + 0.1), f(h[1][1] + 0.05)
    elif variant == 2:                  # outside every grid
        h[n - 1][0] = f(h[n - 1][0] + 20.0)
    elif variant == 3:                  # exactly coincident
        h[1][0], h[1][1] = h[0][0], h[0][1]
    return h


def near_integer(pre, cell_num):
    with np.errstate(invalid="ignore"):
        close = (np.abs(pre - np.round(pre)) <= om_cases.EDGE) & (pre != cell_num / 2)
    return close & ~np.isnan(pre)


def gen_maps():
    Obs = ns.state.ObservableState
    rng = np.random.default_rng(2020)
    cases = []
    for cfg in om_cases.CONFIGS:
        cell_num, cell_size, channels = cfg
        policy, _ = make_policy(cfg)
        counts, humans_all, ref, m64, pres = [], [], [], [], []
        redrawn = pairs = inside = shared = 0
        for n in (2, 3, 5, 9):
            for variant in range(5):
                while True:
                    h = draw_humans(rng, n, variant)
                    maps, pre = om_cases.maps64(h, cell_num, cell_size, channels)
                    if not near_integer(pre, cell_num).any():
                        break
                    redrawn += 1
                got = policy.build_occupancy_maps([Obs(*row, 0.3) for row in h])
                assert got.dtype.is_floating_point and tuple(got.shape) == maps.shape
                fl = np.floor(pre)
                ins = np.all((fl >= 0) & (fl < cell_num), axis=-1)
                pairs += n * (n - 1)
                inside += int(ins.sum())
                for i in range(n):
                    cells = (cell_num * fl[i, ins[i], 1] + fl[i, ins[i], 0]).astype(int)
                    shared += int((np.bincount(cells, minlength=1) >= 2).sum())
                counts.append(n)
                humans_all += h
                ref.append(got.numpy().astype(F32))
                m64.append(maps)
                pres.append(pre.reshape(n * n, 2))
        counts = np.array(counts, np.int32)
        allpre = np.concatenate(pres)
        assert not near_integer(allpre, cell_num).any()
        assert shared >= 1, cfg
        if cell_num == 4:
            assert 2 * inside >= pairs, (cfg, inside, pairs)
        err = float(np.max(np.abs(np.concatenate(ref).astype(np.float64) - np.concatenate(m64))))
        print(f"maps {cfg}: {len(counts)} states, {pairs} pairs, {inside} inside, {shared} cells with two or more, {redrawn} redrawn, "
              f"reference against maps64: max |diff| {err:.3e}")
        cases.append(dict(kind="maps", cell_num=cell_num, cell_size=float(cell_size), channels=channels, n=counts,
                          offset=np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32),
                          pre_offset=np.concatenate([[0], np.cumsum(counts.astype(np.int64) ** 2)[:-1]]).astype(np.int32),
                          humans=np.array(humans_all, np.float64), ref=np.concatenate(ref), maps64=np.concatenate(m64), pre=allpre))
    return cases


def weights_case(wkey, policy, seed, digest, cols):
    sd = policy.model.state_dict()
    return dict(kind="weights", wkey=wkey, cols=cols, seed=seed, calm=True, sha256=digest, weights_keys=sorted(str(k) for k in sd.keys()),
                weights_shapes=[list(sd[k].shape) for k in sorted(sd.keys())])


def gen_transform():
    import torch
    from crowd_nav.utils.state import JointState

    import make_golden_g19 as g19

    State, Obs, ObsHeaded = ns.state.FullState, ns.state.ObservableState, ns.state.ObservableStateHeaded
    rng = np.random.default_rng(2021)
    cases = []
    for headed in (False, True):
        cols, seed = 15 if headed else 13, 2001 + 10 * int(headed)
        policy, digest = make_policy(headed=headed, seed=seed)
        assert policy.input_dim() == cols + 48
        cases.append(weights_case(f"om_sarl_{cols}", policy, seed, digest, cols))
        robots, counts, humans_all, rows, outs = [], [], [], [], []
        for n in (2, 5):
            for _ in range(4):
                while True:
                    robot, humans = g19.draw_state(rng, n, headed)
                    _, pre = om_cases.maps64(humans, 4, 1.0, 3)
                    if not near_integer(pre, 4).any():
                        break
                state = JointState(State(*robot), [(ObsHeaded if headed else Obs)(*h) for h in humans])
                with torch.no_grad():
                    x = policy.transform(state)
                    assert x.dtype == torch.float32 and tuple(x.shape) == (n, cols + 48)
                    v = policy.model(x.unsqueeze(0))
                robots.append(robot)
                counts.append(n)
                humans_all += [h + [0.0] * (7 - len(h)) for h in humans]
                rows.append(x.numpy().astype(F32))
                outs.append(float(v.item()))
        counts = np.array(counts, np.int32)
        print(f"transform {cols} columns: {len(counts)} states, max |V| {float(np.max(np.abs(outs))):.3f}, finite: {bool(np.all(np.isfinite(outs)))}")
        cases.append(dict(kind="transform", wkey=f"om_sarl_{cols}", cols=cols, headed=headed, n=counts,
                          offset=np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32), robot=np.array(robots, np.float64),
                          humans=np.array(humans_all, np.float64)[:, :7 if headed else 5], rows=np.concatenate(rows), out=np.array(outs, F32)))
    return cases


def gen_decisions():
    import torch

    env, _ = mg.make_env("hsfm_farina", "circle_crossing", 5, robot_visible=False)
    seed = 2002
    policy, digest = make_policy(seed=seed)
    policy.set_env(env)
    env.robot.set_policy(policy)
    cases = [weights_case("om_sarl_decide", policy, seed, digest, 13)]
    rec = {"net": []}
    orig_maps = policy.build_occupancy_maps

    def build_maps(human_states):
        out = orig_maps(human_states)
        rec["next"] = np.array([[h.px, h.py, h.vx, h.vy] for h in human_states], np.float64)
        rec["maps"] = out.numpy().astype(F32)
        return out
    policy.build_occupancy_maps = build_maps
    hook = policy.model.register_forward_hook(lambda mod, inp, out: rec["net"].append(float(out.detach().item())))
    rewards = []
    orig_look = env.onestep_lookahead

    def look(action, *a, **k):
        ob, reward = orig_look(action, *a, **k)
        rewards.append(float(reward))
        return ob, reward
    env.onestep_lookahead = look
    try:
        with torch.no_grad():
            for test_case in range(4):
                ob, _ = env.reset(phase="test", test_case=test_case)
                if test_case == 0:      # the parallel branch, as reset leaves the policy: recorded, not described
                    assert policy.parallelize
                    try:
                        env.robot.act(ob)
                        raise AssertionError("the parallel branch decided")
                    except UnboundLocalError as e:
                        cases.append(dict(kind="exception", branch="parallel", type=type(e).__name__, message=str(e)))
                        print("parallel branch:", type(e).__name__, e)
                    ob, _ = env.reset(phase="test", test_case=test_case)
                policy.parallelize = False
                for k in range(8):
                    rec.pop("next", None)
                    rec["net"].clear()
                    rewards.clear()
                    f = env.robot.get_full_state()
                    action = env.robot.act(ob)
                    if "next" not in rec:        # reach_destination: no decision was taken
                        break
                    assert len(rec["net"]) == len(policy.action_space) == len(rewards) == 81
                    values = np.array(policy.action_values, np.float64)
                    cases.append(dict(kind="decision", wkey="om_sarl_decide", test_case=test_case, step=k, n=5, gamma=policy.gamma, dt=env.robot_time_step,
                                      action_space=np.array(policy.action_space_ndarray),
                                      robot=np.array([f.px, f.py, f.vx, f.vy, f.radius, f.gx, f.gy, f.v_pref, f.theta]), obs=mg.ob_to_array(ob),
                                      next_humans=rec["next"], maps=rec["maps"], net_outputs=np.array(rec["net"]), rewards=np.array(rewards),
                                      action_values=values, chosen=int(np.argmax(values)), action=np.array([action.vx, action.vy])))
                    ob, reward, term, trunc, info = env.step(action)
                    if term or trunc:
                        break
    finally:
        hook.remove()
    n_dec = sum(c["kind"] == "decision" for c in cases)
    assert n_dec >= 20, n_dec
    print(f"decisions: {n_dec}, max |net output| {max(float(np.max(np.abs(c['net_outputs']))) for c in cases if c['kind'] == 'decision'):.3f}")
    return cases


def edge_probe():
    """The float32 cell coordinates (dot and cross products with v_i / |v_i|, as the device computes them) against the float64 ones of
    maps64 on 4 000 random crowds: how far apart, whether a pair changes its cell, how many pairs lie within 1e-5 cells of an edge."""
    rng = np.random.default_rng(4000)
    pairs = inside = moved = close = 0
    worst = 0.0
    for _ in range(4000):
        n = int(rng.integers(2, 12))
        h = np.concatenate([rng.uniform(-2.5, 2.5, (n, 2)), rng.uniform(-1, 1, (n, 2))], 1).astype(F32)
        _, pre = om_cases.maps64(h, 4, 1.0, 3)
        speed = np.hypot(h[:, 2], h[:, 3]).astype(F32)
        ux, uy = (h[:, 2] / speed).astype(F32), (h[:, 3] / speed).astype(F32)
        dx, dy = (h[None, :, 0] - h[:, None, 0]).astype(F32), (h[None, :, 1] - h[:, None, 1]).astype(F32)
        x = ((dx * ux[:, None] + dy * uy[:, None]).astype(F32) / F32(1.0) + F32(2.0)).astype(F32)
        y = ((dy * ux[:, None] - dx * uy[:, None]).astype(F32) / F32(1.0) + F32(2.0)).astype(F32)
        pre32 = np.stack([x, y], -1).astype(np.float64)
        off = ~np.eye(n, dtype=bool)
        fl = np.floor(pre[off])
        ins = np.all((fl >= 0) & (fl < 4), axis=-1)
        pairs += int(off.sum())
        inside += int(ins.sum())
        worst = max(worst, float(np.max(np.abs(pre32[off] - pre[off]))))
        moved += int(np.any(np.floor(pre32[off]) != fl, axis=-1).sum())
        close += int(np.any(np.abs(pre[off] - np.round(pre[off])) <= om_cases.EDGE, axis=-1).sum())
    print(f"edge probe: {pairs} pairs, {inside} inside the grid; float32 against float64 pre-floor coordinates: max |diff| {worst:.2e} cells, "
          f"{moved} pairs in another cell, {close} pairs within {om_cases.EDGE} cells of an edge")


if __name__ == "__main__":
    cases = gen_maps() + gen_transform() + gen_decisions()
    edge_probe()
    print("g20_occupancy:", len(cases), "cases ->", save_cases("g20_occupancy", cases))
