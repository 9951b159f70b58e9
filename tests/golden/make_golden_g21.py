#!/usr/bin/env python3
"""Generate tests/golden/g21_lstm_rl.npz by RUNNING THE REFERENCE's LSTM-RL (crowd_nav/policy/lstm_rl.py): both of its networks on seeded
rows, its ``transform``, and its decisions in its own Gym.

TEST INFRASTRUCTURE ONLY.  Run from the repo root:  python tests/golden/make_golden_g21.py

The reference is imported through make_golden.py's harness; only numbers (inputs and what the reference produced) and short names are
written.  Weights are recorded as seed + key order + SHA-256 (tests/lstm_cases.py draw_weights: om_cases.draw_weights(calm=True), and
with ``calm_last`` mlp's output layer times 0.1).  Case kinds:

  "weights"   one per network: ValueNetwork1 on 13 columns ("lstm1_13") and on 15 ("lstm1_15"), ValueNetwork2 on 13 ("lstm2_13")
  "forward"   per network seeded rows [B, n, cols] for n in {1, 2, 5, 9}, in the order given, and the reference module's outputs
  "transform" per network states, the reference's transform(state) rows (the humans' own order: the reference sorts in predict only) and
              model(rows[None])
  "decision"  the reference LSTM-RL deciding in its own Gym (hsfm_farina, circle crossing, 5 humans, robot_visible=False, as G16) through
              the PARALLEL branch, as reset leaves the policy, 4 test cases x up to 12 steps for "lstm1_13" and "lstm2_13": the robot's full
              state, the observation, the next human states, the 81 network outputs, rewards and action values, the arg-max and the
              action.  The rotated tensor is not recorded (cs_lookahead rebuilds it, as for G16 / G20).  The SERIAL branch
              (parallelize = False) is asserted to pick the same action on the same state.

Two conditions are asserted and printed per decision network; a seed is redrawn (+10) until they hold, and when six seeds fail mlp's output
layer is calmed (``calm_last``):
  (a) in every (decision, action) the two closest distances of column 11 differ by more than 1e-5 m: the float32 order is the float64 order;
  (b) the smallest gap between the best and the second-best action value, computed with lstm_cases' float64 restatement of the network,
      is at least 8 x E_ref, E_ref the largest difference between the reference's float32 module and that restatement over the network's
      decisions.
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
import lstm_cases  # noqa: E402
import make_golden_g19 as g19  # noqa: E402
from golden_io import save_cases  # noqa: E402

ns = mg.ns
F32 = np.float32
DA_GAP = 1e-5
MARGIN = 8.0


def make_policy(network, headed, seed, calm_last=False):
    import torch
    from crowd_nav.policy.policy_factory import policy_factory

    pcfg = configparser.RawConfigParser()
    pcfg.read(os.path.join(_refharness.REFERENCE_ROOT, "crowd_nav", "configs", "policy.config"))
    pcfg.set("lstm_rl", "with_interaction_module", "true" if network == 2 else "false")
    pcfg.set("sarl", "with_theta_and_omega_visible", "true" if headed else "false")
    policy = policy_factory["lstm_rl"]()
    policy.configure(pcfg)
    assert policy.name == "LSTM-RL" and type(policy.model).__name__ == f"ValueNetwork{network}"
    digest = lstm_cases.draw_weights(policy.model, seed, calm_last)
    policy.set_device(torch.device("cpu"))
    policy.set_phase("test")
    return policy, digest


def weights_case(wkey, network, policy, seed, calm_last, digest, cols):
    sd = policy.model.state_dict()
    return dict(kind="weights", wkey=wkey, network=network, cols=cols, seed=seed, calm=True, calm_last=calm_last, sha256=digest,
                weights_keys=sorted(str(k) for k in sd.keys()), weights_shapes=[list(sd[k].shape) for k in sorted(sd.keys())])


def gen_forward(wkey, policy, cols, rng):
    import torch

    cases = []
    for n in (1, 2, 5, 9):
        rows = rng.uniform(-2.0, 2.0, (6, n, cols)).astype(F32)
        rows[..., 11] = np.abs(rows[..., 11]) + F32(0.3)
        with torch.no_grad():
            out = policy.model(torch.from_numpy(rows))
        assert tuple(out.shape) == (6, 1)
        cases.append(dict(kind="forward", wkey=wkey, cols=cols, n=n, rows=rows, out=out[:, 0].numpy().astype(F32)))
    return cases


def gen_transform(wkey, policy, cols, rng):
    import torch
    from crowd_nav.utils.state import JointState

    State, Obs, ObsHeaded = ns.state.FullState, ns.state.ObservableState, ns.state.ObservableStateHeaded
    headed = cols == 15
    robots, counts, humans_all, rows, outs = [], [], [], [], []
    for n in (1, 2, 5):
        for _ in range(3):
            robot, humans = g19.draw_state(rng, n, headed)
            state = JointState(State(*robot), [(ObsHeaded if headed else Obs)(*h) for h in humans])
            with torch.no_grad():
                x = policy.transform(state)
                assert x.dtype == torch.float32 and tuple(x.shape) == (n, cols)
                v = policy.model(x.unsqueeze(0))
            robots.append(robot)
            counts.append(n)
            humans_all += [h + [0.0] * (7 - len(h)) for h in humans]
            rows.append(x.numpy().astype(F32))
            outs.append(float(v.item()))
    counts = np.array(counts, np.int32)
    return [dict(kind="transform", wkey=wkey, cols=cols, headed=headed, n=counts, offset=np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32),
                 robot=np.array(robots, np.float64), humans=np.array(humans_all, np.float64)[:, :7 if headed else 5], rows=np.concatenate(rows),
                 out=np.array(outs, F32))]


def run_decisions(wkey, network, seed, calm_last):
    """The reference deciding with the network of (seed, calm_last): (policy, digest, decision cases, statistics)."""
    import torch
    import crowd_nav.policy.multi_human_rl as mh_mod

    env, _ = mg.make_env("hsfm_farina", "circle_crossing", 5, robot_visible=False)
    policy, digest = make_policy(network, False, seed, calm_last)
    policy.set_env(env)
    env.robot.set_policy(policy)
    w64 = lstm_cases.weights64(policy.model)
    rec = {}
    orig_peek = env.motion_model_manager.__class__.get_next_human_observable_states
    orig_cav, orig_rot = mh_mod.compute_action_value, mh_mod.compute_rotated_states_and_reward

    def cav(rewards, outs, dt, gamma, vpref):
        v = orig_cav(rewards, outs, dt, gamma, vpref)
        rec["values"], rec["rewards"], rec["net"], rec["discount"] = np.array(v), np.array(rewards), np.array(outs), pow(gamma, dt * vpref)
        return v

    def rot(*a, **k):
        out = orig_rot(*a, **k)
        rec["rotated"] = np.array(out[0], np.float64)
        return out
    mh_mod.compute_action_value, mh_mod.compute_rotated_states_and_reward = cav, rot
    cases, e_ref, min_da, min_gap, vmax, flips = [], 0.0, np.inf, np.inf, 0.0, 0
    try:
        with torch.no_grad():
            for test_case in range(4):
                ob, _ = env.reset(phase="test", test_case=test_case)
                assert policy.parallelize
                mm = env.motion_model_manager

                def peek(self, dt, theta_and_omega_visible=False, _o=orig_peek):
                    r = _o(self, dt, theta_and_omega_visible)
                    rec["next"] = np.array(r)
                    return r
                mm.__class__.get_next_human_observable_states = peek
                for k in range(12):
                    rec.clear()
                    f = env.robot.get_full_state()
                    rng_state = np.random.get_state()
                    action = env.robot.act(ob)
                    if "values" not in rec:      # reach_destination: no decision was taken
                        break
                    keep = dict(rec)
                    np.random.set_state(rng_state)          # the serial branch on the same state, from the same numpy stream
                    policy.parallelize = False
                    serial = env.robot.act(ob)
                    policy.parallelize = True
                    assert (serial.vx, serial.vy) == (action.vx, action.vy), (test_case, k, serial, action)
                    rotated = keep["rotated"]
                    assert rotated.shape == (81, 5, 13)
                    da = np.sort(rotated[..., 11], axis=1)
                    min_da = min(min_da, float(np.min(np.diff(da, axis=1))))
                    flips += int(np.any(lstm_cases.decision_order(rotated[..., 11]) != lstm_cases.decision_order(rotated[..., 11].astype(F32))))
                    v64 = lstm_cases.forward64(w64, lstm_cases.sort_rows(rotated.astype(F32).astype(np.float64)))
                    e_ref = max(e_ref, float(np.max(np.abs(keep["net"] - v64))))
                    vmax = max(vmax, float(np.max(np.abs(v64))))
                    top = np.sort(keep["rewards"] + keep["discount"] * v64)
                    min_gap = min(min_gap, float(top[-1] - top[-2]))
                    cases.append(dict(kind="decision", wkey=wkey, test_case=test_case, step=k, n=5, gamma=policy.gamma, dt=env.robot_time_step,
                                      action_space=np.array(policy.action_space_ndarray),
                                      robot=np.array([f.px, f.py, f.vx, f.vy, f.radius, f.gx, f.gy, f.v_pref, f.theta]), obs=mg.ob_to_array(ob),
                                      next_humans=keep["next"], net_outputs=keep["net"], rewards=keep["rewards"], action_values=keep["values"],
                                      chosen=int(np.argmax(keep["values"])), action=np.array([action.vx, action.vy])))
                    ob, reward, term, trunc, info = env.step(action)
                    if term or trunc:
                        break
    finally:
        mh_mod.compute_action_value, mh_mod.compute_rotated_states_and_reward = orig_cav, orig_rot
        env.motion_model_manager.__class__.get_next_human_observable_states = orig_peek
    stats = dict(decisions=len(cases), min_da=min_da, flips=flips, e_ref=e_ref, vmax=vmax, min_gap=min_gap)
    return policy, digest, cases, stats


def gen_network(wkey, network, first_seed):
    """The decisions of one network with the first (seed, calm_last) that meets conditions (a) and (b); then its forward and transform cases."""
    for calm_last in (False, True):
        for seed in range(first_seed, first_seed + 60, 10):
            policy, digest, decisions, st = run_decisions(wkey, network, seed, calm_last)
            ok_a = st["min_da"] > DA_GAP and st["flips"] == 0
            ok_b = st["min_gap"] >= MARGIN * st["e_ref"]
            print(f"{wkey} seed {seed} calm_last {calm_last}: {st['decisions']} decisions, min da gap {st['min_da']:.2e} m, f32 sort orders differing "
                  f"{st['flips']}, E_ref {st['e_ref']:.2e}, |V| up to {st['vmax']:.1f}, min top-two gap {st['min_gap']:.2e}, ratio "
                  f"{st['min_gap'] / st['e_ref']:.1f}: (a) {'holds' if ok_a else 'FAILS'}, (b) {'holds' if ok_b else 'FAILS'}")
            if ok_a and ok_b and st["decisions"] >= 20:
                assert st["min_da"] > DA_GAP and st["min_gap"] >= MARGIN * st["e_ref"]
                rng = np.random.default_rng(2100 + network)
                return ([weights_case(wkey, network, policy, seed, calm_last, digest, 13)] + gen_forward(wkey, policy, 13, rng)
                        + gen_transform(wkey, policy, 13, rng) + decisions + [dict(kind="conditions", wkey=wkey, **st)])
    raise AssertionError(f"{wkey}: no seed met the conditions")


if __name__ == "__main__":
    cases = gen_network("lstm1_13", 1, 2101) + gen_network("lstm2_13", 2, 2102)
    policy, digest = make_policy(1, True, 2111)
    rng = np.random.default_rng(2111)
    cases += [weights_case("lstm1_15", 1, policy, 2111, False, digest, 15)] + gen_forward("lstm1_15", policy, 15, rng) + gen_transform("lstm1_15", policy, 15, rng)
    print("g21_lstm_rl:", len(cases), "cases ->", save_cases("g21_lstm_rl", cases))
