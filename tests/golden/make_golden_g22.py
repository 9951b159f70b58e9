#!/usr/bin/env python3
"""Generate tests/golden/g22_om_lstm_rl.npz by RUNNING THE REFERENCE's OM-LSTM-RL (crowd_nav/policy/lstm_rl.py with ``lstm_rl.with_om =
true``): both of its networks on seeded wide rows, its ``transform``, and its decisions in its own Gym.

TEST INFRASTRUCTURE ONLY.  Run from the repo root:  python tests/golden/make_golden_g22.py

The reference is imported through make_golden.py's harness; only numbers (inputs and what the reference produced) and short names are
written.  Weights are recorded as seed + key order + SHA-256 (tests/lstm_cases.py draw_weights).  Case kinds:

  "weights"   one per network: ValueNetwork1 on 13 + 48 columns ("omlstm1_13") and on 15 + 48 ("omlstm1_15"), ValueNetwork2 on 13 + 48
              ("omlstm2_13"); the reference keeps the name "LSTM-RL"
  "forward"   per network seeded wide rows [B, n, cols + 48] for n in {2, 5, 9}, in the order given, and the reference module's outputs
  "transform" per network states, the reference's transform(state) rows [n, cols + 48] (the humans' own order, every human beside its own
              map) and model(rows[None])
  "decision"  the reference deciding in its own Gym (hsfm_farina, circle crossing, 5 humans, robot_visible=False, as G21) through the SERIAL
              branch (policy.parallelize = False after reset) for "omlstm1_13" and "omlstm2_13": the first ten test cases x up to 12 steps are
              run, and the KEEP = 2 test cases with the most decisions in which some action reorders the humans are kept (ties: the lower
              test case).  Whether an action reorders them is a matter of the layout and of where the robot has gone -- two humans about
              equally far from it --, a property of the decision's inputs; in most test cases next to no action does (condition c).  Kept: the robot's
              full state, the observation, the unsorted next human states (the same for all 81 actions: the robot is invisible), what the
              reference handed to its network -- ``order0``, the order of the humans it built the maps on (the first action's sorted humans),
              ``maps`` [n, 48] as build_occupancy_maps returned them, in that order, ``orders`` [81, n] the order of every action's rows --,
              the 81 network outputs, rewards and action values, the arg-max and the action.  build_occupancy_maps is called ONCE per
              decision (asserted).
  "exception" what the PARALLEL branch (policy.parallelize = True, as SocialNavGym.reset leaves it) raises
  "conditions" per decision network, the statistics below

Three conditions are asserted and printed per decision network; a seed is redrawn (+10) until they hold, and when six seeds fail mlp's
output layer is calmed (``calm_last``):
  (a) in every (decision, action) the two closest distances of column 11 differ by more than 1e-5 m and the float32 order is the float64
      order: the order is no matter of rounding (nor of the tie rule: the reference's ``sorted`` keeps tied humans in ascending order);
  (b) the smallest gap between the best and the second-best action value under om_lstm_cases' float64 restatement with the reference's
      pairing is at least 8 x E_ref, E_ref the largest difference between the reference's network outputs and that restatement;
  (c) in at least half of the decisions some action's order differs from action 0's, and in at least one decision the restatement with the
      OWN pairing differs from the recorded values by more than 100 x E_ref: the pairing is observable.
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
import om_cases  # noqa: E402
import om_lstm_cases as olc  # noqa: E402
import make_golden_g19 as g19  # noqa: E402
from golden_io import save_cases  # noqa: E402

ns = mg.ns
F32 = np.float32
DA_GAP = 1e-5
MARGIN = 8.0
C = 48
TEST_CASES, KEEP, STEPS = range(10), 2, 12


def make_policy(network, headed, seed, calm_last=False):
    import torch
    from crowd_nav.policy.policy_factory import policy_factory

    pcfg = configparser.RawConfigParser()
    pcfg.read(os.path.join(_refharness.REFERENCE_ROOT, "crowd_nav", "configs", "policy.config"))
    pcfg.set("lstm_rl", "with_om", "true")
    pcfg.set("lstm_rl", "with_interaction_module", "true" if network == 2 else "false")
    pcfg.set("sarl", "with_theta_and_omega_visible", "true" if headed else "false")
    policy = policy_factory["lstm_rl"]()
    policy.configure(pcfg)
    assert policy.name == "LSTM-RL" and policy.with_om and type(policy.model).__name__ == f"ValueNetwork{network}"
    assert policy.input_dim() == (15 if headed else 13) + C
    digest = lstm_cases.draw_weights(policy.model, seed, calm_last)
    policy.set_device(torch.device("cpu"))
    policy.set_phase("test")
    return policy, digest


def weights_case(wkey, network, policy, seed, calm_last, digest, cols):
    sd = policy.model.state_dict()
    return dict(kind="weights", wkey=wkey, network=network, cols=cols, om_cols=C, name=policy.name, seed=seed, calm=True, calm_last=calm_last,
                sha256=digest, weights_keys=sorted(str(k) for k in sd.keys()), weights_shapes=[list(sd[k].shape) for k in sorted(sd.keys())])


def gen_forward(wkey, policy, cols, rng):
    import torch

    cases = []
    for n in (2, 5, 9):
        rows = rng.uniform(-2.0, 2.0, (6, n, cols + C)).astype(F32)
        rows[..., 11] = np.abs(rows[..., 11]) + F32(0.3)
        rows[..., cols::3] = (rows[..., cols::3] > 0).astype(F32)             # the occupancy channel: 0 or 1
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
    for n in (2, 5):
        for _ in range(3):
            while True:
                robot, humans = g19.draw_state(rng, n, headed)
                _, pre = om_cases.maps64(humans, 4, 1.0, 3)
                if not om_cases.near_edge(pre, 4).any():
                    break
            state = JointState(State(*robot), [(ObsHeaded if headed else Obs)(*h) for h in humans])
            with torch.no_grad():
                x = policy.transform(state)
                assert x.dtype == torch.float32 and tuple(x.shape) == (n, cols + C)
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


def order_of(handed, unsorted):
    """the indices into `unsorted` [n, 4] of the human states `handed` (matched by their exact positions, which must be distinct)"""
    idx = [int(np.flatnonzero((unsorted[:, 0] == h[0]) & (unsorted[:, 1] == h[1]))[0]) for h in handed]
    assert sorted(idx) == list(range(len(unsorted)))
    return np.array(idx, np.int32)


def run_decisions(wkey, network, seed, calm_last, exceptions):
    """The reference deciding with the network of (seed, calm_last): (policy, digest, decision cases, statistics)."""
    import torch

    env, _ = mg.make_env("hsfm_farina", "circle_crossing", 5, robot_visible=False)
    policy, digest = make_policy(network, False, seed, calm_last)
    policy.set_env(env)
    env.robot.set_policy(policy)
    w64 = lstm_cases.weights64(policy.model)
    rec = {"net": [], "inputs": [], "maps": [], "looks": []}
    orig_maps = policy.build_occupancy_maps

    def build_maps(human_states):
        out = orig_maps(human_states)
        rec["maps"].append((np.array([[h.px, h.py, h.vx, h.vy] for h in human_states], np.float64), out.numpy().astype(F32)))
        return out
    policy.build_occupancy_maps = build_maps

    def fwd(mod, inp, out):
        rec["net"].append(float(out.detach().item()))
        rec["inputs"].append(inp[0].detach().numpy()[0].astype(F32))
    hook = policy.model.register_forward_hook(fwd)
    orig_look = env.onestep_lookahead

    def look(action, *a, **k):
        ob, reward = orig_look(action, *a, **k)
        rec["looks"].append((np.array([[h.px, h.py, h.vx, h.vy] for h in ob], np.float64), float(reward)))
        return ob, reward
    env.onestep_lookahead = look
    cases = []
    try:
        with torch.no_grad():
            for test_case in TEST_CASES:
                ob, _ = env.reset(phase="test", test_case=test_case)
                if test_case == TEST_CASES[0] and exceptions is not None:      # the parallel branch, as reset leaves the policy: recorded, not described
                    assert policy.parallelize
                    try:
                        env.robot.act(ob)
                        raise AssertionError("the parallel branch decided")
                    except UnboundLocalError as e:
                        exceptions.append(dict(kind="exception", wkey=wkey, branch="parallel", type=type(e).__name__, message=str(e)))
                        print("parallel branch:", type(e).__name__, e)
                    ob, _ = env.reset(phase="test", test_case=test_case)
                policy.parallelize = False
                for k in range(STEPS):
                    for v in rec.values():
                        v.clear()
                    f = env.robot.get_full_state()
                    action = env.robot.act(ob)
                    if not rec["net"]:           # reach_destination: no decision was taken
                        break
                    A = len(policy.action_space)
                    assert len(rec["net"]) == len(rec["looks"]) == A == 81 and len(rec["maps"]) == 1      # the maps are built ONCE
                    nxt = rec["looks"][0][0]
                    assert all(np.array_equal(nh, nxt) for nh, _ in rec["looks"])                         # the robot is invisible
                    handed, maps = rec["maps"][0]
                    order0 = order_of(handed, nxt)
                    inputs = np.stack(rec["inputs"])                                                      # [81, n, 61] what the network read
                    assert all(np.array_equal(inputs[a, :, 13:], maps) for a in range(A))                 # attached by position
                    rewards = np.array([r for _, r in rec["looks"]])
                    values = np.array(policy.action_values, np.float64)
                    case = dict(kind="decision", wkey=wkey, test_case=test_case, step=k, n=5, gamma=policy.gamma, dt=env.robot_time_step,
                                action_space=np.array(policy.action_space_ndarray),
                                robot=np.array([f.px, f.py, f.vx, f.vy, f.radius, f.gx, f.gy, f.v_pref, f.theta]), obs=mg.ob_to_array(ob),
                                next_humans=nxt, order0=order0, maps=maps, net_outputs=np.array(rec["net"]), rewards=rewards, action_values=values,
                                chosen=int(np.argmax(values)), action=np.array([action.vx, action.vy]))
                    ref_v, ref_net, rot, own_maps = olc.restate_decision(w64, case, "reference")
                    own_v = olc.restate_decision(w64, case, "own")[0]
                    orders = lstm_cases.decision_order(rot[..., 11])
                    # the rows the reference handed over are the restatement's rows in the restatement's order (float32 against float64)
                    assert np.array_equal(orders[0], order0), (orders[0], order0)
                    assert float(np.max(np.abs(inputs[..., :13] - np.take_along_axis(rot, orders[..., None], axis=1)))) < 1e-4
                    assert float(np.max(np.abs(maps - own_maps[order0]))) < 1e-5
                    case["orders"] = orders.astype(np.int32)
                    da = np.sort(rot[..., 11], axis=1)
                    top = np.sort(ref_v)
                    case["_st"] = dict(min_da=float(np.min(np.diff(da, axis=1))), flip=int(np.any(orders != lstm_cases.decision_order(rot[..., 11].astype(F32)))),
                                       reordered=int(np.any(orders != orders[:1])), e=float(np.max(np.abs(case["net_outputs"] - ref_net))),
                                       vmax=float(np.max(np.abs(ref_net))), own=float(np.max(np.abs(own_v - values))), gap=float(top[-1] - top[-2]),
                                       same_pick=int(np.argmax(ref_v)) == case["chosen"])
                    cases.append(case)
                    ob, reward, term, trunc, info = env.step(action)
                    if term or trunc:
                        break
    finally:
        hook.remove()
    count = {tc: sum(c["_st"]["reordered"] for c in cases if c["test_case"] == tc) for tc in TEST_CASES}
    kept = sorted(sorted(TEST_CASES, key=lambda tc: (-count[tc], tc))[:KEEP])
    cases = [c for c in cases if c["test_case"] in kept]
    sts = [c.pop("_st") for c in cases]
    stats = dict(decisions=len(cases), test_cases=[int(tc) for tc in kept], min_da=min(s["min_da"] for s in sts), flips=sum(s["flip"] for s in sts),
                 e_ref=max(s["e"] for s in sts), vmax=max(s["vmax"] for s in sts), min_gap=min(s["gap"] for s in sts),
                 reordered=sum(s["reordered"] for s in sts), own_diff=max(s["own"] for s in sts))
    assert all(s["same_pick"] or s["gap"] < MARGIN * stats["e_ref"] for s in sts)
    return policy, digest, cases, stats


def gen_network(wkey, network, first_seed, exceptions):
    """The decisions of one network with the first (seed, calm_last) that meets conditions (a), (b) and (c); then its forward and transform cases."""
    for calm_last in (False, True):
        for seed in range(first_seed, first_seed + 60, 10):
            exc = [] if exceptions is not None and not exceptions else None
            policy, digest, decisions, st = run_decisions(wkey, network, seed, calm_last, exc)
            if exc:
                exceptions += exc
            ok_a = st["min_da"] > DA_GAP and st["flips"] == 0
            ok_b = st["min_gap"] >= MARGIN * st["e_ref"]
            ok_c = 2 * st["reordered"] >= st["decisions"] and st["own_diff"] > 100 * st["e_ref"]
            print(f"{wkey} seed {seed} calm_last {calm_last}: test cases {st['test_cases']}, {st['decisions']} decisions, min da gap {st['min_da']:.2e} m, f32 sort orders differing "
                  f"{st['flips']}, E_ref {st['e_ref']:.2e}, |V| up to {st['vmax']:.1f}, min top-two gap {st['min_gap']:.2e} (ratio "
                  f"{st['min_gap'] / st['e_ref']:.1f}), {st['reordered']} decisions with an order other than action 0's, own pairing off by up to "
                  f"{st['own_diff']:.2e} (ratio {st['own_diff'] / st['e_ref']:.0f}): (a) {'holds' if ok_a else 'FAILS'}, (b) "
                  f"{'holds' if ok_b else 'FAILS'}, (c) {'holds' if ok_c else 'FAILS'}")
            if ok_a and ok_b and ok_c and st["decisions"] >= 20:
                rng = np.random.default_rng(2200 + network)
                return ([weights_case(wkey, network, policy, seed, calm_last, digest, 13)] + gen_forward(wkey, policy, 13, rng)
                        + gen_transform(wkey, policy, 13, rng) + decisions + [dict(kind="conditions", wkey=wkey, **st)])
    raise AssertionError(f"{wkey}: no seed met the conditions")


if __name__ == "__main__":
    exceptions = []
    cases = gen_network("omlstm1_13", 1, 2201, exceptions) + gen_network("omlstm2_13", 2, 2202, None)
    assert len(exceptions) == 1
    policy, digest = make_policy(1, True, 2211)
    rng = np.random.default_rng(2211)
    cases += [weights_case("omlstm1_15", 1, policy, 2211, False, digest, 15)] + gen_forward("omlstm1_15", policy, 15, rng) + gen_transform("omlstm1_15", policy, 15, rng)
    cases += exceptions
    print("g22_om_lstm_rl:", len(cases), "cases ->", save_cases("g22_om_lstm_rl", cases))
