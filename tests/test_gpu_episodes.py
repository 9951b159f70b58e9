"""GPU suite of the device episode buffer (crowd_nav/utils/episodes.py over csrc/episodes.hip: cs_episode_append, cs_episode_flush) against
the restatement of tests/episode_cases.py, which tests/test_episodes_cpu.py pins on the reference through G26.

States, rewards, positions, counts and stored targets must be exact.  A return-to-go may differ from the restatement's float32 by one
float32 ulp: both sides sum the same float64 products in the same order, the device's pow is within one float64 ulp of libm's, and a
float64 difference of that size can only move the one final rounding.  Every returns comparison prints how many values were not bit-equal.

Observed on an MI355X: no value of the suite was not bit-equal (G26: 0 of 204 IL values; the edge table: 0 in every row; end to end: 0 of
110)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import episode_cases as ec  # noqa: E402
from golden_io import load_cases  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
GAMMA, DT = 0.9, 0.25


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pair(W, T, capacity, gamma=GAMMA, dt=DT):
    """(device buffer, device memory, restated buffer, restated memory)"""
    from social_navigation_pyenvs_amd.crowd_nav.utils.episodes import EpisodeBuffer
    from social_navigation_pyenvs_amd.crowd_nav.utils.memory import ReplayMemory

    return EpisodeBuffer(W, T, gamma, dt), ReplayMemory(capacity), ec.RefEpisodeBuffer(W, T, gamma, dt), ec.RefMemory(capacity)


def snapshot(memory, dump=None):
    """The ring on the host.  Row `capacity`, where a masked push_batch drops what its mask excludes, is no flush's to write: it must
    hold `dump` (None: the zeros it was allocated with)."""
    import torch

    torch.cuda.synchronize()
    cap = memory.capacity
    states, values = memory.states.cpu().numpy(), memory.values.cpu().numpy()[:, 0]
    if dump is None:
        assert not states[cap].any() and values[cap] == 0.0, "a flush wrote the dump row of masked pushes"
    else:
        assert states[cap].tobytes() == dump[0].tobytes() and values[cap] == dump[1], "a flush wrote the dump row of masked pushes"
    return dict(states=states[:cap], values=values[:cap], position=int(memory._position.item()), length=int(memory._count.item()))


def ulps(a, b):
    """Distance of two float32 arrays in units in the last place (finite values)"""
    def key(x):
        i = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def agree(got, want, mode, what):
    """The memory `got` (snapshot of the device's) is the memory `want` (the restatement's snapshot, or G26's record); returns the number of
    values not bit-equal (0 in "stored" mode, where they must be)."""
    n = want["length"]
    assert (got["position"], got["length"]) == (want["position"], n), what
    assert got["states"][:n].tobytes() == want["states"][:n].tobytes(), what
    assert not got["states"][n:].any() and not got["values"][n:].any(), what
    d = ulps(got["values"][:n], want["values"][:n])
    unequal = int(np.count_nonzero(d))
    assert int(d.max(initial=0)) <= (1 if mode == "returns" else 0), (what, int(d.max()))
    return unequal


G26 = load_cases("g26_episodes")


@pytest.mark.parametrize("k", range(len(G26)))
def test_g26_through_the_buffer(k):
    """The reference's Explorer.update_memory + ReplayMemory on G26's episodes, IL (returns) and RL (stored targets), roomy and wrapping
    twice: the device memory against the reference's own record."""
    c = G26[k]
    lengths = [int(n) for n in c["lengths"]]
    buf, mem, _, _ = pair(len(lengths), max(lengths), c["capacity"], c["gamma"], c["time_step"])
    ec.play_golden(c, buf, mem, dev)
    mode = "returns" if c["mode"] == "il" else "stored"
    want = dict(states=c["mem_states"], values=c["mem_values"], position=c["mem_position"], length=c["mem_length"])
    unequal = agree(snapshot(mem), want, mode, f"G26 case {k}")
    print(f"G26 case {k} ({c['mode']}, capacity {c['capacity']}): {unequal} of {c['mem_length']} values not bit-equal")
    assert len(mem) == c["mem_length"] and mem.is_full() == (c["mem_length"] == c["capacity"])
    assert not buf.cursor.any().item() and not buf.overflowed().any().item()


def figures_agree(buf, ref):
    got, want = buf.figures(time_limit=50.0), ref.figures(time_limit=50.0)
    for key in ("episodes", "success", "collision", "timeout", "success_rate", "collision_rate"):
        assert got[key] == want[key], (key, got, want)
    for key in ("nav_time_sum", "discounted_reward_sum", "avg_nav_time", "avg_discounted_reward"):
        assert abs(got[key] - want[key]) <= 1e-12 * abs(want[key]), (key, got[key], want[key])


@pytest.mark.parametrize("index", range(len(ec.EDGE_CASES)), ids=[f"W{c[0]}-T{c[1]}-{'x'.join(map(str, c[2]))}-{c[3]}" for c in ec.EDGE_CASES])
def test_edge_table(index):
    """One row of tests/episode_cases.py's table (play_edge says what a row does): memory, cursors, overflow flags and figures after the main
    flush and at the end."""
    W, T, shape, kind = ec.EDGE_CASES[index]
    lengths, running, codes, _ = ec.edge_plan(index, W, T)
    capacity = ec.edge_capacity(kind, lengths, running, codes, W)
    buf, mem, rbuf, rmem = pair(W, T, capacity)
    mode = "stored" if index % 2 else "returns"
    seen = []

    def check(tag):
        seen.append((tag, snapshot(mem), buf.cursor.cpu().numpy().copy(), buf.overflowed().cpu().numpy().copy(), buf.figures(50.0)))

    ec.play_edge(index, W, T, shape, buf, mem, dev, check)
    # the restatement, stopped at the same two places
    want = []
    ec.play_edge(index, W, T, shape, rbuf, rmem, check=lambda tag: want.append((tag, rmem.snapshot(), rbuf.cursor(), rbuf.overflow.copy(),
                                                                                 rbuf.figures(50.0))))
    unequal = 0
    for (tag, snap, cursor, overflow, fig), (_, rsnap, rcursor, roverflow, rfig) in zip(seen, want):
        unequal += agree(snap, rsnap, mode, (index, tag))
        assert np.array_equal(cursor, rcursor) and np.array_equal(overflow, roverflow), (index, tag)
        for key in ("episodes", "success", "collision", "timeout"):
            assert fig[key] == rfig[key], (tag, key)
        for key in ("nav_time_sum", "discounted_reward_sum"):
            assert abs(fig[key] - rfig[key]) <= 1e-12 * abs(rfig[key]), (tag, key, fig[key], rfig[key])
    assert len(seen) == len(want) == 2 and len(mem) == len(rmem)
    print(f"edge {index}: W {W} T {T} state {shape} capacity {capacity} ({kind}), {mode}: {unequal} values not bit-equal")


def test_three_flushes_with_a_masked_push_between():
    """Positions, counts and len(memory) carry from a flush through a masked push_batch to the next flush and on."""
    import torch

    W, T, shape, capacity = 5, 4, (2, 13), 23
    buf, mem, rbuf, rmem = pair(W, T, capacity)
    rng = np.random.default_rng(2626)
    dump = None
    for round_ in range(3):
        for _ in range(round_ + 2):
            state, reward = rng.uniform(-1, 1, (W,) + shape).astype(F32), rng.choice(np.array([0.0, -0.0125, 1.0], F32), W)
            buf.append(dev(state), dev(reward))
            rbuf.append(state, reward)
        done, code = rng.random(W) < 0.7, rng.choice([2, 3, 4], W).astype(np.int32)
        done[round_] = True
        code[round_] = 2
        buf.flush(mem, dev(done), dev(code), 0.8)
        rbuf.flush(rmem, done, code, 0.8)
        assert mem._len is None                                   # unknown to the host, as after a masked push
        assert len(mem) == len(rmem) and agree(snapshot(mem, dump), rmem.snapshot(), "returns", f"flush {round_}") >= 0
        states, values, keep = rng.uniform(-1, 1, (W,) + shape).astype(F32), rng.uniform(-1, 1, W).astype(F32), rng.random(W) < 0.5
        keep[round_] = False
        mem.push_batch(dev(states), dev(values), keep=dev(keep))
        rmem.push_batch(states, values, keep)
        dump = (mem.states[capacity].cpu().numpy().copy(), float(mem.values[capacity, 0].item()))     # what the mask dropped: the push's
        assert dump[0].any()
        assert len(mem) == len(rmem) and agree(snapshot(mem, dump), rmem.snapshot(), "returns", f"push {round_}") >= 0
    assert len(mem) == len(rmem) and mem.is_full() == (len(rmem) == capacity)
    assert np.array_equal(buf.cursor.cpu().numpy(), rbuf.cursor())
    figures_agree(buf, rbuf)
    buf.reset()
    assert buf.figures()["episodes"] == 0 and not buf.cursor.any().item()
    assert isinstance(mem.sample(4)[0], torch.Tensor)


def test_a_world_stepped_beyond_max_steps_is_flagged_and_never_stored():
    W, T, shape = 3, 4, (7,)
    buf, mem, rbuf, rmem = pair(W, T, 64)
    rng = np.random.default_rng(2627)

    def step():
        state, reward = rng.uniform(-1, 1, (W,) + shape).astype(F32), rng.choice(np.array([0.0, -0.02, 1.0], F32), W)
        buf.append(dev(state), dev(reward))
        rbuf.append(state, reward)

    def flush(done, code=2):
        buf.flush(mem, dev(np.asarray(done, bool)), dev(np.full(W, code, np.int32)))
        rbuf.flush(rmem, done, np.full(W, code, np.int32))

    for _ in range(3):
        step()
    flush([True, False, True])
    for _ in range(3):
        step()                                                    # world 1 holds 4 steps after the first of these, then overflows twice
    assert buf.overflowed().cpu().tolist() == [0, 1, 0] and buf.cursor.cpu().tolist() == [3, 4, 3]
    flush([True, True, True])
    assert buf.overflowed().cpu().tolist() == [0, 0, 0] and buf.cursor.cpu().tolist() == [0, 0, 0]
    assert len(mem) == 12                                         # 3 + 3, then 3 + 3: nothing of world 1
    agree(snapshot(mem), rmem.snapshot(), "returns", "overflow")
    step()
    step()
    flush([True, True, True], 3)                                  # its next episode is stored like any other
    assert len(mem) == 18
    agree(snapshot(mem), rmem.snapshot(), "returns", "after the overflow")
    figures_agree(buf, rbuf)
    assert buf.figures()["episodes"] == 8


def test_a_world_alone_and_in_a_batch_of_65_gives_the_same_bits():
    T, shape, L = 40, (5, 13), 37
    rng = np.random.default_rng(2628)
    states = rng.uniform(-2, 2, (L, 65) + shape).astype(F32)
    rewards = rng.choice(np.array([0.0, -0.0125, -0.00625, 1.0, -0.25], F32), (L, 65))
    v_pref = rng.choice([0.8, 1.0, 1.3], 65)
    out = []
    for W in (1, 65):
        buf, mem, _, _ = pair(W, T, 65 * T)
        for t in range(L):
            buf.append(dev(states[t, :W]), dev(rewards[t, :W]))
        buf.flush(mem, dev(np.ones(W, bool)), dev(np.full(W, 3, np.int32)), dev(v_pref[:W]))
        snap = snapshot(mem)
        assert snap["length"] == W * L
        out.append((snap["states"][:L].tobytes(), snap["values"][:L].tobytes()))
    assert out[0] == out[1]


E2E = dict(W=64, humans=5, rounds=12, time_limit="2", sim="circle_crossing", radius="2.5")


def test_end_to_end_with_the_resident_worlds():
    """64 worlds x 5 humans on a small crossing circle with a time limit of 2 s (eight steps), a seeded SARL, 12 rounds of act_device,
    joint_state_device, step_device(auto_reset=True), value_device(bootstrap) and append, a flush after every round -- into one memory with
    the stored targets (RL) and into another with the returns (IL).  Every round's tensors also go to the host and through the
    restatement: the memories must be identical, with episodes dropped as Timeouts and episodes kept among them."""
    import copy

    import torch
    from test_gpu_generators import _config
    from test_gpu_value_policy import _calm, _ready
    from test_value_policy_cpu import make_policy, seeded_weights

    from social_navigation_pyenvs_amd.crowd_nav.utils.episodes import EpisodeBuffer
    from social_navigation_pyenvs_amd.crowd_nav.utils.memory import ReplayMemory
    from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym

    W = E2E["W"]
    cfg = _config(E2E["sim"], human_num=E2E["humans"], policy="sfm_guo")
    cfg.set("env", "time_limit", E2E["time_limit"])
    cfg.set("sim", "circle_radius", E2E["radius"])
    env = BatchedSocialNavGym(cfg, W)
    env.reset(phase="test", first_case=11, device=True)
    policy = _ready(make_policy("sarl"), env)
    seeded_weights(policy.model, 2629)
    _calm(policy)
    target = copy.deepcopy(policy.model)
    T = 16
    bufs = {m: EpisodeBuffer(W, T, GAMMA, env.robot_time_step) for m in ("stored", "returns")}
    mems = {m: ReplayMemory(150) for m in bufs}
    rbufs = {m: ec.RefEpisodeBuffer(W, T, GAMMA, env.robot_time_step) for m in bufs}
    rmems = {m: ec.RefMemory(150) for m in bufs}
    outcomes = np.zeros(5, int)
    with torch.cuda.stream(env.device_stream()):
        for _ in range(E2E["rounds"]):
            action = env.act_device(policy)
            state = env.joint_state_device(policy)
            _, reward, terminated, truncated, info = env.step_device(action, auto_reset=True)
            boot = env.value_device(policy, model=target, rewards=reward, bootstrap=True)
            done = terminated | truncated
            tgt = torch.where(done, reward, boot)
            for m in bufs:
                bufs[m].append(state, reward, tgt if m == "stored" else None)
                bufs[m].flush(mems[m], done, info, 1.0, m)
            env.device_stream().synchronize()
            h = [t.cpu().numpy().copy() for t in (state, reward, tgt, done, info)]
            outcomes += np.bincount(h[4][h[3]], minlength=5)[:5]
            for m in bufs:
                rbufs[m].append(h[0], h[1], h[2] if m == "stored" else None)
                rbufs[m].flush(rmems[m], h[3], h[4], 1.0, m)
    print(f"end to end: outcomes by code {outcomes.tolist()}, {len(rmems['stored'])} samples in the memory")
    for m in bufs:
        unequal = agree(snapshot(mems[m]), rmems[m].snapshot(), m, f"end to end, {m}")
        print(f"end to end, {m}: {unequal} of {len(rmems[m])} values not bit-equal")
        assert np.array_equal(bufs[m].cursor.cpu().numpy(), rbufs[m].cursor())
        figures_agree(bufs[m], rbufs[m])
    assert outcomes[4] > 0 and outcomes[2] + outcomes[3] > 0 and len(rmems["stored"]) > 0, outcomes
    env.close()


def test_the_imitation_learning_loop_of_the_integration_guide():
    """INTEGRATION.md's IL loop on 16 worlds: a no-train policy drives the robots, the value policy's transform gives the states, the
    flush stores returns; the restatement fed with the same tensors holds the same memory and gives the same figures."""
    import torch
    from test_gpu_generators import _config
    from test_gpu_value_policy import _ready
    from test_value_policy_cpu import make_policy

    from social_navigation_pyenvs_amd.crowd_nav.utils.episodes import EpisodeBuffer
    from social_navigation_pyenvs_amd.crowd_nav.utils.memory import ReplayMemory
    from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym

    W = 16
    cfg = _config(E2E["sim"], human_num=E2E["humans"], policy="sfm_guo")
    cfg.set("env", "time_limit", "8")                     # 32 steps: most episodes end before the limit (on the small circle, in collisions)
    cfg.set("sim", "circle_radius", E2E["radius"])
    env = BatchedSocialNavGym(cfg, W)
    env.reset(phase="test", first_case=3, device=True)
    policy = _ready(make_policy("sarl"), env)
    T = int(env.time_limit / env.robot_time_step) + 1
    buf, memory, rbuf, rmem = pair(W, T, 40, GAMMA, env.robot_time_step)
    with torch.cuda.stream(env.device_stream()):
        for _ in range(40):
            state = env.joint_state_device(policy)
            obs, reward, terminated, truncated, info = env.step_device(env.act_device("sfm_helbing"), auto_reset=True)
            buf.append(state, reward)
            buf.flush(memory, terminated | truncated, info, v_pref=1.0, targets="returns")
            env.device_stream().synchronize()
            h = [t.cpu().numpy().copy() for t in (state, reward, terminated | truncated, info)]
            rbuf.append(h[0], h[1])
            rbuf.flush(rmem, h[2], h[3], 1.0, "returns")
    fig = buf.figures(time_limit=env.time_limit)
    print(f"imitation loop: {fig}")
    assert fig["episodes"] >= W and fig["success"] + fig["collision"] > 0 and not buf.overflowed().any().item()
    unequal = agree(snapshot(memory), rmem.snapshot(), "returns", "imitation loop")
    print(f"imitation loop: {unequal} of {len(rmem)} values not bit-equal")
    assert len(memory) == len(rmem) > 0
    figures_agree(buf, rbuf)
    env.close()
