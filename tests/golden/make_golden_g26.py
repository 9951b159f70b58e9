#!/usr/bin/env python3
"""Generate tests/golden/g26_episodes.npz by RUNNING THE REFERENCE's ``Explorer.update_memory`` and ``ReplayMemory`` on seeded synthetic
episodes.

TEST INFRASTRUCTURE ONLY.  Run from the repo root:  python tests/golden/make_golden_g26.py

The reference is imported through make_golden.py's harness; only numbers are written.  An Explorer is built around a stub robot that carries
``time_step`` and ``desired_speed``, a target policy whose ``transform`` is the identity on tensors and, for RL, a target model that is a
tiny seeded ``nn.Linear`` on the flattened state.  An episode is a list of [2, 13] float32 states and of rewards drawn from the Gym's own
values -- 0, the discomfort term (d - 0.2) * 0.5 * time_step for a few distances d < 0.2, and at the last step 1 (ReachGoal), -0.25
(Collision) or whatever the step gave (Timeout) -- rounded to float32, the store's precision, and handed to the reference as Python floats.
Episodes go through ``update_memory`` in order when their outcome is ReachGoal or Collision, the filter of ``run_k_episodes``
(explorer.py:94-97).  Per case:

  mode, capacity, gamma, time_step, desired_speed
  lengths, codes [E]        the episodes: number of steps, outcome code (2 ReachGoal, 3 Collision, 4 Timeout)
  states, rewards [sum L]   the steps of all episodes, concatenated
  targets [sum L]           what update_memory stores for every step of every episode (Timeouts too, through a memory of their own): the
                            return-to-go for IL, reward + gamma^(time_step desired_speed) target_model(next state) for RL
  mem_states, mem_values    the reference memory's samples in list order, mem_position, mem_length
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401  (imports the reference through _refharness)
from golden_io import save_cases  # noqa: E402

F32 = np.float32
GAMMA, TIME_STEP = 0.9, 0.25
# (mode, desired_speed, capacity, [(length, code) ...]); 2 ReachGoal, 3 Collision, 4 Timeout
CASES = [
    ("il", 1.0, 400, [(1, 3), (100, 2), (7, 4), (13, 2), (30, 3)]),          # 144 samples kept, room for all
    ("il", 0.8, 60, [(100, 2), (1, 2), (9, 4), (22, 3), (30, 2), (1, 3)]),   # 154 kept in 60 slots: wraps twice
    ("rl", 1.0, 400, [(100, 3), (1, 2), (5, 4), (17, 2)]),
    ("rl", 0.8, 50, [(12, 2), (100, 2), (1, 4), (1, 3), (26, 3)]),           # 139 kept in 50 slots: wraps twice
]


class Stub:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def generate():
    import torch
    from crowd_nav.utils.explorer import Explorer
    from crowd_nav.utils.memory import ReplayMemory

    cases = []
    for k, (mode, speed, capacity, episodes) in enumerate(CASES):
        rng = np.random.default_rng(2600 + k)
        torch.manual_seed(2600 + k)
        robot = Stub(time_step=TIME_STEP, desired_speed=speed, v_pref=speed)
        memory = ReplayMemory(capacity)
        explorer = Explorer(None, robot, torch.device("cpu"), memory, GAMMA, Stub(transform=lambda state: state))
        explorer.target_model = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(26, 1))
        states, rewards, targets = [], [], []
        for length, code in episodes:
            s = rng.uniform(-2, 2, (length, 2, 13)).astype(F32)
            discomfort = ((rng.uniform(0.0, 0.2, length) - 0.2) * 0.5 * TIME_STEP).astype(F32)
            r = np.where(rng.random(length) < 0.3, discomfort, F32(0.0)).astype(F32)
            if code != 4:
                r[-1] = F32(1.0 if code == 2 else -0.25)
            s_list, r_list = [torch.from_numpy(x) for x in s], [float(x) for x in r]
            own = ReplayMemory(length)
            explorer.memory = own
            explorer.update_memory(s_list, [], r_list, mode == "il")
            targets.append(np.array([v.item() for _, v in own.memory], F32))
            assert all(v.dtype == torch.float32 for _, v in own.memory)
            explorer.memory = memory
            if code in (2, 3):
                explorer.update_memory(s_list, [], r_list, mode == "il")
            states.append(s)
            rewards.append(r)
        cases.append(dict(mode=mode, capacity=capacity, gamma=GAMMA, time_step=TIME_STEP, desired_speed=speed,
                          lengths=np.array([e[0] for e in episodes], np.int32), codes=np.array([e[1] for e in episodes], np.int32),
                          states=np.concatenate(states), rewards=np.concatenate(rewards), targets=np.concatenate(targets),
                          mem_states=np.stack([s.numpy() for s, _ in memory.memory]).astype(F32),
                          mem_values=np.array([v.item() for _, v in memory.memory], F32), mem_position=int(memory.position),
                          mem_length=len(memory)))
    return cases


if __name__ == "__main__":
    cases = generate()
    for c in cases:
        print(f"{c['mode']} capacity {c['capacity']} speed {c['desired_speed']}: {int(c['lengths'].sum())} steps in {len(c['lengths'])} episodes, "
              f"memory {c['mem_length']} samples, position {c['mem_position']}")
    path = save_cases("g26_episodes", cases)
    print("g26_episodes:", len(cases), "cases ->", path, os.path.getsize(path), "bytes")
