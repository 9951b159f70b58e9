"""Shared by tests/test_episodes_cpu.py and tests/test_gpu_episodes.py: a numpy / pure-Python restatement of the device episode buffer
(crowd_nav/utils/episodes.py over csrc/episodes.hip; the contract is in include/crowdstep.h), written with Python float64 arithmetic in the
order of the reference's Explorer, the scripts that drive a buffer -- this restatement or the device one, through the same calls -- and the
case tables.

``RefMemory`` is the ring of the reference's ReplayMemory (one sample per ``push``); ``RefEpisodeBuffer`` has ``EpisodeBuffer``'s interface
on numpy arrays and flushes by pushing sample after sample, world-ascending then step-ascending: what the kernels must leave behind."""
import itertools

import numpy as np

F32 = np.float32
REACH_GOAL, COLLISION, TIMEOUT = 2, 3, 4       # social_gym/src/info.py INFO_BY_CODE


class RefMemory:
    def __init__(self, capacity):
        self.capacity, self.position, self.length = int(capacity), 0, 0
        self.states = self.values = None

    def push(self, state, value):
        if self.states is None:
            self.states = np.zeros((self.capacity,) + state.shape, F32)
            self.values = np.zeros(self.capacity, F32)
        self.states[self.position], self.values[self.position] = state, value
        self.length = max(self.length, self.position + 1)     # the reference appends while the list is short, then overwrites
        self.position = (self.position + 1) % self.capacity

    def push_batch(self, states, values, keep=None):
        for w in range(len(states)):
            if keep is None or keep[w]:
                self.push(states[w], F32(values[w]))

    def __len__(self):
        return self.length

    def snapshot(self):
        return dict(states=self.states.copy(), values=self.values.copy(), position=self.position, length=self.length)


def return_to_go(rewards, i, gamma, dt, v):
    """The value of step i of an episode with these rewards: the sum over t >= i of gamma^((t - i) dt v) r_t, float64, ascending t."""
    value = 0.0
    for t in range(i, len(rewards)):
        value = value + gamma ** ((t - i) * dt * v) * rewards[t]
    return value


class RefEpisodeBuffer:
    def __init__(self, n_worlds, max_steps, gamma, time_step, keep=(REACH_GOAL, COLLISION)):
        self.W, self.T, self.gamma, self.dt, self.keep = n_worlds, max_steps, float(gamma), float(time_step), tuple(keep)
        self.steps = [[] for _ in range(n_worlds)]        # per world: (state, reward as a Python float, target or None)
        self.overflow = np.zeros(n_worlds, np.int32)
        self.fig = dict(episodes=0, success=0, collision=0, timeout=0, nav_time_sum=0.0, discounted_reward_sum=0.0)

    def append(self, state, reward, target=None):
        for w in range(self.W):
            if len(self.steps[w]) < self.T:
                self.steps[w].append((np.array(state[w], F32), float(F32(reward[w])), None if target is None else F32(target[w])))
            else:
                self.overflow[w] = 1

    def flush(self, memory, done, info_code, v_pref=1.0, targets="returns"):
        v_of = (lambda w: float(v_pref[w])) if np.ndim(v_pref) else (lambda w: float(v_pref))
        for w in range(self.W):
            if not done[w]:
                continue
            steps, code, v = self.steps[w], int(info_code[w]), v_of(w)
            rewards = [s[1] for s in steps]
            self.fig["episodes"] += 1
            if code == REACH_GOAL:
                self.fig["success"] += 1
                self.fig["nav_time_sum"] += len(steps) * self.dt
            elif code == COLLISION:
                self.fig["collision"] += 1
            elif code == TIMEOUT:
                self.fig["timeout"] += 1
            self.fig["discounted_reward_sum"] += return_to_go(rewards, 0, self.gamma, self.dt, v)
            if code in self.keep and not self.overflow[w]:
                for i, (state, _, target) in enumerate(steps):
                    memory.push(state, F32(return_to_go(rewards, i, self.gamma, self.dt, v)) if targets == "returns" else target)
            self.steps[w], self.overflow[w] = [], 0

    def cursor(self):
        return np.array([len(s) for s in self.steps], np.int32)

    def figures(self, time_limit=None):
        f = dict(self.fig)
        n = f["episodes"]
        f.update(success_rate=f["success"] / n if n else 0.0, collision_rate=f["collision"] / n if n else 0.0,
                 avg_nav_time=f["nav_time_sum"] / f["success"] if f["success"] else time_limit,
                 avg_discounted_reward=f["discounted_reward_sum"] / n if n else 0.0)
        return f


# ---------------------------------------------------------------------------------------------------------------- G26
def play_golden(case, buf, memory, dev=lambda a: a):
    """The episodes of a G26 case through a buffer of W = len(episodes) worlds in the reference's order: world w holds episode w, the
    episodes end together at step T = the longest length.  A world whose episode is shorter steps on filler rows first and drops them
    in a flush of its own (done with the code Timeout, which is not kept) at the step its episode begins."""
    lengths = [int(n) for n in case["lengths"]]
    W, T = len(lengths), max(lengths)
    mode = "returns" if case["mode"] == "il" else "stored"
    starts = np.concatenate([[0], np.cumsum(lengths)])
    filler = np.full((W,) + case["states"].shape[1:], -7.0, F32)
    for s in range(T):
        begins = np.array([T - n == s and s > 0 for n in lengths])
        if begins.any():
            buf.flush(memory, dev(begins.astype(np.uint8)), dev(np.full(W, TIMEOUT, np.int32)), case["desired_speed"], mode)
        state, reward, target = filler.copy(), np.zeros(W, F32), np.zeros(W, F32)
        for w, n in enumerate(lengths):
            i = s - (T - n)
            if i >= 0:
                state[w], reward[w], target[w] = case["states"][starts[w] + i], case["rewards"][starts[w] + i], case["targets"][starts[w] + i]
        buf.append(dev(state), dev(reward), dev(target) if mode == "stored" else None)
    buf.flush(memory, dev(np.ones(W, np.uint8)), dev(np.asarray(case["codes"], np.int32)), case["desired_speed"], mode)


# ---------------------------------------------------------------------------------------------------------------- the edge table
EDGE_WORLDS = (1, 3, 65, 1025)          # one world; fewer than a wavefront; more than one; more than one 1024-thread block of the prefix sum
EDGE_SHAPES = ((1, 13), (5, 15), (3, 61), (7,))     # rows of 13, 75, 183 and 7 floats: the dword copy
EDGE_CAPACITIES = ("roomy", "wraps", "exact", "small", "one")
EDGE_CASES = [(W, 6, shape, cap) for W, shape, cap in itertools.product(EDGE_WORLDS, EDGE_SHAPES, EDGE_CAPACITIES)] + [(3, 100, (1, 13), "small")]
# rows of 52 floats, a multiple of 16 bytes: the 16-byte copy
EDGE_CASES += [(W, 6, (4, 13), cap) for W in (3, 65) for cap in ("wraps", "small")]


def edge_plan(index, W, T):
    """Seeded: the length every world has at the main flush (1, T and others), the worlds left running there, the outcome codes."""
    rng = np.random.default_rng(2600 + index)
    lengths = rng.integers(1, T + 1, W)
    lengths[0] = 1 if W > 1 else (T if index % 2 else 1)
    if W > 1:
        lengths[1] = T
    running = (rng.random(W) < 0.2) & (lengths < T)
    running[0] = False
    codes = rng.choice([REACH_GOAL, COLLISION, TIMEOUT], W).astype(np.int32)
    codes[0] = REACH_GOAL if index % 3 else COLLISION
    return lengths, running, codes, rng


def edge_capacity(kind, lengths, running, codes, W):
    k_main = int(sum(n for n, r, c in zip(lengths, running, codes) if not r and c != TIMEOUT))
    total = W + k_main + int(sum(n + 1 for n, r, c in zip(lengths, running, codes) if r and c != TIMEOUT)) + W
    return {"roomy": total + 7, "wraps": k_main + 1, "exact": k_main, "small": max(1, int(k_main / 2.5)), "one": 1}[kind]


def play_edge(index, W, T, shape, buf, memory, dev=lambda a: a, check=None):
    """One row of the edge table.  A first step flushed whole (Collision: the ring's position is not 0 afterwards); T steps in which world
    w drops its filler steps T - L_w steps in (a flush of Timeouts, or a flush where nobody is done), so that the main flush finds lengths
    1 .. T, some worlds still running and codes 2 / 3 / 4; one more step and the running worlds' flush; two steps flushed as Timeouts only;
    one step flushed as ReachGoal everywhere.  `check(tag)` is called after the main flush and at the end."""
    lengths, running, codes, rng = edge_plan(index, W, T)
    mode = "stored" if index % 2 else "returns"
    v_pref = rng.choice([0.8, 1.0, 1.3], W) if index % 4 >= 2 else (1.0, 0.8)[index % 3 == 0]
    v_dev = dev(np.asarray(v_pref, np.float64)) if np.ndim(v_pref) else v_pref

    def step():
        reward = rng.choice(np.array([0.0, -0.0125, -0.00625, -0.02, 1.0, -0.25], F32), W)
        target = rng.uniform(-1, 1, W).astype(F32)
        buf.append(dev(rng.uniform(-2, 2, (W,) + shape).astype(F32)), dev(reward), dev(target) if mode == "stored" else None)

    def flush(done, code):
        buf.flush(memory, dev(np.asarray(done, bool).astype(np.uint8)), dev(np.asarray(code, np.int32)), v_dev, mode)

    step()
    flush(np.ones(W, bool), np.full(W, COLLISION))
    for s in range(1, T + 1):
        step()
        if s < T:
            flush(T - lengths == s, np.full(W, TIMEOUT))          # often nobody: a no-op
    flush(~running, codes)
    if check:
        check("main")
    if T > 1:
        step()
    flush(running, codes)
    for _ in range(min(2, T)):
        step()
    flush(np.ones(W, bool), np.full(W, TIMEOUT))
    step()
    flush(np.ones(W, bool), np.full(W, REACH_GOAL))
    if check:
        check("end")
