"""Cases and reference of the ORCA robot policy (crowd_nav/policy_no_train/orca.py, csrc/policy_orca.hip), shared by its CPU and GPU suites.

The reference is the C restatement of RVO2 (oracle/orca_oracle.c): the robot is agent 0, the humans follow, only agent 0's row is read.
The inputs are built in float32 exactly as the kernel builds them, so the comparison is bit for bit."""
from collections import namedtuple

import numpy as np

F = np.float32
NEIGHBOR_DIST, MAX_NEIGHBORS, TIME_HORIZON, MAX_SPEED = 10.0, 10, 5.0, 1.0
SIZES = (0, 1, 5, 9, 10, 11, 25, 64, 65, 70)
WORLDS_PER_SIZE = 48
TIME_STEP = 0.25
# edge_cases()'s tie: the seed of the first velocity draw for which swapping the two tied rows changes the oracle's answer (_tie_case)
TIE_SEED = 0

Ref = namedtuple("Ref", "action lines kind colliding")


def robot_row(px, py, vx, vy, radius, gx, gy, v_pref):
    """The 13-column safe-state row: px, py, ., vx, vy, ., ., ., radius, ., gx, gy, v_pref."""
    return np.array([px, py, 0.0, vx, vy, 0.0, 0.0, 0.0, radius, 0.0, gx, gy, v_pref], F)


def _rows(obs):
    """Observation rows as a float32 [n][5|7] array (n may be 0)."""
    obs = np.asarray(obs, F)
    assert obs.ndim == 2 and obs.shape[1] in (5, 7), obs.shape
    return obs


def _violation(lines, v):
    """det(direction, point - v) of every line [k][4] = (point.x, point.y, direction.x, direction.y) in float32: > 0 is violated."""
    lines = np.asarray(lines, F).reshape(-1, 4)
    return lines[:, 2] * (lines[:, 1] - v[1]) - lines[:, 3] * (lines[:, 0] - v[0])


def reference_action(robot13, obs, time_step, safety_space=0):
    """Agent 0's new velocity from the oracle, its ORCA lines and the class of the case: 'free' (no line violated at the clipped
    preferred velocity), 'lp2' (one is, and the answer satisfies every line) or 'lp3' (the answer violates a line by more than 1e-4);
    ``colliding``: some centre distance is below the combined radii."""
    from oracle import crowd_oracle as orc

    r = np.asarray(robot13, F)
    obs = _rows(obs)
    n = obs.shape[0]
    margin = F(0.01 + safety_space)
    pos = np.concatenate([r[None, 0:2], obs[:, 0:2]]).astype(F)
    vel = np.concatenate([r[None, 3:5], obs[:, 2:4]]).astype(F)
    radius = (np.concatenate([r[8:9], obs[:, 4]]).astype(F) + margin).astype(F)
    maxspeed = np.concatenate([r[12:13], np.full(n, MAX_SPEED, F)]).astype(F)
    d = (r[10:12] - r[0:2]).astype(F)
    s = np.sqrt(F(F(d[0] * d[0]) + F(d[1] * d[1])))
    pref = np.zeros((n + 1, 2), F)
    pref[0] = (d / s).astype(F) if s > F(1.0) else d
    out, lines, nl = orc.orca_new_velocities(pos, vel, pref, radius, maxspeed, NEIGHBOR_DIST, MAX_NEIGHBORS, TIME_HORIZON, time_step,
                                             return_lines=True)
    action, L = out[0].copy(), lines[0][:nl[0]].copy()
    # linearProgram2's start: the preferred velocity clipped to the maxSpeed circle
    start = pref[0].astype(np.float64)
    if start @ start > float(r[12]) ** 2:
        start = start / np.sqrt(start @ start) * float(r[12])
    if not np.any(_violation(L, start.astype(F)) > 0):
        kind = "free"
    elif np.any(_violation(L, action) > F(1e-4)):
        kind = "lp3"
    else:
        kind = "lp2"
    dist = np.hypot(*(pos[1:] - pos[0]).astype(np.float64).T) if n else np.zeros(0)
    colliding = bool(np.any(dist < (radius[1:] + radius[0]).astype(np.float64)))
    return Ref(action, L, kind, colliding)


def _case(name, robot13, obs, time_step=TIME_STEP, safety_space=0):
    obs = _rows(obs)
    return dict(name=name, robot=np.asarray(robot13, F), obs=obs, n=obs.shape[0], time_step=time_step, safety_space=safety_space)


def random_cases():
    """48 worlds for every n of SIZES, seeded per n: crowded to sparse, far and near goals, three v_pref."""
    out = []
    for n in SIZES:
        rng = np.random.default_rng(7000 + n)
        for w in range(WORLDS_PER_SIZE):
            p = rng.uniform(-1, 1, 2)
            v = rng.uniform(-1, 1, 2)
            g = rng.uniform(-6, 6, 2)
            if w % 8 == 7:
                g = g * 0.1                  # a goal inside 1 m: the unnormalised branch of the preferred velocity
            spread = (1.5, 3.0, 6.0)[w % 3]
            hp = p + rng.uniform(-spread, spread, (n, 2))
            hv = rng.uniform(-1, 1, (n, 2))
            rad = rng.uniform(0.2, 0.4, n + 1)
            v_pref = (1.0, 0.7, 1.3)[w % 3]
            obs = np.concatenate([hp, hv, rad[1:, None]], axis=1)
            out.append(_case(f"random-n{n}-w{w}", robot_row(p[0], p[1], v[0], v[1], rad[0], p[0] + g[0], p[1] + g[1], v_pref), obs))
    return out


def cases_of_size(cases, n):
    return [c for c in cases if c["n"] == n and c["name"].startswith("random")]


def _tie_rows(seed):
    """Twelve humans around a robot at the origin, on exactly representable coordinates: nine near ones, one beyond neighbor_dist, and the
    last two at the same distSq (6.25) -- they compete for the tenth slot, the lower row index wins.  Velocities from ``seed``."""
    near = [(-0.75, 0.5), (0.5, -1.0), (-1.0, -0.75), (1.25, 0.25), (0.25, 1.5), (-1.5, 0.75), (1.0, -1.5), (-0.5, -1.75), (1.75, 1.0)]
    pos = np.array(near + [(8.0, 8.0), (2.0, 1.5), (1.5, 2.0)], F)
    rng = np.random.default_rng(seed)
    vel = rng.uniform(-1, 1, (12, 2)).astype(F)
    return np.concatenate([pos, vel, np.full((12, 1), 0.25, F)], axis=1).astype(F)


def tie_case(seed=TIE_SEED, swapped=False):
    obs = _tie_rows(seed)
    if swapped:
        obs[[10, 11]] = obs[[11, 10]]
    return _case("tie-swapped" if swapped else "tie", robot_row(0.0, 0.0, 0.5, 0.5, 0.25, 4.0, 4.0, 1.0), obs)


def search_tie_seed(limit=2000):
    """The first seed whose tie case discriminates: the oracle's answer changes when the two tied rows are swapped."""
    for seed in range(limit):
        a, b = tie_case(seed), tie_case(seed, swapped=True)
        ra, rb = (reference_action(c["robot"], c["obs"], c["time_step"]) for c in (a, b))
        if not np.array_equal(ra.action, rb.action):
            return seed
    raise AssertionError("no discriminating tie within the limit")


def edge_cases():
    rng = np.random.default_rng(99)

    def crowd(n, spread=2.0, cols=5):
        rows = np.concatenate([rng.uniform(-spread, spread, (n, 2)), rng.uniform(-1, 1, (n, 2)), rng.uniform(0.2, 0.4, (n, 1))], axis=1)
        if cols == 7:
            rows = np.concatenate([rows, rng.uniform(-3, 3, (n, 2))], axis=1)       # theta, omega: not read
        return rows.astype(F)

    just_above = float(np.nextafter(F(1.0), F(2.0)))
    out = [
        _case("goal-on-robot", robot_row(0.25, -0.5, 0.3, 0.1, 0.3, 0.25, -0.5, 1.0), crowd(4)),
        _case("goal-at-exactly-1", robot_row(0.0, 0.0, 0.2, -0.1, 0.3, 1.0, 0.0, 1.0), crowd(4)),
        _case("goal-just-above-1", robot_row(0.0, 0.0, 0.2, -0.1, 0.3, just_above, 0.0, 1.0), crowd(4)),
        _case("goal-at-exactly-1-alone", robot_row(0.0, 0.0, 0.2, -0.1, 0.3, 1.0, 0.0, 1.3), np.zeros((0, 5), F)),
        _case("goal-just-above-1-alone", robot_row(0.0, 0.0, 0.2, -0.1, 0.3, just_above, 0.0, 1.3), np.zeros((0, 5), F)),
        # |(6, 8)| = 10 exactly: distSq = 100 is not < neighbor_dist^2, so the oracle builds ONE line, for the near human
        _case("human-at-exactly-10", robot_row(0.0, 0.0, 0.4, 0.3, 0.3, 3.0, 4.0, 1.0),
              np.array([[6.0, 8.0, -0.5, -0.5, 0.3], [1.0, 0.5, -0.3, 0.0, 0.3]], F)),
        # two humans ahead, no overlap: the combined radii (and with them the safety space) shape the half-planes the answer lies on
        _case("safety-space", robot_row(0.0, 0.0, 0.5, 0.0, 0.3, 5.0, 0.0, 1.0),
              np.array([[1.5, 0.2, -0.5, 0.0, 0.3], [1.0, -1.2, 0.0, 0.4, 0.25]], F), safety_space=0.1),
        _case("seven-columns", robot_row(0.5, 0.5, -0.2, 0.4, 0.3, -3.0, 2.0, 1.0), crowd(12, 2.5, cols=7)),
        tie_case(),
        tie_case(swapped=True),
    ]
    return out
