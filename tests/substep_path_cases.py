"""Inputs of the substep-path tests (test_gpu_substep_paths.py on the GPU, test_substep_paths_cpu.py on the oracle alone): small hybrid
worlds -- even worlds circular crossings with two-goal lists, odd worlds parallel traffic under the respawn rule -- walking at distinct
speeds, with ONE rare event of the substep loop planted in each case:

  * "contact": in world 0 the humans 0 and 1 overlap by two centimetres and walk apart at 1 m/s each, so the contact pass runs in substep
    0 and in no substep behind it;
  * "goals":   in world 0 (two-goal lists) human 2 stands inside its radius of goals[0] on the incoming row, and human 3 walks at 1 m/s
    towards a goals[0] that is r + 2 cm away: it is inside r on the row substep 2 receives (the third), not before;
  * "respawn": in world 1 (traffic, the respawn rule on) a human walks at 1 m/s towards its goal from 3.02 m: the row substep 1 leaves is
    within 3 m and the rule moves it behind everybody else.

The events as the oracle sees them (`events`) are asserted without a GPU; an input that stops producing its event fails there.
Everything is float32-valued, made once per key and handed out as copies."""
import numpy as np

DT = 0.0125
NSUB = 3
R_BODY = 0.3
MODELS = ["sfm_helbing", "hsfm_farina", "hsfm_new_moussaid"]
KINDS = ["contact", "goals", "respawn"]
# (W, humans, robot row): a full wavefront and one with idle lanes at 25 rows, one world per wavefront at 50, 25 humans + a robot row
SHAPES = [(2, 25, False), (3, 25, False), (2, 50, False), (3, 50, False), (2, 25, True)]
OVERLAP = 0.02
_CACHE = {}


def _face(S, w, i, direction, speed):
    """human i of world w walks along `direction` at `speed`: heading, linear and body velocity agree"""
    d = np.asarray(direction, dtype=np.float64)
    d = d / np.linalg.norm(d)
    S[w, i, 2] = np.arctan2(d[1], d[0])
    S[w, i, 3:5] = speed * d
    S[w, i, 5:7] = (speed, 0.0)
    S[w, i, 7] = 0.0


def _clear_of_others(S, w, i, p, gap, skip=()):
    others = [j for j in range(S.shape[1]) if j != i and j not in skip]
    return np.linalg.norm(S[w, others, 0:2] - np.asarray(p), axis=1).min() > gap


def walking_worlds(W, n, model, seed):
    """hybrid worlds, every human walking towards its goal at 0.3 .. 0.9 m/s"""
    from social_navigation_pyenvs_amd import scenarios as sc

    # (50 humans do not fit the default circle and lane without overlaps at the start: a wider circle, a longer lane)
    S, goals, P, rb = sc.hybrid_worlds(W, n, model, seed0=seed) if n <= 25 else sc.hybrid_worlds(W, n, model, radius=14.0, length=28.0, seed0=seed)
    speed = 0.3 + 0.6 * np.random.default_rng(seed).random((W, n))
    d = goals[:, :, 0] - S[:, :, 0:2]
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    S[..., 2] = np.arctan2(d[..., 1], d[..., 0])          # (what _face does, for every human at once)
    S[..., 3:5] = speed[..., None] * d
    S[..., 5] = speed
    S[..., 6:8] = 0.0
    rw = (np.arange(W) % 2 == 1).astype(np.int32)
    return S, goals, P, rb, rw


def plant(kind, S, goals, w_even=0, w_odd=1):
    """Plant the event of `kind` (module docstring) in world w_even (contact, goals) or w_odd (respawn); returns the humans involved."""
    n = goals.shape[1]
    if kind == "contact":
        w = w_even
        for ang in np.linspace(0.0, 2 * np.pi, 24, endpoint=False):
            d = np.array([np.cos(ang), np.sin(ang)])
            p1 = S[w, 0, 0:2] + (2 * R_BODY - OVERLAP) * d
            if _clear_of_others(S, w, 1, p1, 2 * R_BODY + 0.3, skip=(0,)):
                break
        else:
            raise AssertionError("no free place beside human 0")
        S[w, 1, 0:2] = p1
        _face(S, w, 0, -d, 1.0)
        _face(S, w, 1, d, 1.0)
        return w, (0, 1)
    if kind == "goals":
        w = w_even
        assert not np.isnan(goals[w]).any(), "two-goal lists"
        far = goals[w, 2, 0].copy()
        goals[w, 2, 0] = S[w, 2, 0:2] + (0.1, 0.05)
        goals[w, 2, 1] = far
        d = goals[w, 3, 0] - S[w, 3, 0:2]
        d = d / np.linalg.norm(d)
        goals[w, 3, 1] = goals[w, 3, 0]
        goals[w, 3, 0] = S[w, 3, 0:2] + (R_BODY + 0.02) * d
        _face(S, w, 3, d, 1.0)
        S[w, 2:4, 10:12] = goals[w, 2:4, 0]
        return w, (2, 3)
    if kind == "respawn":
        w = w_odd
        assert np.isnan(goals[w, :, 1]).all(), "a traffic world: one goal per human"
        for i in range(n):
            p = np.array([goals[w, i, 0, 0] + 3.02, S[w, i, 1]])
            if _clear_of_others(S, w, i, p, 2 * R_BODY + 0.3):
                break
        else:
            raise AssertionError("no free lane at the goal line")
        S[w, i, 0:2] = p
        _face(S, w, i, (-1.0, 0.0), 1.0)
        return w, (i,)
    raise ValueError(kind)


def robots(W):
    """a visible robot beside the crowd (circle worlds reach |y| <= 7.5, traffic worlds |y| <= 1.5), moved by a constant action"""
    R = np.zeros((W, 13), np.float32)
    R[:, 0] = 0.25 * np.arange(W); R[:, 1] = 9.0; R[:, 8] = 0.3; R[:, 9] = 80; R[:, 10:12] = -R[:, 0:2]; R[:, 12] = 1.0
    A = np.tile(np.array([[0.3, -0.2]], np.float32), (W, 1))
    return R, A


def case(kind, model, W, n, robot_row=False, seed=4100):
    """(S [W, rows, 13], goals [W, n, 2, 2], P [n, 20], respawn bounds, respawn worlds, robot rows or None, action or None, world, humans)"""
    key = (kind, model, W, n, robot_row, seed)
    if key not in _CACHE:
        S, goals, P, rb, rw = walking_worlds(W, n, model, seed + n)
        w, who = plant(kind, S, goals)
        R = A = None
        if robot_row:
            R, A = robots(W)
            S = np.concatenate([S, R[:, None, :].astype(np.float64)], axis=1)
        _CACHE[key] = (S.astype(np.float32), goals.astype(np.float32), P.astype(np.float32), rb, rw, R, A, w, who)
    S, goals, P, rb, rw, R, A, w, who = _CACHE[key]
    return S.copy(), goals.copy(), P.copy(), rb, rw.copy(), None if R is None else R.copy(), None if A is None else A.copy(), w, who


def oracle_substeps(model, S, goals, P, rb, rw, R=None, A=None, nsub=NSUB):
    """The oracle's rows and goal lists ENTERING substep 0 .. nsub (float64 from the float32 inputs): lists of [W, rows, 13], [W, n, G, 2]"""
    from oracle import crowd_oracle as orc
    from social_navigation_pyenvs_amd.scenarios import SFMS

    type_ = SFMS.index(model)
    S = S.astype(np.float64); goals = goals.astype(np.float64); P = P.astype(np.float64)
    W, n = goals.shape[0], goals.shape[1]
    rob = None if R is None else R.astype(np.float64)
    act = None if A is None else A.astype(np.float64)
    rows_at, goals_at = [S.copy()], [goals.copy()]
    for _ in range(nsub):
        Sn, gn = np.empty_like(S), np.empty_like(goals)
        for flag in (0, 1):
            m = rw == flag
            if not m.any():
                continue
            s2, g2, r2 = orc.step_block(type_, S[m], goals[m], None, P, DT, 1, np.zeros((int(m.sum()), S.shape[1])), True, robot_visible=R is not None,
                                        robot=None if rob is None else rob[m], action=None if act is None else act[m], respawn=bool(flag),
                                        respawn_par=(rb[0], rb[1], 0.0) if flag else (0.0, 0.0, 0.0))
            Sn[m], gn[m] = s2, g2.reshape(-1, n, goals.shape[2], 2)
            if rob is not None:
                rob[m] = r2
        S, goals = Sn, gn
        rows_at.append(S.copy()); goals_at.append(goals.copy())
    return rows_at, goals_at


def overlaps(S_w, n):
    """unordered pairs of humans of one world whose bodies overlap"""
    p, r = S_w[:n, 0:2], S_w[:n, 8]
    d = np.linalg.norm(p[:, None] - p[None], axis=-1)
    i, j = np.nonzero(np.triu(d < r[:, None] + r[None], 1))
    return sorted(zip(i.tolist(), j.tolist()))


def events(kind, model, W, n, robot_row=False):
    """What the oracle says of the case: a dict the CPU test asserts on"""
    S, goals, P, rb, rw, R, A, w, who = case(kind, model, W, n, robot_row)
    rows_at, goals_at = oracle_substeps(model, S, goals, P, rb, rw, R, A)
    out = {"world": w, "who": who}
    out["overlaps_entering"] = [[(wi, pr) for wi in range(W) for pr in overlaps(rows_at[k][wi], n)] for k in range(NSUB)]
    # a goal list rotated in substep k: its head after the substep is its second entry of before
    out["rotated_in"] = [[(wi, i) for wi in range(W) for i in range(n)
                          if not np.isnan(goals_at[k][wi, i, 1]).any() and np.array_equal(goals_at[k + 1][wi, i, 0], goals_at[k][wi, i, 1])
                          and not np.array_equal(goals_at[k][wi, i, 0], goals_at[k][wi, i, 1])] for k in range(NSUB)]
    # a row respawned in substep k: moved to the right of the bound, from the left half
    out["respawned_in"] = [[(wi, i) for wi in range(W) for i in range(n)
                            if rows_at[k][wi, i, 0] < 0.0 and rows_at[k + 1][wi, i, 0] >= rb[0]] for k in range(NSUB)]
    return out
