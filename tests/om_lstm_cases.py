"""What the OM-LSTM-RL tests share (test_value_om_lstm_cpu.py, test_gpu_value_om_lstm.py, golden/make_golden_g22.py): the float64
restatement of a decision on rows widened by occupancy maps -- lstm_cases' order rule and network (``forward64`` is width-generic), om_cases'
maps, and the rule that pairs a step's row with a map --, cs_value_net_pack_lstm_om's blob layout, the policy configuration and golden G22's
weights rebuilt from their seed.  No GPU, no reference."""
import functools

import numpy as np

import lstm_cases as lc
import om_cases

F32 = np.float32
PAIRINGS = ("reference", "own")         # value_net.MAP_ORDERS: the map at that place of action 0's order / every human's own map
DEFAULT_GRID = om_cases.CONFIGS[0]      # the reference's [om]: 4 x 4 cells of 1 m, 3 channels = 48 columns


def om_lstm_policy(network=1, cols=13, grid=DEFAULT_GRID, **overrides):
    from social_navigation_pyenvs_amd.crowd_nav.policy.policy_factory import policy_factory

    kw = dict(lstm_rl__with_om="true", lstm_rl__with_interaction_module="true" if network == 2 else "false", om__cell_num=grid[0],
              om__cell_size=grid[1], om__om_channel_size=grid[2])
    if cols == 15:
        kw["sarl__with_theta_and_omega_visible"] = "true"
    kw.update(overrides)
    pol = policy_factory["om_lstm_rl"]()
    pol.configure(lc.lstm_config(**kw))
    return pol


# ---------------------------------------------------------------------------------------------------------------- the wide rows
def wide_rows(rot, maps, pairing, sort=True):
    """rot [W, A, n, cols] rotated rows as they lie, maps [W, n, C] every human's own map -> [W, A, n, cols + C] in evaluation order.
    `sort`: the decision's order per (world, action) (lstm_cases.decision_order on column 11), else the rows as they lie.  Step t of (w, a)
    is rot[w, a, perm_a[t]] beside maps[w, perm_a[t]] ("own") or maps[w, perm_0[t]] ("reference": the order of the world's action 0)."""
    assert pairing in PAIRINGS
    rot, maps = np.asarray(rot), np.asarray(maps)
    W, A, n, _ = rot.shape
    perm = lc.decision_order(rot[..., 11]) if sort else np.broadcast_to(np.arange(n), (W, A, n))
    rows = np.take_along_axis(rot, perm[..., None], axis=2)
    mperm = perm if pairing == "own" else np.broadcast_to(perm[:, :1], perm.shape)
    paired = np.take_along_axis(np.broadcast_to(maps[:, None], (W, A) + maps.shape[1:]), mperm[..., None], axis=2)
    return np.concatenate([rows, paired.astype(rows.dtype)], axis=3)


def maps64_of(next_humans, grid, vel_col=2):
    """om_cases.maps64 of every world of next_humans [W, n, 4 | 6] (velocity at vel_col) -> float64 [W, n, C]"""
    cell_num, cell_size, channels = grid
    nh = np.asarray(next_humans, np.float64)
    return np.stack([om_cases.maps64(h[:, [0, 1, vel_col, vel_col + 1]], cell_num, cell_size, channels)[0] for h in nh])


def rotated64(robot, actions, next_humans, radii, dt):
    """The serial decision's rotated rows in float64 (cadrl.py propagate + rotate, holonomic): robot [9] FullState order, actions [A, 2],
    next_humans [n, 4] (px, py, vx, vy), radii [n] -> [A, n, 13]"""
    robot, acts, nh = np.asarray(robot, np.float64), np.asarray(actions, np.float64), np.asarray(next_humans, np.float64)
    out = []
    for vx, vy in acts:
        px, py = robot[0] + vx * dt, robot[1] + vy * dt
        gx, gy, radius, v_pref = robot[5], robot[6], robot[4], robot[7]
        rot = np.arctan2(gy - py, gx - px)
        c, s = np.cos(rot), np.sin(rot)
        one = np.ones(len(nh))
        hx, hy = nh[:, 0] - px, nh[:, 1] - py
        out.append(np.stack([np.hypot(gx - px, gy - py) * one, v_pref * one, 0.0 * one, radius * one, (vx * c + vy * s) * one, (vy * c - vx * s) * one,
                             hx * c + hy * s, hy * c - hx * s, nh[:, 2] * c + nh[:, 3] * s, nh[:, 3] * c - nh[:, 2] * s, np.asarray(radii, np.float64),
                             np.hypot(hx, hy), radius + np.asarray(radii, np.float64)], 1))
    return np.stack(out)


def restate_decision(w64, case, pairing, grid=DEFAULT_GRID):
    """A recorded G22 decision restated in float64 from its states alone: (action values [A], network outputs [A], rotated [A, n, 13] as they
    lie, own maps [n, C])."""
    rot = rotated64(case["robot"], case["action_space"], case["next_humans"], case["obs"][:, 4], float(case["dt"]))
    maps = maps64_of(case["next_humans"][None], grid)
    net = lc.forward64(w64, wide_rows(rot[None], maps, pairing))[0]
    disc = float(case["gamma"]) ** (float(case["dt"]) * float(case["robot"][7]))
    return np.asarray(case["rewards"], np.float64) + disc * net, net, rot, maps[0]


# ---------------------------------------------------------------------------------------------------------------- the blob layout
def pack_call(dims, cols, om_cols, arrays, size_only=False):
    """(status, message, blob) of cs_value_net_pack_lstm_om on host arrays"""
    import ctypes as C

    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    d = np.ascontiguousarray(dims, np.int32)
    nf = C.c_size_t(0)
    rc = lib.cs_value_net_pack_lstm_om(d.ctypes.data if len(d) else None, len(d), cols, om_cols, None, None, C.byref(nf))
    if rc != 0 or size_only:
        return rc, lib.cs_last_error().decode(), nf.value
    arrays = [np.ascontiguousarray(a, F32) for a in arrays]
    ptrs = (C.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])
    blob = np.full(nf.value, F32(-7.0))
    rc = lib.cs_value_net_pack_lstm_om(d.ctypes.data, len(d), cols, om_cols, ptrs, blob.ctypes.data, C.byref(nf))
    return rc, lib.cs_last_error().decode(), blob


# ---------------------------------------------------------------------------------------------------------------- golden G22
@functools.lru_cache(maxsize=None)
def g22():
    """golden G22 by case kind: {kind: [cases]}"""
    from golden_io import load_cases

    out = {}
    for c in load_cases("g22_om_lstm_rl"):
        out.setdefault(c["kind"], []).append(c)
    return out


def g22_policy(wkey):
    """A configured OM-LSTM-RL of this project with the weights of G22's network `wkey`, rebuilt from the seed and checked by SHA-256"""
    case = next(c for c in g22()["weights"] if c["wkey"] == wkey)
    pol = om_lstm_policy(int(case["network"]), int(case["cols"]))
    sd = pol.model.state_dict()
    assert sorted(sd) == list(case["weights_keys"]) and [list(sd[k].shape) for k in sorted(sd)] == case["weights_shapes"]
    assert lc.draw_weights(pol.model, int(case["seed"]), bool(case["calm_last"])) == case["sha256"]
    return pol
