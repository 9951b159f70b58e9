"""What the OM-SARL tests (test_value_om_cpu.py, test_gpu_value_om.py) and golden G20's generator share: a float64 numpy restatement of the
reference's ``build_occupancy_maps`` (crowd_nav/policy/multi_human_rl.py:133-187), the grid configurations, the random cases with their
edge condition, and the seeded weights of an OM-SARL network.  No GPU, no reference."""
import hashlib

import numpy as np

F32 = np.float32
# (cell_num, cell_size, om_channel_size): the reference's default first
CONFIGS = ((4, 1.0, 3), (4, 1.0, 1), (4, 1.0, 2), (3, 0.7, 3), (1, 2.0, 3))
WIDE_CONFIG = (8, 0.5, 3)          # C = 192
EDGE = 1e-5                        # cells: a pair this close to a cell edge in float64 may fall either side in float32


def maps64(humans, cell_num, cell_size, channels):
    """humans [n][4+] (px, py, vx, vy) -> (maps [n][cell_num^2 * channels] float64 laid out [cell][channel], pre [n][n][2]: the pre-floor
    cell coordinates (x / cell_size + cell_num / 2, y ...) of human j in human i's frame, NaN on the diagonal).  The reference's formulas
    in float64, the sums in ascending j."""
    h = np.asarray(humans, np.float64)
    n, cells = len(h), cell_num * cell_num
    maps = np.zeros((n, cells * channels))
    pre = np.full((n, n, 2), np.nan)
    for i in range(n):
        a = np.arctan2(h[i, 3], h[i, 2])
        members = [[] for _ in range(cells)]
        dx, dy = h[:, 0] - h[i, 0], h[:, 1] - h[i, 1]
        rot, dist = np.arctan2(dy, dx) - a, np.sqrt(dx * dx + dy * dy)
        pre[i, :, 0] = np.cos(rot) * dist / cell_size + cell_num / 2
        pre[i, :, 1] = np.sin(rot) * dist / cell_size + cell_num / 2
        pre[i, i] = np.nan
        vrot, speed = np.arctan2(h[:, 3], h[:, 2]) - a, np.sqrt(h[:, 2] ** 2 + h[:, 3] ** 2)
        ovx, ovy = np.cos(vrot) * speed, np.sin(vrot) * speed
        with np.errstate(invalid="ignore"):
            ix, iy = np.floor(pre[i, :, 0]), np.floor(pre[i, :, 1])
            inside = (ix >= 0) & (ix < cell_num) & (iy >= 0) & (iy < cell_num)      # (a NaN fails every comparison)
        for j in np.nonzero(inside)[0]:
            members[int(cell_num * iy[j] + ix[j])].append((ovx[j], ovy[j]))
        for cell, m in enumerate(members):
            occ = 1.0 if m else 0.0
            mean = [sum(v[k] for v in m) / len(m) if m else 0.0 for k in (0, 1)]
            maps[i, cell * channels:(cell + 1) * channels] = {1: [occ], 2: mean, 3: [occ] + mean}[channels]
    return maps, pre


def near_edge(pre, cell_num, exempt_centre=False):
    """bool [n][n]: pairs whose pre-floor coordinate lies within EDGE of an integer that is a cell edge of the grid or beside it.
    exempt_centre: a coordinate of exactly cell_num / 2 (a coincident pair: float32 gives the same exact value) does not count."""
    with np.errstate(invalid="ignore"):
        close = np.abs(pre - np.round(pre)) <= EDGE
        if exempt_centre:
            close &= pre != cell_num / 2
        close &= (pre > -1) & (pre < cell_num + 1)        # far outside the grid no rounding changes the verdict
    return np.any(close & ~np.isnan(pre), axis=-1)


def occupancy_columns(cells, channels):
    """(occupancy column indices, mean-velocity column indices) of a map row"""
    occ = [c * channels for c in range(cells)] if channels != 2 else []
    vel = [c * channels + k for c in range(cells) for k in range(channels) if not (channels != 2 and k == 0)]
    return np.array(occ, int), np.array(vel, int)


def random_worlds(seed, W, n, stride, vel_col):
    """float32 [W][n][stride]: positions within 2.5 m of a common centre, velocities within 1 m/s at vel_col, the other columns noise"""
    rng = np.random.default_rng(seed)
    h = rng.normal(size=(W, n, stride)).astype(F32)
    centre = rng.uniform(-5, 5, size=(W, 1, 2))
    h[..., 0:2] = (centre + rng.uniform(-2.5, 2.5, size=(W, n, 2))).astype(F32)
    h[..., vel_col:vel_col + 2] = rng.uniform(-1, 1, size=(W, n, 2)).astype(F32)
    return h


def reference_rows(humans, stride, vel_col, cfg):
    """maps64 of every world of a random case with the rows to leave out: (want [W][n][C] float64, keep bool [W][n]).  A row is left out
    when one of its pairs lies within EDGE cells of an edge in float64; at most 1 % of a case's rows may be (asserted here, on the CPU)."""
    W, n = humans.shape[:2]
    cell_num, cell_size, channels = cfg
    want = np.zeros((W, n, cell_num * cell_num * channels))
    keep = np.ones((W, n), bool)
    for w in range(W):
        hw = humans[w][:, [0, 1, vel_col, vel_col + 1]]
        want[w], pre = maps64(hw, cell_num, cell_size, channels)
        keep[w] = ~np.any(near_edge(pre, cell_num), axis=1)
    left_out = int((~keep).sum())
    assert left_out <= 0.01 * W * n, f"{left_out} of {W * n} rows have a pair within {EDGE} cells of an edge"
    return want, keep


def draw_weights(model, seed, calm=True):
    """Golden G19's draw_weights: N(0, 0.25) matrices and N(0, 0.1) biases from numpy's frozen RandomState stream in the sorted order of the
    state_dict keys, SARL's attention output layer times 0.1.  Returns the SHA-256 of the float32 bytes."""
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
