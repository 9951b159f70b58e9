"""Input builders and the host reference of the laser-scan tests: tests/test_laser_cpu.py proves the conditions on these inputs without a
device, tests/test_gpu_laser.py runs cs_laser_scan (csrc/laser.hip) on them, every world and every ray.

Everything here is host numpy.  A case is a dict: S [W, rows, 13] float32 state rows (x, y in columns 0, 1, the radius in column 8; the first
`n` rows are the humans), pose [W, 3] float32 (x, y, yaw), rng (float32 opening angle), samples, md (max_distance), walls (None, [O, Smax, 2, 2]
shared or [W, O, Smax, 2, 2] per world, NaN-padded).  One section per case set:
  far discs        12 discs per world at 0.6 .. 9.9 m inside the fan: where b * b - c of the reference's disc formula loses its digits in float32
  launch edges     samples {1, 2, 63, 64, 65, 129} x W {1, 3, 67}, n {0, 1, 25, 64}, max_distance {4, 10}, a sensor inside a disc
  per-world walls  a different NaN-padded polygon set per world, and one of them once more as a shared array
  poisoned rows    NaN in every state and pose column a scan has no business reading
  robot row        rows = n + 1: a sensor 2 m from the robot row's disc, one ray through its centre
  grid y           65 537 worlds of one disc dead ahead

The reference is scan64, the bound of a ray comes from scan64 alone (reference()): nothing here looks at what a kernel returns."""
import functools

import numpy as np

F32 = np.float32
BAR = 1e-5              # the project's parity bar for a float32 kernel against float64 (README, round 6)
ANGLE_ERR = 2.0 ** -20  # rad: two float32 ulps at 2 pi, the largest angle a scan forms; the kernel rounds three times on the way to the angle
PROBE = 1e-5            # rad: the rotation that measures a ray's sensitivity to its angle
EDGE_SLACK = 1e-4       # m: a ray whose slack exceeds this sits on a hit / miss boundary, a grazing hit or a segment end
FAR = 7.0               # m: "at range"


# ---------------------------------------------------------------------------------------------------------------- the ray cast
def _cast(pos, ang, hp, hr, walls, md, dtype, disc="reference"):
    """LaserSensor.get_laser_measurements without noise (sensors.py:51-66) for W sensors at once, every operation in `dtype`.
    pos [W, 2], ang [W, K], hp [W, n, 2], hr [W, n], walls None | [1 | W, M, 2, 2] -> [W, K].
    disc: "reference" = sphere_ray_intersect as written (:24-33: c = |s|^2 - r^2, h = b^2 - c), "cross" = the same real number as
    h = r^2 - (s x d)^2 (d is a unit vector).  Walls: segment_ray_intersect (:35-49) with (x3 - x4, y3 - y4) = -(dx, dy)."""
    dt = np.dtype(dtype).type
    pos, ang, md = np.asarray(pos, dtype), np.asarray(ang, dtype), dt(md)
    dx, dy = np.cos(ang).astype(dtype)[:, :, None], np.sin(ang).astype(dtype)[:, :, None]        # [W, K, 1]
    x3, y3 = pos[:, 0][:, None, None], pos[:, 1][:, None, None]                                  # [W, 1, 1]
    out = np.full(ang.shape, md, dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        if hp.shape[1]:
            hp, r = np.asarray(hp, dtype), np.asarray(hr, dtype)[:, None, :]
            sx, sy = x3 - hp[:, None, :, 0], y3 - hp[:, None, :, 1]                              # [W, 1, n]
            b = sx * dx + sy * dy
            if disc == "reference":
                h = b * b - (sx * sx + sy * sy - r * r)
            else:
                x = sx * dy - sy * dx
                h = r * r - x * x
            t = -b - np.sqrt(h)
            t = np.where((h >= 0) & (t >= 0), np.minimum(t, md), md)                             # h < 0: no hit; t < 0: the sensor is inside
            out = np.minimum(out, t.min(axis=2))
        if walls is not None:
            sg = np.asarray(walls, dtype)
            x1, y1, x2, y2 = (sg[:, None, :, i, j] for i, j in ((0, 0), (0, 1), (1, 0), (1, 1)))  # [1 | W, 1, M]
            den = (x1 - x2) * (-dy) - (y1 - y2) * (-dx)
            t = ((x1 - x3) * (-dy) - (y1 - y3) * (-dx)) / den
            u = -((x1 - x2) * (y1 - y3) - (y1 - y2) * (x1 - x3)) / den
            ix, iy = x1 + t * (x2 - x1), y1 + t * (y2 - y1)
            d = np.sqrt((x3 - ix) * (x3 - ix) + (y3 - iy) * (y3 - iy))
            hit = ~np.isnan(x1) & (den > 0) & (t > 0) & (t < 1) & (u > 0)                        # one-sided: den <= 0 sees nothing
            out = np.minimum(out, np.where(hit, np.minimum(d, md), md).min(axis=2))
    return out


def _flat_walls(walls):
    """None | [O, S, 2, 2] | [W, O, S, 2, 2] -> None | [1 | W, O * S, 2, 2]"""
    if walls is None:
        return None
    walls = np.asarray(walls)
    return walls.reshape((1 if walls.ndim == 4 else walls.shape[0], -1, 2, 2))


def angles64(pose, rng, samples):
    """np.linspace(yaw - range / 2, yaw + range / 2, samples) (sensors.py:55) per world in float64 from the float32 yaw and range: [W, samples]"""
    yaw, half = np.asarray(pose, F32)[:, 2].astype(np.float64), np.float64(F32(rng)) / 2.0
    return np.linspace(yaw - half, yaw + half, int(samples), axis=-1)


def scan64(pose, discs, radius, walls, rng, samples, md, offset=0.0):
    """The float64 answer on the float32-rounded inputs: pose [W, 3], discs [W, n, 2], radius [W, n], walls as in a case -> [W, samples].
    `offset` (rad) rotates every ray: the probe of reference()."""
    up = lambda a: np.asarray(a, F32).astype(np.float64)
    return _cast(up(pose)[:, 0:2], angles64(pose, rng, samples) + offset, up(discs), up(radius), None if walls is None else up(_flat_walls(walls)),
                 np.float64(F32(md)), np.float64)


def scan32(pose, discs, radius, walls, rng, samples, md, disc):
    """The kernel's statement in numpy float32 (no FMA contraction, numpy's cos / sin): the angle as k_laser_scan builds it (start + k * step,
    the last sample the stop value), then _cast in float32 with the reference's disc formula ("reference") or the cross-product form ("cross")."""
    yaw, half = np.asarray(pose, F32)[:, 2], F32(rng) * F32(0.5)
    start, stop = yaw - half, yaw + half
    k = np.arange(int(samples), dtype=F32)[None, :]
    ang = np.broadcast_to(start[:, None], (len(yaw), int(samples))).copy()
    if samples > 1:
        ang = start[:, None] + k * ((stop - start) / F32(samples - 1))[:, None]
        ang[:, -1] = stop
    return _cast(np.asarray(pose, F32)[:, 0:2], ang.astype(F32), np.asarray(discs, F32), np.asarray(radius, F32),
                 None if walls is None else _flat_walls(walls).astype(F32), F32(md), F32, disc)


# ---------------------------------------------------------------------------------------------------------------- the bound
def bound(pose, discs, radius, walls, rng, samples, md):
    """dict(m, slack, edge, hit) [W, samples] from scan64 alone.  kappa = max |scan64(angle +- PROBE) - m| / PROBE (m / rad), slack = kappa *
    ANGLE_ERR; an edge ray (slack > EDGE_SLACK) is left out, every other ray owes |got - m| <= BAR + slack."""
    args = (pose, discs, radius, walls, rng, samples, md)
    m = scan64(*args)
    kappa = np.maximum(np.abs(scan64(*args, offset=PROBE) - m), np.abs(scan64(*args, offset=-PROBE) - m)) / PROBE
    slack = kappa * ANGLE_ERR
    return dict(m=m, slack=slack, edge=slack > EDGE_SLACK, hit=m < np.float64(F32(md)))


def case_args(c):
    return c["pose"], c["S"][:, :c["n"], 0:2], c["S"][:, :c["n"], 8], c["walls"], c["rng"], c["samples"], c["md"]


def reference(c):
    """bound() of a case, computed once and kept on the case"""
    if "ref" not in c:
        c["ref"] = bound(*case_args(c))
        for v in c["ref"].values():
            v.setflags(write=False)
    return c["ref"]


def excess(got, ref):
    """|got - m| - slack over the kept rays (edge rays: -inf), [W, samples]: the test holds its maximum to BAR"""
    return np.where(ref["edge"], -np.inf, np.abs(np.asarray(got, np.float64) - ref["m"]) - ref["slack"])


def same_words(a, b):
    """float32 arrays equal as raw 32-bit words"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.all(a.view(np.uint32) == b.view(np.uint32)))


def shares(cases):
    """(edge share of all rays, edge share of the hits, kept hits beyond FAR) over a case set"""
    refs = [reference(c) for c in cases]
    rays = sum(r["m"].size for r in refs)
    hits = sum(int(r["hit"].sum()) for r in refs)
    edge = sum(int(r["edge"].sum()) for r in refs)
    edge_hits = sum(int((r["edge"] & r["hit"]).sum()) for r in refs)
    far = sum(int((r["hit"] & ~r["edge"] & (r["m"] > FAR)).sum()) for r in refs)
    return edge / rays, (edge_hits / hits if hits else 0.0), far


# ---------------------------------------------------------------------------------------------------------------- builders
def _case(name, S, n, pose, rng, samples, md, walls=None, **extra):
    c = dict(name=name, S=np.ascontiguousarray(S, F32), n=int(n), pose=np.ascontiguousarray(pose, F32), rng=F32(rng), samples=int(samples),
             md=float(md), walls=None if walls is None else np.ascontiguousarray(walls, F32), **extra)
    assert np.all(np.abs(c["pose"][:, 2]) <= np.pi)          # LaserSensor.update_pose: the largest angle of a scan is 2 pi
    for v in (c["S"], c["pose"], c["walls"]):
        if v is not None:
            v.setflags(write=False)
    return c


def _poses(r, W, span=3.0):
    return np.concatenate([r.uniform(-span, span, (W, 2)), r.uniform(-np.pi, np.pi, (W, 1)) * 0.999], axis=1)


def _rows(W, n, fill=0.0):
    return np.full((W, n, 13), fill, F32)


def _discs_in_fan(r, pose, n, rng, near, far, rmin=0.2, rmax=0.5):
    """n discs per world at `near` .. `far` m from the sensor, bearings inside the fan (the whole circle for 2 pi): rows [W, n, 13]"""
    W = len(pose)
    dist = r.uniform(near, far, (W, n))
    bearing = pose[:, 2:3] + r.uniform(-0.5, 0.5, (W, n)) * rng
    S = _rows(W, n)
    S[:, :, 0] = pose[:, 0:1] + dist * np.cos(bearing)
    S[:, :, 1] = pose[:, 1:2] + dist * np.sin(bearing)
    S[:, :, 8] = r.uniform(rmin, rmax, (W, n))
    return S


def box(half):
    """A square of side 2 * half about the origin in both windings, [2, 4, 2, 2]: segment_ray_intersect sees a segment from one side only"""
    v = np.array([[-half, -half], [half, -half], [half, half], [-half, half]], np.float64)
    ccw = np.stack([np.stack([v[j], v[(j + 1) % 4]]) for j in range(4)])
    return np.stack([ccw, ccw[:, ::-1]])


def polygons_and_box(half=7.5, smax=5):
    """scenarios.polygon_walls() (3, 4, 5 segments) and the 15 m box in both windings: [5, smax, 2, 2], NaN-padded"""
    from social_navigation_pyenvs_amd import scenarios as sc

    arr = np.full((5, smax, 2, 2), np.nan)
    arr[:3, :5] = sc.polygon_walls()
    arr[3:, :4] = box(half)
    return arr


FAR_W = 260            # worlds per opening angle
FAR_RANGES = (np.pi / 2, np.pi, 2 * np.pi)


@functools.lru_cache(maxsize=None)
def far_discs():
    """Three cases (one per opening angle) of FAR_W worlds x 12 discs at 0.6 .. 9.9 m, radius 0.2 .. 0.5, 181 rays, max_distance 10"""
    cases = []
    for j, rng in enumerate(FAR_RANGES):
        r = np.random.default_rng([j, 71])
        pose = _poses(r, FAR_W)
        cases.append(_case(f"far discs, range {rng:.3f}", _discs_in_fan(r, pose, 12, rng, 0.6, 9.9), 12, pose, rng, 181, 10.0))
    return tuple(cases)


EDGE_SAMPLES = (1, 2, 63, 64, 65, 129)
EDGE_W = (1, 3, 67)
EDGE_N = (0, 1, 25, 64)


@functools.lru_cache(maxsize=None)
def launch_edges():
    """samples x W, n and max_distance cycling through their values, the opening angle through 2 pi (first ray = last ray modulo 2 pi), pi and
    2.5; walls (polygons and the 15 m box, shared) in two cases of three; with n > 0 the sensor of world 0 stands inside its disc 0."""
    cases = []
    for i, samples in enumerate(EDGE_SAMPLES):
        for j, W in enumerate(EDGE_W):
            q = i * len(EDGE_W) + j
            n, md, rng = EDGE_N[(i + j) % 4], (4.0, 10.0)[q % 2], (2 * np.pi, np.pi, 2.5)[(i + 2 * j) % 3]
            r = np.random.default_rng([samples, W, 72])
            pose = _poses(r, W)
            S = _discs_in_fan(r, pose, n, rng, 0.8, 9.0) if n else _rows(W, 0)
            if n:
                S[0, 0, 0:2], S[0, 0, 8] = pose[0, 0:2] + (0.1, -0.05), 0.4
            walls = polygons_and_box() if q % 3 != 2 or n == 0 else None
            cases.append(_case(f"launch edges, samples {samples} W {W} n {n} md {md:g}", S, n, pose, rng, samples, md, walls))
    return tuple(cases)


WALL_W = 40


def _world_walls(w):
    """World w's polygon set [6, 5, 2, 2]: polygon_walls() turned by 0.37 w about the origin, a box of half side 5 + 0.05 w in both windings
    (every world's box 5 cm further out than its predecessor's: a ray cast against a neighbour's walls misses the bound by far), and one
    all-NaN polygon whose slot moves with w."""
    from social_navigation_pyenvs_amd import scenarios as sc

    a = 0.37 * w
    rot = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    polys = [sc.polygon_walls()[i] @ rot.T for i in range(3)]
    bx = np.full((2, 5, 2, 2), np.nan)
    bx[:, :4] = box(5.0 + 0.05 * w)
    polys += [bx[0], bx[1]]
    polys.insert(w % 6, np.full((5, 2, 2), np.nan))
    return np.stack(polys)


@functools.lru_cache(maxsize=None)
def per_world_walls():
    """(per-world case, shared case): WALL_W worlds, 3 discs, 91 rays over 2 pi, max_distance 10; walls [W, 6, 5, 2, 2] = _world_walls(w), and
    the same worlds with world 7's walls as one shared [6, 5, 2, 2] array"""
    r = np.random.default_rng(73)
    pose = _poses(r, WALL_W, span=1.5)
    pose[:, 0:2] += (3.0, -2.5)                       # clear of the turned polygons' ring: few sensors inside a polygon
    pose[1::2] = pose[0::2]                           # neighbours share a pose: only their walls tell them apart
    S = _discs_in_fan(r, pose, 3, 2 * np.pi, 0.8, 4.0)
    walls = np.stack([_world_walls(w) for w in range(WALL_W)])
    return (_case("per-world walls", S, 3, pose, 2 * np.pi, 91, 10.0, walls), _case("shared walls", S, 3, pose, 2 * np.pi, 91, 10.0, walls[7]))


SCAN_STATE_COLUMNS = (0, 1, 8)


@functools.lru_cache(maxsize=None)
def poisoned_rows():
    """One case: 5 worlds x 7 discs and the walls; every state column but x, y, radius is NaN.  c["robot"] [W, 13]: the pose in columns 0, 1, 2
    and NaN behind it (the robot rows of a CrowdWorlds); c["pose5"] [W, 5]: the same with two NaN columns (a pose_stride of 5)."""
    r = np.random.default_rng(74)
    W, n = 5, 7
    pose = _poses(r, W)
    S = _discs_in_fan(r, pose, n, np.pi, 0.8, 9.0)
    keep = S[:, :, SCAN_STATE_COLUMNS].copy()
    S[:] = np.nan
    S[:, :, SCAN_STATE_COLUMNS] = keep
    robot, pose5 = np.full((W, 13), np.nan, F32), np.full((W, 5), np.nan, F32)
    robot[:, 0:3] = pose5[:, 0:3] = pose
    return _case("poisoned rows", S, n, pose, np.pi, 65, 10.0, polygons_and_box(), robot=robot, pose5=pose5)


ROBOT_GAP = 2.0        # m between the explicit sensor pose and the centre of the robot row's disc


@functools.lru_cache(maxsize=None)
def robot_row():
    """One case: 12 hybrid worlds (scenarios.hybrid_worlds) x 25 humans and the robot as row 25 (radius 0.3), S [W, 26, 13].  The explicit
    pose stands ROBOT_GAP from the robot's centre and looks at it: ray 32 of 65 goes through the centre.  The reference scans the 25 humans.
    c["goals"], c["params"], c["robot"] [W, 13] build the CrowdWorlds."""
    from social_navigation_pyenvs_amd import scenarios as sc

    W, n = 12, 25
    S, goals, P, _ = sc.hybrid_worlds(W, n, "hsfm_farina")
    r = np.random.default_rng(75)
    robot = np.zeros((W, 13))
    robot[:, 0:2] = r.uniform(-3, 3, (W, 2)); robot[:, 2] = r.uniform(-3, 3, W); robot[:, 8] = 0.3; robot[:, 9] = 80
    robot[:, 10:12] = -robot[:, 0:2]; robot[:, 12] = 1.0
    robot = robot.astype(F32)
    S = np.concatenate([S.astype(F32), robot[:, None, :]], axis=1)
    phi = r.uniform(-np.pi, np.pi, W) * 0.999
    pose = np.stack([robot[:, 0] - ROBOT_GAP * np.cos(phi), robot[:, 1] - ROBOT_GAP * np.sin(phi), phi], axis=1)
    return _case("robot row", S, n, pose, np.pi / 2, 65, 10.0, None, goals=goals.astype(F32), params=P.astype(F32), robot=robot)


GRID_W = 65537         # one more than a 16-bit grid extent holds


@functools.lru_cache(maxsize=None)
def grid_y():
    """One case: GRID_W worlds, one disc (radius 0.3) dead ahead of each sensor at 0.5 + 2.5 w / W m, two rays, opening angle 0.  Neighbouring
    worlds differ by 3.8e-5 m, four times the bar: a world that reads another world's rows shows."""
    w = np.arange(GRID_W, dtype=np.float64)
    pose = np.stack([np.cos(w) * 2.0, np.sin(0.7 * w) * 2.0, (w % 629) / 100.0 - np.pi + 0.001], axis=1)
    dist = 0.5 + 2.5 * w / GRID_W
    S = _rows(GRID_W, 1)
    S[:, 0, 0] = pose[:, 0] + dist * np.cos(pose[:, 2])
    S[:, 0, 1] = pose[:, 1] + dist * np.sin(pose[:, 2])
    S[:, 0, 8] = 0.3
    return _case("grid y", S, 1, pose, 0.0, 2, 10.0, None, dist=dist)


CASE_SETS = {"far discs": far_discs, "launch edges": launch_edges, "per-world walls": per_world_walls, "poisoned rows": lambda: (poisoned_rows(),),
             "robot row": lambda: (robot_row(),), "grid y": lambda: (grid_y(),)}
