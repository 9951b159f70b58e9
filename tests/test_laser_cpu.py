"""The laser-scan cases of tests/laser_cases.py without a device: scan64 is the oracle's scan, the inputs meet the caps the bound needs, a
float32 statement of the reference's disc formula breaks the bound at range (the test has teeth) and the cross-product form and the float32
wall formula keep it (the bound is attainable).  tests/test_gpu_laser.py holds cs_laser_scan to the same bound on the same inputs."""
import numpy as np
import pytest

import laser_cases as lc
from oracle import crowd_oracle as orc

SETS = list(lc.CASE_SETS)


def _sampled_worlds(c):
    W = len(c["pose"])
    return sorted({0, W // 2, W - 1})


@pytest.mark.parametrize("name", SETS)
def test_scan64_is_the_oracles_scan(name):
    rays = 0
    for c in lc.CASE_SETS[name]():
        pose, discs, radius, walls, rng, samples, md = lc.case_args(c)
        got = lc.reference(c)["m"]
        for w in _sampled_worlds(c):
            ow = None if walls is None else (walls if walls.ndim == 4 else walls[w]).astype(np.float64)
            ang, ref = orc.laser_scan(pose[w, 0:2].astype(np.float64), pose[w, 2], rng, samples, np.float64(np.float32(md)), discs[w].astype(np.float64),
                                      radius[w].astype(np.float64), ow, dtype=np.float64)
            np.testing.assert_array_equal(lc.angles64(pose[w:w + 1], rng, samples)[0], ang)
            np.testing.assert_allclose(got[w], ref, rtol=0, atol=1e-12)
            rays += samples
    assert rays >= 4


@pytest.mark.parametrize("name", SETS)
def test_case_sets_meet_the_caps(name):
    cases = lc.CASE_SETS[name]()
    edge_rays, edge_hits, far = lc.shares(cases)
    print(f"{name}: edge share of rays {edge_rays:.5f}, of hits {edge_hits:.5f}, kept hits beyond {lc.FAR:g} m {far}")
    assert edge_rays <= 0.01 and edge_hits <= 0.01
    if name == "far discs":
        assert far >= 5000
    for c in cases:
        assert np.all(np.isfinite(lc.reference(c)["m"])) and np.all(lc.reference(c)["m"] >= 0)


def test_builders_cover_what_they_name():
    edges = lc.launch_edges()
    assert {(c["samples"], len(c["pose"])) for c in edges} == {(s, w) for s in lc.EDGE_SAMPLES for w in lc.EDGE_W}
    assert {c["n"] for c in edges} == set(lc.EDGE_N) and {c["md"] for c in edges} == {4.0, 10.0}
    assert any(c["walls"] is None for c in edges) and any(c["walls"] is not None and c["n"] == 0 for c in edges)
    for c in edges:
        if c["n"]:                                        # the sensor of world 0 stands inside its disc 0, which therefore hides nothing
            assert np.hypot(*(c["S"][0, 0, 0:2] - c["pose"][0, 0:2])) < c["S"][0, 0, 8]
        far_discs = np.hypot(*np.moveaxis(c["S"][:, :c["n"], 0:2] - c["pose"][:, None, 0:2], -1, 0)) - c["S"][:, :c["n"], 8]
        assert c["md"] > 4.0 or c["n"] < 25 or np.any(far_discs > c["md"])       # discs beyond max_distance
    two_pi = [c for c in edges if c["rng"] == np.float32(2 * np.pi) and c["samples"] > 1]
    assert len(two_pi) >= 4                               # the first and the last ray coincide modulo 2 pi (to the rounding of float32(2 pi))
    for c in two_pi:
        keep = ~(lc.reference(c)["edge"][:, 0] | lc.reference(c)["edge"][:, -1])
        np.testing.assert_allclose(lc.reference(c)["m"][keep, 0], lc.reference(c)["m"][keep, -1], rtol=0, atol=1e-5)

    per_world, shared = lc.per_world_walls()
    wl = per_world["walls"]
    assert wl.ndim == 5 and shared["walls"].ndim == 4 and np.array_equal(shared["walls"], wl[7], equal_nan=True)
    nan_poly = np.all(np.isnan(wl), axis=(2, 3, 4))
    assert np.all(nan_poly.sum(axis=1) == 1) and len({int(np.argmax(p)) for p in nan_poly}) == wl.shape[1]      # one all-NaN polygon, its slot moves
    segs = (~np.isnan(wl[..., 0, 0])).sum(axis=2)
    assert np.any((segs > 0) & (segs < wl.shape[2]))      # polygons with fewer than Smax segments
    # the offset trap: world w cast against world w - 1's walls misses the bound on a large part of its rays
    ref = lc.reference(per_world)
    pose, discs, radius, _, rng, samples, md = lc.case_args(per_world)
    wrong = lc.scan64(pose, discs, radius, np.roll(wl, 1, axis=0), rng, samples, md)
    missed = (lc.excess(wrong, ref) > lc.BAR).mean(axis=1)
    assert np.all(missed > 0.25), missed.min()

    p = lc.poisoned_rows()
    other = [k for k in range(13) if k not in lc.SCAN_STATE_COLUMNS]
    assert np.all(np.isnan(p["S"][:, :, other])) and np.all(np.isfinite(p["S"][:, :, lc.SCAN_STATE_COLUMNS]))
    assert np.all(np.isnan(p["robot"][:, 3:])) and np.all(np.isnan(p["pose5"][:, 3:])) and np.array_equal(p["robot"][:, 0:3], p["pose"])

    g = lc.grid_y()
    m = lc.reference(g)["m"]
    assert len(g["pose"]) == 65537 and not lc.reference(g)["edge"].any()
    np.testing.assert_allclose(m, np.repeat(g["dist"][:, None] - 0.3, 2, axis=1), rtol=0, atol=2e-6)        # (float32-rounded inputs)
    assert np.all(np.diff(m[:, 0]) > 3 * lc.BAR)          # a world that reads its neighbour's rows misses the bound


def test_robot_row_case_tells_a_scan_of_the_robot_row():
    c = lc.robot_row()
    n, mid = c["n"], c["samples"] // 2
    assert c["S"].shape[1] == n + 1 and np.array_equal(c["S"][:, n], c["robot"])
    ref = lc.reference(c)
    with_robot = lc.scan64(c["pose"], c["S"][:, :, 0:2], c["S"][:, :, 8], None, c["rng"], c["samples"], c["md"])
    # the ray through the centre of the robot row's disc: a kernel that scans rows = n + 1 reads ROBOT_GAP - radius there ...
    seen = np.abs(with_robot[:, mid] - (lc.ROBOT_GAP - 0.3)) < 1e-5
    # ... and the reference, which scans the n humans, something else by far in most worlds
    assert (seen & (ref["m"][:, mid] > lc.ROBOT_GAP) & ~ref["edge"][:, mid]).sum() >= len(c["pose"]) // 2


def _far(ref):
    return ref["hit"] & ~ref["edge"] & (ref["m"] > lc.FAR)


def test_float32_reference_disc_formula_breaks_the_bound_at_range():
    bad = total = 0
    for c in lc.far_discs():
        ref = lc.reference(c)
        ex = lc.excess(lc.scan32(*lc.case_args(c), "reference"), ref)
        bad += int((ex[_far(ref)] > lc.BAR).sum())
        total += int(_far(ref).sum())
    print(f"float32 b * b - c on the far-disc set: {bad} of {total} kept hits beyond {lc.FAR:g} m miss the bound")
    assert bad >= 0.01 * total
    # the oracle's own float32 instantiation (its angles from np.linspace in float32) on the first worlds of the widest fan
    c = lc.far_discs()[-1]
    pose, discs, radius, _, rng, samples, md = lc.case_args(c)
    ref = lc.reference(c)
    worlds = range(12)
    got = np.stack([orc.laser_scan(pose[w, 0:2], pose[w, 2], rng, samples, md, discs[w], radius[w], None, dtype=np.float32)[1] for w in worlds])
    sub = {k: v[:len(worlds)] for k, v in ref.items()}
    ex = lc.excess(got, sub)
    assert (ex[_far(sub)] > lc.BAR).sum() >= 0.01 * _far(sub).sum()


@pytest.mark.parametrize("name", SETS)
def test_float32_cross_form_and_wall_formula_keep_the_bound(name):
    worst = -np.inf
    for c in lc.CASE_SETS[name]():
        worst = max(worst, float(lc.excess(lc.scan32(*lc.case_args(c), "cross"), lc.reference(c)).max()))
    print(f"{name}: float32 cross-product form and wall formula, worst |got - m| - slack over kept rays {worst:.3e}")
    assert worst <= lc.BAR
