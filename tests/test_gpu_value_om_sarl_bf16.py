"""GPU suite of the opt-in bf16 arithmetic of OM-SARL's decision (cs_value_net_decide_om_bf16, csrc/value_net_om_bf16.hip; Python:
``OMSARL.set_wide_precision("bf16")``).  The reference is tests/om_sarl_bf16_emulation.py, the float64 restatement of the arithmetic's
contract; the rows and rewards are cs_lookahead's and the maps cs_occupancy_maps' on synthetic worlds whose humans are
pulled together so that the maps are filled, and golden G20 (c).

The bar of the comparison is the project's rule for one float32 realisation against another (parity_util.F32_SLACK): the kernel's worst
relative action-value error against the float64 emulation is at most F32_SLACK times the error of the emulation's own
float32-accumulation mode against its float64 mode, over the same sweep.  No case is excluded.

Every comparison between two launches of this library is bitwise unless it says otherwise."""
import numpy as np
import pytest

import bf16_emulation as em
import decision_edges as de
import om_sarl_bf16_emulation as oem
import parity_util
from test_gpu_value_bf16 import WIDTHS
from test_gpu_value_om import compare_maps
from test_gpu_value_worlds import worlds
from test_value_om_cpu import g20, g20_policy, om_policy
from test_value_om_sarl_bf16_cpu import GRIDS, g20_decision_values, narrow_twin, wide_model
from test_value_policy_cpu import numpy_weights
from value_calls import DT, GAMMA, _stream, _up, lookahead_call

pytestmark = pytest.mark.gpu

F32 = np.float32
N_WIDE = [2, 16, 17, 31, 32, 33, 70]                # whole groups a tile, one group and zero rows behind it, one full tile, chunks
WA = de.WA_SWEEP[:4]                                # W * A of 1, 31, 32, 33
ODD_WIDTHS = {k.split("__")[1].replace("_dims", ""): [int(x) for x in v.split(",")] for k, v in WIDTHS.items()}      # 40, 256 | 72, 33 | 20, 1 | 90, 1


def device_net(model, cols, C_):
    """The DeviceNet of a module moved to the GPU, both blobs packed"""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    net = value_net.DeviceNet(model.to(torch.device("cuda")), cols, C_, GRIDS[C_])
    net.refresh_selected("f32", "f32", "f32", "bf16")
    return net


def rows_and_maps(W, n, A, cols, C_, seed):
    """cs_lookahead's rows and rewards and cs_occupancy_maps' maps of the next humans (the first C_ columns of GRIDS[C_]'s) for synthetic
    worlds whose humans are pulled towards their robot (halfway; two humans alone to a fifth, or the smallest grids stay empty): device
    tensors rot [W, A, n, cols], rew [W, A], maps [W, n, C_]; acts, rob numpy"""
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    acts, nxt, cur, rob = worlds(W, n, A, cols == 15, seed=seed)
    pull = F32(0.5 if n > 2 else 0.2)
    nxt[..., 0:2] = rob[:, None, 0:2] + (nxt[..., 0:2] - rob[:, None, 0:2]) * pull            # closer together: filled maps
    cur[..., 0:2] = rob[:, None, 0:2] + (cur[..., 0:2] - rob[:, None, 0:2]) * pull
    rot, rew = lookahead_call(acts, nxt, cur, rob)
    maps = value_net.maps_of(_up(nxt), 3 if cols == 15 else 2, GRIDS[C_], _stream())[..., :C_].contiguous()
    return rot, rew, maps, acts, rob


def decide_wide(net, rot, rew, acts, rob, maps, gamma=GAMMA, dt=DT):
    """value_net.decide_om_bf16 on device tensors / host arrays: (values [W, A], choice [W], action [W, 2]) numpy; the outputs start as NaN / -5"""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    W, A, n, _ = rot.shape
    vals = torch.full((W, A), np.nan, device="cuda")
    pick = torch.full((W,), -5, dtype=torch.int32, device="cuda")
    act = torch.full((W, 2), np.nan, device="cuda")
    d_rot, d_rew, d_acts, d_rob, d_maps = (_up(a, torch.float32) for a in (rot, rew, acts, rob, maps))
    assert tuple(d_maps.shape) == (W, n, net.om_cols) and d_maps.is_contiguous() and d_rot.is_contiguous()
    value_net.decide_om_bf16(net, W, A, n, d_rot.data_ptr(), d_maps.data_ptr(), d_rew.data_ptr(), d_acts.data_ptr(), d_rob.data_ptr(), d_rob.shape[1], gamma, dt,
                             None, vals.data_ptr(), pick.data_ptr(), act.data_ptr(), _stream())
    torch.cuda.synchronize()
    return vals.cpu().numpy(), pick.cpu().numpy(), act.cpu().numpy()


# (cols, C, with_global, widths, weight scale, sweep of (n, W, A)): every n with every W * A on the reference's network; every other axis
# -- the crowd mean, 15 columns, the map columns on, one over and far beyond a k-step of 16, one column, widths off 16 -- crossed with the
# tile edges of n
VARIANTS = {
    "default": (13, 48, True, None, 1.0, [(n, W, A) for n in N_WIDE for W, A in WA] + [(5, 2, 81), (33, 2, 81)]),
    "no global": (13, 48, False, None, 1.0, [(n, 3, 11) for n in N_WIDE]),
    "15 columns": (15, 48, True, None, 1.0, [(n, 3, 11) for n in (2, 17, 32, 33)] + [(16, 1, 32), (70, 31, 1)]),
    "1 map column": (15, 1, True, None, 1.0, [(n, 3, 11) for n in (2, 16, 31, 33)] + [(17, 1, 32), (32, 31, 1)]),
    "16 map columns": (13, 16, False, None, 1.0, [(n, 3, 11) for n in (2, 17, 32, 70)] + [(33, 1, 32), (31, 31, 1)]),
    "17 map columns": (15, 17, True, None, 1.0, [(n, 3, 11) for n in (2, 16, 31, 33, 70)] + [(32, 1, 32)]),
    "192 map columns": (15, 192, True, None, 1.0, [(n, 3, 11) for n in (2, 17, 32, 33)] + [(31, 1, 32), (70, 1, 1)]),
    # (a 256-wide layer at N(0, 0.25) blows the activations up: the default init's scale, as test_gpu_value_bf16 takes it)
    "widths": (13, 48, True, ODD_WIDTHS, 0.25, [(n, 3, 11) for n in N_WIDE]),
    "widths, 15 + 17 columns": (15, 17, False, ODD_WIDTHS, 0.25, [(n, 3, 11) for n in (2, 17, 32, 33)] + [(16, 1, 32), (70, 31, 1)]),
}


def test_the_variants_cover_the_axes():
    cases = list(VARIANTS.values())
    assert {c[1] for c in cases} == {1, 16, 17, 48, 192} and {c[0] for c in cases} == {13, 15} and {c[2] for c in cases} == {True, False}
    assert {(W, A) for n, W, A in VARIANTS["default"][5]} >= set(WA) | {(2, 81)} and {n for n, _, _ in VARIANTS["default"][5]} >= set(N_WIDE)
    assert all(w % 16 for widths in (ODD_WIDTHS["mlp1"][:1], ODD_WIDTHS["mlp2"], ODD_WIDTHS["attention"][:1], ODD_WIDTHS["mlp3"][:1]) for w in widths)
    for name, c in VARIANTS.items():
        assert {n for n, _, _ in c[5]} >= {2, 33} and any(n in (16, 17) for n, _, _ in c[5]) and any(n in (31, 32) for n, _, _ in c[5]), name
    assert max(c[0] + c[1] for c in cases) == 207                   # K of mlp1's layer 0


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_kernel_against_the_float64_emulation(variant):
    """Worst relative action-value error of the kernel against the float64 emulation over the variant's sweep (decision_edges.rel_error's
    scale), held to F32_SLACK times the float32-accumulation emulation's error against the same reference over the same sweep.

    Measured on the MI355X: see HISTORY.md ("OM-SARL bf16 decision") for the two figures of every variant."""
    cols, C_, with_global, widths, scale, sweep = VARIANTS[variant]
    model = wide_model(cols, C_, with_global, widths, seed=4600 + C_, scale=scale)
    w = numpy_weights(model)
    net = device_net(model, cols, C_)
    worst = worst32 = 0.0
    for n, W, A in sweep:
        rot, rew, maps, acts, rob = rows_and_maps(W, n, A, cols, C_, seed=7000 + 10 * n + W)
        h_rot, h_rew, h_maps = rot.cpu().numpy(), rew.cpu().numpy(), maps.cpu().numpy()
        assert np.count_nonzero(h_maps) > 0, (variant, n, W, A)
        disc = de.discount(rob, GAMMA, DT)
        e64 = oem.action_values(h_rot, h_maps, h_rew, disc, w, with_global)
        e32 = oem.action_values(h_rot, h_maps, h_rew, disc, w, with_global, acc="f32")
        vals, pick, _ = decide_wide(net, rot, rew, acts, rob, maps)
        assert np.isfinite(e64).all() and np.isfinite(vals).all(), (variant, n, W, A)
        err, err32 = de.rel_error(vals, e64), de.rel_error(e32, e64)
        print(f"{variant} n={n} W={W} A={A}: kernel {err:.3e}, float32-accumulation emulation {err32:.3e}")
        np.testing.assert_array_equal(pick, de.expected_pick(vals))
        worst, worst32 = max(worst, err), max(worst32, err32)
    print(f"OM-SARL bf16 {variant}: worst relative action-value error against the float64 emulation: kernel {worst:.3e}, float32-accumulation emulation {worst32:.3e}")
    parity_util.record(f"OM-SARL bf16 decision: kernel against the float64 emulation, {variant} (relative action value)", worst, bar=de.REL_BAR)
    parity_util.record(f"OM-SARL bf16 decision: float32-accumulation emulation against the float64 emulation, {variant} (relative action value)", worst32, bar=de.REL_BAR)
    assert worst <= parity_util.F32_SLACK * worst32, (variant, worst, worst32)


@pytest.mark.parametrize("n", [2, 17, 32, 33, 70])
def test_zero_map_weights_give_the_values_of_the_narrow_bf16_kernel(n):
    """The map k-steps add +0 behind the float32 k-groups of the same chain: values, choice and action are numerically those of
    cs_value_net_decide_bf16 on the twin SARL network."""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    for i, (W, A) in enumerate(((1, 1), (1, 32), (3, 11), (2, 81))):
        with_global, cols = bool((i + n) % 2), (13, 15)[(i // 2 + n) % 2]
        C_ = (48, 17, 16, 192)[i]
        wide, twin = narrow_twin(wide_model(cols, C_, with_global, seed=4700 + i), cols)
        net = device_net(wide, cols, C_)
        sarl = value_net.DeviceNet(twin.to(torch.device("cuda")), cols)
        sarl.refresh("bf16")
        rot, rew, maps, acts, rob = rows_and_maps(W, n, A, cols, C_, seed=7300 + 10 * n + i)
        assert float(maps.abs().sum()) > 0
        vals = torch.full((W, A), np.nan, device="cuda")
        pick = torch.full((W,), -5, dtype=torch.int32, device="cuda")
        act = torch.full((W, 2), np.nan, device="cuda")
        d_acts, d_rob = _up(acts), _up(rob)
        value_net.decide(sarl, W, A, n, rot.data_ptr(), rew.data_ptr(), d_acts.data_ptr(), d_rob.data_ptr(), d_rob.shape[1], GAMMA, DT, None,
                         vals.data_ptr(), pick.data_ptr(), act.data_ptr(), _stream(), precision="bf16")
        torch.cuda.synchronize()
        want = (vals.cpu().numpy(), pick.cpu().numpy(), act.cpu().numpy())
        got = decide_wide(net, rot, rew, acts, rob, maps)
        assert np.all(np.isfinite(want[0]))
        for g, w_ in zip(got, want):
            assert np.array_equal(g, w_), (n, W, A, with_global, cols, C_)


@pytest.fixture(scope="module")
def default_net():
    model = wide_model(13, 48, seed=4800)
    return numpy_weights(model), device_net(model, 13, 48)


def test_one_map_row_serves_all_actions_of_its_world(default_net):
    _, net = default_net
    rot, rew, maps, acts, rob = rows_and_maps(3, 5, 81, 13, 48, seed=7400)
    base = decide_wide(net, rot, rew, acts, rob, maps)[0]
    moved = maps.clone()
    moved[1] += 0.5
    got = decide_wide(net, rot, rew, acts, rob, moved)[0]
    assert de.same_words(got[0], base[0]) and de.same_words(got[2], base[2]) and np.all(np.isfinite(got))
    assert np.all(got[1] != base[1])


def test_one_world_alone_and_inside_batches_of_33_and_4096(default_net):
    """W = 1 against the same world inside batches of 33 and 4096 (n = 5, A = 11: 45056 groups in 1408 workgroups)"""
    _, net = default_net
    A, n = 11, 5
    rot, rew, maps, acts, rob = rows_and_maps(4096, n, A, 13, 48, seed=7500)
    big = decide_wide(net, rot, rew, acts, rob, maps)
    assert np.isfinite(big[0]).all() and float(maps.abs().sum()) > 0
    cut = lambda lo, hi: (rot[lo:hi].contiguous(), rew[lo:hi].contiguous(), acts, rob[lo:hi], maps[lo:hi].contiguous())
    mid = decide_wide(net, *cut(100, 133))
    for b, m in zip(big, mid):
        np.testing.assert_array_equal(m, b[100:133])
    for w in (0, 100, 117, 132, 4095):
        one = decide_wide(net, *cut(w, w + 1))
        for b, o in zip(big, one):
            np.testing.assert_array_equal(o[0], b[w])


def test_a_nan_map_value_follows_the_emulation(default_net):
    """One NaN in one map row of world 1: rounded to bf16 it stays a NaN, the row's pre-activations, the crowd mean and the softmax's sum
    are NaN, so every action value of that world is -- the emulation's words; the other worlds keep their bits."""
    w, net = default_net
    rot, rew, maps, acts, rob = rows_and_maps(3, 5, 11, 13, 48, seed=7600)
    clean = decide_wide(net, rot, rew, acts, rob, maps)
    bad = maps.clone()
    bad[1, 3, 20] = float("nan")
    vals, pick, _ = decide_wide(net, rot, rew, acts, rob, bad)
    want = oem.action_values(rot.cpu().numpy(), bad.cpu().numpy(), rew.cpu().numpy(), de.discount(rob, GAMMA, DT), w).astype(F32)
    assert np.isnan(want[1]).all() and np.isfinite(want[[0, 2]]).all()
    np.testing.assert_array_equal(np.isnan(vals), np.isnan(want))
    assert de.same_words(vals[1], want[1]) and pick[1] == 0
    assert de.same_words(vals[0], clean[0][0]) and de.same_words(vals[2], clean[0][2]) and pick[0] == clean[1][0] and pick[2] == clean[1][2]


def test_g20_every_flipped_decision_is_explained():
    """G20 (c), the reference's 32 recorded decisions as one batch, decided with the bf16 arithmetic: the pick is the argmax of the returned
    values; a pick that differs from the reference's `chosen` is explained when gap <= 2 e (bf16_emulation.classify_flip), with e from the
    float64 EMULATION on the batch's own rows and maps, never from the kernel.  Zero unexplained flips; the count is recorded."""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    pol = g20_policy("om_sarl_decide")
    w = numpy_weights(pol.model)
    pol.set_phase("test")
    pol.set_device(torch.device("cuda"))
    pol.set_wide_precision("bf16")
    net = pol.device_net()
    cs = g20()["decision"]
    acts = cs[0]["action_space"].astype(F32)
    nxt, cur, rob = (np.stack([c[k] for c in cs]).astype(F32) for k in ("next_humans", "obs", "robot"))
    rot, rew = lookahead_call(acts, nxt, cur, rob, float(cs[0]["dt"]))
    maps = value_net.maps_of(_up(nxt), 2, net.om_grid, _stream())
    compare_maps(maps.cpu().numpy(), np.stack([c["maps"] for c in cs]), net.om_grid)
    vals, pick, _ = decide_wide(net, rot, rew, acts, rob, maps, gamma=float(cs[0]["gamma"]), dt=float(cs[0]["dt"]))
    assert np.isfinite(vals).all()
    np.testing.assert_array_equal(pick, np.argmax(vals, axis=1))
    h_rot, h_rew, h_maps = rot.cpu().numpy(), rew.cpu().numpy(), maps.cpu().numpy()
    flips = 0
    for k, c in enumerate(cs):
        if int(pick[k]) != int(c["chosen"]):
            flips += 1
            full, e64 = g20_decision_values(c, w, h_rot[k], h_maps[k], h_rew[k])
            ok, gap, e = em.classify_flip(int(c["chosen"]), int(pick[k]), full, e64)
            print(f"G20 (c) decision {k}: bf16 picks {int(pick[k])}, the reference {int(c['chosen'])}: gap {gap:.3e}, emulation error e {e:.3e}")
            assert ok, (k, gap, e)
    print(f"G20 (c) OM-SARL bf16: {flips} of {len(cs)} decisions flipped, all explained")
    parity_util.REPORT["OM-SARL bf16 decision: G20 (c) decisions flipped against the reference's choice (all explained by gap <= 2 e)"] = {"decisions": len(cs), "flips": flips}
    assert len(cs) == 32


def test_refusals_with_real_buffers(default_net):
    """cs_value_net_decide_om's messages from the bf16 entry on real device buffers; the float32 blob is refused by its size"""
    import ctypes as C

    import torch

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    _, net = default_net
    rot, rew, maps, acts, rob = rows_and_maps(2, 5, 81, 13, 48, seed=7700)
    d_acts, d_rob = _up(acts), _up(rob)
    vals, act = torch.zeros((2, 81), device="cuda"), torch.zeros((2, 2), device="cuda")
    P = C.c_void_p
    wide_blob, f32_blob = net.blobs[value_net.WIDE_BF16], net.blobs["f32"]
    assert wide_blob.dtype == torch.uint8 and f32_blob.dtype == torch.float32 and wide_blob.data_ptr() != f32_blob.data_ptr()

    def call(kind=net.kind, dims=net.dims, om_cols=48, d_maps=maps.data_ptr(), blob=wide_blob.data_ptr(), n_bytes=wide_blob.numel()):
        rc = _lib.load().cs_value_net_decide_om_bf16(
            C.c_int(kind), dims.ctypes.data_as(P), C.c_int(len(dims)), P(blob), C.c_size_t(n_bytes), C.c_int(2), C.c_int(81), C.c_int(5), C.c_int(13),
            C.c_int(om_cols), P(rot.data_ptr()), P(d_maps), P(rew.data_ptr()), P(d_acts.data_ptr()), P(d_rob.data_ptr()), C.c_int(9), C.c_float(0.9),
            C.c_float(0.25), None, P(vals.data_ptr()), None, P(act.data_ptr()), P(_stream()))
        return rc, _lib.load().cs_last_error().decode()

    assert call()[0] == 0
    for kw, fragment in ((dict(kind=0, dims=np.array([2, 8, 1], np.int32)), "occupancy maps belong to SARL's network"),
                         (dict(om_cols=0), "om_cols must be at least 1"),
                         (dict(om_cols=9 * 9 * 3 + 2), "exceed a layer's 256 inputs"), (dict(d_maps=None), "null argument"),
                         (dict(blob=f32_blob.data_ptr(), n_bytes=4 * f32_blob.numel()), "the weight blob does not have the size of this network"),
                         (dict(n_bytes=wide_blob.numel() - 1), "the weight blob does not have the size of this network")):
        rc, message = call(**kw)
        assert rc == _lib.CS_ERR_ARG and fragment in message, message
    torch.cuda.synchronize()


def test_act_device_and_predict_agree_and_the_two_blobs_do_not_alias():
    """4 device-reset worlds, 5 humans, 3 steps: the bf16 actions of act_device equal the W = 1 predict of every world; the bf16 and the
    float32 blob are two tensors; a parameter change repacks the bf16 blob; switching back to "f32" reproduces, bit for bit, the float32
    decision taken on the same observation before the switch."""
    import torch

    from test_gpu_value_policy import _PeekedEnv, _batched, _ready

    import om_cases
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net
    from social_navigation_pyenvs_amd.crowd_nav.utils.state import FullState, JointState, ObservableState

    env = _batched(5, W=4)
    pol = _ready(om_policy(), env)
    om_cases.draw_weights(pol.model, 2400)
    differ = 0
    for step in range(3):
        f32_act = env.act_device(pol).cpu().numpy().copy()
        f32_values = env.last_values_device()[0].cpu().numpy().copy()
        pol.set_wide_precision("bf16")
        act = env.act_device(pol).cpu().numpy().copy()
        values, choice = (t.cpu().numpy().copy() for t in env.last_values_device())
        np.testing.assert_array_equal(choice, np.argmax(values, axis=1))
        differ += int((values != f32_values).sum())
        net = pol.device_net()
        wide_blob, f32_blob = net.blobs[value_net.WIDE_BF16], net.blobs["f32"]
        assert wide_blob.dtype == torch.uint8 and wide_blob.data_ptr() != f32_blob.data_ptr() and 4 * f32_blob.numel() != wide_blob.numel()
        robot, obs, peek = env.cw.d_robot.download(), env.observe_device().cpu().numpy(), env.cw.peek(env.robot_time_step)
        for wi in range(4):
            r = robot[wi]
            state = JointState(FullState(*[float(x) for x in (r[0], r[1], r[3], r[4], r[8], r[10], r[11], r[12], r[2])]),
                               [ObservableState(*[float(x) for x in h]) for h in obs[wi]])
            pol.set_env(_PeekedEnv(peek[wi][:, :6]))
            a = pol.predict(state)
            assert np.float32(a.vx) == act[wi, 0] and np.float32(a.vy) == act[wi, 1], (step, wi)
            np.testing.assert_array_equal(np.asarray(pol.action_values, np.float32), values[wi])
        if step == 1:                       # a parameter change repacks the bf16 blob from the new numbers, and back (a factor of 2 is exact)
            before = wide_blob.cpu().numpy().copy()
            with torch.no_grad():
                pol.model.mlp1[0].weight[:, 13:].mul_(2.0)
            changed = pol.device_net().blobs[value_net.WIDE_BF16].cpu().numpy().copy()
            assert changed.shape == before.shape and not np.array_equal(changed, before)
            with torch.no_grad():
                pol.model.mlp1[0].weight[:, 13:].mul_(0.5)
            np.testing.assert_array_equal(pol.device_net().blobs[value_net.WIDE_BF16].cpu().numpy(), before)
        pol.set_wide_precision("f32")
        np.testing.assert_array_equal(env.act_device(pol).cpu().numpy(), f32_act)
        np.testing.assert_array_equal(env.last_values_device()[0].cpu().numpy(), f32_values)
        env.step_device(env.action_buffer())
    assert differ > 0                       # the two arithmetics are two: the bf16 values are not the float32 ones
    env.close()
