"""GPU suite of OM-SARL: the occupancy maps (cs_occupancy_maps, csrc/occupancy_map.hip) against the reference's recorded maps
(golden G20) and om_cases' float64 restatement; the wide-row decision (cs_value_net_decide_om, csrc/value_net_om.hip) against
cs_value_net_decide with zero map weights, against the torch forward of the same module on the same device and against the reference's
recorded decisions; and the policy and the batched Gym on top of them.

Every comparison between two launches of this library is bitwise (np.array_equal on the int32 views) unless it says otherwise."""
import functools

import numpy as np
import pytest

import om_cases
from test_gpu_value_policy import REL_BAR, _batched, _ready, _torch_values
from test_gpu_value_worlds import GAMMA, HEADED, worlds
from test_value_om_cpu import g20, g20_policy, om_policy
from test_value_policy_cpu import make_policy
from value_calls import _stream, _up, decide_call, lookahead_call, same_bits

pytestmark = pytest.mark.gpu

F32 = np.float32
DT = 0.25
MEAN_BAR = 1e-5         # the project's per-substep contract; speeds are <= 1.5 m/s, float32 rounding two orders below
GUARD = (5, 8)
ALL_CONFIGS = om_cases.CONFIGS + (om_cases.WIDE_CONFIG,)


def maps_call(humans, vel_col, cfg):
    """cs_occupancy_maps on a host array [W, n, stride] -> [W, n, C] numpy.  The output lies between guard floats and is NaN-filled before:
    every float of it must be written, none outside it."""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    W, n, stride = humans.shape
    C_ = cfg[0] ** 2 * cfg[2]
    flat = torch.full((GUARD[0] + W * n * C_ + GUARD[1],), np.nan, device="cuda")
    flat[:GUARD[0]] = -77.0
    flat[-GUARD[1]:] = -77.0
    d_h = _up(humans)
    value_net.occupancy_maps(W, n, d_h.data_ptr(), stride, vel_col, cfg[0], cfg[1], cfg[2], flat.data_ptr() + 4 * GUARD[0], _stream())
    torch.cuda.synchronize()
    flat = flat.cpu().numpy()
    assert np.all(flat[:GUARD[0]] == F32(-77.0)) and np.all(flat[-GUARD[1]:] == F32(-77.0)), "a store outside [W, n, C]"
    return flat[GUARD[0]:-GUARD[1]].reshape(W, n, C_)


def compare_maps(got, want, cfg):
    """occupancy exactly, means within MEAN_BAR: the largest mean difference"""
    occ, vel = om_cases.occupancy_columns(cfg[0] ** 2, cfg[2])
    assert np.all(np.isfinite(got))
    assert np.array_equal(got[..., occ].astype(np.float64), np.asarray(want)[..., occ].astype(np.float64))
    if not len(vel):
        return 0.0
    err = float(np.max(np.abs(got[..., vel].astype(np.float64) - np.asarray(want)[..., vel])))
    assert err <= MEAN_BAR, err
    return err


# ---------------------------------------------------------------------------------------------------------------- the maps
def test_maps_reproduce_the_reference_on_g20():
    worst = 0.0
    for c in g20()["maps"]:
        cfg = (c["cell_num"], c["cell_size"], c["channels"])
        for n, off in zip(c["n"], c["offset"]):
            got = maps_call(c["humans"][off:off + n].astype(F32)[None], 2, cfg)[0]
            worst = max(worst, compare_maps(got, c["ref"][off:off + n], cfg))
    print(f"cs_occupancy_maps against the reference's maps on G20 (a): largest mean-velocity difference {worst:.3e}")


RANDOM_CASES = [(W, n, ALL_CONFIGS[k % 6], ((4, 2), (6, 3))[(k // 6 + k % 6) % 2])
                for k, (W, n) in enumerate((W, n) for W in (1, 3, 33) for n in (2, 5, 31, 32, 33, 70))]


@functools.lru_cache(maxsize=None)
def random_case(W, n, cfg, layout):
    stride, vel_col = layout
    seed = 20000 + 100 * n + W
    while True:         # the condition on the inputs (at most 1 % of the rows near an edge in float64) is met before any launch
        humans = om_cases.random_worlds(seed, W, n, stride, vel_col)
        try:
            want, keep = om_cases.reference_rows(humans, stride, vel_col, cfg)
            return humans, want, keep
        except AssertionError:
            seed += 7919


@pytest.mark.parametrize("W,n,cfg,layout", RANDOM_CASES)
def test_maps_against_the_float64_restatement(W, n, cfg, layout):
    humans, want, keep = random_case(W, n, cfg, layout)
    assert keep.sum() >= 0.99 * W * n
    got = maps_call(humans, layout[1], cfg)
    compare_maps(got[keep], want[keep], cfg)


def test_every_configuration_meets_both_layouts():
    seen = {(cfg, layout) for _, _, cfg, layout in RANDOM_CASES}
    assert all((cfg, layout) in seen for cfg in ALL_CONFIGS for layout in ((4, 2), (6, 3)))


@pytest.mark.parametrize("n,cfg", [(5, om_cases.CONFIGS[0]), (33, om_cases.WIDE_CONFIG), (70, om_cases.CONFIGS[2])])
def test_a_world_alone_gives_the_bits_of_the_batch(n, cfg):
    humans = om_cases.random_worlds(31 + n, 33, n, 6, 3)
    batch = maps_call(humans, 3, cfg)
    for w in (0, 1, 16, 31, 32):
        assert same_bits(maps_call(humans[w:w + 1], 3, cfg)[0], batch[w]), w


def test_one_human_writes_zeros_and_a_nan_stays_in_its_pairs():
    cfg = om_cases.CONFIGS[0]
    assert np.array_equal(maps_call(om_cases.random_worlds(1, 7, 1, 4, 2), 2, cfg), np.zeros((7, 1, 48), F32))
    humans = om_cases.random_worlds(2, 3, 6, 4, 2)
    humans[..., 0:2] = humans[..., 0:2] * F32(0.4)           # close together: most cells' neighbours inside the grid
    clean = maps_call(np.delete(humans, 2, axis=1), 2, cfg)
    assert np.count_nonzero(clean) > 20
    humans[:, 2, 0] = np.nan
    got = maps_call(humans, 2, cfg)
    assert np.all(np.isfinite(got)) and np.array_equal(got[:, 2], np.zeros((3, 48), F32))
    assert same_bits(np.ascontiguousarray(np.delete(got, 2, axis=1)), clean)      # the others' rows: the world without that human


# ---------------------------------------------------------------------------------------------------------------- the decision
@pytest.fixture(scope="module")
def twins():
    """(with_global, headed) -> (SARL DeviceNet, its OM twin's DeviceNet): the same weights, zeros on the map columns of mlp1's first layer"""
    made = {}

    def get(with_global, headed):
        import torch

        if (with_global, headed) not in made:
            kw = dict(sarl__with_global_state=str(with_global).lower(), **(HEADED if headed else {}))
            sarl = _ready(make_policy("sarl", **kw))
            om_cases.draw_weights(sarl.model, 3100 + 2 * int(with_global) + int(headed))
            twin = _ready(om_policy(15 if headed else 13, **{k: v for k, v in kw.items() if k != "sarl__with_theta_and_omega_visible"}))
            cols = sarl.joint_state_dim
            with torch.no_grad():
                sd, td = sarl.model.state_dict(), twin.model.state_dict()
                for k in td:
                    if k == "mlp1.0.weight":
                        td[k].zero_()
                        td[k][:, :cols].copy_(sd[k])
                    else:
                        td[k].copy_(sd[k])
            made[with_global, headed] = (sarl.device_net(), twin.device_net())
        return made[with_global, headed]

    return get


@pytest.mark.parametrize("n", [2, 5, 16, 17, 31, 32, 33, 70])
def test_zero_map_weights_give_the_values_of_sarl(twins, n):
    """The extra k-groups add exact zeros to the same fmaf chain: values, choice and action are numerically those of cs_value_net_decide."""
    import torch

    for i, (W, A) in enumerate(((1, 1), (1, 31), (1, 32), (1, 33), (3, 81))):
        with_global, headed = bool((i + n) % 2), bool((i // 2 + n // 2) % 2)
        sarl, twin = twins(with_global, headed)
        acts, nxt, cur, rob = worlds(W, n, A, headed, seed=4000 + 10 * n + i)
        rot, rew = lookahead_call(acts, nxt, cur, rob)
        maps = torch.randn((W, n, twin.om_cols), device="cuda", generator=torch.Generator("cuda").manual_seed(n + i))
        want = decide_call(sarl, rot, rew, acts, rob)
        got = decide_call(twin, rot, rew, acts, rob, maps)
        assert np.all(np.isfinite(want[0]))
        for g, w_ in zip(got, want):
            assert np.array_equal(g, w_), (n, W, A, with_global, headed)


TORCH_CASES = [(13, (1, 2.0, 1), {}), (13, (1, 2.0, 3), {}), (15, (1, 2.0, 1), {}), (13, (4, 1.0, 3), {}), (15, (4, 1.0, 3), {}),
               (15, (8, 0.5, 3), {}), (13, (8, 0.5, 3), dict(sarl__with_global_state="false")),
               (15, (4, 1.0, 3), dict(sarl__mlp1_dims="40, 72", sarl__mlp2_dims="33", sarl__attention_dims="20, 1", sarl__mlp3_dims="90, 1")),
               (13, (3, 0.7, 2), dict(sarl__mlp1_dims="40, 72", sarl__mlp2_dims="33", sarl__attention_dims="20, 1", sarl__mlp3_dims="90, 1",
                                      sarl__with_global_state="false"))]


@pytest.mark.parametrize("cols,cfg,overrides", TORCH_CASES)
def test_values_against_the_torch_forward(cols, cfg, overrides):
    """rewards + gamma^(dt v_pref) * model(cat(rows, maps)), float32 torch on the same device, within 1e-4 relative to max(1, max |V|)."""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    pol = _ready(om_policy(cols, cfg, **overrides))
    om_cases.draw_weights(pol.model, 3300 + cols + cfg[0])
    net = pol.device_net()
    worst = 0.0
    for W, n in ((3, 5), (2, 33)):
        acts, nxt, cur, rob = worlds(W, n, 81, cols == 15, seed=5000 + n)
        nxt[..., 0:2] = rob[:, None, 0:2] + (nxt[..., 0:2] - rob[:, None, 0:2]) * F32(0.5)       # closer together: filled maps
        cur[..., 0:2] = rob[:, None, 0:2] + (cur[..., 0:2] - rob[:, None, 0:2]) * F32(0.5)
        rot, rew = lookahead_call(acts, nxt, cur, rob)
        maps = value_net.maps_of(_up(nxt), 3 if cols == 15 else 2, cfg, _stream())
        assert float(maps.abs().sum()) > 0
        got = decide_call(net, rot, rew, acts, rob, maps)[0].astype(np.float64)
        wide = torch.cat([rot, maps[:, None].expand(W, 81, n, maps.shape[-1])], dim=-1).contiguous()
        want = _torch_values(pol, wide, rew, _up(rob[:, 7]), GAMMA, DT).cpu().numpy().astype(np.float64)
        assert np.all(np.isfinite(want)) and np.all(np.isfinite(got))
        worst = max(worst, float(np.max(np.abs(got - want))) / max(1.0, float(np.max(np.abs(want)))))
    print(f"cs_value_net_decide_om against torch, K = {cols + cfg[0] ** 2 * cfg[2]}: worst relative difference {worst:.3e}")
    assert worst < REL_BAR


@pytest.fixture(scope="module")
def default_net():
    pol = _ready(om_policy())
    om_cases.draw_weights(pol.model, 3400)
    return pol, pol.device_net()


def test_one_map_row_serves_all_actions_of_its_world(default_net):
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    _, net = default_net
    acts, nxt, cur, rob = worlds(3, 5, 81, False, seed=6000)
    rot, rew = lookahead_call(acts, nxt, cur, rob)
    maps = value_net.maps_of(_up(nxt), 2, net.om_grid, _stream())
    base = decide_call(net, rot, rew, acts, rob, maps)[0]
    moved = maps.clone()
    moved[1] += 0.5
    got = decide_call(net, rot, rew, acts, rob, moved)[0]
    assert same_bits(got[0], base[0]) and same_bits(got[2], base[2])
    assert np.all(got[1] != base[1])


@pytest.mark.parametrize("W,n", [(50, 5), (3, 33)])
def test_a_decision_alone_gives_the_bits_of_the_batch(default_net, W, n):
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    _, net = default_net
    acts, nxt, cur, rob = worlds(W, n, 81, False, seed=6100 + n)
    rot, rew = lookahead_call(acts, nxt, cur, rob)
    maps = value_net.maps_of(_up(nxt), 2, net.om_grid, _stream())
    batch = decide_call(net, rot, rew, acts, rob, maps)
    for w in range(W):
        alone = decide_call(net, rot[w:w + 1].contiguous(), rew[w:w + 1].contiguous(), acts, rob[w:w + 1], maps[w:w + 1].contiguous())
        assert same_bits(alone[0][0], batch[0][w]) and alone[1][0] == batch[1][w] and same_bits(alone[2][0], batch[2][w]), w


def test_the_reference_decisions_of_g20():
    """G20 (c), the 32 decisions as one batch: with zero rewards and gamma = 1 the values are the network outputs (1e-4 relative to
    max(1, max |V|) of the decision); with cs_lookahead's rewards the pick is the reference's, or a tie of the reference's own values."""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    pol = _ready(g20_policy("om_sarl_decide"))
    net = pol.device_net()
    cs = g20()["decision"]
    acts = cs[0]["action_space"].astype(F32)
    assert all(np.array_equal(c["action_space"], cs[0]["action_space"]) for c in cs)
    nxt, cur, rob = (np.stack([c[k] for c in cs]).astype(F32) for k in ("next_humans", "obs", "robot"))
    rot, rew = lookahead_call(acts, nxt, cur, rob, float(cs[0]["dt"]))
    maps = value_net.maps_of(_up(nxt), 2, net.om_grid, _stream())
    worst_map = compare_maps(maps.cpu().numpy(), np.stack([c["maps"] for c in cs]), net.om_grid)
    net_out = decide_call(net, rot, torch.zeros_like(rew), acts, rob, maps, gamma=1.0)[0].astype(np.float64)
    _, pick, _ = decide_call(net, rot, rew, acts, rob, maps, gamma=float(cs[0]["gamma"]), dt=float(cs[0]["dt"]))
    worst = 0.0
    for w, c in enumerate(cs):
        worst = max(worst, float(np.max(np.abs(net_out[w] - c["net_outputs"]))) / max(1.0, float(np.max(np.abs(c["net_outputs"])))))
        ref = np.asarray(c["action_values"])
        if int(pick[w]) != int(c["chosen"]):
            assert abs(ref[int(pick[w])] - ref[int(c["chosen"])]) <= 1e-4 * max(1.0, float(np.max(np.abs(ref)))), (c["test_case"], c["step"])
    print(f"G20 (c): {len(cs)} decisions, network outputs worst relative {worst:.3e}, maps worst mean difference {worst_map:.3e}")
    assert worst < REL_BAR


def test_refusals_with_real_buffers(default_net):
    import ctypes as C

    import torch

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    _, net = default_net
    acts, nxt, cur, rob = worlds(2, 5, 81, False, seed=6200)
    rot, rew = lookahead_call(acts, nxt, cur, rob)
    maps = value_net.maps_of(_up(nxt), 2, net.om_grid, _stream())
    d_acts, d_rob = _up(acts), _up(rob)
    vals, act = torch.zeros((2, 81), device="cuda"), torch.zeros((2, 2), device="cuda")
    P = C.c_void_p

    def call(kind=net.kind, dims=net.dims, om_cols=48, d_maps=maps.data_ptr()):
        rc = _lib.load().cs_value_net_decide_om(
            C.c_int(kind), dims.ctypes.data_as(P), C.c_int(len(dims)), P(net.blob.data_ptr()), C.c_size_t(net.blob.numel()), C.c_int(2), C.c_int(81),
            C.c_int(5), C.c_int(13), C.c_int(om_cols), P(rot.data_ptr()), P(d_maps), P(rew.data_ptr()), P(d_acts.data_ptr()), P(d_rob.data_ptr()),
            C.c_int(9), C.c_float(0.9), C.c_float(0.25), None, P(vals.data_ptr()), None, P(act.data_ptr()), P(_stream()))
        return rc, _lib.load().cs_last_error().decode()

    assert call()[0] == 0
    for kw, fragment in ((dict(kind=0, dims=np.array([2, 8, 1], np.int32)), "occupancy maps belong to SARL's network"),
                         (dict(om_cols=9 * 9 * 3 + 2), "exceed a layer's 256 inputs"), (dict(d_maps=None), "null argument")):
        rc, message = call(**kw)
        assert rc == _lib.CS_ERR_ARG and fragment in message, message
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the public interface
def _joint_state(robot, humans, headed):
    from social_navigation_pyenvs_amd.crowd_nav.utils.state import FullState, JointState, ObservableState, ObservableStateHeaded

    return JointState(FullState(*[float(x) for x in robot]), [(ObservableStateHeaded if headed else ObservableState)(*[float(x) for x in h]) for h in humans])


def test_build_occupancy_maps_is_the_w1_launch_on_g20():
    from social_navigation_pyenvs_amd.crowd_nav.utils.state import ObservableState

    for c in g20()["maps"]:
        cfg = (c["cell_num"], c["cell_size"], c["channels"])
        pol = _ready(om_policy(13, cfg))
        for n, off in list(zip(c["n"], c["offset"]))[::3]:
            h = c["humans"][off:off + n]
            got = pol.build_occupancy_maps([ObservableState(*row, 0.3) for row in h.tolist()])
            assert got.dtype.is_floating_point and got.device.type == "cpu" and tuple(got.shape) == (n, cfg[0] ** 2 * cfg[2])
            assert same_bits(got.numpy(), maps_call(h.astype(F32)[None], 2, cfg)[0])


@pytest.mark.parametrize("cols", [13, 15])
def test_transform_predict_and_state_value_on_g20_states(cols):
    """``transform`` against the reference's recorded rows and as cat(rotate, W = 1 maps); ``predict`` as the W = 1 launches of the batch
    entries on the same arrays, bitwise; ``state_value`` against the torch forward on ``transform``'s rows."""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net
    from social_navigation_pyenvs_amd.crowd_nav.policy.cadrl import propagate_humans_state_with_constant_velocity_model as propagate
    from test_value_state_cpu import ROW_SLACK, g19_reference_row_error

    headed = cols == 15
    pol = _ready(g20_policy(f"om_sarl_{cols}"))
    pol.query_env, pol.time_step = False, DT
    c = next(c for c in g20()["transform"] if int(c["cols"]) == cols)
    net = pol.device_net()
    for i, (n, off) in enumerate(zip(c["n"], c["offset"])):
        robot, humans = c["robot"][i], c["humans"][off:off + n]
        state = _joint_state(robot, humans, headed)
        rows = pol.transform(state)
        assert rows.dtype == torch.float32 and tuple(rows.shape) == (n, cols + 48)
        got = rows.cpu().numpy()
        assert float(np.max(np.abs(got[:, :cols].astype(np.float64) - c["rows"][off:off + n, :cols]))) <= 2 * g19_reference_row_error() + ROW_SLACK
        compare_maps(got[:, cols:], c["rows"][off:off + n, cols:], (4, 1.0, 3))
        assert same_bits(np.ascontiguousarray(got[:, cols:]), maps_call(humans[:, :4].astype(F32)[None], 2, (4, 1.0, 3))[0])
        # predict: the W = 1 launch of lookahead -> maps of the next humans -> decide_om
        np.random.seed(3)
        action = pol.predict(state)
        cur = humans.astype(F32)[None]
        nxt = np.asarray(propagate(humans, DT, headed), F32)[None]
        rob = robot.astype(F32)[None]
        acts = np.asarray(pol.action_space_ndarray, F32)
        rot, rew = lookahead_call(acts, nxt, cur, rob)
        maps = value_net.maps_of(_up(nxt), 3 if headed else 2, net.om_grid, _stream())
        vals, pick, _ = decide_call(net, rot, rew, acts, rob, maps, gamma=pol.gamma, dt=DT)
        assert same_bits(np.asarray(pol.action_values, F32), vals[0])
        assert (action.vx, action.vy) == tuple(pol.action_space_ndarray[int(pick[0])])
        weights = pol.get_attention_weights()
        assert weights.shape == (n,) and abs(float(weights.sum()) - 1.0) < 1e-5
        # state_value: the network on transform's rows
        with torch.no_grad():
            want = float(pol.model(rows[None]).item())
        assert abs(pol.state_value(state) - want) <= REL_BAR * max(1.0, abs(want))
        assert abs(want - float(c["out"][i])) <= REL_BAR * max(1.0, float(np.max(np.abs(c["out"]))))


def test_the_batched_gym_decides_and_evaluates_with_om_sarl(default_net):
    """W = 33 worlds x 5 humans: act_device is lookahead_device -> occupancy_maps_device("next") -> cs_value_net_decide_om, bitwise;
    joint_state_device is SARL's rows beside the maps of the current humans, bitwise; value_device is the torch forward on those rows
    (1e-4) and bootstraps as the 13-column policies do; act_step_device keeps refusing."""
    import torch

    pol, net = default_net
    env = _batched(5, W=33)
    _ready(pol, env)
    act = env.act_device(pol).clone()
    values, choice = (t.clone() for t in env.last_values_device())
    torch.cuda.synchronize()
    rot, rew = env.lookahead_device(pol.action_space_ndarray)
    maps = env.occupancy_maps_device(4, 1.0, 3, which="next")
    torch.cuda.synchronize()
    assert tuple(maps.shape) == (33, 5, 48) and same_bits(net.last_maps.cpu().numpy(), maps.cpu().numpy())
    _, _, rob = env._worlds_on_side_stream(env._device_loop_state(), peek=False)
    torch.cuda.synchronize()
    acts = np.asarray(pol.action_space_ndarray, F32)
    want = decide_call(net, rot.contiguous(), rew.contiguous(), acts, rob.cpu().numpy(), maps.contiguous(), gamma=pol.gamma, dt=env.robot_time_step)
    assert same_bits(values.cpu().numpy(), want[0]) and np.array_equal(choice.cpu().numpy(), want[1]) and same_bits(act.cpu().numpy(), want[2])
    assert np.all(np.isfinite(want[0]))

    sarl = _ready(make_policy("sarl"), env)
    rows = env.joint_state_device(pol)
    current = env.occupancy_maps_device(4, 1.0, 3)
    narrow = env.joint_state_device(sarl)
    torch.cuda.synchronize()
    assert tuple(rows.shape) == (33, 5, 61)
    assert same_bits(rows.cpu().numpy(), torch.cat([narrow, current], dim=2).cpu().numpy())
    v, rows2 = env.value_device(pol, with_state=True)
    torch.cuda.synchronize()
    assert same_bits(rows2.cpu().numpy(), rows.cpu().numpy())
    with torch.no_grad():
        ref = pol.model(rows)[:, 0].cpu().numpy().astype(np.float64)
    assert float(np.max(np.abs(v.cpu().numpy() - ref))) <= REL_BAR * max(1.0, float(np.max(np.abs(ref))))
    r = torch.linspace(-0.25, 1.0, 33, device="cuda")
    target = env.value_device(pol, rewards=r, bootstrap=True)
    disc = pol.gamma ** (env.robot_time_step * rob[:, 7].double())
    torch.cuda.synchronize()
    assert float((target.double() - (r.double() + disc * v.double())).abs().max()) <= 1e-5 * max(1.0, float(v.abs().max()))
    with pytest.raises(TypeError, match="no-train policy"):
        env.act_step_device(pol)
