"""GPU test of the one state-value function of the value-network families (value_net.state_values_for_worlds), at the seam: for the four
default policies -- CADRL, SARL, OM-SARL (4 x 4 cells, 3 channels), LSTM-RL network 1 -- on 13 columns, the batch against every world alone,
the rows against ``rotated_rows`` (beside the maps), and the values against the launches written out by hand: cs_value_net_state for the
feed-forward networks; rotated_rows -> [maps_of(cur, 2)] -> decide_om / decide_lstm(sorted_by_distance = 0) with A = 1 for the others.

n = 2 is the fewest humans an occupancy map takes, n = 33 one human over the 32-row tile.  Every comparison is bitwise (32-bit words)."""
import numpy as np
import pytest

import lstm_cases as lc
import om_cases
from test_gpu_value_policy import _calm, _ready
from test_gpu_value_worlds import worlds
from test_value_om_cpu import om_policy
from test_value_policy_cpu import make_policy, seeded_weights
from value_calls import DT, F32, GAMMA, _stream, _up, decide_call, same_bits, state_call

pytestmark = pytest.mark.gpu

W = 3


@pytest.fixture(scope="module")
def nets():
    """policy name -> (policy, its float32 DeviceNet), built once"""
    made = {}

    def get(name):
        if name not in made:
            if name == "om_sarl":
                pol = _ready(om_policy())
                om_cases.draw_weights(pol.model, 3500)
            elif name == "lstm_rl":
                pol = _ready(lc.lstm_policy(1))
                lc.draw_weights(pol.model, 3501, calm_last=True)
            else:
                pol = _ready(make_policy(name))
                seeded_weights(pol.model, 3502 + len(name))
                if name == "sarl":
                    _calm(pol)
            made[name] = (pol, pol.state_net())
        return made[name]

    return get


def call(net, cur, rob, rewards=None, dt=0.0, want_rows=True):
    """state_values_for_worlds on host arrays: (values [W], rows or None) numpy"""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    values, rows = value_net.state_values_for_worlds(net, _up(cur), _up(rob), None if rewards is None else _up(rewards), GAMMA, dt, want_rows, _stream())
    torch.cuda.synchronize()
    return values.cpu().numpy(), None if rows is None else rows.cpu().numpy()


def by_hand(net, cur, rob, rewards, dt):
    """The launches of a family written out: (values [W], rows [W, n, 13 (+ 48)]) numpy"""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    if net.family is value_net.FEED_FORWARD:
        return state_call(net, cur, rob, rewards=rewards, dt=dt)
    d_cur, d_rob = _up(cur), _up(rob)
    maps = value_net.maps_of(d_cur, 2, net.om_grid, _stream()) if net.family is value_net.MAPPED else None
    rows = value_net.rotated_rows(d_cur, d_rob, _stream())
    torch.cuda.synchronize()
    rew = np.zeros(len(cur), F32) if rewards is None else rewards
    values = decide_call(net, rows[:, None].contiguous(), rew.reshape(-1, 1), np.zeros((1, 2), F32), rob, maps if maps is not None else 0, gamma=GAMMA, dt=dt)[0]
    return values[:, 0], (rows if maps is None else torch.cat([rows, maps], dim=2)).cpu().numpy()


@pytest.mark.parametrize("n", [2, 33])
@pytest.mark.parametrize("name", ["cadrl", "sarl", "om_sarl", "lstm_rl"])
def test_state_values_for_worlds_is_the_familys_launches(nets, name, n):
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    pol, net = nets(name)
    assert net.cols == 13 and (net.om_cols, net.om_grid) == ((48, (4, 1.0, 3)) if name == "om_sarl" else (0, None))
    assert net.family is {"om_sarl": value_net.MAPPED, "lstm_rl": value_net.RECURRENT}.get(name, value_net.FEED_FORWARD) is type(pol).family
    _, _, cur, rob = worlds(W, n, 1, False, seed=21000 + n)
    rewards = np.linspace(-0.25, 1.0, W).astype(F32)

    values, rows = call(net, cur, rob)
    assert values.shape == (W,) and values.dtype == F32 and np.all(np.isfinite(values)) and len(set(values.tolist())) == W
    want_values, want_rows = by_hand(net, cur, rob, None, 0.0)
    assert same_bits(values, want_values), (name, n, values, want_values)
    assert rows.shape == (W, n, 13 + net.om_cols) and same_bits(rows, want_rows), (name, n)
    if name == "om_sarl":
        assert np.any(rows[..., 13:] != 0)

    for w in range(W):          # a world alone: the same words
        alone_v, alone_r = call(net, cur[w:w + 1], rob[w:w + 1])
        assert same_bits(alone_v, values[w:w + 1]) and same_bits(alone_r, rows[w:w + 1]), (name, n, w)

    # without the rows: the same values; a feed-forward network then makes none
    lean_v, lean_r = call(net, cur, rob, want_rows=False)
    assert same_bits(lean_v, values) and (lean_r is None or not net.family.state_launch), (name, n)

    # the trainer's target: rewards + gamma^(dt * v_pref) * V
    target, _ = call(net, cur, rob, rewards=rewards, dt=DT)
    assert same_bits(target, by_hand(net, cur, rob, rewards, DT)[0]), (name, n)
    assert np.all(np.isfinite(target)) and not np.any(target == values)
