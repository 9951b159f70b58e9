"""What the suites of the loss-and-gradient kernels on rows with occupancy-map columns share (tests/test_value_om_grad_cpu.py,
tests/test_gpu_value_om_grad.py; cs_value_net_loss_grad_om, cs_value_net_loss_grad_lstm_om and their pack, train-step and blob-index
siblings, ``Trainer.set_gradient("device_om")`` / ``("device_lstm_om")``): golden G25 (the reference's networks with
``input_dim = cols + om_cols`` under autograd and its Trainer, tests/golden/make_golden_g25.py), this project's modules with G25's widths
and weights, seeded modules at other column counts, seeded minibatches whose map columns are sparse, and the kernel call with its
comparison against autograd.

A network is named by (policy, which, cols, om_cols): policy "sarl" with which = with_global (0 | 1), or "lstm" with which = the network
(1 | 2).  A row is the cols rotated columns of a human, then its om_cols map columns, as ``transform`` stores a state.

The yardstick is tests/value_grad_cases.py's, unchanged: per tensor e_candidate <= 16 * max(e_torch, 2^-22) against float64 CPU autograd,
with its zero-gradient fallback; tests/lstm_grad_cases.py's ``check_loss`` is the same measure for the loss."""
import copy
import functools

import numpy as np

import lstm_grad_cases as lg
import value_grad_cases as vg
from value_grad_cases import F32, load_cases

G25_NETS = ["om_sarl_13_48_1", "om_sarl_15_18_1", "om_sarl_13_18_0", "om_lstm1_13_48", "om_lstm1_15_18", "om_lstm2_13_18", "om_lstm2_15_48"]
# the first layer's K = cols + om_cols: 14 | 16 (16: a whole k-group, no padding), 31 | 33 (either side of a 32-column block of bwd_dw),
# 61 | 63 (the reference's default), 205 | 207 (seven blocks, the widest stride of the test widths, their largest LDS block)
WIDTHS = [(13, 18), (15, 18), (13, 48), (15, 48)]
EDGE_WIDTHS = [(13, 1), (15, 1), (13, 192), (15, 192)]
SARL_SHAPES = [(1, 2), (7, 5), (33, 3), (100, 5), (2, 33)]
MIN_RMS = 0.25             # the least root-mean-square distance of a minibatch's targets from its values (``batch``)
WORST = {"ratio": 0.0}      # the largest e_candidate / max(e_torch, 2^-22) a run of the suite has seen (of 16)


@functools.lru_cache(maxsize=None)
def g25():
    """golden G25: {net name: case}"""
    return {c["net"]: c for c in load_cases("g25_om_trainer")}


def module(policy, which, cols, om_cols, full=False):
    """This project's module of the network (policy, which) on rows of cols + om_cols columns; `full`: at the reference's widths"""
    if policy == "sarl":
        return vg.sarl_module(cols + om_cols, bool(which), vg.SARL_FULL if full else None)
    if full:
        return lg.lstm_module(which, cols + om_cols, lg.H_FULL, lg.MLP1_FULL, lg.MLP_FULL)
    return lg.lstm_module(which, cols + om_cols)


def key_of(net):
    """(policy, which, cols, om_cols) of a G25 network"""
    case = g25()[net]
    policy = str(case["policy"])
    return policy, int(case["with_global"]) if policy == "sarl" else int(case["network"]), int(case["cols"]), int(case["om_cols"])


def g25_module(net):
    """This project's module with the weights of G25's network `net`, checked against the recorded digest"""
    case = g25()[net]
    model = module(*key_of(net))
    sd = model.state_dict()
    assert sorted(sd) == list(case["weights_keys"]) and [list(sd[k].shape) for k in sorted(sd)] == case["weights_shapes"]
    assert vg.draw_weights(model, case["seed"], bool(case["calm"])) == case["sha256"], "the seeded weights are not the ones the fixture was recorded with"
    return model


def g25_batches(net):
    import torch

    case = g25()[net]
    return [(torch.from_numpy(case[f"inputs{b}"]), torch.from_numpy(case[f"values{b}"])) for b in range(3)]


@functools.lru_cache(maxsize=None)
def seeded(policy, which, cols, om_cols, full=False):
    model = module(policy, which, cols, om_cols, full)
    vg.draw_weights(model, 2540 + 1000 * (policy == "lstm") + 100 * which + cols + 7 * om_cols + int(full), calm=policy == "sarl")
    return model


def rows(rs, shape, cols, om_cols):
    """[.., cols + om_cols] float32: uniform rotated columns, then map columns that are 0 with probability 3 / 4, else uniform"""
    rot = rs.uniform(-1, 1, shape + (cols,))
    maps = rs.uniform(-1, 1, shape + (om_cols,)) * (rs.uniform(0, 1, shape + (om_cols,)) < 0.25)
    return np.concatenate([rot, maps], axis=-1).astype(F32)


def batch(model, cols, om_cols, B, n, salt=0):
    """A seeded minibatch (inputs [B, n, cols + om_cols], values [B, 1]) with every sample redrawn until no ReLU of the float64 module
    reads an input within vg.KINK_MARGIN of zero (value_grad_cases.batch_away_from_kinks says why), and the targets redrawn until their
    root-mean-square distance from the float64 module's values is at least MIN_RMS.

    MIN_RMS is tests/lstm_grad_cases.py ``case``'s reasoning for B = 1, for any B: the loss is mean (V - target)^2, so a forward error dV
    is 2 dV / rms(V - target) of it, whatever the kernel sums; the forward is the decision kernel's by contract, within a few 1e-7 absolute
    of torch's (its sigmoid and tanh are within 3e-7 each), and the yardstick grants the loss 16 * 2^-22 = 3.8e-6.  At a distance of 0.25
    that error is 2.4e-6 of the loss; two targets drawn 0.03 from their values would measure the draw.  Uniform targets of a large minibatch
    lie 0.6 away and are never redrawn."""
    import torch

    rs = np.random.RandomState(2500 + 1000 * B + n + 7919 * salt + 31 * om_cols + cols)
    x = torch.from_numpy(rows(rs, (B, n), cols, om_cols))
    v = torch.from_numpy(rs.uniform(-1, 1, (B, 1)).astype(F32))
    for _ in range(50):
        near = vg.relu_margins(model, x) < vg.KINK_MARGIN
        if not near.any():
            break
        x[torch.from_numpy(near)] = torch.from_numpy(rows(rs, (int(near.sum()), n), cols, om_cols))
    else:
        raise AssertionError("no minibatch away from the ReLUs' kinks in 50 draws")
    with torch.no_grad():
        out = copy.deepcopy(model).double()(x.double())
    for _ in range(50):
        if float(((out - v.double()) ** 2).mean().sqrt()) >= MIN_RMS:
            return x, v
        v = torch.from_numpy(rs.uniform(-1, 1, (B, 1)).astype(F32))
    raise AssertionError("no targets away from the values in 50 draws")


@functools.lru_cache(maxsize=None)
def case(policy, which, cols, om_cols, B, n, full=False):
    """(model, x, v, references) of one case, computed once and shared.  B = 1: the target lies one unit below the float64 module's value,
    for the reason tests/lstm_grad_cases.py ``case`` gives (one sample's gradient is 2 (V - target) times a direction: a drawn target next
    to V measures the draw)."""
    import torch

    model = seeded(policy, which, cols, om_cols, full)
    x, v = batch(model, cols, om_cols, B, n)
    if B == 1:
        with torch.no_grad():
            v = (copy.deepcopy(model).double()(x.double()) - 1.0).float()
    return model, x, v, vg.references(model, x, v)


# ---------------------------------------------------------------------------------------------------------------- the kernel's call
def device_net(model, cols, om_cols):
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    return value_net.DeviceNet(model, cols, om_cols=om_cols, map_order="own")


def host_pack(net, flat):
    """cs_value_net_pack_om / cs_value_net_pack_lstm_om of the flat parameters `flat` (numpy), on the host"""
    import value_step_cases as vs

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    return value_net.pack(net.kind, net.dims, net.cols, vs.split_flat(net, flat), "f32", net.om_cols)


def by_sorted_name(net, model, host):
    """A flat array in value_net.param_offsets' layout cut into float64 arrays per parameter, in the sorted order of the names"""
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    offsets = value_net.param_offsets(net)
    described = [p for layer in net.layers for p in value_net.layer_params(layer)]
    by_id = {id(p): host[a:b].reshape(tuple(p.shape)).astype(np.float64) for p, a, b in zip(described, offsets, offsets[1:])}
    return [by_id[id(p)] for p in vg.sorted_parameters(model)]


def kernel_gradient(model, cols, om_cols, x, v, values=False, poison=np.nan):
    """pack_om_on_device + loss_and_grad_om for `model` on one minibatch: (loss, [gradient per parameter in sorted-name order], the flat
    gradient's bytes, values [B] or None).  The gradient buffer is filled with `poison` before."""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    net = device_net(model, cols, om_cols)
    flat = vg.flat_parameters(net, model)
    grad = torch.full_like(flat, poison)
    vals = torch.full((x.shape[0],), np.nan, device="cuda") if values else None
    value_net.pack_om_on_device(net, flat)
    loss = value_net.loss_and_grad_om(net, flat, vg.to_device(x), vg.to_device(v).reshape(-1), grad, vals)
    torch.cuda.synchronize()
    host = grad.cpu().numpy()
    return float(loss.item()), by_sorted_name(net, model, host), host.tobytes(), None if vals is None else vals.cpu().numpy()


def within_yardstick(candidate, torch32, ref64, what):
    """vg.assert_within_yardstick, with the largest ratio e_candidate / max(e_torch, 2^-22) (of 16) printed and kept in WORST"""
    ratio = max(ec / max(et, vg.FLOOR) for ec, et in vg.errors(candidate, torch32, ref64))
    WORST["ratio"] = max(WORST["ratio"], ratio)
    print(f"{what}: yardstick ratio {ratio:.3f} of {vg.FACTOR:g} (worst so far {WORST['ratio']:.3f})")
    return vg.assert_within_yardstick(candidate, torch32, ref64, what)


def check_against_autograd(model, cols, om_cols, x, v, what, refs=None):
    """The kernel's gradient per tensor and its loss against float64 autograd under the yardstick; returns the gradients by sorted name"""
    loss_k, g_k, _, _ = kernel_gradient(model, cols, om_cols, x, v)
    (loss32, g32), (loss64, g64) = refs or vg.references(model, x, v)
    assert np.isfinite(loss_k) and all(np.all(np.isfinite(g)) for g in g_k)
    within_yardstick(g_k, g32, g64, what)
    lg.check_loss(loss_k, loss32, loss64, what)
    return dict(zip(sorted(dict(model.named_parameters())), g_k))


def first_weight(model):
    """The name of the parameter whose columns cols .. are the map columns: mlp1's first weight, or network 1's weight_ih"""
    names = dict(model.named_parameters())
    return "mlp1.0.weight" if "mlp1.0.weight" in names else "lstm.weight_ih_l0"
