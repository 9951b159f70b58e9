"""What the LSTM-RL tests share (test_value_lstm_cpu.py, test_gpu_value_lstm.py, golden/make_golden_g21.py): a float64 numpy restatement of
both networks written from the published architecture (an LSTM cell in torch's gate order i, f, g, o over the rows, an MLP on (the first
row's first six columns, h_n); network 2 with a pairwise MLP in front), the decision's order rule, cs_value_net_pack_lstm's blob layout
worked out independently from include/crowdstep.h's comment, the policy configuration and golden G21's weights rebuilt from their seed."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

F32 = np.float32
SELF_DIM = 6
LSTM_SECTION = {"global_state_dim": "50", "mlp1_dims": "150, 100, 100, 50", "mlp2_dims": "150, 100, 100, 1", "multiagent_training": "true",
                "with_om": "false", "with_interaction_module": "false", "with_theta_and_omega_visible": "false"}      # the reference's policy.config


def lstm_config(**overrides):
    """test_value_policy_cpu.policy_config with the reference's [lstm_rl] section; `section__key=value` overrides."""
    from test_value_policy_cpu import policy_config

    cfg = policy_config()
    if not cfg.has_section("lstm_rl"):
        cfg.add_section("lstm_rl")
    for k, v in LSTM_SECTION.items():
        cfg.set("lstm_rl", k, v)
    for k, v in overrides.items():
        sec, key = k.split("__", 1)
        cfg.set(sec, key, str(v))
    return cfg


def lstm_policy(network=1, cols=13, **overrides):
    from social_navigation_pyenvs_amd.crowd_nav.policy.policy_factory import policy_factory

    kw = dict(lstm_rl__with_interaction_module="true" if network == 2 else "false")
    if cols == 15:
        kw["sarl__with_theta_and_omega_visible"] = "true"
    kw.update(overrides)
    pol = policy_factory["lstm_rl_device"]()
    pol.configure(lstm_config(**kw))
    return pol


# ---------------------------------------------------------------------------------------------------------------- the order
def decision_order(da):
    """The decision's order of the rows of [..., n] distances: decreasing distance, ties by decreasing human index."""
    return np.flip(np.argsort(np.asarray(da), axis=-1, kind="stable"), axis=-1)


def sort_rows(rot):
    """rotated [..., n, cols] in the decision's order (by column 11)"""
    idx = decision_order(rot[..., 11])
    return np.take_along_axis(rot, idx[..., None], axis=-2)


# ---------------------------------------------------------------------------------------------------------------- float64 restatement
def weights64(model):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in model.state_dict().items()}


def _mlp64(w, name, x, last_relu=False):
    idx = sorted({int(k.split(".")[1]) for k in w if k.startswith(name + ".")})
    for i in idx:
        x = x @ w[f"{name}.{i}.weight"].T + w[f"{name}.{i}.bias"]
        if i != idx[-1] or last_relu:
            x = np.maximum(x, 0.0)
    return x


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def forward64(w, rows):
    """The network on rows [..., n, cols] in the order given (float64) -> [...] values.  `w`: weights64 of either network."""
    rows = np.asarray(rows, np.float64)
    lead, n = rows.shape[:-2], rows.shape[-2]
    x = rows.reshape((-1,) + rows.shape[-2:])
    seq = _mlp64(w, "mlp1", x) if any(k.startswith("mlp1.") for k in w) else x
    wih, whh, b = w["lstm.weight_ih_l0"], w["lstm.weight_hh_l0"], w["lstm.bias_ih_l0"] + w["lstm.bias_hh_l0"]
    H = whh.shape[1]
    h = np.zeros((x.shape[0], H))
    c = np.zeros((x.shape[0], H))
    for t in range(n):
        g = seq[:, t] @ wih.T + h @ whh.T + b
        i, f, gg, o = _sigmoid(g[:, :H]), _sigmoid(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sigmoid(g[:, 3 * H:])
        c = f * c + i * gg
        h = o * np.tanh(c)
    return _mlp64(w, "mlp", np.concatenate([x[:, 0, :SELF_DIM], h], axis=1))[:, 0].reshape(lead)


def torch_values(model, rows):
    """torch's CPU float32 module on rows [..., n, cols] in the order given -> [...] float64"""
    import torch

    rows = np.asarray(rows, F32)
    with torch.no_grad():
        out = model(torch.from_numpy(np.ascontiguousarray(rows.reshape((-1,) + rows.shape[-2:]))))
    return out[:, 0].numpy().astype(np.float64).reshape(rows.shape[:-2])


# ---------------------------------------------------------------------------------------------------------------- the blob layout
def model_dims(model):
    lin = lambda seq: [int(m.out_features) for m in seq if hasattr(m, "out_features")]
    first = lin(model.mlp1) if hasattr(model, "mlp1") else []
    last = lin(model.mlp)
    return [int(model.lstm.hidden_size), len(first)] + first + [len(last)] + last


def model_arrays(model):
    """params in cs_value_net_pack_lstm's order: mlp1's pairs, the LSTM's four tensors, mlp's pairs"""
    sd = {k: v.detach().cpu().numpy().astype(F32) for k, v in model.state_dict().items()}
    pairs = lambda name: [sd[f"{name}.{i}.{p}"] for i in sorted({int(k.split(".")[1]) for k in sd if k.startswith(name + ".")}) for p in ("weight", "bias")]
    return pairs("mlp1") + [sd["lstm.weight_ih_l0"], sd["lstm.weight_hh_l0"], sd["lstm.bias_ih_l0"], sd["lstm.bias_hh_l0"]] + pairs("mlp")


def _linear_piece(wgt, bias):
    """a float32 layer as include/crowdstep.h states it: [ncb][kg][64 lanes][4], then bias[32 ncb]"""
    N, K = wgt.shape
    ncb, kg = -(-N // 32), -(-K // 8)
    out = np.zeros((ncb, kg, 64, 4), F32)
    for cb in range(ncb):
        for g in range(kg):
            for l in range(64):
                for s in range(4):
                    k, col = 8 * g + 4 * (l >> 5) + s, 32 * cb + (l & 31)
                    if k < K and col < N:
                        out[cb, g, l, s] = wgt[col, k]
    b = np.zeros(32 * ncb, F32)
    b[:N] = bias
    return np.concatenate([out.ravel(), b])


def _gate_piece(wih, whh, bih, bhh):
    """the gates as include/crowdstep.h states them: [nb][kg][64 lanes][4] with h's k-groups first, then bias[32 nb] = bias_ih + bias_hh"""
    H, K = whh.shape[1], wih.shape[1]
    nb, kgh, kgx = -(-H // 8), -(-H // 8), -(-K // 8)
    out = np.zeros((nb, kgh + kgx, 64, 4), F32)
    bias = np.zeros(32 * nb, F32)
    for b in range(nb):
        for j in range(32):
            unit = 8 * b + (j & 7)
            if unit >= H:
                continue
            row = (j >> 3) * H + unit
            bias[32 * b + j] = F32(bih[row]) + F32(bhh[row])
            for g in range(kgh + kgx):
                for half in range(2):
                    for s in range(4):
                        k = 8 * (g if g < kgh else g - kgh) + 4 * half + s
                        src = whh if g < kgh else wih
                        if k < src.shape[1]:
                            out[b, g, 32 * half + j, s] = src[row, k]
    return np.concatenate([out.ravel(), bias])


def layout_blob(dims, arrays):
    """cs_value_net_pack_lstm's blob rebuilt from the header's words alone"""
    n1 = dims[1]
    n2 = dims[2 + n1]
    pieces = [_linear_piece(arrays[2 * l], arrays[2 * l + 1]) for l in range(n1)]
    pieces.append(_gate_piece(*arrays[2 * n1:2 * n1 + 4]))
    pieces += [_linear_piece(arrays[2 * n1 + 4 + 2 * l], arrays[2 * n1 + 5 + 2 * l]) for l in range(n2)]
    return np.concatenate(pieces)


def pack_call(dims, cols, arrays, size_only=False):
    """(status, message, blob) of cs_value_net_pack_lstm on host arrays"""
    import ctypes as C

    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    d = np.ascontiguousarray(dims, np.int32)
    nf = C.c_size_t(0)
    rc = lib.cs_value_net_pack_lstm(d.ctypes.data if len(d) else None, len(d), cols, None, None, C.byref(nf))
    if rc != 0 or size_only:
        return rc, lib.cs_last_error().decode(), nf.value
    arrays = [np.ascontiguousarray(a, F32) for a in arrays]
    ptrs = (C.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])
    blob = np.full(nf.value, F32(-7.0))
    rc = lib.cs_value_net_pack_lstm(d.ctypes.data, len(d), cols, ptrs, blob.ctypes.data, C.byref(nf))
    return rc, lib.cs_last_error().decode(), blob


# ---------------------------------------------------------------------------------------------------------------- golden G21
@functools.lru_cache(maxsize=None)
def g21():
    """golden G21 by case kind: {kind: [cases]}"""
    from golden_io import load_cases

    out = {}
    for c in load_cases("g21_lstm_rl"):
        out.setdefault(c["kind"], []).append(c)
    return out


def draw_weights(model, seed, calm_last=False):
    """om_cases.draw_weights(calm=True); with `calm_last` mlp's output layer is then multiplied by 0.1 (an untrained value head of a few
    units instead of tens).  Returns the SHA-256 of the drawn float32 bytes."""
    import torch

    import om_cases

    digest = om_cases.draw_weights(model, seed, calm=True)
    if calm_last:
        last = max(int(k.split(".")[1]) for k in model.state_dict() if k.startswith("mlp.") and k.endswith(".weight"))
        with torch.no_grad():
            model.mlp[last].weight.mul_(0.1)
            model.mlp[last].bias.mul_(0.1)
    return digest


def g21_policy(wkey):
    """A configured LSTM-RL of this project with the weights of G21's network `wkey`, rebuilt from the seed and checked by SHA-256"""
    case = next(c for c in g21()["weights"] if c["wkey"] == wkey)
    pol = lstm_policy(int(case["network"]), int(case["cols"]))
    sd = pol.model.state_dict()
    assert sorted(sd) == list(case["weights_keys"]) and [list(sd[k].shape) for k in sorted(sd)] == case["weights_shapes"]
    assert draw_weights(pol.model, int(case["seed"]), bool(case["calm_last"])) == case["sha256"]
    return pol
