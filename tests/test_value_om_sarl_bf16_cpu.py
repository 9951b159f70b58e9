"""CPU side of the opt-in bf16 arithmetic of OM-SARL's decision (cs_value_net_pack_om_bf16 / cs_value_net_decide_om_bf16):
the two entries as include/crowdstep.h declares them, the blob rebuilt from the header's words, the argument checks without a device,
the setter of its own beside the refusals that stay, the key sets of a ``DeviceNet``, and the properties of the arithmetic itself -- zero
map weights, the mutants the contract excludes, golden G20 (c) -- shown with tests/om_sarl_bf16_emulation.py.  The kernel against that
emulation is tests/test_gpu_value_om_sarl_bf16.py, which takes its networks and grids from here."""
import ctypes as C
import functools
import inspect
import os

import numpy as np
import pytest
import torch

import bf16_emulation as em
import decision_edges as de
import om_cases
import om_sarl_bf16_emulation as oem
import parity_util
from test_value_om_cpu import g20, g20_policy, om_policy
from test_value_policy_cpu import make_policy, numpy_weights

F32 = np.float32
SYMBOLS = ("cs_value_net_pack_om_bf16", "cs_value_net_decide_om_bf16")
DEFAULT_WIDTHS = dict(mlp1=[150, 100], mlp2=[100, 50], attention=[100, 100, 1], mlp3=[150, 100, 100, 1])
SMALL_WIDTHS = dict(mlp1=[40, 24], mlp2=[33], attention=[20, 1], mlp3=[9, 1])
# C -> the grid (cell_num, cell_size, om_channel_size) whose maps supply the columns.  No grid has 17 columns (C = cells x 1, 2 or 3):
# the 17 are the first 17 of the 18-column grid's, one column over the k-step of 16
GRIDS = {1: (1, 2.0, 1), 16: (4, 1.0, 1), 17: (3, 0.7, 2), 48: (4, 1.0, 3), 192: (8, 0.5, 3)}


def wide_model(cols, C_, with_global=True, widths=None, seed=4500, scale=1.0):
    """SARL's module on rows of cols + C_ columns with om_cases.draw_weights' seeded weights (the calm attention layer), on the CPU"""
    from social_navigation_pyenvs_amd.crowd_nav.policy.sarl import ValueNetwork

    d = dict(DEFAULT_WIDTHS, **(widths or {}))
    model = ValueNetwork(cols + C_, 6, d["mlp1"], d["mlp2"], d["mlp3"], d["attention"], with_global)
    om_cases.draw_weights(model, seed)
    if scale != 1.0:
        with torch.no_grad():
            for prm in model.parameters():
                prm.mul_(scale)
    return model


def model_arrays(model):
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    kind, dims, layers = value_net.describe(model)
    return kind, dims, [p.detach().cpu().numpy() for l in layers for p in (l.weight, l.bias)]


def narrow_twin(model, cols):
    """(the module with zeros on the map columns of mlp1's first layer -- in place --, the SARL module on `cols` columns with the same weights)"""
    from social_navigation_pyenvs_amd.crowd_nav.policy.sarl import ValueNetwork

    lin = lambda seq: [m.out_features for m in seq if isinstance(m, torch.nn.Linear)]
    twin = ValueNetwork(cols, 6, lin(model.mlp1), lin(model.mlp2), lin(model.mlp3), lin(model.attention), model.with_global_state)
    with torch.no_grad():
        model.mlp1[0].weight[:, cols:].zero_()
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        sd["mlp1.0.weight"] = sd["mlp1.0.weight"][:, :cols].contiguous()
        twin.load_state_dict(sd, strict=True)
    return model, twin


@functools.lru_cache(maxsize=None)
def host_case(cols, C_, n, W, A):
    """Rows without a device: torch.randn rotated rows with one self state per (world, action), as decision_edges' sweep draws them; maps
    of humans pulled together (om_cases.maps64, float32), the first C_ columns of GRIDS[C_]'s; rewards; robot rows.  Read-only."""
    g = torch.Generator().manual_seed(100000 * n + 100 * A + W + cols)
    rot = torch.randn((W, A, n, cols), generator=g)
    rot[..., :6] = rot[:, :, :1, :6]
    rew = torch.randn((W, A), generator=g) * 0.1
    humans = om_cases.random_worlds(900 + n + C_, W, n, 4, 2)
    humans[..., 0:2] = humans[..., 0:2] * F32(0.4)
    maps = np.stack([om_cases.maps64(h, *GRIDS[C_])[0][:, :C_] for h in humans]).astype(F32)
    assert np.count_nonzero(maps) > 0
    out = rot.numpy(), maps, rew.numpy(), de.robot_rows(W, 9, np.random.default_rng([n, W, A, C_]))
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_the_entries_are_bound_with_the_headers_argument_types():
    from test_abi_cpu import _header_prototypes

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib._PKG), "include", "crowdstep.h")).read()
    protos = _header_prototypes(header)
    I, P, Z, F_ = C.c_int, C.c_void_p, C.c_size_t, C.c_float
    spelled = {SYMBOLS[0]: [I, P, I, I, I, P, P, P],
               SYMBOLS[1]: [I, P, I, P, Z, I, I, I, I, I, P, P, P, P, P, I, F_, F_, P, P, P, P, P]}
    for sym in SYMBOLS:
        assert sym in _lib.ABI_SYMBOLS and sym in _lib.ABI and hasattr(lib, sym) and f"int {sym}(" in header, sym
        fn = getattr(lib, sym)
        assert (fn.restype, list(fn.argtypes)) == protos[sym] == (C.c_int, spelled[sym]) == (_lib.ABI[sym][0], list(_lib.ABI[sym][1])), sym
    # the float32 entries beside them: the same arguments but the blob's pointer type, which ctypes does not tell apart
    assert protos[SYMBOLS[1]][1] == protos["cs_value_net_decide_om"][1] and protos[SYMBOLS[0]][1] == protos["cs_value_net_pack_om"][1]
    assert _lib.ABI_VERSION == 4 and lib.cs_abi_version() == 4 and "#define CS_ABI_VERSION 4" in header      # an added symbol bumps nothing
    wide = value_net.MAPPED.wide
    assert (wide.pack, wide.decide, wide.word, wide.key) == ((SYMBOLS[0], np.uint8), SYMBOLS[1], "wide", "wide_bf16") and wide.key == value_net.WIDE_BF16
    assert value_net.WIDE_PRECISIONS == ("f32", "bf16") and value_net.WIDE_BF16 not in value_net.PRECISIONS + (value_net.RECURRENT_BF16, value_net.MAPPED_RECURRENT_BF16)
    assert "refresh_wide" in wide.no_blob and value_net.own_arithmetic(value_net.MAPPED) is wide
    assert value_net.own_arithmetic(value_net.FEED_FORWARD) is None and value_net.own_arithmetic(value_net.RECURRENT) is value_net.RECURRENT.own


# ---------------------------------------------------------------------------------------------------------------- the blob
def _bf16_words(a):
    return torch.tensor(np.asarray(a, F32)).bfloat16().view(torch.int16).numpy().view(np.uint16)


def _lane_slots(part, per_lane):
    """[ncb][slots][64 lanes][per_lane] of a weight part [N][K]: element e of lane l of slot s of block b =
    part[32 b + (l & 31)][2 per_lane s + per_lane (l >> 5) + e], zeros beyond N and K"""
    N, K = part.shape
    ncb, slots = -(-N // 32), -(-K // (2 * per_lane))
    padded = np.zeros((32 * ncb, 2 * per_lane * slots), part.dtype)
    padded[:N, :K] = part
    return padded.reshape(ncb, 32, slots, 2, per_lane).transpose(0, 2, 3, 1, 4).reshape(ncb, slots, 64, per_lane)


def _piece(slot_bytes, bias):
    ncb = slot_bytes.shape[0]
    bb = np.zeros(32 * ncb, F32)
    bb[:len(bias)] = bias
    return np.concatenate([np.ascontiguousarray(slot_bytes).reshape(-1), bb.view(np.uint8)])


def layout_blob(dims, arrays, cols):
    """cs_value_net_pack_om_bf16's blob from the words of include/crowdstep.h alone: cs_value_net_pack_bf16's layout -- mlp3 float32
    [ncb][kg][64][4], every other layer bf16 [ncb][ks][64][8] with the attention's crowd-mean half in k-steps of its own behind the first
    source's -- with mlp1's layer 0 as [ncb][2 + ksm][64] slots of 16 bytes: 4 floats of the rotated columns, 8 bf16 of a map k-step."""
    dims = list(dims)
    with_global, at, chains = dims[0], 1, []
    for _ in range(4):
        chains.append(dims[at + 1:at + 1 + dims[at]])
        at += 1 + dims[at]
    as_bytes = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[:3] + (16,))
    pieces, l = [], 0
    for c, widths in enumerate(chains):
        for i in range(len(widths)):
            wgt, bias = np.asarray(arrays[2 * l], F32), np.asarray(arrays[2 * l + 1], F32)
            if c == 0 and i == 0:
                slots = np.concatenate([as_bytes(_lane_slots(wgt[:, :cols], 4)), as_bytes(_lane_slots(_bf16_words(wgt[:, cols:]), 8))], axis=1)
                assert slots.shape[1] == 2 + -(-(wgt.shape[1] - cols) // 16)
            elif c == 3:
                slots = as_bytes(_lane_slots(wgt, 4))
            elif c == 2 and i == 0 and with_global:
                half = wgt.shape[1] // 2
                slots = np.concatenate([as_bytes(_lane_slots(_bf16_words(wgt[:, :half]), 8)), as_bytes(_lane_slots(_bf16_words(wgt[:, half:]), 8))], axis=1)
            else:
                slots = as_bytes(_lane_slots(_bf16_words(wgt), 8))
            pieces.append(_piece(slots, bias))
            l += 1
    return np.concatenate(pieces)


def pack_call(kind, dims, cols, C_, arrays, size_only=False, fill=0xA5):
    """(status, message, blob bytes or the size) of cs_value_net_pack_om_bf16 on host arrays; the blob is handed over filled with `fill`"""
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    d = np.ascontiguousarray(dims, np.int32)
    nb = C.c_size_t(0)
    rc = lib.cs_value_net_pack_om_bf16(kind, d.ctypes.data, len(d), cols, C_, None, None, C.byref(nb))
    if rc != 0 or size_only:
        return rc, lib.cs_last_error().decode(), nb.value
    arrays = [np.ascontiguousarray(a, F32) for a in arrays]
    ptrs = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
    blob = np.full(nb.value, fill, np.uint8)
    rc = lib.cs_value_net_pack_om_bf16(kind, d.ctypes.data, len(d), cols, C_, ptrs, blob.ctypes.data, C.byref(nb))
    return rc, lib.cs_last_error().decode(), blob


@pytest.mark.parametrize("cols,C_,with_global,widths", [(13, 1, True, SMALL_WIDTHS), (15, 16, False, SMALL_WIDTHS), (13, 17, True, SMALL_WIDTHS),
                                                        (15, 48, True, SMALL_WIDTHS), (13, 48, True, None), (15, 17, False, dict(mlp1=[33]))])
def test_the_blob_is_the_documented_layout(cols, C_, with_global, widths):
    """Map columns on and off the k-step of 16, both column counts, widths off 32, mlp1 of one layer, with and without the crowd-mean half:
    the bytes of the layout rebuilt from the header, whatever the blob held before (the padding is written as zero)."""
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    model = wide_model(cols, C_, with_global, widths, seed=60 + C_)
    kind, dims, arrays = model_arrays(model)
    want = layout_blob(dims, arrays, cols)
    rc, msg, size = pack_call(kind, dims, cols, C_, None, size_only=True)
    assert (rc, size) == (0, want.size), msg
    for fill in (0xA5, 0x00):
        rc, msg, blob = pack_call(kind, dims, cols, C_, arrays, fill=fill)
        assert rc == 0 and blob.tobytes() == want.tobytes(), msg
    got = value_net.pack_om_bf16(dims, cols, C_, arrays)
    assert got.dtype == np.uint8 and got.tobytes() == want.tobytes()
    f32_blob = value_net.pack(kind, dims, cols, arrays, om_cols=C_)          # the float32 entry is untouched by the new one
    assert f32_blob.dtype == F32 and f32_blob.nbytes != want.size
    # the layers behind the first are cs_value_net_pack_bf16's, byte for byte, on the narrow twin
    wide, twin = narrow_twin(model, cols)
    _, ndims, narrays = model_arrays(twin)
    narrow = value_net.pack(kind, ndims, cols, narrays, precision="bf16")
    ncb = -(-dims[2] // 32)
    assert narrow[ncb * 2 * 1024:].tobytes() == want[ncb * (2 + -(-C_ // 16)) * 1024:].tobytes()


# ---------------------------------------------------------------------------------------------------------------- the entries' checks
_SARL = [1, 2, 150, 100, 2, 100, 50, 3, 100, 100, 1, 4, 150, 100, 100, 1]
_CADRL = [4, 150, 100, 100, 1]
FAKE = 0x1000


def _decide(**change):
    """cs_value_net_decide_om_bf16 on fake pointers (never followed: every call here fails a check)"""
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    a = dict(kind=1, dims=_SARL, W=4, A=81, n=5, cols=13, om_cols=48, robot_stride=9, n_bytes=None, null=())
    a.update(change)
    dims = np.array(a["dims"], np.int32)
    if a["n_bytes"] is None:
        rc, _, a["n_bytes"] = pack_call(1, _SARL, 13, 48, None, size_only=True)
        assert rc == 0 and a["n_bytes"] > 0
    fake = lambda name: None if name in a["null"] else FAKE
    rc = lib.cs_value_net_decide_om_bf16(a["kind"], dims.ctypes.data, len(dims), fake("d_weights"), a["n_bytes"], a["W"], a["A"], a["n"], a["cols"], a["om_cols"],
                                         fake("d_rotated"), fake("d_maps"), fake("d_rewards"), fake("d_actions"), fake("d_robot"), a["robot_stride"], 0.9, 0.25,
                                         None, fake("d_values"), None, fake("d_action_out"), None)
    return rc, lib.cs_last_error().decode()


def _f32_bytes():
    from test_value_om_cpu import _pack_size

    return 4 * _pack_size(1, _SARL, 13, 48)[2]


def _narrow_bytes():
    from social_navigation_pyenvs_amd import _lib

    nb, d = C.c_size_t(0), np.array(_SARL, np.int32)
    assert _lib.load().cs_value_net_pack_bf16(1, d.ctypes.data, len(d), 13, None, None, C.byref(nb)) == 0
    return nb.value


@pytest.mark.parametrize("change,fragment", [
    (dict(kind=0, dims=_CADRL), "occupancy maps belong to SARL's network"),
    (dict(kind=2), "unknown value network kind"),
    (dict(cols=14), "rotated rows have 13 or 15 columns"),
    (dict(om_cols=0), "om_cols must be at least 1"), (dict(om_cols=-3), "om_cols must be at least 1"),
    (dict(om_cols=244), "exceed a layer's 256 inputs"), (dict(cols=15, om_cols=243), "exceed a layer's 256 inputs"),
    (dict(dims=_SARL[:-5]), "layer description ends early"),
    (dict(W=0), "W and A must be positive"), (dict(A=0), "W and A must be positive"), (dict(n=0), "n must be at least 1"),
    *[(dict(null=(name,)), "null argument") for name in ("d_weights", "d_rotated", "d_maps", "d_rewards", "d_actions", "d_robot", "d_values", "d_action_out")],
    (dict(n_bytes=5), "does not have the size"),
    (dict(n_bytes="f32"), "does not have the size"),       # (cs_value_net_pack_om's blob)
    (dict(n_bytes="narrow"), "does not have the size"),    # (cs_value_net_pack_bf16's)
    (dict(om_cols=49), "does not have the size"),          # (a fourth map k-step, not the blob packed for 48)
    (dict(robot_stride=7), "robot rows need at least 8 columns"),
])
def test_the_decide_entry_checks_its_arguments_before_touching_a_device(change, fragment):
    """cs_value_net_decide_om's table (test_value_om_cpu.py) for the new entry: the same fragments in the same cases, and the blobs of the
    two parent kernels refused by their size."""
    from social_navigation_pyenvs_amd import _lib

    change = dict(change)
    if change.get("n_bytes") == "f32":
        change["n_bytes"] = _f32_bytes()
    elif change.get("n_bytes") == "narrow":
        change["n_bytes"] = _narrow_bytes()
    rc, message = _decide(**change)
    assert rc == _lib.CS_ERR_ARG and fragment in message, message


def test_the_pack_entry_answers_the_size_and_refuses_what_pack_om_refuses():
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    for args, fragment in (((0, _CADRL, 13, 48), "occupancy maps belong to SARL's network"), ((1, _SARL, 13, 0), "om_cols must be at least 1"),
                           ((1, _SARL, 15, 242), "exceed a layer's 256 inputs"), ((1, _SARL, 12, 48), "rotated rows have 13 or 15 columns"),
                           ((3, _SARL, 13, 48), "unknown value network kind")):
        rc, message, _ = pack_call(*args, None, size_only=True)
        assert rc == _lib.CS_ERR_ARG and fragment in message, message
    d = np.array(_SARL, np.int32)
    assert lib.cs_value_net_pack_om_bf16(1, d.ctypes.data, len(d), 13, 48, None, None, None) == _lib.CS_ERR_ARG and b"null argument" in lib.cs_last_error()
    rc, _, size = pack_call(1, _SARL, 13, 48, None, size_only=True)
    # mlp1 layer 0: 5 blocks x (2 float32 k-groups + 3 map k-steps) slots of 64 x 16 bytes; one k-step fewer for 32 map columns
    assert rc == 0 and size - pack_call(1, _SARL, 13, 32, None, size_only=True)[2] == 5 * 1024 and len({size, _f32_bytes(), _narrow_bytes()}) == 3
    assert pack_call(1, _SARL, 13, 243, None, size_only=True)[0] == 0 and pack_call(1, _SARL, 15, 241, None, size_only=True)[0] == 0
    blob = np.zeros(size, np.uint8)
    nb = C.c_size_t(0)
    assert lib.cs_value_net_pack_om_bf16(1, d.ctypes.data, len(d), 13, 48, None, blob.ctypes.data, C.byref(nb)) == _lib.CS_ERR_ARG
    assert b"null argument" in lib.cs_last_error()


# ---------------------------------------------------------------------------------------------------------------- the setters
def test_the_setter_holds_the_new_mode_and_the_pinned_refusals_still_raise():
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net
    from social_navigation_pyenvs_amd.crowd_nav.policy.policy_factory import policy_factory

    pol = om_policy()
    assert type(pol) is policy_factory["om_sarl"] and pol.wide_precision == "f32"
    pol.set_wide_precision("bf16")
    assert (pol.wide_precision, pol.decision_precision, pol.decision_input, pol.recurrent_precision, pol.mapped_precision) == ("bf16", "f32", "tensor", "f32", "f32")
    for bad in ("fp8", "BF16", None, 16, ""):
        with pytest.raises(ValueError, match="wide precision .*'f32', 'bf16'"):
            pol.set_wide_precision(bad)
    assert pol.wide_precision == "bf16"
    # the refusals the existing tests pin, repeated: nobody "fixes" them by routing them to the new kernel
    for call, arg in ((pol.set_decision_input, "fused"), (pol.set_decision_precision, "bf16")):
        with pytest.raises(ValueError, match="occupancy-map columns.*OM-SARL decides with"):
            call(arg)
    with pytest.raises(ValueError, match="the kernel of OM-LSTM-RL"):
        value_net.check_mapped_precision("bf16", value_net.MAPPED)
    with pytest.raises(ValueError, match="OM-SARL decides with"):
        value_net.pack(*value_net.describe(pol.model)[:2], 13, [], precision="bf16", om_cols=48)
    assert not hasattr(pol, "set_mapped_precision") and not hasattr(pol, "set_recurrent_precision") and pol.mapped_precision == "f32"
    assert not hasattr(policy_factory["om_sarl"](), "set_mapped_precision") and policy_factory["om_sarl"]().mapped_precision == "f32"
    pol.set_wide_precision("f32")
    assert pol.wide_precision == "f32"
    fam = value_net.MAPPED                                           # the family's row is what it was
    assert fam.own is None and fam.modes == (("tensor", "f32"),) and dict(fam.pack) == {"f32": ("cs_value_net_pack_om", F32)}
    assert dict(fam.decide) == {"f32": "cs_value_net_decide_om"}
    # only OM-SARL gets the setter; every policy holds the attribute the Gym reads
    for key in ("cadrl", "sarl", "lstm_rl_device", "om_lstm_rl"):
        other = policy_factory[key]()
        assert not hasattr(other, "set_wide_precision") and other.wide_precision == "f32", key
    for family in (value_net.FEED_FORWARD, value_net.RECURRENT, value_net.RECURRENT_MAPPED):
        assert family.wide is None
        with pytest.raises(ValueError, match="the kernel of OM-SARL"):
            value_net.check_wide_precision("bf16", family)
        assert value_net.check_wide_precision("f32", family) == "f32"
    assert value_net.check_wide_precision("bf16", value_net.MAPPED) == "bf16" and value_net.check_wide_precision("bf16") == "bf16"


def test_the_blob_key_exists_on_an_om_sarl_net_alone():
    import lstm_cases as lc
    import om_lstm_cases as olc

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    key = value_net.WIDE_BF16
    fourth = list(inspect.signature(value_net.DeviceNet.refresh_selected).parameters.values())[4]
    assert (fourth.name, fourth.default) == ("wide_precision", "f32")
    assert inspect.signature(value_net.decide_for_worlds).parameters["wide_precision"].default == "f32"
    pol = om_policy()
    net = pol._new_device_net(pol.model)
    assert net.family is value_net.MAPPED and set(net._keys) == set(net.blobs) == {"f32", "bf16", value_net.RECURRENT_BF16, key}
    net._keys.update({"f32": "a", "bf16": "b", value_net.RECURRENT_BF16: "c", key: "d"})
    net.flat = object()
    net.updated_on_device()                                         # a fused training step drops it with the other non-float32 ones
    assert net._keys == {"f32": "a", "bf16": None, value_net.RECURRENT_BF16: None, key: None}
    others = {"sarl": value_net.DeviceNet(make_policy("sarl").model, 13), "cadrl": value_net.DeviceNet(make_policy("cadrl").model, 13),
              "lstm": value_net.DeviceNet(lc.lstm_policy(1).model, 13)}
    om_lstm = olc.om_lstm_policy(1)
    others["om_lstm"] = value_net.DeviceNet(om_lstm.model, om_lstm.joint_state_dim, om_lstm.map_columns(), om_lstm.om_grid())
    for name, other in others.items():
        extra = {value_net.MAPPED_RECURRENT_BF16} if name == "om_lstm" else set()
        assert set(other._keys) == set(other.blobs) == {"f32", "bf16", value_net.RECURRENT_BF16} | extra, name
        with pytest.raises(ValueError, match="the kernel of OM-SARL"):
            other.refresh_wide("bf16")
        with pytest.raises(ValueError, match="wide precision 'half'"):
            other.refresh_wide("half")
        with pytest.raises(ValueError, match="decide_om_bf16: the network is not SARL's with occupancy-map columns"):
            value_net.decide_om_bf16(other, 1, 1, 2, 0, 0, 0, 0, 0, 9, 0.9, 0.25, None, 0, None, 0)
    with pytest.raises(ValueError, match=r"decide_om_bf16: the network has no wide bf16 blob yet \(DeviceNet.refresh_wide"):
        value_net.decide_om_bf16(net, 1, 1, 2, 0, 0, 0, 0, 0, 9, 0.9, 0.25, None, 0, None, 0)
    with pytest.raises(ValueError, match="om_cols must be at least 1"):
        value_net.pack_om_bf16(np.array(_SARL, np.int32), 13, 0, [])


# ---------------------------------------------------------------------------------------------------------------- the arithmetic alone
@pytest.mark.parametrize("cols,C_,with_global,n", [(13, 48, True, 5), (15, 17, False, 17), (13, 16, True, 33), (15, 1, True, 2)])
def test_zero_map_weights_give_the_narrow_emulation_exactly(cols, C_, with_global, n):
    """With all-zero map weights the map columns' part is an exact zero behind the rotated columns' part: the emulation equals
    bf16_emulation.network("sarl", ...) on the narrow rows, in both accumulation modes."""
    wide, twin = narrow_twin(wide_model(cols, C_, with_global, seed=70 + C_), cols)
    rot, maps, _, _ = host_case(cols, C_, n, 3, 11)
    w, wn = numpy_weights(wide), numpy_weights(twin)
    for acc in ("f64", "f32"):
        got, want = oem.network(rot, maps, w, with_global, acc), em.network("sarl", rot, wn, with_global, acc)
        assert np.all(np.isfinite(want)) and np.array_equal(got, want), acc


MUTANT_CASES = ((13, 48, True, 5, 3, 11), (15, 17, False, 17, 3, 11), (13, 16, True, 33, 1, 32))


@pytest.mark.parametrize("mutant", oem.MUTANTS)
def test_mutant_arithmetics_fail_the_kernel_bar(mutant):
    """A kernel that rounded the rotated columns, left the map weights unrounded, or truncated instead of rounding to nearest even would miss
    the GPU file's bar on these inputs: its error against the float64 emulation is beyond F32_SLACK times the float32-accumulation
    emulation's."""
    worst = worst32 = 0.0
    for cols, C_, with_global, n, W, A in MUTANT_CASES:
        w = numpy_weights(wide_model(cols, C_, with_global, seed=80 + C_))
        rot, maps, rew, rob = host_case(cols, C_, n, W, A)
        disc = de.discount(rob)
        e64 = oem.action_values(rot, maps, rew, disc, w, with_global)
        assert np.all(np.isfinite(e64))
        worst32 = max(worst32, de.rel_error(oem.action_values(rot, maps, rew, disc, w, with_global, acc="f32"), e64))
        worst = max(worst, de.rel_error(oem.action_values(rot, maps, rew, disc, w, with_global, mutant=mutant), e64))
    print(f"OM-SARL {mutant}: {worst:.3e} against the float64 emulation; float32-accumulation emulation {worst32:.3e}")
    assert worst > parity_util.F32_SLACK * worst32


# ---------------------------------------------------------------------------------------------------------------- golden G20 (c)
G20_EMULATION_FLIPS = 7             # of the 32 recorded decisions (HISTORY.md)


def g20_decision_values(c, w, rot32, maps32, rew):
    """(float64 full-precision action values, the float64 emulation's) of one recorded decision on the float32 rows and maps a kernel is
    handed: rot32 [81, n, 13], maps32 [n, 48], rew [81]"""
    disc = np.array([float(c["gamma"]) ** (float(c["dt"]) * float(c["robot"][7]))])
    full = np.asarray(rew, np.float64) + disc * em.full_precision("sarl", oem.wide_rows(rot32[None], maps32[None])[0], w)
    return full, oem.action_values(rot32[None], maps32[None], np.asarray(rew)[None], disc, w)[0]


def test_every_flip_of_the_emulation_on_g20_is_explained():
    """The criterion the GPU file holds the kernel to, met by the arithmetic alone: the float64 emulation's pick of every recorded decision
    of G20 (c) is the reference's `chosen`, or gap <= 2 e (bf16_emulation.classify_flip).  The count is pinned, to be read beside the
    kernel's (HISTORY.md)."""
    from oracle import crowd_oracle as orc

    w = numpy_weights(g20_policy("om_sarl_decide").model)
    decisions = g20()["decision"]
    flips = 0
    for k, c in enumerate(decisions):
        rot, rew = orc.lookahead(c["action_space"], c["next_humans"], c["obs"], c["robot"], float(c["dt"]))
        full, e64 = g20_decision_values(c, w, rot.astype(F32), c["maps"].astype(F32), rew)
        chosen = int(c["chosen"])
        assert int(np.argmax(full)) == chosen, k                 # (the full-precision restatement picks the reference's action)
        pick = int(np.argmax(e64))
        if pick != chosen:
            flips += 1
            ok, gap, e = em.classify_flip(chosen, pick, full, e64)
            print(f"G20 (c) decision {k}: the emulation picks {pick}, the reference {chosen}: gap {gap:.3e}, e {e:.3e}")
            assert ok, (k, gap, e)
    print(f"G20 (c), float64 emulation of the bf16 arithmetic: {flips} of {len(decisions)} decisions flipped, all explained")
    assert len(decisions) >= 20 and flips == G20_EMULATION_FLIPS
