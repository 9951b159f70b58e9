"""CPU side of the opt-in bf16 arithmetic of LSTM-RL's decision (cs_value_net_pack_lstm_bf16 / cs_value_net_decide_lstm_bf16):
the exported symbols, the blob as include/crowdstep.h words it, the pack entry's rounding, the argument checks without a device, the
setters, and the properties of the arithmetic itself -- on the cases the GPU file (tests/test_gpu_value_lstm_bf16.py) holds the kernel to,
on the mutants the contract excludes and on golden G21 -- shown with tests/lstm_bf16_emulation.py.

The cases and their references are built here once (``case_data``, cached) and shared with the GPU file."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

import bf16_emulation as em
import lstm_bf16_emulation as lem
import lstm_cases as lc
import parity_util
from social_navigation_pyenvs_amd.crowd_nav.policy.value_net import RECURRENT_BF16, RECURRENT_PRECISIONS      # (the mode under test)

F32 = np.float32
DT, GAMMA = 0.25, 0.9
MARGIN = 4.0
TIGHT_CAP, REFERENCE_CAP, MUTANT_FLOOR = 1 / 4, 1 / 8, 1 / 2

# (network, cols, H, n, W, A, overrides, W_hh zeroed)
TIGHT = [
    (1, 13, 50, 5, 3, 81, {}, False),                                                            # the default, register build
    (1, 15, 8, 1, 2, 33, dict(lstm_rl__mlp2_dims="1"), False),                                   # one block, one k-step
    (1, 13, 16, 2, 3, 27, {}, False),                                                            # H on the k-step
    (1, 13, 17, 2, 3, 27, {}, False),                                                            # H one over the k-step
    (1, 13, 33, 2, 3, 27, dict(lstm_rl__mlp2_dims="70, 33, 1"), False),
    (1, 13, 64, 5, 3, 27, {}, False),
    (1, 15, 96, 5, 3, 27, dict(lstm_rl__mlp2_dims="40, 1"), False),                              # weights from the blob
    (2, 13, 50, 5, 3, 27, {}, False),
    (2, 15, 33, 5, 3, 81, dict(lstm_rl__mlp1_dims="40, 20", lstm_rl__mlp2_dims="70, 1"), False),
    (2, 13, 64, 2, 3, 27, dict(lstm_rl__mlp1_dims="60, 50"), False),
    # long sequences with lstm.weight_hh_l0 zeroed: c and every step still matter, only the last h is an operand
    (1, 13, 50, 33, 1, 64, {}, True),
    (1, 13, 64, 64, 1, 64, {}, True),
    (1, 15, 96, 128, 1, 64, dict(lstm_rl__mlp2_dims="40, 1"), True),
    (2, 13, 50, 33, 1, 64, {}, True),
]
LOOSE_ONLY = [
    (1, 13, 50, 25, 2, 81, {}, False),
    (1, 13, 64, 33, 1, 64, {}, False),
    (1, 15, 96, 64, 1, 64, dict(lstm_rl__mlp2_dims="40, 1"), False),
    (1, 13, 50, 128, 1, 64, {}, False),
    (2, 13, 50, 25, 2, 81, {}, False),
]


def case_id(case):
    network, cols, H, n, W, A, _, zeroed = case
    return f"net{network}-{cols}c-H{H}-n{n}-{W}x{A}" + ("-whh0" if zeroed else "")


def case_policy(case):
    import torch

    from test_gpu_value_lstm import seeded_policy

    network, cols, H, n, W, A, overrides, zeroed = case
    pol = seeded_policy(network, cols, 100 + H + n, lstm_rl__global_state_dim=H, **overrides)
    pol.set_recurrent_precision("bf16")                         # (the mode the GPU file decides in)
    if zeroed:
        with torch.no_grad():
            pol.model.lstm.weight_hh_l0.zero_()
    return pol


@functools.lru_cache(maxsize=None)
def _case_data(idx):
    from test_gpu_value_lstm import random_case

    case = (TIGHT + LOOSE_ONLY)[idx]
    network, cols, H, n, W, A, _, _ = case
    pol = case_policy(case)
    rot, rew, acts, rob = random_case(7 * n + W, W, A, n, cols)
    w = lc.weights64(pol.model)
    rows = lc.sort_rows(rot.astype(np.float64))
    v64 = lc.forward64(w, rows)
    e_ref = float(np.max(np.abs(lc.torch_values(copy.deepcopy(pol.model).cpu(), rows) - v64)))      # as test_gpu_value_lstm.restated measures it
    disc = np.power(GAMMA, DT * rob[:, 7].astype(np.float64))
    full = rew.astype(np.float64) + disc[:, None] * v64
    emu64 = lem.action_values(w, rot, rew, disc)
    emu32 = lem.action_values(w, rot, rew, disc, acc="f32")
    data = dict(case=case, pol=pol, w=w, rot=rot, rew=rew, acts=acts, rob=rob, disc=disc, e_ref=e_ref, full=full, emu64=emu64, emu32=emu32,
                own_error=float(np.max(np.abs(emu64 - full))))
    for a in (rot, rew, acts, rob, full, emu64, emu32):
        a.setflags(write=False)
    return data


def case_data(case):
    """The inputs (test_gpu_value_lstm.random_case), the policy (seeded_policy), E_ref and the references of one case, computed once:
    full = the float64 full-precision restatement, emu64 / emu32 = the emulation of the bf16 contract, own_error = worst |emu64 - full|."""
    return _case_data((TIGHT + LOOSE_ONLY).index(case))


def share_beyond(got, d):
    """(share of the case's sequences farther than MARGIN x E_ref from the float64 emulation, the median distance)"""
    err = np.abs(np.asarray(got, np.float64) - d["emu64"]).ravel()
    return float(np.mean(err > MARGIN * d["e_ref"])), float(np.median(err))


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_the_symbols_are_declared_listed_and_exported():
    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    lib = _lib.load()
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib._PKG), "include", "crowdstep.h")).read()
    for sym in ("cs_value_net_pack_lstm_bf16", "cs_value_net_decide_lstm_bf16"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(lib, sym) and f"int {sym}(" in header, sym
    assert _lib.ABI_VERSION == 4 and lib.cs_abi_version() == 4 and "#define CS_ABI_VERSION 4" in header
    assert value_net.RECURRENT_PRECISIONS == RECURRENT_PRECISIONS == ("f32", "bf16") and RECURRENT_BF16 not in value_net.PRECISIONS


# ---------------------------------------------------------------------------------------------------------------- the pack entry
def pack_call(dims, cols, arrays, size_only=False, fill=0xA5):
    """(status, message, blob bytes or the size) of cs_value_net_pack_lstm_bf16 on host arrays; the blob is handed over filled with `fill`"""
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    d = np.ascontiguousarray(dims, np.int32)
    nb = C.c_size_t(0)
    rc = lib.cs_value_net_pack_lstm_bf16(d.ctypes.data if len(d) else None, len(d), cols, None, None, C.byref(nb))
    if rc != 0 or size_only:
        return rc, lib.cs_last_error().decode(), nb.value
    arrays = [np.ascontiguousarray(a, F32) for a in arrays]
    ptrs = (C.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])
    blob = np.full(nb.value, fill, np.uint8)
    rc = lib.cs_value_net_pack_lstm_bf16(d.ctypes.data, len(d), cols, ptrs, blob.ctypes.data, C.byref(nb))
    return rc, lib.cs_last_error().decode(), blob


def _words(a):
    """float32 values -> bf16 bit patterns by bf16_emulation.bf16 (nearest even; the float32 of a bf16 value holds it in its upper half)"""
    r = em.bf16(np.asarray(a, F32)).astype(F32)
    out = (r.view(np.uint32) >> 16).astype(np.uint16)
    return np.where(np.isnan(r), np.uint16(0x7FC0), out)


def _f32_piece(wgt, bias):
    """a float32 layer in the header's words: float [ncb][kg][64 lanes][4], then float bias[32 ncb]"""
    return lc._linear_piece(wgt, bias).view(np.uint8)


def _bf16_piece(wgt, bias):
    """a bf16 layer in the header's words: bf16 [ncb][ks][64 lanes][8], element e of lane l of k-step s of block b = weight[32 b + (l & 31)]
    [16 s + 8 (l >> 5) + e]; then float bias[32 ncb]"""
    N, K = wgt.shape
    ncb, ks = -(-N // 32), -(-K // 16)
    img = np.zeros((ncb, ks, 64, 8), np.uint16)
    want = _words(wgt)
    for b in range(ncb):
        for s in range(ks):
            for l in range(64):
                for e in range(8):
                    row, k = 32 * b + (l & 31), 16 * s + 8 * (l >> 5) + e
                    if row < N and k < K:
                        img[b, s, l, e] = want[row, k]
    bb = np.zeros(32 * ncb, F32)
    bb[:N] = bias
    return np.concatenate([img.ravel().view(np.uint8), bb.view(np.uint8)])


def _gate_piece(wih, whh, bih, bhh, net2):
    """the gates in the header's words: [nb][ksh + ksx][64 lanes] slots of 16 bytes, then float bias[32 nb]"""
    H, K = whh.shape[1], wih.shape[1]
    nb, ksh = -(-H // 8), -(-H // 16)
    ksx = -(-K // 16) if net2 else -(-K // 8)
    slots = np.zeros((nb, ksh + ksx, 64, 16), np.uint8)
    hh_words, ih_words = _words(whh), _words(wih)
    bias = np.zeros(32 * nb, F32)
    for b in range(nb):
        for l in range(64):
            j = l & 31
            unit = 8 * b + (j & 7)
            if unit >= H:
                continue
            row = (j >> 3) * H + unit
            bias[32 * b + j] = F32(bih[row]) + F32(bhh[row])
            for s in range(ksh + ksx):
                if s < ksh or net2:
                    src, base = (hh_words, 16 * s) if s < ksh else (ih_words, 16 * (s - ksh))
                    el = np.zeros(8, np.uint16)
                    for e in range(8):
                        k = base + 8 * (l >> 5) + e
                        if k < src.shape[1]:
                            el[e] = src[row, k]
                    slots[b, s, l] = el.view(np.uint8)
                else:
                    el = np.zeros(4, F32)
                    for e in range(4):
                        k = 8 * (s - ksh) + 4 * (l >> 5) + e
                        if k < K:
                            el[e] = wih[row, k]
                    slots[b, s, l] = el.view(np.uint8)
    return np.concatenate([slots.ravel(), bias.view(np.uint8)])


def layout_blob(dims, arrays):
    """cs_value_net_pack_lstm_bf16's blob rebuilt from the header's words alone"""
    n1 = dims[1]
    n2 = dims[2 + n1]
    pieces = [(_f32_piece if l == 0 else _bf16_piece)(arrays[2 * l], arrays[2 * l + 1]) for l in range(n1)]
    pieces.append(_gate_piece(*arrays[2 * n1:2 * n1 + 4], net2=n1 > 0))
    pieces += [(_f32_piece if l == 0 else _bf16_piece)(arrays[2 * n1 + 4 + 2 * l], arrays[2 * n1 + 5 + 2 * l]) for l in range(n2)]
    return np.concatenate(pieces)


@pytest.mark.parametrize("H", [8, 17, 50, 96])
@pytest.mark.parametrize("network,cols", [(1, 13), (1, 15), (2, 13), (2, 15)])
def test_the_blob_is_the_documented_layout(H, network, cols):
    """Both networks, both column counts, H on and off the blocks of 8 and the k-steps of 16, widths off 32: the bytes of the layout rebuilt
    from the header, whatever the blob held before (the padding is written as zero)."""
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    kw = dict(lstm_rl__global_state_dim=H, lstm_rl__mlp2_dims="70, 33, 1")
    if network == 2:
        kw["lstm_rl__mlp1_dims"] = "40, 20"
    pol = lc.lstm_policy(network, cols, **kw)
    lc.draw_weights(pol.model, 40 + H)
    dims, arrays = lc.model_dims(pol.model), lc.model_arrays(pol.model)
    want = layout_blob(dims, arrays)
    rc, msg, size = pack_call(dims, cols, None, size_only=True)
    assert (rc, size) == (0, want.size), msg
    for fill in (0xA5, 0x00):
        rc, msg, blob = pack_call(dims, cols, arrays, fill=fill)
        assert rc == 0 and blob.tobytes() == want.tobytes(), msg
    assert value_net.pack_lstm_bf16(dims, cols, arrays).tobytes() == want.tobytes()
    f32_blob = value_net.pack(value_net.CS_VN_LSTM, dims, cols, arrays)                 # the float32 entry is untouched by the new one
    assert f32_blob.tobytes() == lc.layout_blob(dims, arrays).tobytes() and f32_blob.nbytes != want.size


def test_the_pack_rounds_to_nearest_even():
    """W_hh of a one-block network filled with exact ties, +-0, subnormals, the overflow edge, NaN and +-inf: every stored bf16 is
    bf16_emulation.bf16's."""
    H = 8
    dims = [H, 0, 1, 1]
    special = np.array([1.00390625, 1.01171875, -1.00390625, 1.0078125, 3.3895314e38, 3.39e38, -3.39e38, 1e-40, 4.6e-41, -4.6e-41, np.inf, -np.inf,
                        np.nan, 0.0, -0.0, 0.1, -0.3, 65280.0, 65408.0, 2.0 ** -133, 2.0 ** -134, 3.0 * 2.0 ** -134], F32)
    whh = np.resize(special, (4 * H, H)).astype(F32)
    rng = np.random.default_rng(3)
    arrays = [rng.normal(size=(4 * H, 13)).astype(F32), whh, np.zeros(4 * H, F32), np.zeros(4 * H, F32), np.zeros((1, 6 + H), F32), np.zeros(1, F32)]
    rc, msg, blob = pack_call(dims, 13, arrays)
    assert rc == 0, msg
    img = blob[:1 * 3 * 64 * 16].reshape(1, 3, 64, 16)[0, 0].copy().view(np.uint16).reshape(64, 8)      # block 0, slot 0: W_hh's only k-step
    want = _words(whh)
    for l in range(32):                                                                 # (lanes 32.. hold k = 8.., beyond H = 8: zero)
        row = (l >> 3) * H + (l & 7)
        assert np.array_equal(img[l], want[row]), (l, img[l], want[row])
    assert not img[32:].any()
    with np.errstate(invalid="ignore"):
        back = (img[:32].astype(np.uint32) << 16).view(F32)
        ref = em.bf16(whh[[(l >> 3) * H + (l & 7) for l in range(32)]])
    assert np.all((back == ref) | (np.isnan(back) & np.isnan(ref)))
    keep = ~np.isnan(ref)
    assert np.array_equal(np.signbit(back[keep]), np.signbit(ref[keep]))


def test_the_pack_entry_answers_the_size_and_refuses_null_arrays():
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    dims = np.array([8, 0, 1, 1], np.int32)
    nb = C.c_size_t(0)
    assert lib.cs_value_net_pack_lstm_bf16(dims.ctypes.data, 4, 13, None, None, None) == _lib.CS_ERR_ARG and b"null argument" in lib.cs_last_error()
    assert lib.cs_value_net_pack_lstm_bf16(dims.ctypes.data, 4, 13, None, None, C.byref(nb)) == 0
    # one block: (1 k-step of W_hh + 2 float32 k-groups of W_ih) slots of 64 x 16 bytes + 32 biases; mlp: 2 float32 k-groups + 32 biases
    assert nb.value == (3 * 64 * 16 + 128) + (2 * 64 * 16 + 128)
    blob = np.zeros(nb.value, np.uint8)
    assert lib.cs_value_net_pack_lstm_bf16(dims.ctypes.data, 4, 13, None, blob.ctypes.data, C.byref(nb)) == _lib.CS_ERR_ARG
    assert b"null argument" in lib.cs_last_error()
    ptrs = (C.c_void_p * 6)(*([blob.ctypes.data] * 5 + [None]))
    assert lib.cs_value_net_pack_lstm_bf16(dims.ctypes.data, 4, 13, ptrs, blob.ctypes.data, C.byref(nb)) == _lib.CS_ERR_ARG
    assert b"null weight or bias array" in lib.cs_last_error()
    for bad, cols, fragment in (([50, 0, 2, 10, 2], 13, "mlp ends in one output"), ([257, 0, 1, 1], 13, "hidden width"), ([8, 0, 1, 1], 14, "13 or 15")):
        rc, msg, _ = pack_call(bad, cols, None, size_only=True)
        assert (rc, fragment in msg) == (_lib.CS_ERR_ARG, True), msg


# ---------------------------------------------------------------------------------------------------------------- the decide entry
def decide_refusal(dims, n_bytes, W=2, A=3, n=5, cols=13, sorted_by_distance=1, stride=9, null=None):
    """cs_value_net_decide_lstm_bf16 with dummy device addresses: only calls whose checks refuse them before any device call"""
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    d = np.ascontiguousarray(dims, np.int32)
    dev = {k: 0x1000 for k in ("weights", "rotated", "rewards", "actions", "robot", "values", "action_out")}
    if null:
        dev[null] = None
    rc = lib.cs_value_net_decide_lstm_bf16(d.ctypes.data, len(d), dev["weights"], n_bytes, W, A, n, cols, sorted_by_distance, dev["rotated"],
                                           dev["rewards"], dev["actions"], dev["robot"], stride, 0.9, 0.25, None, dev["values"], None, dev["action_out"], None)
    return rc, lib.cs_last_error().decode()


def test_the_decide_entry_checks_its_arguments_without_a_device():
    """cs_value_net_decide_lstm's table (test_value_lstm_cpu.py) for the new entry: the same fragments, and the float32 blob's size refused.  (The
    LDS refusal has no row: with bf16 rows the widest network the description allows, 256 everywhere at n = 128, needs about 153 KiB.)"""
    from social_navigation_pyenvs_amd import _lib

    dims = [50, 0, 4, 150, 100, 100, 1]
    _, _, size = pack_call(dims, 13, None, size_only=True)
    _, _, f32_floats = lc.pack_call(dims, 13, None, size_only=True)
    assert size != 4 * f32_floats
    for kw, fragment in [
        (dict(cols=12), "rotated rows have 13 or 15 columns"),
        (dict(W=0), "W and A must be positive"),
        (dict(A=0), "W and A must be positive"),
        (dict(n=0), "n must be at least 1"),
        (dict(null="rotated"), "null argument"),
        (dict(null="weights"), "null argument"),
        (dict(null="action_out"), "null argument"),
        (dict(n_bytes=size - 4), "the weight blob does not have the size of this network"),
        (dict(n_bytes=size - 1), "the weight blob does not have the size of this network"),
        (dict(n_bytes=4 * f32_floats), "the weight blob does not have the size of this network"),
        (dict(stride=7), "robot rows need at least 8 columns"),
        (dict(sorted_by_distance=2), "sorted_by_distance is 0 or 1"),
        (dict(n=129), "at most 128 humans a world (CS_VN_LSTM_MAX_N)"),
    ]:
        kw = dict(kw)
        rc, msg = decide_refusal(kw.pop("dims", dims), kw.pop("n_bytes", size), **kw)
        assert (rc, fragment in msg) == (_lib.CS_ERR_ARG, True), (kw, msg)
    for bad in ([50, 0, 2, 10, 2], [0, 0, 1, 1]):                   # the description's errors come through the decision too
        assert decide_refusal(bad, 4)[0] == _lib.CS_ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- the setters
def test_the_setters_hold_the_new_mode_and_leave_the_old_refusals():
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net
    from social_navigation_pyenvs_amd.crowd_nav.policy.policy_factory import policy_factory
    from om_lstm_cases import om_lstm_policy as om_policy

    for network in (1, 2):
        pol = lc.lstm_policy(network)
        assert pol.recurrent_precision == "f32"
        pol.set_recurrent_precision("bf16")
        assert pol.recurrent_precision == "bf16" and (pol.decision_precision, pol.decision_input) == ("f32", "tensor")
        for bad in ("fp8", "BF16", None, 16, ""):
            with pytest.raises(ValueError, match="'f32', 'bf16'"):
                pol.set_recurrent_precision(bad)
        assert pol.recurrent_precision == "bf16"
        with pytest.raises(ValueError, match="recurrent"):           # the feed-forward setter refuses a recurrent network as before
            pol.set_decision_precision("bf16")
        pol.set_recurrent_precision("f32")
        assert pol.recurrent_precision == "f32" and (pol.decision_precision, pol.decision_input) == ("f32", "tensor")
        assert type(pol) is policy_factory["lstm_rl_device"]
    om = om_policy(1)
    with pytest.raises(ValueError, match="OM-LSTM-RL has the one kernel"):
        om.set_recurrent_precision("bf16")
    with pytest.raises(ValueError, match="'f32', 'bf16'"):
        om.set_recurrent_precision("half")
    om.set_recurrent_precision("f32")
    assert om.recurrent_precision == "f32" and (om.decision_precision, om.decision_input) == ("f32", "tensor")
    # the blob of the new mode has a key of its own, which updated_on_device drops with every other non-float32 one
    net = value_net.DeviceNet(lc.lstm_policy(1).model, 13)
    assert value_net.RECURRENT_BF16 in net.blobs and value_net.RECURRENT_BF16 not in value_net.PRECISIONS
    net._keys.update({"f32": "a", "bf16": "b", value_net.RECURRENT_BF16: "c"})
    net.flat = object()
    net.updated_on_device()
    assert net._keys == {"f32": "a", "bf16": None, value_net.RECURRENT_BF16: None}
    with pytest.raises(ValueError, match="OM-LSTM-RL has the one kernel"):
        value_net.DeviceNet(om.model, om.joint_state_dim, om.map_columns(), om.om_grid()).refresh_recurrent("bf16")
    with pytest.raises(ValueError, match="not an LSTM-RL"):
        value_net.check_recurrent_precision("bf16", value_net.FEED_FORWARD)


# ---------------------------------------------------------------------------------------------------------------- the arithmetic alone
@pytest.mark.parametrize("case", TIGHT, ids=case_id)
def test_the_float32_emulation_is_within_the_tight_cap(case):
    """The GPU file's tight tier met by ONE float32 realisation of the contract: at most 1/8 of a case's sequences farther than 4 x E_ref
    from the float64 emulation -- half the kernel's cap."""
    d = case_data(case)
    share, median = share_beyond(d["emu32"], d)
    print(f"{case_id(case)}: E_ref {d['e_ref']:.3e}; float32 emulation: share beyond {MARGIN:g} x E_ref {share:.3f}, median {median:.3e}")
    assert d["rot"].shape[0] * d["rot"].shape[1] >= 64 and np.all(np.isfinite(d["emu64"]))
    assert share <= REFERENCE_CAP, (share, d["e_ref"])


@pytest.mark.parametrize("case", TIGHT + LOOSE_ONLY, ids=case_id)
def test_the_float32_emulation_is_within_the_loose_bar(case):
    """The GPU file's loose tier met by the float32 emulation: every sequence within F32_SLACK x the case's worst |float64 emulation -
    full-precision float64|, the arithmetic's own error."""
    d = case_data(case)
    worst = float(np.max(np.abs(d["emu32"] - d["emu64"])))
    print(f"{case_id(case)}: the arithmetic's own error {d['own_error']:.3e}; float32 emulation against the float64 one {worst:.3e} "
          f"(ratio {worst / d['own_error']:.3f})")
    assert worst <= parity_util.F32_SLACK * d["own_error"], (worst, d["own_error"])


@pytest.mark.parametrize("mutant", lem.MUTANTS)
def test_every_mutant_is_separated(mutant):
    """An arithmetic the contract excludes is farther than 4 x E_ref from the float64 emulation on MORE than 1/2 of the sequences of every
    tight-tier case that contains what it changes, so the cap of 1/4 tells it from the contract.  What a case must contain: "h_unrounded" a
    rounded h that is not exact (every case); "truncate" and "round_inputs" any (every case); "round_first_layers" any."""
    for case in TIGHT:
        d = case_data(case)
        got = lem.action_values(d["w"], d["rot"], d["rew"], d["disc"], mutant=mutant)
        share, median = share_beyond(got, d)
        print(f"{mutant} on {case_id(case)}: share beyond {MARGIN:g} x E_ref {share:.3f}, median {median:.3e} (E_ref {d['e_ref']:.3e})")
        assert share > MUTANT_FLOOR, (case_id(case), share)


# ---------------------------------------------------------------------------------------------------------------- golden G21
def g21_decisions(wkey):
    """Per recorded decision of G21's network `wkey`: (chosen, float64 full-precision action values, the float64 emulation's)"""
    from oracle import crowd_oracle as orc

    pol = lc.g21_policy(wkey)
    w = lc.weights64(pol.model)
    out = []
    for c in (c for c in lc.g21()["decision"] if c["wkey"] == wkey):
        rot, rew = orc.lookahead(c["action_space"], c["next_humans"], c["obs"], c["robot"], float(c["dt"]))
        rot32 = rot.astype(F32)                                  # what the kernel is handed: float32 rows
        disc = np.array([float(c["gamma"]) ** (float(c["dt"]) * float(c["robot"][7]))])
        full = rew + disc * lc.forward64(w, lc.sort_rows(rot32.astype(np.float64)))
        out.append((int(c["chosen"]), full, lem.action_values(w, rot32[None], rew[None], disc)[0]))
    return out


G21_EMULATION_FLIPS = {"lstm1_13": 9, "lstm2_13": 5}          # of 48 recorded decisions each


@pytest.mark.parametrize("wkey", ["lstm1_13", "lstm2_13"])
def test_every_flip_of_the_emulation_on_g21_is_explained(wkey):
    """The criterion the GPU file holds the kernel to, met by the arithmetic alone: the float64 emulation's pick of every recorded decision;
    where it differs from the reference's `chosen`, gap <= 2 e (bf16_emulation.classify_flip).  The count is pinned, to be read beside the
    kernel's (HISTORY.md)."""
    ds = g21_decisions(wkey)
    flips = 0
    for k, (chosen, full, e64) in enumerate(ds):
        assert int(np.argmax(full)) == chosen, k                 # (the full-precision restatement picks the reference's action)
        pick = int(np.argmax(e64))
        if pick != chosen:
            flips += 1
            ok, gap, e = em.classify_flip(chosen, pick, full, e64)
            print(f"G21 {wkey} decision {k}: the emulation picks {pick}, the reference {chosen}: gap {gap:.3e}, e {e:.3e}")
            assert ok, (k, gap, e)
    print(f"G21 {wkey}, float64 emulation of the bf16 arithmetic: {flips} of {len(ds)} decisions flipped, all explained")
    assert len(ds) >= 20 and flips == G21_EMULATION_FLIPS[wkey]
