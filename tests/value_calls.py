"""What the GPU suites of the value networks share (test_gpu_value_om / _lstm / _state / _worlds / _families): uploads, the current stream,
the bitwise comparison, and the library calls of value_net on host arrays.  A plain helper module, not a conftest."""
import numpy as np

F32 = np.float32
GAMMA, DT = 0.9, 0.25
GUARD = (5, 8)          # floats before / behind an output: it starts 4 bytes behind a 16-byte boundary


def _up(a, dtype=None):
    """A host array on the device; a tensor stays where it is"""
    import torch

    if torch.is_tensor(a):
        return a if dtype is None else a.to(dtype)
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def lookahead_call(acts, nxt, cur, rob, dt=DT):
    """value_net.lookahead on host arrays: (rotated [W, A, n, cols], rewards [W, A]) device tensors, synchronised"""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    out = value_net.lookahead(_up(acts), _up(nxt), _up(cur), _up(rob), dt, _stream())
    torch.cuda.synchronize()
    return out


def decide_call(dnet, rot, rew, acts, rob, extra=None, gamma=GAMMA, dt=DT, override=None):
    """The decide entry of `dnet`'s family -- cs_value_net_decide, cs_value_net_decide_om (`extra`: the maps, a device tensor [W, n,
    om_cols]) or cs_value_net_decide_lstm (`extra`: sorted_by_distance) -- on rot [W, A, n, cols], rew [W, A], acts [A, 2], rob [W, 9],
    host arrays or device tensors; override: int32 [W] or None.  (values [W, A], choice [W], action [W, 2]) numpy.  The outputs are NaN- /
    -5-filled before: every element must be written."""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    W, A, n, _ = rot.shape
    vals = torch.full((W, A), np.nan, device="cuda")
    pick = torch.full((W,), -5, dtype=torch.int32, device="cuda")
    act = torch.full((W, 2), np.nan, device="cuda")
    d_rot, d_rew, d_acts, d_rob = _up(rot, torch.float32), _up(rew, torch.float32), _up(acts, torch.float32), _up(rob, torch.float32)
    d_ovr = None if override is None else _up(override, torch.int32)
    common = (d_rew.data_ptr(), d_acts.data_ptr(), d_rob.data_ptr(), d_rob.shape[1], gamma, dt, None if d_ovr is None else d_ovr.data_ptr(),
              vals.data_ptr(), pick.data_ptr(), act.data_ptr(), _stream())
    if dnet.family is value_net.MAPPED:
        assert tuple(extra.shape) == (W, n, dnet.om_cols) and extra.is_contiguous()
        value_net.decide_om(dnet, W, A, n, d_rot.data_ptr(), extra.data_ptr(), *common)
    elif dnet.family is value_net.RECURRENT:
        value_net.decide_lstm(dnet, W, A, n, extra, d_rot.data_ptr(), *common)
    else:
        assert extra is None
        value_net.decide(dnet, W, A, n, d_rot.data_ptr(), *common)
    torch.cuda.synchronize()
    return vals.cpu().numpy(), pick.cpu().numpy(), act.cpu().numpy()


def state_call(dnet, cur, rob, rewards=None, dt=0.0, rows=True, gamma=GAMMA):
    """cs_value_net_state on host arrays: (values [W], rows [W, n, cols] or None) as numpy.  The rows are written between guard floats,
    which must come back untouched: the output is dense, nothing is stored for the tile's padded columns or rows."""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    d_cur, d_rob = _up(cur), _up(rob)
    W, n, headed = cur.shape[0], cur.shape[1], cur.shape[2] == 7
    cols = 15 if headed else 13
    vals = torch.full((W,), np.nan, device="cuda")
    flat = torch.full((GUARD[0] + W * n * cols + GUARD[1],), -77.0, device="cuda") if rows else None
    d_rew = None if rewards is None else _up(rewards)
    value_net.state_values(dnet, W, n, headed, d_cur.data_ptr(), d_rob.data_ptr(), rob.shape[1], None if d_rew is None else d_rew.data_ptr(), gamma, dt,
                           None if flat is None else flat.data_ptr() + 4 * GUARD[0], vals.data_ptr(), _stream())
    torch.cuda.synchronize()
    out = None
    if rows:
        flat = flat.cpu().numpy()
        assert np.all(flat[:GUARD[0]] == F32(-77.0)) and np.all(flat[-GUARD[1]:] == F32(-77.0)), "a store outside [W, n, cols]"
        out = flat[GUARD[0]:-GUARD[1]].reshape(W, n, cols)
    return vals.cpu().numpy(), out
