"""The opt-in bf16 arithmetic of OM-SARL's decision (csrc/value_net_om_bf16.hip) restated on numpy arrays, as
bf16_emulation.py restates the narrow kernel's and on that module's ``bf16``, ``_chain`` and ``_affine``: the reference the kernel is held
to.  Test code, independent of the kernel: it knows the rounding points and the order of a chain, not the lanes.

The contract.  A row is `cols` rotated columns followed by C map columns.  mlp1's layer 0 is split by column:
  * its rotated columns: full-precision weights [:, :cols], unrounded inputs;
  * its map columns: weights [:, cols:] rounded to bf16 (nearest even), a map value rounded once, nearest even;
  * a pre-activation is the bias, then the rotated columns' part, then the map columns' part; then the ReLU; then it is rounded once as the
    operand of the next layer.
Everything else is bf16_emulation's contract: every later layer outside mlp3 in bf16 with float32 accumulation, mlp3 float32 on the
unrounded self state (the first six columns of the first human's row), what a reduction consumes not rounded, the crowd mean summed in
human order from the rounded mlp1 outputs and rounded once, the masked softmax without maximum subtraction, the weighted sum and
rewards + discount * V unrounded.

  acc="f64"   every product and sum in float64, the roundings where the contract puts them
  acc="f32"   the same roundings with float32 accumulation (bf16_emulation's: torch CPU matmuls, numpy float32 reductions), the parts of
              the first layer added in the stated order: ONE float32 realisation of this arithmetic; the kernel is another.

`mutant` builds the arithmetics the contract excludes: "round_rotated" (the rotated columns rounded to bf16 before layer 0),
"map_weights_unrounded" (full weights on the map columns), "truncate" (round toward zero instead of to nearest even)."""
import numpy as np

from bf16_emulation import _affine, _chain, _indices, bf16

MUTANTS = ("round_rotated", "map_weights_unrounded", "truncate")


def network(rot, maps, w, with_global=True, acc="f64", mutant=None):
    """The network's output per (world, action): rot [W, A, n, cols] beside maps [W, n, C] (float32 values; one map row serves the A
    actions of its world) -> [W, A].  w: the state_dict as float64 arrays (test_value_policy_cpu.numpy_weights); mlp1's first weight is
    [N, cols + C]."""
    assert acc in ("f64", "f32") and mutant in (None,) + MUTANTS
    ft = np.float64 if acc == "f64" else np.float32
    rnd = lambda a: bf16(a, truncate=mutant == "truncate").astype(ft)
    rot = np.asarray(rot, np.float32)
    cols = rot.shape[-1]
    x = rot.astype(ft)
    xr = rnd(x) if mutant == "round_rotated" else x
    xm = rnd(np.broadcast_to(np.asarray(maps, np.float32)[:, None], rot.shape[:-1] + np.shape(maps)[-1:]))
    first, *later = _indices(w, "mlp1")
    wt, b = w[f"mlp1.{first}.weight"], w[f"mlp1.{first}.bias"]
    assert wt.shape[1] == cols + xm.shape[-1]
    wm = wt[:, cols:] if mutant == "map_weights_unrounded" else rnd(wt[:, cols:])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pre = _affine(xr, np.ascontiguousarray(wt[:, :cols]), b, acc)      # the bias starts the sum, then the rotated columns
        pre = pre + (xm @ wm.T.astype(ft)).astype(ft)         # then the map columns
        m1 = rnd(np.maximum(pre, 0.0))                        # (mlp1's ReLU follows its last layer too: cadrl.py mlp(last_relu=True))
        rest = {k: v for k, v in w.items() if k.startswith("mlp1.") and int(k.split(".")[1]) in later}
        m1 = _chain(m1, rest, "mlp1", acc, rnd, last_relu=True, round_last=True)
        # from here on bf16_emulation.network's SARL branch, word for word
        m2 = _chain(m1, w, "mlp2", acc, rnd)
        a_in = m1
        if with_global:
            mean = np.zeros(m1.shape[:-2] + m1.shape[-1:], ft)
            for j in range(m1.shape[-2]):                     # in human order
                mean = mean + m1[..., j, :]
            g = rnd(mean / ft(m1.shape[-2]))
            a_in = np.concatenate([m1, np.broadcast_to(g[..., None, :], m1.shape)], axis=-1)
        s = _chain(a_in, w, "attention", acc, rnd)[..., 0]
        e = (np.exp(s) * (s != 0)).astype(ft)
        wts = e / e.sum(axis=-1, keepdims=True)
        feat = (wts[..., None] * m2).sum(axis=-2)
        joint = np.concatenate([x[..., 0, :6], feat], axis=-1)
        return _chain(joint, w, "mlp3", acc, rnd, all_f32=True)[..., 0]


def action_values(rot, maps, rew, disc, w, with_global=True, acc="f64", mutant=None):
    """rewards + gamma^(dt v_pref) * network: rew [W, A], disc [W] -> [W, A] float64 (acc="f32": computed in float32)"""
    net = network(rot, maps, w, with_global, acc, mutant)
    if acc == "f32":
        return (np.asarray(rew, np.float32) + np.asarray(disc, np.float32)[:, None] * net.astype(np.float32)).astype(np.float64)
    return np.asarray(rew, np.float64) + np.asarray(disc, np.float64)[:, None] * net


def wide_rows(rot, maps):
    """[W, A, n, cols + C]: every (world, action, human)'s rotated columns beside that (world, human)'s map"""
    rot, maps = np.asarray(rot), np.asarray(maps)
    return np.concatenate([rot, np.broadcast_to(maps[:, None], rot.shape[:-1] + maps.shape[-1:]).astype(rot.dtype)], axis=-1)
