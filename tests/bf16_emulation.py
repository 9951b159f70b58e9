"""The opt-in bf16 arithmetic of the value-network decision (csrc/value_net_bf16.hip) restated on numpy arrays: the reference
the kernel is held to.  Test code, independent of the kernel: it knows the rounding points, not the lanes.

  acc="f64"   every product and sum in float64, the roundings to bf16 where the contract puts them
  acc="f32"   the same roundings with float32 accumulation: a torch CPU matmul on the rounded operands, the reductions in numpy float32.
              Its distance from the float64 mode is what ONE float32 realisation of this arithmetic loses; the kernel is another.

The contract, as the issue states it:
  * float32 layers: CADRL value_network layer 0, SARL mlp1 layer 0, all of mlp3 (full-precision weights, unrounded inputs);
  * every other layer: weights rounded to bf16 (nearest even), float32 biases, operands that were rounded when they were stored;
  * an activation is rounded once, after bias and ReLU, when it is the operand of a bf16 layer; what a reduction consumes -- attention
    scores, mlp2's features, CADRL's per-human value -- is not rounded;
  * with_global_state: the mean of the rounded mlp1 outputs, summed in human order, divided by n, rounded once;
  * masked softmax exp(s) * (s != 0) without maximum subtraction, minimum, weighted sum, rewards + discount * out: unrounded.

`mutant` builds the arithmetics the contract excludes: "round_reductions" (the reduction inputs rounded too), "round_inputs" (the rows
rounded before layer 0), "truncate" (round toward zero instead of to nearest even)."""
import numpy as np
import torch

MUTANTS = ("round_reductions", "round_inputs", "truncate")


def bf16(x, truncate=False):
    """x (float64 or float32 values) rounded to bfloat16 -- 8 significant bits, float32's exponent range -- returned as float64.  Nearest even
    (np.rint) or toward zero; NaN and +-inf pass, values beyond bf16's largest finite one become +-inf, the subnormal grid is 2^-133."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        m, e = np.frexp(x)                                    # x = m 2^e, 0.5 <= |m| < 1
        e = np.maximum(e, -125)                               # below 2^-126 the grid stops shrinking
        q = np.ldexp(np.where(np.isfinite(x), x, 0.0), 8 - e)
        q = np.trunc(q) if truncate else np.rint(q)
        out = np.ldexp(q, e - 8)
        out = np.where(np.abs(out) >= 2.0 ** 128, np.copysign(np.inf, out), out)
    return np.where(np.isfinite(x), out, x)


def _indices(w, prefix):
    return sorted({int(k[len(prefix) + 1:].split(".")[0]) for k in w if k.startswith(prefix + ".")})


def _affine(x, wt, b, acc):
    """x [..., K] @ wt [N, K]^T + b with the bias starting the sum"""
    if acc == "f64":
        return x @ wt.T + b
    lead = x.shape[:-1]
    with torch.no_grad():
        y = torch.addmm(torch.from_numpy(np.array(b, np.float32)), torch.from_numpy(np.array(x, np.float32).reshape(-1, x.shape[-1])),
                        torch.from_numpy(np.ascontiguousarray(wt.T, np.float32)))
    return y.numpy().reshape(lead + (wt.shape[0],))


def _chain(x, w, prefix, acc, rnd, *, first_f32=False, all_f32=False, last_relu=False, round_last=False):
    """cadrl.py mlp() with the contract's roundings.  first_f32 / all_f32: which layers keep full-precision weights; round_last: the
    chain's output is itself the operand of a bf16 layer (mlp1).  The input of a bf16 layer arrives rounded."""
    idx = _indices(w, prefix)
    for j, i in enumerate(idx):
        wt, b = w[f"{prefix}.{i}.weight"], w[f"{prefix}.{i}.bias"]
        f32_layer = all_f32 or (first_f32 and j == 0)
        x = _affine(x, wt if f32_layer else rnd(wt), b, acc)
        last = j == len(idx) - 1
        if not last or last_relu:
            x = np.maximum(x, 0.0)                            # (a NaN stays a NaN, -inf becomes 0: the kernel's v < 0 ? 0 : v)
        if not all_f32 and (not last or round_last):
            x = rnd(x)
    return x


def network(name, rot, w, with_global=True, acc="f64", mutant=None):
    """The network's output per (world, action): rot [..., N, 13 | 15] (float32 values) -> [...].  name "cadrl" | "sarl"; w: the state_dict as
    float64 arrays (test_value_policy_cpu.numpy_weights)."""
    assert acc in ("f64", "f32") and mutant in (None,) + MUTANTS
    ft = np.float64 if acc == "f64" else np.float32
    rnd = lambda a: bf16(a, truncate=mutant == "truncate").astype(ft)
    red = rnd if mutant == "round_reductions" else (lambda a: a)
    x = np.asarray(rot, ft)
    if mutant == "round_inputs":
        x = rnd(x)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if name == "cadrl":
            return red(_chain(x, w, "value_network", acc, rnd, first_f32=True)[..., 0]).min(axis=-1)
        m1 = _chain(x, w, "mlp1", acc, rnd, first_f32=True, last_relu=True, round_last=True)
        m2 = red(_chain(m1, w, "mlp2", acc, rnd))
        a_in = m1
        if with_global:
            mean = np.zeros(m1.shape[:-2] + m1.shape[-1:], ft)
            for j in range(m1.shape[-2]):                     # in human order
                mean = mean + m1[..., j, :]
            g = rnd(mean / ft(m1.shape[-2]))
            a_in = np.concatenate([m1, np.broadcast_to(g[..., None, :], m1.shape)], axis=-1)
        s = red(_chain(a_in, w, "attention", acc, rnd)[..., 0])
        e = (np.exp(s) * (s != 0)).astype(ft)
        wts = e / e.sum(axis=-1, keepdims=True)
        feat = (wts[..., None] * m2).sum(axis=-2)
        joint = np.concatenate([np.asarray(rot, ft)[..., 0, :6], feat], axis=-1)
        return _chain(joint, w, "mlp3", acc, rnd, all_f32=True)[..., 0]


def action_values(name, rot, rew, disc, w, with_global=True, acc="f64", mutant=None):
    """rewards + gamma^(dt v_pref) * network: rew [W, A], disc [W] -> [W, A] float64 (acc="f32": computed in float32)"""
    net = network(name, rot, w, with_global, acc, mutant)
    if acc == "f32":
        return (np.asarray(rew, np.float32) + np.asarray(disc, np.float32)[:, None] * net.astype(np.float32)).astype(np.float64)
    return np.asarray(rew, np.float64) + np.asarray(disc, np.float64)[:, None] * net


def full_precision(name, rot, w, with_global=True):
    """The float64 network with full-precision weights and no rounding (test_policy_seam.VALUE, and SARL without the crowd mean)"""
    from test_policy_seam import VALUE, _mlp

    rot = np.asarray(rot, np.float64)
    if name == "cadrl" or with_global:
        return VALUE[name](rot, w)
    m1 = _mlp(rot, w, "mlp1", last_relu=True)
    s = _mlp(m1, w, "attention")[..., 0]
    e = np.exp(s) * (s != 0)
    feat = ((e / e.sum(-1, keepdims=True))[..., None] * _mlp(m1, w, "mlp2")).sum(-2)
    return _mlp(np.concatenate([rot[..., 0, :6], feat], -1), w, "mlp3")[..., 0]


def classify_flip(chosen_ref, chosen_got, full64, emu64):
    """The issue's criterion for a decision whose pick differs from the reference's: explained when gap <= 2 e, gap = the float64
    full-precision-weight value difference between the reference's action and the other pick, e = the worst |emulation - float64
    full-precision value| over the decision's actions.  full64, emu64: [A] action values.  Returns (explained, gap, e)."""
    gap = float(abs(full64[chosen_ref] - full64[chosen_got]))
    e = float(np.max(np.abs(np.asarray(emu64) - np.asarray(full64))))
    return gap <= 2.0 * e, gap, e
