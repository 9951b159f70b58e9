"""The opt-in bf16 arithmetic of OM-LSTM-RL's decision (csrc/value_net_lstm_om_bf16.hip) restated on numpy arrays, as
lstm_bf16_emulation.py restates the narrow kernel's: the reference the kernel is held to.  Test code, independent of the kernel: it knows
the rounding points and the order of a chain, not the lanes.  numpy only.

The contract.  A row is `cols` rotated columns followed by C map columns.  The first layer that reads a row -- network 1's W_ih, network
2's mlp1 layer 0 -- is split by column:
  * float32, unrounded inputs, full weights: its rotated columns, weights [:, :cols]; and layer 0 of mlp, which reads the raw self state;
  * bf16 operands, float32 accumulation: its map columns -- weights [:, cols:] rounded to bf16 (nearest even), a map value rounded once,
    nearest even -- and everything the narrow bf16 kernel runs in bf16: W_hh, network 2's W_ih, the layers behind each chain's first;
  * rounded once when stored as a bf16 operand: h_t, an mlp1 / mlp activation behind bias and ReLU that a bf16 layer reads, mlp1's last output;
  * never rounded: c, the pre-activations, sigmoid and tanh, mlp's last output, rewards + discount * V;
  * order: a first-layer pre-activation is the bias (the gates': b_ih + b_hh summed in float32), then the rotated columns' part, then the
    map columns' part, for network 1's gates then W_hh's part.

  acc="f64"   every product and sum in float64, the roundings where the contract puts them
  acc="f32"   the same roundings with float32 products and sums, the parts of a chain added in the stated order: ONE float32 realisation
              of this arithmetic; the kernel is another.

`mutant` builds the arithmetics the contract excludes: "round_rotated" (the rotated columns rounded to bf16 before the first layer),
"maps_unrounded" (the map values stay float32), "map_weights_unrounded" (full weights on the map columns), "h_unrounded" (h stays float32
from step to step and into mlp), "c_rounded" (c rounded to bf16 after every step)."""
import numpy as np

import om_lstm_cases as olc
from bf16_emulation import bf16
from lstm_bf16_emulation import SELF_DIM, _indices, _sigmoid

MUTANTS = ("round_rotated", "maps_unrounded", "map_weights_unrounded", "h_unrounded", "c_rounded")


def forward(w, rows, cols, acc="f64", mutant=None):
    """The network on wide rows [..., n, cols + C] (float32 values) in the order given -> [...] (float64).  `w`: lstm_cases.weights64 of
    either network of an OM-LSTM-RL policy."""
    assert acc in ("f64", "f32") and mutant in (None,) + MUTANTS
    ft = np.float64 if acc == "f64" else np.float32
    rnd = lambda a: bf16(a).astype(ft)
    keep = lambda a: np.asarray(a, ft)
    rows = np.asarray(rows, np.float32)
    lead, n = rows.shape[:-2], rows.shape[-2]
    x = rows.reshape((-1,) + rows.shape[-2:]).astype(ft)
    xr = rnd(x[..., :cols]) if mutant == "round_rotated" else x[..., :cols]
    xm = x[..., cols:] if mutant == "maps_unrounded" else rnd(x[..., cols:])
    map_weights = keep if mutant == "map_weights_unrounded" else rnd
    hold = keep if mutant == "h_unrounded" else rnd

    def first_layer(b, wt):
        """bias, then the rotated columns' part, then the map columns' part: [rows, n, N]"""
        return (b.astype(ft) + xr @ keep(wt[:, :cols]).T) + xm @ map_weights(wt[:, cols:]).T

    def chain(v, prefix, round_last, first_done):
        idx = _indices(w, prefix)
        for j, i in enumerate(idx):
            if not (first_done and j == 0):
                wt, b = w[f"{prefix}.{i}.weight"], w[f"{prefix}.{i}.bias"].astype(ft)
                v = b + v @ (keep(wt) if j == 0 else rnd(wt)).T
            last = j == len(idx) - 1
            if not last:
                v = np.maximum(v, 0.0)                         # (a NaN stays a NaN: np.maximum propagates it)
            if not last or round_last:
                v = rnd(v)
        return v

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        net2 = any(k.startswith("mlp1.") for k in w)
        bias = (w["lstm.bias_ih_l0"].astype(np.float32) + w["lstm.bias_hh_l0"].astype(np.float32)).astype(ft)
        if net2:
            i0 = _indices(w, "mlp1")[0]
            seq = chain(first_layer(w[f"mlp1.{i0}.bias"], w[f"mlp1.{i0}.weight"]), "mlp1", True, True)
            xpart = bias + seq @ rnd(w["lstm.weight_ih_l0"]).T
        else:
            xpart = first_layer(bias, w["lstm.weight_ih_l0"])
        whh = rnd(w["lstm.weight_hh_l0"])
        H = whh.shape[1]
        h = np.zeros((x.shape[0], H), ft)
        c = np.zeros((x.shape[0], H), ft)
        for t in range(n):
            g = xpart[:, t] + h @ whh.T
            i, f, gg, o = _sigmoid(g[:, :H]), _sigmoid(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sigmoid(g[:, 3 * H:])
            c = f * c + i * gg
            if mutant == "c_rounded":
                c = rnd(c)
            h = hold(o * np.tanh(c))
        out = chain(np.concatenate([x[:, 0, :SELF_DIM], h], axis=1), "mlp", False, False)[:, 0]
    return out.astype(np.float64).reshape(lead)


def action_values(w, rot, maps, rew, disc, pairing, acc="f64", mutant=None, sort=True):
    """rewards + gamma^(dt v_pref) * network on rot [W, A, n, cols] beside maps [W, n, C] paired by `pairing` (om_lstm_cases.wide_rows: the
    order and the pairing are worked out on the unrounded float32 values), in the decision's order (`sort`) or as the rows lie: rew [W, A],
    disc [W] -> [W, A] float64 (acc="f32": the last step in float32 too)"""
    rot = np.asarray(rot, np.float32)
    rows = olc.wide_rows(rot, np.asarray(maps, np.float32), pairing, sort)
    net = forward(w, rows, rot.shape[-1], acc, mutant)
    if acc == "f32":
        return (np.asarray(rew, np.float32) + np.asarray(disc, np.float32)[:, None] * net.astype(np.float32)).astype(np.float64)
    return np.asarray(rew, np.float64) + np.asarray(disc, np.float64)[:, None] * net
