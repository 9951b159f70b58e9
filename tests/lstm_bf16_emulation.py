"""The opt-in bf16 arithmetic of LSTM-RL's decision (csrc/value_net_lstm_bf16.hip) restated on numpy arrays from the published
architecture, as lstm_cases.forward64 restates the float32 one and bf16_emulation.py the feed-forward bf16 one: the reference the kernel is
held to.  Test code, independent of the kernel: it knows the rounding points, not the lanes.  numpy only.

The contract:
  * float32 layers (full-precision weights, unrounded inputs): network 1's W_ih on the raw row x_t, network 2's mlp1 layer 0, layer 0 of mlp
    (it reads the raw self state);
  * bf16 layers (weights rounded to bf16, nearest even; float32 biases): W_hh in both networks, network 2's W_ih, every mlp1 and mlp layer
    behind the first;
  * rounded once, nearest even, when stored as a bf16 operand: h_t after o * tanh(c) -- the one rounded value is the next step's operand and
    what mlp reads as h_n --, an mlp1 / mlp activation after bias and ReLU when a bf16 layer reads it, mlp1's last output (no ReLU);
  * never rounded: c, the gate pre-activations, sigmoid and tanh, mlp's last output, rewards + discount * V;
  * the bias is b_ih + b_hh summed in float32; a gate pre-activation is the bias, then the x part, then the h part.

  acc="f64"   every product and sum in float64, the roundings where the contract puts them
  acc="f32"   the same roundings with float32 products and sums (numpy float32 matmul, sigmoid and tanh): ONE float32 realisation of this
              arithmetic; the kernel is another.

`mutant` builds the arithmetics the contract excludes: "truncate" (toward zero instead of nearest even), "h_unrounded" (h stays float32 /
float64 from step to step and into mlp), "round_inputs" (x_t rounded before the gates / mlp1 layer 0), "round_first_layers" (bf16 weights in
the three float32 layers)."""
import numpy as np

from bf16_emulation import bf16

MUTANTS = ("truncate", "h_unrounded", "round_inputs", "round_first_layers")
SELF_DIM = 6


def _indices(w, prefix):
    return sorted({int(k.split(".")[1]) for k in w if k.startswith(prefix + ".")})


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def forward(w, rows, acc="f64", mutant=None):
    """The network on rows [..., n, cols] (float32 values) in the order given -> [...] (float64).  `w`: lstm_cases.weights64 of either network."""
    assert acc in ("f64", "f32") and mutant in (None,) + MUTANTS
    ft = np.float64 if acc == "f64" else np.float32
    rnd = lambda a: bf16(a, truncate=mutant == "truncate").astype(ft)
    first = rnd if mutant == "round_first_layers" else (lambda a: np.asarray(a, ft))      # the weights of a float32 layer
    hold = (lambda a: a) if mutant == "h_unrounded" else rnd
    rows = np.asarray(rows, np.float32)
    lead, n = rows.shape[:-2], rows.shape[-2]
    x = rows.reshape((-1,) + rows.shape[-2:]).astype(ft)
    x_in = rnd(x) if mutant == "round_inputs" else x

    def chain(v, prefix, round_last):
        idx = _indices(w, prefix)
        for j, i in enumerate(idx):
            wt, b = w[f"{prefix}.{i}.weight"], w[f"{prefix}.{i}.bias"].astype(ft)
            v = b + v @ (first(wt) if j == 0 else rnd(wt)).T
            last = j == len(idx) - 1
            if not last:
                v = np.maximum(v, 0.0)                         # (a NaN stays a NaN: np.maximum propagates it)
            if not last or round_last:
                v = rnd(v)
        return v

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        net2 = any(k.startswith("mlp1.") for k in w)
        seq = chain(x_in, "mlp1", True) if net2 else x_in
        wih = rnd(w["lstm.weight_ih_l0"]) if net2 else first(w["lstm.weight_ih_l0"])
        whh = rnd(w["lstm.weight_hh_l0"])
        bias = (w["lstm.bias_ih_l0"].astype(np.float32) + w["lstm.bias_hh_l0"].astype(np.float32)).astype(ft)
        H = whh.shape[1]
        h = np.zeros((x.shape[0], H), ft)
        c = np.zeros((x.shape[0], H), ft)
        for t in range(n):
            g = (bias + seq[:, t] @ wih.T) + h @ whh.T
            i, f, gg, o = _sigmoid(g[:, :H]), _sigmoid(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sigmoid(g[:, 3 * H:])
            c = f * c + i * gg
            h = hold(o * np.tanh(c))
        out = chain(np.concatenate([x[:, 0, :SELF_DIM], h], axis=1), "mlp", False)[:, 0]
    return out.astype(np.float64).reshape(lead)


def action_values(w, rot, rew, disc, acc="f64", mutant=None, sort=True):
    """rewards + gamma^(dt v_pref) * network on rot [W, A, n, cols] in the decision's order (`sort`) or as the rows lie: rew [W, A], disc [W]
    -> [W, A] float64 (acc="f32": the last step in float32 too)"""
    import lstm_cases as lc

    rows = np.asarray(rot, np.float32)
    rows = lc.sort_rows(rows) if sort else rows
    net = forward(w, rows, acc, mutant)
    if acc == "f32":
        return (np.asarray(rew, np.float32) + np.asarray(disc, np.float32)[:, None] * net.astype(np.float32)).astype(np.float64)
    return np.asarray(rew, np.float64) + np.asarray(disc, np.float64)[:, None] * net
