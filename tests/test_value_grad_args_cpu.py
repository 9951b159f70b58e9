"""The refusals of the training entries of the four value-network families (feed-forward, with map columns, recurrent, recurrent with map
columns), pinned message for message: cs_value_net_grad_sizes, cs_value_net_loss_grad, cs_value_net_train_step, cs_value_net_blob_index and
cs_value_net_pack_device with their `_lstm` / `_om` names.  Every check of these entries runs on the host before any launch, so no GPU is
needed: each call here is refused.  The pointers given are host addresses of a small array, never read: a refusal comes before any use of
them.  The networks are golden G23's widths (tests/value_grad_cases.py), the LDS case the reference's widths with 192 map columns."""
import ctypes as C

import numpy as np
import pytest

import lstm_grad_cases as lg
import value_grad_cases as vg

ENTRIES = ("grad_sizes", "loss_grad", "train_step", "blob_index", "pack_device")


def _sarl(w):
    return [1, len(w["mlp1"]), *w["mlp1"], len(w["mlp2"]), *w["mlp2"], len(w["attention"]), *w["attention"], len(w["mlp3"]), *w["mlp3"]]


def _lstm(hidden, mlp1, mlp):
    return [hidden, len(mlp1), *mlp1, len(mlp), *mlp]


# family -> (the entries' infix, takes `kind`, takes om_cols, dims at G23's widths, dims at the reference's widths)
FAMILIES = {
    "feed_forward": ("", True, False, _sarl(vg.SARL_WIDTHS), _sarl(vg.SARL_FULL)),
    "mapped": ("", True, True, _sarl(vg.SARL_WIDTHS), _sarl(vg.SARL_FULL)),
    "recurrent": ("_lstm", False, False, _lstm(lg.H_SMALL, lg.MLP1_SMALL, lg.MLP_SMALL), _lstm(lg.H_FULL, lg.MLP1_FULL, lg.MLP_FULL)),
    "recurrent_mapped": ("_lstm", False, True, _lstm(lg.H_SMALL, lg.MLP1_SMALL, lg.MLP_SMALL), _lstm(lg.H_FULL, lg.MLP1_FULL, lg.MLP_FULL)),
}
CADRL_DIMS = [len(vg.CADRL_WIDTHS), *vg.CADRL_WIDTHS]


def _name(family, entry):
    infix, _, om, _, _ = FAMILIES[family]
    tail = "_om" if om else ""
    return f"cs_value_net_pack{infix}{tail}_device" if entry == "pack_device" else f"cs_value_net_{entry}{infix}{tail}"


class _Call:
    """One call of a family's entry: the good arguments of a minibatch of 7 samples of 5 humans on rows of 13 (+ 18) columns -- the sizes
    asked of the library's host entries --, any of them replaced by `over`."""

    def __init__(self, family, kind=1, dims=None, om_cols=18, B=7, n=5):
        from social_navigation_pyenvs_amd import _lib

        self.lib, self.family = _lib.load(), family
        infix, takes_kind, self.om, small, _ = FAMILIES[family]
        self.dims = np.array(small if dims is None else dims, np.int32)
        self.lead = ((kind,) if takes_kind else ()) + (self.dims.ctypes.data, len(self.dims))
        self.cols, self.om_cols = 13, om_cols
        self.held = np.zeros(4, np.float64)
        ptr = self.held.ctypes.data
        n_params, n_scratch, n_blob = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        _lib.check(getattr(self.lib, _name(family, "grad_sizes"))(*self.lead, *self.width(), B, n, C.byref(n_params), C.byref(n_scratch)))
        pack = getattr(self.lib, f"cs_value_net_pack{infix}{'_om' if self.om else ''}")
        _lib.check(pack(*self.lead, *self.width(), None, None, C.byref(n_blob)))
        self.good = dict(B=B, n=n, cols=self.cols, om_cols=om_cols, weights=ptr, n_weights=n_blob.value, params=ptr, n_params=n_params.value,
                         momentum=ptr, n_momentum=n_params.value, lr=0.01, mu=0.9, rows=ptr, targets=ptr, grad=ptr, loss=ptr, loss_sum=None,
                         values=None, scratch=ptr, n_scratch=n_scratch.value, out_params=ptr, out_scratch=ptr + 8, index=ptr, blob=ptr)

    def width(self, a=None):
        a = a or dict(cols=self.cols, om_cols=self.om_cols)
        return (a["cols"], a["om_cols"]) if self.om else (a["cols"],)

    def __call__(self, entry, **over):
        """(status, message) of the entry with `over` in the place of the good arguments"""
        a = dict(self.good, **over)
        batch = (a["B"], a["n"], *self.width(a), a["rows"], a["targets"], a["grad"], a["loss"])
        tail = (a["values"], a["scratch"], a["n_scratch"], None)
        args = {"grad_sizes": (*self.width(a), a["B"], a["n"], a["out_params"], a["out_scratch"]),
                "loss_grad": (a["weights"], a["n_weights"], a["params"], a["n_params"], *batch, *tail),
                "train_step": (a["weights"], a["n_weights"], a["params"], a["n_params"], a["momentum"], a["n_momentum"], a["lr"], a["mu"], *batch,
                               a["loss_sum"], *tail),
                "blob_index": (*self.width(a), a["index"], a["n_params"]),
                "pack_device": (*self.width(a), a["params"], a["n_params"], a["blob"], a["n_weights"], None)}[entry]
        rc = getattr(self.lib, _name(self.family, entry))(*self.lead, *args)
        return rc, self.lib.cs_last_error().decode()


NULL = "null argument"
LAUNCHES = ("loss_grad", "train_step")
SIZED = ("grad_sizes",) + LAUNCHES


def _refusals(family):
    """[(what, the entries it is driven through, the arguments replaced, the whole message)] of `family`"""
    infix, _, om, _, _ = FAMILIES[family]
    pack, sizes = f"(cs_value_net_pack{infix})", f"(cs_value_net_grad_sizes{infix})"
    flat = f"the flat parameters do not have the size of this network {sizes}"
    blob = f"the weight blob does not have the size of this network {pack}"
    rows = [("B = 0", SIZED, dict(B=0), "B must be positive"),
            ("n = 0", SIZED, dict(n=0), "n must be at least 1: a value network needs a human to look at"),
            ("B * n", SIZED, dict(B=1 << 27, n=1), "B * n is too large")]
    if infix:
        rows.append(("n = 129", SIZED, dict(n=129), "cs_value_net_loss_grad_lstm takes at most 128 humans a sample (CS_VN_LSTM_MAX_N)"))
    if om:
        rows.append(("om_cols = 0", ENTRIES, dict(om_cols=0), "om_cols must be at least 1"))
    rows += [(f"null {name}", ("grad_sizes",), {name: None}, NULL) for name in ("out_params", "out_scratch")]
    rows += [(f"null {name}", LAUNCHES, {name: None}, NULL) for name in ("weights", "params", "rows", "targets", "grad", "loss", "scratch")]
    rows += [("null momentum", ("train_step",), dict(momentum=None), NULL), ("null index", ("blob_index",), dict(index=None), NULL),
             ("null params", ("pack_device",), dict(params=None), NULL), ("null blob", ("pack_device",), dict(blob=None), NULL)]
    rows += [("blob size", LAUNCHES + ("pack_device",), "n_weights", blob), ("flat size", LAUNCHES + ("blob_index", "pack_device"), "n_params", flat),
             ("scratch short", LAUNCHES, "n_scratch", f"the scratch is too small for this minibatch {sizes}"),
             ("momentum size", ("train_step",), "n_momentum", "the momentum buffer does not have the size of the flat parameters")]
    for name, message in (("lr", "lr must be finite and at least 0"), ("mu", "momentum must be finite and at least 0")):
        rows += [(f"{name} {value}", ("train_step",), {name: value}, message) for value in (-1.0, float("nan"))]
    return rows


CASES = [(family, *row) for family in FAMILIES for row in _refusals(family)]


@pytest.fixture(scope="module")
def calls():
    return {family: _Call(family) for family in FAMILIES}


@pytest.mark.parametrize("family,what,entries,over,message", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_every_refusal_of_the_training_entries_has_its_message(calls, family, what, entries, over, message):
    from social_navigation_pyenvs_amd import _lib

    call = calls[family]
    if isinstance(over, str):       # a size one short of the good one
        over = {over: call.good[over] - 1}
    for entry in entries:
        assert call(entry, **over) == (_lib.CS_ERR_ARG, message), (family, entry, what)


@pytest.mark.parametrize("entry", SIZED)
def test_cadrl_takes_one_human_a_sample(entry):
    from social_navigation_pyenvs_amd import _lib

    call = _Call("feed_forward", kind=0, dims=CADRL_DIMS, n=1)
    assert call(entry, n=2) == (_lib.CS_ERR_ARG, "CADRL's trainer stores one human's row per sample: n must be 1")


# the reference's widths with 192 map columns: neither family's tile fits the LDS
LDS = {"mapped": "the activations and gradients of a tile of this network (rows of 13 + 192 columns: 176720 bytes) do not fit the 160 KiB of LDS",
       "recurrent_mapped": "the activations and gradients of a tile of this network (rows of 13 + 192 columns, H = 50: 179328 bytes) do not fit the "
                           "160 KiB of LDS"}


@pytest.mark.parametrize("family", sorted(LDS))
def test_a_tile_that_does_not_fit_the_lds_is_refused_with_its_widths(family):
    from social_navigation_pyenvs_amd import _lib

    call = _Call(family)        # (the pointers and sizes of the small network: the refusal comes before them)
    call.dims = np.array(FAMILIES[family][4], np.int32)
    call.lead = call.lead[:-2] + (call.dims.ctypes.data, len(call.dims))
    for entry in SIZED:
        assert call(entry, om_cols=192) == (_lib.CS_ERR_ARG, LDS[family]), (family, entry)
