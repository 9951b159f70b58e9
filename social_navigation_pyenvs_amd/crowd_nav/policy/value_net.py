"""The seam between the value-based policies (CADRL, SARL) and the fused decision kernel (cs_value_net_decide, csrc/value_net.hip).

``describe(policy)`` turns a policy's torch module into the kernel's layer description, ``DeviceNet`` keeps the packed weight blob on the
GPU and repacks it only when a parameter changed (the tensors' version counters), ``decide`` is the one library call of a decision and
``decide_for_worlds`` the whole sequence from the worlds' rows that CADRL's ``predict`` (W = 1) and the batched Gym's ``act_device`` share.
There is no host implementation of the decision: without the library or a GPU these raise.

Two arithmetics: "f32", the default, and the opt-in "bf16" (cs_value_net_decide_bf16, csrc/value_net_bf16.hip) with its
own blob; a policy chooses with ``set_decision_precision``.  Two inputs: "tensor", the default (cs_lookahead's rows in HBM), and the opt-in
"fused" (``decide_worlds``: cs_value_net_decide_worlds generates the rows in the kernel, float32 only); ``set_decision_input``.

Which entries a network uses, with which arguments, and which modes it may run in is stated once, in the four rows of ``Family``
(DESIGN.md 4.5): FEED_FORWARD (CADRL, SARL), MAPPED (OM-SARL: every human's row widened by its occupancy map, ``om_cols`` > 0), RECURRENT
(LSTM-RL; ``describe`` answers CS_VN_LSTM -- a tag of this module, not a `kind` of the C entries) and RECURRENT_MAPPED (OM-LSTM-RL, whose
entries also take ``map_order``, MAP_ORDERS: "reference" pairs a step's row with the map at that place of action 0's order, as the
reference's serial decision does, "own" with its own map, as ``transform`` stores them).  A ``DeviceNet`` holds its row, a policy class
names its own, and ``pack``, ``decide_rows``, ``decide_for_worlds``, ``state_values_for_worlds`` and ``check_mode`` ask it; ``decide_om``,
``decide_lstm`` and ``decide_lstm_om`` are ``decide_rows`` for one family each.  A family with maps runs lookahead -> ``occupancy_maps``
(cs_occupancy_maps, the next humans) -> its decide entry.

The two recurrent rows also state an arithmetic of their own (``Family.own``, an ``OwnArithmetic``): the opt-in bf16 decision of
csrc/value_net_lstm_bf16.hip and csrc/value_net_lstm_om_bf16.hip, under names apart from ``precision`` so that what ``set_decision_precision``,
``check_decision_input`` and ``pack`` refuse for a recurrent net stays refused.  The row names the blob's key on a ``DeviceNet``
(RECURRENT_BF16, MAPPED_RECURRENT_BF16), the pack and decide entries and the word of its names: ``check_<word>_precision``,
``DeviceNet.refresh_<word>``, ``decide_for_worlds(..., <word>_precision="bf16")`` and a policy's ``set_<word>_precision`` (``LstmRL``: recurrent,
``OMLstmRL``: mapped).  ``pack_lstm_bf16`` / ``pack_lstm_om_bf16`` and ``decide_lstm_bf16`` / ``decide_lstm_om_bf16`` are the public names.

RECURRENT also states an input of its own (``Family.worlds``; RECURRENT_INPUTS, ``check_recurrent_input``): "fused" decides from the worlds' own
rows in either recurrent precision (cs_value_net_decide_lstm_worlds[_bf16], csrc/value_net_lstm_worlds.hip: the recurrent kernels generate
their rows, no look-ahead tensor), bit for bit the tensor path -- ``decide_lstm_worlds`` / ``decide_lstm_worlds_bf16``,
``decide_for_worlds(..., recurrent_input="fused")``, a policy's ``set_recurrent_input``.  A name apart from ``set_decision_input``, whose
"fused" keeps refusing a recurrent net with the sentence it has.

MAPPED states OM-SARL's opt-in bf16 decision (csrc/value_net_om_bf16.hip: mlp1's layer 0 split between float32 rotated columns and bf16 map
columns, everything behind it the feed-forward bf16 arithmetic) the same way, as an ``OwnArithmetic`` with the word "wide" -- in the row's
``wide`` field, not in ``own``: ``MAPPED.own`` is None and ``MAPPED.modes`` holds ("tensor", "f32") alone, so that ``set_decision_precision("bf16")``,
``set_decision_input("fused")`` and ``check_mapped_precision("bf16", MAPPED)`` keep refusing an OM-SARL network with the sentences they have.
``own_arithmetic(family)`` is the one place that answers which of the two a row states.  Its names: WIDE_PRECISIONS, the key WIDE_BF16,
``check_wide_precision``, ``DeviceNet.refresh_wide``, ``decide_for_worlds(..., wide_precision="bf16")``, ``OMSARL.set_wide_precision``,
``pack_om_bf16`` and ``decide_om_bf16``.

``state_values`` is the training side (cs_value_net_state, csrc/value_net_state.hip): the network on the worlds' current state -- the
rotated joint states a trainer stores and V(s) or the target reward + gamma^(dt * v_pref) * V(s) --, float32 whatever the policy's modes;
``state_values_for_worlds`` is that for every family.

The optimisation step has kernels too, for all four families (csrc/value_net_grad.hip: CADRL, SARL and OM-SARL; csrc/value_net_lstm_grad.hip:
LSTM-RL and OM-LSTM-RL by backpropagation through time).  ``param_offsets`` is the flat parameter layout.  Each seam exists
once and takes its entry from the net's row of ``Family`` (``Family.train_entry``: cs_value_net_{grad_sizes|loss_grad|train_step|blob_index}
[_lstm][_om], cs_value_net_pack[_lstm][_om]_device): the sizes of the flat parameters and the scratch; the float32 blob written from the flat
parameters without leaving the device; the forward, the mean-squared-error loss and the whole gradient of a minibatch of stored rows
[B, n, cols (+ om_cols)] -- a human's rotated columns, then its map, as ``transform`` stores them --; that and, in the launch that sums the
gradient, torch's SGD step with momentum and the blob rewritten from the new parameters, the loss added to a device float64 sum, nothing
read back (``Trainer.set_update("device")``; ``DeviceNet.updated_on_device`` is its word that parameters and blob changed together under the
version counters); and, on the host, the blob float of every parameter.  The public names are those seams for one family each, refusing
every other net with their own sentence: ``grad_sizes``, ``pack_on_device``, ``loss_and_grad``, ``train_step`` (the feed-forward family,
``has_gradient_kernel``, GRADIENT_REFUSAL), the same with `_lstm` (the recurrent one without map columns, ``has_recurrent_gradient_kernel``,
RECURRENT_GRADIENT_REFUSAL) and with `_om` and ``blob_index_om`` (both families with map columns, ``has_mapped_gradient_kernel``,
MAPPED_GRADIENT_REFUSAL).  ``DeviceNet.adopt_flat`` is a trainer's word that the module's parameters are views of such a flat tensor
(crowd_nav/utils/trainer.py ``Trainer.set_gradient``; ``mapped=True`` from its map modes)."""
from __future__ import annotations

import ctypes as C
from types import MappingProxyType as frozen
from typing import NamedTuple

import numpy as np

CS_VN_CADRL, CS_VN_SARL = 0, 1     # include/crowdstep.h
CS_VN_LSTM = "lstm"                # this module's tag of an LSTM-RL network: the C entries of that network take no `kind`
MAP_ORDERS = frozen({"own": 0, "reference": 1})      # include/crowdstep.h CS_VN_MAPS_OWN, CS_VN_MAPS_FIRST_ACTION
PRECISIONS = ("f32", "bf16")
DECISION_INPUTS = ("tensor", "fused")
RECURRENT_PRECISIONS = ("f32", "bf16")      # of the recurrent family without map columns: "bf16" is cs_value_net_decide_lstm_bf16
RECURRENT_BF16 = "recurrent_bf16"           # DeviceNet's key of that arithmetic's blob
RECURRENT_INPUTS = ("tensor", "fused")      # of the same family: "fused" is cs_value_net_decide_lstm_worlds[_bf16], no look-ahead tensor
MAPPED_PRECISIONS = ("f32", "bf16")         # of the recurrent family with map columns: "bf16" is cs_value_net_decide_lstm_om_bf16
MAPPED_RECURRENT_BF16 = "mapped_recurrent_bf16"     # the key of that arithmetic's blob, on a DeviceNet of family RECURRENT_MAPPED alone
WIDE_PRECISIONS = ("f32", "bf16")           # of the feed-forward family with map columns (OM-SARL): "bf16" is cs_value_net_decide_om_bf16
WIDE_BF16 = "wide_bf16"                     # the key of that arithmetic's blob, on a DeviceNet of family MAPPED alone


def check_precision(precision):
    if precision not in PRECISIONS:
        raise ValueError(f"decision precision {precision!r}: one of {', '.join(map(repr, PRECISIONS))}")
    return precision


GRADIENT_REFUSAL = ("{0}: the fused loss-and-gradient kernel (cs_value_net_loss_grad) covers the feed-forward networks, CADRL's and SARL's; "
                    'an LSTM without map columns has its own (cs_value_net_loss_grad_lstm: the *_lstm helpers, Trainer.set_gradient("device_lstm")); '
                    'a network with occupancy-map columns has the *_om helpers (Trainer.set_gradient("device_om"), ("device_lstm_om"))')
RECURRENT_GRADIENT_REFUSAL = ("{0}: the recurrent loss-and-gradient kernel (cs_value_net_loss_grad_lstm) covers LSTM-RL's two networks on rows of "
                              '13 or 15 columns; CADRL and SARL have cs_value_net_loss_grad (Trainer.set_gradient("device")), a network with '
                              'occupancy-map columns (OM-SARL, OM-LSTM-RL) has the *_om helpers (Trainer.set_gradient("device_om"), '
                              '("device_lstm_om"))')
MAPPED_GRADIENT_REFUSAL = ("{0}: the *_om helpers cover the networks with occupancy-map columns, OM-SARL's and OM-LSTM-RL's; a network "
                           "without map columns has {1}")


class OwnArithmetic(NamedTuple):
    """A family's own opt-in arithmetic beside its ``modes`` (the recurrent families' and OM-SARL's bf16 decision)."""
    key: str                # DeviceNet's key of its blob
    pack: tuple             # (pack entry, what it counts its blob in)
    decide: str             # the decide entry on the look-ahead tensor: the family's decide_int and takes_maps hold for it too
    word: str               # what its names say: check_<word>_precision, DeviceNet.refresh_<word>, <word>_precision
    no_blob: str            # the sentence a decision without a packed blob is refused with, behind the caller's name


class Family(NamedTuple):
    """What one family of value networks states about itself; everything else in this module, the policies and the Gym ask a row of this
    table."""
    pack: frozen            # precision -> (pack entry, what it counts its blob in)
    takes_kind: bool        # the C entries open with a `kind`
    decide: frozen          # precision -> the decide entry on the look-ahead tensor
    decide_int: str         # the integers that entry takes behind cols: "", "om_cols", "sorted_by_distance" or "om_cols sorted_by_distance
                            # map_order"
    takes_maps: bool        # that entry takes the maps behind rotated; the pack entry om_cols behind cols
    modes: tuple            # the (decision input, precision) pairs the family runs
    refusal: str            # the sentence every other pair is refused with ({0!r}: the input, {1!r}: the precision)
    min_humans: int         # humans a world needs
    state_launch: bool      # V(s) is one cs_value_net_state launch; else rows, [maps,] the decide entry with A = 1
    train_infix: str        # the training entries' infix: "" or "_lstm" (`_om`, and om_cols behind cols, follow from takes_maps)
    flat_rows: bool         # the training seams take rows [B, cols] as n = 1 (CADRL's stored states)
    train_refusal: str      # the sentence the family's training seams refuse every other net with ({0}: the caller, {1}: the helper to use)
    own: OwnArithmetic = None       # the family's own opt-in arithmetic, where it has one
    wide: OwnArithmetic = None      # MAPPED's: the same statement under the word "wide", apart from `own` (the module's docstring)
    worlds: frozen = None           # RECURRENT's: recurrent precision -> the decide entry on the worlds' own rows (RECURRENT_INPUTS "fused")

    def lead(self, kind):
        return (kind,) if self.takes_kind else ()

    def train_entry(self, stem):
        """The name of the family's training entry `stem`: grad_sizes, loss_grad, train_step, blob_index or pack_device."""
        tail = "_om" if self.takes_maps else ""
        return f"cs_value_net_pack{self.train_infix}{tail}_device" if stem == "pack_device" else f"cs_value_net_{stem}{self.train_infix}{tail}"


FEED_FORWARD = Family(
    pack=frozen({"f32": ("cs_value_net_pack", np.float32), "bf16": ("cs_value_net_pack_bf16", np.uint8)}), takes_kind=True,
    decide=frozen({"f32": "cs_value_net_decide", "bf16": "cs_value_net_decide_bf16"}), decide_int="", takes_maps=False,
    modes=(("tensor", "f32"), ("tensor", "bf16"), ("fused", "f32")),
    refusal='decision input "fused" with decision precision "bf16": the bf16 kernel has its own tile loader and reads the look-ahead tensor; '
            'choose "tensor" or "f32"',
    min_humans=1, state_launch=True, train_infix="", flat_rows=True, train_refusal=GRADIENT_REFUSAL)
MAPPED = Family(
    pack=frozen({"f32": ("cs_value_net_pack_om", np.float32)}), takes_kind=True,
    decide=frozen({"f32": "cs_value_net_decide_om"}), decide_int="om_cols", takes_maps=True,
    modes=(("tensor", "f32"),),
    refusal='decision input {0!r} with decision precision {1!r} for a network with occupancy-map columns: no kernel pairs the map columns '
            'with the "fused" or the "bf16" tile loader; OM-SARL decides with "tensor" and "f32"',
    min_humans=2, state_launch=False, train_infix="", flat_rows=False, train_refusal=MAPPED_GRADIENT_REFUSAL,
    wide=OwnArithmetic(key=WIDE_BF16, pack=("cs_value_net_pack_om_bf16", np.uint8), decide="cs_value_net_decide_om_bf16", word="wide",
                       no_blob='the network has no wide bf16 blob yet (DeviceNet.refresh_wide("bf16"))'))
RECURRENT = Family(
    pack=frozen({"f32": ("cs_value_net_pack_lstm", np.float32)}), takes_kind=False,
    decide=frozen({"f32": "cs_value_net_decide_lstm"}), decide_int="sorted_by_distance", takes_maps=False,
    modes=(("tensor", "f32"),),
    refusal='decision input {0!r} with decision precision {1!r} for a recurrent network: LSTM-RL has the one kernel, float32 on the '
            'look-ahead tensor; it decides with "tensor" and "f32"',
    min_humans=1, state_launch=False, train_infix="_lstm", flat_rows=False, train_refusal=RECURRENT_GRADIENT_REFUSAL,
    own=OwnArithmetic(key=RECURRENT_BF16, pack=("cs_value_net_pack_lstm_bf16", np.uint8), decide="cs_value_net_decide_lstm_bf16", word="recurrent",
                      no_blob='the network has no recurrent bf16 blob yet (DeviceNet.refresh_recurrent("bf16"))'),
    worlds=frozen({"f32": "cs_value_net_decide_lstm_worlds", "bf16": "cs_value_net_decide_lstm_worlds_bf16"}))
RECURRENT_MAPPED = Family(
    pack=frozen({"f32": ("cs_value_net_pack_lstm_om", np.float32)}), takes_kind=False,
    decide=frozen({"f32": "cs_value_net_decide_lstm_om"}), decide_int="om_cols sorted_by_distance map_order", takes_maps=True,
    modes=(("tensor", "f32"),),
    refusal='decision input {0!r} with decision precision {1!r} for a recurrent network with occupancy-map columns: OM-LSTM-RL has the one '
            'kernel, float32 on the look-ahead tensor and the maps; it decides with "tensor" and "f32"',
    min_humans=2, state_launch=False, train_infix="_lstm", flat_rows=False, train_refusal=MAPPED_GRADIENT_REFUSAL,
    own=OwnArithmetic(key=MAPPED_RECURRENT_BF16, pack=("cs_value_net_pack_lstm_om_bf16", np.uint8), decide="cs_value_net_decide_lstm_om_bf16",
                      word="mapped", no_blob='the network has no bf16 blob yet (DeviceNet.refresh_mapped("bf16"))'))


def family_of(kind, om_cols=0):
    """The family of a description (``describe``'s kind) with ``om_cols`` map columns."""
    if kind == CS_VN_LSTM:
        return RECURRENT_MAPPED if om_cols else RECURRENT
    return MAPPED if om_cols else FEED_FORWARD


def own_arithmetic(family):
    """The opt-in arithmetic a family states beside its ``modes``, in ``own`` or in ``wide``; None where it states none."""
    return family.own or family.wide


def has_gradient_kernel(family):
    """Whether a family's networks have the fused loss-and-gradient kernel (cs_value_net_loss_grad): the feed-forward ones alone."""
    return family is FEED_FORWARD


def has_recurrent_gradient_kernel(family):
    """Whether a family's networks have the recurrent loss-and-gradient kernel (cs_value_net_loss_grad_lstm): LSTM-RL without map columns."""
    return family is RECURRENT


def has_mapped_gradient_kernel(family):
    """Whether a family's networks have the loss-and-gradient kernels on rows with map columns (cs_value_net_loss_grad_om,
    cs_value_net_loss_grad_lstm_om): OM-SARL's and OM-LSTM-RL's."""
    return family is MAPPED or family is RECURRENT_MAPPED


def check_recurrent_precision(precision, family=None):
    """The arithmetic of the recurrent decision kernel a policy may hold: one of RECURRENT_PRECISIONS; "bf16" for the recurrent family
    without map columns alone (`family`: the policy's or the net's row, None asks only the name)."""
    if precision not in RECURRENT_PRECISIONS:
        raise ValueError(f"recurrent precision {precision!r}: one of {', '.join(map(repr, RECURRENT_PRECISIONS))}")
    if precision == "bf16" and family is not None and family is not RECURRENT:
        if family is RECURRENT_MAPPED:
            raise ValueError('recurrent precision "bf16" for a recurrent network with occupancy-map columns: OM-LSTM-RL has the one kernel, '
                             'cs_value_net_decide_lstm_om, float32 on the look-ahead tensor and the maps')
        raise ValueError('recurrent precision "bf16": the network is not an LSTM-RL one (CADRL and SARL choose with set_decision_precision)')
    return precision


def check_recurrent_input(recurrent_input, family=None):
    """Where the recurrent decision kernel's rows come from, as a policy may hold it: one of RECURRENT_INPUTS; "fused" for the recurrent
    family without map columns alone (`family`: the policy's or the net's row, None asks only the name)."""
    if recurrent_input not in RECURRENT_INPUTS:
        raise ValueError(f"recurrent input {recurrent_input!r}: one of {', '.join(map(repr, RECURRENT_INPUTS))}")
    if recurrent_input == "fused" and family is not None and family is not RECURRENT:
        if family is RECURRENT_MAPPED:
            raise ValueError('recurrent input "fused" for a recurrent network with occupancy-map columns: its kernel pairs every row with a '
                             "map and has no loader that generates the rows; OM-LSTM-RL decides from the look-ahead tensor")
        raise ValueError('recurrent input "fused": the network is not an LSTM-RL one (CADRL and SARL choose with set_decision_input; OM-SARL '
                         "decides from the look-ahead tensor)")
    return recurrent_input


def check_mapped_precision(precision, family=None):
    """The arithmetic of the recurrent decision kernel on rows with map columns a policy may hold: one of MAPPED_PRECISIONS; "bf16" for
    the recurrent family with map columns alone (`family`: the policy's or the net's row, None asks only the name)."""
    if precision not in MAPPED_PRECISIONS:
        raise ValueError(f"mapped precision {precision!r}: one of {', '.join(map(repr, MAPPED_PRECISIONS))}")
    if precision == "bf16" and family is not None and family is not RECURRENT_MAPPED:
        raise ValueError('mapped precision "bf16": cs_value_net_decide_lstm_om_bf16 is the kernel of OM-LSTM-RL, the recurrent network on rows '
                         "with occupancy-map columns; LSTM-RL without map columns chooses with set_recurrent_precision, CADRL and SARL with "
                         "set_decision_precision, OM-SARL decides in float32")
    return precision


def check_wide_precision(precision, family=None):
    """The arithmetic of the decision kernel on SARL's rows with map columns a policy may hold: one of WIDE_PRECISIONS; "bf16" for the
    feed-forward family with map columns alone (`family`: the policy's or the net's row, None asks only the name)."""
    if precision not in WIDE_PRECISIONS:
        raise ValueError(f"wide precision {precision!r}: one of {', '.join(map(repr, WIDE_PRECISIONS))}")
    if precision == "bf16" and family is not None and family is not MAPPED:
        raise ValueError('wide precision "bf16": cs_value_net_decide_om_bf16 is the kernel of OM-SARL, SARL\'s network on rows with '
                         "occupancy-map columns; CADRL and SARL choose with set_decision_precision, LSTM-RL with set_recurrent_precision, "
                         "OM-LSTM-RL with set_mapped_precision")
    return precision


def check_map_order(map_order):
    if map_order not in MAP_ORDERS:
        raise ValueError(f"map order {map_order!r}: one of {', '.join(map(repr, sorted(MAP_ORDERS, reverse=True)))}")
    return map_order


def check_mode(family, decision_input, precision):
    """The pair (decision input, precision) a network of `family` may hold: one of the family's modes.  An input the family runs in every
    precision asks nothing of the precision (``check_precision`` is the setters' and ``DeviceNet.head``'s)."""
    if decision_input not in DECISION_INPUTS:
        raise ValueError(f"decision input {decision_input!r}: one of {', '.join(map(repr, DECISION_INPUTS))}")
    runs = [p for i, p in family.modes if i == decision_input]
    if len(runs) < len(PRECISIONS) and (not runs or check_precision(precision) not in runs):
        raise ValueError(family.refusal.format(decision_input, precision))
    return decision_input


def check_decision_input(decision_input, precision, om_cols=0, recurrent=False):
    """``check_mode`` for who holds no family: "fused" (cs_value_net_decide_worlds: the rows are generated in the kernel, no look-ahead
    tensor) exists for the float32 arithmetic only.  A network with occupancy-map columns (``om_cols`` > 0) has the one kernel
    cs_value_net_decide_om: float32 on the look-ahead tensor.  So has a ``recurrent`` one (LSTM-RL: cs_value_net_decide_lstm)."""
    return check_mode(family_of(CS_VN_LSTM if recurrent else CS_VN_SARL, om_cols), decision_input, precision)


def _linears(seq):
    import torch.nn as nn

    return [m for m in seq if isinstance(m, nn.Linear)]


def describe(model):
    """(kind, dims int32 array, [Linear ...] in the order of dims) of a cadrl.ValueNetwork / sarl.ValueNetwork; for an lstm_rl.ValueNetwork1 /
    ValueNetwork2 (CS_VN_LSTM, cs_value_net_decide_lstm's dims [H, L1, mlp1 widths.., L2, mlp widths..], [mlp1's Linear .., the nn.LSTM,
    mlp's Linear ..])."""
    if hasattr(model, "lstm"):
        first, last = _linears(getattr(model, "mlp1", ())), _linears(model.mlp)
        dims = [model.lstm.hidden_size, len(first)] + [l.out_features for l in first] + [len(last)] + [l.out_features for l in last]
        return CS_VN_LSTM, np.array(dims, np.int32), first + [model.lstm] + last
    if hasattr(model, "value_network"):
        ls = _linears(model.value_network)
        return CS_VN_CADRL, np.array([len(ls)] + [l.out_features for l in ls], np.int32), ls
    dims, layers = [int(bool(model.with_global_state))], []
    for chain in (model.mlp1, model.mlp2, model.attention, model.mlp3):
        ls = _linears(chain)
        dims += [len(ls)] + [l.out_features for l in ls]
        layers += ls
    return CS_VN_SARL, np.array(dims, np.int32), layers


def layer_params(layer):
    """The tensors a pack entry takes of one entry of ``describe``'s list: a Linear's (weight, bias), an nn.LSTM's four."""
    if hasattr(layer, "weight_ih_l0"):
        return layer.weight_ih_l0, layer.weight_hh_l0, layer.bias_ih_l0, layer.bias_hh_l0
    return layer.weight, layer.bias


def pack(kind, dims, cols, arrays, precision="f32", om_cols=0):
    """The kernel's weight blob from [weight_0, bias_0, weight_1, ...] float32 arrays: float32 numpy for "f32", the bytes (uint8 numpy)
    of cs_value_net_pack_bf16's layout for "bf16"; with ``om_cols`` > 0 cs_value_net_pack_om's (float32 only: mlp1 reads cols + om_cols
    columns); for CS_VN_LSTM cs_value_net_pack_lstm's (float32 only; the LSTM's four arrays between mlp1's and mlp's), with ``om_cols`` > 0
    cs_value_net_pack_lstm_om's.  Host only: no GPU needed."""
    family = family_of(kind, om_cols)
    check_mode(family, "tensor", precision)
    return _pack_with(family, kind, family.pack[check_precision(precision)], dims, cols, om_cols, arrays)


def pack_lstm_bf16(dims, cols, arrays):
    """cs_value_net_pack_lstm_bf16's blob (uint8 numpy: include/crowdstep.h states the bytes) of an LSTM-RL network without map columns from
    the float32 arrays ``pack(CS_VN_LSTM, ...)`` takes.  Host only: no GPU needed."""
    return _pack_with(RECURRENT, CS_VN_LSTM, RECURRENT.own.pack, dims, cols, 0, arrays)


def pack_lstm_om_bf16(dims, cols, om_cols, arrays):
    """cs_value_net_pack_lstm_om_bf16's blob (uint8 numpy: include/crowdstep.h states the bytes) of an OM-LSTM-RL network from the float32
    arrays ``pack(CS_VN_LSTM, ..., om_cols=om_cols)`` takes.  Host only: no GPU needed."""
    return _pack_with(RECURRENT_MAPPED, CS_VN_LSTM, RECURRENT_MAPPED.own.pack, dims, cols, om_cols, arrays)


def pack_om_bf16(dims, cols, om_cols, arrays):
    """cs_value_net_pack_om_bf16's blob (uint8 numpy: include/crowdstep.h states the bytes) of an OM-SARL network from the float32 arrays
    ``pack(CS_VN_SARL, ..., om_cols=om_cols)`` takes.  Host only: no GPU needed."""
    return _pack_with(MAPPED, CS_VN_SARL, MAPPED.wide.pack, dims, cols, om_cols, arrays)


def _pack_with(family, kind, entry_and_unit, dims, cols, om_cols, arrays):
    """The size query and the packing call of one of `family`'s pack entries: (its name, what it counts its blob in), from the row's
    ``pack``, its ``own`` or its ``wide``."""
    from ... import _lib

    entry, unit = getattr(_lib.load(), entry_and_unit[0]), entry_and_unit[1]
    dims = np.ascontiguousarray(dims, np.int32)
    lead = family.lead(kind) + (dims.ctypes.data, len(dims), cols) + ((om_cols,) if family.takes_maps else ())
    arrays = [np.ascontiguousarray(a, np.float32) for a in arrays]
    ptrs = (C.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])
    nf = C.c_size_t(0)
    _lib.check(entry(*lead, None, None, C.byref(nf)))
    blob = np.zeros(nf.value, unit)
    _lib.check(entry(*lead, ptrs, blob.ctypes.data, C.byref(nf)))
    return blob


class DeviceNet:
    """A policy's network as the kernel reads it: description + one packed blob per precision in HBM, each rebuilt when the module's
    parameters changed (the same version-counter key for both).  ``blob`` is the float32 one.  ``om_cols`` > 0: an OM-SARL network whose
    mlp1 reads cols + om_cols columns (cs_value_net_pack_om's blob); ``om_grid`` = (cell_num, cell_size, om_channel_size) of its maps;
    ``last_maps``: the maps [W, n, om_cols] of its last ``decide_for_worlds``.  ``lstm``: an LSTM-RL network (cs_value_net_pack_lstm's blob,
    float32 only; the version key covers the LSTM's four tensors); with ``om_cols`` > 0 an OM-LSTM-RL one, ``map_order`` (MAP_ORDERS) the
    pairing of its decisions.  ``family``: its row of the family table, which says all of that."""

    def __init__(self, model, cols, om_cols=0, om_grid=None, map_order="reference"):
        self.model, self.cols, self.om_cols, self.om_grid = model, int(cols), int(om_cols), om_grid
        self.map_order = check_map_order(map_order)
        self.last_maps = None
        self.kind, self.dims, self.layers = describe(model)
        self.family = family_of(self.kind, self.om_cols)
        self.lstm = self.kind == CS_VN_LSTM
        # (an own arithmetic's blob lies under the key its row states: "bf16" stays the feed-forward arithmetic's, which a recurrent net
        # refuses.  RECURRENT's key is on every net, as it was before the table stated it; any other row's on a net of that family alone)
        stated = own_arithmetic(self.family)
        keys = PRECISIONS + (RECURRENT.own.key,) + ((stated.key,) if stated else ())
        self._keys = dict.fromkeys(keys)
        self.blobs = dict.fromkeys(keys)
        self.flat = None

    @property
    def blob(self):
        return self.blobs["f32"]

    def _versions(self):
        return tuple((p.data_ptr(), p._version) for l in self.layers for p in layer_params(l))

    def _repacked(self, key, entry_and_unit):
        """The blob under `key`, packed again through that entry of the family when a parameter's version changed."""
        import torch

        versions = self._versions()
        if versions != self._keys[key]:
            arrays = [p.detach().to("cpu", torch.float32).numpy() for l in self.layers for p in layer_params(l)]
            blob = _pack_with(self.family, self.kind, entry_and_unit, self.dims, self.cols, self.om_cols, arrays)
            self.blobs[key] = torch.from_numpy(blob).to("cuda")
            self._keys[key] = versions
        return self.blobs[key]

    def refresh(self, precision="f32"):
        if self.flat is not None and precision == "f32":        # the parameters are views of `flat` (adopt_flat): packed where they lie
            key = self._versions()
            if key != self._keys[precision]:
                _pack_on_device(self, self.flat)
                self._keys[precision] = key
            return self.blobs[precision]
        check_mode(self.family, "tensor", check_precision(precision))
        return self._repacked(precision, self.family.pack[precision])

    def refresh_recurrent(self, precision="f32"):
        """``refresh`` for the recurrent family's own arithmetics (RECURRENT_PRECISIONS): "f32" is ``refresh("f32")``; "bf16" keeps
        cs_value_net_pack_lstm_bf16's blob under the key RECURRENT_BF16, rebuilt on the same version-counter rule and dropped by
        ``updated_on_device``; it never aliases the float32 blob."""
        if check_recurrent_precision(precision, self.family) == "f32":
            return self.refresh("f32")
        return self._repacked(self.family.own.key, self.family.own.pack)

    def refresh_mapped(self, precision="f32"):
        """``refresh`` for the arithmetics of the recurrent family with map columns (MAPPED_PRECISIONS): "f32" is ``refresh("f32")``; "bf16"
        keeps cs_value_net_pack_lstm_om_bf16's blob under the key MAPPED_RECURRENT_BF16, rebuilt on the same version-counter rule and
        dropped by ``updated_on_device``; it never aliases the float32 blob.  Every other family is refused with the reason."""
        if check_mapped_precision(precision, self.family) == "f32":
            return self.refresh("f32")
        return self._repacked(self.family.own.key, self.family.own.pack)

    def refresh_wide(self, precision="f32"):
        """``refresh`` for the arithmetics of the feed-forward family with map columns (WIDE_PRECISIONS): "f32" is ``refresh("f32")``; "bf16"
        keeps cs_value_net_pack_om_bf16's blob under the key WIDE_BF16, rebuilt on the same version-counter rule and dropped by
        ``updated_on_device``; it never aliases the float32 blob.  Every other family is refused with the reason."""
        if check_wide_precision(precision, self.family) == "f32":
            return self.refresh("f32")
        return self._repacked(self.family.wide.key, self.family.wide.pack)

    def refresh_selected(self, decision_precision, recurrent_precision, mapped_precision, wide_precision="f32"):
        """What a policy's four attributes select: the blob of ``decision_precision`` and, where the others are not "f32", the family's own."""
        self.refresh(decision_precision)
        if recurrent_precision != "f32":
            self.refresh_recurrent(recurrent_precision)
        if mapped_precision != "f32":
            self.refresh_mapped(mapped_precision)
        if wide_precision != "f32":
            self.refresh_wide(wide_precision)

    def adopt_flat(self, flat, mapped=False):
        """A trainer's word that the module's parameters are views of `flat` (a CUDA float32 tensor in ``param_offsets``' layout, as
        ``Trainer.set_gradient("device")`` or ``("device_lstm")`` makes them): from now on ``refresh("f32")`` packs the blob on the device
        (``pack_on_device``, or ``pack_lstm_on_device`` for a recurrent net) when a parameter's version changed, with no host round trip.
        None takes the word back.  ``mapped=True`` is the word of the map modes ("device_om", "device_lstm_om") for a net with map
        columns, which packs through ``pack_om_on_device``; without it such a net is refused as before."""
        if flat is not None:
            if mapped:
                _served(self, "adopt_flat(mapped=True)", MAPPED, RECURRENT_MAPPED, narrow="adopt_flat(flat)")
            else:
                _served(self, "adopt_flat", FEED_FORWARD, RECURRENT)
            total = param_offsets(self)[-1]
            if not flat.is_cuda or flat.dtype != _torch().float32 or flat.dim() != 1 or flat.numel() != total or not flat.is_contiguous():
                raise ValueError(f"adopt_flat: the flat parameters are one contiguous CUDA float32 tensor of {total} elements")
        self.flat = flat
        self._keys["f32"] = None

    def updated_on_device(self):
        """The word of ``train_step`` / ``train_step_lstm`` / ``train_step_om`` that a kernel updated the flat parameters and rewrote the float32 blob from them
        in the same launch.  A kernel's write moves no version counter: the float32 key stays valid (no repack, the blob is current), every
        other precision's key is dropped, so its next ``refresh`` packs from the new numbers."""
        if self.flat is None:
            raise ValueError("updated_on_device: the network has adopted no flat parameters (adopt_flat)")
        for precision in self._keys:
            if precision != "f32":
                self._keys[precision] = None

    def head(self, caller, precision="f32"):
        """The arguments every network entry of the family opens with, for the blob of `precision`; ValueError in `caller`'s name
        without one."""
        blob = self.blobs[check_precision(precision)]
        if blob is None:
            raise ValueError(f"{caller}: the network has no {precision} blob yet (DeviceNet.refresh({precision!r}))")
        return _head(self.family.lead(self.kind), self.dims, blob)


def _head(lead, dims, blob):
    """[kind,] dims (host int32 array), its length, the packed blob (a CUDA tensor) and its length in the blob's own unit."""
    return lead + (dims.ctypes.data, len(dims), blob.data_ptr(), blob.numel())


def _torch():
    import torch

    return torch


def param_offsets(net):
    """The flat layout cs_value_net_loss_grad and cs_value_net_pack_device read: where every tensor of ``describe``'s layers starts, in
    elements -- weight_0, bias_0, weight_1, ... each dense in torch's own layout -- and, last, the total."""
    offsets = [0]
    for layer in net.layers:
        for p in layer_params(layer):
            offsets.append(offsets[-1] + p.numel())
    return tuple(offsets)


def _stream(stream):
    return _torch().cuda.current_stream().cuda_stream if stream is None else stream


# ---------------------------------------------------------------------------------------------------------------- the training seams, once
def _served(net, caller, *families, narrow=None):
    """`net`, when its family is one of `families`; ValueError in `caller`'s name with their refusal sentence otherwise (`narrow`: the
    helper that sentence names for a net without map columns)."""
    if not any(net.family is family for family in families):
        raise ValueError(families[0].train_refusal.format(caller, narrow))
    return net


def _entry(net, stem):
    from ... import _lib

    return getattr(_lib.load(), net.family.train_entry(stem))


def _described(net):
    """What a training entry without a blob opens with: [kind,] dims, its length, cols[, om_cols]"""
    return net.family.lead(net.kind) + (net.dims.ctypes.data, len(net.dims)) + _width(net)


def _width(net):
    return (net.cols, net.om_cols) if net.family.takes_maps else (net.cols,)


def _grad_sizes(net, B, n):
    from ... import _lib

    n_params, n_scratch = C.c_size_t(0), C.c_size_t(0)
    _lib.check(_entry(net, "grad_sizes")(*_described(net), B, n, C.byref(n_params), C.byref(n_scratch)))
    return n_params.value, n_scratch.value


def _pack_on_device(net, flat, stream=None):
    """The float32 blob is allocated once and rewritten in place."""
    from ... import _lib

    blob = net.blobs["f32"]
    if blob is None:
        nf = C.c_size_t(0)
        _lib.check(getattr(_lib.load(), net.family.pack["f32"][0])(*_described(net), None, None, C.byref(nf)))
        blob = net.blobs["f32"] = _torch().empty(nf.value, dtype=_torch().float32, device=flat.device)
    _lib.check(_entry(net, "pack_device")(*_described(net), flat.data_ptr(), flat.numel(), blob.data_ptr(), blob.numel(), _stream(stream)))
    return blob


def _blob_index(net):
    from ... import _lib

    index = np.full(param_offsets(net)[-1], -1, np.int32)
    _lib.check(_entry(net, "blob_index")(*_described(net), index.ctypes.data, index.size))
    return index


def _minibatch(caller, net, flat, rows, targets, grad, values, stream, momentum=None, loss_sum=None):
    """The tensor checks the loss-and-gradient and the train-step seams make alike, in `caller`'s name, and the scratch kept on `net`,
    grown when a larger minibatch comes: (a new tensor for the loss, the entry's arguments from B to the loss, its last four)."""
    torch = _torch()
    if rows.dim() == 2 and net.family.flat_rows:
        rows = rows[:, None, :]
    if rows.dim() != 3:
        raise ValueError(f"{caller}: rows are [B, n, {'cols + om_cols' if net.family.takes_maps else 'cols'}], not {tuple(rows.shape)}")
    B, n, cols = rows.shape
    tensors = [("flat", flat, flat.numel()), ("rows", rows, B * n * cols), ("targets", targets, B), ("grad", grad, flat.numel()), ("values", values, B)]
    if momentum is not None:
        tensors.append(("momentum", momentum, flat.numel()))
    for name, t, numel in tensors:
        if t is not None and (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != numel):
            raise ValueError(f"{caller}: {name} is a contiguous CUDA float32 tensor of {numel} elements")
    if loss_sum is not None and (not loss_sum.is_cuda or loss_sum.dtype != torch.float64 or loss_sum.numel() != 1):
        raise ValueError(f"{caller}: loss_sum is a CUDA float64 tensor of one element")
    if cols != net.cols + net.om_cols:
        raise ValueError(f"{caller}: rows of {cols} columns for a network of {net.cols + net.om_cols}")
    _, need = _grad_sizes(net, B, n)
    scratch = getattr(net, "_grad_scratch", None)
    if scratch is None or scratch.numel() < need or scratch.device != flat.device:
        scratch = net._grad_scratch = torch.empty(need, dtype=torch.float32, device=flat.device)
    loss = torch.empty(1, dtype=torch.float32, device=flat.device)
    return (loss, (B, n, *_width(net), rows.data_ptr(), targets.data_ptr(), grad.data_ptr(), loss.data_ptr()),
            (None if values is None else values.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream(stream)))


def _loss_and_grad(caller, net, flat, rows, targets, grad, values, stream):
    from ... import _lib

    head = net.head(caller)
    loss, batch, tail = _minibatch(caller, net, flat, rows, targets, grad, values, stream)
    _lib.check(_entry(net, "loss_grad")(*head, flat.data_ptr(), flat.numel(), *batch, *tail))
    return loss


def _train_step(caller, net, flat, momentum, rows, targets, grad, lr, mu, values, loss_sum, stream):
    from ... import _lib

    if momentum is None:
        raise ValueError(f"{caller}: momentum is a contiguous CUDA float32 tensor of {flat.numel()} elements")
    head = net.head(caller)
    if net.flat is not flat:
        raise ValueError(f"{caller}: `flat` is not the tensor the network's parameters are views of (DeviceNet.adopt_flat)")
    loss, batch, tail = _minibatch(caller, net, flat, rows, targets, grad, values, stream, momentum, loss_sum)
    _lib.check(_entry(net, "train_step")(*head, flat.data_ptr(), flat.numel(), momentum.data_ptr(), momentum.numel(), float(lr), float(mu), *batch,
                                         None if loss_sum is None else loss_sum.data_ptr(), *tail))
    net.updated_on_device()
    return loss


# ---------------------------------------------------------------------------------------------------------------- their public names
def pack_on_device(net, flat, stream=None):
    """cs_value_net_pack_device: `net`'s float32 blob from the flat parameters `flat` (``param_offsets``' layout, a CUDA tensor), one
    launch on `stream` (None: torch's current one); byte for byte ``pack``'s blob.  The blob is allocated once and rewritten in place."""
    return _pack_on_device(_served(net, "pack_on_device", FEED_FORWARD), flat, stream)


def grad_sizes(net, B, n):
    """cs_value_net_grad_sizes: (the length of the flat parameters, the scratch floats a minibatch of B samples of n humans needs)."""
    return _grad_sizes(_served(net, "grad_sizes", FEED_FORWARD), B, n)


def loss_and_grad(net, flat, rows, targets, grad, values=None, stream=None):
    """cs_value_net_loss_grad: the mean-squared-error loss of `net` on the minibatch rows [B, n, cols] (CADRL: n = 1, or [B, cols])
    against targets [B] or [B, 1], and its gradient into `grad` (the layout of `flat`; written, not accumulated); values [B] or None
    receives the network's outputs.  CUDA float32 tensors; `net`'s float32 blob must hold `flat`'s numbers (``pack_on_device``).
    Returns the loss, a CUDA tensor of one element.  The scratch is kept on `net` and grown when a larger minibatch comes."""
    return _loss_and_grad("loss_and_grad", _served(net, "loss_and_grad", FEED_FORWARD), flat, rows, targets, grad, values, stream)


def train_step(net, flat, momentum, rows, targets, grad, lr, mu, values=None, loss_sum=None, stream=None):
    """cs_value_net_train_step: ``loss_and_grad`` (the same arguments, checks, scratch and results -- `grad`, the returned loss and `values`
    are its bytes) and, in the launch that sums the gradient, torch's SGD step with momentum `mu` at learning rate `lr` on `flat` and
    `momentum` (a CUDA float32 tensor like `flat`: the optimiser's momentum buffers, zeros before the first step) and `net`'s float32 blob
    rewritten from the new parameters, byte for byte ``pack``'s.  `flat` is the tensor `net` adopted (``adopt_flat``) and its float32 blob
    holds `flat`'s numbers on entry, as for ``loss_and_grad``.  loss_sum (a CUDA float64 tensor of one element, or None) has the loss added to
    it on the device.  Nothing is read back.  Ends with ``net.updated_on_device()``."""
    return _train_step("train_step", _served(net, "train_step", FEED_FORWARD), flat, momentum, rows, targets, grad, lr, mu, values, loss_sum, stream)


def pack_lstm_on_device(net, flat, stream=None):
    """cs_value_net_pack_lstm_device: ``pack_on_device`` for a recurrent `net` -- byte for byte ``pack``'s blob (cs_value_net_pack_lstm)."""
    return _pack_on_device(_served(net, "pack_lstm_on_device", RECURRENT), flat, stream)


def grad_sizes_lstm(net, B, n):
    """cs_value_net_grad_sizes_lstm: (the length of the flat parameters, the scratch floats a minibatch of B samples of n humans needs: a
    partial gradient and the tape of n steps per workgroup)."""
    return _grad_sizes(_served(net, "grad_sizes_lstm", RECURRENT), B, n)


def loss_and_grad_lstm(net, flat, rows, targets, grad, values=None, stream=None):
    """cs_value_net_loss_grad_lstm: ``loss_and_grad`` for a recurrent `net` on the minibatch rows [B, n, cols], every sample's rows in the
    order they lie in; `net`'s float32 blob must hold `flat`'s numbers (``pack_lstm_on_device``).  Returns the loss, a CUDA tensor of one
    element.  The scratch (partial gradients and tapes) is kept on `net` and grown when a larger minibatch comes."""
    return _loss_and_grad("loss_and_grad_lstm", _served(net, "loss_and_grad_lstm", RECURRENT), flat, rows, targets, grad, values, stream)


def train_step_lstm(net, flat, momentum, rows, targets, grad, lr, mu, values=None, loss_sum=None, stream=None):
    """cs_value_net_train_step_lstm: ``train_step`` for a recurrent `net` -- ``loss_and_grad_lstm``, the SGD step and the recurrent blob (the
    gate rows, bias_ih + bias_hh) rewritten, in two launches."""
    return _train_step("train_step_lstm", _served(net, "train_step_lstm", RECURRENT), flat, momentum, rows, targets, grad, lr, mu, values, loss_sum,
                       stream)


def _mapped(net, caller, narrow):
    return _served(net, caller, MAPPED, RECURRENT_MAPPED, narrow=narrow)


def grad_sizes_om(net, B, n):
    """cs_value_net_grad_sizes_om / cs_value_net_grad_sizes_lstm_om: ``grad_sizes`` / ``grad_sizes_lstm`` for a net with map columns."""
    return _grad_sizes(_mapped(net, "grad_sizes_om", "grad_sizes / grad_sizes_lstm"), B, n)


def pack_om_on_device(net, flat, stream=None):
    """cs_value_net_pack_om_device / cs_value_net_pack_lstm_om_device: ``pack_on_device`` for a net with map columns -- byte for byte
    ``pack``'s blob (cs_value_net_pack_om / cs_value_net_pack_lstm_om)."""
    return _pack_on_device(_mapped(net, "pack_om_on_device", "pack_on_device / pack_lstm_on_device"), flat, stream)


def loss_and_grad_om(net, flat, rows, targets, grad, values=None, stream=None):
    """cs_value_net_loss_grad_om / cs_value_net_loss_grad_lstm_om: ``loss_and_grad`` / ``loss_and_grad_lstm`` for a net with map columns
    on the minibatch rows [B, n, cols + om_cols] -- a row is a human's rotated columns, then its map, as ``transform`` stores them;
    `net`'s float32 blob must hold `flat`'s numbers (``pack_om_on_device``).  Returns the loss, a CUDA tensor of one element."""
    return _loss_and_grad("loss_and_grad_om", _mapped(net, "loss_and_grad_om", "loss_and_grad / loss_and_grad_lstm"), flat, rows, targets, grad, values,
                          stream)


def train_step_om(net, flat, momentum, rows, targets, grad, lr, mu, values=None, loss_sum=None, stream=None):
    """cs_value_net_train_step_om / cs_value_net_train_step_lstm_om: ``train_step`` / ``train_step_lstm`` for a net with map columns --
    ``loss_and_grad_om``, the SGD step and the blob (the wide first layer included; its k-group padding stays zero) rewritten."""
    return _train_step("train_step_om", _mapped(net, "train_step_om", "train_step / train_step_lstm"), flat, momentum, rows, targets, grad, lr, mu,
                       values, loss_sum, stream)


def blob_index_om(net):
    """cs_value_net_blob_index_om / cs_value_net_blob_index_lstm_om (host only): the float of ``pack``'s blob that holds every parameter
    of ``param_offsets``' flat layout, an int32 numpy array."""
    return _blob_index(_mapped(net, "blob_index_om", "cs_value_net_blob_index / cs_value_net_blob_index_lstm"))


def decide_rows(net, W, A, n, rotated, extra, *tail, precision="f32", own=False):
    """The tensor decide entry of `net`'s family on device pointers (ints).  `extra`: what that entry takes beyond
    cs_value_net_decide's arguments -- the maps [W][n][net.om_cols], or sorted_by_distance, or the pair (maps, sorted_by_distance) for a
    family that takes both (``net.map_order`` goes with them); `tail`: rewards, actions, robot, robot_stride, gamma, dt, override, values,
    choice, action_out, stream.  `own`: the family's own arithmetic (``own_arithmetic``) -- its entry on its blob, the same arguments."""
    from ... import _lib

    family = net.family
    if own:
        stated = own_arithmetic(family)
        entry, blob = stated.decide, net.blobs[stated.key]
        if blob is None:
            raise ValueError(f"{entry.removeprefix('cs_value_net_')}: {stated.no_blob}")
        head = _head(family.lead(net.kind), net.dims, blob)
    else:
        entry, head = family.decide[precision], net.head(family.decide["f32"].removeprefix("cs_value_net_"), precision)
    both = "sorted_by_distance" in family.decide_int and family.takes_maps
    maps, in_order = extra if both else (extra, extra)
    given = {"om_cols": lambda: net.om_cols, "sorted_by_distance": lambda: int(bool(in_order)), "map_order": lambda: MAP_ORDERS[net.map_order]}
    behind_cols = tuple(given[name]() for name in family.decide_int.split())
    behind_rotated = (maps,) if family.takes_maps else ()
    _lib.check(getattr(_lib.load(), entry)(*head, W, A, n, net.cols, *behind_cols, rotated, *behind_rotated, *tail))


def decide(net, W, A, n, rotated, rewards, actions, robot, robot_stride, gamma, dt, override, values, choice, action_out, stream=None,
           precision="f32"):
    """cs_value_net_decide (`precision` "f32") or cs_value_net_decide_bf16 ("bf16") on device pointers (ints); `net` a DeviceNet whose
    blob of that precision is current (refresh(precision))."""
    decide_rows(net, W, A, n, rotated, None, rewards, actions, robot, robot_stride, gamma, dt, override, values, choice, action_out, stream,
                precision=precision)


def occupancy_maps(W, n, humans, stride, vel_col, cell_num, cell_size, channels, maps, stream=None):
    """cs_occupancy_maps on device pointers (ints): humans [W][n][stride] with the position at columns 0, 1 and the velocity at vel_col,
    vel_col + 1 -> maps [W][n][cell_num^2 * channels]."""
    from ... import _lib

    _lib.check(_lib.load().cs_occupancy_maps(W, n, humans, stride, vel_col, cell_num, cell_size, channels, maps, stream))


def maps_of(humans, vel_col, grid, stream=None):
    """occupancy_maps for a CUDA tensor [W, n, stride] of human rows: a new tensor [W, n, C]; `grid` = (cell_num, cell_size, channels).
    Worlds of one human have no other human to map: ValueError, before any launch (the reference's build_occupancy_maps raises it too)."""
    import torch

    W, n, stride = humans.shape
    cell_num, cell_size, channels = grid
    if n < 2:
        raise ValueError("occupancy maps need at least two humans: a lone human has no other human to map")
    maps = torch.empty((W, n, cell_num * cell_num * channels), dtype=torch.float32, device="cuda")
    occupancy_maps(W, n, humans.data_ptr(), stride, vel_col, cell_num, cell_size, channels, maps.data_ptr(), stream)
    return maps


def decide_om(net, W, A, n, rotated, maps, rewards, actions, robot, robot_stride, gamma, dt, override, values, choice, action_out, stream=None):
    """cs_value_net_decide_om on device pointers (ints): ``decide`` for a DeviceNet with map columns, maps [W][n][net.om_cols]."""
    if net.family is not MAPPED:
        raise ValueError("decide_om: the network has no occupancy-map columns (DeviceNet(model, cols, om_cols))")
    decide_rows(net, W, A, n, rotated, maps, rewards, actions, robot, robot_stride, gamma, dt, override, values, choice, action_out, stream)


def decide_om_bf16(net, W, A, n, rotated, maps, rewards, actions, robot, robot_stride, gamma, dt, override, values, choice, action_out, stream=None):
    """cs_value_net_decide_om_bf16 on device pointers (ints): ``decide_om`` in the opt-in bf16 arithmetic, for a DeviceNet of an OM-SARL
    network whose wide bf16 blob is current (``refresh_wide("bf16")``)."""
    if net.family is not MAPPED:
        raise ValueError("decide_om_bf16: the network is not SARL's with occupancy-map columns (DeviceNet(model, cols, om_cols))")
    decide_rows(net, W, A, n, rotated, maps, rewards, actions, robot, robot_stride, gamma, dt, override, values, choice, action_out, stream,
                own=True)


def decide_lstm(net, W, A, n, sorted_by_distance, rotated, rewards, actions, robot, robot_stride, gamma, dt, override, values, choice, action_out,
                stream=None):
    """cs_value_net_decide_lstm on device pointers (ints): ``decide`` for a DeviceNet of an LSTM-RL network; ``sorted_by_distance`` 1: every
    (world, action)'s rows by decreasing column 11 (the decision's order), 0: as they lie."""
    if net.family is not RECURRENT:
        raise ValueError("decide_lstm: the network is not an LSTM-RL one (lstm_rl.ValueNetwork1 / ValueNetwork2)")
    decide_rows(net, W, A, n, rotated, sorted_by_distance, rewards, actions, robot, robot_stride, gamma, dt, override, values, choice,
                action_out, stream)


def decide_lstm_bf16(net, W, A, n, sorted_by_distance, rotated, rewards, actions, robot, robot_stride, gamma, dt, override, values, choice,
                     action_out, stream=None):
    """cs_value_net_decide_lstm_bf16 on device pointers (ints): ``decide_lstm`` in the opt-in bf16 arithmetic, for a DeviceNet of an LSTM-RL
    network without map columns whose recurrent bf16 blob is current (``refresh_recurrent("bf16")``)."""
    if net.family is not RECURRENT:
        raise ValueError("decide_lstm_bf16: the network is not an LSTM-RL one without map columns (lstm_rl.ValueNetwork1 / ValueNetwork2)")
    decide_rows(net, W, A, n, rotated, sorted_by_distance, rewards, actions, robot, robot_stride, gamma, dt, override, values, choice,
                action_out, stream, own=True)


def decide_lstm_om(net, W, A, n, sorted_by_distance, rotated, maps, rewards, actions, robot, robot_stride, gamma, dt, override, values, choice,
                   action_out, stream=None):
    """cs_value_net_decide_lstm_om on device pointers (ints): ``decide_lstm`` for a DeviceNet of an OM-LSTM-RL network, maps
    [W][n][net.om_cols] paired with the rows by ``net.map_order``."""
    if net.family is not RECURRENT_MAPPED:
        raise ValueError("decide_lstm_om: the network is not an LSTM-RL one with occupancy-map columns (DeviceNet(model, cols, om_cols))")
    decide_rows(net, W, A, n, rotated, (maps, sorted_by_distance), rewards, actions, robot, robot_stride, gamma, dt, override, values, choice,
                action_out, stream)


def decide_lstm_om_bf16(net, W, A, n, sorted_by_distance, rotated, maps, rewards, actions, robot, robot_stride, gamma, dt, override, values,
                        choice, action_out, stream=None):
    """cs_value_net_decide_lstm_om_bf16 on device pointers (ints): ``decide_lstm_om`` in the opt-in bf16 arithmetic, for a DeviceNet of an
    OM-LSTM-RL network whose bf16 blob is current (``refresh_mapped("bf16")``); the pairing is ``net.map_order``."""
    if net.family is not RECURRENT_MAPPED:
        raise ValueError("decide_lstm_om_bf16: the network is not an LSTM-RL one with occupancy-map columns (DeviceNet(model, cols, om_cols))")
    decide_rows(net, W, A, n, rotated, (maps, sorted_by_distance), rewards, actions, robot, robot_stride, gamma, dt, override, values, choice,
                action_out, stream, own=True)


def _extra_input(net, humans, vel_col, in_order, stream):
    """What ``decide_rows`` takes as `extra` for `net`: (the argument, the tensor behind it or None) -- the maps of `humans` [W, n, stride]
    for a family with maps (a launch), `in_order` as sorted_by_distance for a recurrent one, the pair for a family with both, nothing
    otherwise."""
    ordered = "sorted_by_distance" in net.family.decide_int
    if net.family.takes_maps:
        maps = maps_of(humans, vel_col, net.om_grid, stream)
        return ((maps.data_ptr(), in_order) if ordered else maps.data_ptr()), maps
    return (in_order if ordered else None), None


_ROWS_BLOB = {}


def rotated_rows(cur, robot, stream=None):
    """The rotated joint states [W, n, 13 | 15] of the worlds' CURRENT state (cur [W, n, 5 | 7], robot [W, 8+], CUDA tensors), written by
    cs_value_net_state's loader: the entry is given a one-layer network of zero weights, whose value nobody reads."""
    import torch

    from ... import _lib

    W, n, cc = cur.shape
    cols = 15 if cc == 7 else 13
    dims = np.array([1, 1], np.int32)
    key = (cols, torch.cuda.current_device())
    if key not in _ROWS_BLOB:
        _ROWS_BLOB[key] = torch.from_numpy(pack(CS_VN_CADRL, dims, cols, [np.zeros((1, cols), np.float32), np.zeros(1, np.float32)])).to("cuda")
    rows = torch.empty((W, n, cols), dtype=torch.float32, device="cuda")
    unread = torch.empty(W, dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().cs_value_net_state(*_head((CS_VN_CADRL,), dims, _ROWS_BLOB[key]), W, n, cc == 7, cur.data_ptr(), robot.data_ptr(),
                                              robot.shape[1], None, 1.0, 0.0, rows.data_ptr(), unread.data_ptr(), stream))
    return rows


def state_values_for_worlds(net, cur, robot, rewards, gamma, dt, want_rows, stream=None):
    """The network on the worlds' CURRENT state, for a trainer: (values [W] = rewards + gamma^(dt * v_pref) * V, rows [W, n, cols
    (+ om_cols)] -- what ``transform`` gives per world -- or None).  CUDA tensors cur [W, n, 5 | 7], robot [W, 8+], rewards [W] or None (0).
    A feed-forward network takes one launch (``state_values``) and makes the rows only when asked.  The other families compose it, rows
    in any case: the maps of the CURRENT humans where the family has maps, the rotated rows (``rotated_rows``), and the family's decide
    entry on them as they lie (sorted_by_distance = 0) with A = 1 -- a one-row action table, no choice, a scratch action row."""
    import torch

    W, n, cc = cur.shape
    if net.family.state_launch:
        values = torch.empty(W, dtype=torch.float32, device="cuda")
        rows = torch.empty((W, n, net.cols), dtype=torch.float32, device="cuda") if want_rows else None
        state_values(net, W, n, cc == 7, cur.data_ptr(), robot.data_ptr(), robot.shape[1], None if rewards is None else rewards.data_ptr(), gamma, dt,
                     None if rows is None else rows.data_ptr(), values.data_ptr(), stream)
        return values, rows
    extra, maps = _extra_input(net, cur, 2, 0, stream)
    rows = rotated_rows(cur, robot, stream)
    values = torch.empty(W, dtype=torch.float32, device="cuda")
    zeros = torch.zeros(max(W, 2), dtype=torch.float32, device="cuda")     # the null rewards; its first two floats the one-row action table
    scratch = torch.empty((W, 2), dtype=torch.float32, device="cuda")
    rew = rewards if rewards is not None else zeros
    decide_rows(net, W, 1, n, rows.data_ptr(), extra, rew.data_ptr(), zeros.data_ptr(), robot.data_ptr(), robot.shape[1],
                gamma, dt, None, values.data_ptr(), None, scratch.data_ptr(), stream)
    return values, rows if maps is None else torch.cat([rows, maps], dim=2)


def _check_cols_headed(caller, net, headed):
    """The entries that generate their rows take `headed` beside the network: its 13 or 15 input columns must say the same."""
    if net.cols != (15 if headed else 13):
        raise ValueError(f"{caller}: a network of {net.cols} input columns and headed={bool(headed)} differ")


def decide_worlds(net, W, A, n, headed, actions, nxt, cur, robot, robot_stride, gamma, dt, override, rewards_out, values, choice, action_out,
                  stream=None):
    """cs_value_net_decide_worlds on device pointers (ints): the decision of ``decide`` from the worlds' own rows -- what cs_lookahead takes
    (actions [A][2], nxt [W][n][4|6], cur [W][n][5|7], robot [W][robot_stride]) -- without the look-ahead tensor.  `net` a DeviceNet whose
    float32 blob is current and whose cols match `headed`; rewards_out [W][A] or None."""
    from ... import _lib

    head = net.head("decide_worlds")
    _check_cols_headed("decide_worlds", net, headed)
    _lib.check(_lib.load().cs_value_net_decide_worlds(*head, W, A, n, bool(headed), actions, nxt, cur, robot, robot_stride, gamma, dt, override,
                                                      rewards_out, values, choice, action_out, stream))


def _decide_lstm_worlds(caller, precision, net, W, A, n, headed, sorted_by_distance, actions, nxt, cur, robot, robot_stride, gamma, dt, override,
                        rewards_out, values, choice, action_out, stream):
    """The RECURRENT row's worlds entry of recurrent precision `precision`, on that arithmetic's blob."""
    from ... import _lib

    if net.family is not RECURRENT:
        raise ValueError(f"{caller}: the network is not an LSTM-RL one without map columns (lstm_rl.ValueNetwork1 / ValueNetwork2)")
    _check_cols_headed(caller, net, headed)
    if precision == "f32":
        head = net.head(caller)
    else:
        blob = net.blobs[net.family.own.key]
        if blob is None:
            raise ValueError(f"{caller}: {net.family.own.no_blob}")
        head = _head((), net.dims, blob)
    _lib.check(getattr(_lib.load(), net.family.worlds[precision])(*head, W, A, n, bool(headed), int(bool(sorted_by_distance)), actions, nxt, cur, robot,
                                                                  robot_stride, gamma, dt, override, rewards_out, values, choice, action_out, stream))


def decide_lstm_worlds(net, W, A, n, headed, sorted_by_distance, actions, nxt, cur, robot, robot_stride, gamma, dt, override, rewards_out, values,
                       choice, action_out, stream=None):
    """cs_value_net_decide_lstm_worlds on device pointers (ints): the decision of ``decide_lstm`` from the worlds' own rows -- what
    cs_lookahead takes (actions [A][2], nxt [W][n][4|6], cur [W][n][5|7], robot [W][robot_stride]) -- without the look-ahead tensor, bit
    for bit.  `net` a DeviceNet of an LSTM-RL network whose float32 blob is current and whose cols match `headed`; rewards_out [W][A] or
    None."""
    _decide_lstm_worlds("decide_lstm_worlds", "f32", net, W, A, n, headed, sorted_by_distance, actions, nxt, cur, robot, robot_stride, gamma, dt,
                        override, rewards_out, values, choice, action_out, stream)


def decide_lstm_worlds_bf16(net, W, A, n, headed, sorted_by_distance, actions, nxt, cur, robot, robot_stride, gamma, dt, override, rewards_out,
                            values, choice, action_out, stream=None):
    """cs_value_net_decide_lstm_worlds_bf16 on device pointers (ints): ``decide_lstm_worlds`` in the opt-in bf16 arithmetic -- the decision
    of ``decide_lstm_bf16``, bit for bit --, for a DeviceNet whose recurrent bf16 blob is current (``refresh_recurrent("bf16")``)."""
    _decide_lstm_worlds("decide_lstm_worlds_bf16", "bf16", net, W, A, n, headed, sorted_by_distance, actions, nxt, cur, robot, robot_stride, gamma,
                        dt, override, rewards_out, values, choice, action_out, stream)


def state_values(net, W, n, headed, cur, robot, robot_stride, rewards, gamma, dt, rotated_out, values, stream=None):
    """cs_value_net_state on device pointers (ints): the network on the worlds' CURRENT state, for a trainer -- cur [W][n][5|7], robot
    [W][robot_stride] as cs_lookahead takes them; rotated_out [W][n][13|15] or None receives the rotated joint states (``transform``),
    values [W] = rewards[w] + gamma^(dt * v_pref) * V(w), rewards [W] or None (0): with None and dt = 0 the network's own output.  `net` a
    DeviceNet whose float32 blob is current and whose cols match `headed`."""
    from ... import _lib

    head = net.head("state_values")
    _check_cols_headed("state_values", net, headed)
    _lib.check(_lib.load().cs_value_net_state(*head, W, n, bool(headed), cur, robot, robot_stride, rewards, gamma, dt, rotated_out, values,
                                              stream))


def lookahead(acts, nxt, cur, robot, dt, stream=None):
    """cs_lookahead on CUDA tensors: actions [A, 2], next humans [W, n, 4 | 6], current humans [W, n, 5 | 7], robot rows [W, 8+] ->
    (rotated [W, A, n, 13 | 15], rewards [W, A]), allocated here and written on `stream` (an int)."""
    import torch

    from ... import _lib

    (W, n, cc), A = cur.shape, acts.shape[0]
    rot = torch.empty((W, A, n, 15 if cc == 7 else 13), dtype=torch.float32, device="cuda")
    rew = torch.empty((W, A), dtype=torch.float32, device="cuda")
    _lib.check(_lib.load().cs_lookahead(W, n, A, cc == 7, acts.data_ptr(), nxt.data_ptr(), cur.data_ptr(), robot.data_ptr(), robot.shape[1], dt,
                                        rot.data_ptr(), rew.data_ptr(), stream))
    return rot, rew


def decide_for_worlds(net, decision_input, precision, acts, nxt, cur, robot, gamma, dt, override, values, choice, action_out, stream=None,
                      recurrent_precision="f32", mapped_precision="f32", wide_precision="f32", recurrent_input="tensor"):
    """The decision of W robots from their worlds' rows (CUDA tensors as ``lookahead`` takes them; override int32 [W] or None; the outputs
    values [W, A], choice [W], action_out [W, 2]), on `stream` (an int): "fused" is decide_worlds alone; "tensor" is lookahead, then
    the family's decide entry with `precision` -- a recurrent net in the decision's order; a net with map columns on occupancy_maps of the
    NEXT humans (the maps the reference's serial branch builds, once per decision; with the net's ``map_order``), which it keeps in
    ``net.last_maps``.  ``recurrent_precision`` / ``mapped_precision`` / ``wide_precision`` "bf16" (the net of that family alone, whose
    ``refresh_recurrent`` / ``refresh_mapped`` / ``refresh_wide("bf16")`` blob is current): the same sequence with the family's own
    arithmetic.  ``recurrent_input`` "fused" (RECURRENT_INPUTS; a recurrent net without map columns alone): one library call on the
    worlds' own rows in either recurrent precision, ``decide_lstm_worlds`` or ``decide_lstm_worlds_bf16``, and no look-ahead tensor.
    Returns (rotated, rewards), the look-ahead tensors it allocated and the launches read -- (None, None) for either "fused"."""
    (W, n, cc), A = cur.shape, acts.shape[0]
    ovr = None if override is None else override.data_ptr()
    if check_recurrent_input(recurrent_input, net.family) == "fused":
        # (a recurrent net without map columns: what the tensor path refuses of the other families' arguments is refused here too)
        check_mapped_precision(mapped_precision, net.family)
        check_wide_precision(wide_precision, net.family)
        check_mode(net.family, decision_input, precision)
        fused = decide_lstm_worlds if check_recurrent_precision(recurrent_precision, net.family) == "f32" else decide_lstm_worlds_bf16
        fused(net, W, A, n, cc == 7, 1, acts.data_ptr(), nxt.data_ptr(), cur.data_ptr(), robot.data_ptr(), robot.shape[1], gamma, dt, ovr, None,
              values.data_ptr(), choice.data_ptr(), action_out.data_ptr(), stream)
        return None, None
    # (the order of these checks is which refusal a caller with several bad arguments sees: the mapped precision; with it "bf16" the mode in
    # front of the recurrent precision, else behind it)
    own = check_mapped_precision(mapped_precision, net.family) == "bf16"
    if own:
        check_mode(net.family, decision_input, precision)
    own = check_recurrent_precision(recurrent_precision, net.family) == "bf16" or own
    own = check_wide_precision(wide_precision, net.family) == "bf16" or own
    if check_mode(net.family, decision_input, precision) == "fused":      # one library call on the worlds' own rows
        decide_worlds(net, W, A, n, cc == 7, acts.data_ptr(), nxt.data_ptr(), cur.data_ptr(), robot.data_ptr(), robot.shape[1], gamma, dt, ovr,
                      None, values.data_ptr(), choice.data_ptr(), action_out.data_ptr(), stream)
        return None, None
    rot, rew = lookahead(acts, nxt, cur, robot, dt, stream)
    extra, maps = _extra_input(net, nxt, 3 if cc == 7 else 2, 1, stream)
    if maps is not None:
        net.last_maps = maps
    decide_rows(net, W, A, n, rot.data_ptr(), extra, rew.data_ptr(), acts.data_ptr(), robot.data_ptr(), robot.shape[1], gamma, dt,
                ovr, values.data_ptr(), choice.data_ptr(), action_out.data_ptr(), stream, precision=precision, own=own)
    return rot, rew
