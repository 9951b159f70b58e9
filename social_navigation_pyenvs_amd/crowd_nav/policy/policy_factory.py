"""policy_factory with the reference's keys (crowd_nav/policy/policy_factory.py): the no-train policies plus the trained value-based ones."""
from ..policy_no_train.policy_factory import policy_factory as _no_train
from .cadrl import CADRL
from .om_sarl import OMSARL
from .sarl import SARL


def lstm_rl(*args, **kwargs):
    raise NotImplementedError("policy 'lstm_rl' is not available: LSTM-RL runs a recurrent network over the humans sorted by distance; the "
                              "fused decision kernel covers the feed-forward CADRL and SARL networks only")


policy_factory = dict(_no_train)
policy_factory["cadrl"] = CADRL
policy_factory["sarl"] = SARL
policy_factory["om_sarl"] = OMSARL
policy_factory["lstm_rl"] = lstm_rl
