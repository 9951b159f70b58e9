"""policy_factory with the reference's keys (crowd_nav/policy/policy_factory.py): the no-train policies plus the trained value-based ones."""
from ..policy_no_train.orca import ORCA
from ..policy_no_train.policy_factory import policy_factory as _no_train
from .cadrl import CADRL
from .lstm_rl import LstmRL
from .om_lstm_rl import OMLstmRL
from .om_sarl import OMSARL
from .sarl import SARL


def lstm_rl(*args, **kwargs):
    raise NotImplementedError("policy 'lstm_rl' is not available under this key: LSTM-RL runs a recurrent network over the humans sorted by distance, "
                              "which has a decision kernel of its own; build it with policy_factory[\"lstm_rl_device\"]")


policy_factory = dict(_no_train)
policy_factory["cadrl"] = CADRL
policy_factory["sarl"] = SARL
policy_factory["om_sarl"] = OMSARL
policy_factory["lstm_rl"] = lstm_rl
policy_factory["lstm_rl_device"] = LstmRL
policy_factory["om_lstm_rl"] = OMLstmRL
# the ORCA robot on the device (csrc/policy_orca.hip); "orca" itself keeps the no-train factory's refusal, which points here
policy_factory["orca_device"] = ORCA
