"""Blind planner (reference: crowd_nav/policy_no_train/blind_planner.py): straight to the goal at v_pref."""
from .policy import CS_PNT_BP, NoTrainPolicy


class BlindPlanner(NoTrainPolicy):
    pnt_id = CS_PNT_BP

    def __init__(self):
        super().__init__()
        self.name = "bp"
        self.trainable = False
        self.kinematics = "holonomic"
        self.multiagent_training = True
