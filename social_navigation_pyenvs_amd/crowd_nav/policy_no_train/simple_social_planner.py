"""Simple social planner (reference: crowd_nav/policy_no_train/simple_social_planner.py): the blind planner's action, or a stop as soon
as one human's surface distance is at most DISTANCE_THRESHOLD."""
from .policy import CS_PNT_SSP, NoTrainPolicy

DISTANCE_THRESHOLD = 0.2


class SimpleSocialPlanner(NoTrainPolicy):
    pnt_id = CS_PNT_SSP

    def __init__(self):
        super().__init__()
        self.name = "ssp"
        self.trainable = False
        self.kinematics = "holonomic"
        self.multiagent_training = True
