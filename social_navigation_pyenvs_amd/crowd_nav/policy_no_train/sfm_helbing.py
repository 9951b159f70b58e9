"""Social-force robot, Helbing's pair law (reference: crowd_nav/policy_no_train/sfm_helbing.py, forces.py)."""
from .policy import CS_PNT_SFM_HELBING, NoTrainPolicy


class SFMHelbing(NoTrainPolicy):
    pnt_id = CS_PNT_SFM_HELBING

    def __init__(self):
        super().__init__()
        self.name = "sfm_helbing"
        self.trainable = False
        self.multiagent_training = None
        self.kinematics = "holonomic"
        self.params = {"relaxation_time": 0.5, "Ai": 2000.0, "Aw": 2000.0, "Bi": 0.08, "Bw": 0.08, "k1": 120000.0, "k2": 240000.0,
                       "mass": 80}

    def set_phase(self, phase):
        return
