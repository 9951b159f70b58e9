"""Social-force robot, Guo's pair law (reference: crowd_nav/policy_no_train/sfm_guo.py, forces.py)."""
from .policy import CS_PNT_SFM_GUO, NoTrainPolicy


class SFMGuo(NoTrainPolicy):
    pnt_id = CS_PNT_SFM_GUO

    def __init__(self):
        super().__init__()
        self.name = "sfm_guo"
        self.trainable = False
        self.multiagent_training = None
        self.kinematics = "holonomic"
        self.params = {"relaxation_time": 0.5, "Ai": 2000.0, "Aw": 2000.0, "Bi": 0.08, "Bw": 0.08, "Ci": 120.0, "Cw": 120.0, "Di": 0.6,
                       "Dw": 0.6, "k1": 120000.0, "k2": 240000.0, "mass": 80}

    def set_phase(self, phase):
        return
