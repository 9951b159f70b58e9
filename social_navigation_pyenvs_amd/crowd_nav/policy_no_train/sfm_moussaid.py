"""Social-force robot, Moussaid's pair law (reference: crowd_nav/policy_no_train/sfm_moussaid.py, forces.py)."""
from .policy import CS_PNT_SFM_MOUSSAID, NoTrainPolicy


class SFMMoussaid(NoTrainPolicy):
    pnt_id = CS_PNT_SFM_MOUSSAID

    def __init__(self):
        super().__init__()
        self.name = "sfm_moussaid"
        self.trainable = False
        self.multiagent_training = None
        self.kinematics = "holonomic"
        self.params = {"relaxation_time": 0.5, "Ei": 360, "agent_lambda": 2.0, "gamma": 0.35, "ns": 2.0, "ns1": 3.0, "Aw": 2000.0,
                       "Bw": 0.08, "k1": 120000.0, "k2": 240000.0, "mass": 80}

    def set_phase(self, phase):
        return
