"""policy_factory with the reference's keys (crowd_nav/policy_no_train/policy_factory.py).

'socialforce' needs the socialforce library, which this project does not ship and nothing here can pin it against.  'orca' needs rvo2 in
the reference; its decision runs here as crowd_nav.policy.policy_factory["orca_device"] (orca.py, csrc/policy_orca.hip), pinned bit for bit on
the project's float32 restatement of RVO2 -- parity with the third-party library itself stays unpinned, as for every ORCA
path here -- and this factory's 'orca' key keeps raising, with a pointer there.  The 'hsfm_*' policies fail inside the reference itself (FullState has no 'w': hsfm_farina.py:61; their ActionXYW would then fail
RobotAgent.check_validity) -- tests/golden/g18_policy_no_train.npz records that exception.  Those keys raise NotImplementedError."""
from .blind_planner import BlindPlanner
from .sfm_guo import SFMGuo
from .sfm_helbing import SFMHelbing
from .sfm_moussaid import SFMMoussaid
from .simple_social_planner import SimpleSocialPlanner


def none_policy():
    return None


def _unsupported(name, reason):
    def make(*args, **kwargs):
        raise NotImplementedError(f"no-train policy {name!r} is not available: {reason}")
    make.__name__ = name
    make.reason = reason
    return make


_NO_LIBRARY = "it needs the {} library, which is not part of this project, so there is nothing to pin it against"
_HSFM_BROKEN = ("the reference's HSFM robot policies fail in predict ('FullState' object has no attribute 'w') and their ActionXYW "
                "fails RobotAgent.check_validity")

policy_factory = dict()
policy_factory["none"] = none_policy
policy_factory["bp"] = BlindPlanner
policy_factory["ssp"] = SimpleSocialPlanner
policy_factory["orca"] = _unsupported("orca", "under this key it needs the rvo2 library, which is not part of this project; the same decision on the "
                                               "project's float32 restatement of RVO2 is crowd_nav.policy.policy_factory[\"orca_device\"]")
policy_factory["socialforce"] = _unsupported("socialforce", _NO_LIBRARY.format("socialforce"))
policy_factory["sfm_helbing"] = SFMHelbing
policy_factory["sfm_guo"] = SFMGuo
policy_factory["sfm_moussaid"] = SFMMoussaid
for _name in ("hsfm_farina", "hsfm_guo", "hsfm_moussaid", "hsfm_new", "hsfm_new_guo", "hsfm_new_moussaid"):
    policy_factory[_name] = _unsupported(_name, _HSFM_BROKEN)

SUPPORTED = ("bp", "ssp", "sfm_helbing", "sfm_guo", "sfm_moussaid")
