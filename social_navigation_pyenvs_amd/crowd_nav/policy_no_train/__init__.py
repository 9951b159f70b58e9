"""The CrowdNav baseline robot policies that need no training (reference: crowd_nav/policy_no_train/): blind planner, simple
social planner and the three social-force robots, each ``predict`` one launch of csrc/policy_no_train.hip."""
