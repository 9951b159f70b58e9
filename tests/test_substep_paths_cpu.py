"""The inputs of tests/test_gpu_substep_paths.py take their rare events -- asserted on the oracle alone, no GPU: a body overlap in substep 0
and in no later one, a goal list rotated on the incoming row and one rotated in substep 2, a row respawned by the traffic rule.  An input
that stops reaching its block of the substep loop fails here, not silently on the GPU."""
import numpy as np
import pytest

import substep_path_cases as spc


@pytest.mark.parametrize("W,n,robot_row", spc.SHAPES)
@pytest.mark.parametrize("model", spc.MODELS)
def test_contact_in_substep_0_and_none_behind_it(model, W, n, robot_row):
    ev = spc.events("contact", model, W, n, robot_row)
    w, (i, j) = ev["world"], ev["who"]
    assert ev["overlaps_entering"][0] == [(w, (i, j))], ev["overlaps_entering"]
    assert ev["overlaps_entering"][1] == [] and ev["overlaps_entering"][2] == [], ev["overlaps_entering"]
    assert ev["respawned_in"] == [[], [], []], ev["respawned_in"]


@pytest.mark.parametrize("W,n,robot_row", spc.SHAPES)
@pytest.mark.parametrize("model", spc.MODELS)
def test_goal_lists_rotate_on_the_incoming_row_and_in_substep_2(model, W, n, robot_row):
    ev = spc.events("goals", model, W, n, robot_row)
    w, (first, later) = ev["world"], ev["who"]
    assert ev["rotated_in"][0] == [(w, first)], ev["rotated_in"]
    assert ev["rotated_in"][1] == [], ev["rotated_in"]
    assert ev["rotated_in"][2] == [(w, later)], ev["rotated_in"]
    assert ev["overlaps_entering"] == [[], [], []], ev["overlaps_entering"]


@pytest.mark.parametrize("W,n,robot_row", spc.SHAPES)
@pytest.mark.parametrize("model", spc.MODELS)
def test_a_row_is_respawned_by_the_traffic_rule(model, W, n, robot_row):
    ev = spc.events("respawn", model, W, n, robot_row)
    w, (i,) = ev["world"], ev["who"]
    assert w % 2 == 1
    assert ev["respawned_in"][0] == [] and ev["respawned_in"][1] == [(w, i)] and ev["respawned_in"][2] == [], ev["respawned_in"]
    assert ev["overlaps_entering"] == [[], [], []], ev["overlaps_entering"]


def test_the_cases_are_float32_and_handed_out_as_copies():
    a = spc.case("contact", "hsfm_farina", 2, 25)
    a[0][:] = 0
    b = spc.case("contact", "hsfm_farina", 2, 25)
    assert b[0].dtype == np.float32 and b[0][..., 8].min() > 0
