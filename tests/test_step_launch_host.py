"""Which library calls a step makes, held to the table recorded before the choice had a module of its own (no GPU, no library:
tests/step_launch_cases.py has the matrix, the harness and how tests/golden/step_launch.json was recorded).  The file passes on
the commit that recorded the table, too, where it drives the old ladder: the table is a statement about behaviour."""
import json
import os

import pytest

import step_launch_cases as SC


@pytest.fixture(scope="module")
def golden():
    with open(SC.GOLDEN) as f:
        return json.load(f)


def test_the_table_covers_the_matrix(golden):
    assert golden["axes"] == [[k, list(v)] for k, v in SC.AXES]
    assert len(SC.ROWS) == 6912 and len(golden["rows"]) == len(SC.ROWS)
    assert len(golden["swaps"]) == len(SC.SWAPS) == 18
    used = set(golden["rows"]) | set(golden["swaps"])
    assert used == set(range(len(golden["outcomes"])))


def test_every_row_is_reproduced(golden):
    bad = [(row, SC.run(row), golden["outcomes"][k]) for row, k in zip(SC.ROWS, golden["rows"]) if SC.run(row) != golden["outcomes"][k]]
    assert not bad, (len(bad), bad[0])


def test_the_choice_is_made_again_after_release_spec(golden):
    through_a_handle = 0
    for row, k in zip(SC.SWAPS, golden["swaps"]):
        steps, latches = got = SC.run(row, swap=True)
        assert got == golden["outcomes"][k], (row, got, golden["outcomes"][k])
        # a launch that goes through a handle: an old one before the release, a new one behind it
        used = [[c.split("#")[1][:2] for c in s if c.startswith("mg_step_render_spec#")] for s in steps]
        assert used[0] == used[1] and used[1] in ([], ["10"]) and used[2] == ["20"] * len(used[1]), (row, steps)
        assert (row[6] != "none") == any(c.startswith("mg_render_spec_release#10") for c in steps[2]), (row, steps)
        through_a_handle += len(used[2])
    assert through_a_handle == 1 + 6        # "plain": the plain step alone; "all": every mix


def test_candidates_alone_name_the_first_call(golden):
    """the pure function of the options, with no library and no env behind it, against the first thing every row without
    refusals does"""
    if not os.path.exists(os.path.join(os.path.dirname(SC.HERE), "marlgrid_amd", "step_launch.py")):
        pytest.skip("the commit that recorded the table: the choice has no module of its own yet")
    from marlgrid_amd import step_launch as SL
    n = 0
    for row, k in zip(SC.ROWS, golden["rows"]):
        obs_delta, episode, encode, fused, groups, fmt, spec, refused = row
        if refused:
            continue
        has = {"none": (), "plain": (0,), "all": (0, 1, 2)}[spec] if fmt == "image" else ()
        kind = SL.candidates(obs_delta, episode is not None, encode, fused, groups == 2, fmt == "encoded", lambda w: w in has)[0]
        first = golden["outcomes"][k][0][0][0]
        if kind.call is None:
            assert first == "raise: " + kind.demand, (row, first)
        else:
            assert first.split("|")[0].split("#")[0] == kind.call, (row, first, kind.call)
            assert ("#" in first) == (kind.want is not None), (row, first)
        n += 1
    assert n == len(SC.ROWS) // 16
