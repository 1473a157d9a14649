"""The oracle against the reference on the action table (CPU): every case of tests/act_table.py replayed on OracleEnv and held
to tests/golden/acttable.npz (tests/golden/make_act_table.py: the reference's run of the same cases) — canonical state and
grid.encode() of every step, the float64 rewards exactly, `done`, the shuffled order, the class of the exception raised.  A
script ends at the step that raised, and nothing is compared at or after it but the exception (the state after a mid-loop
exception depends on where in the shuffled order it struck).  Which cases raise is listed by name in act_table.py: a case
cannot pass by raising."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import act_table as A  # noqa: E402
import canon  # noqa: E402

GOLD = os.path.join(HERE, "golden", "acttable.npz")


@pytest.fixture(scope="module")
def table():
    return A.cases()


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_the_enumeration(table, gold):
    """the exact counts, ragged batches, all four directions in every group, and the fixture is of THESE cases"""
    assert {v: len(b) for v, b in table.items()} == A.COUNTS == {"default": 2518, "noghost": 300, "respawn": 10}
    groups = {}
    for v, batch in table.items():
        assert len(batch) % 8 and len(batch) % 64
        assert list(gold["%s/names" % v]) == [c.name for c in batch]
        for i, c in enumerate(batch):
            assert c.d == i % 4 and c.agents[0] == (A.CX, A.CY, c.d) and 1 <= len(c.actions) <= A.STEPS
            groups.setdefault(c.name.split("/")[0], []).append(c)
    assert {g: len(cs) for g, cs in groups.items()} == {"S": 2400, "T": 44, "R": 64, "G": 300, "P": 20}
    for g, cs in groups.items():
        assert {c.d for c in cs} == {0, 1, 2, 3}, g
    s = groups["S"]
    assert len({(c.actions[0][0], c.d) for c in s}) == 32           # every action in every direction
    assert os.path.getsize(GOLD) < 630000


def test_the_cases_that_raise_are_the_listed_ones(table, gold):
    got = {}
    for v, batch in table.items():
        err, steps = gold["%s/error" % v], gold["%s/steps" % v]
        for b, c in enumerate(batch):
            hit = [(t, str(err[b, t])) for t in range(A.STEPS) if str(err[b, t])]
            assert len(hit) <= 1
            if hit:
                got[c.name] = hit[0]
                assert steps[b] == hit[0][0] + 1, c.name            # the script ended at its error step
            else:
                assert steps[b] == len(c.actions), c.name
    assert got == A.expected_errors()
    by_class = {}
    for _, e in got.values():
        by_class[e] = by_class.get(e, 0) + 1
    assert by_class == {"ValueError": 300, "TypeError": 20, "AssertionError": 4 + len(A.RACE_OUT_ERRORS)}


@pytest.mark.parametrize("variant", sorted(A.VARIANTS))
def test_oracle_replays_the_reference(table, gold, variant):
    batch = table[variant]
    g = {k: gold["%s/%s" % (variant, k)] for k in ("rewards", "env_done", "order", "steps", "error", "encode", "step_count")
         + canon.KEYS[:-1]}
    envs = A.oracle_envs(batch)
    for b, (c, e) in enumerate(zip(batch, envs)):
        for t, act in enumerate(c.actions):
            what = "%s step %d" % (c.name, t)
            rew, done, order, err = A.oracle_step(e, act)
            assert err == str(g["error"][b, t]), what
            if err:
                assert t + 1 == g["steps"][b], what
                break
            st = canon.oracle_canonical(e)
            for k in canon.KEYS[:-1]:
                assert np.array_equal(np.asarray(st[k]), g[k][b, t]), (what, k, st[k], g[k][b, t])
            assert st["step_count"] == g["step_count"][b, t] == t + 1, what
            assert np.array_equal(e.encode(), g["encode"][b, t]), what
            assert np.array_equal(rew, g["rewards"][b, t]), (what, rew, g["rewards"][b, t])
            assert done == bool(g["env_done"][b, t]), what
            assert np.array_equal(order, g["order"][b, t]), what
        else:
            assert g["steps"][b] == len(c.actions), c.name


def test_races_take_both_orders(table):
    """per race, over its seeds, the oracle runs agent 0 before agent 1 and agent 1 before agent 0; the outcomes differ between
    the orders in every race but unlock-against-forward (a door that was locked is closed, not open, after the unlock)"""
    races = {r: [c for c in table["default"] if c.name.startswith("R/%s/" % r)] for r in A.RACES}
    errors = []
    for race, cs in races.items():
        assert len(cs) == A.RACE_SEEDS
        seen = {}
        for c, e in zip(cs, A.oracle_envs(cs)):
            _, _, order, err = _step_with_order(e, c.actions[0])
            order = list(order)
            first = order.index(0) < order.index(1)
            st = e.state()              # the outcome, whichever way the scene is turned
            outcome = (err, tuple(st["pos"][0]) != (A.CX, A.CY), tuple(st["carrying"]), int(st["base"][c.front()]),
                       int(st["base"][A.CX, A.CY]))
            seen.setdefault(first, set()).add(outcome)
            if err:
                errors.append(c.name)
                assert race == "out-of-door-vs-shut" and not first
        assert set(seen) == {True, False}, (race, "one order only")
        assert all(len(v) == 1 for v in seen.values()), race        # the order decides, nothing else does
        assert (seen[True] != seen[False]) == (race != "unlock-vs-forward"), race
    assert errors == ["R/out-of-door-vs-shut/%d" % i for i in A.RACE_OUT_ERRORS]


def _step_with_order(e, acts):
    """oracle_step, with the order also where the step raised (the oracle writes it before the loop)"""
    import ctypes as C
    from oracle import oracle as O
    a = np.ascontiguousarray(acts, dtype=np.int32)
    rew, done, order = np.zeros(e.n, np.float64), C.c_int32(0), np.zeros(e.n, np.int32)
    rc = e.L.mgo_step(e.h, O._p(a, C.c_int32), O._p(rew, C.c_double), C.byref(done), O._p(order, C.c_int32))
    return rew, bool(done.value), order, ("" if rc == 0 else O._ERR[rc].__name__)
