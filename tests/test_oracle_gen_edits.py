"""CPU: the oracle's edit list (oracle/mg_oracle.c: mgo_set_edits, the loop behind the `_gen_grid` program) pinned BEFORE anything
is held to it.  The list is `self.level` of a scenario whose `_gen_grid` ends with `for x, y, o in self.level: self.grid.set(x,
y, o)`: a plain ordered list in the oracle's own data model.

  * against the static twins: `oracle(base spec, set_edits(list))` must do, word for word and state for state, what the oracle
    does with the twin spec that has the same cells as ("put", ...) entries at the end of its program — a path that the
    goldens and the live reference already pin (tests/test_oracle_golden.py, LateStatic) — for the four lists of
    tests/edit_envs.py at K = 4 and 7 and for 24 random lists with a Key and a Ball among the kinds;
  * against the reference's trajectories recorded with such a `_gen_grid` (tests/golden/genedits_*.npz, made by
    tests/golden/make_gen_edits.py);
  * where the reference is present, against the live reference, stepped beside the oracle with random actions."""
import numpy as np
import pytest

import canon
import draw_envs as D
import edit_envs as EE
import level_envs as LE
import viewenc
from golden import refstate  # (crc() only; does not import the reference)
from oracle import oracle as O

REW_TOL = 1e-6
MAX_STEPS = 10


def _same(a, b, what):
    canon.assert_same(canon.oracle_canonical(a), canon.oracle_canonical(b), what)
    assert a.mt_state()[1] == b.mt_state()[1] and np.array_equal(a.mt_state()[0], b.mt_state()[0]), what + ": RNG"
    assert np.array_equal(a.encode(), b.encode()), what + ": encode"
    for va, vb in zip(viewenc.oracle_views(a), viewenc.oracle_views(b)):
        assert np.array_equal(va, vb), what + ": views"


def _lockstep(a, b, T, seed, what):
    """a and b from their first reset on: observations, state, rewards, the shuffle order, encode, views and the RNG after every
    step and reset -> the episodes that ended"""
    assert np.array_equal(a.reset(), b.reset()), what
    _same(a, b, what + " reset")
    rng = np.random.RandomState(seed)
    ends = 0
    for t in range(T):
        act = rng.randint(0, 7, size=a.n)
        oa, ra, da, _, orda = a.step(act, return_order=True)
        ob, rb, db, _, ordb = b.step(act, return_order=True)
        w = "%s step %d" % (what, t)
        assert da == db and np.array_equal(ra, rb) and np.array_equal(orda, ordb), w
        assert np.array_equal(oa, ob), w
        _same(a, b, w)
        if da:
            ends += 1
            assert np.array_equal(a.reset(), b.reset()), w
            _same(a, b, w + ": reset after it")
    return ends


def _twin_spec(base, lst):
    s = dict(base)
    fills = [("put", k, x, y) for x, y, k in lst]
    s["gen_ctor"], s["gen_reset"] = list(base["gen_ctor"]) + fills, list(base["gen_reset"]) + fills
    return s


TWINS = [(K, i) for K in (4, 7) for i in range(4)]


@pytest.mark.parametrize("K,i", TWINS, ids=["K%d-L%d" % c for c in TWINS])
def test_edit_list_equals_the_static_twin(K, i):
    """the four lists of tests/edit_envs.py: the hand-written twin spec EE.spec(i, K) against the base scenario with the list.
    (Neither env runs the constructor's reset: a twin makes it with its fills, an edits env with an empty list.)"""
    base = LE.edits_spec(MAX_STEPS)
    lst = LE.oracle_list(np.asarray(EE.lists(K)[i], np.int64).reshape(-1, 4), len(base["objects"]))
    assert lst == [(x, y, k) for x, y, k, on in EE.lists(K)[i] if on]
    for seed in (21, 22, 23):
        a = O.OracleEnv(base, seed=seed, construct=False)
        b = O.OracleEnv(EE.spec(i, K, max_steps=MAX_STEPS), seed=seed, construct=False)
        a.set_edits(lst)
        assert a.edits() == lst
        assert _lockstep(a, b, 45, seed, "K %d list %d seed %d" % (K, i, seed)) >= 3


@pytest.mark.parametrize("j", range(24))
def test_random_list_equals_its_static_twin(j):
    """random valid lists over None, Wall, Goal, the Key and the Ball, up to 7 entries; cells may repeat"""
    base = LE.edits_spec(MAX_STEPS)
    rng = np.random.RandomState(900 + j)
    lst = LE.random_list(rng, 7)
    if j % 6 == 0 and lst:
        lst = lst + [(lst[0][0], lst[0][1], (lst[0][2] + 1) % 5)]       # one cell twice, whatever was drawn
    a = O.OracleEnv(base, seed=3000 + j, construct=False)
    b = O.OracleEnv(_twin_spec(base, lst), seed=3000 + j, construct=False)
    a.set_edits(lst)
    assert _lockstep(a, b, 45, j, "random list %d %r" % (j, lst)) >= 3


def test_random_lists_reach_every_kind_and_the_full_length():
    lists = [LE.random_list(np.random.RandomState(900 + j), 7) for j in range(24)]
    assert {k for lst in lists for _, _, k in lst} == {0, 1, 2, 3, 4}
    assert max(len(lst) for lst in lists) == 7


def test_a_new_list_waits_for_the_next_reset_and_survives_resets():
    orc = O.OracleEnv(LE.edits_spec(MAX_STEPS), seed=5)
    at = lambda x, y: int(orc.state()["base"][x, y])
    assert orc.edits() == []
    orc.reset()
    assert at(13, 13) == LE.GOAL
    orc.set_edits([(13, 13, 0), (7, 7, LE.GOAL), (7, 7, LE.KEY)])
    assert at(13, 13) == LE.GOAL and at(7, 7) != LE.KEY               # the running episode is untouched
    orc.step([6, 6, 6])
    assert at(13, 13) == LE.GOAL
    for _ in range(3):                                                 # ... and the list stays until another is given
        orc.reset()
        assert at(13, 13) == 0 and at(7, 7) == LE.KEY                  # in list order: the later entry of a cell wins
    orc.set_edits([])
    assert at(7, 7) == LE.KEY
    orc.reset()
    assert at(13, 13) == LE.GOAL and at(7, 7) != LE.KEY and orc.edits() == []


def test_edits_are_applied_after_the_program_and_before_the_agents():
    """a cleared cell is empty whatever the clutter put there, and no agent is ever evicted: the agents are placed afterwards —
    on cells the list emptied, too"""
    spec = LE.edits_spec(MAX_STEPS)
    cells = [(x, y) for x in range(1, 14) for y in range(1, 14) if (x, y) != (13, 13)]
    walls_all = LE.oracle_list([(x, y, LE.WALL, 1) for x, y in cells[:150]], 5)
    for seed in range(6):
        orc = O.OracleEnv(spec, seed=seed)
        orc.set_edits([(x, y, 0) for x, y in cells])
        orc.reset()
        st = orc.state()
        assert (st["base"][1:14, 1:14] != 0).sum() == 1 and st["active"].all() and (st["ordinal"] >= 0).all()
        orc.set_edits(walls_all)                                        # 150 of 168 interior cells walled: the agents still fit
        orc.reset()
        st = orc.state()
        assert all(st["base"][x, y] != LE.WALL for x, y in st["pos"]) and (st["ordinal"] >= 0).all()


def test_an_entry_outside_the_grid_is_the_references_assertion():
    for bad in ((15, 3, 1), (3, 15, 1), (-1, 3, 0), (3, -1, 0)):
        orc = O.OracleEnv(LE.edits_spec(MAX_STEPS), seed=1)
        orc.set_edits([(2, 2, 1), bad])
        with pytest.raises(AssertionError):
            orc.reset()
    orc = O.OracleEnv(LE.edits_spec(MAX_STEPS), seed=1)
    orc.set_edits([(2, 2, 5)])                                          # no such object in the scenario's list
    with pytest.raises(ValueError):
        orc.reset()


def test_set_edits_reaches_one_env_of_a_batch():
    batch = O.OracleBatch(LE.edits_spec(MAX_STEPS), [1, 2, 3])
    batch.envs[1].set_edits([(7, 7, LE.BALL)])
    batch.reset()
    assert [int(e.state()["base"][7, 7] == LE.BALL) for e in batch.envs] == [0, 1, 0]


def test_the_rule_for_entries_that_count():
    e = np.array([(1, 2, 1, 1), (1, 2, 1, 0), (15, 2, 1, 1), (1, 15, 1, 1), (1, 2, 5, 1), (14, 14, 4, 255), (0, 0, 0, 1)])
    assert LE.valid(e, 5).tolist() == [True, False, False, False, False, True, True]
    assert LE.garbage_class(e, 5).tolist() == [-1, 0, 1, 2, 3, -1, -1]
    assert LE.oracle_list(e, 5) == [(1, 2, 1), (14, 14, 4), (0, 0, 0)]
    assert LE.valid(np.array([1, 2, 3, 1]), 3) == False                 # noqa: E712  (a kind the env never registered)


# ---- the hand-written specs against the product's description of the same scenarios ------------------------------------------------
def test_hand_written_specs_agree_with_scenario_spec_except_for_the_edits_op():
    """everything but the programs key by key; the programs entry by entry where the product's notation is the oracle's (the
    curriculum's parameter and its symbolic count are two notations: tests/param_envs.py); an edits op, where the product's
    description has one, is the only entry the hand-written program has no counterpart of"""
    for name, kw in ((LE.EDITS, dict(level_edits=7)), (LE.CURRICULUM, dict(level_edits=5))):
        env = LE.build(name, batch_size=1, _dry=True, max_steps=MAX_STEPS, **kw)
        env.reset()
        got, want = LE.spec_of(name, MAX_STEPS), env.scenario_spec()
        for k in got:
            if k not in ("gen_ctor", "gen_reset", "params"):
                assert got[k] == want[k], (name, k, got[k], want[k])
        assert set(want) - set(got) <= {"params"}
        theirs = [g for g in want["gen_reset"] if g[0] != "edits"]
        assert got["gen_ctor"] == want["gen_ctor"] and len(theirs) == len(got["gen_reset"])
        for mine, g in zip(got["gen_reset"], theirs):
            if mine[0] == "param":
                assert g[0] == "param" and g[1] == mine[1] == 0 and tuple(g[3:5]) == (0, LE.N_CLUTTER_HI), g
            elif mine[0] == "place" and isinstance(mine[2], tuple):
                assert g[0] == "place" and g[1] == mine[1] and D.decode_operand(g[2]) == mine[2] and g[3] == mine[3], g
            else:
                assert tuple(g) == tuple(mine), (name, g, mine)
    env = LE.build(LE.CURRICULUM, batch_size=1, _dry=True)
    d = env._params.decl["n_clutter"]
    assert (d["lo"], d["hi"], d["default"], d["col"]) == (0, LE.N_CLUTTER_HI, LE.N_CLUTTER_DEFAULT, 0)


# ---- the reference's trajectories --------------------------------------------------------------------------------------------------
def _digest(orc):
    return D.rng_digest(orc.mt_state())


@pytest.mark.parametrize("name", sorted(LE.PINNED))
def test_oracle_replays_golden(name):
    g = LE.golden(name)
    level, pixels = LE.PINNED[name]
    assert [tuple(int(v) for v in row) for row in g["level"]] == list(level)
    spec = LE.edits_spec(LE.PIN_MAX_STEPS)
    S, T, n = g["actions"].shape
    assert (S, T) == (len(LE.PIN_SEEDS), LE.PIN_STEPS) and ("obs_crc" in g) == pixels
    vsteps = set(int(v) for v in g["venc_steps"])
    vs = int(g["venc_steps"][1] - g["venc_steps"][0])
    after = iter(g["rng_after_reset"].tolist())

    def views(orc, si, ti, what):
        got = viewenc.oracle_views(orc)
        for k in range(n):
            want = g["venc_reset_a%d" % k][si] if ti is None else g["venc_step_a%d" % k][si, ti]
            assert np.array_equal(got[k], want), (what, "view of agent", k)

    picked = 0
    for si in range(S):
        orc = O.OracleEnv(spec, seed=int(g["seeds"][si]))
        orc.set_edits(level)
        o = orc.reset()
        what = "%s seed %d reset" % (name, si)
        D.cmp_canon(canon.oracle_canonical(orc), g, "reset_", si, None, what)
        assert _digest(orc) == g["rng_reset"][si], what
        views(orc, si, None, what)
        if pixels:
            assert [refstate.crc(x) for x in o] == list(g["obs_crc_reset"][si]), what
        for t in range(T):
            o, r, dn, _, order = orc.step(g["actions"][si, t], return_order=True)
            what = "%s seed %d step %d" % (name, si, t)
            assert np.array_equal(order, g["order"][si, t]), what
            c = canon.oracle_canonical(orc)
            D.cmp_canon(c, g, "step_", si, t, what)
            picked += int(c["carry_enc"].any())
            assert np.abs(r - g["rewards"][si, t]).max() <= REW_TOL and dn == g["ep_done"][si, t], what
            assert np.array_equal(orc.encode(), g["encode"][si, t]), what
            assert _digest(orc) == g["rng_step"][si, t], what
            if t in vsteps:
                views(orc, si, t // vs, what)
            if pixels:
                assert [refstate.crc(x) for x in o] == list(g["obs_crc"][si, t]), what
            if dn:
                orc.reset()
                assert _digest(orc) == next(after), what + ": reset after it"
        if si == 0:
            mt, pos = orc.mt_state()
            assert pos == g["mt_final_pos"] and np.array_equal(mt, g["mt_final"]), name
    assert next(after, None) is None
    if name == "ball-and-key":
        assert picked > 0                                               # something an edit placed was picked up


# ---- beside the live reference -------------------------------------------------------------------------------------------------------
def _same_as_reference(orc, ref, what):
    import refstate as RS
    canon.assert_same(canon.oracle_canonical(orc), dict(RS.canonical(ref)), what)
    rs = ref.np_random.get_state()
    mt, pos = orc.mt_state()
    assert pos == rs[2] and np.array_equal(mt, rs[1]), what + ": RNG"
    assert np.array_equal(orc.encode(), np.asarray(ref.grid.encode(), np.uint8)), what + ": encode"
    for k, a in enumerate(ref.agents):
        gr, vis = ref.gen_obs_grid(a)
        assert np.array_equal(viewenc.oracle_views(orc)[k], np.asarray(gr.encode(vis_mask=vis), np.uint8)), what + ": view %d" % k


LIVE = sorted(LE.PINNED) + ["random-%d" % j for j in range(4)]


@pytest.mark.reference
@pytest.mark.parametrize("name", LIVE)
def test_oracle_vs_live_reference(name):
    """fresh seeds and actions, four episodes a seed, and a NEW list given to both sides after the second: state, RNG, encode
    and every agent's view encoding after every call; the pixels too where the reference's renderer can draw every kind"""
    if name in LE.PINNED:
        level, pixels = LE.PINNED[name]
        second = [(5, 5, LE.WALL), (5, 5, 0), (9, 2, LE.GOAL)]
    else:
        rng = np.random.RandomState(int(name.split("-")[1]))
        level, second = LE.random_list(rng, 7), LE.random_list(rng, 7)
        pixels = not any(k in (LE.KEY, LE.BALL) for _, _, k in level + second)
    for seed in 61000 + np.arange(4):
        ref = LE.ref_env(seed, level, max_steps=MAX_STEPS, render=pixels)
        orc = O.OracleEnv(LE.edits_spec(MAX_STEPS), seed=int(seed))
        _same_as_reference(orc, ref, "%s seed %d ctor" % (name, seed))          # (both made it with no list)
        orc.set_edits(level)
        o, o2 = orc.reset(), ref.reset()
        _same_as_reference(orc, ref, "%s seed %d reset" % (name, seed))
        arng = np.random.RandomState(seed % 1000)
        episodes = t = 0
        while episodes < 4:
            a = arng.randint(0, 7, size=LE.N_AGENTS)
            o, r, d, _ = orc.step(a)
            o2, r2, d2, _ = ref.step(a)
            what = "%s seed %d step %d" % (name, seed, t)
            assert np.abs(r - np.asarray(r2, np.float64)).max() <= REW_TOL and bool(d) == bool(d2), what
            _same_as_reference(orc, ref, what)
            if pixels:
                assert np.array_equal(o, np.stack(o2)), what + ": observations"
            if d2:
                episodes += 1
                if episodes == 2:
                    orc.set_edits(second)
                    ref.level = list(second)
                o, o2 = orc.reset(), ref.reset()
                _same_as_reference(orc, ref, what + ": reset after it")
                if pixels:
                    assert np.array_equal(o, np.stack(o2)), what + ": observations of the reset"
            t += 1
