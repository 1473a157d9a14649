"""CPU: the oracle's control flow and parameters (oracle/mg_oracle.c: MGO_GEN_IF / ELSE / ENDIF, the object lookup, MGO_GEN_PARAM,
a count that is an operand) pinned BEFORE anything is held to them — against every reference trajectory of a `_gen_grid` that
branches on its draws (tests/golden/genbranch_*.npz), the path of every reset included, and, where the reference is present,
against the live reference on every path of every scenario kind.  The reference has no parameters: a parameter spec with the
value v must do, word for word and state for state, what the twin spec with the Python constant v does (the `if` inside the
twins is what the goldens pin).  The hand-written specs (tests/gen_branch_envs.py:spec, tests/param_envs.py:spec) are held to
the product's description of the same scenarios in everything but the programs: guards and blocks are two notations, and the
differentials with full path coverage are their comparison."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import canon  # noqa: E402
import draw_envs as D  # noqa: E402
import gen_branch_envs as G  # noqa: E402
import param_envs as PE  # noqa: E402
import viewenc  # noqa: E402
from golden import refstate  # noqa: E402  (crc() only; does not import the reference)
from oracle import oracle as O  # noqa: E402

REW_TOL = 1e-6
GOLDENS = sorted(f[len("genbranch_"):-len(".npz")] for f in os.listdir(G.GOLD) if f.startswith("genbranch_"))
ALL = dict(G.SCENARIOS, **G.ORACLE_ONLY)


def test_every_genbranch_fixture_is_a_scenario():
    assert GOLDENS == sorted(G.SCENARIOS) and len(GOLDENS) == 6


# ---- the specs ------------------------------------------------------------------------------------------------------------------
def _same_but_for_the_programs(got, want, what):
    for k in got:
        if k not in ("gen_ctor", "gen_reset"):
            assert got[k] == want[k], (what, k, got[k], want[k])
    assert set(want) - set(got) <= {"params"}, (what, sorted(set(want) - set(got)))


@pytest.mark.parametrize("name", sorted(ALL))
def test_hand_written_spec_agrees_with_scenario_spec_in_all_but_the_programs(name):
    G.register()
    env = G.build(name, batch_size=1, _dry=True)
    env.reset()
    _same_but_for_the_programs(env.scenario_spec(), G.spec_of(name), name)


@pytest.mark.parametrize("kind", sorted(PE.KINDS))
def test_hand_written_param_specs_agree_with_scenario_spec_in_all_but_the_programs(kind):
    PE.register()
    lo, hi = PE.interval(kind)
    for v in [None] + list(range(lo, hi)):
        env = PE.build(kind, v, batch_size=1, _dry=True)
        env.reset()
        _same_but_for_the_programs(env.scenario_spec(), PE.spec(kind, v), (kind, v))


def test_the_specs_hold_no_notation_of_the_product():
    """no guard, no packed operand, no register copy: the entries are the oracle's own, and the blocks nest"""
    specs = [G.spec_of(n) for n in ALL] + [PE.spec(k, v) for k in PE.KINDS for v in (None, PE.interval(k)[0])]
    for s in specs:
        for g in s["gen_reset"]:
            assert g[0] in ("wall_rect", "horz_wall", "put", "place", "draw", "fill", "place_sym", "if", "else", "endif", "param"), g
            assert all(abs(v) <= 2 ** 30 for v in g[1:] if isinstance(v, int)), g
        O.check_blocks(s["gen_reset"])
    deep = G.spec_of(G.DEEP)["gen_reset"]
    depth = best = 0
    for g in deep:
        depth += (g[0] == "if") - (g[0] == "endif")
        best = max(best, depth)
    assert best >= 3


def decode_guard(obj):
    """the guard in MgGenOp.obj, restated from the header's description (marlgrid_hip.h MG_GEN_GUARD), not through
    marlgrid_amd: bit 30 guarded, the register in bits 24-26, hi in bits 16-23, lo in bits 8-15; the low byte keeps its meaning
    -> None or (register, lo, hi)"""
    obj = int(obj)
    if not obj & 0x40000000:
        return None
    return (obj >> 24) & 7, (obj >> 8) & 0xFF, (obj >> 16) & 0xFF


def test_guard_decoder():
    assert decode_guard(5) is None and decode_guard(0x43050200 | 9) == (3, 2, 5) and decode_guard(0x47FF0000) == (7, 0, 255)


def test_deep_scenario_is_what_it_is_for():
    """the recorded program of Deep 12 x 10 guards on registers 4, 5 and 6 (the high half of the draw scalar), each guard one
    value; a fork has a guard at the low end, one at the high end and one in the middle of its draw; a draw bounded by a draw
    sits under a guard; a count is `draw - 1`; and the program stays inside the recorder's bounds"""
    G.register()
    env = G.build(G.DEEP, batch_size=1, _dry=True)
    env.reset()
    assert (env.width, env.height) == (12, 10)
    ops = env._dry_trace[1]
    guards = [decode_guard(op[0]) for op in ops]
    assert all(g is None or g[1] == g[2] for g in guards)                             # lo == hi: every guard is one value
    assert {g[0] for g in guards if g} == {4, 5, 6}
    # the spec's entries say the same (scenario_spec() decodes the guard itself: held to the restated decoder)
    entries = [e for e in env.scenario_spec()["gen_reset"] if e[0] == "guard"]
    assert {e[1:4] for e in entries} == {g for g in guards if g}
    # register 4 is the `_rand_int(0, 3)` of `_rand_elem`: guards at its low end, its middle and its high end
    draw4 = [op for op in ops if op[2] == -1 and op[0] & 0xFF == 4 and decode_guard(op[0]) is None]
    assert [(op[3], op[5]) for op in draw4] == [(0, 3)]
    assert {g[1] for g in guards if g and g[0] == 4} == {0, 1, 2}
    # the copies are `draw + 1`: t in 0..2 -> 1..3 on register 5, n in 1..3 -> 2..4 on register 6
    assert {g[1] for g in guards if g and g[0] == 5} == {1, 2, 3} and {g[1] for g in guards if g and g[0] == 6} == {2, 3, 4}
    # a guarded RNG draw whose bound is a draw (register 7, `_rand_int(1, b + 1)`), under the innermost guard
    dep = [op for op in ops if op[2] == -1 and op[0] & 0xFF == 7]
    assert len(dep) == 1 and decode_guard(dep[0][0]) == (6, 2, 2) and D.decode_operand(dep[0][5]) == ("d", 1, 1, 1)
    # `count=n - 1`
    counts = {D.decode_operand(op[1]) for op in ops if op[2] > 0 and op[1] & 0x40000000}
    assert counts == {("d", 2, 1, -1)}
    assert max(op[0] & 0xFF for op in ops if op[2] < 0) == 7 and len(G.paths("deep")) == 7 <= 64


# ---- the oracle against the reference's trajectories ----------------------------------------------------------------------------
def _rng(orc):
    return D.rng_digest(orc.mt_state())


@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_replays_golden(name):
    """everything the fixture holds: canonical state at ctor, reset and every step; rewards, ep_done, the shuffle order, encode,
    the agents' view encodings, the observations where the reference can render them; the RNG after EVERY step and every
    caller-side reset, the final MT19937 words — and the path of every `_gen_grid` run, from what the oracle itself drew"""
    g = G.golden(name)
    spec = G.spec_of(name)
    kind, W = G.SCENARIOS[name][:2]
    pixels = G.SCENARIOS[name][6]
    S, T, n = g["actions"].shape
    vsteps = set(int(v) for v in g["venc_steps"])
    vs = int(g["venc_steps"][1] - g["venc_steps"][0])
    after = iter(g["path_after_reset"].tolist())

    def views(orc, prefix, si, ti, what):
        got = viewenc.oracle_views(orc)
        for k in range(n):
            want = g["venc_%s_a%d" % (prefix, k)][si] if ti is None else g["venc_step_a%d" % k][si, ti]
            assert np.array_equal(got[k], want), (what, "view of agent", k)

    for si in range(S):
        orc = O.OracleEnv(spec, seed=int(g["seeds"][si]))
        what = "%s seed %d ctor" % (name, si)
        D.cmp_canon(canon.oracle_canonical(orc), g, "ctor_", si, None, what)
        assert _rng(orc) == g["rng_ctor"][si], what
        assert G.oracle_path(kind, W, orc) == g["path_ctor"][si], what
        views(orc, "ctor", si, None, what)
        if pixels:
            assert [refstate.crc(x) for x in orc.gen_obs()] == list(g["obs_crc_ctor"][si]), what
        o = orc.reset()
        what = "%s seed %d reset" % (name, si)
        D.cmp_canon(canon.oracle_canonical(orc), g, "reset_", si, None, what)
        assert _rng(orc) == g["rng_reset"][si], what
        assert G.oracle_path(kind, W, orc) == g["path_reset"][si], what
        views(orc, "reset", si, None, what)
        if pixels:
            assert [refstate.crc(x) for x in o] == list(g["obs_crc_reset"][si]), what
            if si == 0:
                assert np.array_equal(o, g["obs_reset_full"][0]), what
        for t in range(T):
            o, r, dn, _, order = orc.step(g["actions"][si, t], return_order=True)
            what = "%s seed %d step %d" % (name, si, t)
            assert np.array_equal(order, g["order"][si, t]), what
            D.cmp_canon(canon.oracle_canonical(orc), g, "step_", si, t, what)
            assert np.abs(r - g["rewards"][si, t]).max() <= REW_TOL, what
            assert dn == g["ep_done"][si, t], what
            assert np.array_equal(orc.encode(), g["encode"][si, t]), what
            assert _rng(orc) == g["rng_step"][si, t], what
            if t in vsteps:
                views(orc, "step", si, t // vs, what)
            if pixels:
                assert [refstate.crc(x) for x in o] == list(g["obs_crc"][si, t]), what
                if si == 0:
                    assert np.array_equal(o, g["obs_full"][0, t]), what
            if g["reset_after"][si, t]:
                orc.reset()
                assert _rng(orc) == g["rng_next"][si, t], what + ": reset after it"
                assert G.oracle_path(kind, W, orc) == next(after), what + ": path of the reset after it"
        if si < len(g["mt_final"]):
            mt, pos = orc.mt_state()
            assert pos == g["mt_final_pos"][si] and np.array_equal(mt, g["mt_final"][si]), name
    assert next(after, None) is None


# ---- blocks, lookups and counts on hand-made programs -----------------------------------------------------------------------------
def _tiny(prog, **more):
    s = D.spec("split", 7, 7)
    s["gen_ctor"], s["gen_reset"] = [("wall_rect", 0, 0, 7, 7)], [("wall_rect", 0, 0, 7, 7)] + prog
    s.update(more)
    return s


def test_a_block_that_is_not_taken_does_nothing_at_all():
    """no RNG word, no write, no error (a draw over an empty range, a fill off the grid, an index outside the list) and the
    registers as they were — beside the same program without the block"""
    dead = [("draw", 1, 4, 2), ("fill", 1, 9, 9, 10, 10), ("put", ("sel", 0, (1,)), 2, 2), ("draw", 0, 0, 100),
            ("if", 0, 0, 0), ("put", 1, 3, 3), G.ENDIF, ("place", 1, 3, 100)]
    head, tail = [("draw", 0, 2, 5)], [("draw", 2, 0, 50), ("place", 2, 1, 100)]
    for block in ([("if", D.dr(0), 7, 9)] + dead + [G.ENDIF],                               # the `if` suite, never true
                  [("if", D.dr(0), 2, 4), G.ELSE] + dead + [G.ENDIF],                       # the `else` suite, never reached
                  [("if", D.dr(0), 2, 4), ("if", D.dr(0), 5, 5)] + dead + [G.ENDIF, G.ENDIF]):     # nested
        for seed in range(20):
            a, b = O.OracleEnv(_tiny(head + block + tail), seed=seed), O.OracleEnv(_tiny(head + tail), seed=seed)
            a.reset()
            b.reset()
            assert np.array_equal(a.state()["base"], b.state()["base"]) and a.mt_state()[1] == b.mt_state()[1]
            assert np.array_equal(a.mt_state()[0], b.mt_state()[0])
            assert np.array_equal(a.draws()[0], b.draws()[0]) and np.array_equal(a.draws()[1], b.draws()[1])


def test_if_else_and_conds():
    prog = [("draw", 0, 0, 4), ("if", D.dr(0), 1, 2), ("put", 1, 2, 2), ("if", D.dr(0), 2, 2), ("put", 1, 3, 3), G.ENDIF,
            G.ELSE, ("put", 1, 4, 4), G.ENDIF, ("put", 1, 5, 5)]
    seen = set()
    for seed in range(60):
        orc = O.OracleEnv(_tiny(prog), seed=seed)
        orc.reset()
        d, base, c = int(orc.draws()[0][0]), orc.state()["base"], orc.conds()
        assert (base[2, 2] == 1) == (d in (1, 2)) and (base[3, 3] == 1) == (d == 2) and (base[4, 4] == 1) == (d in (0, 3))
        assert base[5, 5] == 1
        assert c[2] == int(d in (1, 2)) and c[4] == (int(d == 2) if d in (1, 2) else -1) and (np.delete(c, [2, 4]) == -1).all()
        seen.add(d)
    assert seen == {0, 1, 2, 3}


def test_blocks_nest_at_least_four_deep_and_must_match():
    prog = [("draw", 0, 0, 2)] + [("if", D.dr(0), 0, 0)] * 6 + [("put", 1, 2, 2)] + [G.ENDIF] * 6
    for seed in range(8):
        orc = O.OracleEnv(_tiny(prog), seed=seed)
        orc.reset()
        assert (orc.state()["base"][2, 2] == 1) == (orc.draws()[0][0] == 0)
    for bad in ([("if", 0, 0, 0)], [G.ENDIF], [G.ELSE], [("if", 0, 0, 0), G.ELSE, G.ELSE, G.ENDIF]):
        with pytest.raises(AssertionError):
            O.make_config(_tiny(bad))


def test_the_lookup_is_the_list_of_the_text():
    objs = [None, D._WALL, D._GOAL, dict(type="Goal", color="blue", state=0, reward=2)]
    seen = set()
    for seed in range(40):
        orc = O.OracleEnv(_tiny([("draw", 3, 0, 3), ("put", ("sel", 3, (2, 3, 1)), 2, 2),
                                 ("fill", ("sel", 3, (1, 1, 3)), 3, 3, 4, 5)], objects=objs), seed=seed)
        orc.reset()
        i, base = int(orc.draws()[0][3]), orc.state()["base"]
        assert base[2, 2] == (2, 3, 1)[i] and base[3, 3] == base[3, 4] == (1, 1, 3)[i]
        seen.add(i)
    assert seen == {0, 1, 2}
    orc = O.OracleEnv(_tiny([("draw", 0, 3, 5), ("put", ("sel", 0, (1, 2)), 2, 2)]), seed=1)
    with pytest.raises(ValueError):                                                 # (the oracle's code for IndexError)
        orc.reset()


def test_a_count_below_one_places_nothing():
    """`for _ in range(count)`: 0 and every negative count make no call — no RNG word, and no ValueError from a rectangle that
    would be empty"""
    for c in (3, 1, 0, -1, -5):
        for seed in range(5):
            prog = [("draw", 0, 5, 6), ("place_sym", 1, D.dr(0, c - 5), 100, 1, 1, 6, 6), ("place", 1, D.dr(0, c + 5, -1) if c <= 0 else c, 100)]      # c + 5 - draw: c again
            orc = O.OracleEnv(_tiny(prog), seed=seed)
            orc.reset()
            assert (orc.state()["base"][1:6, 1:6] == 1).sum() == 2 * max(c, 0)
            if c <= 0:
                ref = O.OracleEnv(_tiny([("draw", 0, 5, 6)]), seed=seed)
                ref.reset()
                assert ref.mt_state()[1] == orc.mt_state()[1] and np.array_equal(ref.mt_state()[0], orc.mt_state()[0])
    orc = O.OracleEnv(_tiny([("draw", 0, 5, 6), ("place_sym", 1, D.dr(0, -5), 100, 4, 1, 2, 6)]), seed=1)
    orc.reset()                                                                     # an empty rectangle, never sampled
    orc = O.OracleEnv(_tiny([("draw", 0, 5, 6), ("place_sym", 1, D.dr(0, -4), 100, 4, 1, 2, 6)]), seed=1)
    with pytest.raises(ValueError):
        orc.reset()


# ---- parameters: a parameter spec with the value v is the twin spec with the constant v -------------------------------------------
def _lockstep(a, b, T, seed, what):
    assert a.mt_state()[1] == b.mt_state()[1] and np.array_equal(a.mt_state()[0], b.mt_state()[0]), what
    rng = np.random.RandomState(seed)
    ends = 0
    for t in range(T):
        act = rng.randint(0, 7, size=a.n)
        oa, ra, da, _ = a.step(act)
        ob, rb, db, _ = b.step(act)
        w = "%s step %d" % (what, t)
        assert da == db and np.array_equal(ra, rb), w
        if da:
            ends += 1
            oa, ob = a.reset(), b.reset()
        assert np.array_equal(oa, ob), w
        canon.assert_same(canon.oracle_canonical(a), canon.oracle_canonical(b), w)
        assert a.mt_state()[1] == b.mt_state()[1] and np.array_equal(a.mt_state()[0], b.mt_state()[0]), w
    return ends


PARAM_CASES = [(kind, v) for kind in sorted(PE.KINDS) for v in range(*PE.interval(kind))]


@pytest.mark.parametrize("kind,v", PARAM_CASES, ids=["%s-%d" % c for c in PARAM_CASES])
def test_parameter_spec_equals_the_twin_spec(kind, v):
    """every value of every kind, over resets and steps: observations, state and every RNG word.  (Neither env runs the
    constructor's reset, which a parameter env makes with the default and a twin with its constant: both streams begin at the
    reset after the value is set.)  For `clutter` and `long` this is the symbolic count against the constant count."""
    pname = PE.KINDS[kind][2]
    for seed in (11, 12, 13):
        a = O.OracleEnv(PE.spec(kind), seed=seed, construct=False)
        b = O.OracleEnv(PE.spec(kind, v), seed=seed, construct=False)
        assert a.param(pname) == PE.interval(kind)[0]           # what a new env holds: the default
        a.set_params(**{pname: v})
        assert np.array_equal(a.reset(), b.reset())
        assert _lockstep(a, b, 45, seed, "%s value %d seed %d" % (kind, v, seed)) >= 3
        d, w = a.draws()
        assert d[0] == v and w[0] == 0                          # the parameter's register: the value, and no RNG word


def test_a_parameter_set_mid_episode_is_seen_by_the_next_reset_and_not_before():
    kind, pname = "clutter", "n"
    W, H = PE.KINDS[kind][:2]
    orc = O.OracleEnv(PE.spec(kind), seed=5)
    walls = lambda: int((orc.state()["base"][1:W - 1, 1:H - 1] == 1).sum())
    assert walls() == 0                                         # the constructor's reset: the default, 0 blocks
    orc.set_params(n=7)
    assert walls() == 0 and orc.param(pname) == 7
    orc.step([6, 6])
    assert walls() == 0
    orc.reset()
    assert walls() == 7
    orc.set_params({0: 20})                                     # by column number
    orc.step([6, 6])
    assert walls() == 7
    orc.reset()
    assert walls() == 20


def test_set_params_reaches_one_env_of_a_batch():
    batch = O.OracleBatch(PE.spec("clutter"), [1, 2, 3])
    batch.envs[1].set_params(n=4)
    batch.reset()
    assert [int((e.state()["base"][1:10, 1:10] == 1).sum()) for e in batch.envs] == [0, 4, 0]


# ---- the oracle beside the live reference: every path of every kind -----------------------------------------------------------------
# (kind, W, H, max_steps, seeds): several sizes for sides / cdk; seeds enough that the reference takes every path
LIVE = [("choice", 7, 7, 12, 6), ("sides", 9, 9, 12, 24), ("sides", 7, 7, 12, 12), ("sides", 10, 8, 12, 24),
        ("long", 12, 12, 12, 10), ("cdk", 6, 6, 16, 12), ("cdk", 8, 8, 16, 12), ("cdk", 9, 9, 16, 12),
        ("deep", 12, 10, 12, 24)]


def _same_as_reference(orc, ref, what):
    import refstate as RS
    canon.assert_same(canon.oracle_canonical(orc), dict(RS.canonical(ref)), what)
    rs = ref.np_random.get_state()
    mt, pos = orc.mt_state()
    assert pos == rs[2] and np.array_equal(mt, rs[1]), what + ": RNG"


@pytest.mark.reference
@pytest.mark.parametrize("kind,W,H,max_steps,n_seeds", LIVE, ids=["%s-%dx%d" % c[:3] for c in LIVE])
def test_oracle_vs_live_reference(kind, W, H, max_steps, n_seeds):
    """state and the RNG stream after every call over three episodes a seed, and at every `_gen_grid` run the path the
    reference took (the values its `_fork` was handed) against the path the oracle took; every path of the kind is taken"""
    seen = set()
    all_paths = G.paths(kind, W)
    for seed in 31000 + np.arange(n_seeds):
        ref = G.ref_env(kind, W, H, 7, 8, max_steps, seed, render=False)
        orc = O.OracleEnv(G.spec(kind, W, H, 7, 8, max_steps), seed=int(seed))

        def same(what):
            _same_as_reference(orc, ref, "%s seed %d %s" % (kind, seed, what))
            p = G.take_path(ref, kind, W)
            assert G.oracle_path(kind, W, orc) == p, (kind, seed, what, all_paths[p])
            seen.add(p)
        same("ctor")
        orc.reset()
        ref.reset()
        same("reset")
        arng = np.random.RandomState(seed % 1000)
        episodes = t = 0
        while episodes < 3:
            a = arng.randint(0, 7, size=2)
            _, r, d, _ = orc.step(a)
            _, r2, d2, _ = ref.step(a)
            assert np.abs(r - np.asarray(r2, np.float64)).max() <= REW_TOL and bool(d) == bool(d2), (seed, t)
            _same_as_reference(orc, ref, "%s seed %d step %d" % (kind, seed, t))
            if d2:
                episodes += 1
                orc.reset()
                ref.reset()
                same("reset after step %d" % t)
            t += 1
    assert seen == set(range(len(all_paths))), (kind, W, sorted(set(range(len(all_paths))) - seen))
