"""CPU: the oracle's `_rand_int` draws (oracle/mg_oracle.c: MGO_GEN_DRAW / FILL / PLACE_SYM) pinned BEFORE anything is held to
them — against every reference trajectory of a `_gen_grid` with draws (tests/golden/gendraws_*.npz) and, where the reference
is present, against the live reference — and the hand-written specs the oracle runs (tests/draw_envs.py:spec) held to the
product's own description of the same scenarios."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import canon  # noqa: E402
import draw_envs as D  # noqa: E402
import viewenc  # noqa: E402
from golden import refstate  # noqa: E402  (crc() only; does not import the reference)
from oracle import oracle as O  # noqa: E402

REW_TOL = 1e-6
GOLDENS = sorted(f[len("gendraws_"):-len(".npz")] for f in os.listdir(D.GOLD) if f.startswith("gendraws_"))


def test_every_gendraws_fixture_is_a_scenario():
    assert GOLDENS == sorted(D.SCENARIOS) and len(GOLDENS) == 9


# ---- the specs ------------------------------------------------------------------------------------------------------------------
def test_operand_decoder():
    assert D.decode_operand(5) == 5 and D.decode_operand(0) == 0
    assert D.decode_operand(0x40000000) == ("d", 0, 1, 0)
    assert D.decode_operand(0x40000000 | 7 << 16 | 0xFFFD) == ("d", 7, 1, -3)
    assert D.decode_operand(0x60000000 | 4 << 16 | 10) == ("d", 4, -1, 10)
    assert D.decode_operand(0x40000000 | 3 << 16 | 0x8000) == ("d", 3, 1, -32768)


@pytest.mark.parametrize("name", sorted(D.SCENARIOS) + sorted(D.ORACLE_ONLY))
def test_scenario_spec_decodes_to_the_hand_written_spec(name):
    """as tests/test_host_cpu.py:test_scenario_spec_matches_independent_restatement does for the draw-free envs"""
    D.register()
    env = D.build(name, batch_size=1, _dry=True)
    want = D.spec_of(name)
    assert D.decode_spec(env.scenario_spec())["gen_ctor"] == want["gen_ctor"]
    env.reset()
    got = D.decode_spec(env.scenario_spec())
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    assert set(got) == set(want)


def test_the_make_ids_of_doorkey_decode_to_the_hand_written_spec():
    from marlgrid_amd.envs import make
    for env_id, size in (("MarlGrid-2AgentDoorKey6x6-v0", 6), ("MarlGrid-2AgentDoorKey8x8-v0", 8)):
        env = make(env_id, batch_size=1, _dry=True, max_steps=20)
        got, want = D.decode_spec(env.scenario_spec()), doorkey_make_spec(size, 20)
        for k in want:
            assert got[k] == want[k], (env_id, k, got[k], want[k])


def doorkey_make_spec(size, max_steps):
    """`make("MarlGrid-2AgentDoorKey<N>x<N>-v0")`: two agents in the registered colours, view 7 at 8-pixel tiles"""
    return D.spec("doorkey", size, size, 7, 8, max_steps)


def test_eight_draws_scenario_is_what_it_is_for():
    s = D.spec_of("Draws-2AgentEight12x10")
    prog = s["gen_reset"]
    assert (s["W"], s["H"]) == (12, 10)
    assert [g[1] for g in prog if g[0] == "draw"] == list(range(8))
    regs = lambda gs: {v[1] for g in gs for v in g[2:] if isinstance(v, tuple)}
    assert {4, 5, 6, 7} <= regs([g for g in prog if g[0] == "fill"])
    assert {4, 5, 6, 7} <= regs([(g[0], g[1]) + g[4:] for g in prog if g[0] == "place_sym"])
    ops = [v for g in prog for v in g[2:] if isinstance(v, tuple)]
    assert any(v[2] == 1 and v[3] < 0 for v in ops) and any(v[2] == -1 for v in ops)
    draws = {g[1]: g[2:] for g in prog if g[0] == "draw"}
    assert isinstance(draws[2][1], tuple) and isinstance(draws[3][0], tuple)            # bounded above / below by a draw
    assert draws[4] == (("d", 2, 1, 0), ("d", 2, 1, 1))                                   # the one-value range
    spans = [hi - lo - 1 for lo, hi in draws.values() if not isinstance(lo, tuple) and not isinstance(hi, tuple)]
    assert any((sp + 1) & sp for sp in spans)                                             # a span that is not 2^k - 1


def test_in_place_scenario_takes_the_grid_in_place_kernel():
    from marlgrid_amd import _native as N
    D.register()
    env = D.build("Draws-2AgentSplit160x150", batch_size=1, _dry=True)
    cfg, _raw, _flat, _atlas = env._host_tables()
    assert N.render_kernel_name(cfg)[0] == D.IN_PLACE_KERNEL


# ---- the oracle against the reference's trajectories ----------------------------------------------------------------------------
def _rng(orc):
    return D.rng_digest(orc.mt_state())


@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_replays_golden(name):
    """canonical state at ctor, reset and every step; rewards, ep_done, the shuffle order, encode, the agents' view
    encodings, the observations where the reference can render them; the RNG after EVERY step and every caller-side
    reset, and the final MT19937 words"""
    g = D.golden(name)
    spec = D.spec_of(name)
    pixels = D.SCENARIOS[name][6]
    S, T, n = g["actions"].shape
    vsteps = set(int(v) for v in g["venc_steps"])
    vs = int(g["venc_steps"][1] - g["venc_steps"][0])

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
        views(orc, "ctor", si, None, what)
        if pixels:
            assert [refstate.crc(x) for x in orc.gen_obs()] == list(g["obs_crc_ctor"][si]), what
        o = orc.reset()
        what = "%s seed %d reset" % (name, si)
        D.cmp_canon(canon.oracle_canonical(orc), g, "reset_", si, None, what)
        assert _rng(orc) == g["rng_reset"][si], what
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
        if si < len(g["mt_final"]):
            mt, pos = orc.mt_state()
            assert pos == g["mt_final_pos"][si] and np.array_equal(mt, g["mt_final"][si]), name


# ---- the oracle's error paths: reachable through hand-made specs only -----------------------------------------------------------
def _tiny(prog):
    s = D.spec("split", 7, 7)
    s["gen_ctor"], s["gen_reset"] = [("wall_rect", 0, 0, 7, 7)], [("wall_rect", 0, 0, 7, 7)] + prog
    return s


@pytest.mark.parametrize("prog", [[("draw", 0, 3, 3)], [("draw", 0, 4, 2)],
                                  [("draw", 0, 2, 5), ("draw", 1, D.dr(0), 2)],                # empty for every value but ...
                                  [("draw", 0, 2, 5), ("place_sym", 1, 1, 100, D.dr(0), 0, 2, 7)],   # randint(low >= high)
                                  [("draw", 0, 2, 5), ("place_sym", 1, 1, 100, D.dr(0, 5), 0, D.dr(0, 7), 7)]])
def test_empty_range_is_value_error(prog):
    orc = O.OracleEnv(_tiny(prog), seed=3)
    with pytest.raises(ValueError):
        orc.reset()


@pytest.mark.parametrize("prog", [[("draw", 0, 2, 5), ("fill", 1, D.dr(0, 5), 1, D.dr(0, 6), 2)],      # x = draw + 5 >= 7
                                  [("draw", 0, 2, 5), ("fill", 1, D.dr(0, -5), 1, D.dr(0, -4), 2)],    # x = draw - 5 < 0
                                  [("fill", 0, 1, 6, 2, 8)]])                                          # y up to 7
def test_fill_off_the_grid_is_assertion_error(prog):
    """grid.set asserts (base.py:149-152): the oracle clamps no fill"""
    orc = O.OracleEnv(_tiny(prog), seed=3)
    with pytest.raises(AssertionError):
        orc.reset()


def test_draws_are_reported_and_a_one_value_range_consumes_nothing():
    orc = O.OracleEnv(_tiny([("draw", 0, 2, 5), ("draw", 1, D.dr(0), D.dr(0, 1)), ("draw", 9, 0, 200)]), seed=5)
    seen = set()
    for _ in range(40):
        orc.reset()
        d, w = orc.draws()
        assert 2 <= d[0] <= 4 and d[1] == d[0] and w[1] == 0 and w[0] >= 1 and 0 <= d[9] < 200 and w[9] >= 1
        assert (d[2:9] == -1).all() and (w[2:9] == -1).all()
        seen.add(int(d[0]))
    assert seen == {2, 3, 4}


def test_place_sym_clamps_the_top_first():
    """base.py:692-695: top = max(top, 0), THEN bottom = min(top + size, (W, H)): [d - 3, d + 1) is [0, 4) for d < 3"""
    xs = {}
    for seed in range(300):
        orc = O.OracleEnv(_tiny([("draw", 0, 0, 6), ("place_sym", 2, 1, 100, D.dr(0, -3), 3, D.dr(0, 1), 4)]), seed=seed)
        orc.reset()
        d = int(orc.draws()[0][0])
        x = int(np.argwhere(orc.state()["base"] == 2)[0][0])
        xs.setdefault(d, set()).add(x)
    for d, got in xs.items():        # (column 0 is wall: never accepted)
        assert got == set(range(max(d - 3, 0), max(d - 3, 0) + 4)) - {0}, (d, got)
    assert set(xs) == set(range(6))


# ---- the oracle beside the live reference ---------------------------------------------------------------------------------------
def _eight_cases():
    """ten (W, H, seed) of the eight-draw scenario, sizes drawn until the recorder accepts them (as DoorKey's are)"""
    rng = np.random.RandomState(20241)
    out = []
    while len(out) < 10:
        W, H = (int(v) for v in rng.randint(8, 16, size=2))
        try:
            D.build_sized("eight", W, H, batch_size=1, _dry=True)
        except ValueError:
            continue
        out.append(("eight", W, H, int(rng.randint(0, 2 ** 31))))
    return out


def _live_cases():
    import test_gen_draws_host
    return test_gen_draws_host._live_cases() + _eight_cases()


def _same_as_reference(orc, ref, what):
    import refstate as RS
    canon.assert_same(canon.oracle_canonical(orc), dict(RS.canonical(ref)), what)
    rs = ref.np_random.get_state()
    mt, pos = orc.mt_state()
    assert pos == rs[2] and np.array_equal(mt, rs[1]), what + ": RNG"


@pytest.mark.reference
@pytest.mark.parametrize("kind,W,H,seed", _live_cases())
def test_oracle_vs_live_reference(kind, W, H, seed):
    """state and the RNG stream after every call, over two episodes"""
    ref = D.ref_env(kind, W, H, 7, 8, 40, seed)
    orc = O.OracleEnv(D.spec(kind, W, H, 7, 8, 40), seed=seed)
    _same_as_reference(orc, ref, "ctor")
    orc.reset()
    ref.reset()
    _same_as_reference(orc, ref, "reset")
    arng = np.random.RandomState(seed % 1000)
    episodes = t = 0
    while episodes < 2:
        a = arng.randint(0, 7, size=2)
        _, r, d, _ = orc.step(a)
        _, r2, d2, _ = ref.step(a)
        assert np.abs(r - np.asarray(r2, np.float64)).max() <= REW_TOL and bool(d) == bool(d2), t
        _same_as_reference(orc, ref, "step %d" % t)
        if d2:
            episodes += 1
            orc.reset()
            ref.reset()
            _same_as_reference(orc, ref, "reset after step %d" % t)
        t += 1


@pytest.mark.reference
@pytest.mark.parametrize("seed", [7001, 7002])
def test_oracle_vs_live_reference_split160x150(seed):
    """the grid-in-place scenario: the constructor, three resets and five steps; state and RNG only (the reference's
    gen_agent_obs is stubbed out, as ref_env does for DoorKey: rendering such a grid takes it minutes)"""
    kind, W, H, view, tile, max_steps, _pix = D.ORACLE_ONLY["Draws-2AgentSplit160x150"]
    ref = D.ref_env(kind, W, H, view, tile, max_steps, seed, render=False)
    orc = O.OracleEnv(D.spec(kind, W, H, view, tile, max_steps), seed=seed)
    _same_as_reference(orc, ref, "ctor")
    for i in range(3):
        orc.reset()
        ref.reset()
        _same_as_reference(orc, ref, "reset %d" % i)
    arng = np.random.RandomState(seed)
    for t in range(5):
        a = arng.randint(0, 7, size=2)
        _, r, d, _ = orc.step(a)
        _, r2, d2, _ = ref.step(a)
        assert np.abs(r - np.asarray(r2, np.float64)).max() <= REW_TOL and bool(d) == bool(d2), t
        _same_as_reference(orc, ref, "step %d" % t)
