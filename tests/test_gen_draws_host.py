"""`_gen_grid` that lays the grid out from random draws (`self._rand_int`), without a GPU: the recorder (what it accepts,
what it refuses and why, the encoded program) and the device interpreter — `reset_env` of marlgrid_amd/csrc/mg_core.h built
for the host (tests/native) — against the reference's own trajectories (tests/golden/gendraws_*.npz, made by
tests/golden/make_gen_draws.py) and, where the reference is present, against the live reference."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import draw_envs as D  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402
from marlgrid_amd import seeding  # noqa: E402
from marlgrid_amd.agents import GridAgentInterface  # noqa: E402
from marlgrid_amd.base import GenDraw, MultiGrid, MultiGridEnv  # noqa: E402
from marlgrid_amd.objects import Goal, Wall  # noqa: E402

SYM, NEG = N.GEN_SYM, N.GEN_NEG
REW_TOL = 1e-6


def D_(r, c=0, neg=False):
    """the encoded operand `c +- draw[r]`"""
    return SYM | (NEG if neg else 0) | (r << N.GEN_DRAW_SHIFT) | (c & 0xFFFF)


def _record(gen, W=9, H=9, **kw):
    cls = type("T", (MultiGridEnv,), dict(_gen_grid=gen, mission="", metadata={}))
    env = cls(agents=[GridAgentInterface(color="red", view_size=7, view_tile_size=8)], width=W, height=H, batch_size=1,
              _dry=True, **kw)
    return env, env._dry_trace


def _room(self, width, height):
    self.grid = MultiGrid((width, height))
    self.grid.wall_rect(0, 0, width, height)


# ---- the symbolic value ---------------------------------------------------------------------------------------------------
def test_draw_arithmetic_allowed():
    seen = {}

    def gen(self, w, h):
        _room(self, w, h)
        d = self._rand_int(2, 6)
        seen.update(d=d, a=d + 3, b=3 + d, c=d - 1, e=10 - d, f=(10 - d) - 2, g=4 - (10 - d), h=d + np.int64(2))
    _record(gen)
    assert all(isinstance(v, GenDraw) for v in seen.values())
    form = {k: (v.reg, v.sign, v.const) for k, v in seen.items()}
    assert form == dict(d=(0, 1, 0), a=(0, 1, 3), b=(0, 1, 3), c=(0, 1, -1), e=(0, -1, 10), f=(0, -1, 8), g=(0, 1, -6),
                        h=(0, 1, 2))
    assert seen["e"].encode() == D_(0, 10, neg=True) and seen["c"].encode() == D_(0, -1)


@pytest.mark.parametrize("what", ["d == 3", "d != 3", "d < 3", "d >= 3", "bool(d)", "int(d)", "range(d)", "[0, 1, 2][d]",
                                  "d * 2", "2 * d", "d + d", "d - d", "-d", "d // 2", "d % 2", "abs(d)", "float(d)",
                                  "d + 1.5", "d + e", "not d", "3 if d else 4", "max(d, 3)", "d + True"])
def test_draw_refuses_everything_else(what):
    def gen(self, w, h):
        _room(self, w, h)
        d = self._rand_int(2, 6)
        e = self._rand_int(1, 3)
        eval(what, dict(d=d, e=e))
    with pytest.raises(NotImplementedError, match="may compute with it .* cannot branch on it"):
        _record(gen)


def test_rand_int_outside_gen_grid_refuses():
    env, _ = _record(_room)
    with pytest.raises(NotImplementedError, match="cannot branch on it"):
        env._rand_int(0, 3)


def test_draw_in_agent_spawn_kwargs_refuses():
    def gen(self, w, h):
        _room(self, w, h)
        s = self._rand_int(2, 6)
        self.agent_spawn_kwargs = dict(top=(0, 0), size=(s, h))
    with pytest.raises(NotImplementedError, match="agent_spawn_kwargs"):
        _record(gen)


def test_at_least_eight_draws_and_the_limit_is_named():
    def gen(n):
        def g(self, w, h):
            _room(self, w, h)
            for i in range(n):
                self.put_obj(Wall(), self._rand_int(1, w - 1), 1 + i % (h - 2))
        return g
    _, (_, ops) = _record(gen(8))
    assert [op[0] for op in ops if op[2] < 0] == list(range(8)) and N.GEN_DRAWS == 8
    with pytest.raises(NotImplementedError, match="at most 8"):
        _record(gen(9))


# ---- interval proofs ----------------------------------------------------------------------------------------------------------
def _gen_of(body):
    def gen(self, w, h):
        _room(self, w, h)
        body(self, w, h)
    return gen


ACCEPTED = {
    "fill at the grid's edge": lambda s, w, h: s.put_obj(Wall(), s._rand_int(0, w), s._rand_int(0, h)),
    "wall to the edge": lambda s, w, h: s.grid.horz_wall(s._rand_int(1, w - 1), 3),
    "wall with a drawn length": lambda s, w, h: s.grid.vert_wall(2, 1, s._rand_int(1, h - 1)),
    "wall_rect from draws": lambda s, w, h: s.grid.wall_rect(s._rand_int(0, 3), 1, 4, 3),
    "place left of a draw": lambda s, w, h: s.place_obj(Wall(), top=(0, 0), size=(s._rand_int(1, w), h)),
    "place clamped by the grid": lambda s, w, h: s.place_obj(Wall(), top=(s._rand_int(0, w) - 3, 0), size=(4, h + 5)),
    "place right of a draw": (lambda s, w, h: (lambda d: s.place_obj(Wall(), top=(d + 1, 0), size=(w - d - 1, h)))(s._rand_int(0, w - 1))),
    "draw bounded by a draw": lambda s, w, h: s._rand_int(1, s._rand_int(2, 5)),
    "draw bounded below by a draw": lambda s, w, h: s._rand_int(s._rand_int(0, 4), 4),
}
REFUSED = {
    "fill may leave the grid": lambda s, w, h: s.put_obj(Wall(), s._rand_int(0, w + 1), 1),
    "fill may be negative": lambda s, w, h: s.put_obj(Wall(), s._rand_int(0, 3) - 1, 1),
    "wall may run over the edge": lambda s, w, h: s.grid.horz_wall(s._rand_int(1, 4), 3, w - 2),
    "wall may be empty": lambda s, w, h: s.grid.vert_wall(2, 1, s._rand_int(0, 3)),
    "place rectangle may be empty": lambda s, w, h: s.place_obj(Wall(), top=(0, 0), size=(s._rand_int(0, 3), h)),
    "place rectangle may be empty after the clamp": lambda s, w, h: s.place_obj(Wall(), top=(s._rand_int(0, w + 1), 0), size=(2, 2)),
    "draw range may be empty": lambda s, w, h: s._rand_int(2, s._rand_int(2, 5)),
    "constant draw range is empty": lambda s, w, h: s._rand_int(3, 3),
    "draw may be negative": lambda s, w, h: s._rand_int(-1, 3),
    "draw may exceed a coordinate": lambda s, w, h: s._rand_int(0, 300),
}


@pytest.mark.parametrize("case", sorted(ACCEPTED))
def test_interval_proof_accepts(case):
    _, (_, ops) = _record(_gen_of(ACCEPTED[case]))
    assert any(op[2] < 0 for op in ops)


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_interval_proof_refuses(case):
    with pytest.raises(ValueError):
        _record(_gen_of(REFUSED[case]))


# ---- the encoded program --------------------------------------------------------------------------------------------------
def test_doorkey_7x7_program_literally():
    from marlgrid_amd.envs import DoorKeyEnv, env_from_config
    env = DoorKeyEnv(agents=[GridAgentInterface(color="red", view_size=7, view_tile_size=8)], width=7, height=7,
                     batch_size=1, _dry=True)
    template, ops = env._dry_trace
    wall, goal = env.obj_reg.find(Wall()), env.obj_reg.find(Goal(color="green", reward=1))
    from marlgrid_amd.objects import Door, Key
    door, key = env.obj_reg.find(Door(color="yellow", state=Door.LOCKED)), env.obj_reg.find(Key("yellow"))
    assert (wall, goal, door, key) == (1, 2, 3, 6)           # (a Door registers its other two states with it: 4, 5)
    want = np.zeros((7, 7), np.uint8)
    want[0, :] = want[6, :] = want[:, 0] = want[:, 6] = wall
    want[5, 5] = goal
    assert np.array_equal(template, want)
    S, Dr = 0x40000000, 0x40010000                           # draw[0] (the split column), draw[1] (the door row)
    assert ops == [
        (0, 1, -1, 2, 0, 5, 0, None),                        # draw[0] = _rand_int(2, 5)
        (wall, 1, 0, S, 0, S + 1, 7, None),                  # vert_wall(split, 0)
        (1, 1, -1, 1, 0, 5, 0, None),                        # draw[1] = _rand_int(1, 5)
        (door, 1, 0, S, Dr, S + 1, Dr + 1, None),            # put_obj(Door, split, door)
        (key, 1, 100000, 0, 0, S, 7, None),                  # place_obj(Key, top=(0, 0), size=(split, height))
    ]
    assert env.agent_spawn_kwargs == {}
    e2 = env_from_config(dict(env_class="DoorKeyEnv", agents=[GridAgentInterface(color="red", view_size=7, view_tile_size=8)],
                              width=7, height=7, batch_size=1, _dry=True), randomize_seed=False)
    assert isinstance(e2, DoorKeyEnv) and e2._dry_trace[1] == ops
    with pytest.raises(ValueError):                          # upstream draws the door ROW from the width: provable only if it fits
        DoorKeyEnv(agents=[GridAgentInterface(color="red", view_size=7, view_tile_size=8)], width=12, height=6, batch_size=1,
                   _dry=True)


def test_split_program_operands_and_bookkeeping():
    D.register()
    env = D.build("Draws-2AgentSplit7", batch_size=1, _dry=True)
    _, ops = env._dry_trace
    S, G = D_(0), D_(1)
    assert ops == [
        (0, 1, -1, 2, 0, 5, 0, None),
        (1, 1, 0, S, 0, D_(0, 1), 7, None),
        (1, 1, -1, 1, 0, 6, 0, None),
        (0, 1, 0, S, G, D_(0, 1), D_(1, 1), None),
        (2, 1, 100000, D_(0, 1), 0, 7, 7, None),             # top = s + 1; top + size = (s + 1) + (W - s - 1) = W: a constant
        (1, 2, 100, 0, 0, S, 7, None),                       # the two clutter walls: one op, count 2
    ]
    g = env.grid
    env._gen.active = True                                   # (get() as `_gen_grid` sees it)
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            assert g.get(0, 3) is not None and not w         # the outer wall: static, nothing can have written it
            g.get(3, 3)                                      # a cell the split wall, the gap or the clutter may have written
            assert len(w) == 1 and "may have filled" in str(w[0].message)
            g.get(5, 3)                                      # right of every possible column: only the goal's placement reaches it
            assert len(w) == 2
    finally:
        env._gen.active = False


def test_place_obj_clamps_the_top_first_and_adds_the_size_to_the_clamped_top():
    """base.py:692-695: `top = max(top, 0)`, THEN `bottom = min(top + size, (W, H))`.  A drawn top is clamped on the device,
    which moves the far edge with it (the program keeps top and top + size); a constant one here, size added afterwards"""
    def gen(self, w, h):
        _room(self, w, h)
        d = self._rand_int(0, 6)
        self.place_obj(Wall(), top=(d - 3, 0), size=(4, h + 5), max_tries=100)
        self.place_obj(Goal(color="green", reward=1), top=(-2, -1), size=(d + 1, 3), max_tries=100)
    _, (_, ops) = _record(gen)
    assert ops[1:] == [(1, 1, 100, D_(0, -3), 0, D_(0, 1), 9, None),
                       (2, 1, 100, 0, 0, D_(0, 1), 3, None)]          # upstream: [0, 0 + d + 1) x [0, 0 + 3), not d - 1 and 2

    def empty(self, w, h):                                           # [w + d - 3, ...): past the right edge for d = 3
        _room(self, w, h)
        self.place_obj(Wall(), top=(self._rand_int(0, 4) + w - 3, 0), size=(4, h))
    with pytest.raises(ValueError):
        _record(empty)


def test_static_edits_after_a_draw_go_into_the_program_unmerged():
    def gen(self, w, h):
        _room(self, w, h)
        self.put_obj(Wall(), 2, 2)                           # before the first draw: template
        d = self._rand_int(2, 5)
        self.put_obj(Wall(), 3, 3)                           # after it: ordered program
        self.put_obj(Wall(), 4, 3)                           # ... merged with its constant neighbour, as ever
        self.put_obj(Wall(), d, 4)
        self.put_obj(Wall(), d + 1, 4)                       # symbolic fills: never merged
        self.put_obj(Wall(), 5, 3)                           # (the op before it is symbolic: not merged into it either)
    _, (template, ops) = _record(gen)
    assert template[2, 2] == 1 and template[3, 3] == 0
    assert ops == [(0, 1, -1, 2, 0, 5, 0, None), (1, 1, 0, 3, 3, 5, 4, None), (1, 1, 0, D_(0), 4, D_(0, 1), 5, None),
                   (1, 1, 0, D_(0, 1), 4, D_(0, 2), 5, None), (1, 1, 0, 5, 3, 6, 4, None)]


def test_draw_free_programs_are_byte_identical_to_the_parents():
    """the tuples below were recorded by the commit before `_rand_int` existed"""
    import zlib
    import product_envs
    from marlgrid_amd.envs import make
    e = make("MarlGrid-3AgentCluttered15x15-v0", batch_size=1, _dry=True)
    assert e._dry_trace[1] == [(2, 1, 100, 0, 0, 15, 15, None)] and zlib.crc32(e._dry_trace[0].tobytes()) == 1112786602
    e.reset()
    template, ops = e._dry_trace
    assert ops == [(1, 25, 100, 0, 0, 15, 15, None)] and zlib.crc32(template.tobytes()) == 2523879021
    want = np.zeros((15, 15), np.uint8)
    want[0, :] = want[14, :] = want[:, 0] = want[:, 14] = 1
    want[13, 13] = 2
    assert np.array_equal(template, want)
    e = product_envs.build("Test-2AgentLateStatic10x10", batch_size=1, _dry=True)
    assert e._dry_trace[1] == [(1, 6, 100, 0, 0, 10, 10, None), (2, 1, 0, 8, 8, 9, 9, None), (1, 1, 0, 2, 5, 8, 6, None),
                               (0, 1, 0, 3, 5, 4, 6, None), (2, 1, 100, 1, 1, 4, 4, None), (1, 1, 0, 6, 1, 9, 2, None),
                               (1, 1, 0, 6, 3, 9, 4, None), (1, 1, 0, 6, 1, 7, 4, None), (1, 1, 0, 8, 1, 9, 4, None)]
    assert zlib.crc32(e._dry_trace[0].tobytes()) == 1336133245
    # ... and the struct they are packed into is the one the existing ABI tests pin
    import ctypes
    assert ctypes.sizeof(N.GenOp) == 32 and N.ABI_VERSION == 6


def test_long_program_has_a_draw_behind_op_32():
    D.register()
    _, ops = D.build("Draws-2AgentLongProgram12x12", batch_size=1, _dry=True)._dry_trace
    first = [i for i, op in enumerate(ops) if op[2] < 0]
    assert len(ops) > 32 and first[0] >= 32 and len(first) == 2
    assert any(v & SYM for op in ops[first[0] + 1:] for v in op[3:7])
    assert ops[first[1]][5] == D_(0, 1)                      # the second draw's upper bound is the first draw + 1


# ---- the interpreter on the host against the reference's trajectories ------------------------------------------------------
def _emu_rng(emu, b):
    return D.rng_digest(emu.numpy_rng_state(b))


@pytest.mark.parametrize("par", [False, True])
@pytest.mark.parametrize("name", sorted(D.SCENARIOS))
def test_host_emulation_vs_golden(name, par):
    import hostemu
    D.register()
    g = D.golden(name)
    S, T, n = g["actions"].shape
    emu = hostemu.HostEmu(name, S, g["seeds"], par=par)

    spec, W, H = emu.env.scenario_spec(), emu.env.width, emu.env.height
    rows, everyone = np.arange(S), np.ones(S, bool)

    def same(prefix, t, rng, what):
        st = D.canonical_batch(spec, emu.grid[:, :W * H].reshape(S, W, H), emu.rec)
        D.cmp_canon_batch(st, g, prefix, rows, None if t is None else np.full(S, t), everyone, "%s %s" % (name, what))
        for b in range(S):
            assert _emu_rng(emu, b) == (rng[b] if t is None else rng[b, t]), "%s %s env %d: RNG" % (name, what, b)
    same("ctor_", None, g["rng_ctor"], "ctor")
    emu.reset()
    same("reset_", None, g["rng_reset"], "reset")
    for t in range(T):
        r, d = emu.step(g["actions"][:, t])
        what = "step %d" % t
        assert np.abs(r.astype(np.float64) - g["rewards"][:, t]).max() <= REW_TOL, what
        assert np.array_equal(d, g["ep_done"][:, t]), what
        same("step_", t, g["rng_step"], what)
        if d.any():
            emu.reset(env_mask=d)
            for b in range(S):
                assert _emu_rng(emu, b) == g["rng_next"][b, t], "%s reset after step %d env %d: RNG" % (name, t, b)
    for b in range(len(g["mt_final"])):         # (the words themselves for the first seeds; every seed's digest: above)
        assert seeding.same_stream(emu.numpy_rng_state(b), (g["mt_final"][b], g["mt_final_pos"][b]))
    assert not emu.error.any()


def test_golden_conditions():
    """what the fixtures exist for, checked on the committed files"""
    for name, (kind, W, H, *_rest) in D.SCENARIOS.items():
        g = D.golden(name)
        assert g["reset_after"].sum(axis=1).min() >= D.EPISODES - 1 and (g["seeds"] == D.SEEDS).all()
        if kind == "split":
            assert (g["rewards"] > 0).any()
    g5 = D.golden("Draws-2AgentDoorKey5")
    assert (g5["step_carry_enc"].reshape(len(D.SEEDS), -1).any(axis=1)).sum() >= 5           # pickups
    door = g5["encode"][..., 0] == 11
    assert ((g5["encode"][..., 2] != 3) & door).any()                                         # the door unlocked


# ---- ... and against the live reference ----------------------------------------------------------------------------------------
def _live_cases():
    """30 seeded random (kind, W, H, seed).  DoorKey draws its door row from 1 .. W - 3 (upstream's text), which the recorder
    can prove to lie inside the wall only for W - 3 <= H - 1: its sizes are drawn until that holds (the reference itself
    fails on the others for some seeds)."""
    rng = np.random.RandomState(20240)
    out = []
    while len(out) < 30:
        kind = ("split", "doorkey")[len(out) % 2]
        W, H = (int(v) for v in rng.randint(5, 13, size=2))
        if kind == "doorkey" and W - 3 > H - 1:
            continue
        out.append((kind, W, H, int(rng.randint(0, 2 ** 31))))
    return out


@pytest.mark.reference
@pytest.mark.parametrize("kind,W,H,seed", _live_cases())
def test_host_emulation_vs_live_reference(kind, W, H, seed):
    import canon
    import hostemu
    import refstate
    from marlgrid_amd import envs as E
    name = "Draws-live-%s-%dx%d" % (kind, W, H)
    E._registry[name] = lambda **kw: D.build_sized(kind, W, H, **kw)
    try:
        emu = hostemu.HostEmu(name, 1, [seed], par=bool(seed & 1))
    finally:
        del E._registry[name]
    ref = D.ref_env(kind, W, H, 7, 8, 40, seed)

    def same(what):
        canon.assert_same(emu.canonical()[0], dict(refstate.canonical(ref)), what)
        rs = ref.np_random.get_state()
        assert seeding.same_stream(emu.numpy_rng_state(0), (rs[1], rs[2])), what
    same("ctor")
    emu.reset()
    ref.reset()
    same("reset")
    arng = np.random.RandomState(seed % 1000)
    episodes = t = 0
    while episodes < 2:
        a = arng.randint(0, 7, size=(1, 2))
        r, d = emu.step(a)
        _, r2, d2, _ = ref.step(a[0])
        assert np.abs(r[0].astype(np.float64) - r2).max() <= REW_TOL and bool(d[0]) == bool(d2), t
        same("step %d" % t)
        if d2:
            episodes += 1
            emu.reset()
            ref.reset()
            same("reset after step %d" % t)
        t += 1
    assert not emu.error.any()
