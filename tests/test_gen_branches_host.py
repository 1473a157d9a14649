"""`_gen_grid` that BRANCHES on random draws (`self._fork`, `self._rand_elem`, `self._rand_bool`), without a GPU: the
recorder (one run per path, the runs merged into one guarded program; what it refuses and why) and the device interpreter —
`reset_env` of marlgrid_amd/csrc/mg_core.h built for the host (tests/native) — against the reference's own trajectories
(tests/golden/genbranch_*.npz, made by tests/golden/make_gen_branches.py) and, where the reference is present, against the
live reference."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import draw_envs as D  # noqa: E402
import gen_branch_envs as G  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402
from marlgrid_amd import seeding  # noqa: E402
from marlgrid_amd.agents import GridAgentInterface  # noqa: E402
from marlgrid_amd.base import MultiGrid, MultiGridEnv  # noqa: E402
from marlgrid_amd.objects import Door, Goal, Key, Wall  # noqa: E402

REW_TOL = 1e-6
TRIES = 100000                       # place_obj's default max_tries


def D_(r, c=0, neg=False):
    """the encoded operand `c +- draw[r]` (marlgrid_hip.h MG_GEN_SYM), restated"""
    return 0x40000000 | (0x20000000 if neg else 0) | (r << 16) | (c & 0xFFFF)


def Gd(r, lo, hi=None):
    """the guard bits of MgGenOp.obj, restated from the header: bit 30, r in bits 24-26, hi in 16-23, lo in 8-15"""
    return 0x40000000 | (r << 24) | ((lo if hi is None else hi) << 16) | (lo << 8)


def _record(gen, W=9, H=9, **kw):
    cls = type("T", (MultiGridEnv,), dict(_gen_grid=gen, mission="", metadata={}))
    env = cls(agents=[GridAgentInterface(color="red", view_size=7, view_tile_size=8)], width=W, height=H, batch_size=1,
              _dry=True, **kw)
    return env, env._dry_trace


def _room(self, width, height):
    self.grid = MultiGrid((width, height))
    self.grid.wall_rect(0, 0, width, height)


def _dry(name):
    G.register()
    return G.build(name, batch_size=1, _dry=True)


# ---- the recorder: expected programs, written by hand ------------------------------------------------------------------------
def test_constants_agree_with_the_header():
    assert (N.GEN_GUARD, N.GEN_GUARD_DRAW_SHIFT, N.GEN_GUARD_HI_SHIFT, N.GEN_GUARD_LO_SHIFT) == (0x40000000, 24, 16, 8)
    assert N.ABI_VERSION == 6 and Gd(3, 2, 5) == 0x43050200
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "marlgrid_hip.h")).read()
    for line in ("#define MG_GEN_GUARD 0x40000000", "#define MG_GEN_GUARD_DRAW_SHIFT 24", "#define MG_GEN_GUARD_HI_SHIFT 16",
                 "#define MG_GEN_GUARD_LO_SHIFT 8", "#define MG_ABI_VERSION 6"):
        assert line in hdr, line


def test_choice_program_literally():
    env = _dry("Branch-2AgentChoice7")
    template, ops = env._dry_trace
    wall = env.obj_reg.find(Wall())
    goals = [env.obj_reg.find(Goal(color=c, reward=r)) for c, r in G.GOALS]
    assert (wall, goals) == (1, [2, 3, 4])                   # every path's objects are registered, in path order
    want = [(0, 1, -1, 0, 0, 3, 0, None)]                    # draw[0] = _rand_int(0, 3)
    for i, goal in enumerate(goals):                         # a top-level fork: the guard is on the draw itself
        want += [(goal | Gd(0, i), 1, TRIES, 0, 0, 7, 7, None), (wall | Gd(0, i), 2, 100, 0, 0, 7, 7, None)]
    assert ops == want
    assert template[0, 0] == wall and template[3, 3] == 0
    spec = env.scenario_spec()["gen_reset"]
    assert spec[:3] == [("wall_rect", 0, 0, 7, 7), ("draw", 0, 0, 3), ("guard", 0, 0, 0, ("place_sym", 2, 1, TRIES, 0, 0, 7, 7))]
    assert spec[-1] == ("guard", 0, 2, 2, ("place_sym", 1, 2, 100, 0, 0, 7, 7))


def test_sides_program_literally():
    """a fork on draw 0 (five values), a draw that only two of its branches make, and in every branch a fork on a later draw:
    the conjunction goes through a copy register — `copy = draw + 1` under the outer guard, then guards on the copy"""
    env = _dry("Branch-2AgentSides9")
    _, ops = env._dry_trace
    wall, goal = env.obj_reg.find(Wall()), env.obj_reg.find(Goal(color="green", reward=1))
    assert (wall, goal) == (1, 2)
    S, Gp = D_(0), D_(1)
    want = [(0, 1, -1, 2, 0, 7, 0, None),                    # s = draw[0] = _rand_int(2, 7)
            (wall, 1, 0, S, 0, D_(0, 1), 9, None),           # vert_wall(s, 0)
            (1, 1, -1, 1, 0, 8, 0, None),                    # the gap row, draw[1]
            (0, 1, 0, S, Gp, D_(0, 1), D_(1, 1), None)]
    for s in (2, 3):                                         # goal right; e = draw[2]; the bool draw[3]; its copy draw[4]
        g = Gd(0, s)
        want += [(goal | g, 1, TRIES, D_(0, 1), 0, 9, 9, None),          # the operands stay symbolic; proved for s alone
                 (2 | g, 1, -1, 1, 0, 8, 0, None),
                 (wall | g, 1, 0, 7, D_(2), 8, D_(2, 1), None),
                 (3 | g, 1, -1, 0, 0, 2, 0, None)]
        if s == 3:                                           # register 4 was written by the branch before: zeroed in every env
            want += [(4, 1, -1, 0, 0, 1, 0, None)]
        want += [(4 | g, 1, -1, D_(3, 1), 0, D_(3, 2), 0, None),         # copy = draw[3] + 1: a one-value draw, no RNG word
                 (wall | Gd(4, 1), 1, 0, 1, 1, 2, 2, None)]              # _rand_bool() is draw == 0: copy == 1
    for s in (4, 5, 6):                                      # goal left; the bool is draw[2], its copy draw[3]
        g = Gd(0, s)
        want += [(goal | g, 1, TRIES, 0, 0, S, 9, None),
                 (2 | g, 1, -1, 0, 0, 2, 0, None),
                 (3, 1, -1, 0, 0, 1, 0, None),               # (3 held a draw in the branches s = 2, 3; then a copy)
                 (3 | g, 1, -1, D_(2, 1), 0, D_(2, 2), 0, None),
                 (wall | Gd(3, 1), 1, 0, 1, 1, 2, 2, None)]
    assert ops == want
    assert max(op[0] & 0xFF for op in ops if op[2] < 0) == 4     # registers are shared between the branches: five, not ten


def test_long_program_has_guarded_ops_on_both_sides_of_op_32():
    env = _dry("Branch-2AgentLong12")
    _, ops = env._dry_trace
    wall, goal = 1, 2
    want = []
    for i in range(10):                                      # the common prefix: ops 0 .. 19
        want += [(wall, 1, 100, 0, 0, 12, 12, None), (0, 1, 0, 1 + i % 10, 1, 2 + i % 10, 2, None)]
    want += [(0, 1, -1, 0, 0, 3, 0, None)]                   # op 20: the index into LONG_K
    for j, k in enumerate(G.LONG_K):
        g = Gd(0, j)
        for i in range(10, 17):
            x = 1 + (i + k) % 10
            want += [(wall | g, 1, 100, 0, 0, 12, 12, None), (g, 1, 0, x, 1, x + 1, 2, None)]
        want += [(wall | g, 1, 0, 2, 9, 2 + k, 10, None),    # horz_wall(2, 9, k): its length is the forked value
                 (1 | g, 1, -1, 0, 0, 2, 0, None)]
        if j:
            want += [(2, 1, -1, 0, 0, 1, 0, None)]
        want += [(2 | g, 1, -1, D_(1, 1), 0, D_(1, 2), 0, None),
                 (Gd(2, 1), 1, 0, 2, 9, 3, 10, None),        # put_obj(None, 2, 9) where the bool came out True
                 (goal | Gd(2, 1), 1, 100, 0, 0, 12, 12, None),
                 (goal | Gd(2, 2), 1, 100, 0, 0, 12, 12, None)]
    assert ops == want
    guarded = [i for i, op in enumerate(ops) if op[0] & N.GEN_GUARD]
    assert guarded[0] == 21 and any(i < 32 for i in guarded) and any(i >= 32 for i in guarded) and len(ops) > 64


@pytest.mark.parametrize("size", [6, 8])
def test_colored_doorkey_program_literally(size):
    from marlgrid_amd import envs as E
    env = _dry("Branch-2AgentColoredDoorKey%d" % size)
    assert isinstance(env, E.ColoredDoorKeyEnv) and E.ColoredDoorKeyEnv.door_colors == G.DOOR_COLORS
    template, ops = env._dry_trace
    W = size
    want = [(0, 1, -1, 2, 0, W - 2, 0, None), (1, 1, 0, D_(0), 0, D_(0, 1), W, None), (1, 1, -1, 1, 0, W - 2, 0, None),
            (2, 1, -1, 0, 0, 6, 0, None)]                    # the colour: draw[2] = _rand_int(0, 6)
    for i, c in enumerate(G.DOOR_COLORS):
        door, key = env.obj_reg.find(Door(color=c, state=Door.LOCKED)), env.obj_reg.find(Key(c))
        assert (door, key) == (3 + 4 * i, 6 + 4 * i)         # (a Door registers its other two states with it)
        want += [(door | Gd(2, i), 1, 0, D_(0), D_(1), D_(0, 1), D_(1, 1), None), (key | Gd(2, i), 1, TRIES, 0, 0, D_(0), W, None)]
    assert ops == want
    # the shipped class records what the test's text records (the text is what runs on the reference)
    text = G._factory("cdk", W, W, 7, 8, 16, cls=G.text_class("cdk"), batch_size=1, _dry=True)
    assert text._dry_trace[1] == ops and np.array_equal(text._dry_trace[0], template)


def test_make_knows_the_colored_doorkey_id():
    from marlgrid_amd import envs as E
    name = "MarlGrid-2AgentColoredDoorKey8x8-v0"
    assert name in E.extension_envs and name not in E.registered_envs
    env = E.make(name, batch_size=1, _dry=True)
    assert isinstance(env, E.ColoredDoorKeyEnv) and (env.width, env.height, len(env.agents)) == (8, 8, 2)


def test_fork_of_a_plain_int_is_that_int_and_a_decided_draw_forks_no_more():
    seen = {}

    def gen(self, w, h):
        _room(self, w, h)
        seen["int"] = self._fork(5)
        seen["np"] = self._fork(np.int64(3))
        d = self._rand_int(4, 5)                             # a one-value range: decided
        seen["one"] = self._fork(d + 2)
        e = self._rand_int(1, 4)
        v = self._fork(10 - e)
        seen.setdefault("vals", []).append((v, self._fork(e), self._fork(e + 1)))      # forked before: no new fork
        self.put_obj(Wall(), e, 1)
    _, (_, ops) = _record(gen)
    assert seen["int"] == 5 and type(seen["int"]) is int and seen["np"] == 3 and type(seen["np"]) is int and seen["one"] == 6
    assert seen["vals"] == [(9, 1, 2), (8, 2, 3), (7, 3, 4)]
    assert ops == [(0, 1, -1, 4, 0, 5, 0, None), (1, 1, -1, 1, 0, 4, 0, None)] + [
        (1 | Gd(1, v), 1, 0, D_(1), 1, D_(1, 1), 2, None) for v in (1, 2, 3)]


def test_a_fork_free_gen_grid_records_what_it_recorded_before():
    """the tuples of tests/test_gen_draws_host.py (recorded by the commits before `_fork` existed), and no guard bit anywhere"""
    import product_envs
    from marlgrid_amd.envs import make
    D.register()
    progs = [make("MarlGrid-3AgentCluttered15x15-v0", batch_size=1, _dry=True)._dry_trace[1],
             product_envs.build("Test-2AgentLateStatic10x10", batch_size=1, _dry=True)._dry_trace[1]]
    progs += [D.build(name, batch_size=1, _dry=True)._dry_trace[1] for name in D.SCENARIOS]
    assert progs[0] == [(2, 1, 100, 0, 0, 15, 15, None)]
    assert progs[1][:3] == [(1, 6, 100, 0, 0, 10, 10, None), (2, 1, 0, 8, 8, 9, 9, None), (1, 1, 0, 2, 5, 8, 6, None)]
    assert progs[3] == [(0, 1, -1, 2, 0, 5, 0, None), (1, 1, 0, D_(0), 0, D_(0, 1), 7, None), (1, 1, -1, 1, 0, 6, 0, None),
                        (0, 1, 0, D_(0), D_(1), D_(0, 1), D_(1, 1), None), (2, 1, 100000, D_(0, 1), 0, 7, 7, None),
                        (1, 2, 100, 0, 0, D_(0), 7, None)]           # Draws-2AgentSplit7
    for ops in progs:
        assert all(0 <= op[0] <= 0xFF for op in ops)


def test_narrowed_intervals_make_the_proofs_per_path():
    def gen(self, w, h):
        _room(self, w, h)
        d = self._rand_int(0, 4)
        v = self._fork(d)
        if v >= 1:
            self.put_obj(Wall(), d - 1, 1)                   # provable only where d >= 1: refused without the fork
        self.place_obj(Goal(color="green", reward=1), top=(0, 0), size=(d + 1, h))
    _, (_, ops) = _record(gen)
    assert [op[0] for op in ops[1:]] == [2 | Gd(0, 0), 1 | Gd(0, 1), 2 | Gd(0, 1), 1 | Gd(0, 2), 2 | Gd(0, 2), 1 | Gd(0, 3), 2 | Gd(0, 3)]

    def unforked(self, w, h):
        _room(self, w, h)
        self.put_obj(Wall(), self._rand_int(0, 4) - 1, 1)
    with pytest.raises(ValueError):
        _record(unforked)

    def bad_in_one_branch(self, w, h):
        _room(self, w, h)
        d = self._rand_int(0, 4)
        if self._fork(d) == 3:
            self.put_obj(Wall(), d + w - 3, 1)               # x = w in this branch
    with pytest.raises(ValueError):
        _record(bad_in_one_branch)


# ---- refusals and bounds ------------------------------------------------------------------------------------------------------
def test_draws_still_refuse_to_branch_and_say_how_to():
    def gen(self, w, h):
        _room(self, w, h)
        if self._rand_int(0, 2) == 0:
            pass
    with pytest.raises(NotImplementedError, match="may compute with it .* cannot branch on it .*_fork"):
        _record(gen)


def test_the_helpers_outside_gen_grid_refuse():
    env, _ = _record(_room)
    for call in (lambda: env._rand_elem([1, 2]), env._rand_bool):
        with pytest.raises(NotImplementedError, match="cannot branch on it"):
            call()
    assert env._fork(4) == 4
    with pytest.raises(TypeError):
        env._fork("x")


def test_bound_fork_over_more_than_16_values():
    def gen(n):
        def g(self, w, h):
            _room(self, w, h)
            self._fork(self._rand_int(0, n))
        return g
    _, (_, ops) = _record(gen(16), W=20, H=20)
    assert len(ops) == 1                                     # 16 values: 16 paths that record nothing
    with pytest.raises(NotImplementedError, match="more than 16 values"):
        _record(gen(17), W=20, H=20)
    with pytest.raises(NotImplementedError, match="more than 16 values"):
        _record(lambda self, w, h: (_room(self, w, h), self._rand_elem(range(17))))


def test_bound_more_than_64_paths():
    def gen(n):
        def g(self, w, h):
            _room(self, w, h)
            self._rand_elem(range(8))
            self._rand_elem(range(n))
        return g
    _record(gen(8))                                          # 64 paths
    with pytest.raises(NotImplementedError, match="more than 64 paths"):
        _record(gen(9))


def test_bound_draw_registers_copies_included():
    def gen(n):
        def g(self, w, h):
            _room(self, w, h)
            for _ in range(n):
                self._rand_bool()
        return g
    _, (_, ops) = _record(gen(4))                            # four draws and three copies: 7 registers, 16 paths
    assert max(op[0] & 0xFF for op in ops if op[2] < 0) == 6

    def five(self, w, h):                                    # five draws, then forks: the fifth fork's copy would be register 9
        _room(self, w, h)
        ds = [self._rand_int(0, 2) for _ in range(5)]
        for d in ds:
            self._fork(d)
    with pytest.raises(NotImplementedError, match="MG_GEN_DRAWS"):
        _record(five)
    with pytest.raises(NotImplementedError, match="at most 8"):          # (a ninth plain draw: the existing bound)
        _record(lambda self, w, h: (_room(self, w, h), [self._rand_int(0, 2) for _ in range(9)]))


def test_bound_nested_fork_on_a_draw_that_may_be_255():
    def gen(lo):
        def g(self, w, h):
            _room(self, w, h)
            self._rand_bool()
            self._fork(self._rand_int(lo, lo + 2))           # inside a branch: the copy is draw + 1
        return g
    _, (_, ops) = _record(gen(253))                          # 253, 254: copies 254, 255
    assert ops[2] == (2 | Gd(0, 0), 1, -1, D_(1, 1), 0, D_(1, 2), 0, None) and ops[-1][0] & 0xFF == 2
    with pytest.raises(NotImplementedError, match="may be 255"):
        _record(gen(254))

    def top_level(self, w, h):                               # not inside a branch: guarded directly, no copy
        _room(self, w, h)
        self._fork(self._rand_int(254, 256))
    _record(top_level)


def test_grid_get_warns_on_cells_that_any_path_may_have_written():
    import warnings

    def gen(self, w, h):
        _room(self, w, h)
        if not self._rand_bool():                            # the SECOND path alone writes (3, 3) and samples column 5
            self.put_obj(Wall(), 3, 3)
            self.place_obj(Wall(), top=(5, 1), size=(1, 3), max_tries=10)
    env, _ = _record(gen)
    env._gen.active = True
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            env.grid.get(2, 2)
            assert not w
            env.grid.get(3, 3)
            env.grid.get(5, 2)
            assert len(w) == 2 and "may have filled" in str(w[0].message)
    finally:
        env._gen.active = False


def test_bound_more_than_max_gen_ops():
    def gen(self, w, h):
        _room(self, w, h)
        i = self._rand_elem(range(16))
        for j in range(33):                                  # 66 ops a branch, unmergeable: 16 x 66 > 1024
            self.place_obj(Wall(), max_tries=100)
            self.put_obj(None, 1 + (i + j) % 7, 1)
    with pytest.raises(NotImplementedError, match="MG_MAX_GEN"):
        _record(gen)


def test_agent_spawn_kwargs_that_differ_between_paths_refuse():
    def gen(self, w, h):
        _room(self, w, h)
        v = self._rand_elem([2, 3])
        self.agent_spawn_kwargs = dict(top=(0, 0), size=(v, h))
    with pytest.raises(ValueError, match="agent_spawn_kwargs"):
        _record(gen)

    def same(self, w, h):
        _room(self, w, h)
        self._rand_elem([2, 3])
        self.agent_spawn_kwargs = dict(top=(0, 0), size=(3, h))
    _record(same)


def test_a_gen_grid_that_is_no_function_of_its_draws_refuses():
    calls = []

    def gen(self, w, h):
        _room(self, w, h)
        calls.append(1)
        self._rand_int(1, 3 + len(calls))                    # another program before the fork at every run
        self._rand_bool()
    with pytest.raises(ValueError, match="not a function of its arguments and its draws"):
        _record(gen)


# ---- the interpreter on the host against the reference's trajectories ------------------------------------------------------
def _emu_rng(emu, b):
    return D.rng_digest(emu.numpy_rng_state(b))


def test_golden_conditions():
    """every path of every scenario occurs in at least one reset after the constructor's — on the golden's own arrays"""
    for name, (kind, W, *_rest) in G.SCENARIOS.items():
        g = G.golden(name)
        assert (g["seeds"] == G.SEEDS).all() and g["reset_after"].sum(axis=1).min() >= G.EPISODES - 1
        assert len(g["path_after_reset"]) == g["reset_after"].sum()
        seen = set(g["path_reset"].tolist()) | set(g["path_after_reset"].tolist())
        assert seen == set(range(len(G.paths(kind, W)))), name


@pytest.mark.parametrize("par", [False, True])
@pytest.mark.parametrize("name", sorted(G.SCENARIOS))
def test_host_emulation_vs_golden(name, par):
    import hostemu
    G.register()
    g = G.golden(name)
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
    for b in range(len(g["mt_final"])):
        assert seeding.same_stream(emu.numpy_rng_state(b), (g["mt_final"][b], g["mt_final_pos"][b]))
    assert not emu.error.any()


# ---- ... and against the live reference: 64 further seeds per scenario ----------------------------------------------------
@pytest.mark.reference
@pytest.mark.parametrize("name", sorted(G.SCENARIOS))
def test_host_emulation_vs_live_reference(name):
    import hostemu
    import refstate
    G.register()
    kind, W, H, view, tile, max_steps, _pix = G.SCENARIOS[name]
    seeds = 77000 + np.arange(64)
    S = len(seeds)
    emu = hostemu.HostEmu(name, S, seeds, par=True)
    refs = [G.ref_env(kind, W, H, view, tile, max_steps, s, render=False) for s in seeds]
    spec = emu.env.scenario_spec()

    def same(what):
        st = D.canonical_batch(spec, emu.grid[:, :W * H].reshape(S, W, H), emu.rec)
        for b, ref in enumerate(refs):
            c = refstate.canonical(ref)
            for k in D.CANON_KEYS:
                assert np.array_equal(np.asarray(st[k][b]), np.asarray(c[k])), (what, b, k)
            rs = ref.np_random.get_state()
            assert seeding.same_stream(emu.numpy_rng_state(b), (rs[1], rs[2])), (what, b)
    same("ctor")
    emu.reset()
    for ref in refs:
        ref.reset()
    same("reset")
    seen = set()
    for ref in refs:
        del ref.forked[:]
    arng = np.random.RandomState(5)
    for t in range(2 * max_steps):
        a = arng.randint(0, 7, size=(S, 2))
        r, d = emu.step(a)
        for b, ref in enumerate(refs):
            _, r2, d2, _ = ref.step(a[b])
            assert np.abs(r[b].astype(np.float64) - r2).max() <= REW_TOL and bool(d[b]) == bool(d2), (t, b)
        same("step %d" % t)
        if d.any():
            for b in np.nonzero(d)[0]:
                refs[b].reset()
                seen.add(G.take_path(refs[b], kind, W))
            emu.reset(env_mask=d)
            same("reset after step %d" % t)
    assert seen == set(range(len(G.paths(kind, W))))
    assert not emu.error.any()
