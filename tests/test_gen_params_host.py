"""CPU: per-env `_gen_grid` parameters on the host side — `self._param`, `place_obj(count=)`, `set_params`, `params`,
`scenario_spec()`, the checkpoint key and the shard splitting — on `_dry` envs (no device): what the recorder encodes against
the header's defines, and everything it refuses."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import param_envs as PE  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402
from marlgrid_amd import sharding as S  # noqa: E402
from marlgrid_amd.agents import GridAgentInterface  # noqa: E402
from marlgrid_amd.base import GenDraw, MultiGrid, MultiGridEnv  # noqa: E402
from marlgrid_amd.objects import Goal, Wall  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "marlgrid_hip.h")


def _defines():
    out = {}
    for m in re.finditer(r"^#define (MG_\w+) \(?(-?(?:0x)?[0-9A-Fa-f]+)\)?", open(HEADER).read(), re.M):
        out[m.group(1)] = int(m.group(2), 0)
    return out


def _env(gen, W=9, H=9, B=4, **kw):
    cls = type("T", (MultiGridEnv,), dict(_gen_grid=gen, mission="", metadata={}))
    return cls(agents=[GridAgentInterface(color="red", view_size=7, view_tile_size=8)], width=W, height=H, batch_size=B,
               _dry=True, **kw)


def _room(self, w, h):
    self.grid = MultiGrid((w, h))
    self.grid.wall_rect(0, 0, w, h)
    self.agent_spawn_kwargs = {}


def test_constants_follow_the_header_and_the_abi_stays_6():
    d = _defines()
    assert N.ABI_VERSION == 6 == d["MG_ABI_VERSION"]
    assert N.GEN_PARAM == d["MG_GEN_PARAM"] == -2
    assert (N.GEN_DRAWS, N.GEN_SYM, N.GEN_NEG, N.GEN_DRAW_SHIFT) == (d["MG_GEN_DRAWS"], d["MG_GEN_SYM"], d["MG_GEN_NEG"],
                                                                    d["MG_GEN_DRAW_SHIFT"])
    import ctypes as C
    assert C.sizeof(N.GenOp) == 32 and C.sizeof(N.GenProgram) == 40      # no struct changed


def test_op_encodings():
    env = PE.build("clutter", batch_size=4, _dry=True)
    _, ops = env._dry_trace
    # PARAM: obj = the register, max_tries = MG_GEN_PARAM, x0 / x1 = the interval, y0 = the table column
    assert ops[0] == (0, 1, N.GEN_PARAM, 0, 0, 21, 0, None)
    # the placement's count: `0 + draw[0]`
    wall = env.obj_reg.find(Wall())
    assert ops[1] == (wall, N.GEN_SYM | (0 << N.GEN_DRAW_SHIFT) | 0, 100, 0, 0, 11, 11, None)
    # ... `1 + draw[r]` under a guard, behind 34 ops (the long program); the PARAM is op 34, unguarded
    env = PE.build("long", batch_size=4, _dry=True)
    _, ops = env._dry_trace
    assert len(ops) > 32 and ops[34][:7] == (0, 1, N.GEN_PARAM, 0, 0, 5, 0)
    sym = [(i, op) for i, op in enumerate(ops) if op[2] > 0 and op[1] & N.GEN_SYM]
    assert [i > 34 and bool(op[0] & N.GEN_GUARD) for i, op in sym] == [True, True]
    assert sorted(op[1] & 0xFFFF for _, op in sym) == [0, 1]
    # a twin records plain ints: n calls merged into one op, nothing symbolic, no PARAM
    twin = PE.build("clutter", 7, batch_size=4, _dry=True)
    assert twin._dry_trace[1] == [(wall, 7, 100, 0, 0, 11, 11, None)] and twin.params_t is None
    assert PE.build("clutter", 0, batch_size=4, _dry=True)._dry_trace[1] == []


def test_int_count_is_n_calls_and_merges_with_its_neighbours():
    def a(self, w, h):
        _room(self, w, h)
        self.place_obj(Wall(), max_tries=100)
        self.place_obj(Wall(), max_tries=100, count=3)
        self.place_obj(Wall(), max_tries=100, count=0)
        self.place_obj(Wall(), max_tries=100)

    def b(self, w, h):
        _room(self, w, h)
        for _ in range(5):
            self.place_obj(Wall(), max_tries=100)
    assert _env(a)._dry_trace[1] == _env(b)._dry_trace[1] and _env(a)._dry_trace[1][0][1] == 5

    def c(self, w, h):                  # a symbolic count is an op of its own, before and after
        _room(self, w, h)
        self.place_obj(Wall(), max_tries=100)
        self.place_obj(Wall(), max_tries=100, count=self._param("n", 0, 4))
        self.place_obj(Wall(), max_tries=100)
    ops = _env(c)._dry_trace[1]
    assert [op[1] for op in ops if op[2] > 0] == [1, N.GEN_SYM, 1]


def test_a_param_is_used_like_a_draw():
    def gen(self, w, h):
        _room(self, w, h)
        p = self._param("p", 2, 5)
        assert isinstance(p, GenDraw) and isinstance(p + 1, GenDraw) and isinstance(7 - p, GenDraw)
        assert self._param("p", 2, 5).reg == p.reg                       # the same name: the same register, no second op
        self.grid.vert_wall(p, 1, h - 2)
        self.put_obj(None, p, p - 1)
        self.grid.horz_wall(1, p + 2, p)
        q = self._rand_int(1, p)                                         # a bound of a later draw
        self.put_obj(Goal(color="green", reward=1), q, 1)
        self.place_obj(Wall(), top=(p + 1, 1), size=(w - p - 2, h - 2), max_tries=100)
        v = self._fork(p)
        assert isinstance(v, int) and 2 <= v < 5
        self.put_obj(Wall(), v, h - 2)
    env = _env(gen)
    ops = env._dry_trace[1]
    assert sum(1 for op in ops if op[2] == N.GEN_PARAM) == 1
    assert sum(1 for op in ops if op[0] & N.GEN_GUARD) == 3              # one guarded fill per value of the fork
    assert list(env.params) == ["p"] and env.params["p"].tolist() == [2] * 4


def test_default_and_values_survive_a_re_record():
    def gen(self, w, h):
        _room(self, w, h)
        self.place_obj(Wall(), max_tries=100, count=self._param("n", 1, 9, default=getattr(self, "dflt", 4)))
    env = _env(gen)
    assert env.params["n"].tolist() == [4, 4, 4, 4]
    env.set_params(n=np.array([1, 2, 3, 8]))
    env.dflt = 6
    env.reset()                                                          # records `_gen_grid` again
    assert env.params["n"].tolist() == [1, 2, 3, 8]
    env.set_params(env_mask=np.array([True, False, False, True]), n=5)
    assert env.params["n"].tolist() == [5, 2, 3, 5]
    env.set_params(env_mask=np.array([False, True, False, False]), n=np.array([7, 7, 7, 7]))
    assert env.params["n"].tolist() == [5, 7, 3, 5]
    env.set_params(env_ids=[2, 0], n=[8, 1])
    assert env.params["n"].tolist() == [1, 7, 8, 5]
    env.set_params(env_ids=np.array([3]), n=2)
    assert env.params["n"].tolist() == [1, 7, 8, 2]
    assert env.params_t.shape == (4, N.GEN_DRAWS) and env.params_t.dtype == np.uint8 and not env.params_t[:, 1:].any()


def test_two_names_take_two_columns():
    def gen(self, w, h):
        _room(self, w, h)
        a, b = self._param("a", 1, 4), self._param("b", 0, 256, default=255)
        self.put_obj(Wall(), a, 1)
        self.place_obj(Wall(), max_tries=100, count=b - 250)             # proved for 0 .. 255? no: see the refusals
    with pytest.raises(ValueError, match="below 0"):
        _env(gen)

    def gen2(self, w, h):
        _room(self, w, h)
        a, b = self._param("a", 1, 4), self._param("b", 250, 256, default=255)
        self.put_obj(Wall(), a, 1)
        self.place_obj(Wall(), max_tries=100, count=b - 250)
    env = _env(gen2)
    assert [(op[0], op[4]) for op in env._dry_trace[1] if op[2] == N.GEN_PARAM] == [(0, 0), (1, 1)]
    assert env.params["a"].tolist() == [1] * 4 and env.params["b"].tolist() == [255] * 4
    spec = env.scenario_spec()["gen_reset"]
    assert ("param", 0, 0, 1, 4) in spec and ("param", 1, 1, 250, 256) in spec


def test_scenario_spec_lists_the_param_and_the_symbolic_count():
    env = PE.build("clutter", batch_size=2, _dry=True)
    spec = env.scenario_spec()["gen_reset"]
    wall = env.obj_reg.find(Wall())
    assert spec[-2:] == [("param", 0, 0, 0, 21), ("place", wall, N.GEN_SYM, 100)]
    env = PE.build("long", batch_size=2, _dry=True)
    guarded = [e for e in env.scenario_spec()["gen_reset"] if e[0] == "guard" and e[4][0] == "place_sym" and e[4][2] & N.GEN_SYM]
    assert len(guarded) == 2


# ---- every refusal ---------------------------------------------------------------------------------------------------------
def _refused(gen, exc, match, **kw):
    with pytest.raises(exc, match=match):
        _env(gen, **kw)


def test_refusals():
    def fill_outside_for_one_value(self, w, h):
        _room(self, w, h)
        self.put_obj(Wall(), self._param("p", 1, w + 1), 1)              # p == w: outside the grid
    _refused(fill_outside_for_one_value, ValueError, "not inside the 9 x 9 grid")

    def empty_rectangle_for_one_value(self, w, h):
        _room(self, w, h)
        p = self._param("p", 0, 4)
        self.place_obj(Wall(), top=(1, 1), size=(p, 3))                  # p == 0: nothing to sample
    _refused(empty_rectangle_for_one_value, ValueError, "sampling rectangle .* is empty")

    def draw_bounds_for_one_value(self, w, h):
        _room(self, w, h)
        self._rand_int(3, self._param("p", 3, 6))                        # p == 3: not high > low
    _refused(draw_bounds_for_one_value, ValueError, "not high > low")

    def negative_count_for_one_value(self, w, h):
        _room(self, w, h)
        self.place_obj(Wall(), count=self._param("p", 0, 4) - 1)
    _refused(negative_count_for_one_value, ValueError, "below 0")

    def negative_int_count(self, w, h):
        _room(self, w, h)
        self.place_obj(Wall(), count=-1)
    _refused(negative_int_count, ValueError, "not negative")

    def nine_registers(self, w, h):
        _room(self, w, h)
        for i in range(9):
            self._param("p%d" % i, 0, 2)
    _refused(nine_registers, NotImplementedError, "more than 8 draw registers")

    def draws_and_params_share_the_registers(self, w, h):
        _room(self, w, h)
        for i in range(4):
            self._rand_int(0, 2)
        for i in range(5):
            self._param("p%d" % i, 0, 2)
    _refused(draws_and_params_share_the_registers, NotImplementedError, "more than 8 draw registers")

    def another_interval(self, w, h):
        _room(self, w, h)
        self._param("p", 0, 4)
        self._param("p", 0, 5)
    _refused(another_interval, ValueError, r"declared as \[0, 4\) earlier")

    def outside_a_byte(self, w, h):
        _room(self, w, h)
        self._param("p", 0, 257)
    _refused(outside_a_byte, ValueError, "within 0..255")

    def empty_interval(self, w, h):
        _room(self, w, h)
        self._param("p", 3, 3)
    _refused(empty_interval, ValueError, "non-empty")

    def default_outside(self, w, h):
        _room(self, w, h)
        self._param("p", 1, 4, default=4)
    _refused(default_outside, ValueError, "default lies outside")

    def in_spawn_kwargs(self, w, h):
        _room(self, w, h)
        p = self._param("p", 1, 4)
        self.agent_spawn_kwargs = dict(top=(p, 1), size=(2, 2))
    _refused(in_spawn_kwargs, NotImplementedError, "agent_spawn_kwargs with a _rand_int draw")

    def in_reject_fn(self, w, h):
        _room(self, w, h)
        p = self._param("p", 1, 4)
        self.place_obj(Wall(), reject_fn=lambda pos: pos[0] < p)
    _refused(in_reject_fn, NotImplementedError, "cannot branch on it")

    def fork_over_too_many(self, w, h):
        _room(self, w, h)
        self._fork(self._param("p", 0, 17))
    _refused(fork_over_too_many, NotImplementedError, "more than 16 values")


def test_param_outside_gen_grid_and_count_on_the_live_grid():
    env = PE.build("clutter", batch_size=2, _dry=True)
    with pytest.raises(NotImplementedError, match="_param outside _gen_grid"):
        env._param("n", 0, 21)
    with pytest.raises(NotImplementedError, match="recorded placements of _gen_grid"):
        env.place_obj(Wall(), count=2)


def test_set_params_refuses_what_does_not_fit():
    env = PE.build("clutter", batch_size=4, _dry=True)
    for bad in (21, -1, [0, 0, 0, 21], np.array([0, 5, 300, 1])):
        with pytest.raises(ValueError, match="outside the parameter's interval"):
            env.set_params(n=bad)
    assert env.params["n"].tolist() == [0] * 4                           # nothing was written
    with pytest.raises(KeyError, match="no parameter"):
        env.set_params(m=1)
    with pytest.raises(ValueError, match="one value per env"):
        env.set_params(n=[1, 2, 3])
    with pytest.raises(ValueError, match="integer values"):
        env.set_params(n=1.5)
    with pytest.raises(ValueError, match="not both"):
        env.set_params(env_mask=np.ones(4, bool), env_ids=[0], n=1)
    with pytest.raises(ValueError, match="env_ids outside"):
        env.set_params(env_ids=[4], n=1)
    with pytest.raises(ValueError, match="shape"):
        env.set_params(env_mask=np.ones(3, bool), n=1)


# ---- the shipped scenario -----------------------------------------------------------------------------------------------
def test_cluttered_curriculum_id_and_the_untouched_class():
    from marlgrid_amd import envs as E
    env_id = "MarlGrid-3AgentClutteredCurriculum15x15-v0"
    assert env_id in E.extension_envs and env_id not in E.registered_envs
    env = E.make(env_id, batch_size=3, _dry=True)
    assert isinstance(env, E.ClutteredMultiGrid) and (env.width, env.height, len(env.agents)) == (15, 15, 3)
    assert env.agents[0].view_size == 7 and env.n_clutter_max == 50
    assert env.params["n_clutter"].tolist() == [25, 25, 25]
    wall = env.obj_reg.find(Wall())
    goal = env.obj_reg.find(Goal(color="green", reward=1))
    assert env._spec_ctor.ops == [(goal, 1, 100, 0, 0, 15, 15, None)]    # the constructor's reset: no clutter, as ever
    assert env._dry_trace[1] == [(0, 1, N.GEN_PARAM, 0, 0, 51, 0, None), (wall, N.GEN_SYM, 100, 0, 0, 15, 15, None)]
    # without the kwarg: the class as it was — no parameter, no table, the same program as before
    plain = E.make("MarlGrid-3AgentCluttered15x15-v0", batch_size=3, _dry=True)
    plain.reset()
    assert plain.params_t is None and plain.params == {} and plain._dry_trace[1] == [(wall, 25, 100, 0, 0, 15, 15, None)]
    with pytest.raises(KeyError):
        plain.set_params(n_clutter=3)


# ---- shards -----------------------------------------------------------------------------------------------------------------
def test_split_params_in_global_order():
    ranges = S.shard_ranges(10, 3)                                       # 4 + 3 + 3
    assert ranges == [(0, 4), (4, 7), (7, 10)]
    v = np.arange(10)
    parts = S.split_params(ranges, n=v, m=2)
    assert [p["n"].tolist() for p in parts] == [[0, 1, 2, 3], [4, 5, 6], [7, 8, 9]] and all(p["m"] == 2 for p in parts)
    mask = v % 2 == 0
    parts = S.split_params(ranges, env_mask=mask, n=v)
    assert [p["env_mask"].tolist() for p in parts] == [mask[lo:hi].tolist() for lo, hi in ranges]
    parts = S.split_params(ranges, env_ids=[9, 0, 5, 4], n=[90, 10, 50, 40])
    assert [(p["env_ids"].tolist(), list(p["n"])) for p in parts] == [([0], [10]), ([1, 0], [50, 40]), ([2], [90])]
    parts = S.split_params(ranges, env_ids=[1, 2], n=7)
    assert parts[1] is None and parts[2] is None and parts[0]["env_ids"].tolist() == [1, 2] and parts[0]["n"] == 7
    with pytest.raises(ValueError):
        S.split_params(ranges, env_ids=[10], n=1)
    with pytest.raises(ValueError):
        S.split_params(ranges, n=np.arange(9))
    with pytest.raises(ValueError):
        S.split_params(ranges, env_mask=mask, env_ids=[1], n=1)
    # applied shard by shard it is the one env's set_params
    one = PE.build("clutter", batch_size=10, _dry=True)
    shards = [PE.build("clutter", batch_size=hi - lo, _dry=True) for lo, hi in ranges]
    for kw in (dict(n=v + 3), dict(env_mask=mask, n=1), dict(env_ids=[9, 0, 5, 4], n=[20, 19, 18, 17]), dict(env_ids=[6], n=0)):
        one.set_params(**kw)
        for env, p in zip(shards, S.split_params(ranges, **kw)):
            if p is not None:
                env.set_params(**p)
        assert np.concatenate([e.params["n"] for e in shards]).tolist() == one.params["n"].tolist()


def test_checkpoints_carry_params_t_through_merge_and_split():
    import torch
    ranges = [(0, 2), (2, 5)]
    base = dict(grid_state=torch.zeros(5, 16, dtype=torch.uint8), version=torch.tensor(3))
    sd = dict(base, params_t=torch.arange(40, dtype=torch.uint8).reshape(5, 8))
    parts = S.split_state_dict(sd, ranges)
    assert [tuple(p["params_t"].shape) for p in parts] == [(2, 8), (3, 8)]
    assert torch.equal(S.merge_state_dicts(parts)["params_t"], sd["params_t"])
    with pytest.raises(KeyError):                                        # in every shard's dict or in none
        S.merge_state_dicts([parts[0], {k: v for k, v in parts[1].items() if k != "params_t"}])
