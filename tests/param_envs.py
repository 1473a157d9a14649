"""TEST INFRASTRUCTURE — scenarios whose `_gen_grid` reads a per-env PARAMETER (`self._param`, a PARAM op of the reset program)
and their constant TWINS: the same `_gen_grid` text with the value as a Python constant.  A mixed batch must equal, env by
env, the twin of that env's value built with the same seeds — `register()` makes `Param-<kind>` (the parameter env) and
`Param-<kind>-v<value>` (its twins) known to `marlgrid_amd.envs.make`, which is how tests/native/hostemu.py builds an env.

  clutter   a symbolic COUNT: 0 .. 20 wall blocks on 11 x 11
  split     a wall column at `s`, its gap at row `s + 1`, a block at (`s - 1`, `s`), the goal right of the column and two
            blocks left of it (place_obj regions from `s`), on 9 x 9
  kind      `_fork` on a parameter with 3 values — a Goal, a Key or a Ball — nested under a `_rand_bool` fork
            (no Box: toggling one is the reference's TypeError, and the differentials against the oracle act at random)
  long      more than 32 ops; the PARAM op and a guarded symbolic-count op lie behind the first 32
"""
import functools

import numpy as np

COLORS = ("red", "blue")
# kind -> (W, H, parameter name, low, high)   (the interval is [low, high))
KINDS = {
    "clutter": (11, 11, "n", 0, 21),
    "split": (9, 9, "s", 2, 7),
    "kind": (8, 8, "k", 0, 3),
    "long": (12, 12, "n", 0, 5),
}


def interval(kind):
    return KINDS[kind][3], KINDS[kind][4]


def values(kind, B):
    """the parameter's values cycled over the whole interval"""
    lo, hi = interval(kind)
    return (lo + np.arange(B) % (hi - lo)).astype(np.int64)


def _gen_grid_of(kind):
    from marlgrid_amd.base import MultiGrid
    from marlgrid_amd.objects import Ball, Goal, Key, Wall
    _, _, pname, lo, hi = KINDS[kind]

    def P(self):
        """the parameter, or the twin's constant"""
        return self._param(pname, lo, hi) if self.twin_value is None else int(self.twin_value)

    def clutter(self, width, height):
        self.grid = MultiGrid((width, height))
        self.grid.wall_rect(0, 0, width, height)
        self.put_obj(Goal(color="green", reward=1), width - 2, height - 2)
        self.place_obj(Wall(), max_tries=100, count=P(self))
        self.agent_spawn_kwargs = {}

    def split(self, width, height):
        self.grid = MultiGrid((width, height))
        self.grid.wall_rect(0, 0, width, height)
        s = P(self)
        self.grid.vert_wall(s, 0)
        self.put_obj(None, s, s + 1)
        self.put_obj(Wall(), s - 1, s)
        self.place_obj(Goal(color="green", reward=1), top=(s + 1, 0), size=(width - s - 1, height))
        self.place_obj(Wall(), top=(0, 0), size=(s, height), max_tries=100, count=2)
        self.agent_spawn_kwargs = {}

    def kind_(self, width, height):
        self.grid = MultiGrid((width, height))
        self.grid.wall_rect(0, 0, width, height)
        k = P(self)
        objs = (Goal(color="green", reward=1), Key("blue"), Ball(color="red"))
        for o in objs:                                          # (the same object ids in the parameter env and in every twin)
            self.obj_reg.get_key(o)
        if self._rand_bool():
            self.put_obj(Wall(), 3, 3)
            self.place_obj(objs[self._fork(k)], max_tries=100)
        else:
            self.place_obj(Goal(color="green", reward=1), top=(1, 1), size=(3, 3))
        self.place_obj(Wall(), max_tries=100)
        self.agent_spawn_kwargs = {}

    def long_(self, width, height):
        self.grid = MultiGrid((width, height))
        self.grid.wall_rect(0, 0, width, height)
        for i in range(17):                                     # 34 ops: a placement and a fill, alternating
            self.place_obj(Wall(), max_tries=100)
            self.put_obj(None, 1 + i % (width - 2), 1)
        n = P(self)                                             # op 34: behind the LDS copy's 32
        if self._rand_bool():
            self.place_obj(Wall(), top=(1, 2), size=(width - 2, height - 3), max_tries=100, count=n)
        else:
            self.place_obj(Wall(), top=(1, 2), size=(width - 2, height - 3), max_tries=100, count=n + 1)
        self.place_obj(Goal(color="green", reward=1), max_tries=100)
        self.agent_spawn_kwargs = {}

    return dict(clutter=clutter, split=split, kind=kind_, long=long_)[kind]


def product_class(kind):
    from marlgrid_amd.base import MultiGridEnv
    return type("Param%sEnv" % kind.capitalize(), (MultiGridEnv,),
                dict(_gen_grid=_gen_grid_of(kind), mission="", metadata={}, twin_value=None))


def _factory(kind, twin_value, max_steps=10, view=7, **kw):
    from marlgrid_amd.agents import GridAgentInterface
    W, H = KINDS[kind][:2]
    agents = [GridAgentInterface(color=c, view_size=view, view_tile_size=8) for c in COLORS]
    cls = product_class(kind)
    if twin_value is not None:
        cls = type(cls.__name__ + "Twin", (cls,), dict(twin_value=int(twin_value)))
    return cls(agents=agents, width=W, height=H, max_steps=max_steps, **kw)


def name_of(kind, twin_value=None):
    return "Param-%s" % kind if twin_value is None else "Param-%s-v%d" % (kind, twin_value)


def register():
    from marlgrid_amd import envs as E
    for kind in KINDS:
        lo, hi = interval(kind)
        for v in [None] + list(range(lo, hi)):
            E._registry.setdefault(name_of(kind, v), functools.partial(_factory, kind, v))


# ---- the scenarios restated BY HAND for the oracle (oracle/oracle.py:make_config) -------------------------------------------
# Written from the `_gen_grid` texts above, in the notation of tests/gen_branch_envs.py:spec.  `spec(kind)` reads the parameter
# with ("param", 0, name) — the oracle takes what OracleEnv.set_params gave it, as given —; `spec(kind, twin_value=v)` has the
# Python constant v wherever the text has the parameter, and no param entry.
def spec(kind, twin_value=None, max_steps=10, view=7, tile=8):
    import draw_envs as D
    import gen_branch_envs as G
    W, H, pname, lo, hi = KINDS[kind]
    dr, if_eq, ELSE, ENDIF = D.dr, G.if_eq, G.ELSE, G.ENDIF
    s = dict(W=W, H=H, agents=[dict(color=c) for c in COLORS], view_size=view, tile_size=tile, view_offset=0,
             see_through_walls=False, max_steps=max_steps, reward_decay=True, ghost_mode=True, respawn=False, wall_obj=1)
    s["objects"] = [None, D._WALL, D._GOAL]
    tries = D.DEFAULT_TRIES
    twin = twin_value is not None
    p = (lambda c=0: int(twin_value) + c) if twin else (lambda c=0: dr(0, c))         # the parameter + c
    load = [] if twin else [("param", 0, pname)]
    if not twin:
        s["params"] = [(pname, lo)]                                                  # `_param`'s default: the interval's low end
    room = ("wall_rect", 0, 0, W, H)
    if kind == "clutter":
        prog = [room, ("put", 2, W - 2, H - 2)] + load + [("place", 1, p(), 100)]
    elif kind == "split":
        prog = [room] + load + [("fill", 1, p(), 0, p(1), H),                         # vert_wall(s, 0)
                                ("fill", 0, p(), p(1), p(1), p(2)),                   # put_obj(None, s, s + 1)
                                ("fill", 1, p(-1), p(), p(), p(1)),                   # put_obj(Wall(), s - 1, s)
                                ("place_sym", 2, 1, tries, p(1), 0, W, H),            # top (s + 1, 0), size (W - s - 1, H)
                                ("place_sym", 1, 2, 100, 0, 0, p(), H)]               # top (0, 0), size (s, H), twice
    elif kind == "kind":
        s["objects"] = [None, D._WALL, D._GOAL, dict(type="Key", color="blue", state=0), dict(type="Ball", color="red", state=0)]
        objs = (2, 3, 4)
        chosen = objs[int(twin_value)] if twin else ("sel", 0, objs)                  # objs[k]
        prog = [room] + load + [("draw", 1, 0, 2), if_eq(dr(1), 0), ("put", 1, 3, 3), ("place", chosen, 1, 100),
                                ELSE, ("place_sym", 2, 1, tries, 1, 1, 4, 4), ENDIF,  # top (1, 1), size (3, 3)
                                ("place", 1, 1, 100)]
    elif kind == "long":
        prog = [room]
        for i in range(17):
            prog += [("place", 1, 1, 100), ("put", 0, 1 + i % (W - 2), 1)]
        region = (1, 2, W - 1, H - 1)                                                 # top (1, 2), size (W - 2, H - 3)
        prog += load + [("draw", 1, 0, 2), if_eq(dr(1), 0), ("place_sym", 1, p(), 100) + region,
                        ELSE, ("place_sym", 1, p(1), 100) + region, ENDIF, ("place", 2, 1, 100)]
    s["gen_ctor"], s["gen_reset"] = prog, list(prog)
    return s


def build(kind, twin_value=None, **kw):
    from marlgrid_amd import envs as E
    register()
    return E.make(name_of(kind, twin_value), **kw)
