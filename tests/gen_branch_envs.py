"""TEST INFRASTRUCTURE — scenarios whose `_gen_grid` BRANCHES on random draws (`self._fork`, `self._rand_elem`,
`self._rand_bool`), once for the product (marlgrid_amd) and once on top of the reference's classes
(tests/golden/make_gen_branches.py, the live-parity tests), from the SAME `_gen_grid` text: on the reference's side the three
helpers are gym-minigrid's own and `_fork` hands its argument back.  Built like tests/draw_envs.py, whose comparison helpers
this module uses.

The goldens are tests/golden/genbranch_<name>.npz: the key layout of gendraws_<name>.npz plus the id of the path — an index
into `paths(kind)` — that every reset took: path_ctor [S], path_reset [S], path_after_reset [reset_after.sum()].

`spec` restates every scenario BY HAND for the CPU oracle — a branch is an `if` block there, `lst[i]` a lookup —, and
`oracle_path` reads the path the oracle took off what it drew (tests/test_oracle_gen_branches.py, tests/branch_diff.py).
"""
import os

import numpy as np

import draw_envs as D

GOLD = D.GOLD
SEEDS = 2024 + np.arange(16)
N_AGENTS = D.N_AGENTS
COLORS = D.COLORS
EPISODES = 3

# name -> (kind, W, H, view_size, tile_size, max_steps, pixels pinned)
SCENARIOS = {
    "Branch-2AgentChoice7": ("choice", 7, 7, 7, 8, 12, True),
    "Branch-2AgentChoice7-ts5": ("choice", 7, 7, 7, 5, 12, True),
    "Branch-2AgentSides9": ("sides", 9, 9, 7, 8, 12, True),
    "Branch-2AgentLong12": ("long", 12, 12, 7, 8, 12, True),
    # (the reference's Door / Key sprites raise: state, encodings and encoded views only)
    "Branch-2AgentColoredDoorKey6": ("cdk", 6, 6, 7, 8, 16, False),
    "Branch-2AgentColoredDoorKey8": ("cdk", 8, 8, 7, 8, 16, False),
}
# no golden: pinned through the oracle, and the oracle on it through the live-reference cases (as draw_envs.ORACLE_ONLY).
# Non-square; forks nested three deep behind five draws, so that the recorded program guards on registers 4, 5 and 6
ORACLE_ONLY = {
    "Branch-2AgentDeep12x10": ("deep", 12, 10, 7, 8, 12, True),
}
DEEP = "Branch-2AgentDeep12x10"
DOOR_COLORS = ("red", "green", "blue", "purple", "yellow", "grey")
GOALS = (("green", 1), ("blue", 2), ("red", 0.5))       # Choice: (colour, reward) of the three goals
LONG_K = (2, 3, 5)                                      # Long: the values `_rand_elem` chooses from
LONG_FORK_AT = 9                                        # ... after this many placement / fill pairs


def gen_grid_text(kind, ns):
    """the `_gen_grid` of a test scenario over a namespace with MultiGrid / Wall / Goal / Door / Key (product or reference)"""
    MultiGrid, Wall, Goal, Door, Key = ns["MultiGrid"], ns["Wall"], ns["Goal"], ns["Door"], ns["Key"]

    def choice(self, width, height):
        self.grid = MultiGrid((width, height))
        self.grid.wall_rect(0, 0, width, height)
        goal = self._rand_elem([Goal(color=c, reward=r) for c, r in GOALS])        # an OBJECT chosen by a draw
        self.place_obj(goal)
        for _ in range(2):
            self.place_obj(Wall(), max_tries=100)
        self.agent_spawn_kwargs = {}

    def sides(self, width, height):
        self.grid = MultiGrid((width, height))
        self.grid.wall_rect(0, 0, width, height)
        s = self._rand_int(2, width - 2)                        # the splitting column
        self.grid.vert_wall(s, 0)
        g = self._rand_int(1, height - 1)                       # the gap in it
        self.put_obj(None, s, g)
        if self._fork(s) < 4:                                   # the layout depends on where the split fell
            self.place_obj(Goal(color="green", reward=1), top=(s + 1, 0), size=(width - s - 1, height))
            e = self._rand_int(1, height - 1)                   # a draw that only this branch makes
            self.put_obj(Wall(), width - 2, e)
        else:
            self.place_obj(Goal(color="green", reward=1), top=(0, 0), size=(s, height))
        if self._rand_bool():                                   # a fork on a second draw, inside either branch
            self.put_obj(Wall(), 1, 1)
        self.agent_spawn_kwargs = {}

    def long_program(self, width, height):
        self.grid = MultiGrid((width, height))
        self.grid.wall_rect(0, 0, width, height)
        k = 0
        for i in range(17):                                     # a placement and a fill, alternating
            self.place_obj(Wall(), max_tries=100)
            self.put_obj(None, 1 + (i + k) % (width - 2), 1)
            if i == LONG_FORK_AT:                               # ops 0 .. 19 are common; the branches begin at op 21
                k = self._rand_elem(LONG_K)
        self.grid.horz_wall(2, height - 3, k)                   # a length that is a forked value
        if self._rand_bool():
            self.put_obj(None, 2, height - 3)
        self.place_obj(Goal(color="green", reward=1), max_tries=100)
        self.agent_spawn_kwargs = {}

    def cdk(self, width, height):
        """marlgrid_amd.envs.ColoredDoorKeyEnv, restated (the host tests assert that the two record the same program)"""
        self.grid = MultiGrid((width, height))
        self.grid.wall_rect(0, 0, width, height)
        self.put_obj(Goal(color="green", reward=1), width - 2, height - 2)
        split = self._rand_int(2, width - 2)
        self.grid.vert_wall(split, 0)
        door = self._rand_int(1, width - 2)
        color = self._rand_elem(DOOR_COLORS)
        self.put_obj(Door(color=color, state=Door.states.locked), split, door)
        self.place_obj(obj=Key(color), top=(0, 0), size=(split, height))
        self.agent_spawn_kwargs = {}

    def deep(self, width, height):
        """five draws, then forks three deep: on the `_rand_elem` draw itself (register 4), inside its middle value on `t`,
        inside t's highest value on `n` — and only where n is at its lowest a draw bounded by the gap row `b`.  At 12 x 10:
        a 3..8, b 1..8, n 1..3, t 0..2.  The tail — `n - 1` wall blocks, none where n is 1 — is every path's."""
        self.grid = MultiGrid((width, height))
        self.grid.wall_rect(0, 0, width, height)
        a = self._rand_int(3, width - 3)                        # 0: the splitting column
        self.grid.vert_wall(a, 0)
        b = self._rand_int(1, height - 1)                       # 1: the gap in it
        self.put_obj(None, a, b)
        n = self._rand_int(1, 4)                                # 2
        t = self._rand_int(0, 3)                                # 3
        goal = self._rand_elem([Goal(color=c, reward=r) for c, r in GOALS])    # 4, forked: an OBJECT chosen by a draw
        self.place_obj(goal, top=(a + 1, 0), size=(width - a - 1, height))
        if goal.color == GOALS[1][0]:                           # the middle value of its draw
            v = self._fork(t)
            if v == 2:                                          # the high end of its draw
                m = self._fork(n)
                if m == 1:                                      # the low end of its draw
                    d = self._rand_int(1, b + 1)                # bounded by an earlier draw; only on this path
                    self.put_obj(Wall(), 1, d)
                elif m == 3:
                    self.put_obj(Wall(), 2, 1)
            elif v == 0:
                self.put_obj(Wall(), 1, 1)
        self.place_obj(Wall(), top=(0, 0), size=(a, height), max_tries=100, count=n - 1)      # 0, 1 or 2 blocks
        self.agent_spawn_kwargs = {}

    return dict(choice=choice, sides=sides, long=long_program, cdk=cdk, deep=deep)[kind]


def paths(kind, W=None):
    """every path of a scenario: the tuple of the values `_fork` is handed, in call order"""
    if kind == "choice":
        return [(i,) for i in range(3)]
    if kind == "sides":
        return [(s, b) for s in range(2, W - 2) for b in (0, 1)]
    if kind == "long":
        return [(i, b) for i in range(3) for b in (0, 1)]
    if kind == "deep":                                          # (the goal's index, then t where it is 1, then n where t is 2)
        return [(0,), (1, 0), (1, 1), (1, 2, 1), (1, 2, 2), (1, 2, 3), (2,)]
    return [(i,) for i in range(6)]


# ---- the scenarios restated BY HAND for the oracle (oracle/oracle.py:make_config) -------------------------------------------
# Written from the `_gen_grid` texts above, NOT from the product's recorder or its scenario_spec(): what Python does with a
# forked value is an `if` here, not a guard on every op, and `lst[i]` is a lookup, not one branch per element.
#   ("if", value, lo, hi) ... ("else",) ... ("endif",)       `if lo <= value <= hi:`; value as a coordinate is (draw_envs.dr)
#   an object may be ("sel", reg, (id0, id1, ...))            `lst[draw[reg]]` of a `_rand_elem` over objects
#   a count of place / place_sym may be an operand            `count=n - 1`: that many place_obj calls, below 1 none
ELSE, ENDIF = ("else",), ("endif",)
dr = D.dr


def if_eq(value, k):
    return ("if", value, k, k)


def switch(value, cases):
    """`if value == k0: ... elif value == k1: ... ` (no final else): cases is [(k, ops), ...]"""
    out = []
    for i, (k, ops) in enumerate(cases):
        out += [if_eq(value, k)] + list(ops) + ([ELSE] if i + 1 < len(cases) else [])
    return out + [ENDIF] * len(cases)


_WALL, _GOAL = D._WALL, D._GOAL
_GOALS = [dict(type="Goal", color=c, state=0, reward=r) for c, r in GOALS]


def _door_and_key(color):
    """a locked Door registers its other two states behind it (open, closed), then the Key"""
    return [dict(type="Door", color=color, state=st) for st in (3, 1, 2)] + [dict(type="Key", color=color, state=0)]


def spec(kind, W, H, view=7, tile=8, max_steps=12):
    s = dict(W=W, H=H, agents=[dict(color=c) for c in COLORS], view_size=view, tile_size=tile, view_offset=0,
             see_through_walls=False, max_steps=max_steps, reward_decay=True, ghost_mode=True, respawn=False, wall_obj=1)
    room = ("wall_rect", 0, 0, W, H)
    col = lambda r: (dr(r), 0, dr(r, 1), H)                             # vert_wall(draw[r], 0): the whole column
    cell = lambda x, y: (x, y) + tuple(("d", v[1], v[2], v[3] + 1) if isinstance(v, tuple) else v + 1 for v in (x, y))
    tries = D.DEFAULT_TRIES
    if kind == "choice":
        s["objects"] = [None, _WALL] + _GOALS
        prog = [room, ("draw", 0, 0, 3), ("place", ("sel", 0, (2, 3, 4)), 1, tries), ("place", 1, 2, 100)]
    elif kind == "sides":
        s["objects"] = [None, _WALL, _GOAL]
        prog = [room, ("draw", 0, 2, W - 2), ("fill", 1) + col(0), ("draw", 1, 1, H - 1), ("fill", 0) + cell(dr(0), dr(1)),
                ("if", dr(0), -2 ** 30, 3),                                         # if s < 4:
                ("place_sym", 2, 1, tries, dr(0, 1), 0, W, H),                      # top (s + 1, 0), size (W - s - 1, H)
                ("draw", 2, 1, H - 1), ("fill", 1) + cell(W - 2, dr(2)),
                ELSE, ("place_sym", 2, 1, tries, 0, 0, dr(0), H), ENDIF,            # top (0, 0), size (s, H)
                ("draw", 3, 0, 2), if_eq(dr(3), 0), ("put", 1, 1, 1), ENDIF]        # _rand_bool(): randint(0, 2) == 0
    elif kind == "long":
        s["objects"] = [None, _WALL, _GOAL]
        step = lambda i, k: [("place", 1, 1, 100), ("put", 0, 1 + (i + k) % (W - 2), 1)]
        prog = [room]
        for i in range(LONG_FORK_AT + 1):
            prog += step(i, 0)
        prog += [("draw", 0, 0, len(LONG_K))]                                       # k = LONG_K[draw]: enters `%`, so per value
        prog += switch(dr(0), [(j, sum((step(i, k) for i in range(LONG_FORK_AT + 1, 17)), []) + [("horz_wall", 2, H - 3, k)])
                               for j, k in enumerate(LONG_K)])
        prog += [("draw", 1, 0, 2), if_eq(dr(1), 0), ("put", 0, 2, H - 3), ENDIF, ("place", 2, 1, 100)]
    elif kind == "cdk":
        s["objects"] = [None, _WALL, _GOAL] + sum((_door_and_key(c) for c in DOOR_COLORS), [])
        doors = tuple(3 + 4 * i for i in range(len(DOOR_COLORS)))
        keys = tuple(6 + 4 * i for i in range(len(DOOR_COLORS)))
        prog = [room, ("put", 2, W - 2, H - 2), ("draw", 0, 2, W - 2), ("fill", 1) + col(0),
                ("draw", 1, 1, W - 2), ("draw", 2, 0, len(DOOR_COLORS)),            # (the door ROW from the width, as DoorKey)
                ("fill", ("sel", 2, doors)) + cell(dr(0), dr(1)), ("place_sym", ("sel", 2, keys), 1, tries, 0, 0, dr(0), H)]
    elif kind == "deep":
        s["objects"] = [None, _WALL] + _GOALS
        a, b, n, t, i, d = range(6)
        prog = [room, ("draw", a, 3, W - 3), ("fill", 1) + col(a), ("draw", b, 1, H - 1), ("fill", 0) + cell(dr(a), dr(b)),
                ("draw", n, 1, 4), ("draw", t, 0, 3), ("draw", i, 0, 3),
                ("place_sym", ("sel", i, (2, 3, 4)), 1, tries, dr(a, 1), 0, W, H),
                if_eq(dr(i), 1),
                if_eq(dr(t), 2),
                if_eq(dr(n), 1), ("draw", d, 1, dr(b, 1)), ("fill", 1) + cell(1, dr(d)),
                ELSE, if_eq(dr(n), 3), ("put", 1, 2, 1), ENDIF, ENDIF,
                ELSE, if_eq(dr(t), 0), ("put", 1, 1, 1), ENDIF, ENDIF,
                ENDIF,
                ("place_sym", 1, dr(n, -1), 100, 0, 0, dr(a), H)]
    s["gen_ctor"], s["gen_reset"] = prog, list(prog)
    return s


def spec_of(name, **kw):
    kind, W, H, view, tile, max_steps, _pix = dict(SCENARIOS, **ORACLE_ONLY)[name]
    return spec(kind, W, H, view, tile, kw.get("max_steps", max_steps))


def oracle_path(kind, W, orc):
    """the id (an index into `paths`) of the path the ORACLE's last `_gen_grid` took, from what it drew: the values that the
    text hands to `_fork`, in call order — a register that an untaken block would have drawn reads -1"""
    d, w = orc.draws()
    if kind == "choice":
        p = (d[0],)
    elif kind == "sides":
        p = (d[0], d[3])
    elif kind == "long":
        p = (d[0], d[1])
    elif kind == "cdk":
        p = (d[2],)
    else:                                                       # deep: the goal, t inside goal 1, n inside t == 2
        p = (d[4],) + ((d[3],) + ((d[2],) if d[3] == 2 else ()) if d[4] == 1 else ())
    return paths(kind, W).index(tuple(int(v) for v in p))


# ---- product side -----------------------------------------------------------------------------------------------------
def product_class(kind):
    from marlgrid_amd import envs as E
    from marlgrid_amd.base import MultiGrid, MultiGridEnv
    from marlgrid_amd.objects import Door, Goal, Key, Wall
    if kind == "cdk":
        return E.ColoredDoorKeyEnv
    ns = dict(MultiGrid=MultiGrid, Wall=Wall, Goal=Goal, Door=Door, Key=Key)
    return type("Branch%sEnv" % kind.capitalize(), (MultiGridEnv,), dict(_gen_grid=gen_grid_text(kind, ns), mission="", metadata={}))


def text_class(kind):
    """the product's classes under the scenario's text, whatever the kind (cdk: to compare with the shipped class)"""
    from marlgrid_amd.base import MultiGrid, MultiGridEnv
    from marlgrid_amd.objects import Door, Goal, Key, Wall
    ns = dict(MultiGrid=MultiGrid, Wall=Wall, Goal=Goal, Door=Door, Key=Key)
    return type("BranchText%sEnv" % kind.capitalize(), (MultiGridEnv,), dict(_gen_grid=gen_grid_text(kind, ns), mission="", metadata={}))


def _factory(kind, W, H, view, tile, max_steps, cls=None, **kw):
    from marlgrid_amd.agents import GridAgentInterface
    agents = [GridAgentInterface(color=c, view_size=view, view_tile_size=tile) for c in COLORS]
    return (cls or product_class(kind))(agents=agents, **dict(dict(width=W, height=H, max_steps=max_steps), **kw))


def register():
    import functools
    from marlgrid_amd import envs as E
    for name, (kind, W, H, view, tile, max_steps, _pix) in dict(SCENARIOS, **ORACLE_ONLY).items():
        E._registry.setdefault(name, functools.partial(_factory, kind, W, H, view, tile, max_steps=max_steps))


def build(name, **kw):
    from marlgrid_amd import envs as E
    register()
    return E.make(name, **kw)


# ---- reference side (build container only) ------------------------------------------------------------------------------
def ref_env(kind, W, H, view, tile, max_steps, seed, render=True):
    """the scenario on top of the reference's classes; the helpers as gym-minigrid defines them, `_fork` the identity.  Every
    value `_fork` is handed goes to `env.forked` (a list the caller empties): the path a reset took.  render=False (and
    cdk always: the reference's Door / Key sprites raise): gen_agent_obs stubbed out"""
    import refload
    refload.load()
    from marlgrid.agents import GridAgentInterface
    from marlgrid.base import MultiGrid, MultiGridEnv
    from marlgrid.objects import Door, Goal, Key, Wall

    def _rand_int(self, low, high):
        return self.np_random.randint(low, high)

    def _rand_elem(self, iterable):
        lst = list(iterable)
        return lst[self._fork(self._rand_int(0, len(lst)))]

    def _rand_bool(self):
        return self._fork(self.np_random.randint(0, 2)) == 0

    def _fork(self, d):
        self.__dict__.setdefault("forked", []).append(int(d))
        return d
    ns = dict(MultiGrid=MultiGrid, Wall=Wall, Goal=Goal, Door=Door, Key=Key)
    body = dict(_gen_grid=gen_grid_text(kind, ns), _rand_int=_rand_int, _rand_elem=_rand_elem, _rand_bool=_rand_bool, _fork=_fork,
                mission="", metadata={})
    if kind == "cdk" or not render:
        body["gen_agent_obs"] = lambda self, agent: None
    if kind == "deep":
        def place_obj(self, obj, count=1, **kw):                # the product's `count=`: that many consecutive calls
            for _ in range(count):
                MultiGridEnv.place_obj(self, obj, **kw)
        body["place_obj"] = place_obj
    cls = type("RefBranch" + kind, (MultiGridEnv,), body)
    agents = [GridAgentInterface(color=c, view_size=view, view_tile_size=tile) for c in COLORS]
    return cls(agents=agents, width=W, height=H, max_steps=max_steps, seed=int(seed))


def take_path(env, kind, W):
    """the id of the path of the reference env's last `_gen_grid`, and forget it"""
    p = tuple(env.forked)
    del env.forked[:]
    return paths(kind, W).index(p)


# ---- fixtures and what a state says about its path ---------------------------------------------------------------------------
def golden(name):
    with np.load(os.path.join(GOLD, "genbranch_%s.npz" % name)) as z:
        g = {k: z[k] for k in z.files}
    g["rng_next"] = g["rng_step"].copy()
    g["rng_next"][g["reset_after"]] = g.pop("rng_after_reset")
    return g


def sides_path(grid, wall_id):
    """the path ids of a (B, W, H) array of Sides object ids: the split column is the interior column that is wall but for
    one gap, the second fork's wall stands at (1, 1) or does not (nothing else writes that cell but the goal, which it replaces)"""
    B, W, H = grid.shape
    full = (grid[:, 2:W - 2, 1:H - 1] == wall_id).sum(axis=2) >= H - 3
    assert (full.sum(axis=1) == 1).all(), "not exactly one split column"
    s = 2 + full.argmax(axis=1)
    b = np.where(grid[:, 1, 1] == wall_id, 0, 1)            # `_rand_bool()` is `draw == 0`
    return (s - 2) * 2 + b
