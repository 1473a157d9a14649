"""TEST INFRASTRUCTURE — scenarios whose `_gen_grid` BRANCHES on random draws (`self._fork`, `self._rand_elem`,
`self._rand_bool`), once for the product (marlgrid_amd) and once on top of the reference's classes
(tests/golden/make_gen_branches.py, the live-parity tests), from the SAME `_gen_grid` text: on the reference's side the three
helpers are gym-minigrid's own and `_fork` hands its argument back.  Built like tests/draw_envs.py, whose comparison helpers
this module uses.

The goldens are tests/golden/genbranch_<name>.npz: the key layout of gendraws_<name>.npz plus the id of the path — an index
into `paths(kind)` — that every reset took: path_ctor [S], path_reset [S], path_after_reset [reset_after.sum()].
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

    return dict(choice=choice, sides=sides, long=long_program, cdk=cdk)[kind]


def paths(kind, W=None):
    """every path of a scenario: the tuple of the values `_fork` is handed, in call order"""
    if kind == "choice":
        return [(i,) for i in range(3)]
    if kind == "sides":
        return [(s, b) for s in range(2, W - 2) for b in (0, 1)]
    if kind == "long":
        return [(i, b) for i in range(3) for b in (0, 1)]
    return [(i,) for i in range(6)]


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
    for name, (kind, W, H, view, tile, max_steps, _pix) in SCENARIOS.items():
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
