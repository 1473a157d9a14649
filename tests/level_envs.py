"""TEST INFRASTRUCTURE — the scenarios whole levels (seed, parameters, cell edits) are played on, restated BY HAND for the
oracle, and what the level tests share: the rule that says which entries of a product edit table count, random edit lists,
and the reference-side class whose `_gen_grid` ends with `for x, y, o in self.level: self.grid.set(x, y, o)`.

  CURRICULUM  `MarlGrid-3AgentClutteredCurriculum15x15-v0`: ClutteredMultiGrid 15 x 15, 3 agents, the number of wall blocks a
              per-env parameter `n_clutter` in [0, 51), 25 where nothing was set
  EDITS       tests/edit_envs.py's `Edits-Cluttered15` with two further kinds registered through `env.edit_key`: a blue Key (3)
              and a red Ball (4).  No Box: toggling one is the reference's TypeError, and the differentials act at random.

An oracle entry is (x, y, obj_id); a product entry is (x, y, kind, on).  The product ignores an entry that is off, outside the
grid or of a kind without a descriptor; the oracle is never given one: `valid` is that rule written out from the README's
words, not imported from marlgrid_amd/gen_edits.py."""
import numpy as np

import edit_envs as EE
import scenarios

CURRICULUM = "MarlGrid-3AgentClutteredCurriculum15x15-v0"
EDITS = EE.BASE
W = H = 15
N_AGENTS, VIEW = 3, 7
WALL, GOAL, KEY, BALL = 1, 2, 3, 4
N_CLUTTER_DEFAULT, N_CLUTTER_HI = 25, 51
_KEY = dict(type="Key", color="blue", state=0)
_BALL = dict(type="Ball", color="red", state=0)


def edits_spec(max_steps=10):
    """`Edits-Cluttered15` (clutter_density 0.15: int(0.15 * 13 * 13) = 25 blocks) with the Key and the Ball in its object
    list; the edits themselves are no entry of the program: OracleEnv.set_edits holds them"""
    s = scenarios.cluttered_spec(N_AGENTS, W, VIEW, clutter_density=0.15, max_steps=max_steps)
    s["objects"] = list(s["objects"]) + [_KEY, _BALL]
    return s


def curriculum_spec(max_steps=10):
    """ClutteredMultiGrid(n_clutter=25, n_clutter_max=50): `place_obj(Wall(), max_tries=100, count=self._param("n_clutter", 0,
    51, default=25))` — in the notation of tests/param_envs.py:spec; the constructor's reset is ClutteredMultiGrid's (a random
    goal, no clutter)"""
    import draw_envs as D
    s = scenarios.cluttered_spec(N_AGENTS, W, VIEW, n_clutter=N_CLUTTER_DEFAULT, max_steps=max_steps)
    s["params"] = [("n_clutter", N_CLUTTER_DEFAULT)]
    s["gen_reset"] = [("wall_rect", 0, 0, W, H), ("put", GOAL, W - 2, H - 2), ("param", 0, "n_clutter"),
                      ("place", WALL, D.dr(0), 100)]
    return s


def spec_of(name, max_steps=10):
    return {CURRICULUM: curriculum_spec, EDITS: edits_spec}[name](max_steps)


def build(name, **kw):
    """the product env: `make(name, ...)`; the EDITS scenario with its two further kinds registered"""
    from marlgrid_amd import envs as E
    from marlgrid_amd.objects import Ball, Key
    if name == CURRICULUM:
        return E.make(name, **kw)
    with EE.registered():
        env = E.make(name, **kw)
    assert (env.edit_key(Key("blue")), env.edit_key(Ball(color="red"))) == (KEY, BALL)
    return env


# ---- which entries of a product table count ------------------------------------------------------------------------------------
def valid(entries, n_obj, width=W, height=H):
    """(..., 4) product entries (x, y, kind, on) -> bool (...): the entry is on, inside the grid and of a registered kind"""
    e = np.asarray(entries).astype(np.int64)
    return (e[..., 3] != 0) & (e[..., 0] < width) & (e[..., 1] < height) & (e[..., 2] < n_obj)


def oracle_list(entries, n_obj):
    """(K, 4) product entries -> the ordered list [(x, y, obj_id), ...] the oracle is given: those that count, in table order"""
    e = np.asarray(entries).astype(np.int64).reshape(-1, 4)
    return [(int(x), int(y), int(k)) for x, y, k, _ in e[valid(e, n_obj)]]


GARBAGE = ("off", "x outside", "y outside", "unknown kind")


def garbage_class(entries, n_obj):
    """(..., 4) -> int (...): -1 for an entry that counts, else the index into GARBAGE of the first rule it breaks"""
    e = np.asarray(entries).astype(np.int64)
    out = np.full(e.shape[:-1], -1, np.int64)
    for i, bad in reversed(list(enumerate((e[..., 3] == 0, e[..., 0] >= W, e[..., 1] >= H, e[..., 2] >= n_obj)))):
        out[bad] = i
    return out


# ---- edit lists -----------------------------------------------------------------------------------------------------------------
def random_list(rng, K, kinds=(0, WALL, GOAL, KEY, BALL), box=(1, 1, W - 1, H - 1)):
    """0 .. K entries (x, y, kind) on interior cells of `box` [x0, x1) x [y0, y1) (an edit of the border wall would let an
    agent walk off the grid: the reference's assertion under random actions)"""
    n = rng.randint(0, K + 1)
    return [(int(rng.randint(box[0], box[2])), int(rng.randint(box[1], box[3])), int(kinds[rng.randint(len(kinds))]))
            for _ in range(n)]


def mixed_table(rng, B, K, n_obj=5, box=(1, 1, W - 1, H - 1), garbage=True):
    """(B, K, 4) uint8 product entries, a random list per env, and what L1 wants of them: env b's list has, by b % 8,
    0 anything, 1 one cell twice (the later entry wins), 2 the goal moved (cleared where it is, put elsewhere), 3 a Key and a
    Ball among its entries, 4 nothing at all; the others are plain random lists.  With `garbage`,
    random slots of every env hold an entry of a garbage class — off, x outside, y outside, an unknown kind — whose other
    fields are a legal WALL entry's: it would show if it were applied."""
    t = np.zeros((B, K, 4), np.uint8)
    for b in range(B):
        lst = random_list(rng, K, box=box)
        c = b % 8
        if c == 1 and K >= 2:
            x, y = int(rng.randint(box[0], box[2])), int(rng.randint(box[1], box[3]))
            lst = ([(x, y, GOAL), (x, y, KEY)] + lst)[:K]
        elif c == 2 and K >= 2:
            lst = ([(W - 2, H - 2, 0), (int(rng.randint(box[0], box[2])), int(rng.randint(box[1], min(box[3], H - 2))), GOAL)] + lst)[:K]
        elif c == 3 and K >= 2:
            lst = (lst + [(int(rng.randint(box[0], box[2])), int(rng.randint(box[1], box[3])), KEY),
                          (int(rng.randint(box[0], box[2])), int(rng.randint(box[1], box[3])), BALL)])[-K:]
        elif c == 4:
            lst = []
        rows = [(x, y, k, 1) for x, y, k in lst]
        if garbage:
            for _ in range(rng.randint(0, 3)):
                if len(rows) >= K:
                    break
                x, y = int(rng.randint(box[0], box[2])), int(rng.randint(box[1], box[3]))
                g = [(x, y, WALL, 0), (W + rng.randint(0, 200), y, WALL, 1), (x, H + rng.randint(0, 200), WALL, 1),
                     (x, y, n_obj + rng.randint(0, 200), 1)][rng.randint(4)]
                rows.insert(rng.randint(0, len(rows) + 1), tuple(int(v) for v in g))
        if rows:
            t[b, :len(rows)] = np.asarray(rows, np.uint8)
    return t


# ---- pinned lists: what the oracle's edit op is held to the reference with (tests/test_oracle_gen_edits.py) -------------------------
# name -> (list, the reference can draw every kind in it).  Lists of (x, y, obj_id).
PINNED = {
    "cell-twice": ([(4, 9, GOAL), (4, 9, WALL), (6, 6, WALL), (6, 6, 0)], True),
    "cleared-clutter": ([(x, y, 0) for x in range(5, 9) for y in range(5, 9)], True),         # 16 cells of which clutter fills some
    "moved-goal": ([(W - 2, H - 2, 0), (3, 3, GOAL)], True),
    "ball-and-key": ([(2, 2, BALL), (7, 7, KEY), (12, 3, BALL), (1, 7, 0), (7, 7, KEY), (3, 11, WALL)], False),
    "empty": ([], True),
}
PIN_SEEDS = 5150 + np.arange(3)
PIN_STEPS, PIN_MAX_STEPS = 48, 12


def ref_env(seed, level, max_steps=PIN_MAX_STEPS, render=True):
    """ours, on top of the reference's ClutteredMultiGrid: `_gen_grid` runs the parent's and then writes `self.level`, a
    per-instance list of (x, y, obj_id), cell by cell with put_obj / grid.set — a fresh object per entry, as `_gen_grid`
    makes its own.  The constructor's reset runs before the list exists (an empty one).  render=False: gen_agent_obs stubbed
    out (the reference's Key / Ball sprites raise)"""
    import refload
    refload.load()
    from marlgrid.agents import GridAgentInterface
    from marlgrid.envs.cluttered import ClutteredMultiGrid
    from marlgrid.objects import Ball, Goal, Key, Wall
    make = {WALL: lambda: Wall(), GOAL: lambda: Goal(color="green", reward=1), KEY: lambda: Key(color="blue"),
            BALL: lambda: Ball(color="red")}

    def _gen_grid(self, width, height):
        ClutteredMultiGrid._gen_grid(self, width, height)
        for x, y, o in getattr(self, "level", ()):
            if o == 0:
                self.grid.set(x, y, None)
            else:
                self.put_obj(make[o](), x, y)
    body = dict(_gen_grid=_gen_grid)
    if not render:
        body["gen_agent_obs"] = lambda self, agent: None
    cls = type("RefLevelCluttered", (ClutteredMultiGrid,), body)
    agents = [GridAgentInterface(color=c, view_size=VIEW, view_tile_size=8) for c in scenarios.REG_COLORS[:N_AGENTS]]
    env = cls(agents=agents, grid_size=W, clutter_density=0.15, max_steps=max_steps, seed=int(seed))
    env.level = list(level)
    return env


def golden(name):
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "genedits_%s.npz" % name)) as z:
        return {k: z[k] for k in z.files}
