"""TEST INFRASTRUCTURE — scenarios whose `_gen_grid` lays the grid out from `_rand_int` draws, once for the product
(marlgrid_amd) and once on top of the reference's classes (tests/golden/make_gen_draws.py, the live-parity tests), from the
SAME `_gen_grid` text.  `register()` makes the names known to `marlgrid_amd.envs.make`, which is how tests/product_envs.py
and tests/native/hostemu.py build an env from a name.

The goldens are tests/golden/gendraws_<name>.npz: the key layout of traj_<name>.npz, plus the per-agent view encodings of
viewenc_<name>.npz under `venc_*`, plus RNG digests of every step.  They are not called traj_* / viewenc_*: the suites that
replay every file of those names take their spec from tests/scenarios.py; these are replayed through the oracle by
tests/test_oracle_gen_draws.py, from the hand-written specs below (`spec`).
"""
import os
import zlib

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEEDS = 1337 + np.arange(16)
N_AGENTS = 2
COLORS = ("red", "blue")

# name -> (kind, W, H, view_size, tile_size, max_steps, pixels pinned)
SCENARIOS = {
    "Draws-2AgentSplit6": ("split", 6, 6, 7, 8, 40, True),
    "Draws-2AgentSplit7": ("split", 7, 7, 7, 8, 40, True),
    "Draws-2AgentSplit9": ("split", 9, 9, 7, 8, 40, True),
    "Draws-2AgentSplit9-ts5": ("split", 9, 9, 7, 5, 40, True),
    "Draws-2AgentDoorKey5": ("doorkey", 5, 5, 7, 8, 100, False),
    "Draws-2AgentDoorKey6": ("doorkey", 6, 6, 7, 8, 100, False),
    "Draws-2AgentDoorKey7": ("doorkey", 7, 7, 7, 8, 100, False),
    "Draws-2AgentLongProgram12x12": ("long", 12, 12, 7, 8, 40, True),
    # a non-square grid and eight draws: registers 4 - 7, negative constants, a rectangle only place_obj's clamp makes legal
    "Draws-2AgentEight12x10": ("eight", 12, 10, 7, 8, 30, True),
}
# no reference golden (its renderer takes minutes on such a grid): pinned through the oracle, and the oracle on it through a
# short live-reference case.  160 x 150 cells do not fit LDS: the launcher takes the grid-in-place render kernel
ORACLE_ONLY = {
    "Draws-2AgentSplit160x150": ("split", 160, 150, 7, 8, 40, True),
}
IN_PLACE_KERNEL = "mg::render_kernel<0, 0, 4, 8, 3>"
EPISODES = 3            # a trajectory is EPISODES * max_steps steps: at least three episodes per seed


def gen_grid_text(kind, ns):
    """the `_gen_grid` of a test scenario over a namespace with MultiGrid / Wall / Goal (product or reference)"""
    MultiGrid, Wall, Goal = ns["MultiGrid"], ns["Wall"], ns["Goal"]

    def split(self, width, height):
        self.grid = MultiGrid((width, height))
        self.grid.wall_rect(0, 0, width, height)
        s = self._rand_int(2, width - 2)                        # the splitting column
        self.grid.vert_wall(s, 0)
        g = self._rand_int(1, height - 1)                       # the gap in it
        self.put_obj(None, s, g)
        self.place_obj(Goal(color="green", reward=1), top=(s + 1, 0), size=(width - s - 1, height))
        for _ in range(2):
            self.place_obj(Wall(), top=(0, 0), size=(s, height), max_tries=100)
        self.agent_spawn_kwargs = {}

    def long_program(self, width, height):
        self.grid = MultiGrid((width, height))
        self.grid.wall_rect(0, 0, width, height)
        for i in range(17):                                     # 34 ops: a placement and a fill, alternating
            self.place_obj(Wall(), max_tries=100)
            self.put_obj(None, 1 + i % (width - 2), 1)
        a = self._rand_int(3, width - 3)                        # recorded after op 32
        self.grid.vert_wall(a, 2, height - 4)
        g = self._rand_int(2, a + 1)                            # a draw bounded by a draw
        self.put_obj(None, a, g)
        self.grid.horz_wall(a + 1, height - 3, width - a - 2)   # extent and origin from a draw
        self.put_obj(None, width - 2, height - 3)
        self.place_obj(Goal(color="green", reward=1), top=(a + 1, 1), size=(width - a - 2, height - 2), max_tries=100)
        self.agent_spawn_kwargs = {}

    def eight(self, width, height):
        """exactly eight draws (the product's limit).  At 12 x 10: a 3..8, b 1..8, c 1..a-1, e a+1..10, f = c, g 1..8, h 0..5,
        k 2..4.  Every placement has free cells for every value of the draws (see the comments)."""
        self.grid = MultiGrid((width, height))
        self.grid.wall_rect(0, 0, width, height)
        a = self._rand_int(3, width - 3)                        # 0: the splitting column; six values: masked rejection
        self.grid.vert_wall(a, 0)
        b = self._rand_int(1, height - 1)                       # 1: the gap in it
        self.put_obj(None, a, b)
        c = self._rand_int(1, a)                                # 2: bounded above by a draw
        e = self._rand_int(a + 1, width - 1)                    # 3: bounded below by a draw
        f = self._rand_int(c, c + 1)                            # 4: a one-value range whose bounds are draws: c, no RNG word
        g = self._rand_int(1, height - 1)                       # 5
        h = self._rand_int(0, 6)                                # 6
        k = self._rand_int(2, 5)                                # 7: three values: masked rejection
        self.put_obj(Wall(), f, g)                              # registers 4 and 5 as the coordinates of a fill
        self.put_obj(Wall(), (width - 2) - k, g)                # `k - draw`, register 7
        self.put_obj(Wall(), e - 1, k)                          # `draw - k`: a negative constant next to the draw
        self.put_obj(None, h + 1, height - 2)                   # register 6
        # the goal right of f, in the rows above 1 + g: row 1 has at least four cells there and at most three of them are
        # walls (the column a, the two puts above when g is 1)
        self.place_obj(Goal(color="green", reward=1), top=(f, 1), size=(width - 1 - f, g))
        # [h - 3, h + 1) x [0, height + 5): hangs over the left edge for h < 3 and over the bottom always.  Upstream clamps the
        # top to 0 and THEN adds the size: [0, 4) for h < 3
        self.place_obj(Wall(), top=(h - 3, 0), size=(4, height + 5), max_tries=100)
        self.place_obj(Wall(), top=(1, k), size=(c, height - 1 - k), max_tries=100)      # rows k .. height - 2 of columns 1 .. c
        self.agent_spawn_kwargs = {}

    return dict(split=split, long=long_program, eight=eight)[kind]


# ---- the scenarios restated BY HAND for the oracle (oracle/oracle.py:make_config) -------------------------------------------
# Written from the `_gen_grid` texts above and upstream's envs/doorkey.py, NOT derived from the product's recorder:
# tests/test_oracle_gen_draws.py asserts that the product's scenario_spec() decodes to exactly these.
#   ("draw", r, lo, hi)                                      draw[r] = self._rand_int(lo, hi)
#   ("fill", obj, x0, y0, x1, y1)                            grid.set(x, y, obj) over [x0, x1) x [y0, y1); obj 0: None
#   ("place_sym", obj, count, max_tries, x0, y0, x1, y1)     place_obj(obj, top=(x0, y0), size=(x1 - x0, y1 - y0)), count times
# a coordinate is an int or ("d", reg, sign, const): const + sign * draw[reg]
def dr(reg, const=0, sign=1):
    return ("d", reg, sign, const)


_WALL = dict(type="Wall", color="worst", state=0)                       # objects.py:47, 280
_GOAL = dict(type="Goal", color="green", state=0, reward=1)
_DOOR = [dict(type="Door", color="yellow", state=st) for st in (3, 1, 2)]      # the locked door, then its other two states
_KEY = dict(type="Key", color="yellow", state=0)
DEFAULT_TRIES = 100000                                                  # place_obj's max_tries=1e5 (base.py:690-691)


def spec(kind, W, H, view=7, tile=8, max_steps=40):
    s = dict(W=W, H=H, agents=[dict(color=c) for c in COLORS], view_size=view, tile_size=tile, view_offset=0,
             see_through_walls=False, max_steps=max_steps, reward_decay=True, ghost_mode=True, respawn=False, wall_obj=1)
    room = ("wall_rect", 0, 0, W, H)
    col = lambda r: (dr(r), 0, dr(r, 1), H)                             # vert_wall(draw[r], 0): the whole column
    cell = lambda x, y: (x, y) + tuple(("d", v[1], v[2], v[3] + 1) if isinstance(v, tuple) else v + 1 for v in (x, y))
    if kind == "split":
        s["objects"] = [None, _WALL, _GOAL]
        prog = [room, ("draw", 0, 2, W - 2), ("fill", 1) + col(0), ("draw", 1, 1, H - 1), ("fill", 0) + cell(dr(0), dr(1)),
                ("place_sym", 2, 1, DEFAULT_TRIES, dr(0, 1), 0, W, H),              # top (s + 1, 0), size (W - s - 1, H)
                ("place_sym", 1, 2, 100, 0, 0, dr(0), H)]                           # twice: top (0, 0), size (s, H)
    elif kind == "doorkey":                                                         # envs/doorkey.py:15-41
        s["objects"] = [None, _WALL, _GOAL] + _DOOR + [_KEY]
        prog = [room, ("put", 2, W - 2, H - 2), ("draw", 0, 2, W - 2), ("fill", 1) + col(0),
                ("draw", 1, 1, W - 2),                                              # (the door ROW from the width: doorkey.py:34)
                ("fill", 3) + cell(dr(0), dr(1)), ("place_sym", 6, 1, DEFAULT_TRIES, 0, 0, dr(0), H)]
    elif kind == "long":
        s["objects"] = [None, _WALL, _GOAL]
        prog = [room]
        for i in range(17):
            prog += [("place", 1, 1, 100), ("put", 0, 1 + i % (W - 2), 1)]
        prog += [("draw", 0, 3, W - 3), ("fill", 1, dr(0), 2, dr(0, 1), 2 + (H - 4)),          # vert_wall(a, 2, H - 4)
                 ("draw", 1, 2, dr(0, 1)), ("fill", 0) + cell(dr(0), dr(1)),
                 ("fill", 1, dr(0, 1), H - 3, W - 1, H - 2),            # horz_wall(a + 1, H - 3, W - a - 2): ends at W - 1
                 ("put", 0, W - 2, H - 3),
                 ("place_sym", 2, 1, 100, dr(0, 1), 1, W - 1, H - 1)]   # top (a + 1, 1), size (W - a - 2, H - 2)
    elif kind == "eight":
        s["objects"] = [None, _WALL, _GOAL]
        a, b, c, e, f, g, h, k = range(8)
        prog = [room, ("draw", a, 3, W - 3), ("fill", 1) + col(a), ("draw", b, 1, H - 1), ("fill", 0) + cell(dr(a), dr(b)),
                ("draw", c, 1, dr(a)), ("draw", e, dr(a, 1), W - 1), ("draw", f, dr(c), dr(c, 1)), ("draw", g, 1, H - 1),
                ("draw", h, 0, 6), ("draw", k, 2, 5),
                ("fill", 1) + cell(dr(f), dr(g)), ("fill", 1) + cell(dr(k, W - 2, -1), dr(g)), ("fill", 1) + cell(dr(e, -1), dr(k)),
                ("fill", 0) + cell(dr(h, 1), H - 2),
                ("place_sym", 2, 1, DEFAULT_TRIES, dr(f), 1, W - 1, dr(g, 1)),      # top (f, 1), size (W - 1 - f, g)
                # top (h - 3, 0), size (4, H + 5): x0 + 4 = h + 1; the constant bottom H + 5 is written as upstream's clamp
                # leaves it, min(0 + H + 5, H) — a constant is clamped where it is written, a draw where it is drawn
                ("place_sym", 1, 1, 100, dr(h, -3), 0, dr(h, 1), min(H + 5, H)),
                ("place_sym", 1, 1, 100, 1, dr(k), dr(c, 1), H - 1)]                # top (1, k), size (c, H - 1 - k)
    s["gen_ctor"], s["gen_reset"] = prog, list(prog)
    return s


def spec_of(name, **kw):
    kind, W, H, view, tile, max_steps, _pix = dict(SCENARIOS, **ORACLE_ONLY)[name]
    return spec(kind, W, H, view, tile, kw.get("max_steps", max_steps))


def decode_operand(v):
    """an operand of the product's encoded program (marlgrid_hip.h MG_GEN_SYM) -> int or ("d", reg, sign, const); restated
    from the header's description, not through marlgrid_amd: bit 30 symbolic, bit 29 `const - draw`, bits 16..18 the register,
    the low 16 bits the constant, two's complement"""
    v = int(v)
    if not v & 0x40000000:
        return v
    const = v & 0xFFFF
    return ("d", (v >> 16) & 7, -1 if v & 0x20000000 else 1, const - 0x10000 if const & 0x8000 else const)


def decode_spec(s):
    """the product's scenario_spec() with the operands of its draw / fill / place_sym entries decoded"""
    def entry(g):
        if g[0] == "draw":
            return g[:2] + tuple(decode_operand(v) for v in g[2:])
        if g[0] == "fill":
            return g[:2] + tuple(decode_operand(v) for v in g[2:])
        if g[0] == "place_sym":
            return g[:4] + tuple(decode_operand(v) for v in g[4:])
        return g
    return dict(s, gen_ctor=[entry(g) for g in s["gen_ctor"]], gen_reset=[entry(g) for g in s["gen_reset"]])


# ---- product side -----------------------------------------------------------------------------------------------------
def product_class(kind):
    from marlgrid_amd import envs as E
    from marlgrid_amd.base import MultiGrid, MultiGridEnv
    from marlgrid_amd.objects import Goal, Wall
    if kind == "doorkey":
        return E.DoorKeyEnv
    return type("Draws%sEnv" % kind.capitalize(), (MultiGridEnv,),
                dict(_gen_grid=gen_grid_text(kind, dict(MultiGrid=MultiGrid, Wall=Wall, Goal=Goal)), mission="", metadata={}))


def _factory(kind, W, H, view, tile, max_steps, **kw):
    from marlgrid_amd.agents import GridAgentInterface
    agents = [GridAgentInterface(color=c, view_size=view, view_tile_size=tile) for c in COLORS]
    return product_class(kind)(agents=agents, **dict(dict(width=W, height=H, max_steps=max_steps), **kw))


def register():
    import functools
    from marlgrid_amd import envs as E
    for name, (kind, W, H, view, tile, max_steps, _pix) in dict(SCENARIOS, **ORACLE_ONLY).items():
        # (max_steps by keyword: a caller's max_steps= replaces the scenario's)
        E._registry.setdefault(name, functools.partial(_factory, kind, W, H, view, tile, max_steps=max_steps))


def build(name, **kw):
    from marlgrid_amd import envs as E
    register()
    return E.make(name, **kw)


def build_sized(kind, W, H, **kw):
    """a Split / DoorKey of any size (the live-parity cases)"""
    return _factory(kind, W, H, 7, 8, kw.pop("max_steps", 40), **kw)


# ---- reference side (build container only) ------------------------------------------------------------------------------
def ref_env(kind, W, H, view, tile, max_steps, seed, render=True):
    """the scenario on top of the reference's classes, `_rand_int` as gym-minigrid defines it; render=False: gen_agent_obs
    stubbed out (state and RNG only: step() and reset() call it directly)"""
    import refload
    refload.load()
    from marlgrid.agents import GridAgentInterface
    from marlgrid.base import MultiGrid, MultiGridEnv
    from marlgrid.objects import Goal, Wall

    def _rand_int(self, low, high):
        return self.np_random.randint(low, high)
    if kind == "doorkey":
        from marlgrid.envs.doorkey import DoorKeyEnv
        # (the reference's renderer raises NameError on Key / Door sprites, and step() calls gen_agent_obs directly)
        cls = type("RefDoorKey", (DoorKeyEnv,), dict(_rand_int=_rand_int, gen_agent_obs=lambda self, agent: None))
    else:
        cls = type("RefDraws" + kind, (MultiGridEnv,),
                   dict(dict(_gen_grid=gen_grid_text(kind, dict(MultiGrid=MultiGrid, Wall=Wall, Goal=Goal)), _rand_int=_rand_int,
                             mission="", metadata={}), **({} if render else dict(gen_agent_obs=lambda self, agent: None))))
    agents = [GridAgentInterface(color=c, view_size=view, view_tile_size=tile) for c in COLORS]
    return cls(agents=agents, width=W, height=H, max_steps=max_steps, seed=int(seed))


# ---- comparison helpers ---------------------------------------------------------------------------------------------------
def rng_digest(state):
    """32-bit digest of an MT19937 stream position in numpy's form (key[624], pos): what marlgrid_amd.seeding.same_stream
    compares — the position, words 1..623 and the top bit of word 0"""
    key, pos = state
    key = np.ascontiguousarray(key, np.uint32)
    return zlib.crc32(key[1:].tobytes() + bytes([int(key[0]) >> 31]) + np.int32(pos).tobytes()) & 0xFFFFFFFF


def golden(name):
    """the fixture's arrays, and `rng_next` [S][T] — the RNG after the caller-side reset that follows step t, rng_step where there
    was none — laid out again from `rng_after_reset` (one entry per True of reset_after: make_gen_draws.py)"""
    with np.load(os.path.join(GOLD, "gendraws_%s.npz" % name)) as z:
        g = {k: z[k] for k in z.files}
    g["rng_next"] = g["rng_step"].copy()
    g["rng_next"][g["reset_after"]] = g.pop("rng_after_reset")
    return g


CANON_KEYS = ("base_enc", "pos", "dir", "active", "done", "carry_enc", "ordinal")


def cmp_canon(got, g, prefix, si, t, what):
    for k in CANON_KEYS:
        want = g[prefix + k][si] if t is None else g[prefix + k][si, t]
        assert np.array_equal(np.asarray(got[k]), np.asarray(want)), "%s: %s\ngot=%r\ngolden=%r" % (what, k, got[k], want)


def canonical_batch(spec, grid, rec):
    """tests/product_envs.py:canonical_arrays for the whole batch at once: dict of arrays with a leading B, from the object
    ids (B, W, H) and the packed agent records (B, n)"""
    import _native_consts as K
    import canon
    enc = canon.obj_enc_table(spec)
    rec = np.asarray(rec).astype(np.uint64)
    by = lambda i: ((rec >> np.uint64(8 * i)) & np.uint64(0xFF)).astype(np.int64)
    x, y, d, fl, ca, rk = by(K.AG_X), by(K.AG_Y), by(K.AG_DIR), by(K.AG_FLAGS), by(K.AG_CARRY), by(K.AG_RANK)
    placed = (fl & K.AF_PLACED) != 0
    there = placed | ((fl & K.AF_EVICTED) != 0)
    same = placed[:, :, None] & placed[:, None, :] & (x[:, :, None] == x[:, None, :]) & (y[:, :, None] == y[:, None, :])
    below = (same & (rk[:, None, :] < rk[:, :, None])).sum(axis=2)
    return dict(base_enc=enc[np.asarray(grid)], pos=np.stack([np.where(there, x, -1), np.where(there, y, -1)], axis=2).astype(np.int16),
                dir=d.astype(np.int8), active=(fl & K.AF_ACTIVE) != 0, done=(fl & K.AF_DONE) != 0, carry_enc=enc[ca],
                ordinal=np.where(placed, below, -1).astype(np.int8))


def cmp_canon_batch(got, g, prefix, rows, ts, mask, what):
    """canonical_batch's arrays against the golden's rows `rows` (at steps `ts`, or None: ctor_ / reset_), envs in `mask`"""
    if not mask.any():
        return
    for k in CANON_KEYS:
        want = g[prefix + k][rows] if ts is None else g[prefix + k][rows, ts]
        bad = np.nonzero(mask & (np.asarray(got[k]) != want).reshape(len(rows), -1).any(axis=1))[0]
        assert bad.size == 0, "%s: %s differs in envs %s\ngot=%r\ngolden=%r" % (what, k, bad[:8].tolist(), got[k][bad[0]], want[bad[0]])


def split_structure(grid, wall_id, goal_id):
    """Split's invariant on a (B, W, H) array of object ids: exactly one interior column that is wall but for one gap, the
    goal right of it.  Returns (split column, gap row) per env; asserts."""
    B, W, H = grid.shape
    col_walls = (grid[:, :, 1:H - 1] == wall_id).sum(axis=2)                # interior rows
    is_split = col_walls[:, 2:W - 2] == H - 3                               # legal columns 2 .. W-3
    assert (is_split.sum(axis=1) == 1).all(), "not exactly one split column"
    s = 2 + is_split.argmax(axis=1)
    # (a clutter wall left of the column can fill a second column only if H - 3 <= 2: not at the sizes tested)
    col = grid[np.arange(B), s]
    gap = (col[:, 1:H - 1] != wall_id)
    assert (gap.sum(axis=1) == 1).all()
    gx = (grid == goal_id).reshape(B, -1).argmax(axis=1) // H
    assert ((grid == goal_id).reshape(B, -1).sum(axis=1) == 1).all() and (gx > s).all(), "goal not right of the split"
    return s, 1 + gap.argmax(axis=1)
