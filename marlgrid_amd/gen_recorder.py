"""The `_gen_grid` recorder: what turns a scenario's layout code into a reset program.  Host only — numpy and the constants
of the C ABI; no torch, no library call.

`MultiGridEnv` runs `_gen_grid` under a `GenRecorder`.  Static edits (walls, put_obj / grid.set) made before the first random
placement go into a TEMPLATE grid; everything after it — placements, `_rand_int` draws, `_param` loads, later static edits —
into an ordered list of `RecordedOp`s that every env replays on the device at its reset, with its own RNG.  A value of
`_rand_int` / `_param` is a `GenDraw`, `const +- draw[register]`: layout code computes with it and hands it back as a
coordinate, extent, count or bound; `_fork` makes it a Python int by recording one run of `_gen_grid` per value and merging
the runs into one program whose branches carry guards.  What the recorder cannot prove legal for every possible draw is
refused when it is recorded.

    GenRecorder.record()        -> Recording(template, ops, sym, late)
    pack_program(ops, ...)      -> the MgGenOp array and the stacked reject tables (the device's and the host emulation's)
    decode_program(recording)   -> the symbolic entries of `scenario_spec()`'s gen_ctor / gen_reset
"""
import collections
import itertools
import threading

import numpy as np

from . import _native as N
from .agents import GridAgentInterface

_trace = threading.local()      # .env: the env whose `_gen_grid` runs on this thread (how MultiGrid(...) finds its env)

_NO_BRANCH = ("a value of self._rand_int(...) inside _gen_grid is drawn later, per env, on the device: _gen_grid may compute "
              "with it (draw + k, k + draw, draw - k, k - draw with Python ints) and hand the result to put_obj / grid.set / the "
              "wall helpers / place_obj(top=, size=) / a later _rand_int, but it cannot branch on it (%s) — self._fork(draw) hands "
              "its value over as a Python int, one recorded path per value; self._rand_elem(...) / self._rand_bool() draw and fork")


class GenDraw(object):
    """What `self._rand_int(lo, hi)` returns while `_gen_grid` is recorded: `const + sign * draw[reg]`, sign +-1 — a
    coordinate or extent whose value every env draws for itself at every reset (MgGenOp, MG_GEN_SYM)."""
    __slots__ = ("reg", "sign", "const")
    __hash__ = None

    def __init__(self, reg, sign=1, const=0):
        self.reg, self.sign, self.const = reg, sign, const

    @staticmethod
    def _int(k, what):
        if isinstance(k, (bool, GenDraw)) or not isinstance(k, (int, np.integer)):
            raise NotImplementedError(_NO_BRANCH % what)
        return int(k)

    def __add__(self, k):
        return GenDraw(self.reg, self.sign, self.const + self._int(k, "draw + %s" % type(k).__name__))
    __radd__ = __add__

    def __sub__(self, k):
        return GenDraw(self.reg, self.sign, self.const - self._int(k, "draw - %s" % type(k).__name__))

    def __rsub__(self, k):
        return GenDraw(self.reg, -self.sign, self._int(k, "%s - draw" % type(k).__name__) - self.const)

    def _refuse(name):
        def f(self, *a, **k):
            raise NotImplementedError(_NO_BRANCH % name)
        return f
    for _n in ("eq", "ne", "lt", "le", "gt", "ge", "bool", "int", "index", "float", "mul", "rmul", "floordiv", "rfloordiv",
               "truediv", "rtruediv", "mod", "rmod", "neg", "pos", "abs", "pow", "rpow", "lshift", "rshift", "and", "or",
               "xor", "invert", "round", "trunc"):
        locals()["__%s__" % _n] = _refuse(_n)
    del _n, _refuse

    def __repr__(self):
        return "<%d %s draw[%d]>" % (self.const, "+" if self.sign > 0 else "-", self.reg)

    def encode(self):
        if not -32768 <= self.const <= 32767:
            raise NotImplementedError("_gen_grid: a constant of %d next to a draw does not fit the program's operand" % self.const)
        return N.GEN_SYM | (N.GEN_NEG if self.sign < 0 else 0) | (self.reg << N.GEN_DRAW_SHIFT) | (self.const & 0xFFFF)


def _gen_add(a, b):
    """a + b inside the recorder (top + size, x + length): the two may hold the SAME draw with opposite signs"""
    if isinstance(a, GenDraw) and isinstance(b, GenDraw):
        if a.reg == b.reg and a.sign + b.sign == 0:
            return a.const + b.const
        raise NotImplementedError(_NO_BRANCH % "a sum of two draws")
    return a + b


def _gen_enc(v):
    return v.encode() if isinstance(v, GenDraw) else int(v)


def _any_draw(*vs):
    return any(isinstance(v, GenDraw) for v in vs)


def _same_spawn(a, b):
    """two `agent_spawn_kwargs` left by two runs of one `_gen_grid` (callables by identity)"""
    a, b = a or {}, b or {}
    if set(a) != set(b):
        return False
    return all(a[k] is b[k] if callable(a[k]) else (tuple(a[k]) == tuple(b[k]) if isinstance(a[k], (tuple, list)) else a[k] == b[k])
               for k in a)


def _guard_bits(r, lo, hi):
    return N.GEN_GUARD | (r << N.GEN_GUARD_DRAW_SHIFT) | (hi << N.GEN_GUARD_HI_SHIFT) | (lo << N.GEN_GUARD_LO_SHIFT)


class RecordedOp(collections.namedtuple("RecordedOp", "obj count max_tries x0 y0 x1 y1 reject")):
    """One op of a reset program: MgGenOp's fields (marlgrid_hip.h), with the bytes of a placement's (W, H) reject table —
    or None — where the struct has the table's row.  A plain tuple to whoever compares or hashes it.

    `max_tries` carries the kind:   > 0  `count` placements of object `kind` by rejection sampling in [x0, x1) x [y0, y1)
                                      0  a fill: `kind` into every cell of the rectangle (a static edit after a placement)
                                     -1  a draw: draw[register] = randint(x0, x1)
                              GEN_PARAM  a parameter load: draw[register] = clamp(params[env][y0], x0, x1 - 1)
                              GEN_EDITS  the env's own list of `count` cell edits (x, y, kind, on), applied in order
    `obj`: the object kind or the draw register in the low byte; above it the guard of a branch (`_guard_bits`), 0 for none —
    the op runs only in the envs where lo <= draw[r] <= hi.  `count` and the rectangle may be encoded `GenDraw`s (GEN_SYM)."""
    __slots__ = ()

    @classmethod
    def draw(cls, reg, guard, low, high):
        return cls(reg | guard, 1, -1, _gen_enc(low), 0, _gen_enc(high), 0, None)

    @classmethod
    def param(cls, reg, guard, col, low, high):
        return cls(reg | guard, 1, N.GEN_PARAM, low, col, high, 0, None)

    @classmethod
    def fill(cls, key, guard, rect):
        return cls(int(key) | guard, 1, 0, *rect, None)

    @classmethod
    def edits(cls, K):
        return cls(0, int(K), N.GEN_EDITS, 0, 0, 0, 0, None)

    is_draw = property(lambda self: self.max_tries == -1)
    is_param = property(lambda self: self.max_tries == N.GEN_PARAM)
    is_edits = property(lambda self: self.max_tries == N.GEN_EDITS)
    sets_register = property(lambda self: self.max_tries in (-1, N.GEN_PARAM))      # a draw or a PARAM
    is_fill = property(lambda self: self.max_tries == 0)
    is_placement = property(lambda self: self.max_tries > 0)
    kind = register = property(lambda self: self.obj & 0xFF)            # placements and fills / draws and PARAMs
    guard_bits = property(lambda self: self.obj & ~0xFF)
    rect = property(lambda self: (self.x0, self.y0, self.x1, self.y1))
    has_sym_operand = property(lambda self: any(v & N.GEN_SYM for v in self.rect))
    has_sym_count = property(lambda self: bool(self.count & N.GEN_SYM))

    @property
    def guard(self):
        """(r, lo, hi) of the branch the op belongs to, or None"""
        g = self.guard_bits
        if not g & N.GEN_GUARD:
            return None
        return (g >> N.GEN_GUARD_DRAW_SHIFT) & 7, (g >> N.GEN_GUARD_LO_SHIFT) & 0xFF, (g >> N.GEN_GUARD_HI_SHIFT) & 0xFF


# what a recording leaves: the (W, H) uint8 template, the ops, the symbolic form of the template's edits, and — op index ->
# entries — that of the ops that are no placements (static edits recorded as fills, draws, PARAMs)
Recording = collections.namedtuple("Recording", "template ops sym late")


class GenRecorder(object):
    """All state and logic of recording one env's `_gen_grid`.  From the env it takes `width`, `height`, `obj_reg`,
    `agent_spawn_kwargs`, the `_gen_grid` callable, `_place_region`, `_reject_table` and `_param_column` (the env's ParamTable,
    gen_params.py, owns the device table), and it leaves `env.grid`.  The env's `_rand_int` / `_param` / `_fork` / `place_obj`
    delegate here while `active`; `MultiGrid` reports its static edits here."""

    width = property(lambda self: self.env.width)
    height = property(lambda self: self.env.height)

    def __init__(self, env):
        self.env = env
        self.active = False         # `_gen_grid` is running
        self.grid = None
        self.path = []
        self.written = set()

    def begin(self, grid):
        """a run of `_gen_grid` has made its MultiGrid: fresh per-run state"""
        if not self.active:
            raise RuntimeError("MultiGrid(...) is constructed inside _gen_grid")
        self.grid = grid
        self.sym = []
        self.ops = []
        self.late = {}              # index into ops -> the symbolic form of a static edit recorded as op(s)
        self.draws = []             # per `_rand_int` so far: the (lowest, highest) value it can take, over all earlier draws
        self.guard = 0              # the guard bits (MG_GEN_GUARD) of the branch being recorded: ORed into every op's `obj`
        self.fork_i = 0             # forks met so far in this run of `_gen_grid` (an index into path)
        self.params = {}            # `_param` names of this run: name -> (register, low, high)

    @property
    def in_program(self):
        """something is in the ordered program already: a static edit no longer goes into the template"""
        return bool(self.ops)

    def _emit(self, op, *late):
        self.ops.append(op)
        if late:
            self.late[len(self.ops) - 1] = list(late)

    def _need_grid(self, what):
        if not self.active or self.grid is None:
            raise NotImplementedError(_NO_BRANCH % what)

    def static(self, sym, key, rects):
        """A static layout edit of `_gen_grid` (grid.set / put_obj / the wall helpers).  Before the first random
        place_obj it goes into the template (returns True: the caller writes the template); AFTER one — upstream's
        `_gen_grid` is free Python, envs/cluttered.py:25-36 could as well put its goal last — it is recorded in the
        ordered program as fill ops (max_tries 0: write `key` into every cell of a rectangle, replacing what a
        placement put there, base.py:655-662) and replayed per env between the placements (returns False)."""
        if not self.in_program:
            self.sym.extend(sym if isinstance(sym, list) else [sym])
            return True
        first = None                # the op this edit's first rectangle went into: where its symbolic form is listed
        for (x0, y0, x1, y1) in rects:
            # a fill that continues the one before it (same object, same rows or columns, adjacent) is the same op, larger
            last = self.ops[-1]
            merged = None
            if last.is_fill and last.obj == int(key) | self.guard and last.reject is None and not last.has_sym_operand:
                lx0, ly0, lx1, ly1 = last.rect
                if (ly0, ly1) == (y0, y1) and (lx1 == x0 or x1 == lx0):
                    merged = RecordedOp.fill(last.obj, 0, (min(lx0, x0), y0, max(lx1, x1), y1))
                elif (lx0, lx1) == (x0, x1) and (ly1 == y0 or y1 == ly0):
                    merged = RecordedOp.fill(last.obj, 0, (x0, min(ly0, y0), x1, max(ly1, y1)))
            if merged is not None:
                self.ops[-1] = merged
            else:
                self.ops.append(RecordedOp.fill(key, self.guard, (x0, y0, x1, y1)))
            if first is None:
                first = len(self.ops) - 1
        if first is not None:
            self.late.setdefault(first, []).extend(sym if isinstance(sym, list) else [sym])
        return False

    def cases(self, *operands):
        """every value the operands (ints or GenDraw) can take together, over the static intervals of the draws in them"""
        regs = sorted({v.reg for v in operands if isinstance(v, GenDraw)})
        spans = [range(self.draws[r][0], self.draws[r][1] + 1) for r in regs]
        for vals in itertools.product(*spans):
            d = dict(zip(regs, vals))
            yield tuple(v.const + v.sign * d[v.reg] if isinstance(v, GenDraw) else int(v) for v in operands)

    def rand_int(self, low, high):
        self._need_grid("_rand_int outside _gen_grid, or before self.grid = MultiGrid(...)")
        for v in (low, high):
            if not isinstance(v, GenDraw):
                GenDraw._int(v, "_rand_int(%s)" % type(v).__name__)
        if len(self.draws) >= N.GEN_DRAWS:
            raise NotImplementedError("_gen_grid makes more than %d _rand_int draws: a reset program holds at most %d (MG_GEN_DRAWS: "
                                      "the draws of a reset live in one 64-bit register)" % (N.GEN_DRAWS, N.GEN_DRAWS))
        cases = list(self.cases(low, high))
        if any(hi <= lo for lo, hi in cases):
            raise ValueError("_rand_int(%r, %r): not high > low for every value the earlier draws can take" % (low, high))
        vmin, vmax = min(lo for lo, _ in cases), max(hi for _, hi in cases) - 1
        if vmin < 0 or vmax > 255:
            raise ValueError("_rand_int(%r, %r) inside _gen_grid: values %d..%d do not fit a grid coordinate (0..255)"
                             % (low, high, vmin, vmax))
        reg = len(self.draws)
        self.draws.append((vmin, vmax))
        self._emit(RecordedOp.draw(reg, self.guard, low, high), ("draw", reg, _gen_enc(low), _gen_enc(high)))
        return GenDraw(reg)

    def param(self, name, low, high, default):
        self._need_grid("_param outside _gen_grid, or before self.grid = MultiGrid(...)")
        low, high = GenDraw._int(low, "_param(low=%s)" % type(low).__name__), GenDraw._int(high, "_param(high=%s)" % type(high).__name__)
        if not 0 <= low < high <= 256:
            raise ValueError("_param(%r, %d, %d): the interval [low, high) must be non-empty and within 0..255" % (name, low, high))
        default = low if default is None else GenDraw._int(default, "_param(default=%s)" % type(default).__name__)
        if not low <= default < high:
            raise ValueError("_param(%r, %d, %d, default=%d): the default lies outside the interval" % (name, low, high, default))
        seen = self.params.get(name)
        if seen is not None:
            if seen[1:] != (low, high):
                raise ValueError("_param(%r, %d, %d): declared as [%d, %d) earlier in this _gen_grid" % ((name, low, high) + seen[1:]))
            return GenDraw(seen[0])
        if len(self.draws) >= N.GEN_DRAWS:
            raise NotImplementedError("_gen_grid needs more than %d draw registers (MG_GEN_DRAWS): parameters share them with the "
                                      "_rand_int draws and the copies that forks inside a branch take" % N.GEN_DRAWS)
        col = self.env._param_column(name, low, high, default)
        reg = len(self.draws)
        self.draws.append((low, high - 1))
        self.params[name] = (reg, low, high)
        self._emit(RecordedOp.param(reg, self.guard, col, low, high), ("param", reg, col, low, high))
        return GenDraw(reg)

    def fork(self, d):
        self._need_grid("_fork outside _gen_grid")
        r = d.reg
        lo, hi = self.draws[r]
        if lo == hi:                # decided on this path already (a one-value range, or forked before): nothing to guard
            return d.const + d.sign * lo
        if hi - lo + 1 > 16:
            raise NotImplementedError("_gen_grid: a fork over more than 16 values (draw[%d] takes %d..%d here): every value is a "
                                      "recorded path of its own" % (r, lo, hi))
        i = self.fork_i
        self.fork_i += 1
        if i == len(self.path):                 # met for the first time: take its first value; the later ones are later runs
            q = None
            if self.guard:
                q = len(self.draws)             # a branch inside a branch: the conjunction through a spare register
                if q >= N.GEN_DRAWS:
                    raise NotImplementedError("_gen_grid needs more than %d draw registers (MG_GEN_DRAWS) on one path: %d "
                                              "_rand_int draws and the copies that forks inside a branch of another draw take"
                                              % (N.GEN_DRAWS, N.GEN_DRAWS))
                if hi + 1 > 255:
                    raise NotImplementedError("_gen_grid: a fork inside a branch of another draw, on a draw that may be 255: its "
                                              "copy `draw + 1` must fit a byte of the draw registers")
            self.path.append(dict(values=list(range(lo, hi + 1)), idx=0, q=q, zero=q in self.written))
        f = self.path[i]
        if f["values"] != list(range(lo, hi + 1)):
            raise ValueError("_gen_grid is not a function of its arguments and its draws: run again for another path it forked "
                             "over other values")
        v = f["values"][f["idx"]]
        self.draws[r] = (v, v)                  # inside the branch the draw's interval is the guard's: every later proof is per path
        if f["q"] is None:
            self.guard = _guard_bits(r, v, v)
        else:
            # under the outer guard: q = draw[r] + 1, a one-value DRAW (no RNG word).  Registers start every reset at 0 — a
            # number that a branch recorded earlier may have written is zeroed first, in every env —, so q == v + 1 says
            # "the outer branch was taken and draw[r] == v"
            q = f["q"]
            src = GenDraw(r)
            if f["zero"]:
                self._emit(RecordedOp.draw(q, 0, 0, 1), ("draw", q, 0, 1))
            self._emit(RecordedOp.draw(q, self.guard, src + 1, src + 2), ("draw", q, (src + 1).encode(), (src + 2).encode()))
            self.draws.append((v + 1, v + 1))
            self.guard = _guard_bits(q, v + 1, v + 1)
        f["start"] = len(self.ops)              # the branch's own ops begin here
        return d.const + d.sign * v

    def fill_sym(self, key, rects):
        """A static edit with a draw among its coordinates: one fill op per rectangle, its operands evaluated per env on the
        device; never merged with its neighbours.  Proved here for every possible draw: non-empty and inside the grid."""
        g = self.grid
        for rect in rects:
            cases = list(self.cases(*rect))
            if any(not (0 <= x0 < x1 <= self.width and 0 <= y0 < y1 <= self.height) for x0, y0, x1, y1 in cases):
                raise ValueError("_gen_grid: the edit of cells [%r, %r) x [%r, %r) is not inside the %d x %d grid and non-empty for "
                                 "every value the draws can take" % (rect[0], rect[2], rect[1], rect[3], self.width, self.height))
            enc = tuple(_gen_enc(v) for v in rect)
            self._emit(RecordedOp.fill(key, self.guard, enc), ("fill", int(key)) + enc)
            # every cell the edit can reach may have been written: get() there warns
            g._maybe[min(c[0] for c in cases):max(c[2] for c in cases), min(c[1] for c in cases):max(c[3] for c in cases)] = True

    def _place_region_sym(self, top, size):
        """place_obj's sampling rectangle with a draw in `top` / `size`: constants clamped here, the rest on the device
        (base.py:692-695); returns the operands and the hull of the rectangles the draws can produce"""
        top = (0, 0) if top is None else tuple(top)
        size = (self.width, self.height) if size is None else tuple(size)
        for v in tuple(top) + tuple(size):
            if not isinstance(v, GenDraw):
                GenDraw._int(v, "place_obj(top=, size=) of %s" % type(v).__name__)
        # upstream clamps `top` first and adds `size` to the CLAMPED top (base.py:692, 695): a rectangle that starts outside the
        # grid keeps its extent.  A constant top is clamped here; a drawn one on the device, which moves the far edge with it
        x0, y0 = (v if isinstance(v, GenDraw) else max(int(v), 0) for v in top)
        x1, y1 = _gen_add(x0, size[0]), _gen_add(y0, size[1])
        x1, y1 = (v if isinstance(v, GenDraw) else min(int(v), lim) for v, lim in ((x1, self.width), (y1, self.height)))
        clamped = [(max(a, 0), max(b, 0), min(max(a, 0) + (c - a), self.width), min(max(b, 0) + (d - b), self.height))
                   for a, b, c, d in self.cases(x0, y0, x1, y1)]
        if any(c <= a or d <= b for a, b, c, d in clamped):
            raise ValueError("place_obj: the sampling rectangle [%r, %r) x [%r, %r) is empty for some value the draws can take"
                             % (x0, x1, y0, y1))
        hull = (min(c[0] for c in clamped), min(c[1] for c in clamped), max(c[2] for c in clamped), max(c[3] for c in clamped))
        return (x0, y0, x1, y1), hull

    def place_obj(self, obj, top, size, reject_fn, max_tries, count):
        if isinstance(count, GenDraw):
            if any(c < 0 for c, in self.cases(count)):
                raise ValueError("place_obj(count=%r): below 0 for some value the draws can take" % (count,))
            n_rec = count.encode()
        else:
            n_rec = GenDraw._int(count, "place_obj(count=%s)" % type(count).__name__)
            if n_rec < 0:
                raise ValueError("place_obj(count=%d): a count is not negative" % n_rec)
            if n_rec == 0:
                return None
        if isinstance(obj, GridAgentInterface):
            raise NotImplementedError("inside _gen_grid agents are placed by reset() itself")
        max_tries = int(max(1, min(max_tries, 1e5)))
        key = self.env.obj_reg.get_key(obj)
        if _any_draw(*[v for r in (top, size) if r is not None for v in r]):
            operands, region = self._place_region_sym(top, size)    # (region: the hull — every cell some draw can sample)
            operands = tuple(_gen_enc(v) for v in operands)
        else:
            operands = region = self.env._place_region(top, size)
        rej = self.env._reject_table(reject_fn, region)
        op = RecordedOp(key | self.guard, n_rec, max_tries, *operands, None if rej is None else rej.tobytes())
        x0, y0, x1, y1 = region
        may = self.grid._shadow[x0:x1, y0:y1] == 0              # (only empty cells accept a placement, base.py:672-679)
        if rej is not None:
            may &= rej[x0:x1, y0:y1] == 0
        self.grid._maybe[x0:x1, y0:y1] |= may
        last = self.ops[-1] if self.ops else None
        # the same placement again is the op before it with a larger count (a symbolic count is an op of its own)
        if (last is not None and last.is_placement and last._replace(count=n_rec) == op
                and not (last.has_sym_count or op.has_sym_count)):
            self.ops[-1] = op._replace(count=last.count + n_rec)
        else:
            self.ops.append(op)
        return None

    def record(self):
        """Record `_gen_grid`: once if it forks on no draw, else once per path (`fork`), depth first, every run from a fresh
        MultiGrid and recorder state; the runs merged into ONE program — the ops before a fork once, then each branch's ops
        under its guard, recursively (a path's ops are contiguous from its last fork on: no branch rejoins)."""
        env = self.env
        self.path = []              # the forks of the path being recorded: dict(values, idx, q, zero, start)
        self.written = set()        # draw registers that the branches recorded so far write
        merged = sym = late = template = grid = spawn = None
        runs = 0
        while True:
            runs += 1
            if runs > 64:
                raise NotImplementedError("_gen_grid forks into more than 64 paths: every path is recorded by a run of its own and "
                                          "every env replays the whole merged program")
            self.active = True
            self.grid = None
            _trace.env = env
            try:
                env._gen_grid(self.width, self.height)
            finally:
                _trace.env = None
                self.active = False
            g = self.grid
            if g is None or env.grid is not g:
                raise RuntimeError("_gen_grid must assign self.grid = MultiGrid((width, height))")
            kw = env.agent_spawn_kwargs or {}
            if _any_draw(*[v for k in ("top", "size") if kw.get(k) is not None for v in kw[k]]):
                raise NotImplementedError("agent_spawn_kwargs with a _rand_int draw: the spawn rectangle is also used by respawn and "
                                          "late spawns, long after the reset that made the draw — not supported")
            if self.fork_i != len(self.path):
                raise ValueError("_gen_grid is not a function of its arguments and its draws: run again for another path it made "
                                 "fewer forks")
            if merged is None:
                merged, sym, late, template = list(self.ops), list(self.sym), dict(self.late), g._template
                grid, spawn = g, env.agent_spawn_kwargs
            else:
                # the run shares everything before the fork whose next value it took with the runs before it
                if (self.ops[:shared] != prefix or self.sym != sym or not np.array_equal(g._template, template)):
                    raise ValueError("_gen_grid is not a function of its arguments and its draws: run again for another path it "
                                     "recorded another layout before the fork")
                if not _same_spawn(env.agent_spawn_kwargs, spawn):
                    raise ValueError("_gen_grid leaves agent_spawn_kwargs that differ between the paths of a fork: the spawn "
                                     "rectangle is the launch's, not an env's")
                for i, e in self.late.items():
                    if i >= shared:
                        late[len(merged) + i - shared] = e
                merged.extend(self.ops[shared:])
                # the grid that stays is the first run's: a cell that another path draws differently, or may have filled,
                # counts as "may have been written" there (`grid.get()` warns on it, whatever path is asked about)
                grid._maybe |= g._maybe | (g._shadow != grid._shadow)
            self.written.update(op.register for op in self.ops if op.sets_register)
            while self.path and self.path[-1]["idx"] + 1 == len(self.path[-1]["values"]):
                self.path.pop()
            if not self.path:
                break
            self.path[-1]["idx"] += 1           # the next path: the deepest fork with a value left takes it
            shared = self.path[-1]["start"]
            prefix = self.ops[:shared]
        env.grid = self.grid = grid             # (the first run's: the template is the same in every run, `_maybe` covers them all)
        K = getattr(env, "level_edits", 0)
        if K:       # the env's own cell edits: ONE op behind everything `_gen_grid` recorded, on every path — unguarded
            merged.append(RecordedOp.edits(K))
        if len(merged) > N.MAX_GEN:
            fills = sum(1 for op in merged if op.is_fill)
            raise NotImplementedError("_gen_grid records %d reset-program ops — %d groups of random placements and %d rectangle "
                                      "fills for static edits made after the first place_obj — and a device program holds at most "
                                      "%d (MG_MAX_GEN: a sanity bound — every env replays the whole program at every reset): draw the "
                                      "static layout before the first place_obj (it then costs nothing)"
                                      % (len(merged), len(merged) - fills, fills, N.MAX_GEN))
        self.ops, self.late = merged, late
        return Recording(template, list(merged), list(sym), dict(late))


def pack_program(ops, width, height, cells_stride, n_objs):
    """Recorded ops as the kernels read them: a ctypes MgGenOp array (at least one element) and the reject tables of the
    placements that have one, stacked — (n, cells_stride) uint8, None without any; MgGenOp.reject is an op's row, or -1.
    (The library cannot look into device memory from the host: what the kernels rely on is checked here.)"""
    tables = []
    packed = (N.GenOp * max(1, len(ops)))()
    for o, op in zip(packed, ops):
        op = RecordedOp._make(op)       # (a plain 8-tuple is as good)
        # the guard of a branch in the upper bits of obj (MG_GEN_GUARD): lo <= hi; the low byte as ever
        g = op.guard
        assert op.guard_bits == 0 or (op.guard_bits & ~0x07FFFF00 == N.GEN_GUARD and g[1] <= g[2])
        if op.is_edits:             # the env's edit list: count is K, nothing else is read
            assert 1 <= op.count <= N.GEN_MAX_EDITS and op.kind == 0 and op.rect == (0, 0, 0, 0) and op.reject is None
        elif op.sets_register:      # a `_rand_int` draw, or a PARAM load: obj is its register, y0 a PARAM's table column
            assert 0 <= op.register < N.GEN_DRAWS and (op.is_draw or op.is_param)
            assert op.is_draw or (0 <= op.y0 < N.GEN_DRAWS and 0 <= op.x0 < op.x1 <= 256)
        else:
            assert (1 if op.is_placement else 0) <= op.kind < n_objs and op.count >= 0
            # (a rectangle with a draw operand was proved by the recorder and is clamped on the device)
            assert op.has_sym_operand or (0 <= op.x0 < op.x1 <= width and 0 <= op.y0 < op.y1 <= height)
        o.obj, o.count, o.max_tries, o.x0, o.y0, o.x1, o.y1 = op.obj, op.count, op.max_tries, op.x0, op.y0, op.x1, op.y1
        o.reject = -1
        if op.reject is not None:   # place_obj(reject_fn=), tabulated: one row of cells_stride bytes each
            row = np.zeros(cells_stride, np.uint8)
            row[:width * height] = np.frombuffer(op.reject, np.uint8)
            o.reject = len(tables)
            tables.append(row)
    return packed, (np.stack(tables) if tables else None)


def decode_program(rec, width, height):
    """a Recording as the plain entries of `scenario_spec()`: the template's edits, then the program's ops in order"""
    def rejected(op):
        cells = np.argwhere(np.frombuffer(op.reject, np.uint8).reshape(width, height))
        return tuple((int(x), int(y)) for x, y in cells)

    out = list(rec.sym)
    for i, op in enumerate(rec.ops):
        if op.guard is not None:
            # an op of a branch on a draw: ("guard", r, lo, hi, entry) — the entry as below, run only where
            # lo <= draw[r] <= hi (no oracle replays these)
            grd = ("guard",) + op.guard
            if not op.is_placement:
                out.extend(grd + (e,) for e in rec.late.get(i, []))
            else:
                entry = ("place_sym", op.kind, op.count, op.max_tries) + op.rect
                if op.reject is not None:
                    entry += (rejected(op),)
                out.append(grd + (entry,))
            continue
        if not op.is_placement:     # a static edit after a placement, or a draw: its symbolic form, once
            out.extend(rec.late.get(i, []))
            continue
        head = ("place", op.obj, op.count, op.max_tries)
        if op.has_sym_operand:      # (encoded operands: no oracle replays these)
            out.append(("place_sym",) + head[1:] + op.rect)
        elif op.reject is not None:     # reject_fn, tabulated: the rejected cells of the sampling rectangle
            out.append(head + op.rect + (rejected(op),))
        else:
            out.append(head if op.rect == (0, 0, width, height) else head + op.rect)
    return out
