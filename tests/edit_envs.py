"""TEST INFRASTRUCTURE — per-env cell edits (`MultiGridEnv(level_edits=K)`, the EDITS op of the reset program) and their
constant TWINS: the same scenario subclass whose `_gen_grid` calls the parent's and then writes the same cells with
`self.put_obj(obj, x, y)` / `self.grid.set(x, y, None)` in list order — static fill ops of the recorder, a path already pinned
to the oracle and the reference.  A mixed batch of an edits env must equal, env by env, the twin of that env's list built with
the same seeds.  `registered()` makes `Edits-Cluttered15` (ClutteredMultiGrid 15 x 15, 3 agents; takes `level_edits=`) and
`Edits-Cluttered15-L<i>-K<K>` (the twin of list i at K entries) known to `marlgrid_amd.envs.make`.

An entry is (x, y, kind, on); kinds as ClutteredMultiGrid registers them: 0 None, 1 Wall, 2 the green Goal.  The static goal
sits at (13, 13)."""
import contextlib
import functools

import numpy as np

W = H = 15
N_AGENTS, VIEW = 3, 7
WALL, GOAL = 1, 2
BASE = "Edits-Cluttered15"
_FULL = [(1, 7, 0, 1),          # a clear of a cell next to the border (clutter may have put a wall there)
         (2, 2, WALL, 1), (12, 3, WALL, 1), (6, 10, WALL, 1), (9, 9, WALL, 1), (10, 2, WALL, 1), (3, 11, WALL, 1)]


def lists(K):
    """the four edit lists at K entries per env (K >= 4)"""
    assert 4 <= K <= len(_FULL)
    return [
        [],                                                                 # nothing
        [(7, 7, WALL, 1), (8, 8, WALL, 0)],                                 # one wall on an interior cell (and an entry that is off)
        [(4, 9, GOAL, 1), (4, 9, WALL, 1),                                  # one cell twice: the later wins
         (W - 2, H - 2, 0, 1), (3, 3, GOAL, 1)],                            # the goal moved: cleared where it is, put elsewhere
        _FULL[:K],                                                          # a full list
    ]


def table(K, B):
    """(B, K, 4) uint8: list b % 4 for env b, and which list each env holds"""
    which = np.arange(B) % 4
    t = np.zeros((B, K, 4), np.uint8)
    for i, lst in enumerate(lists(K)):
        if lst:
            t[which == i, :len(lst)] = np.asarray(lst, np.uint8)
    return t, which


def _twin_class(edits):
    from marlgrid_amd import envs as E
    from marlgrid_amd.objects import Goal, Wall

    def make(kind):
        return {WALL: Wall(), GOAL: Goal(color="green", reward=1)}[kind]

    class EditsTwin(E.ClutteredMultiGrid):
        def _gen_grid(self, width, height):
            super()._gen_grid(width, height)
            for x, y, kind, on in edits:
                if not on:
                    continue
                if kind == 0:
                    self.grid.set(x, y, None)
                else:
                    self.put_obj(make(kind), x, y)
    return EditsTwin


def name_of(i=None, K=4):
    return BASE if i is None else "%s-L%d-K%d" % (BASE, i, K)


@contextlib.contextmanager
def registered(Ks=(4, 7)):
    """the ids above in `marlgrid_amd.envs`' registry for the length of the block — tests/native/hostemu.py builds an env by its
    id —, and out of it again: tests/test_gen_recording_pinned.py pins a recording of EVERY id the registry holds"""
    from marlgrid_amd import envs as E
    fixed = dict(grid_size=W, clutter_density=0.15)
    mine = {BASE: functools.partial(E._construct, E.ClutteredMultiGrid, N_AGENTS, (VIEW, 0), None, fixed)}
    for K in Ks:
        for i, lst in enumerate(lists(K)):
            mine[name_of(i, K)] = functools.partial(E._construct, _twin_class(lst), N_AGENTS, (VIEW, 0), None, fixed)
    assert not set(mine) & set(E._registry)
    E._registry.update(mine)
    try:
        yield
    finally:
        for name in mine:
            del E._registry[name]


def build(i=None, K=4, **kw):
    """the edits env (i None; any `make` kwarg: pipeline=, devices=) or the twin of list i"""
    from marlgrid_amd import envs as E
    with registered():
        if i is None:
            return E.make(BASE, level_edits=K, **kw)
        return E.make(name_of(i, K), **kw)


# ---- the twins restated BY HAND for the oracle: the base scenario's entries (tests/scenarios.py:cluttered_spec) plus the fills --
def spec(i, K, max_steps=10):
    import scenarios
    s = scenarios.cluttered_spec(N_AGENTS, W, VIEW, clutter_density=0.15, max_steps=max_steps)
    fills = [("put", kind, x, y) for x, y, kind, on in lists(K)[i] if on]
    s["gen_ctor"] = list(s["gen_ctor"]) + fills
    s["gen_reset"] = list(s["gen_reset"]) + fills
    return s
