"""TEST INFRASTRUCTURE — what tests/test_memory_host.py (the host build of the bodies) and tests/test_hip_memory.py (the device)
share: the scenario table of the memory maps — explore_cases.CASES as they are, and the two registered hide scenarios — and the
driver that steps a subject beside tests/memory_ref.py and compares all SIX tensors — exact equality — after reset() and after
EVERY step, with the invariants between them.

`assert_coverage` reads, on the REFERENCE's side, what a run must have met (a subject cannot pass by exercising nothing); it is
meant for batches of 67 envs and more under `run`'s seeds and action stream (at B = 1 doorkey meets no stale door)."""
import numpy as np

import explore_cases as XC
import memory_ref as MR
import scenarios as S

HIDE3, HIDE4 = "Test-3AgentCluttered9x9-hide", "Test-4AgentEmpty5x5-hide"
CASES = dict(XC.CASES)
CASES["hide_cluttered"] = dict(name=HIDE3, spec=lambda: S.registered(HIDE3), steps=40)
CASES["hide_empty"] = dict(name=HIDE4, spec=lambda: S.registered(HIDE4), steps=40)
TABLE = [k for k in CASES if k != "large"]
KEYS = XC.KEYS + ("memory", "seen_step")


class Case(XC.Case):
    def __init__(self, key):
        c = CASES[key]
        self.key, self.c = key, c
        self.mode, self.steps, self.corners = c.get("mode", False), c["steps"], bool(c.get("corners"))
        self.kw = dict(c.get("kw", {}))
        self.spec = c["spec"]()

    def reference(self, B):
        return MR.RefBatch(self.spec, self.seeds(B), self.mode)


def compare(got, ref, what):
    XC.compare(got, ref, what)
    want = ref.ref.tensors()
    for key in ("memory", "seen_step"):
        g, w = np.asarray(got[key]), want[key]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, key, g.shape, w.shape, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            cells = (g != w).any(axis=-1) if key == "memory" else g != w
            at = tuple(int(v) for v in np.argwhere(cells)[0])
            raise AssertionError("%s: %s differs in %d cells of %d envs; at [b, k, x, y] = %s got %s, want %s; step count %d; "
                                 "oracle state of env %d: %s"
                                 % (what, key, int(cells.sum()), np.unique(np.argwhere(cells)[:, 0]).size, at, g[at], w[at],
                                    ref.ref.sc[at[0]], at[0], {k: v for k, v in ref.state(at[0]).items() if k != "base"}))
    invariants(got, ref.ref.sc, ref.ref.seen_step == ref.ref.sc[:, None, None, None], what)


def invariants(got, step_count, visible_now, what):
    """memory[..., 3] == seen; (seen_step >= 0) == seen; every cell visible in the observation just returned (`visible_now`,
    the reference's) has seen_step == step_count[b]"""
    seen, mem, stamp = np.asarray(got["seen"], bool), np.asarray(got["memory"]), np.asarray(got["seen_step"])
    assert np.array_equal(mem[..., 3] != 0, seen) and (mem[..., 3] <= 1).all(), (what, "memory[..., 3] == seen")
    assert np.array_equal(stamp >= 0, seen), (what, "(seen_step >= 0) == seen")
    assert (stamp[visible_now] == np.broadcast_to(step_count[:, None, None, None], stamp.shape)[visible_now]).all(), (what, "stamps")
    assert not mem[~seen].any(), (what, "a cell never seen is (0, 0, 0, 0)")


def run(case, subject, B, steps=None, after_step=None):
    """explore_cases.run with the six tensors: `subject` as there, its tensors() with `memory` and `seen_step` as well.
    -> the reference (`ref.ref.stats`: the coverage counts)"""
    ref = case.reference(B)
    ref.coverage = XC.Coverage(case)
    subject.reset()
    ref.reset()
    compare(subject.tensors(), ref, "%s, reset()" % case.key)
    for k, x, y, d in case.start(subject.W, subject.H):
        subject.place(k, x, y, d)
        XC.place_oracle(ref, k, x, y, d)
    rng = np.random.RandomState(77 + len(case.key))
    for t in range(1, (steps or case.steps) + 1):
        a = rng.randint(0, 7, size=(B, subject.n))
        done = np.asarray(subject.step(a), bool)
        want_done = ref.step(a)
        assert np.array_equal(done, want_done), (case.key, t, "done")
        compare(subject.tensors(), ref, "%s, step %d" % (case.key, t))
        ref.coverage.watch(ref)
        ref.ref.watch(case.spec)
        if after_step is not None and after_step(t, done, ref):
            compare(subject.tensors(), ref, "%s, after step %d's reset by hand" % (case.key, t))
    return ref


def assert_coverage(case, ref, B, doors=True):
    """B >= 67 only.  (a) every case: a known, currently not visible cell remembers an agent where none stands now — memory, not
    a re-encode of the grid; (b) doorkey*: a remembered door triple differs from the door's present state; (c) hide cases: a
    viewer that hides Wall knows a cell as (0, 0, 0, 1) where the oracle's grid holds a wall; (d) headline: planes with known
    cells were cleared; (e) every case: a known cell was overwritten with a different triple.  Counted at 67 envs over every
    case of TABLE: (a) at least 1 183 times (geo_off2), (e) at least 3 139 (geo_v3), (c) 68 538 and 33 916, (d) 536, (b) 32 for
    doorkey_colored — and 0 for doorkey, where no door is unlocked at that batch: `doors=False` leaves (b) to a run at a
    batch that meets it.  Every case of TABLE meets (a).  How (b) is counted (memory_ref.MemoryRef.watch, `stale_doors`): after
    every step, over all envs, agents and cells, one for each cell that is known, whose remembered type is Door, whose grid
    object is a Door now, and whose remembered triple differs from that door's — a stale door counts once per step and agent
    for as long as it stays stale"""
    assert B >= 67
    st = ref.ref.stats
    assert st["ghost_agents"] > 0, (case.key, st)
    assert st["overwrites"] > 0, (case.key, st)
    if doors and case.key in ("doorkey", "doorkey_colored"):
        assert st["stale_doors"] > 0, (case.key, st)
    if case.key in ("hide_cluttered", "hide_empty"):
        assert st["hidden_walls"] > 0, (case.key, st)
    if case.key == "headline":
        assert st["clears"] > 0, (case.key, st)
