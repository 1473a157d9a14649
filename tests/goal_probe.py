"""TEST INFRASTRUCTURE — what a cell IS to goal_distance, read from what `forward` DOES (numpy only).

tests/goal_ref.py:kinds_of restates the flag rule of mg_goal_core.h:goal_cell_kind; this module asks the step instead.  One
grid — one scenario, one seed — in B = 4 W H envs.  Env (x H + y) 4 + d has agent 0's record overwritten to the state
(x, y, d) and runs ONE step in which agent 0 acts `forward` and every other agent `done`.  States whose cell ahead is outside
the grid are not probed (upstream asserts in grid.get there): that env's agent stays where reset put it and acts `done` too.
Per probed state and its cell ahead c:

    not moved                 c blocks
    moved, not done           c is free
    moved, done, reward > 0   c is a goal  (the first step of an episode: a goal's decayed reward is still positive)
    moved, done, reward <= 0  c blocks     (lava: the episode ends with nothing)

Up to four probes enter one cell and must agree: where the agent stands does not enter the step's decision.  The same verdicts
come from the oracle, one fresh env per probe (tests/test_oracle_goal_kinds.py)."""
import numpy as np

from marlgrid_amd import _native as N

SEED = 1337
FORWARD, DONE = 2, 6
BLOCKED, FREE, GOAL = 0, 1, 2
DX, DY = np.array([1, 0, -1, 0]), np.array([0, 1, 0, -1])
NOGHOST = "Test-3AgentCluttered11x11-noghost"
ZOO = "Test-2AgentEmpty9x7-zoo"
SCENES = ["Limit-3Agent100Kinds24x24", "MarlGrid-3AgentCluttered11x11-v0", "Edge-HumanPlayerConfig",
          "Test-3AgentCluttered12x6-nonsquare", NOGHOST]


class Plan(object):
    """the probe of a W x H grid: per env its state (x, y, d), the cell ahead (cx, cy) and whether it is probed"""

    def __init__(self, W, H):
        self.W, self.H, self.B = W, H, 4 * W * H
        e = np.arange(self.B)
        self.d, self.y, self.x = e & 3, (e >> 2) % H, (e >> 2) // H
        self.cx, self.cy = self.x + DX[self.d], self.y + DY[self.d]
        self.probed = (self.cx >= 0) & (self.cx < W) & (self.cy >= 0) & (self.cy < H)

    def records(self, rec0):
        """agent 0's packed records (B,) with X, Y and DIR overwritten in the probed envs; every other byte as reset left it"""
        rec0 = np.asarray(rec0).astype(np.uint64)
        keep = ~np.uint64((0xFF << (8 * N.AG_X)) | (0xFF << (8 * N.AG_Y)) | (0xFF << (8 * N.AG_DIR)))
        new = ((rec0 & keep) | (self.x.astype(np.uint64) << np.uint64(8 * N.AG_X))
               | (self.y.astype(np.uint64) << np.uint64(8 * N.AG_Y)) | (self.d.astype(np.uint64) << np.uint64(8 * N.AG_DIR)))
        return np.where(self.probed, new, rec0)

    def actions(self, n):
        a = np.full((self.B, n), DONE, np.int64)
        a[self.probed, 0] = FORWARD
        return a

    def errors(self, grid, env, pos):
        """the error word every env has to hold after the probe step, (B,): ERR_ASSERT exactly where the probe stood in a cell
        whose object does not let an agent overlap — a wall, say — and moved out of it (`assert cur_cell.can_overlap()`,
        base.py:558: the step records the error and completes the move, so the verdict is read all the same), 0 elsewhere.
        grid (W, H): the probed grid's object ids; env: whose registry knows the kinds; pos (B, 2): agent 0 after the step"""
        lets_go = np.array([True] + [bool(o.can_overlap()) for o in env.obj_reg.objs[1:]])[np.asarray(grid)]
        pos = np.asarray(pos)
        moved = (pos[:, 0] == self.cx) & (pos[:, 1] == self.cy)
        return np.where(self.probed & moved & ~lets_go[self.x, self.y], N.ERR_ASSERT, 0)

    def verdicts(self, pos, done, rew):
        """agent 0 after the step — pos (B, 2), done (B,) its DONE flag, rew (B,) its reward — -> (verdict (W, H) of BLOCKED /
        FREE / GOAL, counts (moved, ended, paid) over the probes).  Every cell is entered by a probe, and the probes agree."""
        pos, done, rew = np.asarray(pos), np.asarray(done).astype(bool), np.asarray(rew, np.float64)
        moved = (pos[:, 0] == self.cx) & (pos[:, 1] == self.cy)
        stayed = (pos[:, 0] == self.x) & (pos[:, 1] == self.y)
        p = self.probed
        assert (moved[p] | stayed[p]).all()
        assert not (done & ~moved)[p].any()         # (an agent that did not move did not end its episode either)
        v = np.where(~moved, BLOCKED, np.where(~done, FREE, np.where(rew > 0, GOAL, BLOCKED)))
        cell = (self.cx * self.H + self.cy)[p]
        lo = np.full(self.W * self.H, 9)
        hi = np.full(self.W * self.H, -1)
        np.minimum.at(lo, cell, v[p])
        np.maximum.at(hi, cell, v[p])
        assert (hi >= 0).all(), "a cell no probe entered"
        assert np.array_equal(lo, hi), ("probes that enter one cell disagree", np.argwhere((lo != hi).reshape(self.W, self.H)))
        return lo.reshape(self.W, self.H), (int(moved[p].sum()), int((moved & done)[p].sum()), int((rew > 0)[p].sum()))


def assert_probe_ready(grid, flags):
    """grid (B, W, H), flags (B, n): one grid in every env, agent 0 in a cell in every env"""
    assert (grid == grid[0]).all()
    want = N.AF_ACTIVE | N.AF_PLACED
    assert ((flags[:, 0] & (want | N.AF_EVICTED | N.AF_DONE)) == want).all()


def hold(free, goal, verdict, fields, leave_out=()):
    """free, goal (W, H): the flag rule's maps of the probed grid (goal_ref.classify); verdict: Plan.verdicts' map; fields: the
    kernels' field of that grid by path.  The probed maps equal the rule's cell for cell, but exactly the cells `leave_out`, and
    the reverse queue search over the PROBED maps equals every field.  -> that field"""
    import goal_ref as G
    rule = np.where(goal, GOAL, np.where(free, FREE, BLOCKED))
    differ = {(int(x), int(y)) for x, y in np.argwhere(rule != verdict)}
    assert differ == {(int(x), int(y)) for x, y in leave_out}, differ
    free_step, goal_step = verdict == FREE, verdict == GOAL
    for x, y in leave_out:      # (the analysis ignores other agents: a lower bound there, by goal_distance's docstring)
        free_step[x, y], goal_step[x, y] = free[x, y], goal[x, y]
    want = G.field_queue(free_step, goal_step)
    for path, got in fields.items():
        assert np.array_equal(got, want), path
    return want


# The docstring of MultiGridEnv.goal_distance as a table, by object id 1 .. 11 of tests/scenarios.py:objects_zoo_spec — Wall, Goal,
# open / closed / locked Door, Key, Ball, Lava, Floor, BonusTile, Box: free = open Door, Floor, BonusTile; goal = Goal
ZOO_VERDICTS = [BLOCKED, GOAL, FREE, BLOCKED, BLOCKED, BLOCKED, BLOCKED, BLOCKED, FREE, FREE, BLOCKED]


def zoo_objects(PO):
    """(name, object): one of each kind of objects_zoo_spec, in its order — ZOO_VERDICTS[i] is what entry i has to be"""
    return [("Wall", PO.Wall()), ("Goal", PO.Goal(color="green", reward=1)), ("open Door", PO.Door("blue", 1)),
            ("closed Door", PO.Door("blue", 2)), ("locked Door", PO.Door("blue", 3)), ("Key", PO.Key("blue")),
            ("Ball", PO.Ball("purple")), ("Lava", PO.Lava()), ("Floor", PO.Floor("grey")),
            ("BonusTile", PO.BonusTile(color="yellow", reward=1)), ("Box", PO.Box("olive"))]


def zoo_cells(W, H, agent_cells, count=11):
    """`count` interior cells, pairwise non-adjacent (x + y even), none under an agent (putting over an agent evicts it) and
    none the scenario's own goal cell (W - 2, H - 2)"""
    taken = {(int(x), int(y)) for x, y in agent_cells} | {(W - 2, H - 2)}
    cells = [(x, y) for y in range(1, H - 1) for x in range(1, W - 1) if (x + y) % 2 == 0 and (x, y) not in taken]
    assert len(cells) >= count
    return cells[:count]
