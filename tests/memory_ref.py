"""TEST INFRASTRUCTURE — the reference the memory maps (`MultiGridEnv(memory=True)`, mg_memory_update) are held to, on the CPU
and built on tests/explore_ref.py: after each `ExploreRef.observe` the oracle's `vis[k]` and `cells[k]` (mgo_view's post-
hide_item_types top codes) of the envs observed, mapped to world cells by `explore_ref.view_cells` — the reference's crop and
rotate, not mg_core.h's view_map — and to triples by the table tests/viewenc.py uses (an object id: its (type, colour, state);
agent code 1000 + x: (agent_type_idx, colour of x, dir of x)).

Rules: clear where the oracle's step count is 0 (memory 0, seen_step -1), overwrite where visible and in the grid, stamp the
step count.  `stats` counts, on the reference's side, what a subject must have been put through (memory_cases asserts them)."""
import numpy as np

import explore_ref as XR
from oracle import oracle as O

AGENT_BASE = XR.AGENT_BASE


class MemoryRef(XR.ExploreRef):
    """ExploreRef with memory (B, n, W, H, 4) uint8 and seen_step (B, n, W, H) int32"""

    def __init__(self, envs):
        super(MemoryRef, self).__init__(envs)
        B, n, W, H = self.B, self.n, self.W, self.H
        self.memory = np.zeros((B, n, W, H, 4), np.uint8)
        self.seen_step = np.full((B, n, W, H), -1, np.int32)
        first = envs[0].envs[0] if self.views else envs[0]
        cfg = first.cfg
        self.obj_tab = np.zeros((AGENT_BASE, 3), np.uint8)         # (as viewenc.oracle_views_batch builds it)
        for o in range(1, cfg.n_obj):
            self.obj_tab[o] = (cfg.obj[o].type_idx, cfg.obj[o].color_idx, cfg.obj[o].state)
        self.agent_type = int(cfg.agent_type_idx)
        self.agent_color = np.array([cfg.agent_color_idx[x] for x in range(n)], np.uint8)
        self.stats = dict(clears=0, overwrites=0, ghost_agents=0, stale_doors=0, hidden_walls=0)

    def observe(self, ids=None):
        ids = np.arange(self.B) if ids is None else np.asarray(ids, np.int64).reshape(-1)
        if ids.size == 0:
            return
        had = self.seen[ids].reshape(len(ids), -1).any(axis=1)
        super(MemoryRef, self).observe(ids)        # (fetches sc, ag, vis, cells of `ids`; seen / visits brought up to date)
        n, W, H = self.n, self.W, self.H
        fresh = self.sc[ids] == 0
        self.stats["clears"] += int((had & fresh).sum())
        self.memory[ids[fresh]] = 0
        self.seen_step[ids[fresh]] = -1
        mem = self.memory.reshape(self.B, n, W * H, 4)
        stamp = self.seen_step.reshape(self.B, n, W * H)
        for k, (vs, off) in enumerate(self.geom):
            ag = self.ag[ids, k]
            cell = XR.view_cells(ag[:, 0].astype(np.int64), ag[:, 1].astype(np.int64), ag[:, 2], vs, off, W, H)
            mark = (self.vis[k][ids] != 0) & (cell >= 0)
            codes = self.cells[k][ids][mark]
            rows = np.broadcast_to(ids[:, None, None], cell.shape)[mark]
            at = cell[mark]
            agent = codes >= AGENT_BASE
            x = np.where(agent, codes - AGENT_BASE, 0)
            quad = np.ones((len(codes), 4), np.uint8)
            quad[:, :3] = self.obj_tab[np.where(agent, 0, codes)]
            quad[agent, 0] = self.agent_type
            quad[agent, 1] = self.agent_color[x[agent]]
            quad[agent, 2] = self.ag[rows[agent], x[agent], 2]
            old = mem[rows, k, at]
            self.stats["overwrites"] += int(((old[:, 3] == 1) & (old[:, :3] != quad[:, :3]).any(axis=1)).sum())
            mem[rows, k, at] = quad
            stamp[rows, k, at] = self.sc[rows]

    def tensors(self):
        return dict(super(MemoryRef, self).tensors(), memory=self.memory, seen_step=self.seen_step)

    def watch(self, spec):
        """the coverage counts of the state just observed (every env): ghost_agents — a known cell not visible now remembers an
        agent where none stands; stale_doors — a remembered Door triple differs from the triple of the door there now;
        hidden_walls — a cell known as (0, 0, 0, 1) whose grid object is a Wall (only a viewer that hides Wall has those)"""
        B, n, W, H = self.B, self.n, self.W, self.H
        occupied = np.zeros((B, W * H), bool)
        for k in range(n):
            placed = self.ag[:, k, 6] >= 0
            occupied[np.nonzero(placed)[0], self.ag[placed, k, 0] * H + self.ag[placed, k, 1]] = True
        now = self.seen_step == self.sc[:, None, None, None]
        known = self.memory[..., 3] == 1
        is_agent = known & (self.memory[..., 0] == self.agent_type)
        self.stats["ghost_agents"] += int((is_agent & ~now & ~occupied.reshape(B, 1, W, H)).sum())
        door_ids = [i for i, o in enumerate(spec["objects"]) if o and o["type"] == "Door"]
        wall_ids = [i for i, o in enumerate(spec["objects"]) if o and o["type"] == "Wall"]
        present = self.obj_tab[self.base]                                    # (B, W, H, 3)
        if door_ids:
            door_type = int(self.obj_tab[door_ids[0], 0])
            there = np.isin(self.base, door_ids)[:, None]
            differs = (self.memory[..., :3] != present[:, None]).any(axis=-1)
            self.stats["stale_doors"] += int((known & (self.memory[..., 0] == door_type) & there & differs).sum())
        empty = known & (self.memory[..., :3] == 0).all(axis=-1)
        self.stats["hidden_walls"] += int((empty & np.isin(self.base, wall_ids)[:, None]).sum())


class RefBatch(XR.RefBatch):
    """explore_ref.RefBatch whose reference is a MemoryRef"""

    def __init__(self, spec, seeds, mode=False):      # (explore_ref.RefBatch's, with the one reference built: a MemoryRef)
        views = any("view" in a for a in spec["agents"])
        self.orc = None if views else O.OracleBatch(spec, seeds)
        self.envs = [O.make_env(spec, int(s)) for s in seeds] if views else self.orc.envs
        self.mode = mode
        self.ref = MemoryRef(self.envs)
        self.B, self.n = self.ref.B, self.ref.n
        self.pending = np.zeros(self.B, bool)
        self.was_reset = np.zeros(self.B, bool)
