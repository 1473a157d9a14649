"""TEST INFRASTRUCTURE — the differentials of WHOLE LEVELS (seed, parameters, cell edits) against the CPU oracle: what the host
differential (tests/test_levels_diff_host.py) and the GPU differentials (tests/test_hip_levels_oracle.py, L1 - L7) share.  All
go through tests/wide_diff.py:run with a tests/level_ref.py:WideRef — a LevelOracle — as the reference, the hand-written specs of
tests/level_envs.py, and a PLAN: what is set on both sides between two steps.

  EditsPlan   plain `set_edits` under same-step reset: a random list per env from a table that also holds garbage entries, a
              third of the envs given new lists every 20 steps, by mask and by ids in turn
  BankPlan    a full LevelBank of L slots: `set_levels(bank, ids, env_mask=done)` before every step — ids with -1, a slot outside
              the bank and an emptied slot —, `bank.assign(slots, seeds, params=, edits=)` at given steps
  SeedsPlan   the seeds form, `set_levels(seeds=..., env_mask=done)`, with plain `set_params` / `set_edits` on the same envs

Coverage is a condition of every case and is read on the ORACLE's side (`Coverage.watch`, from the LevelOracle's own record of
which envs its last call reset from a level): a subject cannot pass by never taking a level."""
import numpy as np

import level_envs as LE
import level_ref
import wide_diff

SEED0 = 717100
WAVE = 64


def subject_env(subject):
    return subject.env if hasattr(subject, "env") else subject.emu.env


def on_device(subject):
    return hasattr(subject, "env")


def _dev(subject, a):
    if not on_device(subject):
        return a
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(subject.env.device)


def product_rows(lst, K):
    """an oracle list -> (K, 4) uint8 product entries, the slots behind it off"""
    t = np.zeros((K, 4), np.uint8)
    if lst:
        t[:len(lst), :3] = np.asarray(lst, np.uint8)
        t[:len(lst), 3] = 1
    return t


def write_edits(subject, table, mask=None, ids=None):
    """(B, K, 4) uint8 entries, garbage included, into the product's table: on the device `set_edits` with a device tensor (only
    clamped: the device guards what it reads), by mask or by ids; on the host build the same bytes into the dry env's table"""
    env = subject_env(subject)
    if on_device(subject):
        if ids is not None:
            env.set_edits(_dev(subject, table[ids]), env_ids=_dev(subject, np.asarray(ids, np.int64)))
        else:
            env.set_edits(_dev(subject, table), env_mask=None if mask is None else _dev(subject, mask))
    else:
        sel = slice(None) if mask is None and ids is None else (mask if ids is None else ids)
        env.edits_t[sel] = table[sel]


class Coverage(object):
    def __init__(self, lo, B, L=0):
        self.lo, self.B, self.L = lo, B, L
        self.slot_of_env = None                 # BankPlan: the slot each env is pointed at (the plan keeps it up to date)
        self.episode_slot = np.full(B, -1, np.int64)
        self.slots_played = set()
        self.max_shared = 0                     # the most envs that took ONE slot in one launch
        self.full_waves = self.single_lane_waves = 0
        self.last_env_levelled = 0
        self.across_assign = 0                  # episodes of a slot that were running when the slot was assigned to
        self.free_episodes = np.zeros(B, np.int64)
        self.garbage = set()
        self.carried = set()                    # kinds seen in an agent's hands
        self.launches = 0

    def note_table(self, table, n_obj):
        rows = table.reshape(-1, 4)
        rows = rows[rows.any(axis=1)]
        self.garbage |= set(int(c) for c in np.unique(LE.garbage_class(rows, n_obj)) if c >= 0)

    def watch(self, t, envs, mask):
        lo = self.lo
        took = lo.last_reset & (lo.episode_level >= 0)
        self.free_episodes += lo.last_reset & (lo.episode_level < 0)
        if took.any():
            self.launches += 1
            per_wave = np.add.reduceat(took.astype(np.int64), np.arange(0, self.B, WAVE))
            self.full_waves += int((per_wave == WAVE).sum())
            self.single_lane_waves += int((per_wave == 1).sum())
            self.last_env_levelled += int(took[-1])
            if self.slot_of_env is not None:
                s = self.slot_of_env[took]
                self.episode_slot[took] = s
                self.slots_played |= set(int(v) for v in np.unique(s))
                self.max_shared = max(self.max_shared, int(np.bincount(s).max()))
        if self.slot_of_env is not None:
            self.episode_slot[lo.last_reset & ~took] = -1
        if t % 5 == 0 and len(lo.spec["objects"]) > 3:
            for e in envs:
                c = e.state()["carrying"]
                if c.any():
                    self.carried |= set(int(v) for v in c if v)

    def assigned(self, slots):
        running = ~self.lo.pending
        self.across_assign += int((running & np.isin(self.episode_slot, slots)).sum())


class EditsPlan(object):
    """L1: `Edits-Cluttered15`, plain set_edits"""

    def __init__(self, B, K, T, every=20, seed=11, box=(1, 1, LE.W - 1, LE.H - 1)):
        self.B, self.K, self.every, self.box = B, K, every, box
        self.rng = np.random.RandomState(seed)
        self.n_obj = 5

    def attach(self, ref, cov):
        self.lo, self.cov = ref.lo, cov

    def between(self, t, sub, envs):
        B, K = self.B, self.K
        if t == 0:
            tab = LE.mixed_table(self.rng, B, K, self.n_obj, box=self.box)
            write_edits(sub, tab)
            self.lo.set_edits([LE.oracle_list(tab[b], self.n_obj) for b in range(B)])
            self.cov.note_table(tab, self.n_obj)
        elif t % self.every == 0:
            j = t // self.every
            m = (np.arange(B) + j) % 3 == 0
            tab = LE.mixed_table(self.rng, B, K, self.n_obj, box=self.box)
            if j % 2:
                write_edits(sub, tab, mask=m)
            else:
                write_edits(sub, tab, ids=np.nonzero(m)[0])
            self.lo.set_edits([LE.oracle_list(tab[b], self.n_obj) for b in range(B)], mask=m)
            self.cov.note_table(tab[m], self.n_obj)

    def require(self, out):
        assert self.cov.garbage == {0, 1, 2, 3}, self.cov.garbage                 # every garbage class was in a table
        assert self.cov.carried & {LE.KEY, LE.BALL}, self.cov.carried             # something an edit placed was picked up
        assert out["episodes"].min() >= 3


def free_envs(B):
    """the envs that never take a level: lane 1 of every wave but the first (the first reset hands levels to all 64 lanes of
    wave 0; the last env of the ragged wave is not among them), env 33 in a batch of one wave"""
    f = (np.arange(B) % WAVE == 1) & (np.arange(B) >= WAVE)
    if not f.any():
        f[33] = True
    return f


class BankPlan(object):
    """L2 / L3 / L5 / L7 and the host differential: a full bank.  name: LE.CURRICULUM (levels carry `n_clutter`) or LE.EDITS"""
    WATCHER, WATCHED_SLOT = 9, 2

    def __init__(self, name, B, K, T, L=37, assign_at=(), seed=1, box=(1, 1, LE.W - 1, LE.H - 1)):
        self.name, self.B, self.K, self.T, self.L, self.box = name, B, K, T, L, box
        self.par = name == LE.CURRICULUM
        self.kinds = (0, LE.WALL, LE.GOAL) if self.par else (0, LE.WALL, LE.GOAL, LE.KEY, LE.BALL)
        rng = np.random.RandomState(seed)
        self.free = free_envs(B)
        ids = rng.randint(0, L, size=(T + 1, B)).astype(np.int64)
        u = rng.rand(T + 1, B)
        ids[u < 0.04] = -1                                  # now and then free-running for an episode
        ids[(u >= 0.04) & (u < 0.07)] = L                   # ... or pointed at a slot outside the bank
        ids[0] = np.arange(B) % L                           # the first reset: every env a level, every slot played
        ids[0, 20:32] = 3                                   # ... and twelve envs on one slot in one launch
        ids[:, self.WATCHER] = self.WATCHED_SLOT
        ids[:, self.free] = -1
        self.ids = ids
        self.first = self._levels(rng, np.arange(L), 5000)
        self.first[1][1] = 2 ** 32 + 7
        self.events = {}
        for j, t in enumerate(assign_at):
            slots = rng.choice(np.setdiff1d(np.arange(L), [self.WATCHED_SLOT]), size=4, replace=False)
            slots = np.concatenate([[self.WATCHED_SLOT], slots])           # the watched slot is assigned to at every event
            ev = self._levels(rng, slots, 9000 + 100 * j)
            if j % 2 == 0:
                ev[1][-1] = -1                              # a slot is emptied: the envs pointed at it run free
            self.events[t] = ev

    def _levels(self, rng, slots, seed0):
        k = len(slots)
        return [np.asarray(slots, np.int64), seed0 + np.arange(k, dtype=np.int64), rng.randint(0, LE.N_CLUTTER_HI, size=k).astype(np.int64),
                [LE.random_list(rng, self.K, kinds=self.kinds, box=self.box) for _ in range(k)]]

    def attach(self, ref, cov):
        self.lo, self.cov = ref.lo, cov
        self.bankref = level_ref.BankRef(self.L, self.B, {"n_clutter": LE.N_CLUTTER_DEFAULT} if self.par else {})
        cov.slot_of_env = self.bankref.ids

    def _assign(self, sub, ev):
        slots, seeds, clutter, lists = ev
        rows = np.stack([product_rows(lst, self.K) for lst in lists])
        kw = dict(params=dict(n_clutter=_dev(sub, clutter))) if self.par else {}
        self.bank.assign(_dev(sub, slots), _dev(sub, seeds), edits=_dev(sub, rows), **kw)
        self.bankref.assign(slots, seeds, params=dict(n_clutter=clutter) if self.par else None, edits=lists)

    def _point(self, sub, ids, mask):
        env = subject_env(sub)
        if on_device(sub):
            env.set_levels(self.bank, _dev(sub, ids), env_mask=None if mask is None else _dev(sub, mask))
        else:                   # (host values are checked: the slot outside the bank goes into the table as a device tensor's would)
            env.set_levels(self.bank, np.where(ids >= self.L, -1, ids), env_mask=mask)
            m = (ids >= self.L) & (True if mask is None else mask)
            env._levels.level_of_env[m] = ids[m]
        self.bankref.point(ids, mask)

    def between(self, t, sub, envs):
        env, lo = subject_env(sub), self.lo
        if t == 0:
            self.bank = env.level_bank(self.L, full=True)
            self._assign(sub, self.first)
            # the free-running envs' own rows: what they must keep
            own = [LE.random_list(np.random.RandomState(77 + b), min(self.K, 3), kinds=self.kinds, box=self.box) + [(2, 2, LE.WALL)]
                   for b in range(self.B)]
            own = [lst[-self.K:] for lst in own]
            tab = np.stack([product_rows(lst, self.K) for lst in own])
            write_edits(sub, tab, mask=self.free)
            lo.set_edits(own, mask=self.free)
            if self.par:
                vals = (np.arange(self.B) * 5) % LE.N_CLUTTER_HI
                env.set_params(n_clutter=_dev(sub, vals), env_mask=_dev(sub, self.free))
                lo.set_params(mask=self.free, n_clutter=vals)
            self._point(sub, self.ids[0], None)
        else:
            if t in self.events:
                self.cov.assigned(self.events[t][0])
                self._assign(sub, self.events[t])
            self._point(sub, self.ids[t], lo.pending.copy())
        self.bankref.push(lo)

    def require(self, out, wide=True):
        cov, lo = self.cov, self.lo
        lev = lo.levelled[~self.free]
        assert lev.min() >= 3, lev.min()                                   # every env started >= 3 episodes from a level
        assert cov.slots_played == set(range(self.L)), sorted(set(range(self.L)) - cov.slots_played)
        assert cov.max_shared >= 10, cov.max_shared
        assert cov.last_env_levelled >= 1
        assert self.free.any() and (lo.levelled[self.free] == 0).all() and (cov.free_episodes[self.free] >= 3).all()
        assert all(lo.table_edits[b] for b in np.nonzero(self.free)[0])     # ... and their own rows are lists, not nothing
        assert (cov.free_episodes[~self.free] > 0).any()                    # others went back to their running stream in between
        if self.events:
            assert cov.across_assign >= 1, cov.across_assign
        if wide:
            assert cov.full_waves >= 1 and cov.single_lane_waves >= 1, (cov.full_waves, cov.single_lane_waves)


class MaskPlan(BankPlan):
    """L6: no auto-reset — `set_levels(bank, ids, env_mask=mask)` then `reset(env_mask=mask)` every `every` steps, with masks of
    one env, one whole wave, every other env and all, in turn; state and RNG are compared after each reset"""

    def __init__(self, name, B, K, T, every=5, **kw):
        BankPlan.__init__(self, name, B, K, T, **kw)
        self.every = every
        self.ids[:, self.free] = np.arange(B)[self.free] % self.L        # (nobody can run free here: a free env never resets)
        self.free[:] = False
        self.masks_used = []

    def mask(self, j):
        B, m = self.B, np.zeros(self.B, bool)
        kind = j % 4
        if kind == 0:
            m[(37 * j + B - 1) % B] = True                  # one env (the first time: the last env of the ragged wave)
        elif kind == 1:
            w = (j // 4) % (B // WAVE)
            m[w * WAVE:(w + 1) * WAVE] = True               # one whole wave
        elif kind == 2:
            m[(j // 4) % 2::2] = True                       # every other env
        else:
            m[:] = True
        return m

    def between(self, t, sub, envs):
        lo = self.lo
        if t == 0:
            BankPlan.between(self, 0, sub, envs)
            return
        if t in self.events:
            self.cov.assigned(self.events[t][0])
            self._assign(sub, self.events[t])
            self.bankref.push(lo)
        if t % self.every:
            return
        m = self.mask(t // self.every - 1)
        self.masks_used.append(int(m.sum()))
        self._point(sub, self.ids[t], m)
        self.bankref.push(lo)
        sub.reset(m)
        lo.reset_envs(m)
        self.cov.watch(t, envs, m)
        return True

    def require(self, out):
        cov, lo = self.cov, self.lo
        assert lo.levelled.min() >= 3, lo.levelled.min()
        assert cov.slots_played == set(range(self.L)) and cov.max_shared >= 10 and cov.last_env_levelled >= 1
        assert cov.full_waves >= 1 and cov.single_lane_waves >= 1
        assert {1, WAVE, (self.B + 1) // 2, self.B} <= set(self.masks_used), self.masks_used


class SeedsPlan(object):
    """L4: the seeds form with plain set_params / set_edits on the same envs (the README's "parameters together with
    `set_levels`"): the env takes the generator alone, its rows are what the setters gave it"""

    def __init__(self, B, K, T, every=15, seed=2):
        self.B, self.K, self.T, self.every = B, K, T, every
        self.rng = np.random.RandomState(seed)
        self.free = free_envs(B)
        self.pool = 3000 + np.arange(50, dtype=np.int64)
        self.pool[7] = 2 ** 32 + 5

    def attach(self, ref, cov):
        self.lo, self.cov = ref.lo, cov

    def _seeds(self):
        s = self.pool[self.rng.randint(0, len(self.pool), size=self.B)]
        s[self.rng.rand(self.B) < 0.05] = -1
        s[self.free] = -1
        return s

    def _rows(self, sub, m):
        env, lo, B = subject_env(sub), self.lo, self.B
        vals = self.rng.randint(0, LE.N_CLUTTER_HI, size=B).astype(np.int64)
        lists = [LE.random_list(self.rng, self.K, kinds=(0, LE.WALL, LE.GOAL)) for _ in range(B)]
        tab = np.stack([product_rows(lst, self.K) for lst in lists])
        env.set_params(n_clutter=_dev(sub, vals), env_mask=_dev(sub, m))
        write_edits(sub, tab, ids=np.nonzero(m)[0])
        lo.set_params(mask=m, n_clutter=vals)
        lo.set_edits(lists, mask=m)

    def between(self, t, sub, envs):
        env, lo = subject_env(sub), self.lo
        if t == 0:
            self._rows(sub, np.ones(self.B, bool))
            s = self._seeds()
            s[~self.free] = np.where(s[~self.free] < 0, 3000, s[~self.free])        # the first reset: everyone but the free envs
            env.set_levels(seeds=_dev(sub, s))
            lo.set_levels(s)
            return
        if t % self.every == 0:
            self._rows(sub, (np.arange(self.B) + t // self.every) % 3 == 0)
        s, m = self._seeds(), lo.pending.copy()
        env.set_levels(seeds=_dev(sub, s), env_mask=_dev(sub, m))
        lo.set_levels(s, m)

    def require(self, out):
        cov, lo = self.cov, self.lo
        assert lo.levelled[~self.free].min() >= 3 and (lo.levelled[self.free] == 0).all()
        assert cov.last_env_levelled >= 1 and cov.full_waves >= 1 and cov.single_lane_waves >= 1
        assert (cov.free_episodes[~self.free] > 0).any()


def run(subject, name, plan, T, max_steps, mode, spec=None, **kw):
    """wide_diff.run of `subject` against a LevelOracle of the hand-written spec of `name`, with `plan` between the steps and
    its coverage required -> (what run returns, Coverage)"""
    B = subject.B
    spec = spec or LE.spec_of(name, max_steps)
    env = subject_env(subject)
    assert len(env.obj_reg.objs) == len(spec["objects"])
    ref = level_ref.WideRef(spec, SEED0 + np.arange(B), mode, n_obj=len(spec["objects"]))
    cov = Coverage(ref.lo, B, getattr(plan, "L", 0))
    plan.attach(ref, cov)
    out = wide_diff.run(subject, name, SEED0 + np.arange(B), T, spec=spec, mode=mode if mode else "none", ref=ref, watch=cov.watch,
                        between=plan.between, **kw)
    return out, cov
