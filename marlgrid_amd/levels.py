"""Replayable levels, host side: `LevelBank` — freshly seeded generators on one device — and `EnvLevels`, what a MultiGridEnv
keeps for `set_levels` (the env holds one as `env._levels`, as it holds the recorder as `env._gen`): which bank its envs read,
the slot of each, and the mg_level_apply launch in front of every reset and step.  The kernels are csrc/mg_levels.hip."""
import ctypes as C

import numpy as np

from . import _native as N, gen_edits, per_env as P


class LevelBank(object):
    """Replayable levels: L freshly seeded generators on one device.  A level is a seed; playing it is the reference's
    `env.seed(s); env.reset()` (base.py:371-374, 402-416) — layout, agent placement and every later draw of the episode come
    from a generator seeded with s.  `mt` (L, 624), `pos` (L,), `head` (L, 16): what mg_mt_seed leaves per env; `seeds` (L,)
    int64, -1 = empty slot.  `seeds_or_capacity`: an int — that many empty slots — or the slots' seeds (-1: empty).
    An env is pointed at slots with `env.set_levels(bank, ids)` and takes a copy of its slot's generator at its next reset;
    `assign` replaces levels.  Seeds are hashed and the generators seeded on the device (mg_level_seed).

    A FULL bank (`env.level_bank(..., full=True)`; `env`: the env it is made from) holds whole levels — seed, parameters, cell
    edits: `params` (L, MG_GEN_DRAWS) uint8, the columns of the env's `_param` names, every slot at the declared defaults, and
    `edits` (L, K, 4) uint8 entries (x, y, kind, on), K the env's `level_edits`, all off.  An env that takes a slot's generator
    takes a copy of the slot's rows over its own in the same launch (mg_level_apply_rows) and its reset reads them."""

    def __init__(self, seeds_or_capacity, device=None, _dry=False, env=None):
        self._dry = bool(_dry)
        self.full = env is not None
        self._env = env
        self.K = env.level_edits if self.full else 0
        self.params = self.edits = None
        self._replicas = {}         # device -> the copy of this bank a shard on that device reads (sharding._Shards.set_levels)
        self._readers = {}          # streams that read this bank's rows (an env's mg_level_apply): what `assign` orders itself with
        self.launches = 0
        first = None
        if isinstance(seeds_or_capacity, (int, np.integer)) and not isinstance(seeds_or_capacity, bool):
            L = int(seeds_or_capacity)
        else:
            first = seeds_or_capacity
            L = int(first.shape[0]) if hasattr(first, "shape") and len(first.shape) == 1 else len(first)
        if L < 1:
            raise ValueError("LevelBank: at least one slot")
        self.capacity = L
        if self._dry:
            self.device = None
            self.seeds = np.full(L, -1, np.int64)
            if self.full:
                self.params = np.zeros((L, N.GEN_DRAWS), np.uint8)
                self.edits = np.zeros((L, self.K, 4), np.uint8)
        else:
            import torch
            self.device = torch.device(device if device is not None else "cuda")
            if self.device.type != "cuda":
                raise RuntimeError("marlgrid_amd runs on HIP devices only (got %r)" % (device,))
            if self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
            self._lib = N.lib()
            with torch.cuda.device(self.device):
                self.mt = torch.zeros((L, N.MT_N), dtype=torch.int32, device=self.device)
                self.pos = torch.zeros((L,), dtype=torch.int32, device=self.device)
                self.head = torch.zeros((L, N.MT_HEAD), dtype=torch.int32, device=self.device)
                self.seeds = torch.full((L,), -1, dtype=torch.int64, device=self.device)
                if self.full:
                    self.params = torch.zeros((L, N.GEN_DRAWS), dtype=torch.uint8, device=self.device)
                    self.edits = torch.zeros((L, self.K, 4), dtype=torch.uint8, device=self.device)
        if self.full:
            env._ensure_recorded()
            for d in env._params.decl.values():
                self.params[:, d["col"]] = d["default"]
        if first is not None:
            self.assign(None, first)

    def __len__(self):
        return self.capacity

    @property
    def columns(self):
        """a full bank: parameter name -> its column of `params`"""
        return {name: d["col"] for name, d in self._env._params.decl.items()} if self.full else {}

    def assign(self, slots, seeds, params=None, edits=None):
        """Put `seeds` (k,) into `slots` (k,) — None: slots 0 .. k-1 —, in stream order: the envs pointed at a slot play its new
        level from their next reset on.  -1 empties a slot (its envs run free).  Device int64 tensors: one launch, nothing is
        read back, and two entries naming one slot are the caller's error; host values are checked (ValueError for a slot
        outside the bank, a seed < -1, a slot named twice).

        A full bank also takes the slots' rows: `params` {name: an int or (k,) values} by set_params' rules (host values checked
        against the parameter's interval, a device tensor clamped to it) and `edits`, (K', 4) for every slot or (k, K', 4), by
        set_edits' (host entries checked, the slots from K' on switched off).  What is not given stays as the slot has it.  All
        of it goes in stream order on the ordering of the seeds: no env reads a half-written level."""
        L = self.capacity
        if (params is not None or edits is not None) and not self.full:
            raise ValueError("LevelBank.assign(params=, edits=): a bank of seeds holds no rows; env.level_bank(..., full=True) does")
        if P.on_device(seeds, self.device) and (slots is None or P.on_device(slots, self.device)):
            if seeds.dim() != 1 or (slots is not None and tuple(slots.shape) != tuple(seeds.shape)):
                raise ValueError("LevelBank.assign: slots and seeds of one shape (k,)")
        else:
            seeds = P.host_ints(seeds, "LevelBank.assign(seeds=)").reshape(-1)
            if seeds.size and seeds.min() < -1:
                raise ValueError("LevelBank.assign(seeds=): a seed is >= 0, or -1 for none (got %d)" % seeds.min())
            if slots is not None:
                slots = P.host_ints(slots, "LevelBank.assign(slots=)").reshape(-1)
                if slots.shape != seeds.shape:
                    raise ValueError("LevelBank.assign: slots and seeds of one shape (k,)")
                if slots.size and (slots.min() < 0 or slots.max() >= L):
                    raise ValueError("LevelBank.assign: slots outside 0..%d" % (L - 1))
                if len(np.unique(slots)) != slots.size:
                    raise ValueError("LevelBank.assign: a slot is named twice")
            elif seeds.size > L:
                raise ValueError("LevelBank.assign: %d seeds for %d slots" % (seeds.size, L))
        k = int(seeds.shape[0])
        rows = self._rows(k, params, edits)
        if self._dry:
            at = np.arange(k) if slots is None else slots
            self.seeds[at] = seeds
            self._write_rows(at, rows)
            return
        self._seed_rows(seeds, slots, None, rows)
        for rep in self._replicas.values():
            rep.assign(slots, seeds, params, edits)

    def _rows(self, k, params, edits):
        """`assign`'s params / edits for k slots, checked: [(column, values)], (K, 4) or (k, K, 4) entries or None"""
        if not self.full:
            return None
        env, dev = self._env, self.device
        cols = []
        for name, v in (params or {}).items():
            d = env._params.decl.get(name)
            if d is None:
                raise KeyError("LevelBank.assign: %r is no parameter of the env's _gen_grid (declared: %s)"
                               % (name, ", ".join(sorted(env._params.decl)) or "none"))
            cols.append((d["col"], P.values(v, d["lo"], d["hi"], k, None, dev, "LevelBank.assign(%s=)" % name,
                                            "the parameter's interval [%d, %d)" % (d["lo"], d["hi"]), dtype=np.uint8, wide=False,
                                            clamp=True)))
        if edits is not None:
            if not self.K:
                raise ValueError("LevelBank.assign(edits=): the env was built without an edit table (level_edits=K)")
            edits = gen_edits.rows(edits, self.K, k, None, k, env.width, env.height, len(env.obj_reg.objs), dev, "LevelBank.assign")
        return cols, edits

    def _write_rows(self, at, rows):
        """the checked rows into slots `at` (an index array / tensor, or a slice)"""
        if rows is None:
            return
        cols, edits = rows
        for col, v in cols:
            self.params[at, col] = v
        if edits is not None:
            self.edits[at] = edits

    def _seed_rows(self, seeds, slots, mask, rows=None):
        """mg_level_seed — and the slots' rows — on torch's current stream of the bank's device, ordered against the streams
        that read the bank"""
        import torch
        with torch.cuda.device(self.device):
            def dev(v):
                if v is None:
                    return None
                v = v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))
                return v.to(device=self.device, dtype=torch.int64).contiguous()
            seeds, slots = dev(seeds), dev(slots)
            cur = torch.cuda.current_stream(self.device)
            others = [r for r in self._readers.values() if r != cur]
            for r in others:                        # rows an earlier step's launch still reads are not overwritten under it
                cur.wait_event(r.record_event())
            N.check(self._lib.mg_level_seed(int(seeds.shape[0]), seeds.data_ptr(), None if slots is None else slots.data_ptr(),
                                            None if mask is None else mask.data_ptr(), self.capacity, self.mt.data_ptr(),
                                            self.pos.data_ptr(), self.head.data_ptr(), self.seeds.data_ptr(), C.c_void_p(cur.cuda_stream)))
            self.launches += 1
            self._write_rows(slice(0, int(seeds.shape[0])) if slots is None else slots, rows)
            if others:
                ev = cur.record_event()
                for r in others:
                    r.wait_event(ev)

    def copy_rows(self, put):
        """`put(tensor)` for each of this bank's row tensors — seeds, generators, and a full bank's rows — on torch's current
        stream, ordered against the streams that read the bank as `_seed_rows` is (MultiGridEnv.fork, the seeds form)"""
        import torch
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            others = [r for r in self._readers.values() if r != cur]
            for r in others:
                cur.wait_event(r.record_event())
            for t in (self.seeds, self.mt, self.pos, self.head, self.params, self.edits):
                if t is not None:
                    put(t)
            if others:
                ev = cur.record_event()
                for r in others:
                    r.wait_event(ev)

    def replica(self, device, streams=()):
        """this bank's levels on `device`, for shards that live there and step on `streams`: seeded there from `seeds` (one
        launch, no generator crosses devices) and kept up to date by `assign`"""
        import torch
        device = torch.device(device)
        rep = self._replicas.get(device)
        if rep is None:
            rep = LevelBank(self.capacity, device, env=self._env)
            for s in streams:
                rep._readers[s.cuda_stream] = s
            with torch.cuda.device(device):
                whole = None
                if self.full:       # (the rows as they are now, every column: no default is put back)
                    whole = [(c, self.params[:, c].to(device)) for c in range(N.GEN_DRAWS)], self.edits.to(device)
                rep._seed_rows(self.seeds.to(device), None, None, whole)
            self._replicas[device] = rep
        for s in streams:
            rep._readers[s.cuda_stream] = s
        return rep


class EnvLevels(object):
    """The env side of replayable levels — `env._levels`; MultiGridEnv.set_levels, whose docstring is the contract, delegates
    here.  Nothing is allocated or launched until `set` is first called."""

    def __init__(self, env):
        self.env = env
        self.on = False             # set_levels was called: every reset and step is preceded by mg_level_apply
        self.launches = 0           # ... how many of them there were
        self.bank = self.own_bank = None    # the one bank the batch reads now; the env's own (the seeds form: row b is env b's)
        self.level_of_env = None    # (B,) int64: each env's slot of `bank`, -1: free-running

    def enable(self):
        """the tensors of set_levels, made at its first call: an env that never calls it allocates and launches nothing"""
        env = self.env
        if self.on:
            return
        if env.auto_reset_mode == "same_step":
            raise ValueError("set_levels: with auto_reset=True a same-step reset happens inside the launch that ends the episode, "
                             "where no level can be handed over; construct the env with auto_reset='next_step' (or False)")
        self.on = True
        if env._dry:
            self.level_of_env = np.full(env.batch_size, -1, np.int64)
            return
        import torch
        B, dev = env.batch_size, env.device
        self.level_of_env = torch.full((B,), -1, dtype=torch.int64, device=dev)
        for r in env._ring:
            r["level"] = torch.full((B,), -1, dtype=torch.int64, device=dev)
            if "info" in r:
                r["info"]["level"] = r["level"]

    def set(self, bank=None, ids=None, seeds=None, env_mask=None, env_ids=None):
        env, B = self.env, self.env.batch_size
        dev = None if env._dry else env.device
        if (bank is None) == (seeds is None) or (bank is not None and ids is None) or (seeds is not None and ids is not None):
            raise ValueError("set_levels: either (bank, ids) or seeds=")
        mask, eids = P.select(B, dev, env_mask, env_ids, "set_levels")
        self.enable()
        if bank is not None:
            if not isinstance(bank, LevelBank):
                raise ValueError("set_levels: bank must be a LevelBank")
            if dev is not None and bank.device != dev:
                raise ValueError("set_levels: the bank lives on %s, the env on %s (env.level_bank(...) makes one here)" % (bank.device, dev))
            if bank.full and (bank.K != env.level_edits or set(bank._env._params.decl) != set(env._params.decl)):
                raise ValueError("set_levels: the full bank was made from an env with other parameters or another level_edits "
                                 "(env.level_bank(..., full=True) makes one for this env)")
            v = P.values(ids, -1, bank.capacity, B, eids, dev, "set_levels(ids=)", "[-1, %d)" % bank.capacity)
        else:       # (device tensors pass: mg_level_seed guards the range)
            v = P.values(seeds, -1, None, B, eids, dev, "set_levels(seeds=)", "[-1, 2**63)")
            if self.own_bank is None:
                self.own_bank = env.level_bank(B)
            bank = self.own_bank
        if bank is not self.bank:
            if (mask is not None or eids is not None) and self.bank is not None:
                raise ValueError("set_levels: the envs of one batch read one bank at a time; change to another bank (or between a "
                                 "bank and seeds=) with a call for every env")
            self.bank = bank
            if bank is self.own_bank and dev is None:       # row b is env b's: whether it plays a level is whether its row is filled
                self.level_of_env[:] = np.arange(B)
                bank.seeds[:] = -1
            elif bank is self.own_bank:
                import torch
                torch.arange(B, out=self.level_of_env)
                bank.seeds.fill_(-1)
        if bank is self.own_bank and dev is not None:       # (the rows' generators are seeded with them: one launch)
            bank._readers.update(env._launch_streams)
            bank._seed_rows(v if v.ndim else v.expand(B if eids is None else eids.shape[0]).contiguous(), eids, mask)
        else:
            P.write(bank.seeds if bank is self.own_bank else self.level_of_env, v, mask, eids)

    def apply(self, rule, mask_ptr, stream):
        """mg_level_apply in front of a reset or a step: the envs the rule selects take their level's generator; every env's
        running level goes to the current buffer set.  Nothing unless set_levels was ever called."""
        env, bank = self.env, self.bank
        if not self.on or env._dry or bank is None:
            return
        bank._readers.update(env._launch_streams)
        head = (C.byref(env._cfg), C.byref(env._state), rule, mask_ptr, self.level_of_env.data_ptr(), bank.capacity,
                bank.mt.data_ptr(), bank.pos.data_ptr(), bank.head.data_ptr(), bank.seeds.data_ptr(), env.episode_level.data_ptr(),
                env._ring[env._ring_i]["level"].data_ptr())
        if bank.full:       # the slot's parameter row and edit rows go over the env's in the same launch (a part without a table: null)
            par, K = env.params_t is not None, env.level_edits
            N.check(env._lib.mg_level_apply_rows(*head, bank.params.data_ptr() if par else None, bank.edits.data_ptr() if K else None,
                                                 K, env.params_t.data_ptr() if par else None, env.edits_t.data_ptr() if K else None,
                                                 stream))
        else:
            N.check(env._lib.mg_level_apply(*head, stream))
        self.launches += 1

    def fork(self, put):
        """MultiGridEnv.fork: the `dst` envs take the running level and the NEXT level of their `src` envs — `put(tensor)`
        copies rows src -> dst of a (B, ...) tensor.  With a caller's bank the next level is a slot, and the slot is copied.  In
        the seeds form row b of the env's own bank is env b's and `level_of_env` stays `arange(B)`: the bank ROW is copied —
        seed and generator —, so that a later `set_levels(seeds=, env_ids=[dst])` still reaches the env it names, and
        re-seeding `src` leaves `dst` alone."""
        if not self.on:
            return
        put(self.env.episode_level)
        if self.bank is not None and self.bank is self.own_bank:
            self.bank._readers.update(self.env._launch_streams)
            self.bank.copy_rows(put)
        else:
            put(self.level_of_env)

    def next(self):
        """(B,) int64: the seed each env's next reset will use, resolved through the bank (-1: free-running)"""
        import torch
        bank, lv = self.bank, self.level_of_env
        if bank is None:
            return torch.full_like(lv, -1)
        ok = (lv >= 0) & (lv < bank.capacity)
        return torch.where(ok, bank.seeds[lv.clamp(0, bank.capacity - 1)], torch.full_like(lv, -1))
