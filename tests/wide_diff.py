"""TEST INFRASTRUCTURE — one differential driver for the wide tests: a *subject* (the HIP env, or the host build of the
step bodies) is stepped beside the CPU oracle with the same seeds and actions, and ALL envs are compared, never a sample.

  every step                       done (exact), rewards (|d| <= REW_TOL), with episode_info every info field and the return
                                   within REW_TOL * max(length, 1); in next-step mode the observation of every env whose
                                   episode ended in that step (the terminal observation)
  every obs_every-th and the last  the whole observation tensor, byte for byte; `grid_encoding` where the subject has
                                   encode_in_step
  every deep_every-th and the last canonical state of every env (grid, agent records incl. stack order, step counter), the
                                   RNG of every env in numpy's form, and the 16 look-ahead words of `mt_head`

Between two launches all MT_HEAD words of an env's head are unconsumed (mg_core.h: mt_finish / mt_finish_ring top the head up
again before the state is written back; the stream position is mt_pos - 16), so the whole head is compared with the next 16
outputs of the oracle's stream.  numpy's form only carries the head's LENGTH: a wrong word in the head is invisible to the
RNG comparison, and once it has been drawn it may leave no trace in the state at all (a shuffle of agents that never meet).
Only the head comparison sees it, and only while it is unconsumed: `deep_every` bounds what a wide test can promise about
the head — a word that is corrupted and consumed between two deep checks is caught only through what it did to the episode.

The first mismatch raises `Mismatch` (an AssertionError).  Its message localises: scenario, kernel, step, field, the COUNT of
differing envs, their indices as runs ("20480-20487, 31002": a wave of the obs kernel takes consecutive envs, so a wave- or
workgroup-shaped fault shows as runs of neighbours), and for the first few of them the steps since the env's last in-launch
reset and the RNG words it has drawn; for observations also the first differing agent and pixel / cell.  No tensors.

The state arrays are fetched with one device-to-host copy each per deep check and converted on the host:
`numpy_form_rows` is seeding.numpy_form for all rows at once (tests/test_wide_diff_host.py holds it to seeding.numpy_form,
row by row)."""
import ctypes as C
import time

import numpy as np

import canon
import product_envs
import scenarios
from marlgrid_amd import seeding
from oracle import oracle as O

REW_TOL = 1e-6          # per step: float32 output of a float64 sum (tests/test_core_hostemu.py)
MT_N, MT_HEAD = 624, 16
MAX_RUNS = 8
SHOWN = 4               # envs described one by one in a message
_CHUNK = 4096


class Mismatch(AssertionError):
    def __init__(self, message, scenario, kernel, step, field, envs):
        AssertionError.__init__(self, message)
        self.scenario, self.kernel, self.step, self.field = scenario, kernel, step, field
        self.envs = [int(b) for b in envs]


def runs(ids, max_runs=MAX_RUNS):
    """env indices as runs: {5, 6, 7, 8, 900} -> "5-8, 900"; more than `max_runs` runs are cut with "..." """
    ids = np.unique(np.asarray(ids, np.int64))
    if ids.size == 0:
        return ""
    cut = np.nonzero(np.diff(ids) != 1)[0] + 1
    lo = np.concatenate([[0], cut])
    hi = np.concatenate([cut, [ids.size]])
    parts = ["%d" % ids[s] if e - s == 1 else "%d-%d" % (ids[s], ids[e - 1]) for s, e in zip(lo, hi)]
    if len(parts) > max_runs:
        parts = parts[:max_runs] + ["..."]
    return ", ".join(parts)


# ---- the RNG, all rows at once ------------------------------------------------------------------------------------------
_UP, _LO, _MAG = np.uint32(0x80000000), np.uint32(0x7FFFFFFF), np.uint32(0x9908B0DF)


def _twist(hi, lo, m):
    y = (hi & _UP) | (lo & _LO)
    return m ^ (y >> np.uint32(1)) ^ np.where((y & np.uint32(1)) != 0, _MAG, np.uint32(0))


def numpy_form_rows(mt, gen_pos, head=MT_HEAD):
    """seeding.numpy_form for every row: mt (B, 624) uint32 (or int32 bits), gen_pos (B,) -> key (B, 624) uint32, pos (B,).
    The forward branch regenerates slots [G, 624): slot k reads the OLD k and k + 1 and slot k + 397 (mod 624), which for
    k >= 227 is the already regenerated slot k - 227 — three dependent chunks, then slot 623 (which reads the new slot 0)."""
    mt = np.ascontiguousarray(mt).view(np.uint32)
    G = np.asarray(gen_pos).astype(np.int64)
    out = mt.copy()
    fwd = G > head
    for lo, hi in ((0, 227), (227, 454), (454, 623)):
        k = np.arange(lo, hi)
        src = mt[:, lo + 397:hi + 397] if lo == 0 else out[:, lo - 227:hi - 227]
        new = _twist(mt[:, lo:hi], mt[:, lo + 1:hi + 1], src)
        m = fwd[:, None] & (k[None, :] >= G[:, None])
        out[:, lo:hi] = np.where(m, new, out[:, lo:hi])
    out[:, 623] = np.where(fwd, _twist(mt[:, 623], out[:, 0], out[:, 396]), out[:, 623])
    # position still in the previous block: wind the slots [0, G) back
    i = np.arange(head)
    t = mt[:, :head] ^ mt[:, 397:397 + head]
    ys = np.where((t & _UP) != 0, ((t ^ _MAG) << np.uint32(1)) | np.uint32(1), t << np.uint32(1)).astype(np.uint32)
    prev = np.concatenate([np.zeros((len(mt), 1), np.uint32), ys[:, :-1]], axis=1)
    val = (ys & _UP) | (prev & _LO)
    m = (~fwd)[:, None] & (i[None, :] < G[:, None])
    out[:, :head] = np.where(m, val, out[:, :head])
    return out, np.where(fwd, G - head, G - head + MT_N)


def stream_diff(key, pos, okey, opos):
    """seeding.same_stream for every row -> bool (B,), True where the two states are NOT the same stream"""
    return (pos != opos) | (key[:, 1:] != okey[:, 1:]).any(axis=1) | ((key[:, 0] >> np.uint32(31)) != (okey[:, 0] >> np.uint32(31)))


def _temper(v):
    v = v ^ (v >> np.uint32(11))
    v = v ^ ((v << np.uint32(7)) & np.uint32(0x9d2c5680))
    v = v ^ ((v << np.uint32(15)) & np.uint32(0xefc60000))
    return v ^ (v >> np.uint32(18))


def oracle_rng(envs):
    """(key (B, 624) uint32, pos (B,)) of the oracle's envs, and the next MT_HEAD uint32 outputs of each stream: the tempered
    key words where the block still holds 16 of them, numpy's own RandomState where the 16 run into the next block"""
    B = len(envs)
    key = np.zeros((B, MT_N), np.uint32)
    pos = np.zeros(B, np.int64)
    for b, e in enumerate(envs):
        key[b], pos[b] = e.mt_state()
    inside = pos + MT_HEAD <= MT_N
    at = np.where(inside, pos, 0)[:, None] + np.arange(MT_HEAD)[None, :]
    nxt = _temper(np.take_along_axis(key, at, axis=1))
    rs = np.random.RandomState()
    for b in np.nonzero(~inside)[0]:
        rs.set_state(("MT19937", key[b], int(pos[b]), 0, 0.0))
        nxt[b] = rs.randint(0, 2 ** 32, size=MT_HEAD, dtype=np.uint64).astype(np.uint32)
    return key, pos, nxt


# ---- observations -------------------------------------------------------------------------------------------------------
def diff_rows(got, want):
    """(B, ...) against (B, ...), same dtype -> bool (B,): rows that differ anywhere (in chunks, eight bytes at a time)"""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    B = got.shape[0]
    g, w = got.reshape(B, -1), want.reshape(B, -1)
    if g.dtype == np.uint8 and g.shape[1] % 8 == 0 and g.flags.c_contiguous and w.flags.c_contiguous:
        g, w = g.view(np.uint64), w.view(np.uint64)
    bad = np.zeros(B, bool)
    for s in range(0, B, _CHUNK):
        bad[s:s + _CHUNK] = (g[s:s + _CHUNK] != w[s:s + _CHUNK]).any(axis=1)
    return bad


_WHERE = {"obs": "agent %d, pixel (row %d, col %d, channel %d)", "views": "agent %d, cell (%d, %d), field %d",
          "encode": "cell (%d, %d), field %d"}


def compare_rows(got, want, kind, ids=None):
    """-> None when equal, else (differing env indices, "env b: <first differing agent and pixel / cell>: got x, want y").
    kind: "obs" (B, n, P, P, 3) pixels, "views" (B, n, V, V, 3) encoded views, "encode" (B, W, H, 3) grid.encode();
    ids: the env index of each row (default: the row number)"""
    bad = np.nonzero(diff_rows(got, want))[0]
    if bad.size == 0:
        return None
    r = int(bad[0])
    at = tuple(int(v) for v in np.argwhere(got[r] != want[r])[0])
    envs = bad if ids is None else np.asarray(ids)[bad]
    return envs, "env %d: %s: got %d, want %d" % (envs[0], _WHERE[kind] % at, got[r][at], want[r][at])


def render_pixels(envs, ids, out):
    """the oracle's gen_obs of envs[ids] into out (len(ids), n, P, P, 3) uint8"""
    L, n = envs[0].L, envs[0].n
    img = out.shape[2] * out.shape[3] * 3
    assert out.flags.c_contiguous and out.dtype == np.uint8 and out.shape[:2] == (len(ids), n)
    u8p, base = C.POINTER(C.c_uint8), out.ctypes.data
    for i, b in enumerate(ids):
        h = envs[b].h
        for k in range(n):
            L.mgo_render_obs(h, k, C.cast(base + (i * n + k) * img, u8p))
    return out


# ---- subjects -----------------------------------------------------------------------------------------------------------
class HipSubject(object):
    """the product env on the device"""
    has_obs = True

    def __init__(self, env):
        self.env, self.B, self.n = env, env.batch_size, env.num_agents
        self.kernel_name = env.kernel_name
        self.spec = env.scenario_spec()
        self.encode_in_step = bool(env.encode_in_step)
        self._host = None

    def reset(self, mask=None):
        import torch
        return self.env.reset() if mask is None else self.env.reset(env_mask=torch.from_numpy(np.asarray(mask, bool)))

    def step(self, a):
        import torch
        o, r, d, info = self.env.step(torch.from_numpy(a))
        return o, r.cpu().numpy(), d.cpu().numpy(), {k: v.cpu().numpy() for k, v in info.items()}

    def rows(self, obs, ids=None):
        """the observation tensor (or its rows `ids`) on the host; the whole tensor lands in a buffer that is reused"""
        import torch
        assert torch.is_tensor(obs), type(obs)
        if ids is not None:
            return obs[torch.as_tensor(np.asarray(ids, np.int64), device=obs.device)].cpu().numpy()
        if self._host is None or self._host.shape != obs.shape:
            try:
                self._host = torch.empty(obs.shape, dtype=obs.dtype, pin_memory=True)
            except RuntimeError:            # (page-locked memory is limited for this user: an ordinary buffer)
                self._host = torch.empty(obs.shape, dtype=obs.dtype)
        self._host.copy_(obs)
        return self._host.numpy()

    def mt_pos(self):
        return self.env.mt_pos.cpu().numpy()

    def state(self):
        e = self.env
        W, H = e.width, e.height
        return dict(grid=e.grid_state.cpu().numpy()[:, :W * H].reshape(self.B, W, H), rec=e.agent_state.cpu().numpy(),
                    step_count=e.step_count_t.cpu().numpy(), mt=e.mt_state.cpu().numpy().view(np.uint32),
                    mt_pos=e.mt_pos.cpu().numpy(), mt_head=e.mt_head.cpu().numpy().view(np.uint32))

    def grid_encoding(self):
        return self.env.grid_encoding.cpu().numpy()

    def check_errors(self):
        self.env.check_errors()

    def level_state(self):
        """what a level leaves in the env besides its generator (run(ref=...) with a reference that plays levels)"""
        e = self.env
        return dict(episode_level=e.episode_level.cpu().numpy(),
                    params=None if e.params_t is None else {k: v.cpu().numpy() for k, v in e.params.items()},
                    edits=None if e.edits_t is None else e.edits_t.cpu().numpy())


class HostEmuSubject(object):
    """tests/native/hostemu.py: the step bodies built for the host — numpy arrays, no observations"""
    has_obs = False
    encode_in_step = False
    kernel_name = "host build of the step bodies"

    def __init__(self, emu):
        self.emu, self.B, self.n = emu, emu.B, emu.n
        self.spec = emu.env.scenario_spec()

    def reset(self, mask=None):
        self.emu.reset(None if mask is None else np.asarray(mask, bool))
        return None

    def step(self, a):
        r, d = self.emu.step(a)
        return None, r, d, {}

    def mt_pos(self):
        return self.emu.mt_pos.copy()

    def state(self):
        e = self.emu
        W, H = e.env.width, e.env.height
        return dict(grid=e.grid[:, :W * H].reshape(self.B, W, H), rec=e.rec, step_count=e.step_count, mt=e.mt,
                    mt_pos=e.mt_pos, mt_head=e.mt_head)

    def check_errors(self):
        assert not self.emu.error.any(), np.nonzero(self.emu.error)[0][:8]


# ---- the oracle side ----------------------------------------------------------------------------------------------------
class _SameStepRef(object):
    """OracleBatch, reset on done inside the step"""

    def __init__(self, spec, seeds):
        self.orc = O.OracleBatch(spec, seeds)
        self.envs = self.orc.envs

    def reset(self):
        for e in self.envs:
            O._raise(e.L.mgo_reset(e.h, 1))

    def reset_envs(self, mask):
        for b in np.nonzero(mask)[0]:
            O._raise(self.envs[b].L.mgo_reset(self.envs[b].h, 1))

    def step(self, a, pixels):
        o, r, d, _ = self.orc.step(a, render=pixels, auto_reset=True, reuse_obs=True)
        return o, r, d, None


class _EpisodeRef(object):
    """tests/episode_ref.py: next-step reset and / or the expected info fields"""

    def __init__(self, spec, seeds, mode):
        import episode_ref
        self.ep = episode_ref.EpisodeOracle(spec, seeds, mode=mode, render=False)   # (the looks render into one buffer)
        self.envs = self.ep.envs

    def reset(self):
        self.ep.reset()

    def reset_envs(self, mask):
        self.ep.reset_envs(mask)

    def step(self, a, pixels):
        _, r, d, info = self.ep.step(a, render=False)
        return None, r, d, info


# ---- the driver ---------------------------------------------------------------------------------------------------------
def run(subject, name, seeds, T, obs_every=50, deep_every=500, action_seed=5, mode="same_step", episode_info=False,
        obs_format="image", stagger=False, after_step=None, spec=None, watch=None, between=None, ref=None):
    """Step `subject` and the oracle of `spec` (default: scenarios.registered(name)) for T steps (actions
    RandomState(action_seed).randint(0, 7)).
    watch(t, envs, mask): called with the ORACLE's envs after every reset on its side — t = 0: reset() (mask: everyone);
    after step t: the envs whose reset ran in that call (same-step mode: those that ended in it; next-step mode: those that had
    ended in the call before); after a staggered reset by hand.  What a test requires of its own coverage it reads there.
    between(t, subject, envs): called with the subject and the ORACLE's envs before the first reset (t = 0) and after step t and
    all of its checks — where a run calls `set_params` on both sides: a value takes effect at an env's next reset on either.
    A `between` that resets envs by hand on both sides returns True: the deep check then runs once more, on what the resets left.
    mode: the subject's auto-reset mode; stagger: during the first 100 steps env b is reset by hand after step b % 100 (0-based),
    subject and oracle; after_step(t, subject): called between two steps (fault injection in the driver's own tests).
    ref: the oracle side, in place of the driver's own — an object with `envs` (the list of OracleEnvs, looked at again at every
    check: it may swap them), reset(), reset_envs(mask), step(actions, pixels) -> (pixels or None, rewards, done, info or None),
    and optionally extra(subject) -> [(field, differing envs, detail)], asked after every step and reset (tests/level_ref.py:
    WideRef, whole levels).  An info field "level" is compared exactly where the reference returns one.
    -> dict(episodes (B,), draws (B,) RNG words drawn per env, blocks = draws / 624, partial_done_steps: steps on which some
    but not all envs ended, terminal_obs (B,): terminal observations compared per env, seconds: where the time went)"""
    B, n = subject.B, subject.n
    if spec is None:
        spec = scenarios.registered(name)
    use_ep = episode_info or mode == "next_step"
    if ref is None:
        ref = _EpisodeRef(spec, seeds, mode) if use_ep else _SameStepRef(spec, seeds)
    envs = ref.envs
    kind = "views" if obs_format == "encoded" else "obs"
    since = np.full(B, -1, np.int64)            # steps since the env's last in-launch reset (-1: none yet)
    draws = np.zeros(B, np.int64)
    episodes = np.zeros(B, np.int64)
    terminal_obs = np.zeros(B, np.int64)
    sec = dict(subject=0.0, oracle=0.0, fetch=0.0, render=0.0, compare=0.0, deep=0.0)
    clock = [time.time()]
    buf = [None]

    def lap(k):
        now = time.time()
        sec[k] += now - clock[0]
        clock[0] = now

    def fail(t, field, bad, detail=""):
        bad = np.unique(np.asarray(bad, np.int64))
        per = ["env %d: %s, %d RNG words drawn" % (b, "no in-launch reset yet" if since[b] < 0 else
                                                  "%d steps since its last in-launch reset" % since[b], draws[b])
               for b in bad[:SHOWN]]
        msg = "%s [%s] step %d: %s differs in %d of %d envs: %s\n  %s" % (name, subject.kernel_name, t, field, bad.size, B,
                                                                          runs(bad), "\n  ".join(per))
        if detail:
            msg += "\n  first: " + detail
        raise Mismatch(msg, name, subject.kernel_name, t, field, bad)

    def want_obs(ids=None):
        """the oracle's observations of the envs `ids` (all: into one reused buffer)"""
        sel = range(B) if ids is None else ids
        if kind == "views":
            import viewenc
            return viewenc.oracle_views_batch([envs[b] for b in sel])
        P = envs[0].P
        if ids is not None:
            return render_pixels(envs, sel, np.zeros((len(sel), n, P, P, 3), np.uint8))
        if buf[0] is None:
            buf[0] = np.zeros((B, n, P, P, 3), np.uint8)
        return render_pixels(envs, sel, buf[0])

    def check_obs(t, obs, want, ids=None, what=None):
        got = subject.rows(obs, ids)
        lap("fetch")
        if want is None:
            want = want_obs(ids)
            lap("render")
        out = compare_rows(got, want, kind, ids)
        lap("compare")
        if out is not None:
            fail(t, what or ("observations" if kind == "obs" else "encoded views"), out[0], out[1])

    def count_draws(last):
        pos = subject.mt_pos()
        draws[:] += (pos.astype(np.int64) - last) % MT_N       # mt_pos runs modulo 624; no step or reset draws 624 words
        return pos.astype(np.int64)

    def deep(t):
        subject.check_errors()
        st = subject.state()
        got = product_envs.canonical_arrays(subject.spec, st["grid"], st["rec"], st["step_count"])
        want = [canon.oracle_canonical(e) for e in envs]
        for k in canon.KEYS:
            g, w = np.stack([np.asarray(x[k]) for x in got]), np.stack([np.asarray(x[k]) for x in want])
            assert g.shape == w.shape, (k, g.shape, w.shape)
            bad = np.nonzero((g != w).reshape(B, -1).any(axis=1))[0]
            if bad.size:
                b = int(bad[0])
                at = tuple(int(v) for v in np.argwhere(g[b] != w[b])[0])
                fail(t, "canonical state, field %r" % k, bad,
                     "env %d at %s: got %s, want %s" % (b, at, np.asarray(g[b][at]).tolist(), np.asarray(w[b][at]).tolist()))
        okey, opos, onext = oracle_rng(envs)
        key, pos = numpy_form_rows(st["mt"], st["mt_pos"], MT_HEAD)
        for b in (0, B // 2, B - 1):            # (and the product's own conversion, on three rows)
            assert seeding.same_stream(seeding.numpy_form(st["mt"][b], st["mt_pos"][b], MT_HEAD), (key[b], pos[b])), b
        d = stream_diff(key, pos, okey, opos)
        if d.any():
            b = int(np.nonzero(d)[0][0])
            w = np.nonzero(key[b, 1:] != okey[b, 1:])[0]
            fail(t, "RNG state (numpy form)", np.nonzero(d)[0], "env %d: position %d, want %d; %d of 624 words differ%s" % (
                b, pos[b], opos[b], w.size + int((key[b, 0] >> 31) != (okey[b, 0] >> 31)),
                ", the first at index %d" % (w[0] + 1) if w.size else ""))
        head = np.ascontiguousarray(st["mt_head"]).view(np.uint32)
        d = (head != onext).any(axis=1)
        if d.any():
            b = int(np.nonzero(d)[0][0])
            j = int(np.nonzero(head[b] != onext[b])[0][0])
            fail(t, "mt_head (the 16 look-ahead RNG outputs)", np.nonzero(d)[0],
                 "env %d: entry %d is %#010x, the stream's next output there is %#010x" % (b, j, head[b, j], onext[b, j]))
        lap("deep")

    def check_extra(t):
        if hasattr(ref, "extra"):
            for field, bad, detail in ref.extra(subject):
                fail(t, field, bad, detail)

    # -- the constructor's reset has run on both sides; one reset() more, as every caller of the env does
    if between is not None:
        between(0, subject, envs)
    obs = subject.reset()
    ref.reset()
    last_pos = subject.mt_pos().astype(np.int64)
    if watch is not None:
        watch(0, envs, np.ones(B, bool))
    prev_done = np.zeros(B, bool)
    if subject.has_obs:
        check_obs(0, obs, None, what="observations of reset()")
    check_extra(0)
    rng = np.random.RandomState(action_seed)
    partial = 0
    clock[0] = time.time()
    for t in range(1, T + 1):
        a = rng.randint(0, 7, size=(B, n))
        look = t % obs_every == 0 or t == T
        obs, r, d, info = subject.step(a)
        lap("subject")
        pixels, r2, d2, want_info = ref.step(a, look and subject.has_obs and kind == "obs")
        lap("oracle")
        if watch is not None:
            watch(t, envs, prev_done if mode == "next_step" else d2)
            prev_done = d2.copy()
        last_pos = count_draws(last_pos)
        bad = np.asarray(d, bool) != d2
        if bad.any():
            fail(t, "done", np.nonzero(bad)[0])
        bad = ~(np.abs(np.asarray(r, np.float64) - r2) <= REW_TOL).all(axis=1)
        if bad.any():
            b = int(np.nonzero(bad)[0][0])
            fail(t, "rewards", np.nonzero(bad)[0], "env %d: got %s, want %s" % (b, np.asarray(r)[b].tolist(), r2[b].tolist()))
        if episode_info:
            assert set(info.keys()) == set(want_info.keys()), sorted(info.keys())
            for k in ("terminated", "truncated", "reset"):          # episode_ref.assert_info, env by env
                bad = np.asarray(info[k], bool) != want_info[k]
                if bad.any():
                    fail(t, "info[%r]" % k, np.nonzero(bad)[0])
            bad = np.asarray(info["episode_length"]).astype(np.int64) != want_info["episode_length"].astype(np.int64)
            if bad.any():
                fail(t, "info['episode_length']", np.nonzero(bad)[0])
            tol = REW_TOL * np.maximum(want_info["episode_length"], 1)[:, None]
            bad = ~(np.abs(info["episode_return"] - want_info["episode_return"]) <= tol).all(axis=1)
            if bad.any():
                fail(t, "info['episode_return']", np.nonzero(bad)[0])
            if "level" in want_info:
                bad = np.asarray(info["level"]).astype(np.int64) != want_info["level"]
                if bad.any():
                    b = int(np.nonzero(bad)[0][0])
                    fail(t, "info['level']", np.nonzero(bad)[0], "env %d: got %d, want %d" % (b, info["level"][b], want_info["level"][b]))
        check_extra(t)
        lap("compare")
        if subject.has_obs:
            if look:
                check_obs(t, obs, pixels)
                if subject.encode_in_step:
                    got = subject.grid_encoding()
                    want = np.stack([e.encode() for e in envs])
                    out = compare_rows(got, want, "encode")
                    if out is not None:
                        fail(t, "grid_encoding", out[0], out[1])
                    lap("compare")
            elif mode == "next_step" and d2.any():          # the terminal observations of this step, every one
                check_obs(t, obs, None, ids=np.nonzero(d2)[0], what="terminal observations")
            if mode == "next_step":
                terminal_obs += d2
        episodes += d2
        partial += int(d2.any() and not d2.all())
        since[:] = np.where(d2, 0, np.where(since >= 0, since + 1, -1))
        if t % deep_every == 0 or t == T:
            deep(t)
        if stagger and t <= 100:
            mask = (np.arange(B) % 100) == t - 1
            obs = subject.reset(mask)
            ref.reset_envs(mask)
            if watch is not None:
                watch(t, envs, mask)
                prev_done &= ~mask
            last_pos = count_draws(last_pos)
            if subject.has_obs and mask.any():
                check_obs(t, obs, None, ids=np.nonzero(mask)[0], what="observations of reset(env_mask)")
            check_extra(t)
        if after_step is not None:
            after_step(t, subject)
            clock[0] = time.time()
        if between is not None:
            if between(t, subject, envs) is True:       # (it reset envs by hand, on both sides: their state and RNG now)
                last_pos = subject.mt_pos().astype(np.int64)
                deep(t)
            clock[0] = time.time()
    subject.check_errors()
    return dict(episodes=episodes, draws=draws, blocks=draws / float(MT_N), partial_done_steps=partial,
                terminal_obs=terminal_obs, seconds={k: round(v, 2) for k, v in sec.items()})


# ---- the wide cases (tests/test_hip_wide.py): the shapes bench.py runs ----------------------------------------------------
HEADLINE = "MarlGrid-3AgentCluttered15x15-v0"
SEED0 = 424200
# id -> (scenario, B, steps, obs_every, constructor keywords beside auto_reset, stagger, kernel): `kernel` is env.kernel_name,
# the instantiation the launcher names for that shape and bench.py reports (tests/test_wide_diff_host.py reads the render
# kernels off dry envs; the GPU tests confirm each on the device)
WIDE_CASES = {
    "W1": (HEADLINE, 32768, 6000, 50, {}, False, "mg::render_kernel<7, 8, 16, 0, 0>"),
    "W2": (HEADLINE, 32768, 2000, 50, {"encode_in_step": True}, False, "mg::render_kernel<7, 8, 16, 0, 0>"),
    "W3": (HEADLINE, 32768, 2000, 50, {}, True, "mg::render_kernel<7, 8, 16, 0, 0>"),
    "W4": ("MarlGrid-3AgentCluttered11x11-v0", 4096, 6000, 50, {}, False, "mg::render_kernel<7, 8, 16, 0, 0>"),
    "W5": ("MarlGrid-4AgentEmpty9x9-v0", 65536, 1000, 100, {}, False, "mg::render_kernel<7, 8, 16, 0, 0>"),
    "W6": ("Custom-8AgentCluttered30x30", 16384, 2000, 100, {}, False, "mg::render_kernel<9, 8, 16, 0, 0>"),
    "W7": (HEADLINE, 32768, 2000, 100, {"obs_format": "encoded"}, False, "mg::encode_views_kernel<7>"),
    "W8": (HEADLINE, 32768, 1000, 50, {"auto_reset": "next_step", "episode_info": True}, True, "mg::render_kernel<7, 8, 16, 0, 0>"),
}
DEEP_EVERY = 500


def build_case(case, **more):
    """the env of a wide case, built the way bench.py builds its env: make(name, batch_size, seeds, auto_reset=True) and
    everything else at its default (strict=True included)"""
    name, B, T, obs_every, kw, stagger, kernel = WIDE_CASES[case]
    kw = dict({"auto_reset": True}, **kw)
    kw.update(more)
    return product_envs.build(name, batch_size=B, seeds=SEED0 + np.arange(B), **kw)


def run_case(case):
    """-> (env, what `run` returns)"""
    name, B, T, obs_every, kw, stagger, kernel = WIDE_CASES[case]
    env = build_case(case)
    assert env.kernel_name == kernel, (case, env.kernel_name)
    assert env.strict is True
    mode = "next_step" if kw.get("auto_reset") == "next_step" else "same_step"
    out = run(HipSubject(env), name, SEED0 + np.arange(B), T, obs_every=obs_every, deep_every=DEEP_EVERY, mode=mode,
              episode_info=bool(kw.get("episode_info")), obs_format=kw.get("obs_format", "image"), stagger=stagger)
    assert env.kernel_name == kernel, (case, env.kernel_name)
    return env, out
