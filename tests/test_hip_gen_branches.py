"""GPU (-m gpu): `_gen_grid` that branches on random draws — a reset program with GUARDED ops (MgGenOp.obj, MG_GEN_GUARD),
replayed per env by `reset_env` inside every kernel that resets: mg_reset, the step kernel, the encoded-views kernel, the fused
render kernels and a kernel compiled at run time — against the reference's own trajectories (tests/golden/genbranch_*.npz)
and against the same `reset_env` text run on the host (tests/native).  Modelled on tests/test_hip_gen_draws.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import draw_envs as D  # noqa: E402
import gen_branch_envs as G  # noqa: E402
import wide_diff  # noqa: E402
from golden import refstate  # noqa: E402
from marlgrid_amd import seeding  # noqa: E402

pytestmark = pytest.mark.gpu
DOOR, KEY, WALL, GOAL = 11, 9, 8, 4         # type indices of MultiGrid.encode (the reference's)
REW_TOL = 1e-6

PATHS = {"fused": {}, "two_launches": dict(fused_step=False), "encoded": dict(obs_format="encoded"),
         "encode_in_step": dict(encode_in_step=True)}
MODES = {"reset": False, "auto": True, "next_step": "next_step"}


def _run_vs_golden(name, path, mode, rows=None):
    """test_hip_gen_draws.py:_run_vs_golden on the genbranch_* fixtures: env b follows golden row rows[b] with its own time index.
    Full observations where the scenario's pixels are pinned (crc of every env's, the first row's byte for byte), else
    `grid_encoding` / MultiGrid.encode of every env and, on the encoded path, the encoded views."""
    import torch
    G.register()
    g = G.golden(name)
    S, T, n = g["actions"].shape
    rows = np.arange(S) if rows is None else np.asarray(rows)
    B = len(rows)
    pixels = G.SCENARIOS[name][6] and "obs_format" not in PATHS[path]
    encoded = "obs_format" in PATHS[path]
    env = G.build(name, batch_size=B, seeds=g["seeds"][rows], place_obs=False, auto_reset=MODES[mode], **PATHS[path])
    vs = int(g["venc_steps"][1] - g["venc_steps"][0])

    def rng(b):
        return D.rng_digest(env.numpy_rng_state(b))

    def check_obs(obs, b, prefix, t, what):
        o = obs[b].cpu().numpy()
        if pixels:
            want_crc = g["obs_crc_" + prefix][rows[b]] if t is None else g["obs_crc"][rows[b], t]
            assert [refstate.crc(x) for x in o] == list(want_crc), what
            if rows[b] == 0 and prefix != "ctor":
                assert np.array_equal(o, g["obs_reset_full"][0] if t is None else g["obs_full"][0, t]), what
        if encoded and (t is None or t % vs == 0):
            for k in range(n):
                want = g["venc_%s_a%d" % (prefix, k)][rows[b]] if t is None else g["venc_step_a%d" % k][rows[b], t // vs]
                assert np.array_equal(o[k], want), (what, k)

    spec, W, H = env.scenario_spec(), env.width, env.height
    everyone = np.ones(B, bool)

    def canonical():
        return D.canonical_batch(spec, env.grid_state[:, :W * H].reshape(B, W, H).cpu().numpy(), env.agent_state.cpu().numpy())
    obs = env.gen_obs()
    D.cmp_canon_batch(canonical(), g, "ctor_", rows, None, everyone, "%s ctor" % name)
    for b in range(B):
        assert rng(b) == g["rng_ctor"][rows[b]]
        check_obs(obs, b, "ctor", None, "ctor env %d" % b)
    obs = env.reset()
    D.cmp_canon_batch(canonical(), g, "reset_", rows, None, everyone, "%s reset" % name)
    for b in range(B):
        assert rng(b) == g["rng_reset"][rows[b]]
        check_obs(obs, b, "reset", None, "reset env %d" % b)
    tp = np.zeros(B, np.int64)              # the golden step each env does next
    pending = np.zeros(B, bool)             # next_step: the env's next call is its reset
    while (tp < T).any():
        live = (tp < T) & ~pending
        a = np.where(live[:, None], g["actions"][rows, np.minimum(tp, T - 1)], 0).astype(np.int64)
        obs, r, dn, _ = env.step(torch.from_numpy(a))
        r, dn = r.cpu().numpy(), dn.cpu().numpy().astype(bool)
        st = canonical()
        same_state = live & ~(dn & (mode == "auto"))        # (auto: a step with done shows the new episode)
        D.cmp_canon_batch(st, g, "step_", rows, np.minimum(tp, T - 1), same_state, "%s/%s/%s call %d" % (name, path, mode, int(tp.max())))
        enc = (env.grid_encoding if "encode_in_step" in PATHS[path] else env.grid.encode()).cpu().numpy()
        manual = np.zeros(B, bool)
        for b in range(B):
            row, t = rows[b], int(tp[b])
            what = "%s/%s/%s env %d golden step %d" % (name, path, mode, b, t)
            if pending[b]:                  # the reset call of the episode that ended at step t - 1
                assert not dn[b] and not r[b].any(), what
                assert rng(b) == g["rng_next"][row, t - 1], what
                pending[b] = False
                continue
            if t >= T:
                continue
            assert np.abs(r[b].astype(np.float64) - g["rewards"][row, t]).max() <= REW_TOL, what
            assert bool(dn[b]) == bool(g["ep_done"][row, t]), what
            if dn[b] and mode == "auto":
                assert rng(b) == g["rng_next"][row, t], what
            else:
                assert np.array_equal(enc[b], g["encode"][row, t]), what
                if dn[b]:
                    assert rng(b) == g["rng_step"][row, t], what
                check_obs(obs, b, "step", t, what)
            if dn[b] and mode == "reset":
                manual[b] = True
            if dn[b] and mode == "next_step":
                pending[b] = True
            tp[b] += 1
        if manual.any():
            env.reset(env_mask=torch.from_numpy(manual))
            for b in np.nonzero(manual)[0]:
                assert rng(b) == g["rng_next"][rows[b], tp[b] - 1]
    if mode == "reset":
        for b in range(B):                      # every env's end state by its digest, the first seeds' word for word
            assert rng(b) == g["rng_next"][rows[b], T - 1]
            if rows[b] < len(g["mt_final"]):
                assert seeding.same_stream(env.numpy_rng_state(b), (g["mt_final"][rows[b]], g["mt_final_pos"][rows[b]]))
    env.check_errors()


# B1: every golden but the long program, on every launch path, under every reset mode
B1 = [(name, path, mode) for name in sorted(G.SCENARIOS) if name != "Branch-2AgentLong12" for path in PATHS for mode in MODES]


@pytest.mark.parametrize("name,path,mode", B1, ids=["%s-%s-%s" % c for c in B1])
def test_goldens(name, path, mode):
    _run_vs_golden(name, path, mode)


# B2: guarded ops beyond the LDS copy of the program's first 32 — B = 19: the 16 golden seeds and three of them again
@pytest.mark.parametrize("mode", ["reset", "auto"])
def test_long_program(mode):
    _run_vs_golden("Branch-2AgentLong12", "fused", mode, rows=list(range(16)) + [0, 5, 15])


# B3: launch geometry
@pytest.mark.parametrize("B", [67, 4099])
def test_launch_geometry_vs_host_emulation(B):
    """Sides 9 x 9 with max_steps=10, 35 steps: every env resets inside the launch at least three times.  B = 67: 4-wave
    workgroups with a partial last batch; B = 4099: 16-wave workgroups, batches of 8, a partial last batch.  Every env's grid
    bytes, step count, canonical state, RNG position and look-ahead words equal the host emulation's after the reset and after
    steps 10, 20, 35, and every path is seen after an in-launch reset on the emulation's side."""
    import hostemu
    import torch
    G.register()
    name, W, H = "Branch-2AgentSides9", 9, 9
    seeds = 9300 + np.arange(B)
    env = G.build(name, batch_size=B, seeds=seeds, place_obs=False, auto_reset=True, max_steps=10)
    emu = hostemu.HostEmu(name, B, seeds, auto_reset=True, par=True, max_steps=10)
    from marlgrid_amd.objects import Wall
    wall = env.obj_reg.find(Wall())
    spec = env.scenario_spec()

    def check(what):
        grid = env.grid_state.cpu().numpy()
        assert np.array_equal(grid, emu.grid), what
        assert np.array_equal(env.step_count.cpu().numpy(), emu.step_count), what
        got = D.canonical_batch(spec, grid[:, :W * H].reshape(B, W, H), env.agent_state.cpu().numpy())
        want = D.canonical_batch(spec, emu.grid[:, :W * H].reshape(B, W, H), emu.rec)
        for k in D.CANON_KEYS:
            bad = np.nonzero((got[k] != want[k]).reshape(B, -1).any(axis=1))[0]
            assert bad.size == 0, (what, k, bad[:8].tolist())
        key, pos = wide_diff.numpy_form_rows(env.mt_state.cpu().numpy(), env.mt_pos.cpu().numpy())
        bad = np.nonzero(wide_diff.stream_diff(key, pos, *wide_diff.numpy_form_rows(emu.mt, emu.mt_pos)))[0]
        assert bad.size == 0, (what, "rng", bad[:8].tolist())
        assert np.array_equal(env.mt_head.cpu().numpy().view(np.uint32), emu.mt_head), what      # the look-ahead words
        for b in (0, B - 1):
            assert seeding.same_stream(env.numpy_rng_state(b), emu.numpy_rng_state(b)), (what, b)
        assert not grid[:, W * H:].any(), what
        return G.sides_path(emu.grid[:, :W * H].reshape(B, W, H), wall)
    env.reset()
    emu.reset()
    check("reset")
    rng = np.random.RandomState(31)
    ends = np.zeros(B, np.int64)
    seen = set()
    for t in range(1, 36):
        a = rng.randint(0, 7, size=(B, 2))
        _, r, d, _ = env.step(torch.from_numpy(a))
        r2, d2 = emu.step(a)
        assert np.array_equal(d.cpu().numpy().astype(bool), d2) and np.abs(r.cpu().numpy() - r2).max() <= REW_TOL, t
        ends += d2
        if d2.any():                        # the layouts these envs drew inside the launch
            seen |= set(G.sides_path(emu.grid[d2, :W * H].reshape(-1, W, H), wall).tolist())
        if t in (10, 20, 35):
            check("step %d" % t)
    assert ends.min() >= 3
    assert seen == set(range(len(G.paths("sides", W))))
    env.check_errors()
    assert not emu.error.any()


# B4: split invariance
def test_shards_pipeline_and_checkpoint_equal_the_one_env():
    import torch
    from marlgrid_amd import envs as E
    G.register()
    name, B = "Branch-2AgentSides9", 24
    kw = dict(batch_size=B, seed=8800, place_obs=False, auto_reset=True, max_steps=10)
    one = E.make(name, **kw)
    ds = E.make(name, devices=[0, 0], **kw)
    pipe = E.make(name, pipeline=2, **kw)
    o = one.reset()
    assert torch.equal(ds.gather(ds.reset()), o)
    po = pipe.reset()
    pipe.synchronize()
    assert torch.equal(torch.cat(po), o)
    rng = np.random.RandomState(41)
    resumed = None
    for t in range(30):
        a = rng.randint(0, 7, size=(B, 2))
        at = torch.from_numpy(a)
        o, r, d, _ = one.step(at)
        o2, r2, d2, _ = ds.gather(ds.step(a))
        assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2), t
        for k in range(2):
            with pipe.on(k):
                part = slice(k * B // 2, (k + 1) * B // 2)
                o3, r3, d3, _ = pipe.step_part(k, at[part].to(one.device))
                torch.cuda.current_stream().synchronize()
                assert torch.equal(o3, o[part]) and torch.equal(r3, r[part]) and torch.equal(d3, d[part]), (t, k)
        if resumed is not None:
            o4, r4, d4, _ = resumed.step(at)
            assert torch.equal(o4, o) and torch.equal(r4, r) and torch.equal(d4, d), t
        if t == 14:                     # mid-episode (max_steps=10: step 5 of the second episode)
            resumed = E.make(name, **dict(kw, seed=1))
            resumed.reset()
            resumed.load_state_dict(one.state_dict())
    for k in one._STATE_KEYS:
        assert torch.equal(getattr(one, k), getattr(resumed, k)), k
    one.check_errors(), resumed.check_errors(), pipe.check_errors()
    for e in ds.envs:
        e.check_errors()


# B5: a kernel compiled at run time runs the same guarded program
def test_specialized_kernel_equals_the_tables(tmp_path):
    import torch
    B = 16
    seeds = 8700 + np.arange(B)
    kw = dict(batch_size=B, seeds=seeds, place_obs=False, auto_reset=True)       # (max_steps=10: _factory's sixth argument)
    env = G._factory("sides", 9, 9, 11, 8, 10, specialize="auto", specialize_cache=str(tmp_path), **kw)
    twin = G._factory("sides", 9, 9, 11, 8, 10, **kw)
    # as in test_hip_specialize.py: where the GPU tests run, libhiprtc loads — "auto" falling back to the table's kernel for
    # whatever reason fails here, it does not skip
    assert env.kernel_name.startswith("mg::render_kernel<11, 8, ") and twin.kernel_name.startswith("mg::render_kernel<0, 8, ")
    assert torch.equal(env.reset(), twin.reset())
    rng = np.random.RandomState(43)
    ends = 0
    for t in range(30):
        a = torch.from_numpy(rng.randint(0, 7, size=(B, 2)))
        o, r, d, _ = env.step(a)
        o2, r2, d2, _ = twin.step(a)
        assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2), t
        ends += int(d.sum())
    assert ends >= 3 * B
    for k in env._STATE_KEYS:
        assert torch.equal(getattr(env, k), getattr(twin, k)), k
    env.check_errors()


# B6: the shipped id
def test_make_builds_the_colored_doorkey_id():
    import torch
    from marlgrid_amd import envs as E
    env_id, size, B = "MarlGrid-2AgentColoredDoorKey8x8-v0", 8, 32
    assert env_id in E.extension_envs and env_id not in E.registered_envs
    env = E.make(env_id, batch_size=B, seed=77, place_obs=False, auto_reset=True, max_steps=6)
    assert isinstance(env, E.ColoredDoorKeyEnv) and (env.width, env.height, len(env.agents)) == (size, size, 2)
    env.reset()
    rng = np.random.RandomState(45)
    colors = set()
    for t in range(13):                     # two in-launch resets of every env
        st = D.canonical_batch(env.scenario_spec(), env.grid_state[:, :size * size].reshape(B, size, size).cpu().numpy(),
                               env.agent_state.cpu().numpy())
        kind, color = st["base_enc"][..., 0], st["base_enc"][..., 1]        # (B, W, H) type and colour indices of the cells' objects
        door, key, goal, wall = (kind == DOOR), (kind == KEY), (kind == GOAL), (kind == WALL)
        assert (door.reshape(B, -1).sum(axis=1) == 1).all() and (goal[:, size - 2, size - 2]).all(), t
        dx = door.any(axis=2).argmax(axis=1)
        assert ((dx >= 2) & (dx <= size - 3)).all() and (wall[np.arange(B), dx].sum(axis=1) == size - 1).all(), t
        carried = st["carry_enc"][..., 0] == KEY
        on_grid = key.reshape(B, -1).sum(axis=1)
        assert (on_grid + carried.sum(axis=1) == 1).all(), t
        door_color = (color * door).reshape(B, -1).max(axis=1)
        key_color = np.maximum((color * key).reshape(B, -1).max(axis=1), (st["carry_enc"][..., 1] * carried).max(axis=1))
        assert (door_color == key_color).all(), t                           # the door and its key share the colour
        colors |= set(door_color.tolist())
        env.step(torch.from_numpy(rng.randint(0, 7, size=(B, 2))))
    from marlgrid_amd.objects import COLOR_TO_IDX
    assert len(colors) > 1 and colors <= {COLOR_TO_IDX[c] for c in E.ColoredDoorKeyEnv.door_colors}
    env.check_errors()
