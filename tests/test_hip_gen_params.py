"""GPU (-m gpu): per-env `_gen_grid` parameters — a PARAM op loads a draw register from the env's row of the table behind the
program's template, a placement's count may be `const +- draw[r]` — replayed by `reset_env` inside every kernel that resets:
mg_reset, the step kernel, the encoded-views kernel, the fused render kernels and a kernel compiled at run time.  The
yardstick is the constant TWIN (tests/param_envs.py): the same `_gen_grid` with the value as a Python constant and the same
seeds; tests/test_gen_params_diff_host.py closes twin == oracle on the CPU.  No test writes an out-of-range table here.

The constructor's reset of a parameter env runs with the defaults and draws other RNG words than a twin's: both sides are
seeded again (`env.seed()`) once the values are set, then reset."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import draw_envs as D  # noqa: E402
import param_envs as PE  # noqa: E402
import wide_diff  # noqa: E402
from marlgrid_amd import seeding  # noqa: E402

pytestmark = pytest.mark.gpu
REW_TOL = 1e-6

PATHS = {"fused": {}, "two_launches": dict(fused_step=False), "encoded": dict(obs_format="encoded"),
         "encode_in_step": dict(encode_in_step=True)}
MODES = {"reset": False, "auto": True, "next_step": "next_step"}


def _started(env, **params):
    """values set, seeded as the constructor seeded it, reset"""
    if params:
        env.set_params(**params)
    env.seed()
    return env.reset()


# P1: every scenario against its twins, on every launch path, under every reset mode
P1 = [(kind, path, mode) for kind in sorted(PE.KINDS) for path in PATHS for mode in MODES]


@pytest.mark.parametrize("kind,path,mode", P1, ids=["%s-%s-%s" % c for c in P1])
def test_mixed_batch_equals_the_twins(kind, path, mode):
    import torch
    B, T = 48, 30
    pname = PE.KINDS[kind][2]
    lo, hi = PE.interval(kind)
    vals = PE.values(kind, B)
    seeds = 7100 + np.arange(B)
    # (strict=False: an error of the reference's would be recorded per env and compared like the rest)
    kw = dict(batch_size=B, seeds=seeds, place_obs=False, auto_reset=MODES[mode], max_steps=10, strict=False, **PATHS[path])
    env = PE.build(kind, **kw)
    rows = {v: torch.from_numpy(np.nonzero(vals == v)[0]).to(env.device) for v in range(lo, hi)}
    assert all(len(r) for r in rows.values())
    obs = _started(env, **{pname: vals})
    twins = {v: PE.build(kind, v, **kw) for v in range(lo, hi)}
    for v, t in twins.items():
        assert torch.equal(_started(t)[rows[v]], obs[rows[v]]), (v, "reset")
    rng = np.random.RandomState(17)
    ends = 0
    for step in range(T):
        a = torch.from_numpy(rng.randint(0, 7, size=(B, 2))).to(env.device)
        obs, r, d, _ = env.step(a)
        ends += int(d.sum())
        out = [(t.step(a)) for t in twins.values()]
        for (v, t), (o2, r2, d2, _) in zip(twins.items(), out):
            i = rows[v]
            assert torch.equal(obs[i], o2[i]) and torch.equal(d[i], d2[i]), (v, step)
            assert float((r[i] - r2[i]).abs().max()) <= REW_TOL, (v, step)
        if mode == "reset" and bool(d.any()):
            m = d.clone()
            obs = env.reset(env_mask=m)
            for v, t in twins.items():
                assert torch.equal(t.reset(env_mask=m)[rows[v]], obs[rows[v]]), (v, step, "reset(env_mask=)")
    assert ends >= 2 * B
    for v, t in twins.items():
        for k in env._STATE_KEYS:
            assert torch.equal(getattr(env, k)[rows[v]], getattr(t, k)[rows[v]]), (v, k)
    assert not env.grid_state[:, env.width * env.height:].any()


# P2: launch geometry against the host emulation
@pytest.mark.parametrize("B", [67, 4099])
def test_launch_geometry_vs_host_emulation(B):
    """`long` (12 x 12: the PARAM op and the guarded symbolic-count ops lie behind the LDS copy's 32) with max_steps=10, 35
    steps.  B = 67: 4-wave workgroups with a partial last batch; B = 4099: 16-wave workgroups, batches of 8, a partial last
    batch.  Grid bytes, canonical state, RNG position and look-ahead words equal the host emulation's after the reset and
    after steps 10, 20, 35, and every value is seen after an in-launch reset."""
    import hostemu_params
    import torch
    PE.register()
    kind, pname = "long", "n"
    W, H = PE.KINDS[kind][:2]
    seeds = 9400 + np.arange(B)
    vals = PE.values(kind, B)
    env = PE.build(kind, batch_size=B, seeds=seeds, place_obs=False, auto_reset=True, max_steps=10)
    emu = hostemu_params.ParamEmu(PE.name_of(kind), B, seeds, auto_reset=True, par=True, max_steps=10)
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
    _started(env, **{pname: vals})
    emu.set_params(**{pname: vals})
    emu.reseed()
    emu.reset()
    check("reset")
    rng = np.random.RandomState(33)
    ends = np.zeros(B, np.int64)
    seen = set()
    for t in range(1, 36):
        a = rng.randint(0, 7, size=(B, 2))
        _, r, d, _ = env.step(torch.from_numpy(a))
        r2, d2 = emu.step(a)
        assert np.array_equal(d.cpu().numpy().astype(bool), d2) and np.abs(r.cpu().numpy() - r2).max() <= REW_TOL, t
        ends += d2
        seen |= set(vals[d2].tolist())
        if t in (10, 20, 35):
            check("step %d" % t)
    assert ends.min() >= 3
    assert seen == set(range(*PE.interval(kind)))
    env.check_errors()
    assert not emu.error.any()


# P3: the shipped id
def test_curriculum_id_wall_counts_follow_the_table():
    import torch
    from marlgrid_amd import envs as E
    from marlgrid_amd.objects import Wall
    env_id, S, B = "MarlGrid-3AgentClutteredCurriculum15x15-v0", 15, 64
    assert env_id in E.extension_envs and env_id not in E.registered_envs
    kw = dict(batch_size=B, seed=4100, place_obs=False, auto_reset=True, max_steps=6)
    env = E.make(env_id, obs_delta=True, **kw)
    plain = E.make(env_id, obs_delta=False, **kw)
    assert isinstance(env, E.ClutteredMultiGrid) and env.params["n_clutter"].tolist() == [25] * B
    wall = env.obj_reg.find(Wall())

    def walls():
        g = env.grid_state[:, :S * S].reshape(B, S, S)[:, 1:S - 1, 1:S - 1]
        return (g == wall).sum(dim=(1, 2)).cpu().numpy()
    first = np.arange(B) % 51                               # 0 .. 50: the whole interval
    for e in (env, plain):
        e.set_params(n_clutter=first)
    assert torch.equal(env.reset(), plain.reset())
    current = first.copy()
    assert np.array_equal(walls(), current)
    rng = np.random.RandomState(19)
    later = (first * 7 + 3) % 51
    for t in range(20):                                     # three in-launch resets of every env
        if t == 3:                                          # mid-episode: the grid is left alone ...
            before = env.grid_state.clone()
            for e in (env, plain):
                e.set_params(n_clutter=torch.from_numpy(later).to(e.device))     # (a device tensor: clamped in stream order)
            assert torch.equal(env.grid_state, before)
            assert env.params["n_clutter"].cpu().numpy().tolist() == later.tolist()
        a = torch.from_numpy(rng.randint(0, 7, size=(B, 3)))
        o, r, d, _ = env.step(a)
        o2, r2, d2, _ = plain.step(a)
        assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2), t
        dn = d.cpu().numpy().astype(bool)
        current[dn] = (first if t < 3 else later)[dn]       # ... and the value shows after the env's next in-launch reset
        assert np.array_equal(walls(), current), t
    assert np.array_equal(current, later)
    for k in env._STATE_KEYS:
        assert torch.equal(getattr(env, k), getattr(plain, k)), k
    env.check_errors()


# P4: a kernel compiled at run time runs the same program
def test_specialized_kernel_equals_the_tables(tmp_path):
    import torch
    B = 16
    kind, pname = "split", "s"
    seeds = 8900 + np.arange(B)
    vals = PE.values(kind, B)
    kw = dict(batch_size=B, seeds=seeds, place_obs=False, auto_reset=True, view=11)
    env = PE._factory(kind, None, specialize="auto", specialize_cache=str(tmp_path), **kw)
    twin = PE._factory(kind, None, **kw)
    # as in test_hip_specialize.py: where the GPU tests run, libhiprtc loads — "auto" falling back to the table's kernel for
    # whatever reason fails here, it does not skip
    assert env.kernel_name.startswith("mg::render_kernel<11, 8, ") and twin.kernel_name.startswith("mg::render_kernel<0, 8, ")
    assert torch.equal(_started(env, **{pname: vals}), _started(twin, **{pname: vals}))
    rng = np.random.RandomState(43)
    ends = 0
    for t in range(30):
        a = torch.from_numpy(rng.randint(0, 7, size=(B, 2)))
        o, r, d, _ = env.step(a)
        o2, r2, d2, _ = twin.step(a)
        assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2), t
        ends += int(d.sum())
    assert ends >= 2 * B
    for k in env._STATE_KEYS:
        assert torch.equal(getattr(env, k), getattr(twin, k)), k
    # the specialised kernel placed what the table says: the split column is the env's value
    W, H = env.width, env.height
    g = env.grid_state[:, :W * H].reshape(B, W, H).cpu().numpy()
    wall = 1
    assert ((g[np.arange(B), vals, 1:H - 1] == wall).sum(axis=1) == H - 3).all()
    env.check_errors()


# P5: split invariance
def test_shards_pipeline_and_checkpoint_equal_the_one_env():
    import torch
    from marlgrid_amd import envs as E
    PE.register()
    kind, pname, B = "clutter", "n", 24
    name = PE.name_of(kind)
    kw = dict(batch_size=B, seed=8800, place_obs=False, auto_reset=True, max_steps=10)
    one = E.make(name, **kw)
    ds = E.make(name, devices=[0, 0], **kw)
    pipe = E.make(name, pipeline=2, **kw)
    vals = PE.values(kind, B)                               # global env order
    for e in (one, ds, pipe):
        e.set_params(**{pname: vals})
    one.seed(8800)
    ds._each(lambda k, env: env.seed())
    pipe._each(lambda k, env: env.seed())
    o = one.reset()
    assert torch.equal(ds.gather(ds.reset()), o)
    po = pipe.reset()
    pipe.synchronize()
    assert torch.equal(torch.cat(po), o)
    assert torch.equal(torch.cat([p[pname] for p in ds.params]).cpu(), one.params[pname].cpu())
    rng = np.random.RandomState(41)
    resumed = None
    for t in range(30):
        if t == 7:                                          # a change in global order, mid-episode, by id
            ids, new = np.array([23, 0, 11, 12, 5]), np.array([20, 0, 1, 19, 7])
            for e in (one, ds, pipe):
                e.set_params(env_ids=ids, **{pname: new})
        if t == 21:                                         # ... and by mask, from a device tensor
            mask = torch.from_numpy(np.arange(B) % 3 == 0).to(one.device)
            for e in (one, ds, pipe, resumed):
                e.set_params(env_mask=mask, **{pname: 2})
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
            sd = one.state_dict()
            assert "params_t" in sd and torch.equal(sd["params_t"], one.params_t)
            resumed = E.make(name, **dict(kw, seed=1))
            resumed.reset()
            resumed.load_state_dict(sd)
            assert torch.equal(resumed.params_t, one.params_t)
            whole = ds.state_dict()                         # the shards' checkpoint is the one env's, `params_t` included
            assert torch.equal(whole["params_t"], sd["params_t"].cpu())
    for k in one._STATE_KEYS + ("params_t",):
        assert torch.equal(getattr(one, k), getattr(resumed, k)), k
    one.check_errors(), resumed.check_errors(), pipe.check_errors()
    for e in ds.envs:
        e.check_errors()
