"""CPU: what every launch reads (marlgrid_amd/launch_tables.py, uploaded by MultiGridEnv._sync_tables) equals what the tree
derived before that module existed — tests/golden/launch_tables.json, recorded by tests/launch_table_cases.py —; the settings
value is the launch config's scalar part, no more and no less; the gather atlas has the layout the raster reads as 16-byte
pieces (mg_render_kernel.h: `atlas_gather_off`).  The golden and error tests pass on the recording tree too; the ones that
import the new module do not exist there."""
import json

import numpy as np
import pytest

import launch_table_cases as cases


@pytest.fixture(scope="module")
def golden():
    with open(cases.GOLDEN) as f:
        return json.load(f)


def test_every_case_is_recorded(golden):
    names = cases.case_names()
    assert sorted(golden) == sorted(names) and len(names) == len(set(names)) >= 144
    # the six shapes (cases.SHAPES): kernel names and offsets as measured on the recording tree
    for k, want in enumerate((("<7, 8, 4, 0, 0>", 0), ("<7, 5, 4, 0, 2>", 3616), ("<7, 11, 4, 0, 2>", 17440), ("<5, 0, 4, 0, 0>", 0),
                              ("<7, 8, 4, 9, 0>", 0), ("<9, 0, 4, 0, 0>", 0))):
        g, = golden["shape-%d" % k]["groups"]
        assert (g["kernel_name"][len("mg::render_kernel"):], g["atlas_gather_off"]) == want
    assert golden["shape-3"]["groups"][0]["hide_by"] and golden["tile5-no-gather-atlas"]["groups"][0]["atlas_gather_off"] == 0
    assert len(golden["two-groups-reject"]["groups"]) == 2 and golden["two-groups-reject"]["spawn_reject"]
    assert "read in place" in golden["grid-in-place-200"]["warnings"][0]


@pytest.mark.parametrize("name", cases.case_names())
def test_sync_tables_equals_the_recording(golden, name):
    assert cases.row(name) == golden[name]


def test_group_tables_writes_nothing():
    LT = pytest.importorskip("marlgrid_amd.launch_tables")
    env = cases.two_groups_reject()
    del cases.REJECT_CALLS[:]
    before = [dict(vars(env))] + [dict(vars(g)) for g in env._groups]
    for g in env._groups:
        t = LT.group_tables(env, g)
        assert not (t.cfg.obj or t.cfg.atlas or t.cfg.hide_by_obj or t.cfg.spawn_reject or t.cfg.atlas_gather_off)
    assert [dict(vars(env))] + [dict(vars(g)) for g in env._groups] == before and not cases.REJECT_CALLS
    cfg, raw, flat, atlas = env._host_tables(env._groups[1])
    assert bytes(cfg) == bytes(t.cfg) and np.array_equal(raw, t.obj_raw) and np.array_equal(flat, t.atlas_flat)
    assert bytes(env._obj_table(5)) == bytes(LT.obj_table(env.obj_reg, 5))
    # the env's older names: hide_by left on the group by _host_tables, the spawn reject table as a read-only view
    assert env._groups[1].hide_by is None and np.array_equal(env._spawn_reject, LT.reject_table(env, LT.read_settings(env)))
    hiding = cases.build("shape-3")
    t = LT.group_tables(hiding, hiding._groups[0])
    assert not hasattr(hiding._groups[0], "hide_by") and hiding._spawn_reject is None
    hiding._host_tables()
    assert t.hide_by.any() and np.array_equal(hiding._groups[0].hide_by, t.hide_by)
    with pytest.raises(AttributeError):
        hiding._spawn_reject = None


# ---- settings: one value, read in one place ------------------------------------------------------------------------------
def _settings_env():
    return cases._empty([dict(view_tile_size=8), dict(view_tile_size=8, color="blue"), dict(view_tile_size=8, color="prestige")])


def _f(pos):
    return pos[0] == 1


def _g(pos):
    return pos[0] == 1


# (where, attribute, the values assigned in turn; the constructor's default is where every walk starts and ends)
# spawn_delay counts steps: whole numbers, of any numeric type (a fraction would be cut off in the config and is no case here)
SETTINGS = [("env", "max_steps", (50, 100.0, 101)), ("env", "reward_decay", (False, 0, 1, None)),
            ("env", "ghost_mode", (True, False, 0, None, 1, "")), ("env", "respawn", (True, 1, 0)),
            ("env", "agent_spawn_kwargs", (dict(top=(2, 2)), dict(top=np.array([2, 2])), dict(size=(3, 3)), dict(size=(99, 99)), None,
                                           dict(top=(1, 1), size=(3, 4)), dict(max_tries=7), dict(max_tries=2e5), dict(max_tries=0),
                                           dict(reject_fn=_f), dict(reject_fn=_g), dict(reject_fn=_f, top=(0, 0)), dict(reject_fn=None))),
            ("agent0", "spawn_delay", (3, 3.0, True, 0)), ("agent1", "spawn_delay", (1,)),
            ("agent2", "prestige_beta", (0.5, 1)), ("agent2", "prestige_scale", (3, 2.0)), ("agent0", "prestige_scale", (5,))]


@pytest.mark.parametrize("where,attr,values", SETTINGS, ids=["%s.%s" % s[:2] for s in SETTINGS])
def test_settings_value_changes_iff_the_config_does(where, attr, values):
    LT = pytest.importorskip("marlgrid_amd.launch_tables")
    from marlgrid_amd import _native as N
    env = _settings_env()
    obj = env if where == "env" else env.agents[int(where[5:])]
    default = getattr(obj, attr)

    tables = {}                               # settings value -> its reject table: equal values launch with the same one

    def seen():
        s = LT.read_settings(env)
        rej = tables.setdefault(s, LT.reject_table(env, s))
        cfg = N.Config()
        LT.apply_settings(cfg, s, None if rej is None else rej.ctypes.data)
        assert s == LT.read_settings(env)
        return s, bytes(cfg)
    first = last = seen()
    n_changed = 0
    for v in values + (default,):
        setattr(obj, attr, v)
        now = seen()
        assert (now[0] != last[0]) == (now[1] != last[1]), (attr, v)
        assert (now[0] != first[0]) == (now[1] != first[1]), (attr, v)
        n_changed += now[0] != last[0]
        last = now
    assert n_changed >= 2                      # (the values do change it, and the default changes it back)
    assert last == first
    with pytest.raises(AttributeError):
        first[0].max_steps = 1                 # immutable
    # ... and through the env's own thin names: the config a launch would get
    cfg = env._host_tables()[0]
    setattr(obj, attr, values[0])
    env._refresh_cfg(cfg)
    assert bytes(cfg) == bytes(env._host_tables()[0])


def test_reject_fn_is_tabulated_once_per_change_not_once_per_group():
    pytest.importorskip("marlgrid_amd.launch_tables")
    env = cases.on_cpu(cases.two_groups_reject())
    calls = cases.REJECT_CALLS
    rect = [(x, y) for x in range(1, 5) for y in range(1, 6)]
    del calls[:]
    env._sync_tables()
    assert len(env._groups) == 2 and calls == rect
    p0 = env._groups[0].cfg.spawn_reject
    assert p0 and all(g.cfg.spawn_reject == p0 for g in env._groups)
    env._sync_tables()
    env._sync_tables()
    assert calls == rect                                        # nothing changed: one compare
    env.max_steps = 7
    env._sync_tables()
    assert calls == rect * 2 and all(g.cfg.max_steps == 7 and g.cfg.spawn_reject == p0 for g in env._groups)
    env.agent_spawn_kwargs = dict(reject_fn=cases._reject, top=(1, 1), size=(2, 2))
    env._sync_tables()
    env._sync_tables()
    assert calls == rect * 2 + [(1, 1), (1, 2), (2, 1), (2, 2)]
    t = env._spawn_reject_dev.numpy()[:81].reshape(9, 9)
    assert sorted(map(tuple, np.argwhere(t))) == [(1, 2), (2, 1)]
    assert all(g.cfg.spawn_reject == env._spawn_reject_dev.data_ptr() and g.cfg.spawn_x1 == 3 for g in env._groups)
    env.agent_spawn_kwargs = {}
    env._sync_tables()
    assert calls == rect * 2 + [(1, 1), (1, 2), (2, 1), (2, 2)] and not any(g.cfg.spawn_reject for g in env._groups)


@pytest.mark.parametrize("live", [True, False], ids=["tables-current", "tables-stale"])
def test_setting_errors_recur_until_the_attribute_is_fixed(live):
    """the three errors of the settings are raised by the next `_sync_tables()` — and by every later one: the seen value is not
    advanced on a raise —, whether the tables are current (a step) or a new object kind is pending as well"""
    from marlgrid_amd.objects import Goal
    env = cases.on_cpu(cases._empty([dict(view_tile_size=8), dict(view_tile_size=8, color="blue")]))
    env._sync_tables()
    good = bytes(env._groups[0].cfg)
    for k, (exc, match, break_it, mend_it) in enumerate((
            (TypeError, "unexpected keyword argument 'bogus'", lambda: setattr(env, "agent_spawn_kwargs", dict(bogus=1)),
             lambda: setattr(env, "agent_spawn_kwargs", {})),
            (ValueError, "spawn_delay must be >= 0", lambda: setattr(env.agents[1], "spawn_delay", -1),
             lambda: setattr(env.agents[1], "spawn_delay", 0)),
            (ValueError, "empty sampling rectangle", lambda: setattr(env, "agent_spawn_kwargs", dict(top=(3, 3), size=(0, 2))),
             lambda: setattr(env, "agent_spawn_kwargs", None)))):
        if not live:
            env.obj_reg.get_key(Goal(color=("red", "blue", "purple")[k], reward=1))
        break_it()
        for _ in range(3):
            with pytest.raises(exc, match=match):
                env._sync_tables()
        mend_it()
        env._sync_tables()
        if live:
            assert bytes(env._groups[0].cfg) == good
        assert env._tables_version == env.obj_reg.version


# ---- the gather atlas ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ts", [5, 6, 7, 9, 10, 11, 12])
def test_gather_atlas_layout(ts, monkeypatch):
    LT = pytest.importorskip("marlgrid_amd.launch_tables")
    monkeypatch.delenv("MG_NO_GATHER_ATLAS", raising=False)
    n_tiles, seg = 7, 3 * ts
    rng = np.random.RandomState(ts)
    body = rng.randint(1, 256, size=4 * n_tiles * ts * seg).astype(np.uint8)            # (no zero byte: every zero below is padding)
    flat = np.concatenate([body, np.zeros((-body.size) % 16 + 16, np.uint8)])           # as group_tables pads it
    out, off = LT.gather_atlas(flat, n_tiles, ts)
    stride = (16 + seg + 3) // 4 * 4
    assert off % 16 == 0 and out.size % 16 == 0 and off >= flat.size and out.dtype == np.uint8
    assert np.array_equal(out[:flat.size], flat) and not out[flat.size:off].any()
    rows = body.reshape(-1, seg)
    copy = out[off:]
    assert copy.size >= rows.shape[0] * stride + 32 and copy.size - (rows.shape[0] * stride + 32) < 16
    rest = copy.copy()
    for r in range(rows.shape[0]):
        assert np.array_equal(copy[16 + r * stride:16 + r * stride + seg], rows[r]), r
        rest[16 + r * stride:16 + r * stride + seg] = 0
    assert not rest.any()                       # every other byte: the 16 leading ones, the rows' padding, the tail
    # the raster's 16-byte pieces stay inside the buffer: the last row's piece that starts at its last pixel byte
    last = 16 + (rows.shape[0] - 1) * stride + seg - 1
    assert last // 16 * 16 + 16 <= copy.size
    monkeypatch.setenv("MG_NO_GATHER_ATLAS", "1")
    same, zero = LT.gather_atlas(flat, n_tiles, ts)
    assert same is flat and zero == 0


def test_gather_atlas_of_a_real_group_is_what_is_uploaded(golden):
    LT = pytest.importorskip("marlgrid_amd.launch_tables")
    import hashlib
    env = cases.build("shape-2")
    t = LT.group_tables(env, env._groups[0])
    out, off = LT.gather_atlas(t.atlas_flat, t.cfg.n_tiles, 11)
    g, = golden["shape-2"]["groups"]
    assert (hashlib.sha256(out.tobytes()).hexdigest(), out.size, off) == (g["atlas"], g["atlas_bytes"], g["atlas_gather_off"])
