"""CPU tests of tests/wide_diff.py, the differential driver of the wide GPU tests (tests/test_hip_wide.py): a wrong kernel has
to get past it, so it is tested where it can be — with the host build of the step bodies (tests/native/hostemu.py,
`par=True, auto_reset=True`: the step as the obs kernel's fused step runs it) as the subject.

  * clean runs pass, all envs compared, and return the bookkeeping the GPU tests assert on;
  * a fault injected between two steps into ONE env away from both ends of the batch is caught, no later than the next
    deep check, and the message names exactly that env;
  * the observation / encode comparisons report the env, agent and pixel / cell of a one-byte difference;
  * the message writes env indices as runs.

Why `deep_every` bounds what the wide tests can promise about `mt_head`: numpy's form of the RNG carries only the head's
length, so a wrong look-ahead word is visible to the head comparison alone, and only until it is drawn; a wrong draw that has
been consumed can leave no trace in the state (a shuffle of agents that never meet).  The head case below therefore
corrupts the entry furthest from consumption one step before a deep check (the headline draws about 3 words per step): it
is still unconsumed there.  A head word that is corrupted AND consumed between two deep checks is caught only through what
it did to the episode."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import _native_consts as K  # noqa: E402
import scenarios  # noqa: E402
import wide_diff  # noqa: E402
from marlgrid_amd import seeding  # noqa: E402
from oracle import oracle as O  # noqa: E402

HEADLINE = "MarlGrid-3AgentCluttered15x15-v0"
SEED0 = 424200


def _subject(name, B):
    import hostemu
    seeds = SEED0 + np.arange(B)
    return wide_diff.HostEmuSubject(hostemu.HostEmu(name, B, seeds, auto_reset=True, par=True)), seeds


def test_clean_headline_4096_envs():
    sub, seeds = _subject(HEADLINE, 4096)
    s = wide_diff.run(sub, HEADLINE, seeds, 1500, deep_every=500)
    assert s["episodes"].min() >= 15, s["episodes"].min()       # time limit 100 (a few episodes end earlier, at the goal)
    assert s["blocks"].min() >= 6.5, s["blocks"].min()          # ~30 blocks per 6 000 steps (70 words per reset, ~2.5 per step)


def test_clean_config4_8agent_cluttered30x30():
    name = "Custom-8AgentCluttered30x30"
    sub, seeds = _subject(name, 512)
    s = wide_diff.run(sub, name, seeds, 600, deep_every=500)
    assert s["episodes"].min() >= 1 and s["draws"].min() > 600 * 7      # eight agents: >= 7 shuffle draws per step


def test_clean_headline_staggered_through_reset_mask():
    """env b reset by hand after step b % 100 of the first 100, through the driver's own reset(mask): afterwards every step
    ends the episodes of one residue class inside the step (the host build beside the oracle: 1 901 such steps of 2 000)"""
    sub, seeds = _subject(HEADLINE, 4096)
    s = wide_diff.run(sub, HEADLINE, seeds, 2000, deep_every=500, stagger=True)
    assert s["partial_done_steps"] == 1901, s["partial_done_steps"]
    assert s["episodes"].min() >= 19


# ---- a single-env fault is caught, and named ----------------------------------------------------------------------------
B_FAULT, ENV = 4096, 2731
DEEP = 250               # not a multiple of the time limit: the step before a deep check resets nobody


def _corrupt_mt_ahead(emu, b):
    slot = (int(emu.mt_pos[b]) + 5) % 624           # not regenerated yet: read when the generator gets there
    slot = slot or 1                                # (the low 31 bits of word 0 are never read)
    emu.mt[b, slot] ^= np.uint32(0x00010000)


def _corrupt_mt_head(emu, b):
    emu.mt_head[b, 15] ^= np.uint32(0x00010000)     # the entry furthest from consumption


def _corrupt_grid(emu, b):
    W, H = emu.env.width, emu.env.height
    g = emu.grid[b, :W * H].reshape(W, H)
    rec = emu.rec[b]
    ax = ((rec >> np.uint64(8 * K.AG_X)) & np.uint64(0xFF)).astype(np.int64)
    ay = ((rec >> np.uint64(8 * K.AG_Y)) & np.uint64(0xFF)).astype(np.int64)
    wall = g[0, 0]
    for x in range(1, W - 1):
        for y in range(1, H - 1):
            if g[x, y] == wall and (np.maximum(np.abs(ax - x), np.abs(ay - y)) > 1).all():
                g[x, y] = 0                         # a clutter wall removed, next to nobody
                return
    raise AssertionError("no clutter wall away from the agents")


def _corrupt_dir(emu, b):
    sh = np.uint64(8 * K.AG_DIR)
    d = (emu.rec[b, 0] >> sh) & np.uint64(0xFF)
    emu.rec[b, 0] = (emu.rec[b, 0] & ~(np.uint64(0xFF) << sh)) | (((d + np.uint64(1)) % np.uint64(4)) << sh)


def _corrupt_step_count(emu, b):
    emu.step_count[b] += 1


# (fault, after which step): the RNG words after step 130, the head one step before the deep check; the state faults after
# the in-launch reset of step 200 — the reset of step 300 would repair a grid cell or a record that nothing looked at since
FAULTS = {"mt_ahead": (_corrupt_mt_ahead, 130), "mt_head": (_corrupt_mt_head, DEEP - 1), "grid_cell": (_corrupt_grid, 210),
          "agent_dir": (_corrupt_dir, 210), "step_count": (_corrupt_step_count, 210)}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_single_env_fault_is_caught_and_named(fault):
    """injected after step 120 (one in-launch reset has happened, another follows): the driver raises no later than the next
    deep check, and names env 2 731 of 4 096 and no other"""
    corrupt, at = FAULTS[fault]
    sub, seeds = _subject(HEADLINE, B_FAULT)
    hit = []

    def inject(t, subject):
        if t == at:
            corrupt(subject.emu, ENV)
            hit.append(t)
    with pytest.raises(wide_diff.Mismatch) as ei:
        wide_diff.run(sub, HEADLINE, seeds, 2 * DEEP, deep_every=DEEP, after_step=inject)
    e = ei.value
    assert hit == [at] and at > 120
    assert e.envs == [ENV], (e.field, e.envs[:10])
    assert at < e.step <= DEEP, (e.step, e.field)
    msg = str(e)
    assert "%s [%s] step %d: %s differs in 1 of %d envs: %d\n" % (HEADLINE, sub.kernel_name, e.step, e.field, B_FAULT, ENV) in msg
    assert "env %d: " % ENV in msg and "RNG words drawn" in msg and "steps since its last in-launch reset" in msg
    if fault == "mt_head":
        assert e.step == DEEP and e.field.startswith("mt_head") and "entry 1" in msg      # (15 less the ~3 draws of a step)
    if fault == "mt_ahead":
        assert e.field.startswith("RNG state") or e.step < DEEP


# ---- observation and encode comparison ----------------------------------------------------------------------------------
def _oracle_arrays(B=48, steps=7):
    orc = O.OracleBatch(scenarios.registered(HEADLINE), 9000 + np.arange(B))
    rng = np.random.RandomState(2)
    for t in range(steps):
        obs, _, _, _ = orc.step(rng.randint(0, 7, size=(B, 3)), render=True, auto_reset=True)
    return orc, obs


def test_obs_comparison_reports_env_agent_and_pixel():
    orc, obs = _oracle_arrays()
    assert wide_diff.compare_rows(obs, obs.copy(), "obs") is None
    other = obs.copy()
    other[29, 1, 17, 40, 2] ^= 1
    envs, detail = wide_diff.compare_rows(other, obs, "obs")
    assert envs.tolist() == [29]
    assert detail == "env 29: agent 1, pixel (row 17, col 40, channel 2): got %d, want %d" % (other[29, 1, 17, 40, 2], obs[29, 1, 17, 40, 2])
    # rows that stand for other envs (the terminal observations of a step)
    ids = np.array([3, 500, 31002])
    envs, detail = wide_diff.compare_rows(other[[0, 29, 47]], obs[[0, 29, 47]], "obs", ids=ids)
    assert envs.tolist() == [500] and detail.startswith("env 500: agent 1, pixel (row 17, col 40, channel 2)")
    # the oracle's renders into one buffer are its gen_obs
    buf = np.zeros_like(obs)
    assert np.array_equal(wide_diff.render_pixels(orc.envs, range(len(orc.envs)), buf), orc.gen_obs())


def test_encode_comparison_reports_env_and_cell():
    orc, _ = _oracle_arrays()
    enc = np.stack([e.encode() for e in orc.envs])
    assert wide_diff.compare_rows(enc, enc.copy(), "encode") is None
    other = enc.copy()
    other[41, 6, 9, 1] += 1
    envs, detail = wide_diff.compare_rows(other, enc, "encode")
    assert envs.tolist() == [41] and detail.startswith("env 41: cell (6, 9), field 1: got ")


def test_view_comparison_and_the_batched_oracle_views():
    import viewenc
    orc, _ = _oracle_arrays()
    views = viewenc.oracle_views_batch(orc.envs)
    assert views.shape == (48, 3, 7, 7, 3) and views.any()
    for b, e in enumerate(orc.envs):
        assert np.array_equal(views[b], np.stack(viewenc.oracle_views(e))), b
    other = views.copy()
    other[7, 2, 3, 6, 0] ^= 4
    envs, detail = wide_diff.compare_rows(other, views, "views")
    assert envs.tolist() == [7] and detail.startswith("env 7: agent 2, cell (3, 6), field 0: got ")


# ---- the message --------------------------------------------------------------------------------------------------------
def test_env_indices_are_written_as_runs():
    assert wide_diff.runs([5, 6, 7, 8, 900]) == "5-8, 900"
    assert wide_diff.runs([900, 7, 5, 8, 6, 6]) == "5-8, 900"
    assert wide_diff.runs([3]) == "3" and wide_diff.runs([]) == ""
    assert wide_diff.runs(range(20480, 20488)) == "20480-20487"
    many = [10 * i for i in range(11)] + [201, 202]
    assert wide_diff.runs(many) == "0, 10, 20, 30, 40, 50, 60, 70, ..."


def test_message_is_cut_after_eight_runs_with_the_exact_count():
    """a subject that is wrong in 13 envs (11 runs): the count is exact, the list is cut"""
    sub, seeds = _subject(HEADLINE, 256)
    bad = [10 * i for i in range(1, 11)] + [201, 202, 203]

    def inject(t, subject):
        if t == 98:                 # (one step before it shows: a reward earned in between would show the env alone)
            subject.emu.step_count[bad] += 1
    with pytest.raises(wide_diff.Mismatch) as ei:
        wide_diff.run(sub, HEADLINE, seeds, 120, deep_every=500, after_step=inject)
    e = ei.value
    assert e.envs == bad and e.step == 99 and e.field == "done"
    assert "done differs in 13 of 256 envs: 10, 20, 30, 40, 50, 60, 70, 80, ...\n" in str(e)
    assert str(e).count("RNG words drawn") == wide_diff.SHOWN


# ---- the conversions the deep check makes on whole arrays ---------------------------------------------------------------
def test_numpy_form_rows_is_numpy_form_row_by_row():
    """every phase of the block, both branches (position inside the current block / still in the previous one)"""
    sub, seeds = _subject(HEADLINE, 1024)
    rng = np.random.RandomState(5)
    for t in range(130):
        sub.step(rng.randint(0, 7, size=(1024, 3)))
    emu = sub.emu
    emu.mt_pos[:40] = np.arange(40) % 20                  # (states that need not be reachable: the arithmetic is what is compared)
    key, pos = wide_diff.numpy_form_rows(emu.mt, emu.mt_pos)
    assert (emu.mt_pos <= 16).sum() >= 30 and (emu.mt_pos > 16).sum() >= 900
    for b in range(1024):
        k1, p1 = seeding.numpy_form(emu.mt[b], emu.mt_pos[b], 16)
        assert p1 == pos[b] and np.array_equal(k1, key[b]), b
    same = wide_diff.stream_diff(key, pos, key.copy(), pos.copy())
    assert not same.any()
    k2 = key.copy()
    k2[5, 0] ^= np.uint32(1)            # the low bits of word 0: the same stream
    k2[6, 0] ^= np.uint32(1 << 31)
    k2[7, 623] ^= np.uint32(1)
    p2 = pos.copy()
    p2[8] += 1
    assert np.nonzero(wide_diff.stream_diff(k2, p2, key, pos))[0].tolist() == [6, 7, 8]
    for b in (5, 6, 7, 8):
        assert seeding.same_stream((k2[b], p2[b]), (key[b], pos[b])) == (b == 5)


def test_oracle_rng_next_outputs_are_numpys():
    """the 16 outputs the head is held to: numpy's own draws from the oracle's state, every row, both sides of a block's end"""
    orc, _ = _oracle_arrays(B=700, steps=1)
    key, pos, nxt = wide_diff.oracle_rng(orc.envs)
    rs = np.random.RandomState()

    class At(object):                   # the same key at every position 0 .. 624
        def __init__(self, k, p):
            self.k, self.p = k, p

        def mt_state(self):
            return self.k, self.p
    envs = [At(key[b], b % 625) for b in range(700)]
    key2, pos2, nxt2 = wide_diff.oracle_rng(envs)
    assert (pos2 + 16 > 624).sum() >= 16
    for b in range(700):
        rs.set_state(("MT19937", key2[b], int(pos2[b]), 0, 0.0))
        assert np.array_equal(nxt2[b], rs.randint(0, 2 ** 32, size=16, dtype=np.uint64).astype(np.uint32)), b


def test_wide_cases_name_the_kernels_the_launcher_picks():
    """WIDE_CASES' render-kernel names, read off dry envs (no device): what bench.py reports for these shapes"""
    from marlgrid_amd import _native as N
    for case, (name, B, T, obs_every, kw, stagger, kernel) in sorted(wide_diff.WIDE_CASES.items()):
        env = wide_diff.build_case(case, _dry=True)
        assert env.batch_size == B and env.auto_reset is True and env.strict is True
        if kw.get("obs_format") == "encoded":
            assert kernel == "mg::encode_views_kernel<%d>" % env.agents[0].view_size
        else:
            cfg, _raw, _flat, _atlas = env._host_tables()
            assert N.render_kernel_name(cfg) == (kernel, 0), case
