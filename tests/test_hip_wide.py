"""GPU (-m gpu): whole-shard differential tests — every shape bench.py runs, at the width it runs it, against the CPU oracle
through tests/wide_diff.py: ALL envs compared, every step (done, rewards, info), every `obs_every`-th step (the whole
observation tensor, byte for byte), every 500th step (canonical state, the RNG in numpy's form and the 16 look-ahead words of
every env).  The other oracle comparisons are either wide and short or long and narrow; a fault that depends on the position
in the launch (an LDS slot, the DMA refill of one wave, the last batch of a workgroup) AND on the episode count (RNG wrap,
in-launch reset) needs both at once.  tests/wide_diff.py WIDE_CASES has the table; each env is built as bench.py builds it and
its kernel name is asserted, so a case cannot move to another instantiation unnoticed.

Coverage is asserted where the scenario guarantees it by construction (the time limit is 100 steps: steps // 100 episodes per
env), the measured RNG blocks per env are printed (-s), not asserted — except W1, whose minima (60 episodes, 25 blocks of 624
words, in every env) the oracle alone meets for these seeds and actions (60 and 30.26)."""
import pytest

import wide_diff

pytestmark = pytest.mark.gpu


def _record(case, s):
    print("\n%s: episodes per env %d .. %d, RNG blocks per env %.2f .. %.2f, steps on which some but not all envs ended %d, "
          "seconds %r" % (case, s["episodes"].min(), s["episodes"].max(), s["blocks"].min(), s["blocks"].max(),
                          s["partial_done_steps"], s["seconds"]))


def test_w1_bench_shard_6000_steps():
    """the bench shard, same-step reset, the plain instantiation"""
    env, s = wide_diff.run_case("W1")
    _record("W1", s)
    assert s["episodes"].min() >= 60, s["episodes"].min()
    assert s["blocks"].min() >= 25, s["blocks"].min()


def test_w2_bench_shard_encode_in_step():
    """the fused-encode instantiation (mg_step_render_encode): `grid_encoding` of all envs at each look"""
    env, s = wide_diff.run_case("W2")
    _record("W2", s)
    assert env.encode_in_step and env._enc_fused
    assert s["episodes"].min() >= 20, s["episodes"].min()


def test_w3_bench_shard_staggered_episodes():
    """every step resets ~1 % of the envs inside the launch, next to envs that step normally in the same wave"""
    env, s = wide_diff.run_case("W3")
    _record("W3", s)
    assert s["partial_done_steps"] >= 1850, s["partial_done_steps"]
    assert s["episodes"].min() >= 19, s["episodes"].min()


def test_w4_config1_3agent_cluttered11x11():
    """BASELINE configs[1]: one env per wave"""
    env, s = wide_diff.run_case("W4")
    _record("W4", s)
    assert s["episodes"].min() >= 60, s["episodes"].min()


def test_w5_config2_4agent_empty9x9():
    """BASELINE configs[2]: four agents, a different envs-per-batch packing"""
    env, s = wide_diff.run_case("W5")
    _record("W5", s)
    assert s["episodes"].min() >= 10, s["episodes"].min()


def test_w6_config4_8agent_cluttered30x30():
    """BASELINE configs[4]: eight agents, ~10 shuffle draws per step, view 9"""
    env, s = wide_diff.run_case("W6")
    _record("W6", s)
    assert s["episodes"].min() >= 20, s["episodes"].min()


def test_w7_bench_shard_encoded_views():
    """encode_views_kernel<7> with its compiled-in step: the views of all envs (tests/viewenc.py)"""
    env, s = wide_diff.run_case("W7")
    _record("W7", s)
    assert s["episodes"].min() >= 20, s["episodes"].min()


def test_w8_bench_shard_next_step_episode_info_staggered():
    """the _ep instantiation: every info field of all envs on every step, and EVERY terminal observation (the observation of
    each env whose episode ended, on the step it ended) — an episode costs 101 calls in next-step mode"""
    env, s = wide_diff.run_case("W8")
    _record("W8", s)
    assert env._ep_fused and env.auto_reset_mode == "next_step" and env.episode_info
    assert s["terminal_obs"].min() >= 8, s["terminal_obs"].min()
