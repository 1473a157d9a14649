"""GPU (-m gpu): the device-resident branch of the per-env setters (marlgrid_amd/per_env.py), which no host test reaches — mask,
ids and values handed to `set_params` / `set_levels` as device tensors leave, on the device, the tables that the same values left
on the host (tests/golden/per_env_setters.json, the sweep of tests/test_per_env_setters_pinned.py), at 6 envs and at 65, one
past a wave's worth.  Nothing is read back by the calls, no id is out of range, and the launch counts are those of
tests/test_hip_levels.py: none for a set_levels call through a bank, one mg_level_seed for one in the seeds form, one
mg_level_apply for the reset after them.  And what `reset(env_mask=)` does with the done flags, by the mask it is handed."""
import pytest

import test_per_env_setters_pinned as S

pytestmark = pytest.mark.gpu


def _device_rows(rid):
    # `ids_empty_list` as a tensor is `ids_empty`; the seeds form with no env selected is a launch of zero rows from an empty
    # tensor, whose null data pointer the library's argument check refuses — on the host the row is a no-op and stays pinned there
    return "ids_empty_list" not in rid and not rid.startswith("seeds/ids_empty")


@pytest.mark.parametrize("B", S.BATCHES)
def test_device_tensors_leave_the_pinned_tables(B):
    penv, lenv, bank = envs = S.make_envs(B, place_obs=False)
    want = {rid: got for rid, got in S.pinned().items() if rid.startswith("B%d/" % B) and _device_rows(rid[len("B%d/" % B):])}
    assert len(want) == 42 and not any("error" in got for got in want.values())
    got = S.sweep(B, envs, S.as_tensors(penv.device), only=_device_rows)
    assert sorted("B%d/%s" % (B, rid) for rid in got) == sorted(want)
    for rid in sorted(got):
        assert got[rid] == want["B%d/%s" % (B, rid)], rid
    n_seeds = sum(rid.startswith("seeds/") for rid in got)
    assert lenv._level_launches == 0 and bank.launches == 1
    assert lenv._own_bank.launches == 2 * n_seeds       # (each row and the call before it)
    lenv.reset()
    assert lenv._level_launches == 1
    penv.check_errors()
    lenv.check_errors()


def test_host_ids_out_of_range_never_reach_the_device():
    import torch
    penv, lenv, bank = S.make_envs(6, place_obs=False)
    before = penv.params["n"].tolist()
    for bad in (torch.tensor([6]), torch.tensor([0, -1]), [6]):
        with pytest.raises(ValueError, match="env_ids outside 0..5"):
            penv.set_params(n=1, env_ids=bad)
        with pytest.raises(ValueError, match="env_ids outside 0..5"):
            lenv.set_levels(bank, 1, env_ids=bad)
    assert penv.params["n"].tolist() == before


def test_masked_reset_clears_the_done_flags_unless_handed_the_done_buffer():
    """mg_reset clears the done flags of the envs it resets, except when its mask IS the done buffer (`env.done_t`, uint8): then
    they stay readable as step()'s return value.  step()'s bool `done` is a view of that buffer and no such request: its bytes
    are copied, as `.to(uint8)` always copied them, and the flags are cleared."""
    import product_envs
    import torch
    B, M = 65, 3
    env = product_envs.build(S.LEVEL_ENV, batch_size=B, seeds=list(range(B)), place_obs=False, auto_reset=False, max_steps=M)
    acts = torch.zeros((B, env.num_agents), dtype=torch.int64, device=env.device)

    def run_out():
        env.reset()
        for _ in range(M):
            done = env.step(acts)[2]
        assert done.dtype == torch.bool and bool(done.all()) and done.data_ptr() == env.done_t.data_ptr()
        return done
    done = run_out()
    env.reset(env_mask=done)                    # step()'s own tensor
    assert not env.done_t.any() and not done.any() and (env.step_count == 0).all()
    run_out()
    env.reset(env_mask=env.done_t)              # the buffer itself: reset, and the flags stay
    assert env.done_t.all() and (env.step_count == 0).all()
    run_out()
    some = torch.arange(B, device=env.device) % 3 == 1
    for mask in (some, some.to(torch.uint8), some.to(torch.int64) * 256, some.cpu().numpy()):     # any other mask: cleared where it selects
        env.done_t.fill_(1)
        env.reset(env_mask=mask)
        assert env.done_t.tolist() == (~some).to(torch.uint8).tolist(), mask.dtype
    env.check_errors()
