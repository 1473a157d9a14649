"""GPU (-m gpu): mg_level_seed + mg_level_apply through the C ABI alone (ctypes on caller-owned device buffers, nothing of
marlgrid_amd.base): the bank rows against numpy's RandomState, the apply's three rules, and what the entry points refuse."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def test_level_seed_and_apply_on_caller_owned_buffers():
    import torch
    from marlgrid_amd import _native as N
    from marlgrid_amd import seeding
    lib = N.lib()
    dev = torch.device("cuda", 0)
    B, n, L, T = 131, 2, 70, 5
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    bank_mt, bank_pos, bank_head = z((L, N.MT_N), torch.int32), z((L,), torch.int32), z((L, N.MT_HEAD), torch.int32)
    bank_seed = torch.full((L,), -1, dtype=torch.int64, device=dev)
    bank = (L, _ptr(bank_mt), _ptr(bank_pos), _ptr(bank_head), _ptr(bank_seed))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    # seeding: 67 rows (a full wave and three lanes) into slots out of order; an empty seed, a slot outside the bank, a masked row
    seeds = np.array([0, 1, 2 ** 32, 2 ** 63 - 1] + list(range(1000, 1063)), np.int64)
    slots = np.random.RandomState(2).permutation(L)[:len(seeds)].astype(np.int64)
    bank_mt.fill_(0x5A5A5A5A)
    d_seeds, d_slots = torch.from_numpy(seeds).to(dev), torch.from_numpy(slots).to(dev)
    assert lib.mg_level_seed(len(seeds), _ptr(d_seeds), _ptr(d_slots), None, *bank[:1], *bank[1:], stream) == 0
    mt, pos, head, bs = bank_mt.cpu().numpy().view(np.uint32), bank_pos.cpu().numpy(), bank_head.cpu().numpy().view(np.uint32), bank_seed.cpu().numpy()
    for s, slot in zip(seeds.tolist(), slots):
        st = np.random.RandomState(seeding.seed_words(s)).get_state()
        assert bs[slot] == s and seeding.same_stream(seeding.numpy_form(mt[slot], pos[slot], N.MT_HEAD), (st[1], st[2])), s
    rest = np.setdiff1d(np.arange(L), slots)
    assert (bs[rest] == -1).all() and (mt[rest] == 0x5A5A5A5A).all()
    more = torch.tensor([-1, 5, 6, 7], dtype=torch.int64, device=dev)
    where = torch.tensor([int(slots[0]), L, -1, int(slots[1])], dtype=torch.int64, device=dev)
    keep = torch.tensor([1, 1, 1, 0], dtype=torch.uint8, device=dev)
    assert lib.mg_level_seed(4, _ptr(more), _ptr(where), _ptr(keep), *bank, stream) == 0
    bs2 = bs.copy()
    bs2[slots[0]] = -1
    assert np.array_equal(bank_seed.cpu().numpy(), bs2) and np.array_equal(bank_mt.cpu().numpy().view(np.uint32), mt)
    bs = bs2

    # the apply: a state of B envs
    cfg = N.Config()
    cfg.B, cfg.n_agents, cfg.max_steps = B, n, T
    g = torch.Generator().manual_seed(1)
    env_mt = torch.randint(-2 ** 31, 2 ** 31, (B, N.MT_N), generator=g, dtype=torch.int64).to(torch.int32).to(dev)
    env_pos = torch.randint(0, N.MT_N, (B,), generator=g, dtype=torch.int32).to(dev)
    env_head = torch.randint(-2 ** 31, 2 ** 31, (B, N.MT_HEAD), generator=g, dtype=torch.int64).to(torch.int32).to(dev)
    rec = torch.randint(0, 2 ** 62, (B, n), generator=g, dtype=torch.int64) & ~(N.AF_DONE << (8 * N.AG_FLAGS))
    sc = torch.randint(0, T + 1, (B,), generator=g, dtype=torch.int32)
    rec[5] |= N.AF_DONE << (8 * N.AG_FLAGS)          # every agent done
    sc[5] = 0
    rec[6, 0] |= N.AF_DONE << (8 * N.AG_FLAGS)       # all but one
    sc[6] = 0
    rec, sc = rec.to(dev), sc.to(dev)
    done, err, grid = z((B,), torch.uint8), z((B,), torch.int32), z((B, 16), torch.uint8)
    done.fill_(1)                                    # (never read)
    st = N.State(_ptr(grid), _ptr(rec), _ptr(env_mt), _ptr(env_pos), _ptr(sc), _ptr(done), _ptr(err), None, _ptr(env_head), None)
    lvl = torch.from_numpy(np.random.RandomState(4).randint(-1, L + 2, B).astype(np.int64)).to(dev)
    ep_level = torch.full((B,), -7, dtype=torch.int64, device=dev)
    out_level = torch.full((B,), -9, dtype=torch.int64, device=dev)

    def snapshot():
        return [t.cpu().numpy().copy() for t in (env_mt, env_pos, env_head, rec, ep_level)]

    def check(before, selected):
        now = snapshot()
        lv = lvl.cpu().numpy()
        for b in range(B):
            filled = 0 <= lv[b] < L and bs[lv[b]] >= 0
            if selected[b] and filled:
                s = lv[b]
                assert np.array_equal(now[0][b].view(np.uint32), mt[s]) and now[1][b] == pos[s] and np.array_equal(now[2][b].view(np.uint32), head[s]), b
                assert np.array_equal(now[3][b], before[3][b] & ~(0xFF << (8 * N.AG_DIR))) and now[4][b] == bs[s], b
            else:
                assert all(np.array_equal(now[i][b], before[i][b]) for i in range(4)), b
                assert now[4][b] == (-1 if selected[b] else before[4][b]), b
        assert np.array_equal(out_level.cpu().numpy(), now[4])

    args = lambda rule, mask: (C.byref(cfg), C.byref(st), rule, _ptr(mask), _ptr(lvl), *bank, _ptr(ep_level), _ptr(out_level), stream)
    before = snapshot()
    assert lib.mg_level_apply(*args(N.LEVEL_PUBLISH, None)) == 0
    check(before, np.zeros(B, bool))
    scn = sc.cpu().numpy()
    ended = scn >= T
    ended[5] = True
    assert ended.any() and not ended.all() and not ended[6]
    assert lib.mg_level_apply(*args(N.LEVEL_PENDING, None)) == 0
    check(before, ended)
    mask = torch.from_numpy(np.random.RandomState(5).randint(0, 3, B).astype(np.uint8)).to(dev)
    before = snapshot()
    assert lib.mg_level_apply(*args(N.LEVEL_MASK, mask)) == 0
    check(before, mask.cpu().numpy() != 0)
    before = snapshot()
    assert lib.mg_level_apply(*args(N.LEVEL_MASK, None)) == 0
    check(before, np.ones(B, bool))
    assert int(done.sum()) == B and int(err.abs().sum()) == 0

    # what the entry points refuse, before anything is launched
    bad = list(args(N.LEVEL_PENDING, None))
    for i, v in ((0, None), (1, None), (2, 3), (4, None), (5, -1), (6, None), (9, None), (10, None),
                 (6, C.c_void_p(bank_mt.data_ptr() + 4)), (8, C.c_void_p(bank_head.data_ptr() + 8))):
        a = list(bad)
        a[i] = v
        assert lib.mg_level_apply(*a) == N.E_ARG, i
    odd = N.State(_ptr(grid), _ptr(rec), C.c_void_p(env_mt.data_ptr() + 4), _ptr(env_pos), _ptr(sc), _ptr(done), _ptr(err), None, _ptr(env_head), None)
    a = list(bad)
    a[1] = C.byref(odd)
    assert lib.mg_level_apply(*a) == N.E_ARG
    sa = [4, _ptr(more), _ptr(where), _ptr(keep), *bank, stream]
    for i, v in ((0, -1), (1, None), (4, -1), (5, None), (6, None), (7, None), (8, None)):
        a = list(sa)
        a[i] = v
        assert lib.mg_level_seed(*a) == N.E_ARG, i
    assert lib.mg_level_seed(0, _ptr(more), None, None, *bank, stream) == 0         # nothing to do is no error
    torch.cuda.synchronize()
