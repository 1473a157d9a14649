"""The dynamic LDS a launch of the obs kernel asks for against the layout the kernel assumes, where they could disagree: at the
LDS limit.  The launcher takes the size from render_pick (marlgrid_amd/csrc/mg_render_pick.h), the kernel lays its workgroup out
with the layout functions of the same header; a launch that asked for less than the kernel uses would write past its
allocation.  The configurations are ROWS of the recorded sweep (tests/golden/render_picks.npz), built as real envs — the row
with the largest `lds` of each family (chunk raster, gather, 'prestige', the grid read in place, the fused encode, the episode
code) among the rows an env can be: eight object kinds (empty, wall, goal, five boxes: two of them overlappable, as the
sweep's n_tiles assumes; a hundred or 250 kinds with only two overlappable ones are not to be had from the object classes)
and every agent in the launch (the fused steps refuse a view group).  That is the family's largest row for four of the six;
for 'prestige' the row is 16 bytes below it (163 728 of 163 744), for the grid read in place 928 bytes (162 256 of 163 184).
The env's launch config is asserted equal to the row, field by field, and render_pick's `lds` for it equal to the recorded
one — but for the four white sprite tiles an env with a 'prestige' agent appends to its atlas, which the sweep's n_tiles does
not count (both such rows leave the atlas in global memory: its size is no part of their LDS).  Each on the smallest batch that gets the row's pick — 8 envs for the 4-wave picks (a row's B of 4 095 only says "below
4 096"), 4 096 for the 8-wave one —, three steps with auto_reset, compared with the oracle (64 of the 4 096 envs)."""
import ctypes as C
import os

import numpy as np
import pytest

import scenarios
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KINDS = 8                                        # None, Wall, Goal, five Boxes
BOXES = ("red", "blue", "green", "purple", "yellow")
FIELDS = ("n_agents", "view_size", "tile_size", "n_obj", "n_tiles", "n_view", "prestige_mask", "any_hide")
# family: which rows are its own (columns of `pick`: picked, vs, ts, wpb, v, rm, lds per want), the want, constructor arguments
FAMILIES = {
    "chunk": (lambda p: (p[:, 4] == 0) & (p[:, 5] == 0) & np.isin(p[:, 2], (8, 16, 32)), 0, {}),
    "gather": (lambda p: (p[:, 4] == 0) & (p[:, 5] == 2), 0, {}),
    "prestige": (lambda p: np.isin(p[:, 4], (9, 12)) & (p[:, 5] != 3), 0, {}),
    "grid-in-place": (lambda p: p[:, 5] == 3, 0, {}),
    "encode": (lambda p: p[:, 0] == 1, 1, dict(encode_in_step=True)),
    "episode": (lambda p: p[:, 0] == 1, 2, dict(episode_info=True)),
}


def _row(family):
    """the family's row with the largest lds among the rows a real env can be -> (its config as a dict, its pick, the family's max)"""
    own, want, _ = FAMILIES[family]
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_picks.npz"))
    cfg = {str(c): d["cfg"][:, i] for i, c in enumerate(d["cfg_cols"])}
    p = d["pick"][:, 2 + 7 * want:9 + 7 * want]
    mine = (p[:, 0] == 1) & own(p)
    real = mine & (cfg["n_obj"] == KINDS) & (cfg["n_view"] == 0) & (cfg["n_tiles"] == 1 + KINDS + 2 * 4 * cfg["n_agents"])
    i = np.nonzero(real)[0][np.argmax(p[real, 6])]
    return {k: int(v[i]) for k, v in cfg.items()}, p[i], int(p[mine, 6].max())


def _scenario(row):
    """the oracle's spec and the product env class of a `grid` x `grid` room with the eight kinds"""
    from marlgrid_amd.base import MultiGrid, MultiGridEnv
    from marlgrid_amd.objects import Box, Goal, Wall
    n, g = row["n_agents"], row["grid"]
    colors = ["prestige" if (row["prestige_mask"] >> k) & 1 else (scenarios._MANY * 3)[k] for k in range(n)]
    spec = scenarios._base(n, g, row["view_size"], tile_size=row["tile_size"], colors=colors, max_steps=40)
    spec["objects"] = [None, scenarios.WALL, scenarios.GOAL] + [dict(type="Box", color=c, state=0) for c in BOXES]
    spec["wall_obj"] = 1
    prog = [("wall_rect", 0, 0, g, g), ("put", 2, g - 2, g - 2)] + [("put", 3 + i, 1 + 2 * i, 1) for i in range(5)] + [("place", 1, 12, 100)]
    spec["gen_ctor"], spec["gen_reset"] = prog, prog
    if row["any_hide"]:
        scenarios._with_hide(spec, [["Wall"]] + [[]] * (n - 1))

    class EightKindsEnv(MultiGridEnv):
        def _gen_grid(self, width, height):
            self.grid = MultiGrid((width, height))
            self.grid.wall_rect(0, 0, width, height)
            self.put_obj(Goal(color="green", reward=1), width - 2, height - 2)
            for i, c in enumerate(BOXES):
                self.put_obj(Box(color=c), 1 + 2 * i, 1)
            for _ in range(12):
                self.place_obj(Wall(), max_tries=100)
    return spec, EightKindsEnv


def _agents(spec):
    from marlgrid_amd.agents import GridAgentInterface
    return [GridAgentInterface(color=a["color"], view_size=spec["view_size"], view_tile_size=spec["tile_size"],
                               view_offset=spec["view_offset"], see_through_walls=spec["see_through_walls"],
                               hide_item_types=list(a.get("hide_item_types", [])),
                               prestige_beta=a.get("prestige_beta", 0.95), prestige_scale=a.get("prestige_scale", 2))
            for a in spec["agents"]]


def _pick(cfg, want):
    """render_pick's answer for the env's own launch config, from the g++ build of the header (tests/test_render_pick.py)"""
    from marlgrid_amd import _native as N
    from test_render_pick import load_pick_lib
    L = load_pick_lib()
    one = (N.Config * 1)()
    C.memmove(one, C.byref(cfg), C.sizeof(cfg))
    out = np.zeros((3, 7), np.int32)
    low = np.zeros(1, np.int32)
    L.pick_rows(one, 1, C.c_void_p(out.ctypes.data), C.c_void_p(low.ctypes.data))
    assert out[want, 0] == 1
    return "<%d, %d, %d, %d, %d>" % tuple(out[want, 1:6]), int(out[want, 6])


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_largest_lds_row_of_each_family_vs_oracle(family):
    import torch
    row, rp, family_max = _row(family)
    want, ctor = FAMILIES[family][1:]
    inst = "<%d, %d, %d, %d, %d>" % tuple(rp[1:6])
    assert family_max - 1024 < rp[6] <= family_max <= 160 * 1024, (rp[6], family_max)      # (the docstring's distances)
    B = 8 if rp[3] == 4 else 4096
    assert (B >= 4096) == (row["B"] >= 4096)
    spec, cls = _scenario(row)
    seeds = 7000 + np.arange(B)
    env = cls(agents=_agents(spec), grid_size=row["grid"], max_steps=40, batch_size=B, seeds=seeds, auto_reset=True, **ctor)
    cfg = env._cfg
    assert (cfg.W, cfg.H, cfg.cells_stride) == (row["grid"], row["grid"], (row["grid"] ** 2 + 15) // 16 * 16)
    sprites = 4 if row["prestige_mask"] else 0          # (see the docstring)
    assert {f: getattr(cfg, f) for f in FIELDS} == {f: row[f] + (sprites if f == "n_tiles" else 0) for f in FIELDS}
    assert not sprites or rp[4] == 12
    assert _pick(cfg, want) == (inst, int(rp[6]))
    assert env.kernel_name == "mg::render_kernel" + _pick(cfg, 0)[0]
    check = np.arange(B) if B <= 64 else np.r_[0:24, B // 2 - 8:B // 2 + 8, B - 24:B]
    orc = O.OracleBatch(spec, seeds[check])

    def sub(t):
        return t[torch.as_tensor(check, device=t.device)].cpu().numpy()
    assert np.array_equal(sub(env.reset()), orc.reset())
    rng = np.random.RandomState(5)
    n = env.num_agents
    for t in range(3):
        a = rng.randint(0, 7, size=(B, n))
        a[a == 5] = 6          # (toggling a Box is a TypeError upstream, objects.py: reproduced, and not this test's subject)
        o, r, d, _ = env.step(torch.from_numpy(a))
        o2, r2, d2, _ = orc.step(a[check], auto_reset=True)
        assert np.array_equal(sub(o), o2), "obs step %d" % t
        assert np.abs(sub(r).astype(np.float64) - r2).max() <= 1e-6
        assert np.array_equal(sub(d), d2)
        if family == "encode":
            assert torch.equal(env.grid_encoding, env.grid.encode()), t
    env.check_errors()
    # the launch was the fused one: nothing answered MG_E_UNSUPPORTED
    assert env.fused_step and not env._hetero and env._enc_fused and env._ep_fused
