"""Which library calls a step makes, without a GPU and without the library: a dry env whose `_lib` records every mg_* call and
answers 0 — or MG_E_UNSUPPORTED for a scripted set of names —, driven through `_launch_step` three times.  The matrix below is
the full product of the options the choice depends on; tests/golden/step_launch.json is what the tree made of it BEFORE the choice
moved to marlgrid_amd/step_launch.py (recorded with this file: `python tests/step_launch_cases.py record`), outcomes deduplicated,
rows as indices.  tests/test_step_launch_host.py holds the tree to it.

`python tests/step_launch_cases.py time [--tree DIR]`: the host cost of a `_launch_step` whose choice is made, for six
representative rows, of the package in DIR (default: this tree) — profiles/step_launch/README.md."""
import ctypes as C
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "step_launch.json")
REFUSABLE = ("mg_step_render_delta", "mg_step_render_delta_ex", "mg_step_render_encode", "mg_step_render_ep")
AXES = (("obs_delta", ("auto", True, False)),
        ("episode", (None, "episode_info", "next_step")),
        ("encode_in_step", (False, True)),
        ("fused_step", (True, False)),
        ("groups", (1, 2)),                                # two: views 7, 5, 7
        ("obs_format", ("image", "encoded")),
        ("specialize", ("none", "plain", "all")),          # which wants the first step finds a handle for
        ("refused", tuple(range(1 << len(REFUSABLE)))))    # bit k: the library answers MG_E_UNSUPPORTED for REFUSABLE[k]
ROWS = list(itertools.product(*(v for _, v in AXES)))
# the choice is made again after _release_spec(): the same three steps, the handles released and replaced between steps 2 and 3
SWAPS = [("auto", ep, enc, True, 1, "image", spec, 0) for spec in AXES[6][1] for ep in AXES[1][1] for enc in (False, True)]
E_UNSUPPORTED = -101


class Ptr:
    """a tensor, as far as a launch looks at one"""
    def data_ptr(self):
        return 64

    def element_size(self):
        return 8

    def fill_(self, v):
        return self


class FakeLib:
    """every mg_* attribute is a call that is written down — name, for a `specialize` call its handle, which arguments were
    NULL — and answered"""

    def __init__(self, refused=(), log=None):
        self.refused, self.log = frozenset(refused), log

    def __getattr__(self, name):
        if not name.startswith("mg_"):
            raise AttributeError(name)
        rc = E_UNSUPPORTED if name in self.refused else 0
        if self.log is None:            # (timing: nothing is written down)
            f = lambda *a: rc
        else:
            def f(*a):
                null = ",".join(str(i) for i, x in enumerate(a) if x is None or (isinstance(x, C.c_void_p) and not x.value))
                h = "#%x" % a[0].value if name.endswith("_spec") or name.endswith("_spec_release") else ""
                self.log.append("%s%s|%s" % (name, h, null))
                return rc
        self.__dict__[name] = f
        return f


def handles(env, base):
    which = {"none": (), "plain": (0,), "all": (0, 1, 2)}[env._case_spec]
    for k, g in enumerate(env._groups):
        g.spec = {w: C.c_void_p(base + 16 * k + w) if w in which else None for w in (0, 1, 2)}


def build(row, log=None):
    from marlgrid_amd import _native as N
    from marlgrid_amd.envs import ClutteredMultiGrid
    obs_delta, episode, encode, fused, groups, fmt, spec, refused = row
    views = (7, 5, 7) if groups == 2 else (7, 7, 7)
    agents = [dict(view_size=v, view_tile_size=8, observation_style="image", color=c) for v, c in zip(views, ("red", "blue", "purple"))]
    kw = {"episode_info": dict(episode_info=True), "next_step": dict(auto_reset="next_step"), None: {}}[episode]
    env = ClutteredMultiGrid(agents=agents, grid_size=15, n_clutter=0, batch_size=2, obs_delta=obs_delta, encode_in_step=encode,
                             fused_step=fused, obs_format=fmt, specialize=False if spec == "none" else "auto", specialize_cache=False,
                             _dry=True, **kw)
    assert env._hetero == (groups == 2)
    env._lib = FakeLib([n for k, n in enumerate(REFUSABLE) if refused >> k & 1], log)
    env._cfg, env._state = N.Config(), N.State()
    env.obs, env.rewards, env.grid_encoding = Ptr(), Ptr(), Ptr()
    env._stream = lambda: C.c_void_p(8)
    env._case_spec = spec
    for g in env._groups:
        g.cfg, g.obs = N.Config(), Ptr()
    handles(env, 0x1000)
    env._delta_launches = 0
    # (as _alloc_state: signatures only where the step has a delta twin)
    env._ring, env._ring_i = [dict(sig=Ptr() if env._delta_wanted() else None, ep=N.Episode())], 0
    prog = C.byref(N.Episode()) if env.auto_reset else None          # (any non-NULL pointer)
    ep = C.byref(env._ring[0]["ep"]) if env._use_ep else None
    return env, (Ptr(), prog, C.c_void_p(8), None if log is None else lambda k: log.append("probe%d" % k), ep)


def run(row, swap=False):
    """[[the three steps' entries], [_enc_fused, _ep_fused, _delta_ok, _delta_launches, _delta_wanted()]]"""
    log = []
    env, args = build(row, log)
    steps = []
    for t in range(3):
        if swap and t == 2:
            env._release_spec()
            handles(env, 0x2000)
        try:
            env._launch_step(*args)
        except NotImplementedError as e:
            log.append("raise: %s" % e)
        steps.append(list(log))
        del log[:]
    return [steps, [bool(env._enc_fused), bool(env._ep_fused), bool(env._delta_ok), env._delta_launches, bool(env._delta_wanted())]]


def record():
    outcomes, index = [], {}

    def put(o):
        key = json.dumps(o)
        if key not in index:
            index[key] = len(outcomes)
            outcomes.append(o)
        return index[key]
    return {"axes": [[k, list(v)] for k, v in AXES], "rows": [put(run(r)) for r in ROWS],
            "swaps": [put(run(r, True)) for r in SWAPS], "outcomes": outcomes}


# plain delta; delta_ex with both extras; render_ep; render_encode; two launches with mg_encode; encoded views
TIMED = {"delta": ("auto", None, False, True, 1, "image", "none", 0),
         "delta_ex": (True, "episode_info", True, True, 1, "image", "none", 0),
         "render_ep": ("auto", "next_step", False, True, 1, "image", "none", 0),
         "render_encode": (False, None, True, True, 1, "image", "none", 0),
         "two_launches_encode": (False, None, True, False, 1, "image", "none", 0),
         "encode_views": ("auto", None, False, True, 1, "encoded", "none", 0)}


def time_rows(calls=200000):
    import time
    out = {}
    for name, row in TIMED.items():
        env, args = build(row)
        step = env._launch_step
        step(*args)
        t0 = time.perf_counter()
        for _ in range(calls):
            step(*args)
        out[name] = round((time.perf_counter() - t0) / calls * 1e9, 1)
    return out


if __name__ == "__main__":
    tree = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else os.path.dirname(HERE)
    sys.path.insert(0, tree)
    if sys.argv[1] == "record":
        rec = record()
        with open(GOLDEN, "w") as f:
            json.dump(rec, f, separators=(",", ":"))
        print("%d rows + %d swaps, %d outcomes" % (len(rec["rows"]), len(rec["swaps"]), len(rec["outcomes"])))
    elif sys.argv[1] == "time":
        print(json.dumps({"ns_per_launch_step": time_rows()}))
