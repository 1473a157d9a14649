"""Every `_gen_grid` recording the project knows, pinned: the template bytes, the recorded ops (reject tables by CRC), the op
count and `scenario_spec()`'s gen_ctor / gen_reset / objects of each scenario equal tests/golden/gen_recordings.json — the
recorder's own output, written by `python tests/test_gen_recording_pinned.py --write` on the commit BEFORE the recorder moved
out of MultiGridEnv into marlgrid_amd/gen_recorder.py (since then, by changes of the scenarios themselves: the entry of
`Branch-2AgentDeep12x10` added; the Box of `Param-kind` and its twins made a Key — their `objects` alone).  Regenerate the table only with a change that means to alter a
recorded program, and review its diff.  Host only: every env is built `_dry`."""
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "golden", "gen_recordings.json")
MIN_NAMES = 117     # 66 ids in the registry (the package's and the test modules') + 32 test scenarios + 9 draw + 6 branch + 4 parameter


def _plain(v):
    """what json makes of a value, so that a fresh record compares equal to a loaded one"""
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, np.integer):
        return int(v)
    if isinstance(v, np.floating):
        return float(v)
    if isinstance(v, bytes):
        return "crc32:%08x" % zlib.crc32(v)
    return v


def record(env):
    env._ensure_recorded()
    template, ops = env._dry_trace
    spec = env.scenario_spec()
    return _plain(dict(shape=template.shape, template=template.tobytes().hex(), ops=[tuple(op) for op in ops], n_ops=len(ops),
                       gen_ctor=spec["gen_ctor"], gen_reset=spec["gen_reset"], objects=spec["objects"]))


def collect():
    """name -> record, for every scenario there is; each built with batch_size=2, _dry=True"""
    from marlgrid_amd import envs as E
    import draw_envs
    import gen_branch_envs
    import param_envs
    import product_envs
    import scenarios
    kw = dict(batch_size=2, _dry=True)
    out = {}
    for mod in (draw_envs, gen_branch_envs, param_envs):    # their ids join the package's own in the registry
        mod.register()
    for name in sorted(E._registry):
        out["registry:" + name] = record(E.make(name, **kw))
    for name in scenarios.ALL_SCENARIOS:
        out["scenario:" + name] = record(product_envs.build(name, **kw))
    for name in draw_envs.SCENARIOS:
        out["draws:" + name] = record(draw_envs.build(name, **kw))
    for name in gen_branch_envs.SCENARIOS:
        out["branch:" + name] = record(gen_branch_envs.build(name, **kw))
    for kind in param_envs.KINDS:
        out["param:" + kind] = record(param_envs.build(kind, **kw))
    return out


def test_every_recording_is_the_pinned_one():
    with open(TABLE) as f:
        want = json.load(f)
    assert len(want) >= MIN_NAMES, "the table lost scenarios: %d names" % len(want)
    got = collect()
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        for field in sorted(want[name]):
            assert got[name][field] == want[name][field], "%s: %s differs from the pinned recording" % (name, field)
        assert got[name] == want[name], name
    assert max(r["n_ops"] for r in got.values()) == max(r["n_ops"] for r in want.values())


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(HERE, "golden"))
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_gen_recording_pinned.py --write")
    table = collect()
    with open(TABLE, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(name), json.dumps(table[name], sort_keys=True, separators=(",", ":")))
                                   for name in sorted(table)) + "\n}\n")      # (a scenario per line: diffs stay readable)
    print("%d recordings, longest %d ops -> %s" % (len(table), max(r["n_ops"] for r in table.values()), TABLE))
