"""The per-env setters, pinned: `set_params`, `set_levels` (bank form and seeds form), `LevelBank.assign` and the sharded
`split_params` / `split_levels` over every way of selecting envs and of giving values, and every refusal they have — the tables
they leave (or the exception's type and message) equal tests/golden/per_env_setters.json, written by
`python tests/test_per_env_setters_pinned.py --write` on the commit BEFORE the setters' shared logic moved into
marlgrid_amd/per_env.py.  Two rows differ from that commit on purpose and are asserted on their own below (an integer mask
selects where it is nonzero on every path; a CPU tensor of `env_ids` is range-checked by `set_params` too).  Host only: every env
is built `_dry`; tests/test_hip_per_env_setters.py replays the accepted rows with device tensors against the same table."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "golden", "per_env_setters.json")
BATCHES = (6, 65)               # 65: one env past a wave's worth (the GPU replay); refusals and the splits at 6 only
LO, HI = 0, 21                  # the `clutter` parameter's interval
BANK_SEEDS = [10, 2 ** 63 - 1, -1, 7]
RANGES = [(0, 2), (2, 6)]
LEVEL_ENV = "MarlGrid-3AgentCluttered15x15-v0"
SETTERS = ("params", "bank", "seeds")


def selections(B):
    mask = np.arange(B) % 3 != 1
    ids = [B - 1, 0, B // 2]
    return {"all": {}, "mask_bool": dict(env_mask=mask), "mask_int": dict(env_mask=mask.astype(np.int64)),
            "ids_list": dict(env_ids=ids), "ids_array": dict(env_ids=np.array(ids)),
            "ids_empty": dict(env_ids=np.zeros(0, np.int64)), "ids_empty_list": dict(env_ids=[])}


def value_forms(setter, B):
    """(what every row starts from, {form: value}): an int, one per env, one per listed env"""
    r = np.arange(B, dtype=np.int64)
    if setter == "params":
        return (2 * r + 1) % HI, {"int": 7, "per_env": (3 + 5 * r) % HI, "per_id": np.array([20, 0, 11])}
    if setter == "bank":
        return r % 4, {"int": 2, "per_env": r % 5 - 1, "per_id": np.array([3, -1, 0])}
    per_env = np.where(r % 4 == 2, -1, 1000 + r)
    per_env[0], per_env[-1] = 2 ** 63 - 1, 2 ** 32 + 5
    return 500 + r, {"int": 42, "per_env": per_env, "per_id": np.array([9, -1, 2 ** 63 - 1])}


def rows(setter, B):
    """[(row id, selection kwargs, value)]"""
    out = []
    for sname, sel in selections(B).items():
        for vname, v in value_forms(setter, B)[1].items():
            if vname == "per_id" and not sname.startswith("ids"):
                continue
            if vname == "per_id" and "empty" in sname:
                v = v[:0]
            out.append(("%s/%s/%s" % (setter, sname, vname), sel, v))
    return out


def make_envs(B, **kw):
    """(the `clutter` parameter env, the levels env, a bank of the levels env)"""
    import param_envs
    import product_envs
    penv = param_envs.build("clutter", batch_size=B, seeds=list(range(B)), **kw)
    lenv = product_envs.build(LEVEL_ENV, batch_size=B, seeds=list(range(B)), auto_reset="next_step", **kw)
    return penv, lenv, lenv.level_bank(BANK_SEEDS)


def call(setter, penv, lenv, bank, sel, value):
    if setter == "params":
        penv.set_params(n=value, **sel)
    elif setter == "bank":
        lenv.set_levels(bank, value, **sel)
    else:
        lenv.set_levels(seeds=value, **sel)


def tables(setter, penv, lenv):
    if setter == "params":
        return {"n": penv.params["n"].tolist(), "params_t": list(penv.params_t.shape)}
    if setter == "bank":
        return {"level_of_env": lenv._level_of_env.tolist()}
    return {"level_of_env": lenv._level_of_env.tolist(), "own_seeds": lenv._own_bank.seeds.tolist()}


def outcome(fn, state):
    """what `fn()` left: `state()`, and the exception's type and message if it raised"""
    try:
        fn()
    except Exception as e:      # noqa: BLE001 (whatever it is gets pinned)
        return dict(state(), error=[type(e).__name__, str(e)])
    return state()


def sweep(B, envs=None, conv=lambda v: v, only=None):
    """row id -> outcome, for the accepted forms: every row starts from the setter's base table"""
    penv, lenv, bank = envs or make_envs(B, _dry=True)
    out = {}
    for setter in SETTERS:
        base = value_forms(setter, B)[0]
        for rid, sel, v in rows(setter, B):
            if only is not None and not only(rid):
                continue
            call(setter, penv, lenv, bank, {}, base)
            sel = {k: conv(x) for k, x in sel.items()}
            out[rid] = outcome(lambda: call(setter, penv, lenv, bank, sel, conv(v)), lambda: tables(setter, penv, lenv))
    return out


def refusals():
    """row id -> outcome at B = 6: everything the setters refuse (and a few things only some of them do)"""
    B = 6
    penv, lenv, bank = make_envs(B, _dry=True)
    m6, ids = [1, 0, 0, 1, 1, 0], [5, 0, 3]
    common = {"both": dict(env_mask=m6, env_ids=[0]), "mask_shape": dict(env_mask=[1] * 5), "mask_2d": dict(env_mask=[m6]),
              "ids_high": dict(env_ids=[6]), "ids_low": dict(env_ids=[0, -1]), "ids_float": dict(env_ids=[1.0]),
              "ids_bool": dict(env_ids=[True])}
    per = {"params": dict(high=21, low=-1, high_in_array=[0, 1, 2, 3, 4, 25], bool=True, float=1.5, float_array=[1.0] * 6,
                          short=[1, 2], two_d=[[1] * 6], object_overflow=2 ** 70, uint64=np.uint64(2 ** 63),
                          object_small=np.array([1] * 6, dtype=object)),
           "bank": dict(high=4, low=-2, high_in_array=[0, 0, 0, 0, 0, 4], bool=True, float=1.5, float_array=[1.0] * 6,
                        short=[0, 1], two_d=[[0] * 6], object_overflow=2 ** 70, uint64=np.uint64(2 ** 63)),
           "seeds": dict(low=-2, low_in_array=[0, 1, 2, 3, 4, -2], bool=True, float=1.0, float_array=[1.0] * 6, short=[1, 2],
                         two_d=[[1] * 6], object_overflow=2 ** 63, object_array=[1, 2, 3, 4, 5, 2 ** 70], uint64=np.uint64(2 ** 63))}
    out = {}
    for setter in SETTERS:
        base, forms = value_forms(setter, B)
        state = lambda: tables(setter, penv, lenv)      # noqa: E731
        call(setter, penv, lenv, bank, {}, base)
        for name, sel in common.items():
            out["%s/refuse/%s" % (setter, name)] = outcome(lambda: call(setter, penv, lenv, bank, sel, forms["int"]), state)
        for name, v in per[setter].items():
            out["%s/refuse/value_%s" % (setter, name)] = outcome(lambda: call(setter, penv, lenv, bank, {}, v), state)
        for name, v in (("short", [1, 2]), ("long", [1, 2, 3, 4])):
            out["%s/refuse/ids_value_%s" % (setter, name)] = outcome(lambda: call(setter, penv, lenv, bank, dict(env_ids=ids), v), state)
    pstate, lstate = (lambda: tables("params", penv, lenv)), (lambda: tables("seeds", penv, lenv))
    out["params/refuse/unknown_name"] = outcome(lambda: penv.set_params(m=1), pstate)
    out["params/refuse/unknown_name_of_none"] = outcome(lambda: lenv.set_params(n=1), lambda: {})
    out["params/refuse/no_values"] = outcome(lambda: penv.set_params(env_ids=[0]), pstate)
    for name, kw in (("nothing", {}), ("bank_alone", dict(bank=bank)), ("ids_alone", dict(ids=[0] * 6)),
                     ("bank_and_seeds", dict(bank=bank, ids=0, seeds=1)), ("ids_and_seeds", dict(ids=0, seeds=1)),
                     ("no_bank", dict(bank=[1, 2], ids=0)),
                     ("partial_switch_ids", dict(bank=bank, ids=0, env_ids=[0])),       # (the seeds form is the one in use)
                     ("partial_switch_mask", dict(bank=bank, ids=0, env_mask=m6))):
        out["levels/refuse/%s" % name] = outcome(lambda: lenv.set_levels(**kw), lstate)
    lenv.set_levels(bank, 1)
    out["levels/refuse/partial_switch_to_seeds"] = outcome(lambda: lenv.set_levels(seeds=5, env_ids=[0]), lstate)
    import product_envs
    same = product_envs.build(LEVEL_ENV, batch_size=B, seeds=list(range(B)), auto_reset=True, _dry=True)
    out["levels/refuse/same_step_reset"] = outcome(lambda: same.set_levels(seeds=3), lambda: {})
    return out


def bank_assign():
    """row id -> outcome: LevelBank.assign on a bank of 4, one call after the other"""
    from marlgrid_amd import LevelBank
    bank = LevelBank(4, _dry=True)
    calls = [("first", None, [3, 4]), ("slots_list", [0, 3], [10, 2 ** 63 - 1]), ("slots_array", np.array([2, 1]), np.array([-1, 8])),
             ("empty", [], np.zeros(0, np.int64)), ("empty_lists", [], []), ("all", None, np.arange(4)),
             ("slot_high", [4], [1]), ("slot_low", [-1], [1]), ("seed_low", [0], [-2]), ("twice", [1, 1], [1, 2]),
             ("shapes", [0, 1], [1]), ("too_many", None, [1] * 5), ("float_seed", [0], [1.5]), ("float_slot", [0.0], [1]),
             ("bool_seed", [0], [True]), ("object_overflow", [0], [2 ** 63]), ("uint64", [0], np.array([2 ** 63], np.uint64)),
             ("uint64_fits", [0], np.array([2 ** 63 - 1], np.uint64)), ("scalar", 2, 77)]
    out = {}
    for name, slots, seeds in calls:
        out["assign/" + name] = outcome(lambda: bank.assign(slots, seeds), lambda: {"seeds": bank.seeds.tolist()})
    for name, arg in (("ctor_seeds", [5, -1, 6]), ("ctor_none", 0), ("ctor_bad_seed", [1, -3])):
        made = []
        out["assign/" + name] = outcome(lambda: made.append(LevelBank(arg, _dry=True)), lambda: {"seeds": [b.seeds.tolist() for b in made]})
    return out


def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    return v


def splits():
    """row id -> outcome: split_params / split_levels of every accepted row at B = 6 over RANGES, and what they refuse"""
    from marlgrid_amd import sharding
    out = {}
    fns = {"params": lambda sel, v: sharding.split_params(RANGES, n=v, **sel),
           "bank": lambda sel, v: sharding.split_levels(RANGES, ids=v, **sel),
           "seeds": lambda sel, v: sharding.split_levels(RANGES, seeds=v, **sel)}
    m6 = [1, 0, 0, 1, 1, 0]
    bad = {"both": (dict(env_mask=np.array(m6), env_ids=[0]), 1), "mask_shape": (dict(env_mask=np.array(m6[:5])), 1),
           "mask_list_shape": (dict(env_mask=m6[:5]), 1), "ids_high": (dict(env_ids=[6]), 1), "ids_low": (dict(env_ids=[-1]), 1),
           "ids_float": (dict(env_ids=[1.0]), 1), "short": ({}, [1, 2]), "two_d": ({}, [[1] * 6]),
           "ids_value_long": (dict(env_ids=[5, 0, 3]), [1, 2, 3, 4]), "ids_value_per_env": (dict(env_ids=[5, 0, 3]), np.arange(6))}
    for setter, fn in fns.items():
        got = []
        for rid, sel, v in rows(setter, 6):
            out["split/" + rid] = outcome(lambda: got.append(fn(sel, v)), lambda: {"parts": _plain(got[-1:])})
        for name, (sel, v) in bad.items():
            out["split/%s/refuse/%s" % (setter, name)] = outcome(lambda: got.append(fn(sel, v)), lambda: {"parts": _plain(got[-1:])})
            del got[:]
    for name, kw in (("nothing", {}), ("ids_and_seeds", dict(ids=1, seeds=1))):
        out["split/levels/refuse/" + name] = outcome(lambda: sharding.split_levels(RANGES, **kw), lambda: {})
    return out


def collect():
    out = {}
    for B in BATCHES:
        for rid, got in sweep(B).items():
            out["B%d/%s" % (B, rid)] = got
    out.update(refusals())
    out.update(bank_assign())
    out.update(splits())
    return _plain(out)


def pinned():
    with open(TABLE) as f:
        return json.load(f)


def test_every_setter_row_is_the_pinned_one():
    want = pinned()
    got = collect()
    assert sorted(got) == sorted(want)
    assert len(want) >= 287 and sum("error" in r for r in want.values()) >= 121, "the table lost rows: %d" % len(want)
    for rid in sorted(want):
        assert got[rid] == want[rid], "%s differs from the pinned outcome" % rid


def test_the_shared_messages_are_raised_from_one_place():
    pkg = os.path.join(os.path.dirname(HERE), "marlgrid_amd")
    lines = [(name, line) for name in sorted(os.listdir(pkg)) if name.endswith(".py") for line in open(os.path.join(pkg, name))]
    for msg in ("env_mask must have shape", "env_mask or env_ids, not both", "env_ids outside 0..", "an int or one value per env"):
        assert [name for name, line in lines if "raise" in line and msg in line] == ["per_env.py"], msg
    assert not [line for name, line in lines if name == "sharding.py" and "str(e)" in line]      # (no message is rewritten)


def as_tensors(device):
    """arrays and lists -> tensors of `device`; ints stay ints"""
    import torch
    return lambda v: v if isinstance(v, (int, np.integer)) else torch.as_tensor(np.asarray(v)).to(device)


@pytest.mark.parametrize("B", BATCHES)
def test_per_env_functions_over_cpu_tensors_leave_the_numpy_tables(B):
    """marlgrid_amd.per_env driven directly with torch CPU tensors and device=cpu — the torch branch of every function, which an
    env only takes on a GPU: select, values and write leave what the `_dry` (numpy) setters left in the table"""
    import torch
    from marlgrid_amd import per_env as P
    want, cpu, conv = pinned(), torch.device("cpu"), as_tensors("cpu")
    args = {"params": ("set_params", "n", LO, HI, "set_params(n=)", "the parameter's interval [%d, %d)" % (LO, HI),
                       dict(dtype=np.uint8, wide=False, clamp=True)),
            "bank": ("set_levels", "level_of_env", -1, len(BANK_SEEDS), "set_levels(ids=)", "[-1, %d)" % len(BANK_SEEDS), {}),
            "seeds": ("set_levels", "own_seeds", -1, None, "set_levels(seeds=)", "[-1, 2**63)", {})}
    n = 0
    for setter in SETTERS:
        who, key, lo, hi, label, interval, kw = args[setter]
        for rid, sel, v in rows(setter, B):
            dst = torch.from_numpy(value_forms(setter, B)[0].astype(kw.get("dtype", np.int64)))

            def run():
                mask, ids = P.select(B, cpu, conv(sel["env_mask"]) if "env_mask" in sel else None,
                                     conv(sel["env_ids"]) if "env_ids" in sel else None, who, any_number=setter == "params")
                assert mask is None or (mask.dtype == torch.uint8 and int(mask.max()) <= 1)
                P.write(dst, P.values(conv(v), lo, hi, B, ids, cpu, label, interval, **kw), mask, ids)
            got = outcome(run, lambda: {key: dst.tolist()})
            pin = want["B%d/%s" % (B, rid)]
            assert got == {k: pin[k] for k in got}, rid
            assert ("error" in got) == ("error" in pin), rid
            n += 1
    assert n == len([r for r in want if r.startswith("B%d/" % B)])


# ---- the two rows that differ from the parent commit on purpose: its copies of the logic contradicted each other there --------
def test_an_integer_mask_selects_where_it_is_nonzero_on_every_path():
    """(one copy took an integer mask's low byte: 256 selected nothing there)"""
    import torch
    from marlgrid_amd import per_env as P
    m = [0, 1, 2, 256, -1, 0]
    for device, mask in ((None, m), (None, np.array(m)), (torch.device("cpu"), m), (torch.device("cpu"), torch.tensor(m))):
        got = P.select(6, device, mask, None, "reset")[0]
        assert got.tolist() == [0, 1, 1, 1, 1, 0] and got.dtype in (np.uint8, torch.uint8)
    penv, lenv, bank = make_envs(6, _dry=True)
    penv.set_params(n=0)
    penv.set_params(n=9, env_mask=np.array(m))
    lenv.set_levels(bank, 0)
    lenv.set_levels(bank, 3, env_mask=np.array(m))
    assert penv.params["n"].tolist() == [0, 9, 9, 9, 9, 0] and lenv._level_of_env.tolist() == [0, 3, 3, 3, 3, 0]


def test_host_resident_env_ids_are_range_checked_whatever_they_are():
    """(a CPU tensor of ids went to the device unchecked in set_params, and was used as an index there)"""
    import torch
    from marlgrid_amd import per_env as P
    for who, lenient in (("set_params", True), ("set_levels", False)):
        for bad in ([6], np.array([0, 6]), torch.tensor([6]), torch.tensor([2, -1])):
            for device in (None, torch.device("cpu")):
                with pytest.raises(ValueError, match=r"^%s: env_ids outside 0\.\.5$" % who):
                    P.select(6, device, None, bad, who, any_number=lenient)
        assert P.select(6, torch.device("cpu"), None, torch.tensor([5, 0]), who, any_number=lenient)[1].tolist() == [5, 0]
    penv = make_envs(6, _dry=True)[0]
    with pytest.raises(ValueError, match="env_ids outside"):
        penv.set_params(n=1, env_ids=torch.tensor([6]))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_per_env_setters_pinned.py --write")
    table = collect()
    with open(TABLE, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(rid), json.dumps(table[rid], sort_keys=True, separators=(",", ":")))
                                   for rid in sorted(table)) + "\n}\n")       # (a row per line: diffs stay readable)
    print("%d rows, %d refusals -> %s" % (len(table), sum("error" in r for r in table.values()), TABLE))
