"""Build-container only: every case of tests/act_table.py run on the REFERENCE -> tests/golden/acttable.npz.

Per batch ("default", "noghost", "respawn") and per step of a case's script: the canonical state (refstate.canonical),
grid.encode(), the float64 rewards, `done`, the shuffled order and the name of the exception raised ("" for none).  A script
stops at the step that raised; the rows after a case's last step are zero.

The scene is built as make_golden.py:gen_interact builds its scenes — a fresh `_gen_grid` (EmptyMultiGrid's draws nothing),
put_obj, try_place_obj of the agents in index order, `carrying` — with the objects BEFORE the agents, so that an agent goes into
the stack of what lies under it.  The reference's renderer cannot draw closed doors and keys (NameError, objects.py:309, 370)
and step() renders after the state is updated, losing the rewards it was about to return: no observation is recorded, so the
env's gen_agent_obs is replaced by a stub and step() returns what it computed.

    python tests/golden/make_act_table.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import refload  # noqa: E402
import refstate  # noqa: E402
import scenarios  # noqa: E402
import act_table as A  # noqa: E402

CANON = ("base_enc", "pos", "dir", "active", "done", "carry_enc", "ordinal")


def ref_env(case):
    from marlgrid import objects as RO
    sp = A.spec(case.variant)
    recipe = scenarios.ref_recipe(A.NAME)
    env = refstate.make_ref_env(sp, (recipe[0], dict(recipe[1], **A.VARIANTS[case.variant])), seed=case.seed)
    env.reset()
    env._gen_grid(env.width, env.height)
    for oid, x, y in case.objects:
        env.put_obj(A.product_objects(RO)[oid - 1], x, y)
    for k, (x, y, d) in enumerate(case.agents):
        a = env.agents[k]
        a.agents = []
        a.pos = None
        assert env.try_place_obj(a, np.array([x, y]))
        a.dir = d
    for k, oid in enumerate(case.carrying):
        if oid:
            env.agents[k].carrying = A.product_objects(RO)[oid - 1]
    env.gen_agent_obs = lambda agent: None
    env.np_random = refstate.OrderSpy(env.np_random)
    return env


def main():
    refload.load()
    d = {}
    for variant, batch in A.cases().items():
        B, T = len(batch), A.STEPS
        rec = dict(base_enc=np.zeros((B, T, 9, 9, 3), np.uint8), pos=np.zeros((B, T, 3, 2), np.int16),
                   dir=np.zeros((B, T, 3), np.int8), active=np.zeros((B, T, 3), bool), done=np.zeros((B, T, 3), bool),
                   carry_enc=np.zeros((B, T, 3, 3), np.uint8), ordinal=np.zeros((B, T, 3), np.int8),
                   step_count=np.zeros((B, T), np.int32), encode=np.zeros((B, T, 9, 9, 3), np.uint8),
                   rewards=np.zeros((B, T, 3), np.float64), env_done=np.zeros((B, T), bool),
                   order=np.zeros((B, T, 3), np.int8), steps=np.zeros(B, np.int8))
        errors = np.zeros((B, T), "U16")
        for b, case in enumerate(batch):
            env = ref_env(case)
            for t, act in enumerate(case.actions):
                try:
                    _, r, dn, _ = env.step(act)
                    err = ""
                except Exception as ex:       # noqa: BLE001 — the exception's class is the golden
                    err, r, dn = type(ex).__name__, np.zeros(3), False
                c = refstate.canonical(env)
                for k in CANON:
                    rec[k][b, t] = c[k]
                rec["step_count"][b, t] = c["step_count"]
                rec["encode"][b, t] = env.grid.encode()
                rec["rewards"][b, t] = np.asarray(r, np.float64)
                rec["env_done"][b, t] = dn
                rec["order"][b, t] = env.np_random.last
                errors[b, t] = err
                rec["steps"][b] = t + 1
                if err:
                    break
        for k, v in rec.items():
            d["%s/%s" % (variant, k)] = v
        d["%s/error" % variant] = errors
        d["%s/names" % variant] = np.array([c.name for c in batch])
        print(variant, B, "cases;", {e: int((errors == e).sum()) for e in np.unique(errors) if e}, flush=True)
    out = os.path.join(HERE, "acttable.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "B")


if __name__ == "__main__":
    main()
