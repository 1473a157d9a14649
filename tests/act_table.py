"""TEST INFRASTRUCTURE — pickup, drop, toggle and what they leave behind for later moves, case by case (numpy only).

One 9 x 9 room (walls, the goal in the far corner), three agents, the twelve object kinds of `spec()`: the eleven of
tests/scenarios.py:objects_zoo_spec and a Key of another colour than the doors.  ONE ENV PER CASE.  A case is a scene — what
lies under agent 0 (it stands at the centre, (4, 4)), what lies in the cell in front of it, what each agent carries, where agents
1 and 2 stand and face — and a script of one to three action rows.  The direction agent 0 faces is the case's index in its batch
mod 4, so all four arms of dir_dx / dir_dy occur.  Nothing is sampled: `cases()` enumerates

  S  one actor, one step: 15 fronts x 5 carried x 4 under x 8 actions (7 is no action: ValueError); the others act `done`
  T  scripts: a door closed on its occupant, and then the occupant's forward (AssertionError, base.py:558), left, pickup, toggle
     and done; a third agent walking at that door; the door opened again and the occupant leaving; a locked door against the
     matching Key (unlocked, opened, entered), a Ball, a Box and the other Key — each once per direction
  R  same-step races of agents 0 and 1, each on RACE_SEEDS seeds so that both shuffled orders occur
  G  the `forward` slice of S with ghost_mode=False
  P  forward onto Lava and Goal carrying each object, with respawn=True and without

in three batches, by the settings an env batch shares: "default", "noghost", "respawn".  A batch whose size is a multiple of 8
gets one no-op case, so that the last staged group of eight envs and the last wave are ragged.

A scene comes in three notations: `oracle_env` (regen_grid, put_obj, place_agent_at, set_dir, set_carrying), `product_state`
(the grid bytes and the packed agent records of the whole batch, to be written over what reset() left), and the reference's
(tests/golden/make_act_table.py, which writes tests/golden/acttable.npz).  An agent gets INTO a closed door only by a door
closing on it, hence the scripts' lead-in steps; the product's notation could write it there but runs the same script."""
import numpy as np

NAME = "Test-3AgentEmpty9x9-acttable"
LEFT, RIGHT, FORWARD, PICKUP, DROP, TOGGLE, DONE, NO_ACTION = range(8)
WALL, GOAL, DOOR_OPEN, DOOR_CLOSED, DOOR_LOCKED, KEY, BALL, LAVA, FLOOR, BONUS, BOX, KEY_OTHER = range(1, 13)
KIND = ["none", "wall", "goal", "open-door", "closed-door", "locked-door", "key", "ball", "lava", "floor", "bonus", "box",
        "other-key"]
DX, DY = (1, 0, -1, 0), (0, 1, 0, -1)
CX = CY = 4
PARK = [(1, 1, 0), (7, 1, 1)]           # where agents 1 and 2 idle (facing empty cells)
VARIANTS = {"default": {}, "noghost": dict(ghost_mode=False), "respawn": dict(respawn=True)}
STEPS = 3                               # the longest script
RACE_SEEDS = 8
SEED0 = 5000

FRONTS = [("none", 0, False)] + [(KIND[i], i, False) for i in range(1, 12)] + \
         [("agent", 0, True), ("agent-in-door", DOOR_OPEN, True), ("agent-on-floor", FLOOR, True)]
CARRIED = [0, KEY, KEY_OTHER, BALL, BOX]
UNDER = [0, DOOR_OPEN, FLOOR, BONUS]
COUNTS = {"default": 2518, "noghost": 300, "respawn": 10}       # 2 400 S + 44 T + 64 R + 10 P | 300 G | 10 P


def spec(variant="default"):
    import scenarios
    s = scenarios.registered(NAME)
    s["objects"] = scenarios.objects_zoo_spec()["objects"] + [dict(type="Key", color="yellow", state=0)]
    s.update(VARIANTS[variant])
    assert len(s["agents"]) == 3 and s["W"] == s["H"] == 9
    return s


def product_objects(PO):
    """the spec's objects 1 .. 12 as the product's (or, the same constructors, the reference's) classes build them"""
    return [PO.Wall(), PO.Goal(color="green", reward=1), PO.Door("blue", 1), PO.Door("blue", 2), PO.Door("blue", 3),
            PO.Key("blue"), PO.Ball("purple"), PO.Lava(), PO.Floor("grey"), PO.BonusTile(color="yellow", reward=1),
            PO.Box("olive"), PO.Key("yellow")]


class Case(object):
    def __init__(self, name, variant, d, objects, agents, carrying, actions):
        self.name, self.variant, self.d = name, variant, d
        self.objects, self.agents, self.carrying = list(objects), list(agents), list(carrying)
        self.actions = [list(r) for r in actions]
        self.seed = None

    def front(self):
        return CX + DX[self.d], CY + DY[self.d]


def _ahead(d, k=1):
    return CX + k * DX[d], CY + k * DY[d]


def _behind_of(e):
    """the neighbour of the centre from which an agent facing `e` faces the centre"""
    return CX - DX[e], CY - DY[e], e


def _s_case(variant, name, d, front, under, carry, action):
    _, fobj, fagent = front
    fx, fy = _ahead(d)
    objects = ([(under, CX, CY)] if under else []) + ([(fobj, fx, fy)] if fobj else [])
    agents = [(CX, CY, d), (fx, fy, d) if fagent else PARK[0], PARK[1]]
    return Case(name, variant, d, objects, agents, [carry, 0, 0], [[action, DONE, DONE]])


def _t_cases(d):
    """the scripts, for agent 0 facing d: agent 1 faces the centre from the side, agent 2 from the other side"""
    e1, e2 = (d + 1) % 4, (d + 3) % 4
    fx, fy = _ahead(d)
    shut = [DONE, TOGGLE, DONE]
    in_door = dict(agents=[(CX, CY, d), _behind_of(e1), _behind_of(e2)], carrying=[0, 0, 0])
    out = []
    for what, act, front in (("forward", FORWARD, 0), ("left", LEFT, 0), ("pickup", PICKUP, BALL),
                             ("toggle", TOGGLE, DOOR_CLOSED), ("done", DONE, 0)):
        out.append(Case("T/shut-in/%s/d%d" % (what, d), "default", d,
                        [(DOOR_OPEN, CX, CY)] + ([(front, fx, fy)] if front else []),
                        actions=[shut, [act, DONE, DONE]], **in_door))
    out.append(Case("T/shut-in/third-walks-at-it/d%d" % d, "default", d, [(DOOR_OPEN, CX, CY)],
                    actions=[shut, [DONE, DONE, FORWARD]], **in_door))
    out.append(Case("T/shut-in/reopened-leaves/d%d" % d, "default", d, [(DOOR_OPEN, CX, CY)],
                    actions=[shut, shut, [FORWARD, DONE, DONE]], **in_door))
    for what, carry in (("key", KEY), ("ball", BALL), ("box", BOX), ("other-key", KEY_OTHER)):
        out.append(Case("T/locked/%s/d%d" % (what, d), "default", d, [(DOOR_LOCKED, fx, fy)],
                        [(CX, CY, d)] + PARK, [carry, 0, 0], [[TOGGLE, DONE, DONE], [TOGGLE, DONE, DONE], [FORWARD, DONE, DONE]]))
    return out


RACES = ["into-door-vs-shut", "out-of-door-vs-shut", "pickup-vs-pickup", "pickup-vs-forward", "drop-vs-forward",
         "drop-vs-drop", "open-vs-forward", "unlock-vs-forward"]


def _r_case(race, d, i):
    """agents 0 and 1 act in one step; agent 1 faces agent 0's front cell from beyond it, but in the race out of a door, where
    it faces the centre from the side"""
    fx, fy = _ahead(d)
    bx, by = _ahead(d, 2)
    beyond = (bx, by, (d + 2) % 4)
    objects, carrying, a1_at = [], [0, 0, 0], beyond
    if race == "into-door-vs-shut":
        objects, acts = [(DOOR_OPEN, fx, fy)], [FORWARD, TOGGLE, DONE]
    elif race == "out-of-door-vs-shut":
        objects, acts, a1_at = [(DOOR_OPEN, CX, CY)], [FORWARD, TOGGLE, DONE], _behind_of((d + 1) % 4)
    elif race == "pickup-vs-pickup":
        objects, acts = [(BALL, fx, fy)], [PICKUP, PICKUP, DONE]
    elif race == "pickup-vs-forward":
        objects, acts = [(BALL, fx, fy)], [FORWARD, PICKUP, DONE]
    elif race == "drop-vs-forward":
        carrying, acts = [0, BALL, 0], [FORWARD, DROP, DONE]
    elif race == "drop-vs-drop":
        carrying, acts = [KEY, BALL, 0], [DROP, DROP, DONE]
    elif race == "open-vs-forward":
        objects, acts = [(DOOR_CLOSED, fx, fy)], [FORWARD, TOGGLE, DONE]
    elif race == "unlock-vs-forward":
        objects, carrying, acts = [(DOOR_LOCKED, fx, fy)], [0, KEY, 0], [FORWARD, TOGGLE, DONE]
    else:
        raise KeyError(race)
    return Case("R/%s/%d" % (race, i), "default", d, objects, [(CX, CY, d), a1_at, PARK[1]], carrying, [acts])


def cases():
    """-> {variant: [Case]}; a case's seed is SEED0 + its place in the whole enumeration"""
    out = {v: [] for v in VARIANTS}

    def d_of(variant):
        return len(out[variant]) % 4

    for action in range(8):
        for front in FRONTS:
            for under in UNDER:
                for carry in CARRIED:
                    name = "S/a%d/%s/on-%s/with-%s" % (action, front[0], KIND[under], KIND[carry])
                    out["default"].append(_s_case("default", name, d_of("default"), front, under, carry, action))
    for k in range(11):
        for _ in range(4):
            d = d_of("default")
            out["default"].append(_t_cases(d)[k])
    for race in RACES:
        for i in range(RACE_SEEDS):
            out["default"].append(_r_case(race, d_of("default"), i))
    for front in FRONTS:
        for under in UNDER:
            for carry in CARRIED:
                name = "G/%s/on-%s/with-%s" % (front[0], KIND[under], KIND[carry])
                out["noghost"].append(_s_case("noghost", name, d_of("noghost"), front, under, carry, FORWARD))
    for variant in ("respawn", "default"):
        for fobj in (LAVA, GOAL):
            for carry in CARRIED:
                name = "P/%s/with-%s/%s" % (KIND[fobj], KIND[carry], variant)
                out[variant].append(_s_case(variant, name, d_of(variant), (KIND[fobj], fobj, False), 0, carry, FORWARD))
    seed = SEED0
    for v in VARIANTS:
        assert len(out[v]) == COUNTS[v], (v, len(out[v]))
        if len(out[v]) % 8 == 0:
            out[v].append(Case("pad/%s" % v, v, d_of(v), [], [(CX, CY, d_of(v))] + PARK, [0, 0, 0], [[DONE, DONE, DONE]]))
        assert len(out[v]) % 8 != 0 and len(out[v]) % 64 != 0
        for c in out[v]:
            c.seed = seed
            seed += 1
    names = [c.name for v in VARIANTS for c in out[v]]
    assert len(set(names)) == len(names)
    return out


def actions(batch, t):
    """(B, 3) int64: row t of every case's script; a case whose script is over acts `done`"""
    return np.array([c.actions[t] if t < len(c.actions) else [DONE] * 3 for c in batch], np.int64)


def running(batch, t):
    """(B,) bool: the cases whose script has a row t"""
    return np.array([t < len(c.actions) for c in batch])


# ---- which cases raise, by name (the reference's exception classes; pinned by tests/golden/acttable.npz) --------------
# the race out of a door raises where the shuffled order lets agent 1 shut the door first: these seeds
RACE_OUT_ERRORS = (4, 7)


def expected_errors():
    """{case name: (step, exception class name)}"""
    out = {}
    for front in FRONTS:
        for under in UNDER:
            for carry in CARRIED:
                tail = "%s/on-%s/with-%s" % (front[0], KIND[under], KIND[carry])
                out["S/a7/" + tail] = (0, "ValueError")             # base.py:619-620
                if front[1] == BOX:
                    out["S/a5/" + tail] = (0, "TypeError")          # Box.toggle's arity, objects.py:381-382
    for d in range(4):
        out["T/shut-in/forward/d%d" % d] = (1, "AssertionError")    # base.py:558
    for i in RACE_OUT_ERRORS:
        out["R/out-of-door-vs-shut/%d" % i] = (0, "AssertionError")
    return out


# ---- notations ------------------------------------------------------------------------------------------------------
def oracle_env(sp, case, like=None):
    from oracle import oracle as O
    e = O.OracleEnv(sp, case.seed, _like=like)
    e.reset(observe=False)
    e.regen_grid()
    for oid, x, y in case.objects:
        e.put_obj(oid, x, y)
    for k, (x, y, d) in enumerate(case.agents):
        e.place_agent_at(k, x, y)
        e.set_dir(k, d)
    for k, oid in enumerate(case.carrying):
        if oid:
            e.set_carrying(k, oid)
    return e


def oracle_envs(batch):
    sp = spec(batch[0].variant)
    envs = []
    for c in batch:
        envs.append(oracle_env(sp, c, envs[0] if envs else None))
    return envs


EXC = {"ValueError": ValueError, "TypeError": TypeError, "AssertionError": AssertionError, "AttributeError": AttributeError,
       "RecursionError": RecursionError}


def oracle_step(e, acts):
    """-> (rewards, done, order, exception class name or "")"""
    try:
        _, rew, done, _, order = e.step(acts, return_order=True)
        return rew, done, order, ""
    except tuple(EXC.values()) as ex:
        return None, None, None, type(ex).__name__


def register(env, PO):
    """the spec's kinds into a product env's registry, in the spec's order: the product's object ids ARE the spec's"""
    for o in product_objects(PO):
        env.obj_reg.get_key(o)
    got = env.scenario_spec()["objects"]
    assert got == spec()["objects"], got


def product_state(batch, grid, rec, N):
    """grid (B, >= 81) uint8 and rec (B, 3) uint64 as reset() left them (walls and the goal; three placed agents) -> the same
    with every case's scene written in: objects by id at x * 9 + y, agents placed in index order (arrival rank k)"""
    grid, rec = np.array(grid, np.uint8), np.array(rec).astype(np.uint64)
    H = 9
    assert grid.shape[0] == rec.shape[0] == len(batch) and rec.shape[1] == 3
    want = N.AF_ACTIVE | N.AF_PLACED
    fl = (rec >> np.uint64(8 * N.AG_FLAGS)) & np.uint64(0xFF)
    assert (fl == want).all()
    fields = (N.AG_X, N.AG_Y, N.AG_DIR, N.AG_CARRY, N.AG_RANK)
    keep = ~np.uint64(sum(0xFF << (8 * f) for f in fields))
    for b, c in enumerate(batch):
        for oid, x, y in c.objects:
            grid[b, x * H + y] = oid
        for k, (x, y, d) in enumerate(c.agents):
            r = int(rec[b, k] & keep)
            for f, v in zip(fields, (x, y, d, c.carrying[k], k)):
                r |= int(v) << (8 * f)
            rec[b, k] = np.uint64(r)
    return grid, rec


def oracle_trace(batch, obs=False, views=False):
    """the oracle's run of a batch, computed once and shared by the product's rows: a list over the steps 0 .. STEPS - 1 of
    dict(live (B,) bool: the env is compared at this step — no exception at it or before —, err (B,) exception class names at
    THIS step, canon [B] canonical states, rewards (B, 3) float64, done (B,), encode (B, 9, 9, 3) and, asked for, obs
    (B, 3, P, P, 3) / views (B, 3, V, V, 3): gen_obs() / encode(vis_mask) of every agent's view).  A case whose script is over
    acts `done`; a case that raised is stepped no further."""
    import canon
    envs = oracle_envs(batch)
    B = len(batch)
    dead = np.zeros(B, bool)
    out = []
    for t in range(STEPS):
        acts = actions(batch, t)
        step = dict(err=np.zeros(B, "U16"), canon=[None] * B, rewards=np.zeros((B, 3)), done=np.zeros(B, bool),
                    encode=np.zeros((B, 9, 9, 3), np.uint8))
        for b, e in enumerate(envs):
            if dead[b]:
                continue
            rew, done, _, err = oracle_step(e, acts[b])
            step["err"][b] = err
            if err:
                dead[b] = True
                continue
            step["canon"][b], step["rewards"][b], step["done"][b] = canon.oracle_canonical(e), rew, done
            step["encode"][b] = e.encode()
        step["live"] = ~dead
        if obs:
            step["obs"] = np.stack([e.gen_obs() for e in envs])
        if views:
            import viewenc
            step["views"] = viewenc.oracle_views_batch(envs)
        out.append(step)
    return out


def error_names(codes, N):
    """the product's per-env error words as exception class names ("" for 0)"""
    return np.array(["" if c == 0 else N.ERR_EXC[int(c)].__name__ for c in np.asarray(codes)])
