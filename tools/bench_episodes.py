"""What the episode-boundary modes cost: env.step() alone (HIP events, as tools/bench_encoded_views.py times it) on bench.py's
workload, MarlGrid-3AgentCluttered15x15-v0 at 32 768 envs, all 7 action ids.

    python tools/bench_episodes.py [--batch 32768] [--seconds 2] [--legs 5] [--formats image,encoded]
        the variants in ONE process, legs interleaved after a warm-up: default (auto_reset=True), same_step + episode_info,
        next_step, next_step + episode_info.  One JSON line per format: ms per step of every leg, the median, the ratio to
        the default's median.
    python tools/bench_episodes.py --against DIR [--legs 5]
        the default arguments on THIS tree against another checkout of the project built in DIR (the parent commit): one
        child process per leg, alternating between the two trees.  One JSON line: both medians, both min-max.
    python tools/bench_episodes.py --one [--root DIR] ...
        (what --against runs) one leg of the default variant, with the package of DIR when given.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, N_AGENTS = "MarlGrid-3AgentCluttered15x15-v0", 3
VARIANTS = {"default": dict(auto_reset=True),
            "same_step+info": dict(auto_reset="same_step", episode_info=True),
            "next_step": dict(auto_reset="next_step"),
            "next_step+info": dict(auto_reset="next_step", episode_info=True)}


def leg(env, acts, seconds):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    steps, ms, t0 = 0, 0.0, time.time()
    while time.time() - t0 < seconds:
        s.record()
        for i in range(20):
            env.step(acts[i % len(acts)])
        e.record()
        e.synchronize()
        ms += s.elapsed_time(e)
        steps += 20
    return ms / steps


def actions(B):
    import numpy as np
    import torch
    rng = np.random.RandomState(0)
    return [torch.from_numpy(rng.randint(0, 7, size=(B, N_AGENTS))).to("cuda:0") for _ in range(8)]


def run_variants(a):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from marlgrid_amd.envs import make
    B = a.batch
    acts = actions(B)
    for fmt in a.formats.split(","):
        envs = {v: make(NAME, batch_size=B, seed=1337, device="cuda:0", obs_format=fmt, **kw) for v, kw in VARIANTS.items()}
        for env in envs.values():
            leg(env, acts, 1.0)
        ms = {v: [] for v in envs}
        for _ in range(a.legs):
            for v, env in envs.items():
                ms[v].append(leg(env, acts, a.seconds))
        base = float(np.median(ms["default"]))
        out = {"workload": NAME, "batch": B, "obs_format": fmt, "kernel": envs["default"].kernel_name,
               "fused_ep_launch": bool(envs["next_step"]._ep_fused)}
        for v in envs:
            med = float(np.median(ms[v]))
            out[v] = {"ms_per_step": med, "ms_legs": ms[v], "agent_steps_per_s": B * N_AGENTS / (med * 1e-3), "vs_default": med / base}
        print(json.dumps(out), flush=True)
        del envs
        torch.cuda.empty_cache()


def run_one(a):
    root = os.path.abspath(a.root) if a.root else ROOT
    sys.path.insert(0, root)
    from marlgrid_amd import _native
    from marlgrid_amd.envs import make
    assert os.path.abspath(_native.__file__).startswith(root), _native.__file__
    env = make(NAME, batch_size=a.batch, seed=1337, device="cuda:0", auto_reset=True)
    acts = actions(a.batch)
    leg(env, acts, 1.0)
    print(json.dumps({"root": root, "build": _native.lib().mg_build_info().decode(), "kernel": env.kernel_name,
                      "ms_per_step": leg(env, acts, a.seconds)}), flush=True)


def run_against(a):
    import numpy as np
    trees = {"this": None, "other": os.path.abspath(a.against)}
    ms, builds = {k: [] for k in trees}, {}
    for _ in range(a.legs):
        for k, root in trees.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--one", "--batch", str(a.batch), "--seconds", str(a.seconds)]
            if root:
                cmd += ["--root", root]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=120, check=True)      # (a failed or hung leg ends the run)
            r = json.loads(p.stdout.decode().strip().splitlines()[-1])
            ms[k].append(r["ms_per_step"])
            builds[k] = r["build"]
    out = {"workload": NAME, "batch": a.batch, "variant": "default arguments (auto_reset=True)"}
    for k in trees:
        out[k] = {"build": builds[k], "ms_legs": ms[k], "median_ms": float(np.median(ms[k])), "min_ms": min(ms[k]), "max_ms": max(ms[k])}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--formats", default="image,encoded")
    ap.add_argument("--against")
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--root")
    a = ap.parse_args()
    if a.one:
        run_one(a)
    elif a.against:
        run_against(a)
    else:
        run_variants(a)


if __name__ == "__main__":
    main()
