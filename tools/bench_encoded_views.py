"""obs_format="encoded" against "image" on bench.py's workload (MarlGrid-3AgentCluttered15x15-v0): env.step() timed with HIP
events at 4 096, 32 768 and 262 144 envs, the two formats in the same process, legs alternating after a warm-up.  Prints one
JSON line per batch: agent-steps/s of each format (median leg), their ratio, and the bytes each step's output needs.

    python tools/bench_encoded_views.py [--batches 4096,32768,262144] [--seconds 3] [--legs 4]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def main():
    import numpy as np
    import torch
    from marlgrid_amd.envs import make
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,32768,262144")
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--legs", type=int, default=4)
    a = ap.parse_args()
    name, n = "MarlGrid-3AgentCluttered15x15-v0", 3
    for B in [int(x) for x in a.batches.split(",")]:
        envs = {f: make(name, batch_size=B, seed=1337, device="cuda:0", auto_reset=True, obs_format=f) for f in ("image", "encoded")}
        rng = np.random.RandomState(0)
        acts = [torch.from_numpy(rng.randint(0, 7, size=(B, n))).to("cuda:0") for _ in range(8)]     # all 7 ids, as bench.py
        for env in envs.values():
            leg(env, acts, 1.0)                                   # warm-up
        ms = {f: [] for f in envs}
        for _ in range(a.legs):
            for f, env in envs.items():
                ms[f].append(leg(env, acts, a.seconds))
        out = {"workload": name, "batch": B}
        for f, env in envs.items():
            best = float(np.median(ms[f]))
            out[f] = {"ms_per_step": best, "ms_legs": ms[f], "agent_steps_per_s": B * n / (best * 1e-3),
                      "out_bytes_per_step": int(env.obs.numel()), "kernel": env.kernel_name}
        out["speedup"] = out["encoded"]["agent_steps_per_s"] / out["image"]["agent_steps_per_s"]
        print(json.dumps(out), flush=True)
        del envs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
