"""What specialising the observation kernel on demand (MultiGridEnv(specialize=True): mg_render_specialize, hipRTC) buys for
shapes off the library's table: env.step() alone under HIP events — as tools/bench_episodes.py times it — on a cluttered
15 x 15 room with three agents at 16 384 envs (the batch of profiles/r05's fused-gather comparisons), all 7 action ids.

    python tools/bench_specialize.py [--batch 16384] [--seconds 1.5] [--legs 5] [--out profiles/specialize/NAME.jsonl]

Per shape — view 13 at 4-pixel tiles, 17 at 5, 10 at 6 — three envs in ONE process, legs alternating after a warm-up:
the specialised env, its twin on the table's run-time kernel, and the nearest shape the table has compiled in (13 at 5, 15 at
5, 7 at 6).  One JSON line per shape: ms per step of every leg and the median of each env; `speedup` = generic / specialised
(the gate: below 1 the script exits 1); observation bytes per microsecond of the specialised env against the nearest table
entry's (`per_byte_vs_table`, reported: the goal is 1.15); the seconds the compile took (a fresh cache directory) and the
seconds a second env took to get the same instantiation from that directory's file in a fresh process (`cache_load_seconds`).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [((13, 4), (13, 5)), ((17, 5), (15, 5)), ((10, 6), (7, 6))]      # (shape, nearest table entry)
COLORS = ["red", "blue", "purple"]


def build(view, tile, B, **kw):
    from marlgrid_amd.agents import GridAgentInterface
    from marlgrid_amd.envs import ClutteredMultiGrid
    team = [GridAgentInterface(color=c, view_size=view, view_tile_size=tile) for c in COLORS]
    return ClutteredMultiGrid(agents=team, grid_size=15, n_clutter=12, batch_size=B, seed=1337, device="cuda:0", auto_reset=True, **kw)


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


def cache_load(view, tile, B, cache):
    """a fresh process with the cache directory's file: seconds mg_render_specialize took, and that it was a hit"""
    code = ("import sys, time; sys.path.insert(0, %r)\n"
            "sys.path.insert(0, %r)\n"
            "import bench_specialize as S\n"
            "env = S.build(%d, %d, %d, place_obs=False, specialize=True, specialize_cache=%r)\n"
            "i = env.specialization[0]\n"
            "print('RESULT', i['cache_hit'], i['request_seconds'])\n" % (ROOT, os.path.join(ROOT, "tools"), view, tile, B, cache))
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, timeout=300, check=True).stdout.decode()
    hit, seconds = [l for l in out.splitlines() if l.startswith("RESULT")][0].split()[1:]
    return int(hit), float(seconds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--seconds", type=float, default=1.5)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from marlgrid_amd import _native
    B = a.batch
    rng = np.random.RandomState(0)
    acts = [torch.from_numpy(rng.randint(0, 7, size=(B, 3))).to("cuda:0") for _ in range(8)]
    lines, ok = [], True
    with tempfile.TemporaryDirectory() as cache:
        for (view, tile), (tview, ttile) in SHAPES:
            envs = {"specialised": build(view, tile, B, specialize=True, specialize_cache=cache),
                    "generic": build(view, tile, B),
                    "table": build(tview, ttile, B)}
            info = envs["specialised"].specialization[0]
            for env in envs.values():
                leg(env, acts, 0.7)
            ms = {k: [] for k in envs}
            for _ in range(a.legs):
                for k, env in envs.items():
                    ms[k].append(leg(env, acts, a.seconds))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            nbytes = {k: int(env.obs.numel()) for k, env in envs.items()}
            rate = {k: nbytes[k] / (med[k] * 1e3) for k in envs}        # observation bytes per microsecond
            hit, load_s = cache_load(view, tile, B, cache)
            out = {"build": _native.lib().mg_build_info().decode(), "batch": B, "view_size": view, "tile_size": tile,
                   "kernels": {k: env.kernel_name for k, env in envs.items()},
                   "nearest_table_shape": [tview, ttile], "obs_bytes": nbytes, "ms_legs": ms, "median_ms": med,
                   "speedup": med["generic"] / med["specialised"],
                   "bytes_per_us": rate, "per_byte_vs_table": rate["specialised"] / rate["table"],
                   "compile_seconds": info["compile_seconds"], "code_bytes": info["code_bytes"], "lds_bytes": info["lds_bytes"],
                   "lds_static": info["lds_static"], "cache_load_hit": hit, "cache_load_seconds": load_s}
            ok = ok and out["speedup"] >= 1.0
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
            del envs
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not ok:
        print("GATE: a specialised step is slower than the generic one", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
