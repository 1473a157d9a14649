#!/usr/bin/env python
"""DeviceShards against the one env of the same total batch, in ONE process and ONE run, legs alternating block by block.

What is measured, per leg (the one env; the shards stepped with one device tensor of the whole batch; the shards stepped with
a list of per-shard tensors):

  host_issue_us_per_step   wall time for step() to RETURN, no synchronisation: `--issue-steps` calls from an idle device (the
                           queue never fills), per block; median over blocks.  For N shards this is the cost of N launches
                           issued from one thread — the hot path of DeviceShards.
  agent_steps_per_s        `--steps` steps closed by synchronize(), per block; median over blocks.

and for the one env `single_kernel_us`: HIP events around `--issue-steps` back-to-back steps on its stream (the host runs
ahead of the device, so this is the launch's duration on the device, not its latency), per launch; median over blocks.
`issue_longer_than_kernel` says whether issuing all shards of a step takes longer than that one launch runs.

The workload is bench.py's: MarlGrid-3AgentCluttered15x15-v0, auto_reset=True, uniform actions over the 7 ids.  On a machine
with one GPU `--devices cuda:0,cuda:0,...` is plumbing, not scaling: the shards share the GPU the one env has to itself.

usage: bench_device_shards.py --devices cuda:0,cuda:0 [--envs 32768 | --envs-per-shard 32768] [--steps 300] [--blocks 7]
                              [--out profiles/device_shards/NAME.jsonl]        (one JSON line, appended)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WL = "MarlGrid-3AgentCluttered15x15-v0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--devices", required=True, help="comma-separated, repeats allowed: cuda:0,cuda:0")
    ap.add_argument("--envs", type=int, default=32768, help="total envs")
    ap.add_argument("--envs-per-shard", type=int, default=0, help="instead of --envs: total = this x number of devices")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--issue-steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_shards", "device_shards.jsonl"))
    args = ap.parse_args()
    import torch
    from marlgrid_amd.envs import make
    if not torch.cuda.is_available():
        sys.exit("bench_device_shards: no HIP device (there is no CPU fallback, and a CPU timing would say nothing)")
    devices = [d.strip() for d in args.devices.split(",") if d.strip()]
    B = args.envs_per_shard * len(devices) if args.envs_per_shard else args.envs
    n = 3
    kw = dict(batch_size=B, auto_reset=True, strict=False, seed=1337)
    shards = make(WL, devices=devices, **kw)
    one = make(WL, device=shards.devices[0], **kw)
    g = torch.Generator().manual_seed(0)
    host = [torch.randint(0, 7, (B, n), generator=g) for _ in range(16)]
    whole = [a.to(shards.devices[0]) for a in host]
    lists = []
    for a in host:
        per = []
        for k in range(len(devices)):
            with shards.on(k):
                per.append(shards.shard(k, a).to(shards.devices[k]))
        lists.append(per)
    shards.reset(), one.reset()
    shards.synchronize()
    torch.cuda.synchronize(shards.devices[0])
    # the legs step the same trajectories: three steps compared whole before anything is timed
    for i in range(3):
        o, r, d, _ = shards.gather(shards.step(whole[i]))
        o2, r2, d2, _ = one.step(whole[i])
        assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2), "shards differ from the one env at step %d" % i

    def sync():
        shards.synchronize()
        for d in set(shards.devices):
            torch.cuda.synchronize(d)

    legs = {"single": lambda i: one.step(whole[i % 16]),
            "shards_tensor": lambda i: shards.step(whole[i % 16]),
            "shards_list": lambda i: shards.step(lists[i % 16])}
    issue = {k: [] for k in legs}
    rate = {k: [] for k in legs}
    kernel_us = []
    for name, fn in legs.items():
        for i in range(args.warmup):
            fn(i)
    sync()
    for block in range(args.blocks):
        for name, fn in legs.items():
            sync()
            t = time.perf_counter()
            for i in range(args.issue_steps):
                fn(i)
            issue[name].append((time.perf_counter() - t) / args.issue_steps * 1e6)
            sync()
            t = time.perf_counter()
            for i in range(args.steps):
                fn(i)
            sync()
            rate[name].append(B * n * args.steps / (time.perf_counter() - t))
        # the one env's launch on the device: events around back-to-back steps (a few in front, so that the host is ahead)
        s = torch.cuda.current_stream(one.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(8):
            legs["single"](i)
        e0.record(s)
        for i in range(args.issue_steps):
            legs["single"](i)
        e1.record(s)
        e1.synchronize()
        kernel_us.append(e0.elapsed_time(e1) / args.issue_steps * 1e3)
    shards.check_errors(), one.check_errors()

    def stats(v):
        return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    med_issue = {k: statistics.median(v) for k, v in issue.items()}
    med_kernel = statistics.median(kernel_us)
    rec = {"workload": WL, "devices": devices, "distinct_devices": len(set(str(d) for d in shards.devices)),
           "gpu": torch.cuda.get_device_name(shards.devices[0]), "visible_gpus": torch.cuda.device_count(),
           "envs_total": B, "shard_sizes": [hi - lo for lo, hi in shards.ranges], "kernel_names": sorted(set(shards.kernel_names)),
           "single_kernel_name": one.kernel_name, "steps": args.steps, "issue_steps": args.issue_steps, "blocks": args.blocks,
           "host_issue_us_per_step": {k: stats(v) for k, v in issue.items()},
           "agent_steps_per_s": {k: stats(v) for k, v in rate.items()},
           "single_kernel_us": stats(kernel_us),
           "issue_longer_than_kernel": {k: bool(med_issue[k] > med_kernel) for k in ("shards_tensor", "shards_list")},
           "placement_found": {"single": [p and bool(p.get("found")) for p in one.obs_placement],
                               "shards": [[p and bool(p.get("found")) for p in rec] for rec in shards.obs_placement]},
           "torch": torch.__version__, "hip": torch.version.hip}
    line = json.dumps(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    print(line)
    shards.close()


if __name__ == "__main__":
    main()
