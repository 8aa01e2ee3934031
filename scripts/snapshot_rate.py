#!/usr/bin/env python3
"""Device-resident snapshots (csrc/pg_snapshot.hip): what save_all, load_all and a fork of half the batch
onto the other half cost at --num-envs coinrun envs, next to the per-env host path (set_state).

The device calls are timed with events on the engine stream, the median of --reps after a warm-up.
Each timed call follows an enqueued step, so the GPU is still busy while the host uploads the call's id
lists and launches its kernels: the interval between the two events is the kernels' own time.  A load
re-renders the envs it restored, so load_all and fork include one render of those envs; the copy alone
is what save_all shows.  The copy moves only live data: its bytes are estimated from the scalars of
--sample envs (read and written once each) and set against the 8 TB/s HBM peak of the MI355X.

The host path: ProcgenGym3Env.set_state of --host-envs envs (every env restored through the host,
each restore re-rendering the whole batch), wall clock, per env.

Prints one JSON line; --out also writes it to a file.

    python3 scripts/snapshot_rate.py --out profiles/snapshot_rate.json
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "procgen-1_amd"))

HBM_PEAK = 8e12
# PGEnv words (csrc/pg_engine.h)
W_NUM_ENTS, W_MAIN_W, W_MAIN_H, W_GRID8_OK, W_NUM_TAIL = 27, 43, 44, 67, 127
NF, MT_BYTES, PGENV_BYTES = 25, 2 * 625 * 4, 512


def live_bytes(env, sample):
    """Mean bytes of one env's state the copy kernel moves, over `sample` envs spread over the batch."""
    total = 0
    ids = [int(i * env.num / sample) for i in range(sample)]
    for i in ids:
        s = env.debug_env(i)
        ne, nt = int(s[W_NUM_ENTS]), int(s[W_NUM_TAIL])
        cells = int(s[W_MAIN_W]) * int(s[W_MAIN_H])
        quads = (ne + 3) // 4 + (128 - (512 - nt) // 4 if nt else 0)
        total += PGENV_BYTES + NF * 16 * quads + 16 * ((cells + 7) // 8) + MT_BYTES
        if s[W_GRID8_OK]:
            total += 16 * ((cells + 15) // 16)
    return total / len(ids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env-name", default="coinrun")
    ap.add_argument("--num-envs", type=int, default=65536)
    ap.add_argument("--host-envs", type=int, default=64)
    ap.add_argument("--warm-steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    from procgen_amd import ProcgenGym3Env

    n = args.num_envs
    env = ProcgenGym3Env(num=n, env_name=args.env_name, num_levels=0, start_level=0, rand_seed=0, device_buffers=True)
    stream = torch.cuda.ExternalStream(env.device_ptrs().stream)
    t = 0
    for _ in range(args.warm_steps):
        env.act_hashed(1, t)
        t += 1
    env.wait()
    per_env = live_bytes(env, min(args.sample, n))
    store = env.snapshot_store(n)
    half = np.arange(n // 2, dtype=np.int32)

    def timed(fn):
        nonlocal t
        ms = []
        for k in range(args.reps + 1):
            env.act_hashed(1, t)
            t += 1
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            if k:  # the first is the warm-up
                ms.append(a.elapsed_time(b))
        return statistics.median(ms), ms

    save_ms, save_all = timed(store.save_all)
    load_ms, load_all = timed(store.load_all)
    fork_ms, fork_all = timed(lambda: env.fork(half, half + n // 2))
    env.wait()
    store.close()
    env.close()

    m = args.host_envs
    host = ProcgenGym3Env(num=m, env_name=args.env_name, num_levels=0, start_level=0, rand_seed=0)
    rng = np.random.RandomState(0)
    for _ in range(20):
        host.act(rng.randint(0, 15, size=m).astype(np.int32))
        host.observe()
    states = host.get_state()
    host_s = []
    for k in range(args.reps + 1):
        t0 = time.perf_counter()
        host.set_state(states)
        if k:
            host_s.append(time.perf_counter() - t0)
    host.close()
    host_per_env_ms = statistics.median(host_s) / m * 1e3

    moved = 2 * per_env * n  # every live byte is read once and written once
    out = {
        "what": "device-resident snapshots vs the host set_state path",
        "env_name": args.env_name, "num_envs": n, "reps": args.reps,
        "slot_bytes": store.slot_bytes, "store_GB": round(store.slot_bytes * n / 1e9, 3),
        "live_bytes_per_env": round(per_env, 1),
        "save_all_ms": round(save_ms, 4), "save_all_ms_runs": [round(x, 4) for x in save_all],
        "save_all_GB_moved": round(moved / 1e9, 3),
        "save_all_TBps": round(moved / (save_ms * 1e-3) / 1e12, 3),
        "save_all_fraction_of_hbm_peak": round(moved / (save_ms * 1e-3) / HBM_PEAK, 3),
        "save_all_us_per_env": round(save_ms * 1e3 / n, 5),
        "load_all_ms": round(load_ms, 4), "load_all_ms_runs": [round(x, 4) for x in load_all],
        "load_all_us_per_env": round(load_ms * 1e3 / n, 5),
        "fork_half_ms": round(fork_ms, 4), "fork_half_ms_runs": [round(x, 4) for x in fork_all],
        "fork_half_us_per_forked_env": round(fork_ms * 1e3 / (n // 2), 5),
        "host_set_state_envs": m,
        "host_set_state_ms_per_env": round(host_per_env_ms, 4),
        "host_set_state_ms_runs": [round(x * 1e3, 3) for x in host_s],
        "host_over_device_load_per_env": round(host_per_env_ms * 1e3 / (load_ms * 1e3 / n), 1),
        "note": "load_all and fork_half include the re-render of the restored envs; the host figure is per env at "
                "host_set_state_envs envs and grows with the batch (each restore re-renders the whole batch)",
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
