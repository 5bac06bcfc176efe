#!/usr/bin/env python3
"""Circuit scheduler timing: a 16-bit ripple-carry addition (examples/add_two_numbers.rs, 80 gates in 33 levels) at
SECURITY_128_BIT through the native scheduler (Circuit.run_dev -> tfhe_hip_circuit_run_dev + gather) and through the
torch-scheduled path it replaced (Circuit._run_dev_torch), alternating the two after a warm-up, on one GPU.

    python profiles/circuit_bench.py [--reps 15] [--big 4096] [--out FILE]

Prints one JSON object: per path and batch size the median / min wall time of a whole run (host clock, from the first
enqueue to torch.cuda.synchronize()) and, for the big batch, gate bootstraps per second.  Both paths produce the same
words (tests/test_gpu_circuit.py); this only times them."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15, help="timed runs per path at B = 1 (alternating)")
    ap.add_argument("--big", type=int, default=4096, help="the large batch")
    ap.add_argument("--big-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import rs_tfhe_amd as R
    from oracle import oracle as O

    sk, ock = O.keygen(O.SECURITY_128_BIT, 11)
    ck = R.CloudKey(R.params.SECURITY_128_BIT, ock.bootstrapping_key, ock.key_switching_key, ock.decomposition_offset,
                    ock.blind_rotate_testvec)
    eng = R.Engine(R.params.SECURITY_128_BIT, 0)
    eng.load_cloud_key(ck)
    bits = 16
    c = R.Circuit(2 * bits + 1)
    c.add(list(range(bits)), list(range(bits, 2 * bits)), 2 * bits)
    gates = len(c.gates)
    res = {"circuit": "add16", "gates": gates, "levels": len(c.levels()), "params": "SECURITY_128_BIT",
           "clock": "host wall clock (time.perf_counter) around run + torch.cuda.synchronize()"}
    rng = np.random.default_rng(5)

    def inputs(B):
        return torch.from_numpy(sk.encrypt_bool(rng.integers(0, 2, (2 * bits + 1) * B).astype(bool), 77)
                                .reshape(2 * bits + 1, B, -1).view(np.int32)).to("cuda:0")

    paths = {"native": c.run_dev, "torch": c._run_dev_torch}

    def timed(fn, x):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(eng, x)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for B, reps in ((1, args.reps), (args.big, args.big_reps)):
        x = inputs(B)
        for name, fn in paths.items():  # warm-up: plans, allocator, kernels' first launch
            for _ in range(2):
                timed(fn, x)
        ms = {k: [] for k in paths}
        for _ in range(reps):
            for name, fn in paths.items():
                ms[name].append(timed(fn, x))
        for name in paths:
            v = sorted(ms[name])
            entry = {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "runs": len(v)}
            if B > 1:
                entry["gate_bootstraps_per_s"] = gates * B / (entry["median_ms"] / 1e3)
            res[f"B{B}_{name}"] = entry
        res[f"B{B}_native_over_torch"] = res[f"B{B}_native"]["median_ms"] / res[f"B{B}_torch"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
