"""Packing-key generation on one GPU against the host generator, on SECURITY_128_BIT and SECURITY_UINT4: wall time of
tfhe_hip_gen_packing_key with the bodies downloaded, of the same call with bodies = NULL (the key stays on the handle),
and of packing.make_packing_key on this box's host CPUs (numpy), all under one fixed generator key.

    python3 profiles/packing_keygen_bench.py [--reps 5] [--host-reps 5] [--out profiles/packing_keygen_bench.json]
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUPS = 2


def timed(fn, reps, sync):
    """WARMUPS untimed calls, then `reps` timed ones; `sync` drains the device (a no-op for the host generator)."""
    for _ in range(WARMUPS):
        fn()
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(np.min(ts)), 3), "calls": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--sets", default="SECURITY_128_BIT,SECURITY_UINT4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packing_keygen_bench.json"))
    args = ap.parse_args()
    if args.reps < 5 or args.host_reps < 5:
        ap.error("every figure is the median of at least 5 calls")
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd.packing import make_packing_key
    from rs_tfhe_amd.params import PARAM_SETS

    K = bytes(range(32))
    props = torch.cuda.get_device_properties(0)
    res = {"clock": "host wall clock (time.perf_counter) around the call with the device drained before and after; "
                    f"{WARMUPS} warm-up calls per figure, then the median / min of `calls`",
           "device": {"name": props.name, "arch": getattr(props, "gcnArchName", None),
                      "compute_units": props.multi_processor_count, "hip": torch.version.hip},
           "host": {"machine": platform.machine(), "cpus_available": len(os.sched_getaffinity(0)),
                    "python": platform.python_version(), "numpy": np.__version__},
           "host_arrays": "pageable numpy", "sets": {}}
    for name in args.sets.split(","):
        p = PARAM_SETS[name]
        sk = R.SecretKey.new(p, 1)
        e = R.Engine(p, 0)
        try:
            with_dl = timed(lambda: e.gen_packing_key(sk.key_lv0, sk.key_lv1, rng_key=K), args.reps, torch.cuda.synchronize)
            no_dl = timed(lambda: e.gen_packing_key(sk.key_lv0, sk.key_lv1, rng_key=K, download=False), args.reps,
                          torch.cuda.synchronize)
            pk = e.gen_packing_key(sk.key_lv0, sk.key_lv1, rng_key=K)
        finally:
            e.close()
        host = timed(lambda: make_packing_key(p, sk.key_lv0, sk.key_lv1, rng=K), args.host_reps, lambda: None)
        cpu = make_packing_key(p, sk.key_lv0, sk.key_lv1, rng=K)
        res["sets"][name] = {"rows": p.n * p.iks_t, "key_mb": round(pk.nbytes / 1e6, 2),
                             "gen_packing_key_download": with_dl, "gen_packing_key_no_download": no_dl,
                             "make_packing_key_host": host,
                             "gpu_and_host_seeds_equal": pk.mask_seed == cpu.mask_seed,
                             "gpu_and_host_words_differing": int((pk.bodies != cpu.bodies).sum())}
        print(name, json.dumps(res["sets"][name]), flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
