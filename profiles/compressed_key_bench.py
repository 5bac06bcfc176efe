"""Seeded (compressed) cloud keys on one GPU: wall time of loading a full key (tfhe_hip_load_cloud_key) against loading
its compressed form (tfhe_hip_load_compressed_cloud_key), both from pageable host arrays, on SECURITY_128_BIT, UINT4
and UINT8; the times of tfhe_hip_gen_cloud_key_with_key and tfhe_hip_gen_compressed_cloud_key; and expanding 65,536 seeded SECURITY_128_BIT ciphertexts on
the device (tfhe_hip_expand_seeded_tlwe_dev) against staging the full batch from the host.

    python3 profiles/compressed_key_bench.py [--reps 5] [--out profiles/compressed_key_bench.json]
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


def timed(fn, reps):
    """One untimed warm-up call (first launch of the kernels, buffers allocated), then `reps` timed calls."""
    import torch

    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(np.min(ts)), 3)}


def shader_clock(R, p):
    """Shader clock (MHz) a 4,096-gate batch ran at, from the library's in-kernel clock sample: the clock state of the
    device around the measurements."""
    e = R.Engine(p, 0)
    try:
        sk = R.SecretKey.new(p, 9)
        e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=9)
        cts = sk.encrypt_bool(np.arange(4096) % 2 == 0, seed=1)
        e.set_profiling(True)
        e.batch_gate(0, cts, cts)
        return round(e.clock_sample()["shader_mhz"], 1)
    finally:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sets", default="SECURITY_128_BIT,SECURITY_UINT4,SECURITY_UINT8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compressed_key_bench.json"))
    args = ap.parse_args()
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd.params import PARAM_SETS

    props = torch.cuda.get_device_properties(0)
    res = {"clock": "host wall clock (time.perf_counter) around the call + torch.cuda.synchronize(); one warm-up call "
                    "per shape, then the median / min of `reps`",
           "device": {"name": props.name, "arch": getattr(props, "gcnArchName", None),
                      "compute_units": props.multi_processor_count, "memory_gb": round(props.total_memory / 2 ** 30, 1),
                      "hip": torch.version.hip},
           "host": {"machine": platform.machine(), "cpus_available": len(os.sched_getaffinity(0)),
                    "python": platform.python_version(), "numpy": np.__version__, "torch": torch.__version__},
           "reps": args.reps, "host_arrays": "pageable numpy", "sets": {}}
    res["device"]["shader_mhz_before"] = shader_clock(R, PARAM_SETS["SECURITY_128_BIT"])
    for name in args.sets.split(","):
        p = PARAM_SETS[name]
        sk = R.SecretKey.new(p, 1)
        e = R.Engine(p, 0)
        try:
            gen_plain = timed(lambda: e.gen_cloud_key(sk.key_lv0, sk.key_lv1, rng_key=bytes(32)), args.reps)
            gen = timed(lambda: e.gen_compressed_cloud_key(sk.key_lv0, sk.key_lv1, rng_key=bytes(32)), args.reps)
            ck = e.gen_compressed_cloud_key(sk.key_lv0, sk.key_lv1, rng_key=bytes(32))
            full = e.export_cloud_key()
            full_bytes = full.bootstrapping_key.nbytes + full.key_switching_key.nbytes
            load_full = timed(lambda: e.load_cloud_key(full), args.reps)
            load_comp = timed(lambda: e.load_compressed_cloud_key(ck), args.reps)
        finally:
            e.close()
        res["sets"][name] = {"full_mb": round(full_bytes / 1e6, 2), "compressed_mb": round(ck.nbytes / 1e6, 2),
                             "gen_cloud_key": gen_plain, "gen_compressed": gen, "load_cloud_key": load_full, "load_compressed_cloud_key": load_comp,
                             "load_speedup": round(load_full["median_ms"] / load_comp["median_ms"], 2)}
        del full
        print(name, json.dumps(res["sets"][name]), flush=True)
    # seeded inputs: 65,536 SECURITY_128_BIT ciphertexts
    p = PARAM_SETS["SECURITY_128_BIT"]
    sk = R.SecretKey.new(p, 2)
    count = 65536
    sc = sk.encrypt_bool_seeded(np.arange(count) % 2 == 0, mask_seed=bytes(range(32)), seed=3)
    full_batch = sc.expand()
    e = R.Engine(p, 0)
    try:
        out = torch.empty((count, p.n + 1), dtype=torch.int32, device="cuda:0")
        host_bodies = torch.from_numpy(sc.bodies.view(np.int32))
        host_full = torch.from_numpy(full_batch.view(np.int32))

        def seeded():
            e.expand_seeded_dev(sc.mask_seed, sc.first_index, host_bodies.to("cuda:0"), out)

        def staged():
            out.copy_(host_full.to("cuda:0"))

        seeded_t, staged_t = timed(seeded, args.reps), timed(staged, args.reps)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), full_batch)
        seeded()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), full_batch)
    finally:
        e.close()
    res["seeded_inputs"] = {"params": p.name, "count": count, "seeded_bytes": sc.nbytes, "full_bytes": full_batch.nbytes,
                            "upload_bodies_and_expand_dev": seeded_t, "stage_full_batch": staged_t,
                            "speedup": round(staged_t["median_ms"] / seeded_t["median_ms"], 2)}
    print(json.dumps(res["seeded_inputs"]), flush=True)
    res["device"]["shader_mhz_after"] = shader_clock(R, PARAM_SETS["SECURITY_128_BIT"])
    with open(args.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
