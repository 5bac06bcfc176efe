#!/usr/bin/env python3
"""Many-LUT bootstrap timing on one GPU, SECURITY_UINT4: k = 2 functions of 65,536 inputs from one blind rotation
(tfhe_hip_batch_lincomb_bootstrap_many) against two single-LUT calls (tfhe_hip_batch_lincomb_bootstrap), host-array
and device (_dev) forms, alternating after a warm-up; then one batch of the base-4 digit adder
(circuit.lut_add_u8_digits, 4 blind rotations per byte) against the same adder built from single-LUT bootstraps
(8 per byte).

    python profiles/many_lut_bench.py [--count 65536] [--reps 5] [--adder-batch 4096] [--out FILE]

Prints one JSON object: median / min wall time per form (host clock around the call + torch.cuda.synchronize()) and
function evaluations per second (k * count / time).  The words are checked by tests/test_gpu_many_lut.py; this only
times them."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5, help="timed calls per form (alternating)")
    ap.add_argument("--adder-batch", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import rs_tfhe_amd as R
    from oracle import oracle as O
    from rs_tfhe_amd.circuit import lut_add_u8_digits

    sk, ock = O.keygen(O.SECURITY_UINT4, 12)
    P = R.params.SECURITY_UINT4
    ck = R.CloudKey(P, ock.bootstrapping_key, ock.key_switching_key, ock.decomposition_offset, ock.blind_rotate_testvec)
    eng = R.Engine(P, 0)
    eng.load_cloud_key(ck)
    n, w = args.count, P.n + 1
    rng = np.random.default_rng(3)
    a = sk.encrypt_lwe_message(rng.integers(0, 8, n), 8, 31)
    b = sk.encrypt_lwe_message(rng.integers(0, 8, n), 8, 32)
    gen = R.lut.Generator(8)
    fs = [lambda x: x % 4, lambda x: x // 4]
    tv2 = gen.generate_many_lookup_table(fs).poly
    tv_s, tv_c = (gen.generate_lookup_table(f).poly for f in fs)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to("cuda:0")  # noqa: E731
    da, db, dtv2, dts, dtc = dev(a), dev(b), dev(tv2), dev(tv_s), dev(tv_c)
    out2 = torch.empty((2 * n, w), dtype=torch.int32, device="cuda:0")
    out1 = torch.empty((2 * n, w), dtype=torch.int32, device="cuda:0")

    forms = {
        "many_host": lambda: eng.batch_lincomb_bootstrap_many(1, a, 1, b, 0, tv2, n_luts=2),
        "single_x2_host": lambda: (eng.batch_lincomb_bootstrap(1, a, 1, b, 0, testvec=tv_s),
                                   eng.batch_lincomb_bootstrap(1, a, 1, b, 0, testvec=tv_c)),
        "many_dev": lambda: eng.batch_lincomb_bootstrap_many_dev(1, da, 1, db, 0, out2, dtv2, n_luts=2),
        "single_x2_dev": lambda: (eng.batch_lincomb_bootstrap_dev(1, da, 1, db, 0, out1[:n], testvec=dts),
                                  eng.batch_lincomb_bootstrap_dev(1, da, 1, db, 0, out1[n:], testvec=dtc)),
    }

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for fn in forms.values():  # warm-up
        timed(fn)
    ms = {k: [] for k in forms}
    for _ in range(args.reps):
        for k, fn in forms.items():
            ms[k].append(timed(fn))
    res = {"params": "SECURITY_UINT4", "count": n, "n_luts": 2, "reps": args.reps,
           "clock": "host wall clock (time.perf_counter) around the call + torch.cuda.synchronize()", "forms": {}}
    for k, v in ms.items():
        med = statistics.median(v)
        res["forms"][k] = {"median_ms": round(med, 3), "min_ms": round(min(v), 3),
                           "evals_per_s": round(2 * n / (med / 1e3), 1)}
    for form in ("host", "dev"):
        res[f"speedup_{form}"] = round(res["forms"][f"single_x2_{form}"]["median_ms"] / res["forms"][f"many_{form}"]["median_ms"], 3)

    B = args.adder_batch
    xa, xb = rng.integers(0, 256, B), rng.integers(0, 256, B)
    digits = [(xa >> (2 * i)) & 3 for i in range(4)] + [(xb >> (2 * i)) & 3 for i in range(4)]
    ins = np.stack([sk.encrypt_lwe_message(d, 8, 40 + i) for i, d in enumerate(digits)])
    adders = {}
    for k in (2, 1):
        c = R.Circuit(8)
        lut_add_u8_digits(c, list(range(4)), list(range(4, 8)), n_luts=k)
        adders[k] = c
    dins = dev(ins)
    for c in adders.values():
        timed(lambda: c.run_dev(eng, dins))
    am = {1: [], 2: []}
    for _ in range(args.reps):
        for k, c in adders.items():
            am[k].append(timed(lambda: c.run_dev(eng, dins)))
    res["digit_adder"] = {"batch": B, "many_lut_median_ms": round(statistics.median(am[2]), 3),
                          "single_lut_median_ms": round(statistics.median(am[1]), 3),
                          "lut_nodes": {"many": sum(lv["lut_nodes"] for lv in adders[2].describe()),
                                        "single": sum(lv["lut_nodes"] for lv in adders[1].describe())}}
    res["digit_adder"]["speedup"] = round(statistics.median(am[1]) / statistics.median(am[2]), 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
