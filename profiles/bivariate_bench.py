"""Encrypted-table key switch and the tree bootstrap on one GPU, device-resident operands.

(a) tfhe_hip_batch_pack_table_dev of m * count rows against tfhe_hip_batch_pack_tlwe_dev of the same m * count inputs in
    the same process: the contraction is identical, so the ratio isolates the table epilogue and the window.
(b) tfhe_hip_batch_bootstrap_bivariate_dev on SECURITY_UINT4 at (m, k) = (16, 1) and (4, 4), `count` ciphertexts,
    against m / k + 1 plain tfhe_hip_batch_bootstrap_dev launches of the same count in the same run, with the table build
    and one stage-2 (per-ciphertext table) bootstrap launch timed on their own.
The inputs are uniform words (no kernel's work depends on them); one table of every shape is checked against the integer
model before anything is timed.

    python3 profiles/bivariate_bench.py [--reps 5] [--rows 65536] [--count 16384] [--out profiles/bivariate_bench.json]
"""
import argparse
import json
import os
import platform
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from compressed_key_bench import shader_clock, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=65536, help="(a): m * count")
    ap.add_argument("--count", type=int, default=16384, help="(b): ciphertexts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bivariate_bench.json"))
    args = ap.parse_args()
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd.params import N, PARAM_SETS

    props = torch.cuda.get_device_properties(0)
    res = {"clock": "host wall clock (time.perf_counter) around the call + torch.cuda.synchronize(); one warm-up call "
                    "per shape, then the median / min of `reps`",
           "device": {"name": props.name, "arch": getattr(props, "gcnArchName", None),
                      "compute_units": props.multi_processor_count, "hip": torch.version.hip},
           "host": {"machine": platform.machine(), "cpus_available": len(os.sched_getaffinity(0)),
                    "python": platform.python_version(), "numpy": np.__version__, "torch": torch.__version__},
           "reps": args.reps, "table_against_pack": {}, "composite": {}}
    res["device"]["shader_mhz_before"] = shader_clock(R, PARAM_SETS["SECURITY_128_BIT"])
    rng = np.random.default_rng(3)

    def dev_words(rows, width):  # uniform words made on the host in slices (the generator's temporaries stay small)
        t = torch.empty((rows, width), dtype=torch.int32, device="cuda:0")
        for lo in range(0, rows, 8192):
            hi = min(lo + 8192, rows)
            t[lo:hi] = torch.from_numpy(rng.integers(0, 1 << 32, (hi - lo, width), dtype=np.uint64).astype(np.uint32).view(np.int32))
        return t

    # (a) the table build against the packing key switch of the same rows
    for name in ("SECURITY_128_BIT", "SECURITY_UINT4"):
        p = PARAM_SETS[name]
        sk = R.SecretKey.new(p, 1)
        pk = sk.packing_key(rng_key=2)
        rows = args.rows
        e = R.Engine(p, 0)
        try:
            e.load_packing_key(pk)
            d_in = dev_words(rows, p.n + 1)
            d_pack = torch.empty((-(-rows // N), 2, N), dtype=torch.int32, device="cuda:0")
            out = {"rows": rows, "pack_dev": timed(lambda: e.pack_dev(d_in, d_pack), args.reps)}
            for m in (4, 16, 512):
                count = rows // m
                d_tab = torch.empty((count, 2, N), dtype=torch.int32, device="cuda:0")
                e.pack_table_dev(d_in[:m * count], m, d_tab)
                torch.cuda.synchronize()
                s1 = d_in[:m * count].view(m, count, p.n + 1)[:, :2].cpu().numpy().view(np.uint32)
                want = PK.table_model(p, pk.mask_seed, pk.bodies, s1, m)
                assert np.array_equal(d_tab[:2].cpu().numpy().view(np.uint32), want), "table words differ from the model"
                t = timed(lambda: e.pack_table_dev(d_in[:m * count], m, d_tab), args.reps)
                t["over_pack_dev"] = round(t["median_ms"] / out["pack_dev"]["median_ms"], 3)
                out["pack_table_dev_m%d" % m] = t
                del d_tab
            res["table_against_pack"][name] = out
            print(name, json.dumps(out), flush=True)
        finally:
            e.close()
        del d_in, d_pack
        torch.cuda.empty_cache()

    # (b) the composite against its bootstraps
    p = PARAM_SETS["SECURITY_UINT4"]
    sk = R.SecretKey.new(p, 1)
    pk = sk.packing_key(rng_key=2)
    count, w = args.count, p.n + 1
    e = R.Engine(p, 0)
    try:
        e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=5)
        e.load_packing_key(pk)
        d_x, d_y = dev_words(count, w), dev_words(count, w)
        d_out = torch.empty((count, w), dtype=torch.int32, device="cuda:0")
        d_tv1 = dev_words(2, N).view(1, 2, N)
        d_tvs = dev_words(count * 2, N).view(count, 2, N)
        plain = timed(lambda: e.batch_bootstrap_dev(d_y, d_out, testvec=d_tv1), args.reps)
        per_ct = timed(lambda: e.batch_bootstrap_dev(d_x, d_out, testvec=d_tvs, per_ct=True), args.reps)
        res["composite"]["count"] = count
        res["composite"]["batch_bootstrap_dev_one_table"] = plain
        res["composite"]["batch_bootstrap_dev_per_ct_tables"] = per_ct
        for m, k in ((16, 1), (4, 4)):
            d_tabs = dev_words(m // k * 2, N).view(m // k, 2, N)
            launches = m // k + 1
            comp = timed(lambda: e.batch_bootstrap_bivariate_dev(d_x, d_y, d_tabs, m, d_out, n_luts=k), args.reps)

            def plain_launches():
                for _ in range(launches):
                    e.batch_bootstrap_dev(d_y, d_out, testvec=d_tv1)

            base = timed(plain_launches, args.reps)
            d_s1 = dev_words(m * count, w)
            d_tab = torch.empty((count, 2, N), dtype=torch.int32, device="cuda:0")
            table = timed(lambda: e.pack_table_dev(d_s1, m, d_tab), args.reps)
            del d_s1, d_tab
            torch.cuda.empty_cache()
            row = {"m": m, "k": k, "bootstrap_launches": launches, "bivariate_dev": comp,
                   "plain_bootstrap_launches": base, "pack_table_dev": table,
                   "composite_over_plain_launches": round(comp["median_ms"] / base["median_ms"], 3),
                   "table_over_one_per_ct_bootstrap": round(table["median_ms"] / per_ct["median_ms"], 3)}
            res["composite"]["m%d_k%d" % (m, k)] = row
            print(json.dumps(row), flush=True)
    finally:
        e.close()
    res["device"]["shader_mhz_after"] = shader_clock(R, PARAM_SETS["SECURITY_128_BIT"])
    with open(args.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
