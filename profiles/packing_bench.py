"""Packing key switch on one GPU (tfhe_hip_batch_pack_tlwe_dev): the time to pack 65,536 device-resident lv0 results and
one group of N = 1024, and the host download of the packed TRLWEs against the download of the unpacked results, on
SECURITY_128_BIT and SECURITY_UINT4.  The inputs are uniform words (the kernel's work does not depend on them); the
first group is checked against the integer model before anything is timed.

    python3 profiles/packing_bench.py [--reps 5] [--out profiles/packing_bench.json]
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
    ap.add_argument("--count", type=int, default=65536)
    ap.add_argument("--sets", default="SECURITY_128_BIT,SECURITY_UINT4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packing_bench.json"))
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
           "reps": args.reps, "count": args.count, "sets": {}}
    res["device"]["shader_mhz_before"] = shader_clock(R, PARAM_SETS["SECURITY_128_BIT"])
    for name in args.sets.split(","):
        p = PARAM_SETS[name]
        sk = R.SecretKey.new(p, 1)
        pk = sk.packing_key(rng_key=2)
        cts = np.random.default_rng(3).integers(0, 1 << 32, (args.count, p.n + 1), dtype=np.uint64).astype(np.uint32)
        groups = -(-args.count // N)
        e = R.Engine(p, 0)
        try:
            load = timed(lambda: e.load_packing_key(pk), args.reps)
            d_in = torch.from_numpy(cts.view(np.int32)).to("cuda:0")
            d_out = torch.empty((groups, 2, N), dtype=torch.int32, device="cuda:0")
            e.pack_dev(d_in[:N], d_out[:1])
            torch.cuda.synchronize()
            want = PK.pack_model(p, pk.mask_seed, pk.bodies, cts[:N])
            assert np.array_equal(d_out[:1].cpu().numpy().view(np.uint32), want), "packed words differ from the model"
            batch = timed(lambda: e.pack_dev(d_in, d_out), args.reps)
            one = timed(lambda: e.pack_dev(d_in[:N], d_out[:1]), args.reps)
            down_packed = timed(lambda: d_out.cpu(), args.reps)
            down_full = timed(lambda: d_in.cpu(), args.reps)
            host = timed(lambda: e.pack(cts), args.reps)
        finally:
            e.close()
        res["sets"][name] = {
            "packing_key_mb": round(pk.nbytes / 1e6, 2), "load_packing_key": load,
            "pack_dev": batch, "pack_dev_one_group": one, "pack_host_arrays": host,
            "packed_bytes": groups * 2 * N * 4, "unpacked_bytes": cts.nbytes,
            "download_packed": down_packed, "download_unpacked": down_full,
            "int8_ops": 2 * 4 * args.count * p.n * p.iks_t * 2 * N,
        }
        print(name, json.dumps(res["sets"][name]), flush=True)
    res["device"]["shader_mhz_after"] = shader_clock(R, PARAM_SETS["SECURITY_128_BIT"])
    with open(args.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
