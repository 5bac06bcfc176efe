"""Unpacking key switch on one GPU (tfhe_hip_batch_unpack_trlwe_dev): the time to turn 65,536 slots, and one group of
N = 1024, of device-resident TRLWE lv1 ciphertexts back into lv0 ciphertexts, on SECURITY_128_BIT and SECURITY_UINT4.
In the same run: the key-switch time of a 65,536-row gate batch from tfhe_hip_get_kernel_times (the yardstick: the
unpacking call is that key switch plus the extraction that feeds it) and the staged upload of the unpacked ciphertexts
that a packed input replaces.  The inputs are uniform words (the kernels' work does not depend on them); the first
group is checked against the integer model before anything is timed.

    python3 profiles/unpack_bench.py [--reps 5] [--out profiles/unpack_bench.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unpack_bench.json"))
    args = ap.parse_args()
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd.engine import NAND
    from rs_tfhe_amd.params import N, PARAM_SETS

    props = torch.cuda.get_device_properties(0)
    res = {"clock": "host wall clock (time.perf_counter) around the call + torch.cuda.synchronize(); one warm-up call "
                    "per shape, then the median / min of `reps`; key_switch_ms: the library's event pairs around the "
                    "key-switch launches (tfhe_hip_get_kernel_times), median of `reps`",
           "device": {"name": props.name, "arch": getattr(props, "gcnArchName", None),
                      "compute_units": props.multi_processor_count, "hip": torch.version.hip},
           "host": {"machine": platform.machine(), "cpus_available": len(os.sched_getaffinity(0)),
                    "python": platform.python_version(), "numpy": np.__version__, "torch": torch.__version__},
           "reps": args.reps, "count": args.count, "sets": {}}
    res["device"]["shader_mhz_before"] = shader_clock(R, PARAM_SETS["SECURITY_128_BIT"])
    for name in args.sets.split(","):
        p = PARAM_SETS[name]
        sk = R.SecretKey.new(p, 1)
        groups = -(-args.count // N)
        rng = np.random.default_rng(3)
        trlwe = rng.integers(0, 1 << 32, (groups, 2, N), dtype=np.uint32)
        cts = rng.integers(0, 1 << 32, (args.count, p.n + 1), dtype=np.uint32)
        e = R.Engine(p, 0)
        try:
            e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=2)
            ksk = e.export_cloud_key().key_switching_key
            d_in = torch.from_numpy(trlwe.view(np.int32)).to("cuda:0")
            d_out = torch.empty((args.count, p.n + 1), dtype=torch.int32, device="cuda:0")
            d_slots = torch.from_numpy(rng.permutation(args.count).astype(np.uint32).view(np.int32)).to("cuda:0")
            e.unpack_dev(d_in[:1], d_out[:N], N)
            torch.cuda.synchronize()
            want = PK.unpack_model(p, ksk, trlwe[:1], 64)
            assert np.array_equal(d_out[:64].cpu().numpy().view(np.uint32), want), "unpacked words differ from the model"

            def ks_ms(run):
                """median key-switch milliseconds of `run` over reps, from the library's own events"""
                e.set_profiling(True)
                run()
                torch.cuda.synchronize()
                e.kernel_times()  # (the warm-up's)
                ms = []
                for _ in range(args.reps):
                    run()
                    torch.cuda.synchronize()
                    ms.append(e.kernel_times()["key_switch_ms"])
                e.set_profiling(False)
                return float(np.median(ms))

            batch = timed(lambda: e.unpack_dev(d_in, d_out, args.count), args.reps)
            picked = timed(lambda: e.unpack_dev(d_in, d_out, args.count, slots=d_slots), args.reps)
            one = timed(lambda: e.unpack_dev(d_in[:1], d_out[:N], N), args.reps)
            ks_unpack = ks_ms(lambda: e.unpack_dev(d_in, d_out, args.count))
            d_a = torch.from_numpy(cts.view(np.int32)).to("cuda:0")
            ks_gate = ks_ms(lambda: e.batch_gate_dev(NAND, d_a, d_a, d_out))
            up_full = timed(lambda: torch.from_numpy(cts.view(np.int32)).to("cuda:0"), args.reps)
            up_packed = timed(lambda: torch.from_numpy(trlwe.view(np.int32)).to("cuda:0"), args.reps)
            host = timed(lambda: e.unpack(trlwe, args.count), args.reps)
        finally:
            e.close()
        res["sets"][name] = {
            "unpack_dev": batch, "unpack_dev_permuted_slots": picked, "unpack_dev_one_group": one, "unpack_host_arrays": host,
            "key_switch_ms_inside_unpack_dev": ks_unpack, "key_switch_ms_of_gate_batch": ks_gate,
            "packed_bytes": int(trlwe.nbytes), "unpacked_bytes": int(cts.nbytes),
            "upload_unpacked": up_full, "upload_packed": up_packed,
            "lv1_scratch_bytes_written_and_read": args.count * (N + 1) * 4,
        }
        print(name, json.dumps(res["sets"][name]), flush=True)
    res["device"]["shader_mhz_after"] = shader_clock(R, PARAM_SETS["SECURITY_128_BIT"])
    with open(args.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
