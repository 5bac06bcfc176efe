"""The TRLWE key switch on one GPU (tfhe_hip_batch_trlwe_keyswitch_dev), on device buffers, SECURITY_128_BIT, k = 1,
(beta, t) = (4, 6): 1,024 and 16,384 packed ciphertexts.

  whole call    HIP events on the call's stream around one call (torch.cuda.Event), one warm-up call, then the median of
                `reps` calls.
  its two steps the library's own event pairs around the digits kernel and around the contraction of every pass
                (tfhe_hip_get_trlwe_switch_times, profiling on), summed over the passes of a call: the median of `reps`
                further calls.  Their sum is below the whole call's time by the gaps between launches.
  baseline      tfhe_hip_batch_reencrypt_dev, the per-value route, on the same number of VALUES: 1,024 x as many lv0
                ciphertexts.  2^24 of them would be 47 GB each way, so both cases run as back-to-back calls on the same
                buffers of 2^18 ciphertexts (0.7 GB each way) between one pair of events: 4 calls and 64 calls.

The shader clock is sampled before and after (compressed_key_bench.shader_clock).  The switch's result is checked against
the numpy model (tests/trlwe_switch_model.py) on the first three ciphertexts before anything is timed.

    python3 profiles/trlwe_switch_bench.py [--reps 7] [--out profiles/trlwe_switch_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from compressed_key_bench import shader_clock  # noqa: E402
from conv2d_bench import summary  # noqa: E402
from matmul_bench import MFMA_INT8_TOPS, rate  # noqa: E402

K = bytes((53 * i + 7) & 0xFF for i in range(32))
COUNTS = (1024, 16384)
LWE_PER_CALL = 1 << 18


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trlwe_switch_bench.json"))
    args = ap.parse_args()
    import torch

    import rs_tfhe_amd as R
    import trlwe_switch_model as TM
    from rs_tfhe_amd.params import N, SECURITY_128_BIT as p

    basebit, t, k = 4, 6, 1
    props = torch.cuda.get_device_properties(0)
    res = {"clock": "HIP events on the call's stream (torch.cuda.Event.elapsed_time) around each call; the steps from the "
                    "library's event pairs around each kernel (tfhe_hip_get_trlwe_switch_times); one warm-up call, then the "
                    "median of `reps`; operands and results in device memory",
           "device": {"name": props.name, "arch": getattr(props, "gcnArchName", None),
                      "compute_units": props.multi_processor_count, "hip": torch.version.hip},
           "host": {"machine": platform.machine(), "cpus_available": len(os.sched_getaffinity(0)),
                    "python": platform.python_version(), "numpy": np.__version__, "torch": torch.__version__},
           "set": p.name, "k": k, "basebit": basebit, "t": t, "reps": args.reps, "matrix_core_int8_tops": MFMA_INT8_TOPS}
    res["device"]["shader_mhz_before"] = shader_clock(R, p)
    rng = np.random.default_rng(1)
    alice, bob = R.SecretKey.new(p, 3), R.SecretKey.new(p, 4)
    stream = torch.cuda.Stream(device=0)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    e, lwe = R.Engine(p, 0), R.Engine(p, 0)
    try:
        key = e.gen_trlwe_switch_key(alice.key_lv1, bob.key_lv1, k, basebit, t, rng_key=K)
        lwe.gen_reenc_key_symmetric(alice.key_lv0, bob.key_lv0, rng_key=K, download=False)
        cts = torch.from_numpy(rng.integers(0, 1 << 32, (LWE_PER_CALL, p.n + 1), dtype=np.uint64).astype(np.uint32).view(np.int32)).to("cuda:0")
        cts_out = torch.empty_like(cts)
        out = {}
        for count in COUNTS:
            host_in = rng.integers(0, 1 << 32, (count, 2, N), dtype=np.uint64).astype(np.uint32)
            tin = torch.from_numpy(host_in.view(np.int32)).to("cuda:0")
            tout = torch.full(tin.shape, -1, dtype=torch.int32, device="cuda:0")
            calls = count * N // LWE_PER_CALL

            def switch():
                e.batch_trlwe_keyswitch(k, tin, out=tout, stream=stream)

            def baseline():
                for _ in range(calls):
                    lwe.batch_reencrypt_dev(cts, cts_out, stream=stream)

            switch()  # (the warm-up calls)
            baseline()
            stream.synchronize()
            want = TM.switch(TM.key_rows(key.mask_seed, k, t, key.bodies), k, basebit, t, host_in[:3])
            assert np.array_equal(tout[:3].cpu().numpy().view(np.uint32), want), "the switch differs from the model"
            whole, base = [], []
            for _ in range(args.reps):  # the routes alternate: a drift of the clocks meets both alike
                whole.append(timed(switch))
                base.append(timed(baseline))
            e.set_profiling(True)
            e.trlwe_switch_times()
            dig, mm = [], []
            for _ in range(args.reps):
                switch()
                ev = e.trlwe_switch_times()
                dig.append(ev["digits_ms"])
                mm.append(ev["contraction_ms"])
                passes = ev["passes"]
            e.set_profiling(False)
            ops = 8 * count * t * N * 2 * N  # 2 K x columns x 4 byte planes per row, K = t N
            r = {"whole_call": summary(whole), "digits_pass": summary(dig), "contraction": summary(mm), "passes": passes,
                 "in_bytes": tin.numel() * 4, "scratch_bytes": min(count, 2048) * (t * N + 4 * N), "int8_ops": ops,
                 "reencrypt_dev_same_values": {**summary(base), "lwe_ciphertexts": count * N, "calls": calls,
                                               "lwe_bytes_each_way": count * N * (p.n + 1) * 4}}
            r["contraction"].update(rate(r["contraction"]["median_ms"], ops))
            r["whole_call"].update(rate(r["whole_call"]["median_ms"], ops))
            r["us_per_ciphertext"] = round(r["whole_call"]["median_ms"] * 1e3 / count, 3)
            r["ns_per_value"] = round(r["whole_call"]["median_ms"] * 1e6 / (count * N), 3)
            r["reencrypt_ns_per_value"] = round(r["reencrypt_dev_same_values"]["median_ms"] * 1e6 / (count * N), 3)
            r["reencrypt_over_switch_time"] = round(r["reencrypt_dev_same_values"]["median_ms"] / r["whole_call"]["median_ms"], 1)
            r["digits_share_of_steps"] = round(r["digits_pass"]["median_ms"] / (r["digits_pass"]["median_ms"] + r["contraction"]["median_ms"]), 4)
            out[str(count)] = r
            print(json.dumps({count: r}), flush=True)
            del tin, tout
        res["counts"] = out
    finally:
        e.close()
        lwe.close()
    res["device"]["shader_mhz_after"] = shader_clock(R, p)
    with open(args.out, "w") as fh:
        json.dump(res, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
