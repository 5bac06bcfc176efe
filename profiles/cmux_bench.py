"""The packed CMUX on one GPU (tfhe_hip_batch_trlwe_cmux_dev), on device buffers, SECURITY_128_BIT, at (beta, t) = (6, 3)
and (4, 6): 64, 1,024 and 16,384 pairs under one selector.

  whole call     HIP events on the call's stream around one call (torch.cuda.Event), one warm-up call, then the median
                 of `reps` calls.
  its steps      the library's own event pairs around the digits kernel, the contraction and the addend kernel of every
                 pass (tfhe_hip_get_cmux_times, profiling on), summed over the passes of a call: the median of `reps`
                 further calls.  Their sum is below the whole call's time by the gaps between launches.
  yardstick 1    tfhe_hip_batch_trlwe_keyswitch_dev at the same (beta, t) and count, between the same events, the two
                 routes alternating.  The CMUX contracts twice the columns and adds two light passes: about twice the
                 switch's time is the expectation.
  yardstick 2    tfhe_hip_batch_external_product, the f64 FFT stage kernel under a bootstrapping-key row, the only other
                 external product in the tree, at (6, 3) on the same count.  It has a host form only, so it is timed by
                 the host's clock around the call, staging included -- and so is the CMUX's host form beside it.

The shader clock is sampled before and after (compressed_key_bench.shader_clock).  The CMUX's result is checked against
the numpy model (tests/cmux_model.py) on the first three pairs before anything is timed.

    python3 profiles/cmux_bench.py [--reps 7] [--out profiles/cmux_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "profiles"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from compressed_key_bench import shader_clock  # noqa: E402
from conv2d_bench import summary  # noqa: E402
from matmul_bench import MFMA_INT8_TOPS, rate  # noqa: E402

K = bytes((53 * i + 7) & 0xFF for i in range(32))
SHAPES = ((6, 3), (4, 6))
COUNTS = (64, 1024, 16384)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmux_bench.json"))
    args = ap.parse_args()
    import torch

    import cmux_model as CM
    import rs_tfhe_amd as R
    from rs_tfhe_amd.params import N, SECURITY_128_BIT as p

    props = torch.cuda.get_device_properties(0)
    res = {"clock": "HIP events on the call's stream (torch.cuda.Event.elapsed_time) around each call; the steps from the "
                    "library's event pairs around each kernel (tfhe_hip_get_cmux_times); one warm-up call, then the median of "
                    "`reps`; operands and results in device memory.  The host forms: time.perf_counter around the call",
           "device": {"name": props.name, "arch": getattr(props, "gcnArchName", None),
                      "compute_units": props.multi_processor_count, "hip": torch.version.hip},
           "host": {"machine": platform.machine(), "cpus_available": len(os.sched_getaffinity(0)),
                    "python": platform.python_version(), "numpy": np.__version__, "torch": torch.__version__},
           "set": p.name, "reps": args.reps, "matrix_core_int8_tops": MFMA_INT8_TOPS}
    res["device"]["shader_mhz_before"] = shader_clock(R, p)
    rng = np.random.default_rng(1)
    sk = R.SecretKey.new(p, 3)
    stream = torch.cuda.Stream(device=0)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    e = R.Engine(p, 0)
    try:
        e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=5)  # (the FFT stage kernel's rows; the CMUX needs no key)
        out = {}
        for basebit, t in SHAPES:
            sel = e.batch_encrypt_trgsw(sk.key_lv1, np.eye(1, N, 0, dtype=np.int32), basebit, t, rng_key=K)[0]
            tsel = torch.from_numpy(sel.view(np.int32)).to("cuda:0")
            e.gen_trlwe_switch_key(sk.key_lv1, sk.key_lv1, 1, basebit, t, rng_key=K, download=False)
            for count in COUNTS:
                h0 = rng.integers(0, 1 << 32, (count, 2, N), dtype=np.uint64).astype(np.uint32)
                h1 = rng.integers(0, 1 << 32, (count, 2, N), dtype=np.uint64).astype(np.uint32)
                t0, t1 = (torch.from_numpy(h.view(np.int32)).to("cuda:0") for h in (h0, h1))
                tout = torch.full(t1.shape, -1, dtype=torch.int32, device="cuda:0")

                def cmux():
                    e.batch_trlwe_cmux(tsel, basebit, t, t0, t1, out=tout, stream=stream)

                def switch():
                    e.batch_trlwe_keyswitch(1, t1, out=tout, stream=stream)

                cmux()  # (the warm-up calls; the CMUX last: its result is checked)
                switch()
                cmux()
                stream.synchronize()
                want = CM.cmux(sel, basebit, t, h0[:3], h1[:3])
                assert np.array_equal(tout[:3].cpu().numpy().view(np.uint32), want), "the CMUX differs from the model"
                whole, sw = [], []
                for _ in range(args.reps):  # the routes alternate: a drift of the clocks meets both alike
                    whole.append(timed(cmux))
                    sw.append(timed(switch))
                e.set_profiling(True)
                e.cmux_times()
                dig, mm, add = [], [], []
                for _ in range(args.reps):
                    cmux()
                    ev = e.cmux_times()
                    dig.append(ev["digits_ms"])
                    mm.append(ev["contraction_ms"])
                    add.append(ev["addend_ms"])
                    passes = ev["passes"]
                e.set_profiling(False)
                rows = -(-count // 64) * 64  # the GEMM works on whole 64-row tiles
                ops = 8 * count * 2 * t * N * 2 * N  # 2 K x columns x 4 byte planes per row, K = 2t N
                r = {"whole_call": summary(whole), "digits_pass": summary(dig), "contraction": summary(mm), "addend": summary(add),
                     "passes": passes, "in_bytes": 2 * t1.numel() * 4, "scratch_bytes": min(count, 2048) * 2 * t * N,
                     "int8_ops": ops, "tile_rows": rows, "trlwe_keyswitch_dev_same_shape": summary(sw)}
                r["contraction"].update(rate(r["contraction"]["median_ms"], ops))
                r["whole_call"].update(rate(r["whole_call"]["median_ms"], ops))
                r["us_per_pair"] = round(r["whole_call"]["median_ms"] * 1e3 / count, 3)
                r["cmux_over_switch_time"] = round(r["whole_call"]["median_ms"] / r["trlwe_keyswitch_dev_same_shape"]["median_ms"], 3)
                steps = r["digits_pass"]["median_ms"] + r["contraction"]["median_ms"] + r["addend"]["median_ms"]
                r["share_of_steps"] = {k: round(r[k]["median_ms"] / steps, 4) for k in ("digits_pass", "contraction", "addend")}
                if (basebit, t) == (6, 3):
                    idx = np.zeros(count, np.int32)
                    with np.errstate(over="ignore"):
                        x = h1 - h0
                    e.batch_external_product(x[:1], idx[:1])
                    fft = [wall(lambda: e.batch_external_product(x, idx)) for _ in range(args.reps)]
                    e.batch_trlwe_cmux(sel, basebit, t, None, x[:1])
                    own = [wall(lambda: e.batch_trlwe_cmux(sel, basebit, t, None, x)) for _ in range(args.reps)]
                    r["fft_external_product_host_form"] = summary(fft)
                    r["cmux_external_product_host_form"] = summary(own)
                    r["fft_over_cmux_host_form_time"] = round(float(np.median(fft)) / float(np.median(own)), 3)
                out[f"{basebit},{t},{count}"] = r
                print(json.dumps({f"({basebit}, {t}) x {count}": r}), flush=True)
                del t0, t1, tout
            e.drop_trlwe_switch_key(1)
        res["cases"] = out
    finally:
        e.close()
    res["device"]["shader_mhz_after"] = shader_clock(R, p)
    with open(args.out, "w") as fh:
        json.dump(res, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
