"""Plaintext polynomial products on packed ciphertexts on one GPU (tfhe_hip_batch_trlwe_polymul_dev), on device buffers:

  1. packed_conv: the packed counterpart of profiles/conv2d_bench.py -- 16 images of 1 x 32 x 32 values, each ONE TRLWE,
     32 filters of 3 x 3 (linear.conv2d_packed_plan: rows = 32, cols = 1, groups = 16, 900 outputs a filter) -- beside
     the route the library had for a packed input: tfhe_hip_batch_trlwe_matmul_dev(keyswitch = 0) with every filter
     expanded into one weight row per output position (28,800 rows of 1,024 weights), which returns one lv1 row of
     N + 1 words per output.  Time and output bytes of both.
  2. dense_32x32: rows = cols = 32, groups = 64: a half-filled 64-row tile and K = 32,768.  Useful int8 operations,
     2 * rows * cols * N * 2N * groups * 4 byte planes, against the random x random row of profiles/exp/ubench_mfma.hip.
  3. monomial: one X^k on one ciphertext: the call's floor.

The routes alternate within each repetition, so that a drift of the clocks meets all of them alike.  Every result is
checked before anything is timed: the products against linear.polymul_model on group 0, and the two routes of 1.
against each other (the exact lv1 extraction of an output's slot of the product IS the expanded matmul's row).

    python3 profiles/polymul_bench.py [--reps 5] [--out profiles/polymul_bench.json]
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

from compressed_key_bench import shader_clock  # noqa: E402
from conv2d_bench import summary  # noqa: E402
from matmul_bench import MFMA_INT8_TOPS, rate  # noqa: E402

DENSE_MATMUL_SHARE = 0.1865  # profiles/matmul_bench.json: rows = cols = 1024, 64 groups


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polymul_bench.json"))
    args = ap.parse_args()
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd import linear as L
    from rs_tfhe_amd.params import N, SECURITY_128_BIT as p

    def dev(a):
        return torch.from_numpy(a.view(np.int8 if a.dtype == np.int8 else np.int32)).to("cuda:0")

    props = torch.cuda.get_device_properties(0)
    res = {"clock": "host wall clock (time.perf_counter) around each call + torch.cuda.synchronize(); one warm-up call of "
                    "every route, then `reps` repetitions in which the routes alternate; operands and results in device "
                    "memory",
           "device": {"name": props.name, "arch": getattr(props, "gcnArchName", None),
                      "compute_units": props.multi_processor_count, "hip": torch.version.hip},
           "host": {"machine": platform.machine(), "cpus_available": len(os.sched_getaffinity(0)),
                    "python": platform.python_version(), "numpy": np.__version__, "torch": torch.__version__},
           "set": p.name, "reps": args.reps, "matrix_core_int8_tops": MFMA_INT8_TOPS,
           "dense_matmul_share_of_matrix_core_rate": DENSE_MATMUL_SHARE}
    res["device"]["shader_mhz_before"] = shader_clock(R, p)
    rng = np.random.default_rng(1)
    e = R.Engine(p, 0)  # no key: no route needs one
    try:
        # 1. the packed convolution and the expanded matmul
        in_h = in_w = 32
        k, out_c, groups = 3, 32, 16
        plan = L.conv2d_packed_plan(1, in_h, in_w, k, k)
        positions = plan.slots.size
        f = rng.integers(-128, 128, (out_c, k, k, 1)).astype(np.int8)
        wp = L.conv2d_packed_weights(f, plan)                                   # [32][1][N]
        slots = plan.slots.reshape(-1).astype(np.int64)
        wx = np.zeros((out_c, positions, N), np.int8)                            # row (oc, pos): w'[j] = wp[slot - j]
        for m in np.flatnonzero(wp.any(axis=(0, 1))):
            wx[:, np.arange(positions), slots - m] = wp[:, 0, m][:, None]
        wx = wx.reshape(out_c * positions, N)
        maps = rng.integers(0, 1 << 32, (groups, 1, 2, N), dtype=np.uint64).astype(np.uint32)
        t_wp, t_wx, t_maps = dev(wp), dev(wx), dev(maps)
        o_pm = torch.full((groups, out_c, 2, N), -1, dtype=torch.int32, device="cuda:0")
        o_mm = torch.full((groups, out_c * positions, N + 1), -2, dtype=torch.int32, device="cuda:0")

        def packed_conv():
            e.batch_trlwe_polymul_dev(t_wp, t_maps, o_pm)

        def expanded_matmul():
            e.batch_trlwe_matmul_dev(t_wx, t_maps.view(groups, 2, N), o_mm, keyswitch=False)

        # 2. a half-filled tile, K = 32,768
        rows2 = cols2 = 32
        groups2 = 64
        w2 = rng.integers(-128, 128, (rows2, cols2, N)).astype(np.int8)
        in2 = rng.integers(0, 1 << 32, (groups2, cols2, 2, N), dtype=np.uint64).astype(np.uint32)
        t_w2, t_in2 = dev(w2), dev(in2)
        o_2 = torch.full((groups2, rows2, 2, N), -1, dtype=torch.int32, device="cuda:0")

        def dense_32x32():
            e.batch_trlwe_polymul_dev(t_w2, t_in2, o_2)

        # 3. one monomial on one ciphertext
        t_w3 = dev(L.monomial(17).reshape(1, 1, N))
        o_3 = torch.full((1, 1, 2, N), -1, dtype=torch.int32, device="cuda:0")

        def monomial():
            e.batch_trlwe_polymul_dev(t_w3, t_maps[:1], o_3)

        routes = {"packed_conv_polymul_dev": packed_conv, "expanded_trlwe_matmul_dev": expanded_matmul,
                  "dense_32x32_polymul_dev": dense_32x32, "monomial_polymul_dev": monomial}
        for fn in routes.values():  # (the warm-up calls)
            fn()
        torch.cuda.synchronize()
        got = o_pm[:1].cpu().numpy().view(np.uint32)
        assert np.array_equal(got, L.polymul_model(wp, maps[:1])), "packed convolution differs from the model"
        for oc in (0, out_c - 1):  # the two routes against each other: slot's exact lv1 extraction == the matmul's row
            rows = L.extract_rows_exact(got[0, oc], slots)
            assert np.array_equal(rows, o_mm[0, oc * positions:(oc + 1) * positions].cpu().numpy().view(np.uint32)), "routes differ"
        assert np.array_equal(o_2[:1].cpu().numpy().view(np.uint32), L.polymul_model(w2, in2[:1])), "dense product differs"
        assert np.array_equal(o_3.cpu().numpy().view(np.uint32), L.polymul_model(L.monomial(17), maps[:1])), "monomial differs"
        ts = {name: [] for name in routes}
        for _ in range(args.reps):
            for name, fn in routes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts[name].append((time.perf_counter() - t0) * 1e3)
        out = {name: summary(t) for name, t in ts.items()}
        # (rates: every weight counted, the zeros of a 9-tap polynomial and of an expanded row included)
        out["packed_conv_polymul_dev"].update(
            {"rows": out_c, "cols": 1, "groups": groups, "out_bytes": o_pm.numel() * 4, "in_bytes": maps.nbytes,
             **rate(out["packed_conv_polymul_dev"]["median_ms"], 8 * out_c * N * 2 * N * groups)})
        out["expanded_trlwe_matmul_dev"].update(
            {"rows": out_c * positions, "cols": N, "groups": groups, "out_bytes": o_mm.numel() * 4, "weight_bytes": wx.nbytes,
             **rate(out["expanded_trlwe_matmul_dev"]["median_ms"], 8 * out_c * positions * N * (N + 1) * groups)})
        ops2 = 8 * rows2 * cols2 * N * 2 * N * groups2
        out["dense_32x32_polymul_dev"].update({"rows": rows2, "cols": cols2, "groups": groups2, "int8_ops": ops2,
                                               "in_bytes": in2.nbytes, "out_bytes": o_2.numel() * 4,
                                               **rate(out["dense_32x32_polymul_dev"]["median_ms"], ops2)})
        out["monomial_polymul_dev"].update({"rows": 1, "cols": 1, "groups": 1})
        out["packed_conv"] = {
            "shape": {"in_c": 1, "in_h": in_h, "in_w": in_w, "k_h": k, "k_w": k, "out_c": out_c, "positions": positions},
            "polymul_over_expanded_matmul_time": round(out["packed_conv_polymul_dev"]["median_ms"] / out["expanded_trlwe_matmul_dev"]["median_ms"], 4),
            "polymul_over_expanded_matmul_out_bytes": round(o_pm.numel() / o_mm.numel(), 5)}
        res["routes"] = out
        print(json.dumps(out), flush=True)
    finally:
        e.close()
    res["device"]["shader_mhz_after"] = shader_clock(R, p)
    with open(args.out, "w") as fh:
        json.dump(res, fh)
        fh.write("\n")


if __name__ == "__main__":
    main()
