"""Encrypted 2-D convolution on one GPU (tfhe_hip_batch_tlwe_conv2d_dev): a 28 x 28 x 16 map of SECURITY_128_BIT
ciphertexts, 32 filters of 3 x 3, stride 1, padding 1, for 1 and 16 groups, on device buffers -- beside the route the
library had before: an im2col gather on the device (torch.index_select over pixels, with one zero pixel appended for the
padding) followed by tfhe_hip_batch_tlwe_matmul_dev on the gathered [positions][K][n+1] buffer, timed with and without
the gather, and numpy's linear.conv2d_model on the host for one group.  The routes alternate within each repetition, so
that a drift of the clocks meets all of them alike.  Every GPU result is checked before anything is timed: the routes
against each other on all words, group 0 against the integer model.  The int8 operation count is 2 * out_c * K * (n + 1)
* positions * 4 byte planes; its share of the matrix-core rate is against the random x random row of
profiles/exp/ubench_mfma.hip at two waves per SIMD (profiles/exp/logs/r3d_ubench_mfma.log).

    python3 profiles/conv2d_bench.py [--reps 5] [--out profiles/conv2d_bench.json]
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
from matmul_bench import MFMA_INT8_TOPS, rate  # noqa: E402


def summary(ts):
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(np.min(ts)), 3),
            "max_ms": round(float(np.max(ts)), 3), "samples_ms": [round(float(t), 3) for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", default="1,16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv2d_bench.json"))
    args = ap.parse_args()
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd import linear as L
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    in_h = in_w = 28
    in_c, out_c, k, pad = 16, 32, 3, 1
    K, width = k * k * in_c, p.n + 1
    out_h, out_w = L.conv2d_out_shape(in_h, in_w, k, k, 1, pad)
    props = torch.cuda.get_device_properties(0)
    res = {"clock": "host wall clock (time.perf_counter) around each call + torch.cuda.synchronize(); one warm-up call of "
                    "every route per shape, then `reps` repetitions in which the routes alternate; operands and results in "
                    "device memory",
           "device": {"name": props.name, "arch": getattr(props, "gcnArchName", None),
                      "compute_units": props.multi_processor_count, "hip": torch.version.hip},
           "host": {"machine": platform.machine(), "cpus_available": len(os.sched_getaffinity(0)),
                    "python": platform.python_version(), "numpy": np.__version__, "torch": torch.__version__},
           "set": p.name, "shape": {"in_h": in_h, "in_w": in_w, "in_c": in_c, "out_c": out_c, "k_h": k, "k_w": k,
                                    "stride": 1, "padding": pad, "K": K, "out_h": out_h, "out_w": out_w},
           "reps": args.reps, "matrix_core_int8_tops": MFMA_INT8_TOPS, "groups": {}}
    res["device"]["shader_mhz_before"] = shader_clock(R, p)
    rng = np.random.default_rng(1)
    w = rng.integers(-128, 128, (out_c, k, k, in_c)).astype(np.int8)
    bias = rng.integers(0, 1 << 32, out_c, dtype=np.uint32)
    e = R.Engine(p, 0)  # no key: neither route needs one
    try:
        tw = torch.from_numpy(w).to("cuda:0")
        tw2 = tw.view(out_c, K)
        tb = torch.from_numpy(bias.view(np.int32)).to("cuda:0")
        for groups in (int(g) for g in args.groups.split(",")):
            pixels, positions = groups * in_h * in_w, groups * out_h * out_w
            cts = rng.integers(0, 1 << 32, (groups, in_h, in_w, in_c, width), dtype=np.uint64).astype(np.uint32)
            # the map with one zero pixel behind it: what the gather reads for a padding tap
            src = torch.zeros((pixels + 1, in_c * width), dtype=torch.int32, device="cuda:0")
            src[:pixels] = torch.from_numpy(cts.view(np.int32).reshape(pixels, in_c * width)).to("cuda:0")
            t_in = src[:pixels].view(groups, in_h, in_w, in_c, width)
            g, oy, ox, ky, kx = np.meshgrid(np.arange(groups), np.arange(out_h), np.arange(out_w), np.arange(k), np.arange(k),
                                            indexing="ij")
            iy, ix = oy + ky - pad, ox + kx - pad
            idx = np.where((iy >= 0) & (iy < in_h) & (ix >= 0) & (ix < in_w), (g * in_h + iy) * in_w + ix, pixels)
            t_idx = torch.from_numpy(idx.reshape(-1).astype(np.int64)).to("cuda:0")
            cols = torch.empty((positions * k * k, in_c * width), dtype=torch.int32, device="cuda:0")
            t_cols = cols.view(positions, K, width)
            o_conv = torch.full((groups, out_h, out_w, out_c, width), -1, dtype=torch.int32, device="cuda:0")
            o_mm = torch.full((positions, out_c, width), -2, dtype=torch.int32, device="cuda:0")

            def fused():
                e.batch_tlwe_conv2d_dev(tw, t_in, o_conv, bias=tb, stride=1, padding=pad)

            def gather():
                torch.index_select(src, 0, t_idx, out=cols)

            def matmul():
                e.batch_tlwe_matmul_dev(tw2, t_cols, o_mm, bias=tb)

            def gather_matmul():
                gather()
                matmul()

            t0 = time.perf_counter()
            want = L.conv2d_model(p, w, cts[:1], bias, 1, pad)
            numpy_ms = (time.perf_counter() - t0) * 1e3
            fused()  # (the warm-up calls)
            gather_matmul()
            torch.cuda.synchronize()
            assert np.array_equal(o_conv[:1].cpu().numpy().view(np.uint32), want), "conv2d words differ from the model"
            assert torch.equal(o_conv.view(positions, out_c, width), o_mm), "the two routes differ"
            routes = {"conv2d_dev": fused, "gather_matmul_dev": gather_matmul, "matmul_dev_on_gathered": matmul}
            ts = {name: [] for name in routes}
            for _ in range(args.reps):
                for name, fn in routes.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    ts[name].append((time.perf_counter() - t0) * 1e3)
            ops = 8 * out_c * K * width * positions
            out = {name: summary(t) for name, t in ts.items()}
            for name in ("conv2d_dev", "matmul_dev_on_gathered"):
                out[name].update(rate(out[name]["median_ms"], ops))
            spread = max(out[n]["max_ms"] - out[n]["min_ms"] for n in ("conv2d_dev", "gather_matmul_dev"))
            out.update({"int8_ops": ops, "in_bytes": cts.nbytes, "im2col_bytes": cols.numel() * 4,
                        "out_bytes": o_conv.numel() * 4, "numpy_conv2d_model_one_group_ms": round(numpy_ms, 1),
                        "conv2d_over_gather_matmul": round(out["conv2d_dev"]["median_ms"] / out["gather_matmul_dev"]["median_ms"], 3),
                        "conv2d_over_matmul_on_gathered": round(out["conv2d_dev"]["median_ms"] / out["matmul_dev_on_gathered"]["median_ms"], 3),
                        "spread_ms": round(spread, 3),
                        "conv2d_no_slower_than_gather_matmul":
                            bool(out["conv2d_dev"]["median_ms"] <= out["gather_matmul_dev"]["median_ms"] + spread)})
            res["groups"][str(groups)] = out
            print(groups, json.dumps(out), flush=True)
            del src, cols, o_conv, o_mm, t_idx
    finally:
        e.close()
    res["device"]["shader_mhz_after"] = shader_clock(R, p)
    with open(args.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
