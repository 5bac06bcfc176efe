"""Encrypted linear layers on one GPU (tfhe_hip_batch_tlwe_matmul_dev / tfhe_hip_batch_trlwe_matmul_dev): rows = cols =
1024 on SECURITY_128_BIT for 1 and 64 groups, on device buffers -- the dense form, the packed form without and with the
key switch -- beside the route the library had before: a compiled circuit of `rows` lincomb nodes with `cols` terms each
(Circuit.run_dev), and numpy's int64 product on the host (linear.matmul_model).  Every GPU result is checked against
the integer model on its first rows before anything is timed.  The int8 operation count is 2 * rows * cols * columns *
groups * 4 byte planes; its share of the matrix-core rate is against the random x random row of
profiles/exp/ubench_mfma.hip at two waves per SIMD (profiles/exp/logs/r3d_ubench_mfma.log).

    python3 profiles/matmul_bench.py [--reps 5] [--out profiles/matmul_bench.json]
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

from compressed_key_bench import shader_clock, timed  # noqa: E402

MFMA_INT8_TOPS = 3319.7  # random A x random B, 2 waves / SIMD (profiles/exp/logs/r3d_ubench_mfma.log)


def rate(ms, ops):
    tops = ops / (ms * 1e-3) / 1e12
    return {"int8_tops": round(tops, 1), "share_of_matrix_core_rate": round(tops / MFMA_INT8_TOPS, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024, help="rows = cols")
    ap.add_argument("--groups", default="1,64")
    ap.add_argument("--no-circuit", action="store_true", help="skip the lincomb-circuit route")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matmul_bench.json"))
    args = ap.parse_args()
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd import linear as L
    from rs_tfhe_amd.circuit import Circuit
    from rs_tfhe_amd.params import N, SECURITY_128_BIT as p

    rows = cols = args.size
    props = torch.cuda.get_device_properties(0)
    res = {"clock": "host wall clock (time.perf_counter) around the call + torch.cuda.synchronize(); one warm-up call "
                    "per shape, then the median / min of `reps`; operands and results in device memory",
           "device": {"name": props.name, "arch": getattr(props, "gcnArchName", None),
                      "compute_units": props.multi_processor_count, "hip": torch.version.hip},
           "host": {"machine": platform.machine(), "cpus_available": len(os.sched_getaffinity(0)),
                    "python": platform.python_version(), "numpy": np.__version__, "torch": torch.__version__},
           "set": p.name, "rows": rows, "cols": cols, "reps": args.reps, "matrix_core_int8_tops": MFMA_INT8_TOPS,
           "groups": {}}
    res["device"]["shader_mhz_before"] = shader_clock(R, p)
    rng = np.random.default_rng(1)
    w = rng.integers(-128, 128, (rows, cols)).astype(np.int8)
    bias = rng.integers(0, 1 << 32, rows, dtype=np.uint32)
    sk = R.SecretKey.new(p, 2)
    e = R.Engine(p, 0)
    try:
        e.gen_cloud_key(sk.key_lv0, sk.key_lv1, seed=3)
        tw = torch.from_numpy(w).to("cuda:0")
        tb = torch.from_numpy(bias.view(np.int32)).to("cuda:0")
        circ = None
        if not args.no_circuit:  # the route before this call: one n-term lincomb node per output row
            circ = Circuit(cols)
            for r in range(rows):
                circ.lincomb([(int(w[r, j]), j) for j in range(cols)], int(bias[r]))
        for groups in (int(g) for g in args.groups.split(",")):
            cts = rng.integers(0, 1 << 32, (groups, cols, p.n + 1), dtype=np.uint64).astype(np.uint32)
            trlwe = rng.integers(0, 1 << 32, (groups, 2, N), dtype=np.uint64).astype(np.uint32)
            t_in = torch.from_numpy(cts.view(np.int32)).to("cuda:0")
            t_tr = torch.from_numpy(trlwe.view(np.int32)).to("cuda:0")
            o_dense = torch.empty((groups, rows, p.n + 1), dtype=torch.int32, device="cuda:0")
            o_lv1 = torch.empty((groups, rows, N + 1), dtype=torch.int32, device="cuda:0")
            t0 = time.perf_counter()
            want = L.matmul_model(p, w, cts[:1], bias)
            host_ms = (time.perf_counter() - t0) * 1e3 * groups  # one group timed; the groups are independent products
            e.batch_tlwe_matmul_dev(tw, t_in, o_dense, bias=tb)
            e.batch_trlwe_matmul_dev(tw, t_tr, o_lv1, bias=tb, keyswitch=False)
            torch.cuda.synchronize()
            assert np.array_equal(o_dense[:1].cpu().numpy().view(np.uint32), want), "dense words differ from the model"
            assert np.array_equal(o_lv1[:1, :64].cpu().numpy().view(np.uint32),
                                  L.matmul_packed_model(p, w[:64], trlwe[:1], bias[:64])), "packed words differ from the model"
            ops0, ops1 = 8 * rows * cols * (p.n + 1) * groups, 8 * rows * cols * (N + 1) * groups
            out = {"dense_dev": timed(lambda: e.batch_tlwe_matmul_dev(tw, t_in, o_dense, bias=tb), args.reps),
                   "packed_dev": timed(lambda: e.batch_trlwe_matmul_dev(tw, t_tr, o_lv1, bias=tb, keyswitch=False), args.reps),
                   "packed_keyswitch_dev": timed(lambda: e.batch_trlwe_matmul_dev(tw, t_tr, o_dense, bias=tb, keyswitch=True),
                                                 args.reps),
                   "numpy_int64_host_ms": round(host_ms, 1), "numpy_note": "one group timed, times groups",
                   "dense_int8_ops": ops0, "packed_int8_ops": ops1,
                   "in_bytes": cts.nbytes, "trlwe_bytes": trlwe.nbytes, "out_bytes": groups * rows * (p.n + 1) * 4}
            out["dense_dev"].update(rate(out["dense_dev"]["median_ms"], ops0))
            out["packed_dev"].update(rate(out["packed_dev"]["median_ms"], ops1))
            if circ is not None:
                t_ci = t_in.permute(1, 0, 2).contiguous()  # [cols][groups][n+1]: the circuit's input layout
                wires = circ.run_dev(e, t_ci)
                torch.cuda.synchronize()
                got = wires[cols:, 0].cpu().numpy().view(np.uint32)  # group 0 of every output row
                assert np.array_equal(got, want[0]), "circuit words differ from the model"
                del wires
                out["lincomb_circuit_dev"] = timed(lambda: circ.run_dev(e, t_ci), args.reps)
                out["lincomb_circuit_over_dense"] = round(out["lincomb_circuit_dev"]["median_ms"] / out["dense_dev"]["median_ms"], 1)
            res["groups"][str(groups)] = out
            print(groups, json.dumps(out), flush=True)
    finally:
        e.close()
    res["device"]["shader_mhz_after"] = shader_clock(R, p)
    with open(args.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
