"""Decryption on one GPU (include/tfhe_hip.h "decryption"), on SECURITY_128_BIT and SECURITY_UINT4:
tfhe_hip_batch_decrypt_dev of 65,536 and of 1,024 rows in the three modes, and tfhe_hip_batch_decrypt_trlwe_dev of 64 packed
groups.  Yardsticks taken in the same process on the same device tensor, none of them the code under test:
  (a) download_and_numpy   the route without this call: `.cpu()` of the batch plus SecretKey.phase in numpy;
  (b) torch_sum_dim1       `cts.sum(dim=1)`: reads the same bytes, one add a word.
A _dev call is: stage the packed key bits (a small copy the call waits for), the kernel, the wipe.  call_floor is that
call on ONE row.  The figures are CALL times and call_tb_per_s the batch's bytes over them; a kernel's own time is in
`kernel_trace` (below) and nowhere else.  A batch of 65,536 rows
(184 MB) fits the 256 MiB Infinity Cache, so calls on one tensor read from it; the `streamed` figures rotate over
copies of the batch and read from HBM.  Every line records how many words differ from the numpy path (0 expected: the
arithmetic is exact).

`--variant-lib PATH --variant-name NAME` measures the LWE lines once more in a child process on another build of the
library and records both under `variants`.  The committed file's variant is k_lwe_phase with the other load shape
the header of csrc/decrypt.hpp describes, aligned dwordx4 chunks: it was slower, its source was NOT kept in the tree,
and its lines (`variants.x4`, `kernel_trace.x4`) are a record of that comparison which this commit cannot rebuild.

Kernel times proper come from a trace, taken in a run of its own and merged into the file afterwards:

    python3 profiles/decrypt_bench.py [--reps 5] [--out profiles/decrypt_bench.json] [--variant-lib PATH --variant-name x4]
    rocprofv3 --kernel-trace -d DIR -o decrypt -- python3 profiles/decrypt_bench.py --trace-feed
    python3 profiles/decrypt_bench.py --merge-trace DIR/decrypt_results.db [--merge-trace-variant ...]
"""
import argparse
import json
import os
import platform
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from compressed_key_bench import shader_clock  # noqa: E402
from sym_encrypt_bench import event_timed  # noqa: E402

MODES = (("phase", None), ("bool", None), ("message", 16))


def host_synced(fn, reps):
    """One warm-up, then the median / min of `reps` runs on the host clock, the device synchronised before and after"""
    import torch

    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(np.min(ts)), 3), "runs": reps}, got


def numpy_decode(sk, cts, mode, m):
    ph = sk.phase(cts)
    if mode == "bool":
        return (ph.view(np.int32) >= 0).astype(np.uint32)
    return sk.decrypt_lwe_message(cts, m).astype(np.uint32) if mode == "message" else ph


def lwe_lines(R, torch, name, counts, reps, yardsticks=True):
    from rs_tfhe_amd.params import PARAM_SETS

    p = PARAM_SETS[name]
    sk = R.SecretKey.new(p, 1)
    w = p.n + 1
    out = {"n": p.n, "row_bytes": 4 * w, "rows": {}}
    e = R.Engine(p, 0)
    try:
        one = torch.zeros((1, w), dtype=torch.int32, device="cuda")
        o1 = torch.empty(1, dtype=torch.int32, device="cuda")
        floor = event_timed(lambda: e.batch_decrypt_dev(sk.key_lv0, one, o1), reps, 32)
        out["call_floor_one_row"] = floor
        for count in counts:
            cts = np.random.default_rng(count).integers(0, 1 << 32, (count, w), dtype=np.uint64).astype(np.uint32)
            tc = torch.from_numpy(cts.view(np.int32)).cuda()
            to = torch.empty(count, dtype=torch.int32, device="cuda")
            nbytes = count * (w + 1) * 4
            inner = 8 if count >= 16384 else 32
            line = {"batch_mb": round(nbytes / 1e6, 2)}
            for mode, m in MODES:
                t = event_timed(lambda: e.batch_decrypt_dev(sk.key_lv0, tc, to, mode, m), reps, inner)
                got = to.cpu().numpy().view(np.uint32)
                line[mode] = dict(t, modulus=m, call_tb_per_s=round(nbytes / (t["median_ms"] * 1e-3) / 1e12, 3),
                                  mismatching_words_vs_numpy=int((got != numpy_decode(sk, cts, mode, m)).sum()))
            # The same batch every call stays in the 256 MiB Infinity Cache (184 MB at 65,536 rows of SECURITY_128_BIT);
            # `streamed` rotates over copies of it, more than two caches' worth between two reads of one: HBM reads.
            copies = -(-600_000_000 // nbytes) if count >= 16384 else 1
            tcs = [tc] + [tc.clone() for _ in range(copies - 1)]
            turn = [0]

            def rotate(fn):
                def call():
                    turn[0] += 1
                    return fn(tcs[turn[0] % copies])
                return call

            if copies > 1:
                t = event_timed(rotate(lambda x: e.batch_decrypt_dev(sk.key_lv0, x, to)), reps, 2 * copies)
                line["phase_streamed"] = dict(t, copies=copies, call_tb_per_s=round(nbytes / (t["median_ms"] * 1e-3) / 1e12, 3),
                                              mismatching_words_vs_numpy=int((to.cpu().numpy().view(np.uint32) != sk.phase(cts)).sum()))
            if yardsticks:
                line["torch_sum_dim1"] = event_timed(lambda: tc.sum(dim=1), reps, inner)
                line["download_and_numpy"], _ = host_synced(lambda: sk.phase(tc.cpu().numpy().view(np.uint32)), reps)
                b = line["torch_sum_dim1"]["median_ms"]
                line["phase_call_over_torch_sum"] = round(line["phase"]["median_ms"] / b, 3)
                line["torch_sum_tb_per_s"] = round(nbytes / (b * 1e-3) / 1e12, 3)
                if copies > 1:
                    line["torch_sum_dim1_streamed"] = event_timed(rotate(lambda x: x.sum(dim=1)), reps, 2 * copies)
                    bs = line["torch_sum_dim1_streamed"]["median_ms"]
                    line["phase_streamed_call_over_torch_sum_streamed"] = round(line["phase_streamed"]["median_ms"] / bs, 3)
                    line["torch_sum_streamed_tb_per_s"] = round(nbytes / (bs * 1e-3) / 1e12, 3)
            del tcs
            out["rows"][str(count)] = line
            print(name, count, json.dumps(line), flush=True)
    finally:
        e.close()
    return out


def packed_line(R, torch, name, groups, reps):
    from rs_tfhe_amd.params import N, PARAM_SETS

    p = PARAM_SETS[name]
    sk = R.SecretKey.new(p, 2)
    packed = np.random.default_rng(groups).integers(0, 1 << 32, (groups, 2, N), dtype=np.uint64).astype(np.uint32)
    tp = torch.from_numpy(packed.view(np.int32)).cuda()
    to = torch.empty(groups * N, dtype=torch.int32, device="cuda")
    e = R.Engine(p, 0)
    try:
        line = {"groups": groups, "slots": groups * N}
        for mode, m in MODES:
            t = event_timed(lambda: e.batch_decrypt_trlwe_dev(sk.key_lv1, tp, groups * N, to, mode, m), reps, 16)
            got = to.cpu().numpy().view(np.uint32)
            ph = sk.packed_phase(packed, groups * N)
            want = ph if mode == "phase" else (ph.view(np.int32) >= 0).astype(np.uint32) if mode == "bool" else \
                sk.decrypt_packed_lwe_message(packed, groups * N, m).astype(np.uint32)
            line[mode] = dict(t, modulus=m, mismatching_words_vs_numpy=int((got != want).sum()))
        line["download_and_numpy"], _ = host_synced(lambda: sk.packed_phase(tp.cpu().numpy().view(np.uint32), groups * N), reps)
    finally:
        e.close()
    print(name, "packed", json.dumps(line), flush=True)
    return line


def trace_feed(R, torch, names):
    """What a kernel trace is taken of (rocprofv3 --kernel-trace -- python profiles/decrypt_bench.py --trace-feed): per set
    44 PHASE calls rotating over 4 copies of a 65,536-row batch (HBM reads), 44 torch sums likewise, then 40 MESSAGE
    calls on one copy (Infinity Cache reads)."""
    from rs_tfhe_amd.params import PARAM_SETS

    for name in names:
        p = PARAM_SETS[name]
        sk = R.SecretKey.new(p, 1)
        e = R.Engine(p, 0)
        cts = np.random.default_rng(1).integers(0, 1 << 32, (65536, p.n + 1), dtype=np.uint64).astype(np.uint32)
        tcs = [torch.from_numpy(cts.view(np.int32)).cuda() for _ in range(4)]
        to = torch.empty(65536, dtype=torch.int32, device="cuda")
        for i in range(44):
            e.batch_decrypt_dev(sk.key_lv0, tcs[i % 4], to)
        torch.cuda.synchronize()
        for i in range(44):
            tcs[i % 4].sum(dim=1)
        torch.cuda.synchronize()
        for i in range(40):
            e.batch_decrypt_dev(sk.key_lv0, tcs[0], to, "message", 16)
        torch.cuda.synchronize()
        e.close()


def trace_summary(db, names):
    """Kernel durations (us, median / min / max; the first 4 dispatches of a segment are warm-up) of a --trace-feed run, from
    the `kernels` view of rocprofv3's database"""
    import sqlite3

    rows = sqlite3.connect(db).execute("select name, start, end from kernels order by start").fetchall()

    def seg(v):
        return {"median_us": round(float(np.median(v)), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2), "dispatches": len(v)}

    k = [(e - s) / 1e3 for n, s, e in rows if "k_lwe_phase" in n]
    red = [(e - s) / 1e3 for n, s, e in rows if "reduce_kernel" in n]
    cast = [(e - s) / 1e3 for n, s, e in rows if "elementwise_kernel" in n]
    assert len(k) == 84 * len(names) and len(red) == len(cast) == 44 * len(names), (len(k), len(red), len(cast))
    out = {}
    for i, name in enumerate(names):
        out[name] = {"k_lwe_phase_streamed": seg(k[84 * i + 4:84 * i + 44]), "k_lwe_phase_message_resident": seg(k[84 * i + 48:84 * i + 84]),
                     "torch_sum_cast_to_int64_kernel": seg(cast[44 * i + 4:44 * i + 44]),
                     "torch_sum_reduce_kernel": seg(red[44 * i + 4:44 * i + 44])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sets", default="SECURITY_128_BIT,SECURITY_UINT4")
    ap.add_argument("--counts", default="65536,1024")
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decrypt_bench.json"))
    ap.add_argument("--variant-lib", default=None, help="another build of the library: the LWE lines are measured on it too")
    ap.add_argument("--variant-name", default="variant")
    ap.add_argument("--this-name", default="dword", help="the load shape this tree's library is built with")
    ap.add_argument("--lwe-only", action="store_true", help="(the child of --variant-lib) print the LWE lines as JSON and stop")
    ap.add_argument("--trace-feed", action="store_true", help="run the calls a kernel trace is taken of, and stop")
    ap.add_argument("--merge-trace", default=None, help="rocprofv3 database of a --trace-feed run: add `kernel_trace` to --out")
    ap.add_argument("--merge-trace-variant", default=None, help="... and of a --trace-feed run on the --variant-name build")
    args = ap.parse_args()
    if args.merge_trace:  # (no device needed)
        res = json.load(open(args.out))
        res["kernel_trace"] = {"what": "kernel durations of `rocprofv3 --kernel-trace -- python profiles/decrypt_bench.py "
                                       "--trace-feed`, a run of its own (65,536 rows; torch's sum(dim=1) of int32 is two "
                                       "kernels, a cast to int64 and the reduction).  The variant's source was not kept in the tree",
                               args.this_name: trace_summary(args.merge_trace, args.sets.split(","))}
        if args.merge_trace_variant:
            res["kernel_trace"][args.variant_name] = trace_summary(args.merge_trace_variant, args.sets.split(","))
        with open(args.out, "w") as f:
            json.dump(res, f)
            f.write("\n")
        return
    import torch

    assert torch.cuda.is_available(), "this benchmark measures the GPU: no device, no figure"
    import rs_tfhe_amd as R
    from rs_tfhe_amd.params import PARAM_SETS

    names, counts = args.sets.split(","), [int(c) for c in args.counts.split(",")]
    if args.trace_feed:
        trace_feed(R, torch, names)
        return
    if args.lwe_only:
        print("VARIANT " + json.dumps({n: lwe_lines(R, torch, n, counts, args.reps, yardsticks=False) for n in names}))
        return
    props = torch.cuda.get_device_properties(0)
    res = {"clock": "torch.cuda.Event pairs on the current stream around windows of calls, one warm-up call per figure, then "
                    "the median / min of `reps` windows, per call; download_and_numpy: time.perf_counter with the device "
                    "synchronised before and after, one warm-up, the median / min of `reps` runs",
           "device": {"name": props.name, "arch": getattr(props, "gcnArchName", None),
                      "compute_units": props.multi_processor_count, "hip": torch.version.hip},
           "host": {"machine": platform.machine(), "cpus_available": len(os.sched_getaffinity(0)),
                    "python": platform.python_version(), "numpy": np.__version__},
           "reps": args.reps, "sets": {}}
    res["device"]["shader_mhz_before"] = shader_clock(R, PARAM_SETS["SECURITY_128_BIT"])
    for name in names:
        res["sets"][name] = lwe_lines(R, torch, name, counts, args.reps)
        res["sets"][name]["packed"] = packed_line(R, torch, name, args.groups, args.reps)
    if args.variant_lib:
        env = dict(os.environ, TFHE_HIP_LIB=os.path.abspath(args.variant_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--lwe-only", "--reps", str(args.reps), "--sets", args.sets,
                            "--counts", args.counts], env=env, capture_output=True, text=True, check=True)
        other = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("VARIANT "))[8:])

        def phase_ms(sets):
            keys = ("median_ms", "min_ms", "mismatching_words_vs_numpy")
            return {n: {c: {f: {k: sets[n]["rows"][c][f][k] for k in keys if k in sets[n]["rows"][c][f]} for f in ("phase", "phase_streamed")
                            if f in sets[n]["rows"][c]} for c in sets[n]["rows"]} for n in sets}

        res["variants"] = {"what": "k_lwe_phase, PHASE mode, _dev form: the two load shapes of the header of csrc/decrypt.hpp "
                                   "(dword loads at lane stride 1, kept; aligned dwordx4 chunks), each in a process of its "
                                   "own on a library built with it, same run.  The source of the variant was not kept: its lines "
                                   "record the comparison and cannot be rebuilt from this tree",
                           args.this_name: phase_ms(res["sets"]), args.variant_name: phase_ms(other), "shipped": args.this_name}
    res["device"]["shader_mhz_after"] = shader_clock(R, PARAM_SETS["SECURITY_128_BIT"])
    with open(args.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
