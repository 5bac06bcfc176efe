"""Packed TRLWE encryption on one GPU (include/tfhe_hip.h "packed encryption"), on SECURITY_128_BIT:
tfhe_hip_batch_encrypt_trlwe_dev in its full and bodies-only forms and tfhe_hip_expand_seeded_trlwe_dev at 1, 64 and 1,024
groups (1,024 values each), under one fixed generator key.  Two yardsticks, neither of them the code under test:
  (a) numpy_and_upload      the route without these calls: SecretKey.encrypt_packed_f64 in numpy (seed=: numpy's own
                            generator) plus the upload of its result;
  (b) k_gen_packing_key     the same row pieces without the plaintext add: its kernel time per row, from the trace.
A _dev call is: stage K and s1 (a small copy the call waits for), k_key_spectrum, the kernel, the wipe.  The figures are
CALL times; a kernel's own time is in `kernel_trace` (below) and nowhere else.  Every line records how many words differ
from the CPU form, seeded.symmetric_trlwe_rows (a borderline noise sample may move a word by one: DESIGN 11.2).

Kernel times proper come from a trace, taken in a run of its own and merged into the file afterwards:

    python3 profiles/packed_encrypt_bench.py [--reps 5] [--out profiles/packed_encrypt_bench.json]
    rocprofv3 --kernel-trace -d DIR -o packed -- python3 profiles/packed_encrypt_bench.py --trace-feed
    python3 profiles/packed_encrypt_bench.py --merge-trace DIR/packed_results.db
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
from compressed_key_bench import shader_clock  # noqa: E402
from decrypt_bench import host_synced  # noqa: E402
from sym_encrypt_bench import event_timed  # noqa: E402

K = bytes(range(32))
SEED = bytes(range(32, 64))
GROUPS = (1, 64, 1024)
TRACE_GROUPS = GROUPS + (6300,)  # ... and as many groups as the packing key of SECURITY_128_BIT has rows
TRACE_CALLS = 12  # per segment; the first 4 dispatches are warm-up


def lines(R, torch, p, reps):
    from rs_tfhe_amd.client import f64_to_torus
    from rs_tfhe_amd.params import N
    from rs_tfhe_amd.seeded import symmetric_trlwe_rows

    sk = R.SecretKey.new(p, 1)
    out = {}
    e = R.Engine(p, 0)
    try:
        for groups in GROUPS:
            count = groups * N
            pt = np.random.default_rng(groups).uniform(-0.5, 0.5, count)
            plain = f64_to_torus(pt)
            tp = torch.from_numpy(plain.view(np.int32)).cuda()
            full = torch.empty((groups, 2, N), dtype=torch.int32, device="cuda")
            bod = torch.empty((groups, N), dtype=torch.int32, device="cuda")
            exp = torch.empty((groups, 2, N), dtype=torch.int32, device="cuda")
            inner = 16 if groups >= 1024 else 32
            want = symmetric_trlwe_rows(SEED, K, np.arange(groups, dtype=np.uint64), sk.key_lv1, plain, count, p.alpha_lv1)
            line = {"values": count, "ciphertext_mb": round(full.numel() * 4 / 1e6, 3)}
            t = event_timed(lambda: e.batch_encrypt_trlwe_dev(sk.key_lv1, tp, p.alpha_lv1, SEED, K, 0, out=full), reps, inner)
            line["full"] = dict(t, mismatching_words_vs_cpu_form=int((full.cpu().numpy().view(np.uint32) != want).sum()))
            t = event_timed(lambda: e.batch_encrypt_trlwe_dev(sk.key_lv1, tp, p.alpha_lv1, SEED, K, 0, bodies=bod), reps, inner)
            line["bodies_only"] = dict(t, mismatching_words_vs_cpu_form=int((bod.cpu().numpy().view(np.uint32) != want[:, 1]).sum()))
            t = event_timed(lambda: e.expand_seeded_trlwe_dev(SEED, 0, bod, exp), reps, inner)
            line["expand"] = dict(t, mismatching_words_vs_full_form=int((exp != full).sum().item()))
            line["numpy_and_upload"], _ = host_synced(
                lambda: torch.from_numpy(sk.encrypt_packed_f64(pt, seed=1).view(np.int32)).cuda(), reps)
            line["numpy_and_upload_over_full_call"] = round(line["numpy_and_upload"]["median_ms"] / line["full"]["median_ms"], 1)
            out[str(groups)] = line
            print(groups, json.dumps(line), flush=True)
    finally:
        e.close()
    return out


def trace_feed(R, torch, p):
    """What a kernel trace is taken of: per size TRACE_CALLS full calls, bodies-only calls and expansions, then TRACE_CALLS
    generations of the packing key (n t rows of the same pieces)."""
    from rs_tfhe_amd.params import N

    sk = R.SecretKey.new(p, 1)
    e = R.Engine(p, 0)
    for groups in TRACE_GROUPS:
        tp = torch.zeros(groups * N, dtype=torch.int32, device="cuda")
        full = torch.empty((groups, 2, N), dtype=torch.int32, device="cuda")
        bod = torch.empty((groups, N), dtype=torch.int32, device="cuda")
        for _ in range(TRACE_CALLS):
            e.batch_encrypt_trlwe_dev(sk.key_lv1, tp, p.alpha_lv1, SEED, K, 0, out=full)
        for _ in range(TRACE_CALLS):
            e.batch_encrypt_trlwe_dev(sk.key_lv1, tp, p.alpha_lv1, SEED, K, 0, bodies=bod)
        for _ in range(TRACE_CALLS):
            e.expand_seeded_trlwe_dev(SEED, 0, bod, full)
        torch.cuda.synchronize()
    for _ in range(TRACE_CALLS):
        e.gen_packing_key(sk.key_lv0, sk.key_lv1, rng_key=K, download=False)
    torch.cuda.synchronize()
    e.close()


def trace_summary(db, p):
    """Kernel durations (us, median / min / max; the first 4 dispatches of a segment are warm-up) of a --trace-feed run, from
    the `kernels` view of rocprofv3's database"""
    import sqlite3

    rows = sqlite3.connect(db).execute("select name, start, end from kernels order by start").fetchall()

    def seg(v, per):
        v = v[4:]
        return {"median_us": round(float(np.median(v)), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                "dispatches": len(v), "median_us_per_row": round(float(np.median(v)) / per, 3)}

    enc = [(e - s) / 1e3 for n, s, e in rows if "k_trlwe_rows" in n]
    exp = [(e - s) / 1e3 for n, s, e in rows if "k_expand_trlwe" in n]
    gen = [(e - s) / 1e3 for n, s, e in rows if "k_gen_packing_key" in n]
    spec = [(e - s) / 1e3 for n, s, e in rows if "k_key_spectrum" in n]
    c = TRACE_CALLS
    assert len(enc) == 2 * c * len(TRACE_GROUPS) and len(exp) == c * len(TRACE_GROUPS) and len(gen) == c, (len(enc), len(exp), len(gen))
    out = {}
    for i, groups in enumerate(TRACE_GROUPS):
        out[str(groups)] = {"k_trlwe_rows_full": seg(enc[2 * c * i:2 * c * i + c], groups),
                            "k_trlwe_rows_bodies_only": seg(enc[2 * c * i + c:2 * c * (i + 1)], groups),
                            "k_expand_trlwe": seg(exp[c * i:c * (i + 1)], groups)}
    out["k_gen_packing_key"] = dict(seg(gen, p.n * p.iks_t), rows=p.n * p.iks_t)
    out["k_key_spectrum"] = seg(spec, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_encrypt_bench.json"))
    ap.add_argument("--trace-feed", action="store_true", help="run the calls a kernel trace is taken of, and stop")
    ap.add_argument("--merge-trace", default=None, help="rocprofv3 database of a --trace-feed run: add `kernel_trace` to --out")
    args = ap.parse_args()
    from rs_tfhe_amd.params import SECURITY_128_BIT as p

    if args.merge_trace:  # (no device needed)
        res = json.load(open(args.out))
        res["kernel_trace"] = dict(
            {"what": "kernel durations of `rocprofv3 --kernel-trace -- python profiles/packed_encrypt_bench.py --trace-feed`, a "
                     "run of its own; k_gen_packing_key makes n t = 6,300 rows of the same pieces without the plaintext add and "
                     "with both halves stored twice"}, **trace_summary(args.merge_trace, p))
        with open(args.out, "w") as f:
            json.dump(res, f)
            f.write("\n")
        return
    import torch

    assert torch.cuda.is_available(), "this benchmark measures the GPU: no device, no figure"
    import rs_tfhe_amd as R

    if args.trace_feed:
        trace_feed(R, torch, p)
        return
    props = torch.cuda.get_device_properties(0)
    res = {"clock": "torch.cuda.Event pairs on the current stream around windows of calls, one warm-up call per figure, then "
                    "the median / min of `reps` windows, per call; numpy_and_upload: time.perf_counter with the device "
                    "synchronised before and after, one warm-up, the median / min of `reps` runs",
           "device": {"name": props.name, "arch": getattr(props, "gcnArchName", None),
                      "compute_units": props.multi_processor_count, "hip": torch.version.hip},
           "host": {"machine": platform.machine(), "cpus_available": len(os.sched_getaffinity(0)),
                    "python": platform.python_version(), "numpy": np.__version__},
           "reps": args.reps, "set": p.name}
    res["device"]["shader_mhz_before"] = shader_clock(R, p)
    res["groups"] = lines(R, torch, p, args.reps)
    res["device"]["shader_mhz_after"] = shader_clock(R, p)
    with open(args.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
