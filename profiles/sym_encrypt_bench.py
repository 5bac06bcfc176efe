"""Symmetric encryption on one GPU, on SECURITY_128_BIT and SECURITY_UINT4: tfhe_hip_batch_encrypt_dev of 65,536 and of
1,024 rows in the full form and in the bodies-only form, tfhe_hip_gen_public_key (size 2n) and
tfhe_hip_gen_reenc_key_symmetric with and without the download.  Yardsticks taken in the same run on the same box, none
of them the code under test: the package's numpy CPU form for the same rows, the staged upload of the finished array
(load_public_key / load_reenc_key of the host key for the keys) and, for the full form, a hipMemsetAsync of the same number
of bytes on the same stream.  Every line also records how many words differ from the CPU form (0 expected away from
borderline noise samples).

    python3 profiles/sym_encrypt_bench.py [--reps 7] [--out profiles/sym_encrypt_bench.json]
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


def event_timed(fn, reps, inner=1):
    """One untimed warm-up call, then `reps` windows of `inner` calls each between two torch.cuda.Events on the current
    stream; a window ends in an event synchronise.  Milliseconds per call."""
    import torch

    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(np.min(ts)), 4), "calls_per_window": inner}


def host_timed(fn, reps):
    """The CPU yardsticks: (the median / min of `reps` runs, no device involved; the last run's result)."""
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(np.min(ts)), 3), "runs": reps}, got


def hip_memset_async():
    """hipMemsetAsync of the HIP runtime this process already runs on (the one torch loaded), through ctypes."""
    import ctypes as C

    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    fn = C.CDLL(path).hipMemsetAsync
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    return fn


def gbps(nbytes, t):
    return round(nbytes / (t["median_ms"] * 1e-3) / 1e9, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--sets", default="SECURITY_128_BIT,SECURITY_UINT4")
    ap.add_argument("--counts", default="65536,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sym_encrypt_bench.json"))
    args = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "this benchmark measures the GPU: no device, no figure"
    import rs_tfhe_amd as R
    from rs_tfhe_amd import proxy_reenc as PR, seeded as S
    from rs_tfhe_amd.params import PARAM_SETS

    K, SEED = bytes(range(32)), bytes(range(32, 64))
    memset_async = hip_memset_async()
    props = torch.cuda.get_device_properties(0)
    res = {"clock": "torch.cuda.Event pairs on the current stream around windows of calls, one warm-up call per figure, "
                    "then the median / min of `reps` windows, per call; the host-form key calls end in a device "
                    "synchronise of their own; numpy_cpu_form: time.perf_counter on this box's host CPUs",
           "device": {"name": props.name, "arch": getattr(props, "gcnArchName", None),
                      "compute_units": props.multi_processor_count, "hip": torch.version.hip},
           "host": {"machine": platform.machine(), "cpus_available": len(os.sched_getaffinity(0)),
                    "python": platform.python_version(), "numpy": np.__version__},
           "reps": args.reps, "cpu_reps": args.cpu_reps, "host_arrays": "pageable numpy", "sets": {}}
    res["device"]["shader_mhz_before"] = shader_clock(R, PARAM_SETS["SECURITY_128_BIT"])
    for name in args.sets.split(","):
        p = PARAM_SETS[name]
        alice, bob = R.SecretKey.new(p, 1), R.SecretKey.new(p, 2)
        w = p.n + 1
        out = {"n": p.n, "keystream_blocks_per_row": (p.n + 15) // 16 + 1, "encrypt": {}}
        e = R.Engine(p, 0)
        try:
            for count in (int(c) for c in args.counts.split(",")):
                plain = np.random.default_rng(count).integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)
                tp = torch.from_numpy(plain.view(np.int32)).cuda()
                to = torch.empty((count, w), dtype=torch.int32, device="cuda")
                tb = torch.empty(count, dtype=torch.int32, device="cuda")
                inner = 4 if count >= 16384 else 32
                full = event_timed(lambda: e.batch_encrypt_dev(alice.key_lv0, tp, p.alpha_lv0, SEED, K, 0, out=to),
                                   args.reps, inner)
                bodies = event_timed(lambda: e.batch_encrypt_dev(alice.key_lv0, tp, p.alpha_lv0, SEED, K, 0, bodies=tb),
                                     args.reps, inner)
                words, bwords = to.cpu().numpy().view(np.uint32), tb.cpu().numpy().view(np.uint32)
                # yardsticks: a memset of the same bytes, the numpy CPU form of the same rows, staging the finished batch
                nbytes = count * w * 4

                def memset_call():
                    rc = memset_async(to.data_ptr(), 0, nbytes, torch.cuda.current_stream().cuda_stream)
                    assert rc == 0, f"hipMemsetAsync: {rc}"

                memset = event_timed(memset_call, args.reps, inner)
                rows = np.arange(count, dtype=np.uint64)
                cpu, ref = host_timed(lambda: S.symmetric_rows(SEED, K, rows, alice.key_lv0, plain, p.alpha_lv0,
                                                               S.DOMAINS_SYM_TLWE), args.cpu_reps)
                host_ct = np.ascontiguousarray(ref)
                stage = event_timed(lambda: to.copy_(torch.from_numpy(host_ct.view(np.int32))), args.reps)
                out["encrypt"][str(count)] = {
                    "batch_encrypt_dev_full": full, "batch_encrypt_dev_bodies_only": bodies, "memset_same_bytes": memset,
                    "numpy_cpu_form": cpu, "staged_upload": stage, "batch_mb": round(nbytes / 1e6, 1),
                    "full_gb_per_s": gbps(nbytes, full), "memset_gb_per_s": gbps(nbytes, memset),
                    "full_share_of_memset_rate": round(memset["median_ms"] / full["median_ms"], 3),
                    "keystream_gb_per_s_bodies_only": gbps(count * 64 * out["keystream_blocks_per_row"], bodies),
                    "gpu_and_cpu_words_differing": int((words != ref).sum()),
                    "bodies_differing": int((bwords != ref[:, -1]).sum())}
                print(name, count, json.dumps(out["encrypt"][str(count)]), flush=True)
            # the public key, 2n rows
            size = 2 * p.n
            pk_dl = event_timed(lambda: e.gen_public_key(alice.key_lv0, size, p.alpha_lv0, K), args.reps)
            pk_no = event_timed(lambda: e.gen_public_key(alice.key_lv0, size, p.alpha_lv0, K, download=False), args.reps)
            enc = e.gen_public_key(alice.key_lv0, size, p.alpha_lv0, K)
            pk_load = event_timed(lambda: e.load_public_key(enc), args.reps)
            # the symmetric re-encryption key
            rk_dl = event_timed(lambda: e.gen_reenc_key_symmetric(alice.key_lv0, bob.key_lv0, rng_key=K), args.reps)
            rk_no = event_timed(lambda: e.gen_reenc_key_symmetric(alice.key_lv0, bob.key_lv0, rng_key=K, download=False),
                                args.reps)
            key = e.gen_reenc_key_symmetric(alice.key_lv0, bob.key_lv0, rng_key=K)
            rk_load = event_timed(lambda: e.load_reenc_key(key), args.reps)
        finally:
            e.close()
        cpu_pk, ref_pk = host_timed(lambda: PR.PublicKeyLv0.new(alice, rng_key=K).encryptions, args.cpu_reps)
        out["public_key"] = {"size": size, "key_mb": round(enc.nbytes / 1e6, 2), "gen_public_key_download": pk_dl,
                             "gen_public_key_no_download": pk_no, "numpy_cpu_form": cpu_pk,
                             "load_public_key_host_key": pk_load, "gpu_and_cpu_words_differing": int((enc != ref_pk).sum())}
        print(name, "public_key", json.dumps(out["public_key"]), flush=True)
        cpu_key, ref_key = host_timed(lambda: PR.ProxyReencryptionKey.new_symmetric(alice, bob, rng_key=K).key_encryptions,
                                      args.cpu_reps)
        out["reenc_key"] = {"rows": p.n * p.iks_t * p.base, "key_mb": round(key.nbytes / 1e6, 1),
                            "gen_reenc_key_symmetric_download": rk_dl, "gen_reenc_key_symmetric_no_download": rk_no,
                            "numpy_cpu_form": cpu_key, "load_reenc_key_host_key": rk_load,
                            "gpu_and_cpu_words_differing": int((key != ref_key).sum())}
        print(name, "reenc_key", json.dumps(out["reenc_key"]), flush=True)
        res["sets"][name] = out
    res["device"]["shader_mhz_after"] = shader_clock(R, PARAM_SETS["SECURITY_128_BIT"])
    with open(args.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
