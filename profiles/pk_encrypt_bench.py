"""Public-key encryption and the asymmetric re-encryption key on one GPU, on SECURITY_128_BIT and SECURITY_UINT4:
tfhe_hip_batch_pk_encrypt_dev of 65,536 and of 1,024 ciphertexts (with the keystream pass and the contraction apart, by
the library's events), and tfhe_hip_gen_reenc_key_asymmetric with and without the download.  Yardsticks taken in the same
run, none of them the code under test: the package's numpy CPU form on this box's host CPUs for the same rows,
tfhe_hip_load_reenc_key of the host key, and the staged upload of 65,536 ciphertexts.

    python3 profiles/pk_encrypt_bench.py [--reps 5] [--out profiles/pk_encrypt_bench.json]
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


def host_timed(fn, reps):
    """The CPU yardsticks: one warm-up, then the median / min of `reps` (no device involved)."""
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(np.min(ts)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sets", default="SECURITY_128_BIT,SECURITY_UINT4")
    ap.add_argument("--counts", default="65536,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pk_encrypt_bench.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("every figure is the median of at least 5 calls")
    import torch

    import rs_tfhe_amd as R
    from rs_tfhe_amd import proxy_reenc as PR
    from rs_tfhe_amd.params import PARAM_SETS

    K = bytes(range(32))
    props = torch.cuda.get_device_properties(0)
    res = {"clock": "host wall clock (time.perf_counter) around the call + torch.cuda.synchronize(); one warm-up call "
                    "per figure, then the median / min of `reps`; selectors_ms / contraction_ms: the library's HIP events "
                    "(tfhe_hip_get_pk_encrypt_times), per call",
           "device": {"name": props.name, "arch": getattr(props, "gcnArchName", None),
                      "compute_units": props.multi_processor_count, "hip": torch.version.hip},
           "host": {"machine": platform.machine(), "cpus_available": len(os.sched_getaffinity(0)),
                    "python": platform.python_version(), "numpy": np.__version__},
           "reps": args.reps, "host_arrays": "pageable numpy", "sets": {}}
    res["device"]["shader_mhz_before"] = shader_clock(R, PARAM_SETS["SECURITY_128_BIT"])
    for name in args.sets.split(","):
        p = PARAM_SETS[name]
        alice, bob = R.SecretKey.new(p, 1), R.SecretKey.new(p, 2)
        pk = PR.PublicKeyLv0.new(bob, seed=3)
        size, w = pk.encryptions.shape
        out = {"n": p.n, "public_key_size": size, "encrypt": {}}
        e = R.Engine(p, 0)
        try:
            e.load_public_key(pk)
            for count in (int(c) for c in args.counts.split(",")):
                plain = np.random.default_rng(count).integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)
                tp = torch.from_numpy(plain.view(np.int32)).cuda()
                to = torch.empty((count, w), dtype=torch.int32, device="cuda")
                gpu = timed(lambda: e.batch_pk_encrypt_dev(tp, to, p.alpha_lv0, K, 0), args.reps)
                e.set_profiling(True)
                e.pk_encrypt_times()
                for _ in range(args.reps):
                    e.batch_pk_encrypt_dev(tp, to, p.alpha_lv0, K, 0)
                torch.cuda.synchronize()
                ev = e.pk_encrypt_times()
                e.set_profiling(False)
                words = to.cpu().numpy().view(np.uint32)
                host_ct = np.empty((count, w), np.uint32)
                # yardsticks: the numpy CPU form for the same rows, and staging the finished batch to the device
                cpu = host_timed(lambda: pk.encrypt_f64(np.zeros(count), p.alpha_lv0, rng_key=K), args.reps)
                ref = PR.encrypt_rows(pk.encryptions, K, np.arange(count, dtype=np.uint64), plain, p.alpha_lv0,
                                      (PR.DOMAIN_PKE_SEL, PR.DOMAIN_PKE_NOISE))
                host_ct[...] = ref
                stage = timed(lambda: to.copy_(torch.from_numpy(host_ct.view(np.int32))), args.reps)
                out["encrypt"][str(count)] = {
                    "batch_pk_encrypt_dev": gpu,
                    "selectors_ms": round(ev["selectors_ms"] / args.reps, 4),
                    "contraction_ms": round(ev["contraction_ms"] / args.reps, 4),
                    "numpy_cpu_form": cpu, "staged_upload": stage, "batch_mb": round(host_ct.nbytes / 1e6, 1),
                    "int8_ops": 2 * 4 * count * 32 * ((size + 31) // 32) * 256 * ((w + 255) // 256),
                    "gpu_and_cpu_words_differing": int((words != ref).sum())}
                print(name, count, json.dumps(out["encrypt"][str(count)]), flush=True)
            rows = p.n * p.iks_t * p.base
            with_dl = timed(lambda: e.gen_reenc_key_asymmetric(alice.key_lv0, rng_key=K), args.reps)
            no_dl = timed(lambda: e.gen_reenc_key_asymmetric(alice.key_lv0, rng_key=K, download=False), args.reps)
            key = e.gen_reenc_key_asymmetric(alice.key_lv0, rng_key=K)
            load = timed(lambda: e.load_reenc_key(key), args.reps)
        finally:
            e.close()
        cpu_key = host_timed(lambda: PR.ProxyReencryptionKey.new_asymmetric(alice, pk, rng_key=K), args.reps)
        ref_key = PR.ProxyReencryptionKey.new_asymmetric(alice, pk, rng_key=K).key_encryptions
        out["reenc_key"] = {"rows": rows, "key_mb": round(key.nbytes / 1e6, 1), "gen_reenc_key_asymmetric_download": with_dl,
                            "gen_reenc_key_asymmetric_no_download": no_dl, "numpy_cpu_form": cpu_key,
                            "load_reenc_key_host_key": load, "gpu_and_cpu_words_differing": int((key != ref_key).sum())}
        print(name, "reenc_key", json.dumps(out["reenc_key"]), flush=True)
        res["sets"][name] = out
    res["device"]["shader_mhz_after"] = shader_clock(R, PARAM_SETS["SECURITY_128_BIT"])
    with open(args.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
