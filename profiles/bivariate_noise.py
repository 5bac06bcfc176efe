"""Tree bootstrap on the CPU oracle: which (parameter set, message modulus m, functions per rotation k) decode safely.

Per row: `inputs` pairs of fresh encryptions at alpha_lv0, a random m x m table, stage 1 on the oracle (the plain
bootstrap for k = 1, the many-LUT pre-rounding model otherwise), packing.table_model, then the oracle's bootstrap with one
test vector per ciphertext.  Recorded: decode errors, the worst and the rms phase error of the output over the decoding
half-interval 1/(4m), and the deterministic rounding bound of the table build n 2^-(basebit t + 1) over the same
half-interval (the rule of the packing table in DESIGN section 9: safe = at most half of it).  The GPU gives the same
table words, and on SECURITY_128_BIT the same output words; elsewhere its blind rotation differs from the oracle's by
rounding noise far below these figures.  Rows that are not run for lack of CPU time are written as "not run".

    python3 profiles/bivariate_noise.py [--inputs 3000] [--rows UINT4:4:1,UINT4:4:4,...] [--out profiles/bivariate_noise.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_ROWS = "UINT4:4:1,UINT4:4:4,UINT4:8:1,UINT4:8:2,UINT4:16:1,UINT8:16:1"


def many_model(O, ck, cts, tv, k):
    """The many-LUT bootstrap on the oracle: inputs rounded to multiples of 2^(21+d), the ordinary blind rotation,
    sample_extract_index(., j), the key switch -> [k][count][n+1]."""
    d = k.bit_length() - 1
    w = np.asarray(cts, np.uint64)
    wr = ((((w + (1 << (20 + d))) >> (21 + d)) << (21 + d)) & 0xFFFFFFFF).astype(np.uint32)
    tr = O.batch_blind_rotate(ck, wr, testvec=tv)
    return np.stack([O.batch_identity_key_switching(ck, np.stack([O.sample_extract_index(t, j) for t in tr])) for j in range(k)])


def run_row(O, name, m, k, inputs, chunk=512):
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd.lut import Generator
    from rs_tfhe_amd.params import N, PARAM_SETS

    p = PARAM_SETS["SECURITY_" + name]
    t0 = time.time()
    sk, ck = O.keygen(getattr(O, "SECURITY_" + name), 1234)
    pk = PK.make_packing_key(p, sk.key_lv0, sk.key_lv1, rng=4)
    rows = PK.key_rows(p, pk.mask_seed, pk.bodies)
    rng = np.random.default_rng(1000 * m + k)
    T = rng.integers(0, m, (m, m))
    tabs = Generator(m).generate_bivariate_tables(lambda x, y: int(T[x, y]), n_luts=k)
    half = (1 << 32) / (4 * m)
    errs, wrong = [], 0
    for lo in range(0, inputs, chunk):
        cnt = min(chunk, inputs - lo)
        xs, ys = rng.integers(0, m, cnt), rng.integers(0, m, cnt)
        cx, cy = sk.encrypt_lwe_message(xs, m, 11 + lo), sk.encrypt_lwe_message(ys, m, 12 + lo)
        if k == 1:
            stage1 = np.stack([O.batch_bootstrap(ck, cy, testvec=tabs[x]) for x in range(m)])
        else:
            stage1 = np.concatenate([many_model(O, ck, cy, tabs[j], k) for j in range(m // k)])
        tv = PK.table_model(p, pk.mask_seed, pk.bodies, stage1, m, rows=rows)
        out = O.batch_bootstrap(ck, cx, testvec=tv)
        want = T[xs, ys]
        wrong += int((sk.decrypt_lwe_message(out, m) != want).sum())
        enc = np.array([O.lut_encode(int(v), m) for v in want], np.uint32)
        errs.append(np.abs((sk.phase(out) - enc).astype(np.int32).astype(np.float64)) / half)
    e = np.concatenate(errs)
    bound = p.n * 2.0 ** -(p.basebit * p.iks_t + 1) * 4 * m
    return {"set": "SECURITY_" + name, "m": m, "k": k, "inputs": int(inputs), "bootstraps_per_input": m // k + 1,
            "decode_errors": wrong, "worst_error_over_half_interval": round(float(e.max()), 4),
            "rms_error_over_half_interval": round(float(np.sqrt((e ** 2).mean())), 4),
            "table_rounding_bound_over_half_interval": round(bound, 4), "safe_by_the_rounding_rule": bool(bound <= 0.5),
            "cpu_seconds": round(time.time() - t0, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", type=int, default=3000)
    ap.add_argument("--rows", default=DEFAULT_ROWS)
    ap.add_argument("--not-run", default="", help="rows to record as not run, same syntax")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bivariate_noise.json"))
    args = ap.parse_args()
    from oracle import oracle as O

    O.build()
    O.lib()
    res = {"method": "CPU oracle (oracle/), fresh encryptions at alpha_lv0, a random m x m table per row; stage 1 by the "
                     "oracle's bootstrap (k = 1) or the many-LUT pre-rounding model (k > 1), packing.table_model, then "
                     "the oracle's per-ciphertext bootstrap; errors are |phase - encode(f(x, y))| over 1/(4m)",
           "cpus_available": len(os.sched_getaffinity(0)), "rows": []}
    for spec in [s for s in args.rows.split(",") if s]:
        name, m, k = spec.split(":")
        row = run_row(O, name, int(m), int(k), args.inputs)
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
        with open(args.out, "w") as f:  # kept after every row: a long run can be cut short
            json.dump(res, f, indent=1)
            f.write("\n")
    for spec in [s for s in args.not_run.split(",") if s]:
        name, m, k = spec.split(":")
        res["rows"].append({"set": "SECURITY_" + name, "m": int(m), "k": int(k), "status": "not run (CPU time)"})
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
