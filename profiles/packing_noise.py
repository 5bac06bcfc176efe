"""Decode errors of packed results on the CPU integer model (packing.pack_model, which the GPU equals word for word):
fresh lv0 encryptions at the set's alpha_lv0 (the noise level of a bootstrapped, key-switched result) packed under a
packing key at alpha_lv1, decrypted from the packed TRLWEs, counted against the messages.  Also the largest |phase
error| seen, in units of the message's half-interval (1/4 for booleans, 1/(4m) for modulus m): decoding is safe while
that stays well below 1.

    python3 profiles/packing_noise.py [--count 30720] [--out profiles/packing_noise.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = (("SECURITY_128_BIT", 2), ("SECURITY_80_BIT", 2), ("SECURITY_UINT4", 4), ("SECURITY_UINT4", 8),
        ("SECURITY_UINT4", 16), ("SECURITY_UINT4", 32), ("SECURITY_UINT8", 8), ("SECURITY_UINT8", 16), ("SECURITY_UINT8", 256))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=30 * 1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packing_noise.json"))
    args = ap.parse_args()
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.params import PARAM_SETS

    res = {"count": args.count, "inputs": "fresh encrypt_bool / encrypt_lwe_message at alpha_lv0", "rows": []}
    keys = {}
    for name, m in ROWS:
        p = PARAM_SETS[name]
        if name not in keys:
            sk = SecretKey.new(p, 101)
            pk = sk.packing_key(rng_key=102)
            keys[name] = (sk, pk, PK.key_rows(p, pk.mask_seed, pk.bodies))
        sk, pk, rows = keys[name]
        msgs = np.random.default_rng(m).integers(0, m, args.count)
        if m == 2:
            cts, scale = sk.encrypt_bool(msgs.astype(bool), seed=m + 1), 0.125
            ideal = np.where(msgs == 1, 0.125, -0.125)
        else:
            cts, scale = sk.encrypt_lwe_message(msgs, m, seed=m + 1), 1.0 / (4 * m)
            ideal = msgs / (2.0 * m)
        packed = PK.pack_model(p, pk.mask_seed, pk.bodies, cts, rows=rows)
        if m == 2:
            errors = int((sk.decrypt_packed_bool(packed, args.count) != msgs.astype(bool)).sum())
        else:
            errors = int((sk.decrypt_packed_lwe_message(packed, args.count, m) != msgs).sum())
        phase = sk.packed_phase(packed, args.count).astype(np.float64) / 2.0 ** 32
        err = (phase - ideal + 0.5) % 1.0 - 0.5
        row = {"params": name, "message_modulus": m, "errors": errors, "inputs": args.count,
               "max_abs_error_over_half_interval": round(float(np.abs(err).max() / scale), 4),
               "std_error": float(err.std())}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
