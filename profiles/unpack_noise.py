"""Decode errors around the unpacking key switch on the CPU: the oracle makes the results, the integer models
(packing.pack_model / packing.unpack_model, which the GPU equals word for word) pack and unpack them.  Per set and
message modulus of packing's noise table:

  results        NAND outputs of the oracle for booleans, programmable-bootstrap outputs (a table x -> 3x + 1 mod m) for
                 a modulus m; where one bootstrap cannot evaluate a table of that modulus (its first 256 outputs already
                 decode wrong, as at UINT8 m = 256) fresh encryptions at alpha_lv0 stand in, and the row says so
  pack+unpack    the same results packed under a packing key at alpha_lv1 and unpacked under the cloud key's
                 key-switching key
  client-packed  SecretKey.encrypt_packed_* at alpha_lv1, unpacked

For each: decode errors and the largest |phase error| in units of the message's half-interval (1/8 for booleans,
1/(4m) for modulus m), and the deterministic rounding bounds of the two key switches over that half-interval:
n 2^-(beta t + 1) for packing, N 2^-(beta t + 1) for unpacking.

    python3 profiles/unpack_noise.py [--count 30720] [--out profiles/unpack_noise.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unpack_noise.json"))
    args = ap.parse_args()
    from oracle import oracle as O
    from rs_tfhe_amd import packing as PK
    from rs_tfhe_amd.client import SecretKey
    from rs_tfhe_amd.params import N, PARAM_SETS

    O.build()
    res = {"count": args.count, "rows": []}
    keys = {}
    for name, m in ROWS:
        p = PARAM_SETS[name]
        if name not in keys:
            osk, ock = O.keygen(getattr(O, name), 101)
            sk = SecretKey(p, osk.key_lv0, osk.key_lv1)
            pk = sk.packing_key(rng_key=102)
            keys = {name: (sk, ock, pk, PK.key_rows(p, pk.mask_seed, pk.bodies))}  # (one set's keys at a time)
        sk, ock, pk, rows = keys[name]
        ksk = ock.key_switching_key
        msgs = np.random.default_rng(m).integers(0, m, args.count)
        if m == 2:
            other = np.random.default_rng(m + 7).integers(0, 2, args.count).astype(bool)
            cts = O.batch_gate(ock, O.GATE_NAND, sk.encrypt_bool(msgs.astype(bool), seed=m + 1), sk.encrypt_bool(other, seed=m + 3))
            msgs = (~(msgs.astype(bool) & other)).astype(np.int64)
            source, scale, ideal = "oracle NAND outputs", 0.125, np.where(msgs == 1, 0.125, -0.125)
            client = sk.encrypt_packed_bool(msgs.astype(bool), seed=m + 2)
            decode = lambda c: sk.decrypt_bool(c).astype(np.int64)  # noqa: E731
        else:
            f = lambda x: (3 * x + 1) % m  # noqa: E731
            tv, fresh = O.lut_generate(f, m), sk.encrypt_lwe_message(msgs, m, seed=m + 1)
            probe = O.batch_bootstrap(ock, fresh[:256], testvec=tv)
            if np.array_equal(sk.decrypt_lwe_message(probe, m), f(msgs[:256])):
                source = "oracle programmable-bootstrap outputs"
                cts = np.concatenate([probe, O.batch_bootstrap(ock, fresh[256:], testvec=tv)]) if args.count > 256 else probe[:args.count]
                msgs = f(msgs)
            else:
                source, cts = "fresh encryptions at alpha_lv0 (one bootstrap cannot evaluate a table of this modulus)", fresh
            scale, ideal = 1.0 / (4 * m), msgs / (2.0 * m)
            client = sk.encrypt_packed_lwe_message(msgs, m, seed=m + 2)
            decode = lambda c: sk.decrypt_lwe_message(c, m)  # noqa: E731

        def stats(c):
            err = (sk.phase(c).astype(np.float64) / 2.0 ** 32 - ideal + 0.5) % 1.0 - 0.5
            return {"errors": int((decode(c) != msgs).sum()),
                    "max_abs_error_over_half_interval": round(float(np.abs(err).max() / scale), 4),
                    "std_error_over_half_interval": round(float(err.std() / scale), 5)}

        packed = PK.pack_model(p, pk.mask_seed, pk.bodies, cts, rows=rows)
        bt = p.basebit * p.iks_t
        row = {"params": name, "message_modulus": m, "inputs": args.count, "results_are": source,
               "pack_rounding_bound_over_half_interval": round(p.n * 2.0 ** -(bt + 1) / scale, 4),
               "unpack_rounding_bound_over_half_interval": round(N * 2.0 ** -(bt + 1) / scale, 4),
               "results": stats(cts),
               "pack_unpack": stats(PK.unpack_model(p, ksk, packed, args.count)),
               "client_packed_unpack": stats(PK.unpack_model(p, ksk, client, args.count))}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f)
        f.write("\n")


if __name__ == "__main__":
    main()
