"""Writes tests/golden/reference_params.json: the numbers of every SecurityParams constant of the reference's src/params.rs
(n, l, bgbit, basebit, t, alpha lv0, alpha lv1, N per set; no source text), read from the reference tree
(run in the build container).  tests/test_host_logic.py holds the product's table and the C++ mirror's to these numbers
and, where the reference tree is present, re-reads them and compares."""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_reference_signatures import REF  # noqa: E402


def collect(ref=REF) -> dict:
    """name -> [n, l, bgbit, basebit, t, alpha_lv0, alpha_lv1, N]"""
    src = re.sub(r"//[^\n]*", "", open(os.path.join(ref, "params.rs")).read()).replace("_", "")  # comments, digit separators
    found = {}
    for m in re.finditer(r"pub const (SECURITY[A-Z0-9]+): SecurityParams = SecurityParams \{(.*?)\n\};", src, re.S):
        body = m.group(2)
        lv0 = re.search(r"tlwelv0: TlweParams \{\s*n: (\d+),\s*alpha: ([0-9.e+-]+)", body)
        lv1 = re.search(r"tlwelv1: TlweParams \{\s*n: (\d+),\s*alpha: ([0-9.e+-]+)", body)
        g = re.search(r"trgswlv1: TrgswParams \{(.*?)\}", body, re.S).group(1)
        f = {k: re.search(rf"\b{k}: ([0-9.e+-]+)", g).group(1) for k in ("n", "bgbit", "l", "basebit", "ikst")}
        name = m.group(1).replace("SECURITY", "SECURITY_").replace("BIT", "_BIT")
        found[name] = [int(lv0.group(1)), int(f["l"]), int(f["bgbit"]), int(f["basebit"]), int(f["ikst"]),
                       float(lv0.group(2)), float(lv1.group(2)), int(f["n"])]
    return found


if __name__ == "__main__":
    dst = os.path.join(HERE, "reference_params.json")
    json.dump(collect(), open(dst, "w"), indent=1, sort_keys=True)
    print("wrote", dst, file=sys.stderr)
