"""The mutation catalogue (tests/mutants.py) against the sources and the suite, without a GPU: the names the library
knows are the names the catalogue lists, every site uses a listed name and every listed name has a site in the file its
entry names, and every killer and control is a test that exists."""
import ast
import os
import re

import mutants as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rs-tfhe_amd", "csrc")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _sources():
    return {f: _read(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hpp", ".hip"))}


def _listed_names():
    """the X(...) entries of TFHE_MUTANT_LIST in experiment.hpp"""
    src = _read(CSRC, "experiment.hpp")
    m = re.search(r"#define TFHE_MUTANT_LIST\(X\)((?:[^\n]*\\\n)*[^\n]*)\n", src)
    assert m, "experiment.hpp: TFHE_MUTANT_LIST not found"
    return re.findall(r"\bX\((\w+)\)", m.group(1))


def test_the_library_and_the_catalogue_name_the_same_defects():
    listed = _listed_names()
    assert len(listed) == len(set(listed)) and len(M.NAMES) == len(set(M.NAMES))
    assert set(listed) == set(M.NAMES), set(listed) ^ set(M.NAMES)
    assert len(M.NAMES) >= 24
    # the enumerators and the name table TFHE_HIP_MUTANT is looked up in are both made from that one list, and nowhere else
    exp, core = _read(CSRC, "experiment.hpp"), _read(CSRC, "tfhe_hip.hip")
    assert re.search(r"#define TFHE_MUTANT_ENUM\(name\) kMut_##name,\s*\nenum TfheMutant : unsigned \{ kMutNone = 0, TFHE_MUTANT_LIST\(TFHE_MUTANT_ENUM\) kMutCount \};", exp)
    assert re.search(r"#define TFHE_MUTANT_NAME\(name\) \{#name, kMut_##name\},", core)
    assert re.search(r"kMutantNames\[\] = \{TFHE_MUTANT_LIST\(TFHE_MUTANT_NAME\)\};", core)
    for f, src in _sources().items():  # no enumerator is written out by hand
        assert not re.search(r"\bkMut_\w+\s*=", src), f
    # creation refuses what the table does not hold, and only the catalogue build reads the variable
    assert re.search(r"#if TFHE_ABL_CATALOG\n\s*const int mutant = mutant_lookup\(getenv\(\"TFHE_HIP_MUTANT\"\)\);\n\s*if \(mutant < 0\) \{[^}]*return TFHE_HIP_EINVAL;", core)
    assert sum(src.count("TFHE_HIP_MUTANT") for src in _sources().values()) == sum(
        src.count("TFHE_HIP_MUTANT") for f, src in _sources().items() if f in ("experiment.hpp", "tfhe_hip.hip"))


def test_every_site_uses_a_listed_name_and_every_name_has_a_site_in_its_file():
    sites = {}  # name -> files
    for f, src in _sources().items():
        if f == "experiment.hpp":  # the macro's definitions and its description: no kernel, no site
            continue
        for arg in re.findall(r"\bTFHE_MUT\(([^()]*)\)", src):
            m = re.fullmatch(r"kMut_(\w+)", arg.strip())
            assert m, (f, arg)
            assert m.group(1) in M.NAMES, (f, arg)
            sites.setdefault(m.group(1), set()).add(f)
    for e in M.MUTANTS:
        assert e["file"] in sites.get(e["name"], ()), (e["name"], e["file"], sites.get(e["name"]))
        assert sites[e["name"]] == {e["file"]}, (e["name"], sites[e["name"]])  # one defect, one file
    # the kernels the issue keeps free of sites
    for f in ("blind_rotate.hpp", "blind_rotate_wide.hpp", "fft512.hpp"):
        assert "TFHE_MUT(" not in _sources()[f], f
    mfma = _sources()["key_switch_mfma.hpp"]
    assert mfma.count("TFHE_MUT(") == 1 and "TFHE_MUT(" not in mfma[mfma.index("void k_key_switch_mfma("):]  # ks_plane_byte alone


def _test_functions(path):
    """{function name: [parametrize decorators as (argnames, values node, ids node)]} of a test module, by its syntax"""
    out = {}
    for node in ast.parse(_read(ROOT, path)).body:
        if isinstance(node, ast.FunctionDef) and node.name.startswith("test_"):
            out[node.name] = [d for d in node.decorator_list if isinstance(d, ast.Call) and ast.unparse(d.func).endswith("parametrize")]
    return out


def _collected_ids():
    """node ids as pytest collects them (collection imports no device code: the GPU modules import it inside the tests)"""
    import subprocess
    import sys

    files = sorted({n.split("::")[0] for e in M.MUTANTS for n in e["killers"] + e["controls"]})
    p = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + files, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return {line.strip() for line in p.stdout.splitlines() if "::" in line}


def test_killers_and_controls_are_tests_that_exist():
    ids = _collected_ids()
    for e in M.MUTANTS:
        assert len(e["killers"]) >= 1, e["name"]
        assert set(e["killers"]) != set(e["controls"]) and not set(e["killers"]) & set(e["controls"]), e["name"]
        assert len(e["controls"]) >= 1, e["name"]
        killer_files = {k.split("::")[0] for k in e["killers"]}
        for n in e["killers"] + e["controls"]:
            path, func = n.split("::")
            name = func.split("[")[0]
            assert os.path.exists(os.path.join(ROOT, path)), n
            funcs = _test_functions(path)
            assert name in funcs, n
            assert ("[" in func) == bool(funcs[name]), n  # a parametrized test is named with the id of one case
            assert n in ids, n  # ... and that id exists
        for c in e["controls"]:
            assert c.split("::")[0] in killer_files, (e["name"], c)  # a control lives in a killer's file


def test_entries_are_complete():
    for e in M.MUTANTS:
        assert os.path.exists(os.path.join(CSRC, e["file"])), e
        assert e["kernel"] and e["what"].endswith((".", ".)")) and e["found_by"] in ("existing", "new"), e
        assert e["seconds"] > 0 and M.limit_seconds(e["seconds"]) % 10 == 0 and M.limit_seconds(e["seconds"]) >= 3 * e["seconds"], e
    assert M.limit_seconds(3.4) == 20 and M.limit_seconds(10.0) == 30 and M.limit_seconds(0.1) == 10
