"""The suite must NOTICE a wrong word in each integer kernel: every entry of the mutation catalogue (tests/mutants.py;
csrc/experiment.hpp TFHE_ABL_CATALOG, `make -C rs-tfhe_amd/csrc mutation` -> libtfhe_v_catalog.so, built by
__graft_entry__.build()) is switched on in a child pytest of its own -- TFHE_HIP_MUTANT=<name> -- that runs the entry's
killers and controls alone.  Every killer has to FAIL there, with an assertion error of its word-for-word comparison
and for no other reason, and every control has to pass; with no defect selected every killer passes on the same
library.  The children run one after another (this process holds no GPU context of its own), each under the time limit
of its entry (mutants.limit_seconds): a child that runs into it counts as hung and fails the case.  After a child
that hung, or that ended in an abort, a segmentation fault or a GPU fault, no further child is started: the cases that
remain fail without running anything."""
import os
import subprocess
import sys
import time
import xml.etree.ElementTree as ET

import pytest

import mutants as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "rs-tfhe_amd", "libtfhe_v_catalog.so")
COMPARISONS = ("array_equal", "compare_words")  # numpy's, and the key generators' helper (keygen_model.compare_words)


STOPPED = []  # why no further child is started: filled by the first child that hung or died (see the module's text)
DEATHS = (134, 139, -6, -11, 124, 137, -9)  # abort, segmentation fault (as a status and as a signal), a kill at a limit
FAULT_TEXT = ("illegal memory access", "HSA_STATUS_ERROR", "Segmentation fault", "core dumped")


def case_name(node_id):
    """the junit (classname, name) of a node id: the module with dots, the function with its parametrize id"""
    path, func = node_id.split("::", 1)
    return path[:-len(".py")].replace("/", "."), func


def run_child(mutant, node_ids, limit, out_dir, lib=LIB, tag=None):
    """One child pytest on `node_ids` against `lib` with `mutant` selected ("" for none), its junit file in `out_dir`:
    (return code, output, {junit (classname, name): (outcome, failure text)}, seconds).  Raises subprocess.TimeoutExpired at
    the limit; that, or a child that died, also sets STOPPED, after which every further call fails without a child."""
    if STOPPED:
        pytest.fail("not started: " + STOPPED[0])
    env = dict(os.environ, TFHE_HIP_LIB=lib, TFHE_HIP_ALLOW_EXPERIMENT="1", TFHE_HIP_MUTANT=mutant)
    xml = os.path.join(str(out_dir), "mutant_%s_junit.xml" % (tag or mutant or "none"))
    if os.path.exists(xml):
        os.remove(xml)
    t0 = time.monotonic()
    try:
        p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "--junitxml", xml]
                           + [os.path.join(ROOT, n) for n in node_ids], cwd=ROOT, env=env, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        STOPPED.append("the child of %r ran into its limit of %d s and counts as hung" % (mutant or "none", limit))
        raise
    seconds = time.monotonic() - t0
    if p.returncode in DEATHS or any(t in p.stdout + p.stderr for t in FAULT_TEXT):
        STOPPED.append("the child of %r died or faulted the GPU (return code %d)" % (mutant or "none", p.returncode))
        pytest.fail(STOPPED[0] + "\n" + (p.stdout + p.stderr)[-3000:])
    cases = {}
    if os.path.exists(xml):
        for case in ET.parse(xml).getroot().iter("testcase"):
            fail, err, skip = case.find("failure"), case.find("error"), case.find("skipped")
            outcome = "error" if err is not None else "failed" if fail is not None else "skipped" if skip is not None else "passed"
            text = (fail.get("message") or "") + (fail.text or "") if fail is not None else ""
            cases[(case.get("classname"), case.get("name"))] = (outcome, text)
    return p.returncode, p.stdout + p.stderr, cases, seconds


@pytest.fixture(scope="module")
def junit_dir(tmp_path_factory):
    """where the children leave their junit files"""
    return tmp_path_factory.mktemp("mutants")


@pytest.fixture(scope="module")
def catalogue_library():
    # built here if it is missing or older than its sources (`make` decides), as the other two mutation libraries are
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "rs-tfhe_amd", "csrc"), "mutation"], stdout=subprocess.DEVNULL)
    assert os.path.exists(LIB), "mutation build missing: make -C rs-tfhe_amd/csrc mutation"
    return LIB


def test_none_selected_every_killer_passes(catalogue_library, junit_dir):
    """The catalogue library with no defect selected computes the product's words: each failure below is its defect's."""
    killers = M.all_killers()
    try:
        rc, out, cases, seconds = run_child("", killers, M.limit_seconds(M.NONE_SECONDS), junit_dir)
    except subprocess.TimeoutExpired:
        pytest.fail(STOPPED[-1])
    print("MUTANT none: %d killers, %.1f s" % (len(killers), seconds))
    assert rc == 0, out[-3000:]
    for k in killers:
        assert cases.get(case_name(k), ("missing", ""))[0] == "passed", (k, cases.get(case_name(k)))


def test_an_unknown_name_is_refused(catalogue_library):
    """TFHE_HIP_MUTANT is looked up in the library's name table at context creation: no such name, no context."""
    if STOPPED:
        pytest.fail("not started: " + STOPPED[0])
    code = ("import sys; sys.path.insert(0, %r); import rs_tfhe_amd as R; from rs_tfhe_amd import _capi\n"
            "from rs_tfhe_amd.params import SECURITY_80_BIT as p\n"
            "try:\n    R.Engine(p, 0)\nexcept _capi.TfheHipError as e:\n    print('REFUSED', e.code == _capi.EINVAL, e)\n" % ROOT)
    env = dict(os.environ, TFHE_HIP_LIB=catalogue_library, TFHE_HIP_ALLOW_EXPERIMENT="1", TFHE_HIP_MUTANT="no_such_defect")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "REFUSED True" in p.stdout and "TFHE_HIP_MUTANT" in p.stdout, p.stdout + p.stderr


@pytest.mark.parametrize("entry", M.MUTANTS, ids=M.NAMES)
def test_mutant_is_caught(catalogue_library, junit_dir, entry):
    name, killers, controls = entry["name"], entry["killers"], entry["controls"]
    limit = M.limit_seconds(entry["seconds"])
    try:
        rc, out, cases, seconds = run_child(name, killers + controls, limit, junit_dir)
    except subprocess.TimeoutExpired:
        pytest.fail(STOPPED[-1])
    print("MUTANT %s: %.1f s of %d s" % (name, seconds, limit))
    assert rc == 1, out[-3000:]  # tests failed, and nothing else happened (no usage, internal or collection error)
    assert "ImportError" not in out and "Error loading" not in out and "OSError" not in out, out[-3000:]
    for k in killers:  # each fails, in the word-for-word comparison
        outcome, text = cases.get(case_name(k), ("missing", ""))
        assert outcome == "failed", (name, k, outcome, out[-2000:])
        assert "AssertionError" in text and any(c in text for c in COMPARISONS), (name, k, text[-1500:])
    for c in controls:
        assert cases.get(case_name(c), ("missing", ""))[0] == "passed", (name, c, cases.get(case_name(c)), out[-2000:])
