"""The owners of the library's device buffers, pinned arenas and timing events (csrc/resources.hpp), the part a CPU can
check: tests/cpp/test_resources.cpp compiles the header as the library does, over stand-ins for the HIP runtime that keep
a set of live objects and a log and can make any one call fail, and holds the owners to their rules: nothing left
behind, freed twice or used after it was freed whichever call fails; how buffers and arenas grow; what sizing a scratch
buffer synchronises; that a timed stretch closes its event pair once however it is left; what a failed collection of
the timing pairs leaves.  The program runs twice: as built, and under AddressSanitizer + UBSan (host code, its own main,
nothing preloaded)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_resources_program(outdir, sanitize=False):
    exe = os.path.join(outdir, "test_resources" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O3"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unused-function"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "test_resources.cpp")])
    return exe


def test_owners_leave_nothing_behind_and_keep_their_rules(tmp_path):
    for sanitize in (False, True):
        r = subprocess.run([build_resources_program(str(tmp_path), sanitize)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert r.stdout.startswith("resources ok"), r.stdout
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
