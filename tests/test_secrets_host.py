"""The one path for secrets and plaintexts through the library's buffers (csrc/secrets.hpp), the part a CPU can check:
tests/cpp/test_secret_stage.cpp compiles the header as the library does, over stand-ins for the HIP runtime that work on
host memory and can be made to fail, and holds SecretStage and scrub to their promises on every exit path.  The program
runs twice: as built, and under AddressSanitizer + UBSan (host code, its own main, nothing preloaded)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_secret_stage_program(outdir, sanitize=False):
    exe = os.path.join(outdir, "test_secret_stage" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O3"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unused-function"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "test_secret_stage.cpp")])
    return exe


def test_secret_stage_and_scrub(tmp_path):
    for sanitize in (False, True):
        r = subprocess.run([build_secret_stage_program(str(tmp_path), sanitize)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert r.stdout.startswith("secret stage ok"), r.stdout
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
