"""The host halves of the device passes (csrc/*.h without device code) are checked by stand-alone programs, tools/<name>.cpp, that run
under the host sanitizers on the CPU.  run_host_check builds and runs one of them: the one recipe the tests of those passes share."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_host_check(name, tmp_path, args=()):
    """Compiles tools/<name>.cpp with ASan and UBSan, runs it once without arguments, which must print '<name>: ok', and, when `args` are
    given, once more with them.  Returns the last run (a CompletedProcess, exit status 0).  Skips without a host compiler or the
    sanitizers' runtime."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / name
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                            os.path.join(ROOT, "tools", name + ".cpp"), "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"cannot find .*(asan|ubsan)|unsupported option .*-fsanitize|libasan|libubsan", build.stderr):
        pytest.skip("the sanitizer runtime is not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and name + ": ok" in run.stdout, (run.returncode, run.stdout[-1000:], run.stderr[-2000:])
    if args:
        run = subprocess.run([str(exe)] + list(args), capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, (run.returncode, run.stdout[-1000:], run.stderr[-2000:])
    return run
