"""The stand-alone host checks of tests/cpp/: one way to build one (`hipcc --cuda-host-only`: host code only, nothing for a GPU), to
run it and read what it prints, and to get the edge grid such a program writes for the device self-test to run the same operands.
The sanitizer builds are stand-alone programs run directly.  A plain module: the tests import it."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
# -ffp-contract=off / no fast-math: the arithmetic contract's operators (include/rt_detmath.h), as the library itself is built
FLAGS = ("-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math")
SANITIZE = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


def build(name, out_dir, *, sanitize, extra=("-Wno-unused-function",)):
    """tests/cpp/<name>.cpp built into out_dir; returns the program's path.  sanitize: True for AddressSanitizer and UBSan, False
    for none, or the sanitizer flags themselves; extra: further flags (later ones win: "-O1"), libraries ("-l...") go last"""
    assert os.path.exists(HIPCC), "hipcc is what builds this project: no build, no test"
    exe = os.path.join(str(out_dir), name)
    sanitizers = SANITIZE if sanitize is True else tuple(sanitize or ())
    flags, libs = [f for f in extra if not f.startswith("-l")], [f for f in extra if f.startswith("-l")]
    subprocess.run([HIPCC, *FLAGS, *flags, *sanitizers, "-o", exe, os.path.join(ROOT, "tests", "cpp", name + ".cpp"), *libs], check=True)
    return exe


def run(exe, *args, timeout):
    """the program run with args; its lines "<name> <integer> ..." as {name: (integers...)}.  A non-zero exit fails with its output."""
    done = subprocess.run([exe, *(str(a) for a in args)], capture_output=True, text=True, timeout=timeout)
    assert done.returncode == 0, done.stdout + done.stderr
    return {name: tuple(int(x) for x in rest) for name, *rest in (line.split() for line in done.stdout.splitlines())}


def edge_grid(name, width, tmp_path_factory):
    """(n, width) f32: the edge grid of tests/cpp/<name>.cpp, written out by that program itself (built here without the
    sanitizers), so that host and device run the very same operands"""
    d = tmp_path_factory.mktemp(name)
    out = str(d / "grid.bin")
    run(build(name, d, sanitize=False), out, timeout=120)
    return np.fromfile(out, dtype=np.float32).reshape(-1, width)
