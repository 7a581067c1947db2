"""The image walk of the per-crystal kernels (arreau_amd/csrc/crystal_dev.h: crystal_walk, crystal_walk_chunks and the index
arithmetic under them) against plain 64-bit e / M, e % M.  tests/crystal_walk_host.cpp is compiled with the host C++ compiler --
no HIP, no device -- under the address and undefined-behaviour sanitizers and run once.

Spans: 0, below and around one stride, a few multiples of M, walked whole by every lane (each entry met exactly once, every lane of a
chunked walk called in every round); 0xffffffff - stride and one above, the last span walked with 32-bit arithmetic and the first
walked with 64-bit arithmetic; 900 000 * 4913 > 2^32, the 64-bit walk no kernel test reaches.  The three large spans are walked from
span - 1000 - lane.  Strides 64 and 256; M = 27, 125, 4913, the image counts of 1, 2 and 8 shells."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = name and shutil.which(name)
        if path:
            return path
    pytest.fail("no host C++ compiler found (set CXX)")


def test_walk_matches_plain_division(tmp_path):
    exe = str(tmp_path / "crystal_walk_host")
    subprocess.run([_host_compiler(), "-std=c++20", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(HERE, "crystal_walk_host.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok "), run.stdout + run.stderr
    assert int(run.stdout.split()[1]) > 1_000_000  # (the checks were made: the small spans alone hold more entries than this)
