"""csrc/arena.h - the allocator that decides the address of every activation of a UNet forward - against a brute-force model, under
AddressSanitizer and UndefinedBehaviorSanitizer.  tests/arena_check.cpp is a stand-alone program with its own main: it drives seeded
sequences of a few thousand alloc / release calls through a tight arena, an ample one and a dry one, and after every call checks that
live blocks never overlap, offsets are 256-aligned, a zero-byte request gets 256 bytes, first fit picks the lowest offset that fits, alloc
refuses exactly when nothing fits, peak is the largest end offset ever live, release(nullptr) and release of an unknown pointer change
nothing, the dry arena places like the ample real one, and releasing everything coalesces back to one free block.  No GPU, no Python
in the process under the sanitizers."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_arena_against_a_model_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no C++ compiler on this box")
    exe = tmp_path / "arena_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "invertible_cd_amd", "csrc"), os.path.join(ROOT, "tests", "arena_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("arena: ok"), r.stdout[-2000:] + r.stderr[-4000:]
