"""pack_kernel's per-thread pieces (csrc/asm_pack.h) on the CPU: host/pack_host_check.cpp, a stand-alone program built here under
ASan + UBSan, runs the very pack_vec and pack_cut_begin / pack_cut_granule the kernel calls and compares them with the oracle's own
conversion (planes_of of oracle/asm_oracle.c, compiled in unchanged through host/pack_oracle_planes.c).

  bytes   every byte value 0..255 at each of the 16 positions of a vector, the other 15 filled with bases and with non-bases: the
          plane bits equal the oracle's, and exactly 'C', 'G', 'T' set bits
  cut 1   strings of 0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128 characters at byte offsets 0..47 of the converted
          range (every off & 31, both off & 15), a 'T' right behind the string, unwritten plane dwords all ones
  cut 2   two granules: 129, 160, 255, 256 characters, the same offsets

The plane arrays have exactly the kernel's size (pack_plane_dwords), so a read past them fails the run.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "approximate-string-matching_amd")


def san_flags():
    """SAN_FLAGS of oracle/Makefile"""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as fh:
        for line in fh:
            if line.startswith("SAN_FLAGS :="):
                return line.split(":=", 1)[1].split()
    raise AssertionError("oracle/Makefile has no SAN_FLAGS")


@pytest.fixture(scope="module")
def pack_check(tmp_path_factory):
    """arguments -> the program's stdout"""
    tmp = tmp_path_factory.mktemp("pack_check")
    obj, exe = str(tmp / "pack_oracle_planes.o"), str(tmp / "pack_host_check_asan")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-ffp-contract=off"] + san_flags() +
                       ["-c", "-o", obj, os.path.join(PKG, "host", "pack_oracle_planes.c")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + san_flags() +
                       ["-o", exe, os.path.join(PKG, "host", "pack_host_check.cpp"), obj, "-lm"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(*args):
        p = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
        return p.stdout.strip()

    return run


def test_every_byte_value_at_every_vector_position(pack_check):
    assert pack_check("bytes") == "bytes %d ok" % (2 * 16 * 256)


def test_cut_one_granule(pack_check):
    assert pack_check("cut", "1") == "cut %d ok" % (14 * 48)


def test_cut_two_granules(pack_check):
    assert pack_check("cut", "2") == "cut %d ok" % (4 * 48)
