"""The BGZF container's deflate encoder on the CPU (docs/design/mapper.md, "Deflate"): host/deflate_host_check.cpp, built here under
ASan + UBSan, runs the host build of csrc/asm_deflate.h (the per-position code of bgzf_deflate_kernel, serially) on the corpus of
tests/deflate_cases.py; zlib inflates every block.  Then asm_bgzf_compress_host through the library, and its argument checks."""
import ctypes
import os
import subprocess
import zlib

import pytest

from tests import bam_cases as bc
from tests import deflate_cases as dc
from tests.test_map_file_host import san_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "approximate-string-matching_amd")


@pytest.fixture(scope="module")
def deflate_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("deflate_check") / "deflate_host_check_asan")
    src = os.path.join(PKG, "host", "deflate_host_check.cpp")
    assert os.path.exists(src), "host/deflate_host_check.cpp: the host build of the deflate encoder"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas"] + san_flags() + ["-o", exe, src], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def checked(deflate_check, tmp_path_factory):
    """{name: (container, [(payload length, BTYPE, block bytes)])} of the whole corpus, from the sanitizer-built checker"""
    tmp = tmp_path_factory.mktemp("deflate_corpus")
    out = {}
    for name, src in dc.corpus().items():
        inp, dst = tmp / "in.bin", tmp / "out.bgzf"
        inp.write_bytes(src)
        r = subprocess.run([deflate_check, str(inp), str(dst), "1"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.returncode, r.stderr[-3000:])      # a sanitizer report ends the run with another status
        assert r.stderr == "", (name, r.stderr[-3000:])
        out[name] = (dst.read_bytes(), [tuple(int(v) for v in ln.split()) for ln in r.stdout.split("\n") if ln])
    return out


def test_every_payload_inflates(checked):
    for name, src in dc.corpus().items():
        data, printed = checked[name]
        blocks = dc.check_container(data, src)
        assert printed == [(len(b["payload"]), dc.btype(b), b["bsize"]) for b in blocks], name


def test_incompressible_is_the_stored_container(checked):
    """Random bytes come out as the stored container, byte for byte.  Below 257 bytes the contract's own rule (the fewest bits wins)
    can prefer a fixed-Huffman block of literals: it costs 3 + 7 bits and 8 or 9 per byte against the stored block's 40 and 8 per
    byte, so it wins while fewer than 30 bytes are 144 or more.  There the expected type is worked out here, from the bytes."""
    for name, src in dc.corpus().items():
        if not (name.startswith("random ") or name == "copy at 32769"):
            continue
        data, at = checked[name][0], 0
        for k, (n, typ, bsize) in enumerate(checked[name][1]):
            part = src[k * dc.P:(k + 1) * dc.P]
            fixed = 10 + sum(8 if v < 144 else 9 for v in part)
            if n >= 257 or fixed >= 40 + 8 * n:
                assert data[at:at + bsize] == bc.frame_stored(part, eof=False), (name, k)
            else:
                assert (typ, bsize) == (1, 18 + (fixed + 7) // 8 + 8), (name, k)
            at += bsize


def test_compressible_is_smaller_in_every_full_block(checked):
    names = ["%s %d" % (kind, n) for kind in dc.COMPRESSIBLE for n in dc.SIZES if n >= dc.P]
    names += ["period %d" % p for p in dc.PERIODS if p <= 32768] + ["all bytes", "long run"]
    for name in names:
        for n, typ, bsize in checked[name][1]:
            if n == dc.P or name == "long run":
                assert typ != 0 and bsize < n + 31, (name, n, typ, bsize)


def test_corner_cases(checked):
    # one literal, no distance code: a fixed block of literal, end of block and padding
    data, printed = checked["one byte"]
    assert printed == [(1, 1, 18 + 3 + 8)]
    # the record fill is worth a dynamic block
    assert any(typ == 2 for _, typ, _ in checked["records %d" % (2 * dc.P + 1)][1])
    # zeros: a single literal, then matches only; far below a thirtieth
    assert checked["zeros %d" % dc.P][1][0][2] < dc.P // 20
    # a dynamic block's header alone is longer than a short payload's fixed block
    assert checked["random 4"][1][0][1] == 1 and checked["zeros 4"][1][0][1] == 1 and checked["text 63"][1][0][1] != 2


def test_record_fill_against_zlib(checked):
    """The record fill's container against zlib level 1 on the same blocks.  Measured on the 10^6-read workload (docs/design/mapper.md,
    "Deflate"): 0.9844 of zlib level 1; the cap is that plus a tenth, 1.083.  A changed hash or parse moves the ratio by a little, a
    broken match finder leaves Huffman coding alone and moves it to about 1.3."""
    name = "records %d" % (2 * dc.P + 1)
    src = dc.corpus()[name]
    ours = sum(bsize for _, _, bsize in checked[name][1])
    ref = 0
    for at in range(0, len(src), dc.P):
        z = zlib.compressobj(1, wbits=-15)
        ref += len(z.compress(src[at:at + dc.P]) + z.flush()) + 26
    print("record fill: %d bytes, zlib level 1: %d bytes, ratio %.4f" % (ours, ref, ours / ref))
    assert ours < len(src) + 31 * len(checked[name][1])
    assert ours <= 1.083 * ref


# ---- through the library ---------------------------------------------------------------------------------------------------------------
def compress_host(lib, src, level, eof=True, cap=None):
    bound = int(lib.asm_bgzf_bound(len(src), int(eof)))
    cap = bound if cap is None else cap
    out = ctypes.create_string_buffer(max(cap, 1))
    got = ctypes.c_size_t(12345)
    rc = lib.asm_bgzf_compress_host(src if src else None, len(src), int(eof), level, out, cap, ctypes.byref(got))
    return rc, out.raw[:got.value], got.value


def test_library_host_call_equals_the_checker(asm, checked):
    lib = asm.load_library()
    for name, src in dc.corpus().items():
        rc, data, _ = compress_host(lib, src, asm.BGZF_STORED)
        assert rc == 0 and data == bc.frame_stored(src), name
        rc, data, _ = compress_host(lib, src, asm.BGZF_DEFLATE)
        assert rc == 0 and data == checked[name][0], name
        assert asm.bgzf_compress_host(src, level=asm.BGZF_DEFLATE) == checked[name][0], name
    assert asm.bgzf_compress_host(b"", eof=True) == bc.EOF_BLOCK and asm.bgzf_compress_host(b"", eof=False) == b""
    src = dc.corpus()["text 1025"]
    assert asm.bgzf_compress_host(src, eof=False, level=1) + bc.EOF_BLOCK == checked["text 1025"][0]
    assert asm.bgzf_compress_host(src, level=0) == bc.frame_stored(src)


def test_library_argument_checks(asm):
    lib = asm.load_library()
    assert asm.BGZF_STORED == 0 and asm.BGZF_DEFLATE == 1
    src = dc.corpus()["text 1025"]
    for level in (-1, 2, 9):
        rc, _, got = compress_host(lib, src, level)
        assert rc == -1 and got == 12345 and b"level must be" in lib.asm_last_error(None)
    bound = int(lib.asm_bgzf_bound(len(src), 1))
    for level in (0, 1):                  # the bound holds at both levels, whatever the blocks come to
        out = ctypes.create_string_buffer(b"\x55" * bound, bound)
        got = ctypes.c_size_t(12345)
        assert lib.asm_bgzf_compress_host(src, len(src), 1, level, out, bound - 1, ctypes.byref(got)) == -1
        assert b"dst_cap is below asm_bgzf_bound" in lib.asm_last_error(None) and out.raw == b"\x55" * bound
    got = ctypes.c_size_t(0)
    assert lib.asm_bgzf_compress_host(None, 5, 1, 1, ctypes.create_string_buffer(100), 100, ctypes.byref(got)) == -1
    assert lib.asm_bgzf_compress_host(src, len(src), 1, 1, ctypes.create_string_buffer(bound), bound, None) == -1
    # the device call and the setter check the value first, then the handle; no device is touched
    assert lib.asm_bgzf_compress(None, src, len(src), 1, 7, ctypes.create_string_buffer(bound), bound, ctypes.byref(got)) == -1
    assert b"level must be" in lib.asm_last_error(None)
    assert lib.asm_bgzf_compress(None, src, len(src), 1, 1, ctypes.create_string_buffer(bound), bound, ctypes.byref(got)) == -1
    assert lib.asm_last_error(None) == b"asm_bgzf_compress: NULL argument"
    assert lib.asm_map_set_bgzf_level(None, 2) == -1 and b"level must be" in lib.asm_last_error(None)
    assert lib.asm_map_set_bgzf_level(None, 1) == -1 and lib.asm_last_error(None) == b"asm_map_set_bgzf_level: NULL handle"
    assert lib.asm_map_get_bgzf_level(None) == asm.BGZF_STORED
