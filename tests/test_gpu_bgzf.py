"""bgzf_frame_kernel through asm_bgzf_frame / Engine.bgzf_frame (docs/design/mapper.md, "BAM output"): host bytes in, BGZF blocks
of stored deflate out, framed on the device.  The sizes are the kernel's edges: a thread's slice of 64 bytes and its dwords, the
block of 65,280 bytes, and one byte to either side of each; the fills are zeros, 0xff and random bytes.  Every byte is checked:
the 18 header bytes of every block, BSIZE, the stored-block header, the payload, the CRC against zlib.crc32, ISIZE, and the EOF
block."""
import ctypes
import gzip
import random
import struct
import zlib

import pytest

from tests import bam_cases as bc

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 65279, 65280, 65281, 2 * 65280, 2 * 65280 + 1)


def fill(kind, n):
    return {"zeros": bytes(n), "ones": b"\xff" * n, "random": random.Random(n + 1).randbytes(n)}[kind]


@pytest.mark.parametrize("kind", ["zeros", "ones", "random"])
@pytest.mark.parametrize("n", SIZES)
def test_frame(asm, engine, n, kind):
    src = fill(kind, n)
    for eof in (True, False):
        out = engine.bgzf_frame(src, eof=eof)
        assert len(out) == bc.bgzf_bound(n, eof) == engine.lib.asm_bgzf_bound(n, int(eof))
        blocks = bc.bgzf_blocks(out)                      # fixed header bytes, CRC == zlib.crc32(payload), ISIZE
        body = bc.check_stored(blocks, eof)               # BSIZE, 01 LEN ~LEN, payloads full except the last, the EOF block's bytes
        assert len(body) == (n + bc.PAYLOAD - 1) // bc.PAYLOAD
        assert [b["payload"] for b in body] == [src[a:a + bc.PAYLOAD] for a in range(0, n, bc.PAYLOAD)]
        assert [b["crc"] for b in body] == [zlib.crc32(b["payload"]) for b in body]
        if eof:
            assert out[-28:] == bc.EOF_BLOCK
        assert out == bc.frame_stored(src, eof)
        if out:
            assert gzip.decompress(out) == src
    # a short dst_cap is refused and dst stays as it was
    cap = bc.bgzf_bound(n, True)
    dst = ctypes.create_string_buffer(b"\xa5" * (cap + 8), cap + 8)
    got = ctypes.c_size_t(77)
    rc = engine.lib.asm_bgzf_frame(engine.h, src if src else None, n, 1, dst, cap - 1, ctypes.byref(got))
    assert rc == -1 and b"asm_bgzf_bound" in engine.lib.asm_last_error(engine.h)
    assert dst.raw == b"\xa5" * (cap + 8)
    # the exact cap: nothing behind it is written
    rc = engine.lib.asm_bgzf_frame(engine.h, src if src else None, n, 1, dst, cap, ctypes.byref(got))
    assert rc == 0 and got.value == cap and dst.raw[:cap] == bc.frame_stored(src) and dst.raw[cap:] == b"\xa5" * 8


def test_constants_and_arguments(asm, engine):
    assert asm.BGZF_PAYLOAD == bc.PAYLOAD == 65280
    assert engine.bgzf_frame(b"", eof=False) == b"" and engine.bgzf_frame(b"") == bc.EOF_BLOCK
    got = ctypes.c_size_t(0)
    assert engine.lib.asm_bgzf_frame(engine.h, None, 5, 1, ctypes.create_string_buffer(100), 100, ctypes.byref(got)) == -1
    assert engine.lib.asm_bgzf_frame(None, b"abc", 3, 1, ctypes.create_string_buffer(100), 100, ctypes.byref(got)) == -1
    # the header of a block, spelled out once
    one = engine.bgzf_frame(b"abc", eof=False)
    assert one == bytes.fromhex("1f8b08040000000000ff0600424302002100" "0103 00fcff".replace(" ", "")) + b"abc" + struct.pack(
        "<II", zlib.crc32(b"abc"), 3)
