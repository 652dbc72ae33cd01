"""The BGZF container's decoder on the CPU (docs/design/mapper.md, "Compressed input"): host/inflate_host_check.cpp, built here plain
and under ASan + UBSan as a stand-alone program, runs the host build of csrc/asm_inflate.h (the code of bgzf_inflate_kernel's wave,
its lanes as a loop) on the corpus of tests/bgzf_in_cases.py; zlib is the reference.  Then the library's host calls."""
import ctypes
import os
import subprocess

import pytest

from tests import bgzf_in_cases as bi
from tests.test_map_file_host import san_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "approximate-string-matching_amd")
SRC = os.path.join(PKG, "host", "inflate_host_check.cpp")


def compiled(exe, flags):
    assert os.path.exists(SRC), "host/inflate_host_check.cpp: the host build of the BGZF decoder"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags + ["-o", exe, SRC], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def inflate_check(tmp_path_factory):
    return compiled(str(tmp_path_factory.mktemp("inflate_check") / "inflate_host_check_asan"), san_flags())


@pytest.fixture(scope="module")
def inflate_plain(tmp_path_factory):
    return compiled(str(tmp_path_factory.mktemp("inflate_plain") / "inflate_host_check"), ["-O2"])


def run(exe, data, tmp, stdin=False):
    """-> (container line, [(index, offset, csize, isize, status)], output bytes or None); a sanitizer report fails here"""
    inp, dst = tmp / "in.bgzf", tmp / "out.bin"
    inp.write_bytes(data)
    if dst.exists():
        dst.unlink()
    r = subprocess.run([exe, "-" if stdin else str(inp), str(dst)], input=data if stdin else None, capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stderr == b"", (r.returncode, r.stderr[-3000:])
    rows = [tuple(int(v) for v in ln.split()[1:]) for ln in r.stdout.decode().split("\n") if ln.startswith("container")]
    members = [tuple(int(v) for v in ln.split()) for ln in r.stdout.decode().split("\n") if ln and not ln.startswith("container")]
    assert len(rows) == 1
    return rows[0], members, dst.read_bytes() if dst.exists() else None


def first_bad(members):
    return next(((m[4], m[0]) for m in members if m[4]), (0, -1))


def test_good_corpus_equals_zlib(inflate_check, tmp_path):
    for name, data in bi.good().items():
        head, members, out = run(inflate_check, data, tmp_path)
        want = bi.reference(data)
        assert head == (0, len(members), members[-1][1] if members else 0, len(want)), name
        assert [(m[1], m[2]) for m in members] == [(at, len(m)) for at, m in bi.split_members(data)], name
        assert all(m[4] == bi.OK for m in members), (name, members)
        assert out == want, name


def test_own_encoder_round_trip(asm, inflate_check, tmp_path):
    """what this project writes, deflate and stored, read back by its decoder"""
    for name, data in bi.own_encoder(asm).items():
        head, members, out = run(inflate_check, data, tmp_path)
        assert head[0] == 0 and all(m[4] == bi.OK for m in members) and out == bi.reference(data), name
        kind, n = name.split()[3:]
        assert out == bi.source(kind, int(n)), name


def test_plain_build_and_stdin_agree(inflate_check, inflate_plain, tmp_path):
    for name in ("fastq in bgzip members", "empty members", "distance 32768", "only the EOF block"):
        data = bi.good()[name]
        assert run(inflate_plain, data, tmp_path) == run(inflate_check, data, tmp_path) == run(inflate_plain, data, tmp_path, stdin=True), name


@pytest.mark.parametrize("name", sorted(bi.corrupt()))
def test_corrupt_case_gives_its_class(inflate_check, tmp_path, name):
    data, where, index, cls = bi.corrupt()[name]
    head, members, out = run(inflate_check, data, tmp_path)
    if where == "container":
        assert head[:2] == (cls, index) and members == [] and out is None
        assert head[2] == bi.bad_offset(name)
    else:
        assert head[0] == 0 and first_bad(members) == (cls, index), (head, members)
        # the members around the bad one are sound and their bytes are there
        assert [m[4] for m in members if m[0] != index] == [0] * (len(members) - 1)
        assert out[:900] == bi.fastq_text()[:900]


def test_long_container_with_several_bad_members(inflate_check, tmp_path):
    """the composite that tests/test_gpu_inflate.py gives the kernel: the first bad member is the one reported"""
    data, index, cls = bi.long_corrupt()
    head, members, _ = run(inflate_check, data, tmp_path)
    assert head[0] == 0 and first_bad(members) == (cls, index) and sum(1 for m in members if m[4]) == 3


def test_every_class_has_a_case(inflate_check):
    """every status class the header defines (the checker's `classes` form prints them) has a case in the corrupt corpus, but for
    INF_E_TABLE, which the table-size argument rules out"""
    r = subprocess.run([inflate_check, "classes"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == ""
    rows = [ln.split(" ", 2) for ln in r.stdout.split("\n") if ln]
    member = {int(k) for kind, k, _ in rows if kind == "member"}
    container = {int(k) for kind, k, _ in rows if kind == "container"}
    assert member == set(range(16)) and container == set(range(6)) and all(text for _, _, text in rows)
    assert {cls for _, where, _, cls in bi.corrupt().values() if where == "member"} == member - {bi.OK, bi.E_TABLE}
    assert {cls for _, where, _, cls in bi.corrupt().values() if where == "container"} == container - {bi.IN_OK}


def test_seeded_corruptions(inflate_check, tmp_path):
    """a flipped bit in a dynamic member: an error, or zlib's bytes; never a sanitizer report, never a hang"""
    statuses = []
    for data, ref in bi.seeded():
        head, members, out = run(inflate_check, data, tmp_path)
        assert head[0] == 0 and len(members) == 2
        statuses.append(members[0][4])
        assert members[0][4] != bi.OK or out == ref
        if ref is None:
            assert members[0][4] != bi.OK
    print("statuses of the 32 corruptions:", statuses)
    assert len(set(statuses)) >= 3


def test_table_size_bound(inflate_check, tmp_path):
    """inf_build on code-length sets built to use the most subtable entries (chains below as many root indexes as the symbols pay for):
    the assert on the table's room does not fire, and the largest tables stay within the sizes of the design's argument"""
    for nsyms, root, cap in ((286, 10, 2536), (30, 8, 672)):
        cases = bi.table_cases(nsyms, root)
        assert len(cases) >= 10
        inp = tmp_path / "codes.txt"
        inp.write_text("".join(" ".join(map(str, lens)) + "\n" for lens in cases))
        r = subprocess.run([inflate_check, "tables", str(root), str(cap), "@" + str(inp)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
        rows = [tuple(int(v) for v in ln.split()) for ln in r.stdout.split("\n") if ln]
        assert len(rows) == len(cases) and all(kind == 0 for kind, _ in rows)
        most = max(used for _, used in rows)
        print("%d symbols under a root of %d bits: at most %d of %d entries" % (nsyms, root, most, cap))
        assert most <= cap      # the canonical order packs the long codes side by side, so the cases stay well below the bound
        assert most > (1 << root) + 128


# ---- through the library ---------------------------------------------------------------------------------------------------------------
def test_library_host_calls(asm):
    lib = asm.load_library()
    for name, data in dict(bi.good(), **bi.own_encoder(asm)).items():
        want = bi.reference(data)
        assert asm.bgzf_decompressed_size(data) == len(want) == sum(
            int.from_bytes(m[-4:], "little") for _, m in bi.split_members(data)), name
        assert asm.bgzf_decompress_host(data) == want, name
    # a short dst_cap is refused and dst stays as it was; so it does when a member is bad
    data = bi.good()["fastq in bgzip members"]
    size = asm.bgzf_decompressed_size(data)
    dst = ctypes.create_string_buffer(b"\x5a" * size, size)
    got = ctypes.c_size_t(77)
    assert lib.asm_bgzf_decompress_host(data, len(data), dst, size - 1, ctypes.byref(got)) == -1
    assert b"asm_bgzf_decompressed_size (%d bytes)" % size in lib.asm_last_error(None) and dst.raw == b"\x5a" * size
    bad = bi.corrupt()["CRC off by one"][0]
    assert lib.asm_bgzf_decompress_host(bad, len(bad), dst, size, ctypes.byref(got)) == -1 and dst.raw == b"\x5a" * size
    assert lib.asm_bgzf_decompress_host(None, 5, dst, size, ctypes.byref(got)) == -1
    assert lib.asm_bgzf_decompress_host(data, len(data), dst, size, None) == -1
    assert lib.asm_bgzf_decompress(None, data, len(data), dst, size, ctypes.byref(got)) == -1
    assert lib.asm_last_error(None) == b"asm_bgzf_decompress: NULL argument"


@pytest.mark.parametrize("name", sorted(bi.corrupt()))
def test_library_messages(asm, name):
    """ASM_EINVAL, the member's index, its offset and what is wrong"""
    data, where, index, cls = bi.corrupt()[name]
    with pytest.raises(asm.AsmError) as err:
        asm.bgzf_decompress_host(data)
    assert err.value.code == -1 and "BGZF member %d at offset %d: " % (index, bi.bad_offset(name)) in str(err.value), str(err.value)
    if where == "container":
        with pytest.raises(asm.AsmError):
            asm.bgzf_decompressed_size(data)
    else:
        assert asm.bgzf_decompressed_size(data) > 0        # the walk decodes nothing


def test_plain_gzip_is_refused(asm):
    import gzip

    plain = gzip.compress(bi.fastq_text()[:5000])
    for call in (asm.bgzf_decompress_host, asm.bgzf_decompressed_size):
        with pytest.raises(asm.AsmError) as err:
            call(plain)
        assert err.value.code == -4 and "plain gzip" in str(err.value) and "bgzip" in str(err.value)      # ASM_EUNSUPPORTED


# ---- the file calls' fill policy, device-free -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fill_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fill_check") / "bgzf_fill_host_check_asan")
    src = os.path.join(PKG, "host", "bgzf_fill_host_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + san_flags() + ["-o", exe, src, "-lpthread"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def filled(exe, path, want, slot=4096):
    r = subprocess.run([exe, str(path), str(want), str(slot)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-3000:])
    chunks, members, errors = [], [], []
    for ln in r.stdout.split("\n"):
        if ln.startswith("chunk"):
            chunks.append(tuple(int(v) for v in ln.split()[1:]))
        elif ln.startswith("error"):
            errors.append(tuple(int(v) for v in ln.split()[1:]))
        elif ln:
            members.append(tuple(int(v) for v in ln.split()))
    return chunks, members, errors


def test_fill_policy_ships_the_same_members(fill_check, tmp_path):
    """a 300-member file under want = 1, 27, 4 096 and 1 MiB: the same members in the same order, whole, each chunk's text reaching
    `want` with its last member and not before, the carry at most 64 KiB"""
    text = bi.fastq_text()
    sizes = [1, 7, 4099, 0, 65280, 300]
    parts, at = [], 0
    for k in range(300):
        parts.append(text[at % 150_000:at % 150_000 + sizes[k % len(sizes)]])
        at += len(parts[-1])
    data = b"".join(bi.good_member(bi.deflate(p, level=(0, 1, 6)[k % 3]), p) for k, p in enumerate(parts))
    path = tmp_path / "many.gz"
    path.write_bytes(data)
    want_members = [(k, off, len(m), len(parts[k]), zlib_crc(parts[k])) for k, (off, m) in enumerate(bi.split_members(data))]
    assert len(want_members) == 300
    for want in (1, 27, 4096, 1 << 20):
        chunks, members, errors = filled(fill_check, path, want)
        assert members == want_members and errors == [], want
        assert sum(c[0] for c in chunks) == 300 and [c[4] for c in chunks] == [0] * (len(chunks) - 1) + [1]
        k = 0
        for n, text_bytes, _, carry, eof in chunks:
            sizes_here = [m[3] for m in members[k:k + n]]
            assert sum(sizes_here) == text_bytes and (eof or (text_bytes >= want > text_bytes - sizes_here[-1])) and carry <= 65536
            k += n
    assert len(filled(fill_check, path, 1 << 20, slot=1 << 22)[0]) < len(filled(fill_check, path, 4096)[0])


def test_fill_policy_stops_at_a_bad_header(fill_check, tmp_path):
    for name in ("BSIZE past the file", "trailing bytes", "bad magic", "ISIZE 65537", "header cut short"):
        data, _, index, cls = bi.corrupt()[name]
        path = tmp_path / "bad.gz"
        path.write_bytes(data)
        for want in (1, 1 << 20):
            chunks, members, errors = filled(fill_check, path, want)
            assert errors == [(cls, index, bi.bad_offset(name))] and len(members) == index and chunks[-1][4] == 1, (name, want)


def zlib_crc(data):
    import zlib

    return zlib.crc32(data)
