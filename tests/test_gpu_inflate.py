"""bgzf_inflate_kernel through asm_bgzf_decompress / Engine.bgzf_decompress (docs/design/mapper.md, "Compressed input"): the corpus of
tests/bgzf_in_cases.py, which tests/test_inflate_host.py first runs through the host build of the same code under ASan + UBSan.
The device's bytes equal the host build's and zlib's, member by member and as one container of several hundred members; the corrupt
list gives the host's status and member; a second run gives the same bytes."""
import pytest

from tests import bgzf_in_cases as bi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus(asm):
    return dict(bi.good(), **bi.own_encoder(asm))


@pytest.fixture(scope="module")
def decoded(engine, corpus):
    return {name: engine.bgzf_decompress(data) for name, data in corpus.items()}


def test_corpus_equals_host_and_zlib(asm, corpus, decoded):
    for name, data in corpus.items():
        assert decoded[name] == bi.reference(data), name
        assert decoded[name] == asm.bgzf_decompress_host(data), name


def test_corpus_as_one_container(asm, engine, corpus, decoded):
    """one launch of several hundred members: the grid strides, and members start at every 16-byte phase of the output"""
    data = bi.as_one(list(corpus.values()) * 2)
    assert len(bi.split_members(data)) > 512           # more members than the grid has wavefronts
    out = engine.bgzf_decompress(data)
    assert out == b"".join(decoded.values()) * 2 == asm.bgzf_decompress_host(data)
    assert engine.bgzf_decompress(data) == out         # and the same bytes again
    assert len({len(b"".join(list(decoded.values())[:k])) % 16 for k in range(len(decoded))}) == 16


def test_corpus_twice(engine, corpus, decoded):
    for name, data in corpus.items():
        assert engine.bgzf_decompress(data) == decoded[name], name


@pytest.mark.parametrize("name", sorted(bi.corrupt()))
def test_corrupt_gives_the_hosts_error(asm, engine, name):
    data = bi.corrupt()[name][0]
    with pytest.raises(asm.AsmError) as host:
        asm.bgzf_decompress_host(data)
    with pytest.raises(asm.AsmError) as dev:
        engine.bgzf_decompress(data)
    assert dev.value.code == host.value.code == -1
    assert str(dev.value).replace("asm_bgzf_decompress:", "asm_bgzf_decompress_host:") == str(host.value)


def test_corrupt_members_in_a_long_container(asm, engine):
    """of several bad members in one launch the smallest is reported, whatever wavefront finishes first"""
    data, k, _ = bi.long_corrupt()          # tests/test_inflate_host.py runs it through the sanitizer build first
    with pytest.raises(asm.AsmError) as host:
        asm.bgzf_decompress_host(data)
    with pytest.raises(asm.AsmError) as dev:
        engine.bgzf_decompress(data)
    assert "BGZF member %d at offset" % k in str(dev.value) and "CRC-32 mismatch" in str(dev.value)
    assert str(dev.value).replace("asm_bgzf_decompress:", "asm_bgzf_decompress_host:") == str(host.value)


def test_seeded_corruptions_as_the_host(asm, engine):
    for data, ref in bi.seeded():
        try:
            host = asm.bgzf_decompress_host(data)
        except asm.AsmError as e:
            host = str(e)
        try:
            dev = engine.bgzf_decompress(data)
        except asm.AsmError as e:
            dev = str(e).replace("asm_bgzf_decompress:", "asm_bgzf_decompress_host:")
        assert dev == host
        assert isinstance(dev, str) or dev == ref


def test_plain_gzip_and_empty(asm, engine):
    import gzip

    with pytest.raises(asm.AsmError) as err:
        engine.bgzf_decompress(gzip.compress(b"@r\nACGT\n+\nIIII\n"))
    assert err.value.code == -4 and "plain gzip" in str(err.value) and "bgzip" in str(err.value)
    assert engine.bgzf_decompress(b"") == b"" and engine.bgzf_decompress(bi.EOF_BLOCK) == b""
