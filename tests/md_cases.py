"""The MD:Z yardstick of tests/test_md_host.py (CPU) and tests/test_gpu_md.py (device): ref_md, written from the rule of
docs/design/mapper.md, "MD tag", and independent of csrc/asm_md.h; its inverse rebuild_window; and the checks a SAM file with
MD tags has to pass line by line.  A plain helper module: nothing is read from a file."""
import re

from tests.map_cases import cigar_ops
from tests.test_map_host import BASES, revcomp

MD_RE = re.compile(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*")
MD_MAX = 78   # 15 single-base deletions between 16 three-digit numbers: 3 * 16 + 15 + 15
MD_FIELD = re.compile(r"\tMD:Z:[^\t\n]*")


def letter(r):
    """a reference byte as the tag shows it"""
    return r if "A" <= r <= "Z" else "N"


def ref_md(cigar, qs, window):
    """The tag of `cigar` (a string of M, I and D runs) over q_s, the read on the alignment's strand in upper case, against the
    reference window T_r[pos, end).  An M column matches when both bytes are the same base of ACGT (N against N mismatches): the
    counter goes up; a mismatch writes the counter and the reference byte.  I skips read bases.  A D run writes the counter, '^'
    and the deleted bytes.  The counter is written at the end, always."""
    out, run, a, b = [], 0, 0, 0
    for cnt, op in cigar_ops(cigar):
        if op == "M":
            for _ in range(cnt):
                if qs[a] == window[b] and qs[a] in BASES:
                    run += 1
                else:
                    out.append("%d%s" % (run, letter(window[b])))
                    run = 0
                a, b = a + 1, b + 1
        elif op == "I":
            a += cnt
        else:
            out.append("%d^%s" % (run, "".join(letter(r) for r in window[b:b + cnt])))
            run, b = 0, b + cnt
    assert a == len(qs) and b == len(window), (cigar, len(qs), len(window))
    out.append("%d" % run)
    return "".join(out)


def md_letters(md):
    return sum(1 for c in md if "A" <= c <= "Z")


def inserted(cigar):
    return sum(cnt for cnt, op in cigar_ops(cigar) if op == "I")


def rebuild_window(cigar, qs, md):
    """the reference window that read + CIGAR + MD spell: a matched column repeats the read's base, a mismatch and a deletion show
    the reference byte"""
    tok = re.findall(r"(\d+)|\^([A-Z]+)|([A-Z])", md)
    t, run, a, out = 0, 0, 0, []

    def number():
        nonlocal t, run
        assert tok[t][0] != "", (md, t)
        run, t = int(tok[t][0]), t + 1

    number()
    for cnt, op in cigar_ops(cigar):
        if op == "M":
            for _ in range(cnt):
                if run:
                    out.append(qs[a])
                    run -= 1
                else:
                    assert tok[t][2] != "", (md, cigar, t)
                    out.append(tok[t][2])
                    t += 1
                    number()
                a += 1
        elif op == "I":
            a += cnt
        else:
            assert run == 0 and len(tok[t][1]) == cnt, (md, cigar, t)
            out.append(tok[t][1])
            t += 1
            number()
    assert run == 0 and t == len(tok) and a == len(qs), (md, cigar)
    return "".join(out)


def check_md(cigar, qs, window, md, dist=None):
    """what every tag must satisfy: the syntax, the bound, the window back (where the reference byte is a letter) and the invariant
    letters + inserted bases = edits"""
    assert MD_RE.fullmatch(md), md
    assert len(md) <= MD_MAX, (len(md), md)
    assert rebuild_window(cigar, qs, md) == "".join(letter(r) for r in window), (cigar, md)
    if dist is not None:
        assert md_letters(md) + inserted(cigar) == dist, (cigar, md, dist)


def check_sam_md(lines, read_of, refs, names):
    """Every line of a SAM body (no header lines): a line with a CIGAR other than '*' carries exactly one MD, directly behind XG,
    equal to ref_md of that line's own CIGAR, SEQ (the read of that QNAME and mate, turned to the line's strand, for a `SEQ *`
    line), POS and the reference; every other line carries none.  read_of(qname, flag) -> the read as its file holds it.  Returns
    the number of lines with a tag."""
    tagged = 0
    for ln in lines:
        cols = ln.split("\t")
        flag, cigar = int(cols[1]), cols[5]
        mds = [i for i, c in enumerate(cols) if c.startswith("MD:Z:")]
        if cigar == "*":
            assert not mds, ln
            continue
        assert len(mds) == 1 and cols[mds[0] - 1].startswith("XG:i:") and cols[mds[0] - 2].startswith("NM:i:"), ln
        qs = cols[9]
        if qs == "*":
            q = read_of(cols[0], flag).upper()
            qs = revcomp(q) if flag & 16 else q
        span = sum(cnt for cnt, op in cigar_ops(cigar) if op != "I")
        pos = int(cols[3]) - 1
        window = refs[names.index(cols[2])].upper()[pos:pos + span]
        md = cols[mds[0]][5:]
        assert md == ref_md(cigar, qs, window), ln
        check_md(cigar, qs, window, md, dist=int(cols[mds[0] - 2][5:]))
        tagged += 1
    return tagged


def strip_md(data: bytes) -> bytes:
    return re.sub(rb"\tMD:Z:[^\t\n]*", b"", data)
