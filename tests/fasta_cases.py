"""FASTA files for the tests of asm_index_build_file and the parser they are checked against: written from the contract of the file
(docs/design/mapper.md, "Reference: FASTA in, index out"), not from the library's code and not from read_fasta, which strips only
the ends of a line."""
import random
import re


def py_parse(data: bytes):
    """-> (names, offsets of the sequences in the text, text)"""
    names, offs, text = [], [], bytearray()
    for line in data.split(b"\n"):  # a last piece without its newline is a line too; an empty one adds nothing
        if line[:1] == b">":
            body = line[1:-1] if line.endswith(b"\r") and len(line) > 1 else line[1:]
            names.append(re.split(rb"[ \t]", body.lstrip(b" \t"), maxsplit=1)[0])
            offs.append(len(text))
        elif names:
            text += bytes(c - 32 if 97 <= c <= 122 else c for c in line if c not in b" \t\r\n")
    return names, offs, bytes(text)


def lengths(offs, total):
    return [b - a for a, b in zip(offs, offs[1:] + [total])]


def bases(rng, n, alphabet="ACGTacgtNn"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def ugly_file(seed: int, scale: int) -> bytes:
    """Junk before the first header, headers with extra words and tabs, CRLF, a blank line, lower case, blanks and tabs inside sequence
    lines, an empty sequence, a '>' inside a line, no final newline.  scale: bases per full line group; 1 gives about 300 bytes."""
    rng = random.Random(seed)
    w = 11 * scale
    out = "junk line\nacgt before any header\n"
    out += ">chr1 first sequence\twith words\n" + "".join(bases(rng, w) + "\n" for _ in range(5))
    out += "\n" + bases(rng, w // 2) + " " + bases(rng, w // 2) + "\t" + bases(rng, 3) + "\n"
    out += "> \tchr2\tspaced name\r\n" + "".join(bases(rng, w) + "\r\n" for _ in range(4)) + bases(rng, 5) + ">" + bases(rng, 5) + "\r\n"
    out += ">empty\n"
    out += ">\n" + bases(rng, 7) + "\n"
    out += ">chr3\r\n" + "".join(bases(rng, w, "acgtn*-") + "\n" for _ in range(6)) + bases(rng, w // 3)
    return out.encode()


def random_small_file(rng) -> bytes:
    """up to about 200 bytes of lines of every kind, ends LF or CRLF, the last newline present or not"""
    out = []
    for _ in range(rng.randrange(0, 9)):
        eol = rng.choice(["\n", "\n", "\r\n"])
        kind = rng.randrange(8)
        if kind < 2:
            out.append(">" + rng.choice(["", " ", "\t ", "  "]) + bases(rng, rng.randrange(0, 20), "abXY_|>") +
                       rng.choice(["", " more words", "\tx"]) + eol)
        elif kind == 2:
            out.append(eol)
        else:
            out.append(bases(rng, rng.randrange(1, 40), "ACGTacgtnN >\t*-") + eol)
    data = "".join(out)
    if data and rng.random() < 0.5:
        data = data.rstrip("\r\n")
    return data.encode()
