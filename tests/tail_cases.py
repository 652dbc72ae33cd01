"""Inputs and expectations for the sequential-mode tail planes (csrc/asm_tails.h), needing no GPU.

What a sequential-mode batch's packed planes must hold is fully determined by the 2 x 128 bytes that every pair's conversion
sees (`oracle.greedy_views(hb, 0)`, pinned to the compiled reference by test_oracle_vs_reference.py::test_stale_tail_model):
granule 0 is those bytes' 2-bit codes, whatever wrote them.  `expected_planes` turns the views into the bucketed uint4 planes
that `DeviceBatch.download_planes()` returns; the builders below make batches whose views carry OLD bytes across the
resolver's seams (40-pair chunks, 5120-pair workgroups, the carry kernel's segments), which generated 100 bp data never does:
a string of 100 characters rewrites every slot whose orbit under the conversion's permutation meets 0..99, and only four
slots' orbits do not (test_tail_cases_host.py asserts the orbit facts from the permutation's definition).

Vocabulary: a *plant* is a pair with 128-300 characters from CGT on both sides, so it rewrites both whole buffers with non-zero
codes; a *coasting* pair has 0..coast_max characters per side and leaves every slot alone whose orbit avoids the slots below
coast_max (122 of 128 at coast_max = 2), so a plant's bytes stay visible, permuted, until the next plant."""
import numpy as np

from approximate_string_matching_amd import HostBatch

LUT = np.zeros(256, np.uint8)
LUT[ord("C")], LUT[ord("G")], LUT[ord("T")] = 1, 2, 3

CHUNK, GROUP_PAIRS, CARRY_SEGS = 40, 40 * 128, 32   # asm_tails.h: TAIL_CHUNK, TAIL_CHUNK * TAIL_GROUP, TAIL_CARRY_SEGS
MID_LENGTHS = (3, 4, 8, 16, 32, 64, 129)

# The conversion's in-place permutation, from its definition (bit_convert.cpp:265-330): after[q] = before[SRC[q]].
PERM_P = (0, 2, 1, 3, 4, 6, 5, 7)
SRC = np.array([8 * (q % 16) + PERM_P[q // 16] for q in range(128)])


def orbits():
    """The cycles of SRC as lists of slots."""
    seen, out = set(), []
    for q in range(128):
        if q not in seen:
            orb, x = [], q
            while x not in seen:
                seen.add(x)
                orb.append(x)
                x = int(SRC[x])
            out.append(orb)
    return out


def survivors(length):
    """Slots whose orbit never enters [0, length): a byte there outlives any run of pairs of at most `length` characters."""
    return sorted(q for orb in orbits() if min(orb) >= length for q in orb)


# ---- seams ------------------------------------------------------------------------------------------------------------
def seam_pairs(n):
    """{kind: period} of the resolver's seams for a batch of n pairs; a seam pair is the first pair behind a boundary, i.e. every
    multiple t of the period with 0 < t < n.  'segment' is there when the carry kernel folds more than one workgroup per
    thread (more than 32 workgroups, n > 163 840; three per thread from 65 workgroups, n > 327 680)."""
    ngroups = -(-(-(-n // CHUNK)) // 128)
    per = -(-ngroups // CARRY_SEGS)
    kinds = {"chunk": CHUNK, "workgroup": GROUP_PAIRS}
    if per > 1:
        kinds["segment"] = per * GROUP_PAIRS
    return {k: p for k, p in kinds.items() if p < n}


def nearest_seam(t, n):
    """(distance, kind, boundary) of the seam boundary nearest to pair t, the widest kind winning ties."""
    best = None
    for kind, period in seam_pairs(n).items():
        b = int(round(t / period)) * period
        if 0 < b < n and (best is None or abs(t - b) <= best[0]):
            best = (abs(t - b), kind, b)
    return best


# ---- expectation --------------------------------------------------------------------------------------------------------
def bucket_layout(m, nn, order, planes_entries):
    """[(lo, hi, w4, base)]: slots [lo, hi) of the bucketed order hold pairs of w4 granules, their uint4[4][w4][hi - lo] block
    starts at entry `base` (one bucket of the batch's widest class, or one per width class present)."""
    n = len(m)
    maxlen = int(max(m.max(initial=0), nn.max(initial=0)))
    wmax = 1 if maxlen <= 128 else (maxlen + 127) // 128
    if planes_entries == 4 * wmax * max(n, 1) or n == 0:
        spans = [(0, n, wmax)]
    else:
        cls = np.minimum((np.maximum(np.maximum(m, nn), 1)[order] + 127) // 128 - 1, 3)
        assert np.all(np.diff(cls) >= 0), "order is not sorted by width class"
        spans = [(int(np.searchsorted(cls, c)), int(np.searchsorted(cls, c, "right")), int(c) + 1) for c in np.unique(cls)]
    out, base = [], 0
    for lo, hi, w4 in spans:
        out.append((lo, hi, w4, base))
        base += 4 * w4 * (hi - lo)
    return out


def host_order(hb, bucketed):
    """(order, planes_entries) as the device lays a batch out: input order in one bucket, or a stable sort by width class."""
    m, nn = hb.lengths()
    if not bucketed:
        maxlen = int(max(m.max(initial=0), nn.max(initial=0)))
        return np.arange(hb.n), 4 * (1 if maxlen <= 128 else (maxlen + 127) // 128) * max(hb.n, 1)
    cls = np.minimum((np.maximum(np.maximum(m, nn), 1) + 127) // 128 - 1, 3)
    return np.argsort(cls, kind="stable"), int(4 * (cls + 1).sum())


def _pack128(bits):
    """(..., 128) of 0/1 -> (..., 4) uint32, bit q of the 128 = position q."""
    return np.packbits(bits.astype(np.uint8), axis=-1, bitorder="little").view("<u4")


def _upper_granules(text, off, length, idx, w4):
    """(len(idx), 2 planes, w4 - 1, 4): granules 1.. of the strings idx of one side, by the clean rule (bits beyond the end 0)."""
    text = np.concatenate([np.asarray(text, np.uint8), np.zeros(w4 * 128, np.uint8)])
    col = np.arange(128, w4 * 128)
    codes = LUT[text[off[idx][:, None] + col[None, :]]]
    codes[col[None, :] >= length[idx][:, None]] = 0
    out = np.empty((len(idx), 2, w4 - 1, 4), np.uint32)
    for p in range(2):
        out[:, p] = _pack128(((codes >> p) & 1).reshape(len(idx), w4 - 1, 128))
    return out


def expected_planes(hb, views, order, planes_entries):
    """(planes uint32[planes_entries, 4], lens uint32[n]) of a sequential-mode batch whose conversions see `views`
    (uint8[n, 2, 128]): granule 0 of side s, plane p, pair t is bit p of the code of views[t, s, q], q = 0..127 -- the string's own
    characters below min(len, 128), the stale bytes above; granules >= 1 hold the string's own characters only."""
    n = hb.n
    order = np.asarray(order, np.int64)
    m, nn = hb.lengths()
    planes = np.zeros((planes_entries, 4), np.uint32)
    sides = ((hb.reads, hb.read_off.astype(np.int64), m), (hb.refs, hb.ref_off.astype(np.int64), nn))
    g0 = np.empty((2, 2, n, 4), np.uint32)                       # [side][plane][pair]
    for s in range(2):
        codes = LUT[np.asarray(views)[:, s, :]]
        for p in range(2):
            g0[s, p] = _pack128((codes >> p) & 1)
    for lo, hi, w4, base in bucket_layout(m, nn, order, planes_entries):
        bn, idx = hi - lo, order[lo:hi]
        for s, (text, off, length) in enumerate(sides):
            upper = _upper_granules(text, off, length, idx, w4) if w4 > 1 and bn else None
            for p in range(2):
                at = base + (2 * s + p) * w4 * bn
                planes[at:at + bn] = g0[s, p, idx]
                for g in range(1, w4):
                    planes[at + g * bn:at + (g + 1) * bn] = upper[:, p, g - 1]
    lens = (m | (nn << 16)).astype(np.uint32)[order]
    return planes, lens


def locate_entry(hb, order, planes_entries, entry):
    """(pair, side, plane, granule) of a planes entry."""
    m, nn = hb.lengths()
    for lo, hi, w4, base in bucket_layout(m, nn, np.asarray(order, np.int64), planes_entries):
        bn = hi - lo
        if base <= entry < base + 4 * w4 * bn:
            r = entry - base
            return int(order[lo + r % bn]), r // (2 * w4 * bn), (r // (w4 * bn)) % 2, (r // bn) % w4
    raise IndexError(entry)


def describe_mismatch(hb, order, got, want):
    """First differing (pair, side, plane, dword) in input order and how far it is from the nearest seam."""
    bad = np.nonzero((got != want).any(axis=1))[0]
    where = [locate_entry(hb, order, got.shape[0], int(e)) + (int(e),) for e in bad[:4096]]
    pair, side, plane, gran, e = min(where)
    dword = int(np.nonzero(got[e] != want[e])[0][0])
    seam = nearest_seam(pair, hb.n)
    near = "no seam in the batch" if seam is None else f"{seam[0]} pairs from the {seam[1]} seam at {seam[2]}"
    return (f"{bad.size} of {got.shape[0]} plane entries differ; first: pair {pair} side {side} plane {plane} granule {gran} "
            f"dword {dword} got {int(got[e, dword]):#010x} want {int(want[e, dword]):#010x}; {near}")


# ---- builders -----------------------------------------------------------------------------------------------------------
def _assemble(rng, la, lb, cgt_rows):
    """A batch with the given lengths: ACGT everywhere, CGT only in the pairs cgt_rows."""
    def side(lengths):
        off = np.zeros(len(lengths) + 1, np.int64)
        off[1:] = np.cumsum(lengths)
        text = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(off[-1]))]
        for t in cgt_rows:
            text[off[t]:off[t + 1]] = np.frombuffer(b"CGT", np.uint8)[rng.integers(0, 3, int(lengths[t]))]
        return text, off.astype(np.uint32)
    (ra, ro), (fa, fo) = side(la), side(lb)
    return HostBatch(ra, ro, fa, fo)


def _coast_lengths(rng, n, plants, coast_max):
    la, lb = rng.integers(0, coast_max + 1, n), rng.integers(0, coast_max + 1, n)
    plants = [p for p in plants if p < n]
    la[plants], lb[plants] = rng.integers(128, 301, len(plants)), rng.integers(128, 301, len(plants))
    return la, lb, plants


def plant_and_coast(n, plants, coast_max=2, seed=0):
    """Plants at the indices `plants` (those below n), coasting pairs everywhere else."""
    rng = np.random.default_rng(seed)
    la, lb, plants = _coast_lengths(rng, n, plants, coast_max)
    return _assemble(rng, la, lb, plants)


def eroding(n, plants, seed=0, every=1500):
    """plant_and_coast with rare mid-length pairs: about one pair in `every` has a length from MID_LENGTHS on one side (the
    other side coasts), so what a plant wrote is overwritten piece by piece, at many ages, before the next plant."""
    rng = np.random.default_rng(seed)
    la, lb, plants = _coast_lengths(rng, n, plants, 2)
    mids = np.setdiff1d(np.nonzero(rng.random(n) < 1.0 / every)[0], plants)
    length, on_b = rng.choice(MID_LENGTHS, mids.size), rng.random(mids.size) < 0.5
    la[mids[~on_b]], lb[mids[on_b]] = length[~on_b], length[on_b]
    return _assemble(rng, la, lb, plants)


def one_sided(n, plants, seed=0, empty_side=0):
    """plant_and_coast on one side; every string of the other side is empty."""
    hb = plant_and_coast(n, plants, seed=seed)
    if empty_side == 0:
        return HostBatch(np.zeros(0, np.uint8), np.zeros(n + 1, np.uint32), hb.refs, hb.ref_off)
    return HostBatch(hb.reads, hb.read_off, np.zeros(0, np.uint8), np.zeros(n + 1, np.uint32))


def all_empty(n):
    return HostBatch(np.zeros(0, np.uint8), np.zeros(n + 1, np.uint32), np.zeros(0, np.uint8), np.zeros(n + 1, np.uint32))


def with_empty_pair(hb, t):
    """hb with pair t replaced by a pair of two empty strings."""
    def side(text, off):
        off = off.astype(np.int64)
        cut = off[t + 1] - off[t]
        new = off.copy()
        new[t + 1:] -= cut
        return np.concatenate([text[:off[t]], text[off[t + 1]:]]), new.astype(np.uint32)
    (ra, ro), (fa, fo) = side(hb.reads, hb.read_off), side(hb.refs, hb.ref_off)
    return HostBatch(ra, ro, fa, fo)


# ---- the cases of test_gpu_tail_planes.py, shared with the host test that proves what they exercise ----------------------
PLANTS_A = (0, 38, 39, 40, 41, 79)
PLANTS_B = (0, 5118, 5119, 5120, 5121, 10239)
PLANTS_B_FAR = (0, 39, 5119)          # nothing planted behind 5119: its bytes cross whole workgroups
PLANTS_C = (0, 5119, 81920, 163839, 163840, 163841, 327679)
PLANTS_D = tuple(int(x) for x in np.cumsum([0] + [4099, 7001, 12007, 23003] * 4)[:-2]) + (163839,)  # gaps within and beyond a segment
SIZES_A = (1, 9, 10, 11, 39, 40, 41, 81, 400)
SIZES_B = (5119, 5120, 5121, 10241)
SIZES_B_FAR = (5121, 10241, 15361)
SIZES_C = (163840, 163841, 327681)
N_D = 163841
CUTS_G = (40, 5080, 5121, 153599, 1, 0, 163840)


def case_batch(case, n):
    """The batch of a lettered case; seeds are fixed so that test_tail_cases_host.py's conditions hold."""
    if case == "A":
        return plant_and_coast(n, PLANTS_A, seed=101)
    if case == "B":
        return plant_and_coast(n, PLANTS_B, seed=102)
    if case == "B-far":
        return plant_and_coast(n, PLANTS_B_FAR, seed=112)
    if case == "C":
        return plant_and_coast(n, PLANTS_C, seed=103)
    if case == "D-eroding":
        return eroding(n, PLANTS_D, seed=134)
    if case == "D-reads-empty":
        return one_sided(n, PLANTS_D, seed=105, empty_side=0)
    if case == "D-refs-empty":
        return one_sided(n, PLANTS_D, seed=106, empty_side=1)
    raise KeyError(case)
