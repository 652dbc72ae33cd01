#!/usr/bin/env python3
"""Generates tests/golden/structured_*.npz and structured_index.json: the compiled reference's answers on the structured corpus
(tests/structured_cases.py: homopolymers, tandem repeats, shifted copies, block gaps, edits on word edges, unrelated pairs), so
that a machine without the reference still carries the pin.  Needs oracle/_ref (built only where the reference tree exists).
Run from the repo root:  python tests/golden/make_golden_structured.py

Per fixture (one all_kinds_batch, inputs pinned by SHA-256): the reference's Greedy cost and CIGAR digest in both buffer-tail
modes, LEAP get_ED(), SIMD_ED's verdict and distance per (threshold, SHD), SHD's verdict per error threshold, affine SIMD_ED at two
settings, and NW for the first 150 pairs from make_golden.py's pure-Python Gotoh.  Fixtures are data only.  The archive is
written with fixed member dates, so that a second run gives the same bytes."""
import io
import json
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import approximate_string_matching_amd as asm  # noqa: E402
from tests import oracle_binding, structured_cases  # noqa: E402
from tests.golden.make_golden import digest, gotoh_py, inputs_sha  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [  # name, (lo, hi), k, (x, o, e), length difference bounded by k (a Greedy batch)
    ("structured_100_128_k3", (100, 128), 3, (1, 1, 1), True),
    ("structured_100_128_k16_x2o3e1", (100, 128), 16, (2, 3, 1), True),
    ("structured_31_128_k10_x4o6e2", (31, 128), 10, (4, 6, 2), False),
    ("structured_129_256_k6", (129, 256), 6, (1, 1, 1), False),
]
SIMD_SETTINGS = [(t, shd) for t in (1, 3, 8, 9, 16, 25) for shd in ((0, 1) if t <= 16 else (0,))]  # (ED threshold, SHD enable)
SHD_ERRORS = [0, 1, 3, 7, 16]
AFFINE_SETTINGS = [(3, 60, 2, 3, 1), (12, 120, 4, 6, 2)]  # (gap threshold, affine threshold, x, o, e), clean
NW_FIRST = 150


def case_batch(lo, hi, k, capped):
    return structured_cases.all_kinds_batch(asm, lo, hi, k, max_diff=k if capped else None)


def save_npz(path, arrays):
    """np.savez_compressed with fixed member dates and order: the same arrays give the same file."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    ref, simd = oracle_binding.load_reference(), oracle_binding.load_reference_simd()
    index = {}
    for name, (lo, hi), k, (x, o, e), capped in CASES:
        hb = case_batch(lo, hi, k, capped)
        out = {}
        for mode, tag in ((0, "seq"), (1, "clean")):
            cost, cig = ref.greedy(hb, k=k, x=x, o=o, e=e, mode=mode, cigars=True)
            out[f"greedy_{tag}_cost"] = cost
            out[f"greedy_{tag}_cigar"] = digest(cig)
        out["leap_ed"] = ref.leap(hb, k=k, x=x, o=o, e=e)
        for t, shd in SIMD_SETTINGS:
            ed, ps = simd.simd_ed(hb, t, bool(shd))
            out[f"pass_t{t}_shd{shd}"] = ps.astype(np.uint8)
            out[f"ed_t{t}_shd{shd}"] = ed.astype(np.int32)
        for me in SHD_ERRORS:
            out[f"shd_e{me}"] = simd.shd(hb, me).astype(np.uint8)
        for g, af, ax, ao, ae in AFFINE_SETTINGS:
            ed, ps = simd.simd_ed_affine(hb, g, af, ax, ao, ae)
            out[f"af_pass_g{g}_a{af}_x{ax}o{ao}e{ae}"] = ps.astype(np.uint8)
            out[f"af_ed_g{g}_a{af}_x{ax}o{ao}e{ae}"] = ed.astype(np.int32)
        out["nw_first"] = np.array([gotoh_py(*hb.pair(i), x, o, e) for i in range(NW_FIRST)], np.int32)
        save_npz(os.path.join(HERE, name + ".npz"), out)
        index[name] = {"lo": lo, "hi": hi, "k": k, "x": x, "o": o, "e": e, "capped": capped, "n": hb.n,
                       "inputs_sha256": inputs_sha(hb), "nw_first": NW_FIRST}
        print(name, "greedy mean", out["greedy_clean_cost"].mean(), "leap mean", out["leap_ed"].mean())
    with open(os.path.join(HERE, "structured_index.json"), "w") as fh:
        json.dump({"cases": index, "simd_settings": SIMD_SETTINGS, "shd_errors": SHD_ERRORS, "affine_settings": AFFINE_SETTINGS,
                   "warm_state": list(oracle_binding.SIMD_WARM_STATE)}, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
