"""What the slice tests share: the SliceMode=1 rule of the reference restated in numpy, and a loader for fixtures whose pictures have several
'B' records (one per slice) -- tests/gen_golden_slices.py writes them, tests/test_slices_host.py and tests/test_gpu_slices.py read them."""
import os

import numpy as np

import common

# the WaveFrontSynchro clip of gen_golden_slices.py is not among them: hm355_set_slices refuses WaveFrontSynchro so far
SLICE_CASES = ["slices_ai_328x200_8b_qp30", "slices_ldp_328x136_8b_qp30", "slices_ra_264x136_10b_qp36"]
INTER_CASES = SLICE_CASES[1:]
MAX_BYTES = 700000


def fixed_ctu_slices(w_ctu, h_ctu, wpp, ctus_per_slice):
    """TEncSlice::calculateBoundingCtuTsAddrForSlice (TEncSlice.cpp:1097-1182) for SliceMode=1 without tiles: a slice ends ctus_per_slice CTUs
    after its start or with the picture; under WaveFrontSynchro a slice that starts inside a CTU row ends with that row at the latest.
    -> the raster addresses of the first CTUs"""
    n, first, a = w_ctu * h_ctu, [], 0
    while a < n:
        first.append(a)
        end = min(a + ctus_per_slice, n)
        if wpp and a % w_ctu:
            end = min(end, a - a % w_ctu + w_ctu)
        a = end
    return first


def slice_of(first, n):
    """-> per raster address the index of its slice"""
    return np.searchsorted(np.asarray(first), np.arange(n), side="right") - 1


def load_slices_case(name):
    """-> (cfg, one 'S' record per picture -- the last one the reference wrote, the complete picture --, {poc: 'F'}, {poc: 'A'},
    {poc: ['B' record of every slice, in coding order]}, the fixture's own arrays (slice_first_ctu, slice_arg, diff_first_ctu_vs_off, qp)).
    Also loads a clip of one slice per picture (the unsliced combo_* clips: one 'B' record per picture, no diff_first_ctu_vs_off)"""
    recs, sao = [], {}
    cfg, slices, finals = common.load_ldp_case(name, records=recs, sao=sao)
    bits = {}
    for r in recs:
        if r["tag"] == "B":
            bits.setdefault(r["poc"], []).append(r)
    g = np.load(os.path.join(common.GOLD, name + ".npz"))
    extra = {k: g[k] for k in ("slice_first_ctu", "slice_arg", "diff_first_ctu_vs_off", "qp") if k in g}
    return cfg, slices, finals, sao, bits, extra
