"""Regenerates tests/golden/slices_*.npz: clips the REAL reference encoded with --SliceMode=1 --SliceArgument=N (a new slice every N CTUs,
LFCrossSliceBoundaryFlag=1), in the layout of gen_golden.run_ldp_case.  The reference compresses and encodes a picture slice by slice, so its
record stream holds one 'S' and one 'B' record per slice; an 'S' record carries the whole picture's CTU arrays as they stand after its slice.
The fixture keeps the last 'S' record of every picture (the complete picture), every 'B' record, and 'F' and 'A'.  Development container only
(see gen_golden.py).

Every clip is also encoded without slices with otherwise equal options.  Stored next to the records: `slice_first_ctu` (the first CTU of every
slice), `slice_arg`, `qp`, and `diff_first_ctu_vs_off` -- per picture and slice, whether the slice's first CTU differs from the unsliced run.  A
clip that misses one of the conditions below is not written: change its QP or seed, never the slice argument, and record the final options here.

    python tests/gen_golden_slices.py [--only NAME] [--wpp]
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402
from gen_golden_fast import _CTU_FIELDS  # noqa: E402
from slices_common import MAX_BYTES, fixed_ctu_slices  # noqa: E402

# name, width, height, bit depth, frames, qp, seed, cfg, WaveFrontSynchro, SliceArgument
SLICE_CLIPS = [
    # I picture, 6 x 4 CTUs: slices start at 0, 8, 16 -- both later starts lie inside a CTU row
    ("slices_ai_328x200_8b_qp30", 328, 200, 8, 1, 30, 21, "encoder_intra_main.cfg", 0, 8),
    # P pictures, 6 x 3 CTUs: 0, 4, 8, 12, 16; 12 and 16 lie in the bottom CTU row, which the picture edge cuts (m_integerMv2Nx2N is carried)
    ("slices_ldp_328x136_8b_qp30", 328, 136, 8, 4, 30, 22, "encoder_lowdelay_P_main.cfg", 0, 4),
    # B pictures, 5 x 3 CTUs: 0, 7, 14; the last slice is the one corner CTU, partial both ways
    ("slices_ra_264x136_10b_qp36", 264, 136, 10, 4, 36, 24, "encoder_randomaccess_main10.cfg", 0, 7),
]
# WaveFrontSynchro: 0, 9, 12, 21 -- a slice that starts inside a CTU row ends with it.  Not among the committed fixtures while hm355_set_slices
# refuses WaveFrontSynchro; `--wpp` generates it
WPP_CLIP = ("slices_ldpwpp_328x200_8b_qp32", 328, 200, 8, 3, 32, 23, "encoder_lowdelay_P_main.cfg", 1, 9)


def _records(path):
    g = dict(np.load(path))
    return g, [chr(int(g[f"r{i}_tag"])) for i in range(int(g["num_records"]))]


def run_slices_case(name, w, h, bd, nf, qp, seed, cfg, wpp, arg):
    gold = gen_golden.GOLD
    with tempfile.TemporaryDirectory() as td:
        gen_golden.GOLD = td
        try:
            gen_golden.run_ldp_case(name, w, h, bd, nf, qp, seed, wpp, cfg, ("--SliceMode=1", f"--SliceArgument={arg}", "--LFCrossSliceBoundaryFlag=1"))
            on, on_tags = _records(os.path.join(td, name + ".npz"))
            gen_golden.run_ldp_case(name, w, h, bd, nf, qp, seed, wpp, cfg, ())                # the same clip without slices
            off, off_tags = _records(os.path.join(td, name + ".npz"))
        finally:
            gen_golden.GOLD = gold
    w_ctu, h_ctu = (w + 63) // 64, (h + 63) // 64
    n = w_ctu * h_ctu
    first = fixed_ctu_slices(w_ctu, h_ctu, wpp, arg)
    ends = first[1:] + [n]
    assert len(first) > 1, f"{name}: one slice"
    # the 'S' / 'B' records of every picture, in stream order
    s_of, b_of, order = {}, {}, []
    for i, t in enumerate(on_tags):
        if t in "SB":
            poc = int(on[f"r{i}_poc"])
            if t == "S" and poc not in s_of:
                order.append(poc)
            (s_of if t == "S" else b_of).setdefault(poc, []).append(i)
    assert len(order) == nf, f"{name}: {len(order)} pictures"
    for poc in order:
        assert len(s_of[poc]) == len(b_of.get(poc, [])) == len(first), f"{name} POC {poc}: {len(s_of[poc])} 'S' and {len(b_of.get(poc, []))} 'B' records, {len(first)} slices"
        # all compressSlice calls of a picture run before any encodeSlice: every 'S' record of a picture is searched with the same context table
        assert len(set(int(on[f"r{i}_cabac_init_type"]) for i in s_of[poc])) == 1, f"{name} POC {poc}: the 'S' records differ in cabac_init_type"
        if wpp:                                                    # the non-empty substreams of a slice are exactly its CTU rows
            for k, i in enumerate(b_of[poc]):
                rows = set(range(first[k] // w_ctu, (ends[k] - 1) // w_ctu + 1))
                sizes = on[f"r{i}_sub_sizes"]
                assert len(sizes) == h_ctu and set(int(r) for r in np.nonzero(sizes)[0]) == rows, f"{name} POC {poc} slice {k}: substreams {sizes}"
    off_s = {int(off[f"r{i}_poc"]): i for i, t in enumerate(off_tags) if t == "S"}
    assert sorted(off_s) == sorted(order), f"{name}: the two runs code other pictures"
    diff, n_inter = [], 0
    for poc in order:
        i, j = s_of[poc][-1], off_s[poc]
        a, b = on[f"r{i}_ctus"], off[f"r{j}_ctus"]
        st = int(on[f"r{i}_slice_type"])
        assert st == int(off[f"r{j}_slice_type"])
        d = np.zeros(n, bool)
        for f in _CTU_FIELDS:
            d |= (a[f] != b[f]).reshape(n, -1).any(axis=1)
        assert all(d[f0] for f0 in first[1:]), f"{name} POC {poc}: the first CTU of a slice equals the unsliced run ({[int(d[f0]) for f0 in first]})"
        if st == 2:
            assert not d[:first[1]].any(), f"{name} POC {poc}: the first slice of an I picture differs from the unsliced run"
        else:
            n_inter += 1
        diff.append([int(d[f0]) for f0 in first])
    assert n_inter == 0 or n_inter >= 2, f"{name}: {n_inter} inter pictures"
    # keep the last 'S' of every picture, renumber
    drop = set(i for poc in order for i in s_of[poc][:-1])
    keep = [i for i in range(len(on_tags)) if i not in drop]
    data = {k: v for k, v in on.items() if not (k.startswith("r") and k[1:].split("_")[0].isdigit())}
    for new, old in enumerate(keep):
        for k, v in on.items():
            if k.startswith(f"r{old}_"):
                data[f"r{new}_" + k[len(f"r{old}_"):]] = v
    data["num_records"] = np.array(len(keep))
    data.update(slice_first_ctu=np.array(first, np.int32), slice_arg=np.array(arg), qp=np.array(qp), diff_first_ctu_vs_off=np.array(diff, np.int32))
    tmp = os.path.join(gold, name + ".tmp.npz")
    np.savez_compressed(tmp, **data)
    size = os.path.getsize(tmp)
    if size >= MAX_BYTES:
        os.remove(tmp)
        raise AssertionError(f"{name}: {size} bytes, the bound is {MAX_BYTES}: raise the QP or change the seed")
    os.replace(tmp, os.path.join(gold, name + ".npz"))
    print(name, "slices start at", first, "; first CTUs differ from the unsliced run:", diff, ";", size, "bytes")


if __name__ == "__main__":
    for c in SLICE_CLIPS + ([WPP_CLIP] if "--wpp" in sys.argv else []):
        if "--only" in sys.argv and c[0] != sys.argv[sys.argv.index("--only") + 1]:
            continue
        run_slices_case(*c)
