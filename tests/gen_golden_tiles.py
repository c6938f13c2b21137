"""Regenerates tests/golden/tiles_*.npz: clips the REAL reference encoded with tiles (uniform spacing or explicit column widths / row heights,
WaveFrontSynchro=0, LFCrossTileBoundaryFlag=1), in the layout of gen_golden.run_ldp_case: one 'S' record per picture with the CTUs in raster
order, one 'B' record with rows x cols substreams in tile order.  Development container only (see gen_golden.py).

Every clip is also encoded untiled with otherwise equal options: the number of CTUs per picture whose decisions or motion differ is stored in
the fixture (`diff_ctus_vs_off`, one entry per 'S' record) next to the layout itself (`tile_cols`, `tile_rows`: CTU counts per tile column /
row, and `tile_uniform`).  A clip that misses one of the conditions below is not written: change its QP or seed, never the tile layout or the
number of inter slices, and record the final options here.

    python tests/gen_golden_tiles.py [--only NAME]
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402
from gen_golden_fast import _CTU_FIELDS, _slice_records  # noqa: E402

MAX_BYTES = 700000
# name, width, height, bit depth, frames, qp, seed, cfg, tile options, (tile_cols, tile_rows) in CTUs, uniform spacing
TILE_CASES = [
    # I pictures; partial last CTU column and row; the CABAC chain runs through a 3-row tile
    ("tiles_ai_2x1_520x136_8b_qp27", 520, 136, 8, 2, 27, 11, "encoder_intra_main.cfg",
     ("--TileUniformSpacing=1", "--NumTileColumnsMinus1=1"), ((4, 5), (3,)), 1),
    # a middle tile with a tile edge on both sides; explicit spacing; six substreams; 1-high partial bottom tiles in an I slice
    ("tiles_ai_3x2_776x72_10b_qp32", 776, 72, 10, 1, 32, 12, "encoder_intra_main10.cfg",
     ("--NumTileColumnsMinus1=2", "--TileColumnWidthArray=4,4", "--NumTileRowsMinus1=1", "--TileRowHeightArray=1"), ((4, 4, 5), (1, 1)), 0),
    # P slices, 4 references, merge / AMVP neighbours at tile edges, motion across tile edges
    ("tiles_ldp_2x2_512x128_8b_qp30", 512, 128, 8, 4, 30, 13, "encoder_lowdelay_P_main.cfg",
     ("--TileUniformSpacing=1", "--NumTileColumnsMinus1=1", "--NumTileRowsMinus1=1"), ((4, 4), (1, 1)), 1),
    # B slices; the bottom tile row is 1 CTU high and cut by the picture edge: the first CTU of a bottom tile starts from the m_integerMv2Nx2N
    # of the last CTU of the tile before it.  QP 32 gave 759 kB with 4 pictures: QP 38 brings the file under MAX_BYTES with the same three B slices
    ("tiles_ra_2x2_520x136_10b_qp38", 520, 136, 10, 4, 38, 14, "encoder_randomaccess_main10.cfg",
     ("--NumTileColumnsMinus1=1", "--TileColumnWidthArray=5", "--NumTileRowsMinus1=1", "--TileRowHeightArray=2"), ((5, 4), (2, 1)), 0),
]


def run_tiles_case(name, w, h, bd, nf, qp, seed, cfg, options, layout, uniform):
    gold = gen_golden.GOLD
    with tempfile.TemporaryDirectory() as td:
        gen_golden.GOLD = td
        try:
            gen_golden.run_ldp_case(name, w, h, bd, nf, qp, seed, 0, cfg, tuple(options) + ("--LFCrossTileBoundaryFlag=1",))
            on_path = os.path.join(td, name + ".npz")
            data = dict(np.load(on_path))
            on = _slice_records(on_path)
            gen_golden.run_ldp_case(name, w, h, bd, nf, qp, seed, 0, cfg, ())                  # the same clip without tiles
            off = _slice_records(on_path)
        finally:
            gen_golden.GOLD = gold
    cols, rows = layout
    w_ctu, h_ctu = (w + 63) // 64, (h + 63) // 64
    assert sum(cols) == w_ctu and sum(rows) == h_ctu, f"{name}: the layout does not cover the picture"
    assert [(p, t) for p, t, _ in on] == [(p, t) for p, t, _ in off], f"{name}: the two runs code other pictures"
    n_sub = [len(data[f"r{i}_sub_sizes"]) for i in range(int(data["num_records"])) if chr(int(data[f"r{i}_tag"])) == "B"]
    assert len(n_sub) == len(on) and all(n == len(cols) * len(rows) for n in n_sub), f"{name}: substreams per picture {n_sub}"
    diff = []
    for (_, _, a), (_, _, b) in zip(on, off):
        d = np.zeros(len(a), bool)
        for f in _CTU_FIELDS:
            d |= (a[f] != b[f]).reshape(len(a), -1).any(axis=1)
        diff.append(int(d.sum()))
    assert all(2 * d >= w_ctu * h_ctu for d in diff), f"{name}: fewer than half of the CTUs differ from the untiled run in a picture ({diff})"
    n_inter = sum(1 for _, t, _ in on if t != 2)
    assert n_inter == 0 or n_inter >= 3, f"{name}: {n_inter} inter slices"
    data.update(tile_cols=np.array(cols, np.int32), tile_rows=np.array(rows, np.int32), tile_uniform=np.array(uniform), qp=np.array(qp),
                diff_ctus_vs_off=np.array(diff, np.int32))
    tmp = os.path.join(gold, name + ".tmp.npz")
    np.savez_compressed(tmp, **data)
    size = os.path.getsize(tmp)
    if size >= MAX_BYTES:
        os.remove(tmp)
        raise AssertionError(f"{name}: {size} bytes, the bound is {MAX_BYTES}: raise the QP or change the seed")
    os.replace(tmp, os.path.join(gold, name + ".npz"))
    print(name, "differs from the untiled run in", diff, "CTUs per picture;", n_sub[0], "substreams;", size, "bytes")


if __name__ == "__main__":
    for c in TILE_CASES:
        if "--only" in sys.argv and c[0] != sys.argv[sys.argv.index("--only") + 1]:
            continue
        run_tiles_case(*c)
