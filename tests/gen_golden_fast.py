"""Regenerates tests/golden/fast_*.npz: clips the REAL reference encoded with its fast encoder decisions --ESD (early skip detection),
--CFM (CBF fast mode) and --ECU (early CU), in the layout of gen_golden.run_ldp_case.  Development container only (see gen_golden.py).

A clip the switches do not change proves nothing, so every clip is also encoded with the switches off: the per-CTU results must differ in at
least two inter pictures, and the number of differing CTUs per picture is stored in the fixture (`diff_ctus_vs_off`, one entry per 'S' record),
next to the switches themselves (`esd`, `cfm`, `ecu`).  The evidence that a switch acts is the first non-zero entry of `diff_ctus_vs_off`: up to
that picture both runs searched identical inputs (same original, same reference pictures), so the switch alone made the difference.  The later
entries also contain the drift of the reference pictures that follows.

    python tests/gen_golden_fast.py [--only NAME]
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402

# name, width, height, bit depth, frames, qp, seed, wpp, cfg, (esd, cfm, ecu), further options
FAST_CASES = [
    ("fast_esd_ldp_192x128_8b_qp32", 192, 128, 8, 5, 32, 1234, 0, "encoder_lowdelay_P_main.cfg", (1, 0, 0), ()),       # reordered 2Nx2N / merge, MVD rule in P
    ("fast_cfm_ldp_200x136_8b_qp30", 200, 136, 8, 5, 30, 5, 0, "encoder_lowdelay_P_main.cfg", (0, 1, 0), ()),          # partial last CTU row and column, AMP gates
    ("fast_ecu_ldpwpp_256x136_8b_qp30", 256, 136, 8, 4, 30, 77, 1, "encoder_lowdelay_P_main.cfg", (0, 0, 1), ()),      # split flag after a cut CU, integer-MV carry across rows
    ("fast_all_ra_192x128_10b_qp32", 192, 128, 10, 9, 32, 4321, 0, "encoder_randomaccess_main10.cfg", (1, 1, 1), ()),  # B slices, both directions
    ("fast_all_ldb_200x136_8b_qp30", 200, 136, 8, 4, 30, 99, 0, "encoder_lowdelay_main.cfg", (1, 1, 1), ()),           # mvd_l1_zero in the ESD sum
    ("fast_all_aq_ldp_256x136_8b_qp32", 256, 136, 8, 4, 32, 53, 1, "encoder_lowdelay_P_main.cfg", (1, 1, 1), ("--AdaptiveQP=1",)),   # delta-QP pricing with reordered candidates
]
_CTU_FIELDS = ("total_cost", "total_bits", "total_dist", "depth", "part_size", "pred_mode", "tr_idx", "cbf", "skip", "merge_flag", "merge_idx", "inter_dir",
               "mv0", "mv1", "ref_idx0", "ref_idx1", "coeff_y", "coeff_cb", "coeff_cr")


def _slice_records(path):
    g = np.load(path)
    out = []
    for i in range(int(g["num_records"])):
        if chr(int(g[f"r{i}_tag"])) == "S":
            out.append((int(g[f"r{i}_poc"]), int(g[f"r{i}_slice_type"]), g[f"r{i}_ctus"]))
    return out


def run_fast_case(name, w, h, bd, nf, qp, seed, wpp, cfg, flags, extra):
    switches = tuple(f"--{k}={v}" for k, v in zip(("ESD", "CFM", "ECU"), flags))
    gen_golden.run_ldp_case(name, w, h, bd, nf, qp, seed, wpp, cfg, tuple(extra) + switches)
    path = os.path.join(gen_golden.GOLD, name + ".npz")
    gold = gen_golden.GOLD
    with tempfile.TemporaryDirectory() as td:                    # the same clip with the switches off, kept out of tests/golden
        gen_golden.GOLD = td
        try:
            gen_golden.run_ldp_case(name, w, h, bd, nf, qp, seed, wpp, cfg, tuple(extra) + ("--ESD=0", "--CFM=0", "--ECU=0"))
        finally:
            gen_golden.GOLD = gold
        off = _slice_records(os.path.join(td, name + ".npz"))
    on = _slice_records(path)
    assert [(p, t) for p, t, _ in on] == [(p, t) for p, t, _ in off], f"{name}: the two runs code other pictures"
    diff = []
    for (_, _, a), (_, _, b) in zip(on, off):
        d = np.zeros(len(a), bool)
        for f in _CTU_FIELDS:
            d |= (a[f] != b[f]).reshape(len(a), -1).any(axis=1)
        diff.append(int(d.sum()))
    n_inter = sum(1 for _, t, _ in on if t != 2)
    n_diff = sum(1 for (_, t, _), d in zip(on, diff) if t != 2 and d > 0)
    assert n_inter >= 3, f"{name}: {n_inter} inter slices"
    assert n_diff >= 2, f"{name}: the switches change the decisions of {n_diff} inter pictures only ({diff}): choose another QP or seed"
    data = dict(np.load(path))
    data.update(esd=np.array(flags[0]), cfm=np.array(flags[1]), ecu=np.array(flags[2]), diff_ctus_vs_off=np.array(diff, np.int32))
    np.savez_compressed(path, **data)
    print(name, "differs from the run without the switches in", diff, "CTUs per picture;", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for c in FAST_CASES:
        if "--only" in sys.argv and c[0] != sys.argv[sys.argv.index("--only") + 1]:
            continue
        run_fast_case(*c)
