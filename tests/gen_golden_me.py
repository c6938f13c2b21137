"""Regenerates tests/golden/me_*.npz: clips the REAL reference encoded with a motion search other than its default -- --FastSearch=0 (the
exhaustive xPatternSearch for uni-prediction), --SearchRange, --BipredSearchRange -- in the layout of gen_golden.run_ldp_case.  Development
container only (see gen_golden.py).

Every clip is also encoded with the defaults (FastSearch 1, SearchRange 64, BipredSearchRange 4): the number of CTUs per picture whose decisions
or motion differ is stored in the fixture (`diff_ctus_vs_off`, one entry per 'S' record) next to the settings themselves (`fast_search`,
`search_range`, `bipred_search_range`).  A clip with a condition (`min_diff` inter pictures that differ) that the reference alone does not
meet is not written: change its seed or lower its range, and record the final options here.

    python tests/gen_golden_me.py [--only NAME]
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402
from gen_golden_fast import _CTU_FIELDS, _slice_records  # noqa: E402

DEFAULTS = (1, 64, 4)
# name, width, height, bit depth, frames, qp, seed, wpp, cfg, (fast_search, search_range, bipred_search_range), inter pictures that must differ
ME_CASES = [
    ("me_full8_ldp_192x128_8b_qp32", 192, 128, 8, 4, 32, 1234, 0, "encoder_lowdelay_P_main.cfg", (0, 8, 4), 2),        # every PU width 4..64 and AMP through full search, 4 references
    ("me_full16_ldpwpp_200x136_8b_qp30", 200, 136, 8, 4, 30, 5, 1, "encoder_lowdelay_P_main.cfg", (0, 16, 4), 2),      # partial CTUs, window clipped at all four picture edges, 33 points per row
    ("me_full8_ra_192x128_10b_qp32", 192, 128, 10, 5, 32, 4321, 0, "encoder_randomaccess_main10.cfg", (0, 8, 2), 2),   # B slices, 10-bit SAD shift, both lists, 25-point bi search
    ("me_full32_ldp_136x72_8b_qp28", 136, 72, 8, 4, 28, 66, 0, "encoder_lowdelay_P_main.cfg", (0, 32, 4), 2),          # 65 points per row: two passes; strips of the large PUs do not fit
    ("me_tz24_ldp_200x136_8b_qp30", 200, 136, 8, 4, 30, 5, 0, "encoder_lowdelay_P_main.cfg", (1, 24, 4), 1),           # TZ, diamonds end at 16, raster over a small window
    # no condition: on a picture this small +-128 need not change a decision.  The clip pins the distance 128 in the queue of search points
    # and the 17 x 17 bi search whose window does not fit for large PUs -- it does not discriminate.
    ("me_tz128_bi8_ldb_136x72_8b_qp30", 136, 72, 8, 4, 30, 66, 0, "encoder_lowdelay_main.cfg", (1, 128, 8), 0),
]


def _options(me):
    return (f"--FastSearch={me[0]}", f"--SearchRange={me[1]}", f"--BipredSearchRange={me[2]}")


def run_me_case(name, w, h, bd, nf, qp, seed, wpp, cfg, me, min_diff):
    gold = gen_golden.GOLD
    with tempfile.TemporaryDirectory() as td:
        gen_golden.GOLD = td
        try:
            gen_golden.run_ldp_case(name, w, h, bd, nf, qp, seed, wpp, cfg, _options(me))
            on_path = os.path.join(td, name + ".npz")
            data = dict(np.load(on_path))
            on = _slice_records(on_path)
            gen_golden.run_ldp_case(name, w, h, bd, nf, qp, seed, wpp, cfg, _options(DEFAULTS))      # the same clip with the default search
            off = _slice_records(on_path)
        finally:
            gen_golden.GOLD = gold
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
    assert n_diff >= min_diff, f"{name}: the search changes {n_diff} inter pictures only ({diff}): change the seed or lower the range"
    data.update(fast_search=np.array(me[0]), search_range=np.array(me[1]), bipred_search_range=np.array(me[2]), diff_ctus_vs_off=np.array(diff, np.int32))
    path = os.path.join(gold, name + ".npz")
    np.savez_compressed(path, **data)
    print(name, "differs from the default search in", diff, "CTUs per picture;", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    for c in ME_CASES:
        if "--only" in sys.argv and c[0] != sys.argv[sys.argv.index("--only") + 1]:
            continue
        run_me_case(*c)
