"""Regenerates tests/golden/combo_*.npz: clips the REAL reference encoded with two or more of the features that have a sticky setter of their own --
tiles, slices (--SliceMode=1), the fast encoder decisions (--ESD / --CFM / --ECU), a motion search other than the default (--FastSearch /
--SearchRange / --BipredSearchRange) and the LCU-level rate control -- in the layout of gen_golden.run_ldp_case; the sliced clips keep the last 'S'
record of every picture and every 'B' record, as gen_golden_slices.py does.  Development container only (see gen_golden.py).

The settings of every feature are stored under the keys of the single-feature fixtures, with the defaults for a feature the clip does not use:
`tile_cols`, `tile_rows`, `tile_uniform`; `slice_first_ctu`, `slice_arg` (0: one slice); `esd`, `cfm`, `ecu`; `fast_search`, `search_range`,
`bipred_search_range`; `qp`; and `features`, the names of the features the clip combines.

A feature that does not matter in a clip proves nothing about its combination with the others, so every clip is encoded once more per feature
with ONLY THAT FEATURE off: the number of CTUs per picture whose decisions, motion, costs or coefficients differ is stored as
`diff_ctus_without_<feature>` (one entry per picture, in coding order).  A clip that misses one of these conditions is not written:
  * tiles / slices: at least half of the CTUs of every picture differ;
  * fast decisions, motion search: two inter pictures or more differ;
  * rate control: the QPs the rate model handed the CTUs ('L' records) are not all the slice QP;
  * three inter pictures or more;
  * `combo_tiles_fast_ldp`, `combo_slices_fast_ldb`: the first CTU of a bottom tile / of a later slice that the picture edge cuts -- it starts from
    the m_integerMv2Nx2N of the last CTU of the chain before it -- differs from the run without the fast decisions in one inter picture or more
    (`carry_first_ctus`, `diff_carry_ctus_without_fast`: per picture and such CTU);
  * the file is smaller than MAX_BYTES.
Change the QP or the seed of a clip that misses one, never its layout or its features, and record the final values here.

Tile columns: the reference (TComPicSym::initTiles) and hm355_set_tiles both refuse a tile column narrower than 4 CTUs in Main / Main10, so a
picture with two tile columns and a partial last CTU column is 9 CTUs wide (520 samples) and one with three is 13 CTUs wide (776 samples).

    python tests/gen_golden_combo.py [--only NAME]
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

ME_DEFAULTS = (1, 64, 4)
RC_OPTIONS = ("--RateControl=1", "--TargetBitrate=400000", "--LCULevelRateControl=1", "--InitialQP=30")     # as rc2_ldp_256x128_8b
FEATURES = ("tiles", "slices", "fast", "me", "rc")
# tiles: (reference options, (tile_cols, tile_rows) in CTUs, uniform spacing); slices: SliceArgument; fast: (esd, cfm, ecu);
# me: (fast_search, search_range, bipred_search_range); rc: reference options
COMBO_CLIPS = [
    # P slices, 9 x 3 CTUs; the bottom tiles are one CTU high and cut by the picture edge: their first CTUs (18, 22) take the carried integer MVs
    dict(name="combo_tiles_fast_ldp", w=520, h=136, bd=8, frames=4, qp=34, seed=43, wpp=0, cfg="encoder_lowdelay_P_main.cfg",
         tiles=(("--NumTileColumnsMinus1=1", "--TileColumnWidthArray=4", "--NumTileRowsMinus1=1", "--TileRowHeightArray=2"), ((4, 5), (2, 1)), 0),
         fast=(1, 1, 1)),
    # B slices of both directions, 10 bit; the exhaustive search window (+-16) of a CU at the tile edge reaches into the other tile
    dict(name="combo_tiles_me_ra", w=520, h=136, bd=10, frames=4, qp=38, seed=32, wpp=0, cfg="encoder_randomaccess_main10.cfg",
         tiles=(("--NumTileColumnsMinus1=1", "--TileColumnWidthArray=5"), ((5, 4), (3,)), 0), me=(0, 16, 2)),
    # low-delay B, 13 x 2 CTUs, a middle tile; all three setters at once
    dict(name="combo_tiles_fast_me_ldb", w=776, h=72, bd=8, frames=4, qp=34, seed=33, wpp=0, cfg="encoder_lowdelay_main.cfg",
         tiles=(("--TileUniformSpacing=1", "--NumTileColumnsMinus1=2"), ((4, 4, 5), (2,)), 1), fast=(1, 0, 1), me=(0, 8, 4)),
    # 6 x 3 CTUs, slices start at 0, 7, 14: both later starts inside a CTU row, 14 in the bottom row the picture edge cuts
    dict(name="combo_slices_fast_ldb", w=328, h=136, bd=8, frames=4, qp=32, seed=40, wpp=0, cfg="encoder_lowdelay_main.cfg", slices=7, fast=(1, 1, 1)),
    # 5 x 3 CTUs, slices start at 0, 4, 8, 12; TZ with a small range, 4 references: the one clip that may run as teams of wavefronts
    dict(name="combo_slices_me_ldp", w=264, h=136, bd=8, frames=4, qp=30, seed=35, wpp=0, cfg="encoder_lowdelay_P_main.cfg", slices=4, me=(1, 24, 4)),
    # the only pair that can run under WaveFrontSynchro, which tiles and slices refuse
    dict(name="combo_fast_me_rawpp", w=192, h=136, bd=10, frames=4, qp=32, seed=36, wpp=1, cfg="encoder_randomaccess_main10.cfg", fast=(1, 1, 1), me=(0, 8, 2)),
    # a lambda and a QP per CTU from the rate model with reordered / cut candidate lists and a small TZ range
    dict(name="combo_rc2_fast_me_ldpwpp", w=256, h=136, bd=8, frames=4, qp=32, seed=37, wpp=1, cfg="encoder_lowdelay_P_main.cfg", rc=RC_OPTIONS,
         fast=(1, 1, 1), me=(1, 24, 4)),
]


def _options(clip, without=None):
    """the reference's options for the clip's features, `without` left at its default"""
    o = []
    if clip.get("tiles") and without != "tiles":
        o += list(clip["tiles"][0]) + ["--LFCrossTileBoundaryFlag=1"]
    if clip.get("slices") and without != "slices":
        o += ["--SliceMode=1", f"--SliceArgument={clip['slices']}", "--LFCrossSliceBoundaryFlag=1"]
    fast = clip["fast"] if clip.get("fast") and without != "fast" else (0, 0, 0)
    o += [f"--{k}={v}" for k, v in zip(("ESD", "CFM", "ECU"), fast)]
    me = clip["me"] if clip.get("me") and without != "me" else ME_DEFAULTS
    o += [f"--FastSearch={me[0]}", f"--SearchRange={me[1]}", f"--BipredSearchRange={me[2]}"]
    if clip.get("rc") and without != "rc":
        o += list(clip["rc"])
    return tuple(o)


def _encode(clip, td, without=None):
    gen_golden.run_ldp_case(clip["name"], clip["w"], clip["h"], clip["bd"], clip["frames"], clip["qp"], clip["seed"], clip["wpp"], clip["cfg"],
                            _options(clip, without))
    return dict(np.load(os.path.join(td, clip["name"] + ".npz")))


def _tags(data):
    return [chr(int(data[f"r{i}_tag"])) for i in range(int(data["num_records"]))]


def _pictures(data):
    """-> [(poc, slice_type, ctus)] in coding order, from the last 'S' record of every picture (the reference writes one per slice, each with the
    whole picture's CTU arrays as they stand after that slice)"""
    last, order = {}, []
    for i, t in enumerate(_tags(data)):
        if t == "S":
            poc = int(data[f"r{i}_poc"])
            if poc not in last:
                order.append(poc)
            last[poc] = i
    return [(poc, int(data[f"r{last[poc]}_slice_type"]), data[f"r{last[poc]}_ctus"]) for poc in order]


def _keep_last_s(data, n_slices, name):
    """drops every 'S' record of a picture but the last and renumbers (gen_golden_slices.py); checks one 'S' and one 'B' record per slice"""
    tags = _tags(data)
    s_of, b_of = {}, {}
    for i, t in enumerate(tags):
        if t in "SB":
            (s_of if t == "S" else b_of).setdefault(int(data[f"r{i}_poc"]), []).append(i)
    for poc, idx in s_of.items():
        assert len(idx) == len(b_of.get(poc, [])) == n_slices, f"{name} POC {poc}: {len(idx)} 'S' and {len(b_of.get(poc, []))} 'B' records, {n_slices} slices"
        assert len(set(int(data[f"r{i}_cabac_init_type"]) for i in idx)) == 1, f"{name} POC {poc}: the 'S' records differ in cabac_init_type"
    drop = set(i for idx in s_of.values() for i in idx[:-1])
    keep = [i for i in range(len(tags)) if i not in drop]
    out = {k: v for k, v in data.items() if not (k.startswith("r") and k[1:].split("_")[0].isdigit())}
    for new, old in enumerate(keep):
        for k, v in data.items():
            if k.startswith(f"r{old}_"):
                out[f"r{new}_" + k[len(f"r{old}_"):]] = v
    out["num_records"] = np.array(len(keep))
    return out


def _diff(a, b):
    """per CTU: any of _CTU_FIELDS differs"""
    d = np.zeros(len(a), bool)
    for f in _CTU_FIELDS:
        d |= (a[f] != b[f]).reshape(len(a), -1).any(axis=1)
    return d


def run_combo_case(clip):
    name, w, h = clip["name"], clip["w"], clip["h"]
    w_ctu, h_ctu = (w + 63) // 64, (h + 63) // 64
    n = w_ctu * h_ctu
    features = [f for f in FEATURES if clip.get(f)]
    assert len(features) >= 2 and h % 64, f"{name}: two features or more, a partial CTU row at the bottom"
    assert w % 64 or not (clip.get("tiles") or clip.get("slices")), f"{name}: a clip with a layout has a partial CTU column on the right"
    gold = gen_golden.GOLD
    with tempfile.TemporaryDirectory() as td:
        gen_golden.GOLD = td
        try:
            on = _encode(clip, td)
            off = {f: _pictures(_encode(clip, td, without=f)) for f in features}
        finally:
            gen_golden.GOLD = gold
    pics = _pictures(on)
    assert len(pics) == clip["frames"], f"{name}: {len(pics)} pictures"
    inter = [k for k, (_, t, _) in enumerate(pics) if t != 2]
    assert len(inter) >= 3, f"{name}: {len(inter)} inter pictures"
    # the layout
    cols, rows, uniform = (clip["tiles"][1] + (clip["tiles"][2],)) if clip.get("tiles") else ((w_ctu,), (h_ctu,), 0)
    assert sum(cols) == w_ctu and sum(rows) == h_ctu, f"{name}: the tile layout does not cover the picture"
    first = fixed_ctu_slices(w_ctu, h_ctu, clip["wpp"], clip["slices"]) if clip.get("slices") else [0]
    n_sub = [len(on[f"r{i}_sub_sizes"]) for i, t in enumerate(_tags(on)) if t == "B"]
    if clip.get("tiles"):
        assert len(n_sub) == len(pics) and all(s == len(cols) * len(rows) for s in n_sub), f"{name}: substreams per picture {n_sub}"
    extra = {}
    if clip.get("slices"):
        assert len(first) > 1 and len(n_sub) == len(pics) * len(first), f"{name}: {len(n_sub)} 'B' records"
        on = _keep_last_s(on, len(first), name)
        extra["diff_first_ctu_vs_off"] = np.array([[int(_diff(a, b)[f0]) for f0 in first] for (_, _, a), (_, _, b) in zip(pics, off["slices"])], np.int32)
    # every feature matters
    for f in features:
        assert [(p, t) for p, t, _ in pics] == [(p, t) for p, t, _ in off[f]], f"{name}: the run without {f} codes other pictures"
        d = [int(_diff(a, b).sum()) for (_, _, a), (_, _, b) in zip(pics, off[f])]
        extra[f"diff_ctus_without_{f}"] = np.array(d, np.int32)
        if f in ("tiles", "slices"):
            assert all(2 * v >= n for v in d), f"{name}: fewer than half of the CTUs of a picture differ from the run without {f} ({d})"
        elif f in ("fast", "me"):
            assert sum(d[k] > 0 for k in inter) >= 2, f"{name}: {f} changes fewer than two inter pictures ({d}): choose another QP or seed"
    if clip.get("rc"):
        tags = _tags(on)
        moved = [bool((on[f"r{i}_ctu_qp"] != int(on[f"r{tags.index('S', i)}_qp"])).any()) for i, t in enumerate(tags) if t == "L"]
        assert any(moved), f"{name}: the rate model hands every CTU the slice QP"
    # the witness for the carried integer MVs: first CTUs of chains (not the picture's first) whose 64x64 CU the picture edge cuts
    if name in ("combo_tiles_fast_ldp", "combo_slices_fast_ldb"):
        cb, rb = np.concatenate([[0], np.cumsum(cols)]), np.concatenate([[0], np.cumsum(rows)])
        starts = [int(y * w_ctu + x) for y in rb[:-1] for x in cb[:-1]] if clip.get("tiles") else list(first)
        carry = [a for a in starts if a and ((a % w_ctu) * 64 + 63 >= w or (a // w_ctu) * 64 + 63 >= h)]
        dc = np.array([[int(_diff(a, b)[c]) for c in carry] for (_, _, a), (_, _, b) in zip(pics, off["fast"])], np.int32)
        assert carry and dc[inter].any(), f"{name}: no first CTU of a bottom chain ({carry}) differs from the run without the fast decisions"
        extra.update(carry_first_ctus=np.array(carry, np.int32), diff_carry_ctus_without_fast=dc)
    fast, me = clip.get("fast") or (0, 0, 0), clip.get("me") or ME_DEFAULTS
    on.update(extra)
    on.update(features=np.array(features), tile_cols=np.array(cols, np.int32), tile_rows=np.array(rows, np.int32), tile_uniform=np.array(uniform),
              slice_first_ctu=np.array(first, np.int32), slice_arg=np.array(clip.get("slices") or 0), esd=np.array(fast[0]), cfm=np.array(fast[1]),
              ecu=np.array(fast[2]), fast_search=np.array(me[0]), search_range=np.array(me[1]), bipred_search_range=np.array(me[2]), qp=np.array(clip["qp"]))
    tmp = os.path.join(gold, name + ".tmp.npz")
    np.savez_compressed(tmp, **on)
    size = os.path.getsize(tmp)
    if size >= MAX_BYTES:
        os.remove(tmp)
        raise AssertionError(f"{name}: {size} bytes, the bound is {MAX_BYTES}: raise the QP or change the seed")
    os.replace(tmp, os.path.join(gold, name + ".npz"))
    print(name, {k[len("diff_ctus_without_"):]: v.tolist() for k, v in extra.items() if k.startswith("diff_ctus_without_")},
          ("carried " + str(extra["diff_carry_ctus_without_fast"].tolist())) if "carry_first_ctus" in extra else "", size, "bytes", flush=True)


if __name__ == "__main__":
    for c in COMBO_CLIPS:
        if "--only" in sys.argv and c["name"] != sys.argv[sys.argv.index("--only") + 1]:
            continue
        run_combo_case(c)
